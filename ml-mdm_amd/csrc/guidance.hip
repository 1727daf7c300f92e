// Projected and rescaled classifier-free guidance, the combine in front of the (unchanged) step kernels:
//   APG       Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion
//             Models", ICLR 2025: the guidance update in x0 space split into the part parallel to the conditional x0
//             (scaled by eta) and the part orthogonal to it, its norm capped, a momentum across steps
//   rescale   Lin, Liu, Li, Yang, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", WACV 2024, section 3.4:
//             the guided prediction pulled back to the per-sample standard deviation of the conditional one
//   interval  Kynkaanniemi et al., "Applying Guidance in a Limited Interval Improves Sample and Distribution Quality in
//             Diffusion Models", NeurIPS 2024: a device gate; off -> the conditional prediction bit for bit
// Per sample, x0 = a x_t + be p (V: a = sqrt(g), be = -sqrt(1 - g); eps: a = 1 / sqrt(g), be = -sqrt(1 - g) / sqrt(g)):
//   D = a x_t + be p_c ;  E = be (p_c - p_u) [+ momentum run_prev] ;  run_out = E
//   s = min(1, thr / (sc sqrt(<E, E> / chw))) ;  c = <E, D> / <D, D>
//   p_g = p_c + k1 E + k2 D ,   k1 = (w - 1) s / be ,  k2 = -(w - 1) s (1 - eta) c / be
//   out = p_g (rescale std(p_c) / std(p_g) + 1 - rescale)
// Two launches (mdm_hip_ext.h).  mdm_cfg_stats reads (x_t, p_c, p_u[, run_prev]) once, writes E to run_out under momentum
// and the per-slab sums of the Gram matrix of (p_c, E, D) -- 3 entries, or all 9 with the three plain sums when the
// rescale is on: p_g is a per-sample linear combination of the three, so its mean and variance follow from them and no
// second pass over the images is needed.  mdm_cfg_combine adds every sample's slab sums in a fixed order in fp64 (each
// block for itself: no third launch), forms k1, k2 and the rescale factor in fp64, and streams (x_t, p_c, and p_u or E).
// The slab geometry is a function of chw alone, so a sample's bits do not depend on the batch it sits in.  No atomics.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

enum { PT_EPS = 0, PT_V = 2 };   // PredictionType as in diffusion_ops.hip: DDPM (0) and DDIM (1) both predict eps
constexpr int CG_THREADS = 256;
constexpr int CG_MAX_SLABS = 512;
constexpr int CG_MIN_SLAB4 = 512;   // 16-byte groups per slab at least: two per thread
constexpr int CG_COLS = 16;         // the combine adds slab s into column s % 16, then the columns 0 .. 15

struct CgGeom {
  size_t slab4;   // 16-byte groups per slab, a multiple of CG_THREADS
  int slabs;
};
// chw4 = chw / 4 groups per sample: 512 slabs where the sample has them (B = 1 at 3 x 1024 x 1024: 512 blocks of 6 groups
// per thread), fewer of at least 512 groups below that
static CgGeom cg_geom(size_t chw4) {
  CgGeom q;
  size_t per = (chw4 + CG_MAX_SLABS - 1) / CG_MAX_SLABS;
  if (per < (size_t)CG_MIN_SLAB4) per = CG_MIN_SLAB4;
  q.slab4 = (per + CG_THREADS - 1) / CG_THREADS * CG_THREADS;
  q.slabs = (int)((chw4 + q.slab4 - 1) / q.slab4);
  return q;
}

// (a, be) of x0 = a x_t + be pred
__device__ __forceinline__ void cg_coefs(float g, int ptype, float& a, float& be) {
  const float sg = sqrtf(g), s1g = sqrtf(1.f - g);
  if (ptype == PT_V) { a = sg; be = -s1g; }
  else { a = 1.f / sg; be = -s1g / sg; }
}
// the guidance update in x0 space: both launches form it with these very operations
__device__ __forceinline__ float cg_delta(float pc, float pu, float be) { return be * (pc - pu); }
__device__ __forceinline__ bool cg_gate(const float* gate) { return gate == nullptr || gate[0] != 0.f; }

// grid (slabs, B).  part[(b * slabs + slab) * NQ + q]; q = 0 <E,E>, 1 <E,D>, 2 <D,D>, and with RESCALE 3 sum p, 4 sum E,
// 5 sum D, 6 <p,p>, 7 <p,E>, 8 <p,D>.  run_out (momentum): E where the guidance gate is on; where it is off the history
// passes through -- run_prev where run_gate is on, 0 where it is off -- and no sum is written (the combine reads none).
template <bool RESCALE>
__global__ __launch_bounds__(CG_THREADS) void cfg_stats_kernel(const float* x_t, const float* pred, const float* pred_uncond,
                                                               const float* __restrict__ gamma, const float* run_prev,
                                                               float* run_out, const float* __restrict__ run_gate,
                                                               const float* __restrict__ w_gate, float momentum,
                                                               float* __restrict__ part, size_t chw4, size_t slab4,
                                                               int ptype) {
  constexpr int NQ = RESCALE ? 9 : 3;
  __shared__ float sh[CG_THREADS / 64][NQ];
  const int b = blockIdx.y, slab = blockIdx.x, slabs = gridDim.x;
  const size_t base = (size_t)b * chw4;
  const size_t i0 = (size_t)slab * slab4, i1 = i0 + slab4 < chw4 ? i0 + slab4 : chw4;
  const bool run_on = run_prev != nullptr && cg_gate(run_gate);
  if (!cg_gate(w_gate)) {
    if (run_out != nullptr && !(run_on && run_out == run_prev)) {
      for (size_t i = i0 + threadIdx.x; i < i1; i += CG_THREADS) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (run_on) r = reinterpret_cast<const f32x4*>(run_prev)[base + i];
        reinterpret_cast<f32x4*>(run_out)[base + i] = r;
      }
    }
    return;
  }
  float a, be;
  cg_coefs(gamma[b], ptype, a, be);
  float acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
#pragma unroll 2
  for (size_t i = i0 + threadIdx.x; i < i1; i += CG_THREADS) {
    const f32x4 x = reinterpret_cast<const f32x4*>(x_t)[base + i], pc = reinterpret_cast<const f32x4*>(pred)[base + i];
    const f32x4 pu = reinterpret_cast<const f32x4*>(pred_uncond)[base + i];
    f32x4 rp = {0.f, 0.f, 0.f, 0.f};
    if (run_on) rp = reinterpret_cast<const f32x4*>(run_prev)[base + i];
    f32x4 ev;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float E = cg_delta(pc[e], pu[e], be);
      if (run_on) E = fmaf(momentum, rp[e], E);
      const float D = fmaf(a, x[e], be * pc[e]);
      ev[e] = E;
      acc[0] = fmaf(E, E, acc[0]);
      acc[1] = fmaf(E, D, acc[1]);
      acc[2] = fmaf(D, D, acc[2]);
      if (RESCALE) {
        acc[3] += pc[e];
        acc[4] += E;
        acc[5] += D;
        acc[6] = fmaf(pc[e], pc[e], acc[6]);
        acc[7] = fmaf(pc[e], E, acc[7]);
        acc[8] = fmaf(pc[e], D, acc[8]);
      }
    }
    if (run_out != nullptr) reinterpret_cast<f32x4*>(run_out)[base + i] = ev;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = wave_sum(acc[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[threadIdx.x >> 6][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x;
    part[((size_t)b * slabs + slab) * NQ + q] = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
  }
}

// grid (slabs, B), the geometry of the statistics.  `run`: E as mdm_cfg_stats stored it (momentum), or nullptr: E is
// formed from pred_uncond again.  Every thread reads its elements before it writes them: out may alias pred.
template <bool RESCALE>
__global__ __launch_bounds__(CG_THREADS) void cfg_combine_kernel(const float* x_t, const float* pred, const float* pred_uncond,
                                                                 const float* __restrict__ gamma, const float* run,
                                                                 const float* __restrict__ w_gate,
                                                                 const float* __restrict__ part, float* out, float w,
                                                                 float eta, float thr, float rescale, float sc, size_t chw4,
                                                                 size_t slab4, int ptype) {
  constexpr int NQ = RESCALE ? 9 : 3;
  __shared__ double red[NQ][CG_COLS];
  __shared__ double tot[NQ];
  __shared__ float coef[3];
  const int b = blockIdx.y, slab = blockIdx.x, slabs = gridDim.x;
  const size_t base = (size_t)b * chw4;
  const size_t i0 = (size_t)slab * slab4, i1 = i0 + slab4 < chw4 ? i0 + slab4 : chw4;
  if (!cg_gate(w_gate)) {
    if (out != pred)
      for (size_t i = i0 + threadIdx.x; i < i1; i += CG_THREADS)
        reinterpret_cast<f32x4*>(out)[base + i] = reinterpret_cast<const f32x4*>(pred)[base + i];
    return;
  }
  float a, be;
  cg_coefs(gamma[b], ptype, a, be);
  if (threadIdx.x < NQ * CG_COLS) {
    const int q = threadIdx.x / CG_COLS, l = threadIdx.x % CG_COLS;
    double t = 0.0;
    for (int s = l; s < slabs; s += CG_COLS) t += (double)part[((size_t)b * slabs + s) * NQ + q];
    red[q][l] = t;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {   // one thread per sum: thread 0 below holds 9 doubles, not 9 x 16
    double t = 0.0;
    for (int l = 0; l < CG_COLS; ++l) t += red[threadIdx.x][l];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* S = tot;
    const double n = 4.0 * (double)chw4;
    const double rms = (double)sc * sqrt(S[0] / n);
    double s = 1.0;
    if (thr > 0.f && rms > 0.0 && (double)thr < rms) s = (double)thr / rms;
    const double c = S[2] > 0.0 ? S[1] / S[2] : 0.0;
    // be == 0 (gamma == 1, where no step starts): no guidance update can be mapped back -- the conditional prediction
    const double g = be != 0.f ? ((double)w - 1.0) * s / (double)be : 0.0;
    const float k1 = (float)g, k2 = (float)(-g * (1.0 - (double)eta) * c);
    float fac = 1.f;
    if (RESCALE) {
      const double d1 = k1, d2 = k2;
      const double mc = S[3] / n, var_c = S[6] / n - mc * mc;
      const double mg = (S[3] + d1 * S[4] + d2 * S[5]) / n;
      const double sq = (S[6] + d1 * d1 * S[0] + d2 * d2 * S[2] + 2.0 * (d1 * S[7] + d2 * S[8] + d1 * d2 * S[1])) / n;
      const double var_g = sq - mg * mg;
      if (var_g > 0.0) fac = (float)((double)rescale * sqrt((var_c > 0.0 ? var_c : 0.0) / var_g) + 1.0 - (double)rescale);
    }
    coef[0] = k1; coef[1] = k2; coef[2] = fac;
  }
  __syncthreads();
  const float k1 = coef[0], k2 = coef[1], fac = coef[2];
#pragma unroll 2
  for (size_t i = i0 + threadIdx.x; i < i1; i += CG_THREADS) {
    const f32x4 x = reinterpret_cast<const f32x4*>(x_t)[base + i], pc = reinterpret_cast<const f32x4*>(pred)[base + i];
    const f32x4 u = reinterpret_cast<const f32x4*>(run != nullptr ? run : pred_uncond)[base + i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float E = run != nullptr ? u[e] : cg_delta(pc[e], u[e], be);
      const float D = fmaf(a, x[e], be * pc[e]);
      o[e] = fac * fmaf(k2, D, fmaf(k1, E, pc[e]));
    }
    reinterpret_cast<f32x4*>(out)[base + i] = o;
  }
}

static inline bool cg_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int cg_check_shape(int B, size_t chw) {
  MDM_CHECK_ARG(B >= 1 && B <= 65535);
  MDM_CHECK_ARG(chw >= 4 && chw % 4 == 0);
  return 0;
}
static inline size_t cg_ws_floats(int B, size_t chw, int rescale_on) {
  return (size_t)B * cg_geom(chw / 4).slabs * (rescale_on ? 9 : 3);
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_cfg_plan(int B, size_t chw, int rescale_on, size_t* ws_bytes) {
  MDM_CHECK_ARG(ws_bytes);
  if (cg_check_shape(B, chw) != 0) return -1;
  *ws_bytes = cg_ws_floats(B, chw, rescale_on) * sizeof(float);
  return 0;
}

extern "C" int mdm_cfg_stats(const float* x_t, const float* pred, const float* pred_uncond, const float* gamma,
                             const float* run_prev, float* run_out, const float* run_gate, const float* w_gate,
                             float momentum, int rescale_on, void* ws, size_t ws_bytes, int B, size_t chw, int pred_type,
                             void* stream) {
  MDM_CHECK_ARG(x_t && pred && pred_uncond && gamma && ws);
  if (cg_check_shape(B, chw) != 0) return -1;
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2);
  MDM_CHECK_ARG(run_out || !run_prev);   // a history is read only to be carried on
  MDM_CHECK_ARG(!run_out || (run_out != x_t && run_out != pred && run_out != pred_uncond));   // run_out may alias run_prev only
  MDM_CHECK_ARG(cg_aligned(x_t) && cg_aligned(pred) && cg_aligned(pred_uncond) && cg_aligned(run_prev) && cg_aligned(run_out));
  MDM_CHECK_ARG(momentum > -1.f && momentum < 1.f);   // NaN fails both
  MDM_CHECK_ARG(ws_bytes >= cg_ws_floats(B, chw, rescale_on) * sizeof(float));
  const CgGeom q = cg_geom(chw / 4);
  const int pt = pred_type == 2 ? PT_V : PT_EPS;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rescale_on)
    hipLaunchKernelGGL(cfg_stats_kernel<true>, dim3(q.slabs, B), dim3(CG_THREADS), 0, st, x_t, pred, pred_uncond, gamma,
                       run_prev, run_out, run_gate, w_gate, momentum, reinterpret_cast<float*>(ws), chw / 4, q.slab4, pt);
  else
    hipLaunchKernelGGL(cfg_stats_kernel<false>, dim3(q.slabs, B), dim3(CG_THREADS), 0, st, x_t, pred, pred_uncond, gamma,
                       run_prev, run_out, run_gate, w_gate, momentum, reinterpret_cast<float*>(ws), chw / 4, q.slab4, pt);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_cfg_combine(const float* x_t, const float* pred, const float* pred_uncond, const float* gamma,
                               const float* run, const float* w_gate, const void* ws, size_t ws_bytes, float* out,
                               float guidance, float eta, float norm_threshold, float rescale, float image_scale, int B,
                               size_t chw, int pred_type, void* stream) {
  MDM_CHECK_ARG(x_t && pred && (pred_uncond || run) && gamma && ws && out);
  if (cg_check_shape(B, chw) != 0) return -1;
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2);
  MDM_CHECK_ARG(out != x_t && out != pred_uncond && out != run);   // out may alias pred only
  MDM_CHECK_ARG(cg_aligned(x_t) && cg_aligned(pred) && cg_aligned(pred_uncond) && cg_aligned(run) && cg_aligned(out));
  MDM_CHECK_ARG(eta >= -3.0e38f && eta <= 3.0e38f && guidance >= -3.0e38f && guidance <= 3.0e38f);   // finite; NaN fails
  MDM_CHECK_ARG(norm_threshold >= 0.f && norm_threshold <= 3.0e38f && rescale >= 0.f && rescale <= 1.f);
  MDM_CHECK_ARG(image_scale > 0.f && image_scale <= 3.0e38f);
  const int rescale_on = rescale > 0.f;
  MDM_CHECK_ARG(ws_bytes >= cg_ws_floats(B, chw, rescale_on) * sizeof(float));
  const CgGeom q = cg_geom(chw / 4);
  const int pt = pred_type == 2 ? PT_V : PT_EPS;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float* part = reinterpret_cast<const float*>(ws);
  if (rescale_on)
    hipLaunchKernelGGL(cfg_combine_kernel<true>, dim3(q.slabs, B), dim3(CG_THREADS), 0, st, x_t, pred, pred_uncond, gamma, run,
                       w_gate, part, out, guidance, eta, norm_threshold, rescale, image_scale, chw / 4, q.slab4, pt);
  else
    hipLaunchKernelGGL(cfg_combine_kernel<false>, dim3(q.slabs, B), dim3(CG_THREADS), 0, st, x_t, pred, pred_uncond, gamma,
                       run, w_gate, part, out, guidance, eta, norm_threshold, rescale, image_scale, chw / 4, q.slab4, pt);
  MDM_LAUNCH_STATUS();
}
