// SA-Solver (Xue et al., NeurIPS 2023, "SA-Solver: Stochastic Adams Solver for Fast Sampling of Diffusion Models") on a
// [B, chw] fp32 image: one launch per scale and per step.  Not in the reference.  The definition (include/mdm_hip_ext.h
// repeats it): alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda = log(alpha / sigma); a step from node a to node b,
// h = lambda_b - lambda_a > 0, kappa = 1 + tau^2, m_j the guided, thresholded x0 formed at node j, l_j the Lagrange basis
// over the nodes' offsets s_j = lambda_j - lambda_a:
//   x_b = (sigma_b / sigma_a) e^{-tau^2 h} x_a + alpha_b sum_j c_j m_j + sigma_b sqrt(-expm1(-2 tau^2 h)) z
//   c_j = kappa int_0^h e^{-kappa (h - s)} l_j(s) ds
// Predictor of order p: nodes a, a-1, .., a-p+1.  Corrector of order k: the step a-1 -> a redone with nodes a, .., a-k+1;
// the x_{a-1} term and the noise are the predictor's, so it is a difference, x_a <- x_a - psum_a + alpha_a sum_j c^c_j m_j.
//
// One launch at node a: form m_a from (x_t, pred); correct x_t; predict x_b; store psum_b = alpha_b sum_j c^p_j m_j;
// rotate the history (h1 <- h0, h0 <- m_a).
//
// Coefficients: with u = s / h, x = kappa h and phi_n(x) = x int_0^1 e^{-x (1 - u)} u^n du the c_j are the Lagrange
// coefficients applied to phi_0..2.  phi_n = n! sum_k (-1)^k x^{k+1} / (n + k + 1)! for x < 1 (20 terms, no cancellation),
// phi_0 = -expm1(-x), phi_n = 1 - (n / x) phi_{n-1} from there on.  The differences of lambda come from
// 2 (lambda_b - lambda_a) = log1p((g_b - g_a) / (g_a (1 - g_b))).  All of it in fp64, once per block: a block works on ONE
// sample (blockIdx.x / bps), lane 0 of wave 0 forms the predictor's set, lane 0 of wave 1 the corrector's, and the 256
// threads then stream the sample's slab with fp32 coefficients from LDS.  So a row's bits depend on nothing but the row.
#include "common.hpp"

namespace mdm {

struct SaRngState { unsigned long long seed, offset; };

// four standard normals of counter block `blk`: the draw of diffusion_ops.hip (normal4), statement for statement, so that
// element i of a launch is element i of mdm_randn from the same state
__device__ __forceinline__ void sa_normal4(const SaRngState& st, unsigned long long blk, uint32_t stream, float (&out)[4]) {
  const unsigned long long ctr = st.offset + blk;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), stream, 0u};
  philox4x32_10(c, (uint32_t)st.seed, (uint32_t)(st.seed >> 32));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)c[2 * h] + 1.0f) * 2.3283064365386963e-10f;      // (0, 1]
    const float u2 = (float)c[2 * h + 1] * 2.3283064365386963e-10f;            // [0, 1]
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    out[2 * h] = r * cs; out[2 * h + 1] = r * sn;
  }
}

enum { SA_PT_EPS = 0, SA_PT_V = 2 };

__device__ __forceinline__ float sa_x0_of(float xt, float pred, float sg, float s1g, int ptype) {
  return ptype == SA_PT_V ? xt * sg - pred * s1g : (xt - pred * s1g) / sg;
}

// lambda_b - lambda_a for g_b > g_a, without cancellation
__device__ __forceinline__ double sa_dlambda(double ga, double gb) { return 0.5 * log1p((gb - ga) / (ga * (1.0 - gb))); }

template <int N>
__device__ __forceinline__ double sa_phi_series(double x) {
  double s = 1.0;
#pragma unroll
  for (int k = 19; k >= 1; --k) s = 1.0 - x * s * (1.0 / (double)(N + k + 1));
  return x * s * (1.0 / (double)(N + 1));
}

// phi_0, phi_1, phi_2 at x > 0
__device__ __forceinline__ void sa_phi(double x, double (&phi)[3]) {
  if (x < 1.0) {
    phi[0] = sa_phi_series<0>(x); phi[1] = sa_phi_series<1>(x); phi[2] = sa_phi_series<2>(x);
  } else {
    phi[0] = -expm1(-x);
    phi[1] = 1.0 - phi[0] / x;
    phi[2] = 1.0 - 2.0 * phi[1] / x;
  }
}

struct StepSAArgs {
  const float* x_t; const float* pred; const float* pred_uncond; float guidance;
  const float* gamma; const float* gamma_last; const float* gamma_h0; const float* gamma_h1;
  const float* gate; const float* thr; const float* noise; const SaRngState* rng; uint32_t rng_stream;
  float* h0; float* h1; float* psum; float* x0_out; float* x_last_out;
  size_t chw4; int B, bps; int ptype, clip; float scale; int pmax, cmax;
};

// what the 256 threads of a block read back from LDS
struct SaCoef {
  float cx, cn;       // on x_a and on z
  float cp[3];        // alpha_b c^p_j, j = a, a-1, a-2
  float cc[3];        // alpha_a c^c_j
};

__global__ __launch_bounds__(256) void sampler_step_sa_kernel(StepSAArgs a) {
  __shared__ SaCoef co;
  const int b = (int)(blockIdx.x / (unsigned)a.bps), slab = (int)(blockIdx.x % (unsigned)a.bps);
  const float g = a.gamma[b], gl = a.gamma_last[b];
  // the gate SELECTS: the last step (gamma_last == 1: h = inf) is first order, tau = 0, no corrector, whatever it says
  const bool last = gl >= 1.f;
  const int p = last ? 1 : min(max((int)a.gate[0], 1), a.pmax);
  const int c = last ? 0 : min(max((int)a.gate[1], 0), a.cmax);
  const bool src = a.noise || a.rng;             // without a source of normals there is no stochastic part
  const float tau = (last || !src) ? 0.f : fmaxf(a.gate[2], 0.f);
  const bool noisy = tau > 0.f;
  if (!last) {
    if (threadIdx.x == 0) {   // the predictor's set
      const double gd = g, gld = gl, t2 = (double)tau * (double)tau;
      const double h = sa_dlambda(gd, gld);
      double phi[3];
      sa_phi((1.0 + t2) * h, phi);
      double c0 = phi[0], c1 = 0.0, c2 = 0.0;
      if (p >= 2) {
        const double gh0 = a.gamma_h0[b];
        const double u1 = -sa_dlambda(gh0, gd) / h;
        if (p >= 3) {
          const double u2 = u1 - sa_dlambda((double)a.gamma_h1[b], gh0) / h;
          c1 = (phi[2] - u2 * phi[1]) / (u1 * (u1 - u2));
          c2 = (phi[2] - u1 * phi[1]) / (u2 * (u2 - u1));
        } else {
          c1 = phi[1] / u1;
        }
        c0 = phi[0] - c1 - c2;
      }
      const double ab = sqrt(gld);
      co.cp[0] = (float)(ab * c0); co.cp[1] = (float)(ab * c1); co.cp[2] = (float)(ab * c2);
      co.cx = (float)(sqrt((1.0 - gld) / (1.0 - gd)) * exp(-t2 * h));
      co.cn = noisy ? (float)(sqrt(1.0 - gld) * sqrt(-expm1(-2.0 * t2 * h))) : 0.f;
    }
    if (threadIdx.x == 64 && c >= 1) {   // the corrector's: the step h0's node -> this one, with the tau it was taken at
      const double gd = g, gh0 = a.gamma_h0[b], tc = a.gate[3];
      const double h = sa_dlambda(gh0, gd);
      double phi[3];
      sa_phi((1.0 + tc * tc) * h, phi);
      double ca = phi[0], c0 = 0.0, c2 = 0.0;
      if (c >= 3) {
        const double u2 = -sa_dlambda((double)a.gamma_h1[b], gh0) / h;
        ca = (phi[2] - u2 * phi[1]) / (1.0 - u2);
        c2 = (phi[2] - phi[1]) / (u2 * (u2 - 1.0));
        c0 = phi[0] - ca - c2;
      } else if (c == 2) {
        ca = phi[1];
        c0 = phi[0] - phi[1];
      }
      const double aa = sqrt(gd);
      co.cc[0] = (float)(aa * ca); co.cc[1] = (float)(aa * c0); co.cc[2] = (float)(aa * c2);
    }
    __syncthreads();
  }
  const float cx = last ? 0.f : co.cx, cn = last ? 0.f : co.cn;
  const float cp0 = last ? 0.f : co.cp[0], cp1 = last ? 0.f : co.cp[1], cp2 = last ? 0.f : co.cp[2];
  const float cc0 = c >= 1 ? co.cc[0] : 0.f, cc1 = c >= 1 ? co.cc[1] : 0.f, cc2 = c >= 1 ? co.cc[2] : 0.f;
  const float sg = sqrtf(g), s1g = sqrtf(1.f - g);
  const float thr = a.clip == 2 ? a.thr[b] : 1.f;
  // what of the history this launch reads: h0 where an order asks for it or h1 takes it over, h1 and psum where an order does
  const bool rd0 = !last && a.h0 && (p >= 2 || c >= 2 || a.h1);
  const bool rd1 = p >= 3 || c >= 3;
  SaRngState st = {0ull, 0ull};
  if (noisy && !a.noise) st = *a.rng;
  const size_t base = (size_t)b * a.chw4;
  for (size_t j = (size_t)slab * 256 + threadIdx.x; j < a.chw4; j += (size_t)a.bps * 256) {
    const size_t i = base + j;
    const f32x4 xt = reinterpret_cast<const f32x4*>(a.x_t)[i];
    f32x4 pr = reinterpret_cast<const f32x4*>(a.pred)[i];
    if (a.pred_uncond) {
      const f32x4 pu = reinterpret_cast<const f32x4*>(a.pred_uncond)[i];
      pr = pu + a.guidance * (pr - pu);
    }
    f32x4 m;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = sa_x0_of(xt[e], pr[e], sg, s1g, a.ptype);
      if (a.clip == 1) v = fminf(fmaxf(v * a.scale, -1.f), 1.f) / a.scale;
      else if (a.clip == 2) v = fminf(fmaxf(v * a.scale, -thr), thr) / thr / a.scale;
      m[e] = v;
    }
    if (last) {   // x_b = m_a bit for bit; nothing of the history is read
      reinterpret_cast<f32x4*>(a.x0_out)[i] = m;
      if (a.h0 && a.h0 != a.x0_out) reinterpret_cast<f32x4*>(a.h0)[i] = m;
      reinterpret_cast<f32x4*>(a.x_last_out)[i] = m;
      continue;
    }
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, ps = v0;
    if (rd0) v0 = reinterpret_cast<const f32x4*>(a.h0)[i];
    if (rd1) v1 = reinterpret_cast<const f32x4*>(a.h1)[i];
    if (c >= 1) ps = reinterpret_cast<const f32x4*>(a.psum)[i];
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) {
      if (a.noise) { const f32x4 t = reinterpret_cast<const f32x4*>(a.noise)[i]; nz[0] = t[0]; nz[1] = t[1]; nz[2] = t[2]; nz[3] = t[3]; }
      else sa_normal4(st, i, a.rng_stream, nz);
    }
    f32x4 xl, pn;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xa = xt[e];
      if (c >= 1) {
        float s = cc0 * m[e];
        if (c >= 2) s += cc1 * v0[e];
        if (c >= 3) s += cc2 * v1[e];
        xa = xa - ps[e] + s;
      }
      float s = cp0 * m[e];
      if (p >= 2) s += cp1 * v0[e];
      if (p >= 3) s += cp2 * v1[e];
      pn[e] = s;
      float x = cx * xa + s;
      if (noisy) x += cn * nz[e];
      xl[e] = x;
    }
    reinterpret_cast<f32x4*>(a.x0_out)[i] = m;
    if (a.h0 && a.h0 != a.x0_out) reinterpret_cast<f32x4*>(a.h0)[i] = m;
    if (a.h1 && rd0) reinterpret_cast<f32x4*>(a.h1)[i] = v0;
    if (a.psum) reinterpret_cast<f32x4*>(a.psum)[i] = pn;
    reinterpret_cast<f32x4*>(a.x_last_out)[i] = xl;
  }
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_sampler_step_sa(const float* x_t, const float* pred, const float* pred_uncond, float guidance,
                                   const float* gamma, const float* gamma_last, const float* gamma_h0,
                                   const float* gamma_h1, const float* gate, const float* thr, const float* noise,
                                   const unsigned long long* rng_state, int rng_stream, float* h0, float* h1, float* psum,
                                   float* x0_out, float* x_last_out, int B, size_t chw, int pred_type, int clip,
                                   float image_scale, int max_predictor, int max_corrector, void* stream) {
  MDM_CHECK_ARG(x_t && pred && gamma && gamma_last && gate && x0_out && x_last_out);
  MDM_CHECK_ARG(B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2 && clip >= 0 && clip <= 2);
  MDM_CHECK_ARG(clip != 2 || thr);
  MDM_CHECK_ARG(image_scale > 0.f);
  MDM_CHECK_ARG(max_predictor >= 1 && max_predictor <= 3 && max_corrector >= 0 && max_corrector <= 3);
  MDM_CHECK_ARG(!(max_predictor >= 2 || max_corrector >= 1) || gamma_h0);   // the corrector's step starts at h0's node
  MDM_CHECK_ARG(!(max_predictor >= 2 || max_corrector >= 2) || h0);
  MDM_CHECK_ARG(!(max_predictor >= 3 || max_corrector >= 3) || (h0 && h1 && gamma_h1));
  MDM_CHECK_ARG(max_corrector == 0 || psum);
  // x_last_out aliases nothing; x0_out may be h0; the three state buffers are distinct
  MDM_CHECK_ARG(x_last_out != x0_out && x_last_out != x_t && x_last_out != pred && x_last_out != pred_uncond);
  MDM_CHECK_ARG(x_last_out != h0 && x_last_out != h1 && x_last_out != psum && x_last_out != noise);
  MDM_CHECK_ARG(x0_out != x_t && x0_out != pred && x0_out != pred_uncond && x0_out != noise);
  MDM_CHECK_ARG(!h1 || (h1 != x0_out && h1 != h0 && h1 != x_t && h1 != pred && h1 != pred_uncond && h1 != noise));
  MDM_CHECK_ARG(!psum || (psum != x0_out && psum != h0 && psum != h1 && psum != x_t && psum != pred &&
                          psum != pred_uncond && psum != noise));
  MDM_CHECK_ARG(!h0 || (h0 != x_t && h0 != pred && h0 != pred_uncond && h0 != noise));
  StepSAArgs a;
  a.x_t = x_t; a.pred = pred; a.pred_uncond = pred_uncond; a.guidance = guidance;
  a.gamma = gamma; a.gamma_last = gamma_last; a.gamma_h0 = gamma_h0; a.gamma_h1 = gamma_h1;
  a.gate = gate; a.thr = thr; a.noise = noise; a.rng = reinterpret_cast<const SaRngState*>(rng_state);
  a.rng_stream = (uint32_t)rng_stream;
  a.h0 = h0; a.h1 = h1; a.psum = psum; a.x0_out = x0_out; a.x_last_out = x_last_out;
  a.chw4 = chw / 4; a.B = B; a.ptype = pred_type == 2 ? SA_PT_V : SA_PT_EPS; a.clip = clip; a.scale = image_scale;
  a.pmax = max_predictor; a.cmax = max_corrector;
  // blocks per sample: enough for one vec4 per thread, at most about 4096 blocks in all
  size_t bps = (a.chw4 + 255) / 256;
  const size_t cap = (size_t)B >= 4096 ? 1 : 4096 / (size_t)B;
  if (bps > cap) bps = cap;
  a.bps = (int)bps;
  MDM_CHECK_ARG((size_t)B * bps <= 0x7fffffffull);
  hipLaunchKernelGGL(sampler_step_sa_kernel, dim3((unsigned)((size_t)B * bps)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  MDM_LAUNCH_STATUS();
}
