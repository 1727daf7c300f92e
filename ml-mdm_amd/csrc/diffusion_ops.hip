// Per-pixel arithmetic AROUND the denoiser: the sampling update, the train-side noising / loss, the image pyramid,
// the per-sample input normalisation of a nested level and the uint8 input stage.  (SURVEY.md section 8f rows N1,
// N3, N4 and row a7's x / std.)  In the reference each of these is a chain of 5-40 elementwise ATen launches on
// [B, 3, H, W] fp32 images; here each is one streaming kernel (16-byte accesses, fp32 math, NCHW fp32 at the model
// boundary like the reference).
//
// Reference semantics (paths relative to ml-mdm-matryoshka/ml_mdm/):
//   samplers.py:281-345   get_prediction_xt_last: v/eps -> x0, clip, DDPM posterior mean or DDIM(eta) step, noise
//   samplers.py:445-456   classifier-free guidance combine  p = p_u + w (p_c - p_u)
//   samplers.py:461-508   clip_sample: CLIP = clamp(x0 s, -1, 1) / s; DYNAMIC = clamp(x0 s, -q, q) / q / s
//   samplers.py:233-279   get_eps_time / get_xt / get_prediction_targets (+ 347-390 x0 <-> prediction conversions)
//   diffusion.py:144-168, 315-387  get_loss: MSE(pred_target_space, target).mean(C, H, W); F.avg_pool2d pyramid
//   models/unet.py:871-872 x_t / x_t.std((1, 2, 3))   (unbiased), nested level with skip_normalization = false
//   clis/train_parallel.py:194-195  images = (uint8 - 127) / 128, NHWC -> NCHW
#include "common.hpp"
#include "step_math.hpp"

namespace mdm {

// ---------------------------------------------------------------------------------------------------------
// Counter-based RNG: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller.  Element i of a draw takes lane (i & 3) of
// the block with counter (offset + i / 4, stream): a draw is a pure function of (seed, offset, stream, i), so the
// same numbers can be regenerated on the host (oracle/philox_ref.py) -- "device RNG replayable from a CPU seed".
// ---------------------------------------------------------------------------------------------------------
struct RngState { unsigned long long seed, offset; };

// (philox4x32_10 itself: common.hpp -- the GroupNorm re-apply kernel of norm.hip replays the dropout mask with it)
// four standard normals of block `blk` of stream `stream`
__device__ __forceinline__ void normal4(const RngState& st, unsigned long long blk, uint32_t stream, float (&out)[4]) {
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

__global__ void rng_advance_kernel(RngState* st, unsigned long long blocks) { st->offset += blocks; }

// (for_each_vec4, x0_of and the step's own arithmetic -- step_row / step_mean: step_math.hpp, shared with invert.hip)

// ---------------------------------------------------------------------------------------------------------
// N1: one reverse step on a [B, chw] image.  mode 0 = ancestral DDPM posterior mean (ddim_eta is None),
// 1 = DDIM with eta (eta == 0: deterministic, no noise).  clip: 0 none, 1 CLIP, 2 DYNAMIC (thr[b] given), 3 = emit
// the UNCLIPPED x0 * scale into x0_out and stop (first pass of dynamic thresholding: the quantile needs it).
// ---------------------------------------------------------------------------------------------------------
struct StepArgs {
  const float* x_t; const float* pred; const float* pred_uncond; float guidance;
  const float* gamma; const float* gamma_last; const float* noise; const float* noise_gate; const float* thr;
  const RngState* rng; uint32_t rng_stream;
  float* x0_out; float* x_last_out;
  size_t chw4; int B; int ptype, mode; float eta; int need_noise, clip; float scale;
};

__global__ __launch_bounds__(256) void sampler_step_kernel(StepArgs a) {
  const size_t total4 = (size_t)a.B * a.chw4;
  RngState st = {0ull, 0ull};
  const bool gen = a.need_noise && !a.noise && a.rng;
  if (gen) st = *a.rng;
  const float gate = a.noise_gate ? a.noise_gate[0] : 1.f;
  for_each_vec4(total4, [&](size_t i) {
    const int b = (int)(i / a.chw4);
    const StepRow r = step_row(a.gamma[b], a.gamma_last[b], a.mode, a.eta);
    const f32x4 xt = reinterpret_cast<const f32x4*>(a.x_t)[i];
    f32x4 p = reinterpret_cast<const f32x4*>(a.pred)[i];
    if (a.pred_uncond) p = guided(p, reinterpret_cast<const f32x4*>(a.pred_uncond)[i], a.guidance);
    f32x4 x0, xl;
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.need_noise) {
      if (a.noise) { const f32x4 t = reinterpret_cast<const f32x4*>(a.noise)[i]; nz[0] = t[0]; nz[1] = t[1]; nz[2] = t[2]; nz[3] = t[3]; }
      else if (gen) normal4(st, i, a.rng_stream, nz);
    }
    const float thr = a.clip == 2 ? a.thr[b] : 1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v;
      float x = step_mean(r, xt[e], p[e], thr, a.ptype, a.mode, a.eta, a.clip, a.scale, v);
      if (a.need_noise && !(a.mode == 1 && a.eta <= 0.f)) x += sqrtf(r.beta_t) * gate * nz[e];
      x0[e] = v; xl[e] = x;
    }
    reinterpret_cast<f32x4*>(a.x0_out)[i] = x0;
    if (a.clip != 3) reinterpret_cast<f32x4*>(a.x_last_out)[i] = xl;
  });
}

// ---------------------------------------------------------------------------------------------------------
// DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models",
// multistep, data prediction) on a [B, chw] image: same guidance combine, x0 and clip as above, then
//   D = second ? x0 + r (x0 - x0_prev) : x0,   r = h / (2 h_prev)
//   x_s = (sigma_s / sigma_t) x_t + (alpha_s - sigma_s alpha_t / sigma_t) D
// with alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda = log(alpha / sigma).  The differences of lambda are
// taken without cancellation: 2 (lambda_s - lambda_t) = log(g_s (1 - g_t) / (g_t (1 - g_s))) = log1p((g_s - g_t) /
// (g_t (1 - g_s))).  `second` is uniform over the launch (order_gate[0]); when it is off neither a logarithm nor
// x0_prev is touched (the last step has gamma_s = 1: sigma_s = 0, h = inf, x_s = x0).  x0_out may alias x0_prev: a
// thread reads its four elements of x0_prev before it writes them.
// ---------------------------------------------------------------------------------------------------------
struct Step2MArgs {
  const float* x_t; const float* pred; const float* pred_uncond; float guidance;
  const float* gamma; const float* gamma_last; const float* gamma_prev; const float* order_gate; const float* thr;
  const float* x0_prev; float* x0_out; float* x_last_out;
  size_t chw4; int B; int ptype, clip; float scale;
};

__global__ __launch_bounds__(256) void sampler_step_2m_kernel(Step2MArgs a) {
  const size_t total4 = (size_t)a.B * a.chw4;
  const bool second = a.x0_prev && a.gamma_prev && a.order_gate && a.order_gate[0] != 0.f;
  for_each_vec4(total4, [&](size_t i) {
    const int b = (int)(i / a.chw4);
    const float g = a.gamma[b], gl = a.gamma_last[b];
    const float sg = sqrtf(g), s1g = sqrtf(1.f - g);
    const float cx = sqrtf(1.f - gl) / s1g;   // sigma_s / sigma_t
    const float cd = sqrtf(gl) - cx * sg;     // alpha_s - sigma_s alpha_t / sigma_t
    const f32x4 xt = reinterpret_cast<const f32x4*>(a.x_t)[i];
    f32x4 p = reinterpret_cast<const f32x4*>(a.pred)[i];
    if (a.pred_uncond) {
      const f32x4 pu = reinterpret_cast<const f32x4*>(a.pred_uncond)[i];
      p = pu + a.guidance * (p - pu);
    }
    float r = 0.f;
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    if (second) {
      const float gp = a.gamma_prev[b];
      const float h2 = log1pf((gl - g) / (g * (1.f - gl)));    // 2 h
      const float hp2 = log1pf((g - gp) / (gp * (1.f - g)));   // 2 h_prev
      r = 0.5f * h2 / hp2;
      xp = reinterpret_cast<const f32x4*>(a.x0_prev)[i];
    }
    const float thr = a.clip == 2 ? a.thr[b] : 1.f;
    f32x4 x0, xl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = x0_of(xt[e], p[e], sg, s1g, a.ptype);
      if (a.clip == 1) v = fminf(fmaxf(v * a.scale, -1.f), 1.f) / a.scale;
      else if (a.clip == 2) v = fminf(fmaxf(v * a.scale, -thr), thr) / thr / a.scale;
      x0[e] = v;
      const float d = second ? v + r * (v - xp[e]) : v;
      xl[e] = cx * xt[e] + cd * d;
    }
    reinterpret_cast<f32x4*>(a.x0_out)[i] = x0;
    reinterpret_cast<f32x4*>(a.x_last_out)[i] = xl;
  });
}

// ---------------------------------------------------------------------------------------------------------
// Known-region sampling (the replacement method of RePaint, Lugmayr et al. 2022; not in the reference).  After a reverse
// step has produced x at noise level gamma[b], the known pixels are replaced by the known image diffused to that level:
//   k = sqrt(g) known inv_scale + sqrt(1 - g) n,   x = (m == 0) ? x : (m == 1) ? k : m k + (1 - m) x
// on [B, C, H, W] with a [B, 1, H, W] mask.  The mask SELECTS at 0 and 1: a vec4 whose four mask values are 0 is neither
// read nor written, and at m == 1, g == 1 the result is known * inv_scale exactly (1 * v + 0 * n).  hw % 4 == 0, so a
// 16-byte access never straddles a channel plane or a mask row.  The normals of vec4 i are block offset + i whatever the
// mask says (the indexing of noise_images_kernel).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void known_blend_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                          const float* __restrict__ mask, const float* __restrict__ gamma,
                                                          float inv_scale, const float* __restrict__ noise,
                                                          const RngState* __restrict__ rng, uint32_t stream, int B, int C,
                                                          size_t hw4) {
  RngState st = {0ull, 0ull};
  if (!noise) st = *rng;
  const size_t chw4 = (size_t)C * hw4;
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const size_t b = i / chw4;
    const f32x4 m = reinterpret_cast<const f32x4*>(mask)[b * hw4 + (i - b * chw4) % hw4];
    if (m[0] == 0.f && m[1] == 0.f && m[2] == 0.f && m[3] == 0.f) return;
    const float g = gamma[b], sg = sqrtf(g), s1g = sqrtf(1.f - g);
    const f32x4 kn = reinterpret_cast<const f32x4*>(known)[i];
    f32x4 o = reinterpret_cast<const f32x4*>(x)[i];
    float nz[4];
    if (noise) { const f32x4 t = reinterpret_cast<const f32x4*>(noise)[i]; nz[0] = t[0]; nz[1] = t[1]; nz[2] = t[2]; nz[3] = t[3]; }
    else normal4(st, i, stream, nz);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float k = sg * (kn[e] * inv_scale) + s1g * nz[e];
      o[e] = m[e] == 0.f ? o[e] : (m[e] == 1.f ? k : m[e] * k + (1.f - m[e]) * o[e]);
    }
    reinterpret_cast<f32x4*>(x)[i] = o;
  });
}

// ---------------------------------------------------------------------------------------------------------
// The forward transition of a resampling jump (RePaint section 4.2): from level gamma_s back to the noisier gamma_t,
//   a = g_t / g_s,   x_t = sqrt(a) x_s + sqrt(max(1 - a, 0)) n
// on a [B, chw] image.  jump_gate[0] (uniform over the launch; NULL = on) SELECTS: with it off x_t = x_s and no normal is
// drawn.  x_t_out may alias x_s: a thread reads its four elements before it writes them.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jump_kernel(const float* x_s, const float* __restrict__ gamma_t,
                                                   const float* __restrict__ gamma_s, const float* __restrict__ noise,
                                                   const float* __restrict__ jump_gate, const RngState* __restrict__ rng,
                                                   uint32_t stream, float* x_t, int B, size_t chw4) {
  const bool on = !jump_gate || jump_gate[0] != 0.f;
  if (!on && x_t == x_s) return;
  RngState st = {0ull, 0ull};
  if (on && !noise) st = *rng;
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    f32x4 o = reinterpret_cast<const f32x4*>(x_s)[i];
    if (on) {
      const int b = (int)(i / chw4);
      const float a = gamma_t[b] / gamma_s[b];
      const float sa = sqrtf(a), s1a = sqrtf(fmaxf(1.f - a, 0.f));
      float nz[4];
      if (noise) { const f32x4 t = reinterpret_cast<const f32x4*>(noise)[i]; nz[0] = t[0]; nz[1] = t[1]; nz[2] = t[2]; nz[3] = t[3]; }
      else normal4(st, i, stream, nz);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = sa * o[e] + s1a * nz[e];
    }
    reinterpret_cast<f32x4*>(x_t)[i] = o;
  });
}

// ---------------------------------------------------------------------------------------------------------
// N3 (a): x_t = sqrt(g) * images * inv_scale + sqrt(1 - g) * eps; eps given, or drawn here (and stored)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void noise_images_kernel(const float* __restrict__ images, const float* __restrict__ eps_in,
                                                           const float* __restrict__ gamma, float inv_scale,
                                                           float* __restrict__ x_t, float* __restrict__ eps_out,
                                                           const RngState* __restrict__ rng, uint32_t stream, int B,
                                                           size_t chw4) {
  RngState st = {0ull, 0ull};
  if (!eps_in) st = *rng;
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const int b = (int)(i / chw4);
    const float g = gamma[b], sg = sqrtf(g), s1g = sqrtf(1.f - g);
    const f32x4 im = reinterpret_cast<const f32x4*>(images)[i];
    float nz[4];
    if (eps_in) { const f32x4 t = reinterpret_cast<const f32x4*>(eps_in)[i]; nz[0] = t[0]; nz[1] = t[1]; nz[2] = t[2]; nz[3] = t[3]; }
    else normal4(st, i, stream, nz);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = sg * (im[e] * inv_scale) + s1g * nz[e];
    reinterpret_cast<f32x4*>(x_t)[i] = o;
    if (eps_out) reinterpret_cast<f32x4*>(eps_out)[i] = f32x4{nz[0], nz[1], nz[2], nz[3]};
  });
}

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, const RngState* __restrict__ rng, uint32_t stream,
                                                    size_t n4) {
  const RngState st = *rng;
  for_each_vec4(n4, [&](size_t i) {
    float nz[4];
    normal4(st, i, stream, nz);
    reinterpret_cast<f32x4*>(out)[i] = f32x4{nz[0], nz[1], nz[2], nz[3]};
  });
}

// ---------------------------------------------------------------------------------------------------------
// N3 (b): per-sample loss.  p = al * x_t + be * pred (the prediction in the loss-target space), t = ce * eps + ci * img
//   prediction V, target eps:  al = sqrt(1-g), be = sqrt(g)          target eps: ce = 1,       ci = 0
//   prediction eps, target V:  al = -sqrt(1-g)/sqrt(g), be = 1/sqrt(g)   target V:   ce = sqrt(g), ci = -sqrt(1-g)
//   same space:                al = 0, be = 1
// loss[b] = mean_i (p - t)^2 ;  dpred = gloss[b] * (2 / chw) * be * (p - t)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void loss_coefs(float g, int ptype, int ttype, float& al, float& be, float& ce, float& ci) {
  const float sg = sqrtf(g), s1g = sqrtf(1.f - g);
  const bool pv = ptype == PT_V, tv = ttype == PT_V;
  if (pv == tv) { al = 0.f; be = 1.f; }
  else if (pv) { al = s1g; be = sg; }
  else { al = -s1g / sg; be = 1.f / sg; }
  if (tv) { ce = sg; ci = -s1g; } else { ce = 1.f; ci = 0.f; }
}

// grid (slabs, B): part[b][slab] = sum over the slab's elements of (p - t)^2
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ x_t, const float* __restrict__ pred,
                                                           const float* __restrict__ images, const float* __restrict__ eps,
                                                           const float* __restrict__ gamma, float inv_scale,
                                                           float* __restrict__ part, size_t chw4, int ptype, int ttype) {
  __shared__ float sh[4];
  const int b = blockIdx.y;
  float al, be, ce, ci;
  loss_coefs(gamma[b], ptype, ttype, al, be, ce, ci);
  const size_t base = (size_t)b * chw4;
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chw4; i += (size_t)gridDim.x * 256) {
    const f32x4 xt = reinterpret_cast<const f32x4*>(x_t)[base + i], pr = reinterpret_cast<const f32x4*>(pred)[base + i];
    const f32x4 im = reinterpret_cast<const f32x4*>(images)[base + i], ep = reinterpret_cast<const f32x4*>(eps)[base + i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = (al * xt[e] + be * pr[e]) - (ce * ep[e] + ci * im[e] * inv_scale);
      s += d * d;
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void loss_final_kernel(const float* __restrict__ part, float* __restrict__ loss, int B, int slabs, float inv_n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int k = 0; k < slabs; ++k) s += part[(size_t)b * slabs + k];
  loss[b] = s * inv_n;
}
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ x_t, const float* __restrict__ pred,
                                                       const float* __restrict__ images, const float* __restrict__ eps,
                                                       const float* __restrict__ gamma, const float* __restrict__ gloss,
                                                       float inv_scale, float* __restrict__ dpred, int B, size_t chw4,
                                                       int ptype, int ttype, float two_over_n) {
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const int b = (int)(i / chw4);
    float al, be, ce, ci;
    loss_coefs(gamma[b], ptype, ttype, al, be, ce, ci);
    const float k = gloss[b] * two_over_n * be;
    const f32x4 xt = reinterpret_cast<const f32x4*>(x_t)[i], pr = reinterpret_cast<const f32x4*>(pred)[i];
    const f32x4 im = reinterpret_cast<const f32x4*>(images)[i], ep = reinterpret_cast<const f32x4*>(eps)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = k * ((al * xt[e] + be * pr[e]) - (ce * ep[e] + ci * im[e] * inv_scale));
    reinterpret_cast<f32x4*>(dpred)[i] = o;
  });
}

// ---------------------------------------------------------------------------------------------------------
// F.avg_pool2d(x, r) on NCHW fp32 (diffusion.py:346-348); one thread per output pixel
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t planes, int H,
                                                      int W, int r) {
  const int Ho = H / r, Wo = W / r;
  const size_t total = planes * Ho * Wo;
  const float inv = 1.f / (float)(r * r);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ow = (int)(i % Wo);
    const size_t t = i / Wo;
    const int oh = (int)(t % Ho);
    const size_t pl = t / Ho;
    const float* src = x + (pl * H + (size_t)oh * r) * W + (size_t)ow * r;
    float s = 0.f;
    for (int dy = 0; dy < r; ++dy)
      for (int dx = 0; dx < r; ++dx) s += src[(size_t)dy * W + dx];
    y[i] = s * inv;
  }
}

// ---------------------------------------------------------------------------------------------------------
// per-sample std normalisation y = x / std(x) (unbiased, over C*H*W) and its gradient.
//   partial: grid (slabs, N): (sum (x - K), sum (x - K)^2) with K = x[n][0]   [bwd: sum dy * x]
//   apply:   every block re-reduces the slab partials of its sample (<= 64 pairs) and scales its range
// stats [N][2] = (mean, 1 / std) are kept for the backward pass.
//   dx = dy / s - (x - mean) * (sum dy x) / ((n - 1) s^3)
// ---------------------------------------------------------------------------------------------------------
constexpr int STD_SLABS = 64;

__global__ __launch_bounds__(256) void std_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ part, size_t n4) {
  __shared__ float sh[2][4];
  const int n = blockIdx.y;
  const f32x4* xn = reinterpret_cast<const f32x4*>(x) + (size_t)n * n4;
  const f32x4* gn = dy ? reinterpret_cast<const f32x4*>(dy) + (size_t)n * n4 : nullptr;
  const float K = x[(size_t)n * n4 * 4];
  float s1 = 0.f, s2 = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = xn[i];
    if (gn) {
      const f32x4 g = gn[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) s1 += g[e] * v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[e] - K; s1 += d; s2 += d * d; }
    }
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s1; sh[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 2;
    o[0] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    o[1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

__global__ __launch_bounds__(256) void std_apply_kernel(const float* __restrict__ x, const float* __restrict__ part,
                                                        float* __restrict__ y, float* __restrict__ stats, size_t n4,
                                                        int slabs) {
  const int n = blockIdx.y;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < slabs; ++k) { s1 += part[((size_t)n * slabs + k) * 2]; s2 += part[((size_t)n * slabs + k) * 2 + 1]; }
  const float cnt = (float)(n4 * 4);
  const float K = x[(size_t)n * n4 * 4];
  const float dm = s1 / cnt;                                   // mean - K
  const float var = fmaxf((s2 - cnt * dm * dm) / (cnt - 1.f), 0.f);
  const float inv = rsqrtf(var);
  if (blockIdx.x == 0 && threadIdx.x == 0) { stats[2 * n] = K + dm; stats[2 * n + 1] = inv; }
  const f32x4* xn = reinterpret_cast<const f32x4*>(x) + (size_t)n * n4;
  f32x4* yn = reinterpret_cast<f32x4*>(y) + (size_t)n * n4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) yn[i] = xn[i] * inv;
}

__global__ __launch_bounds__(256) void std_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ part, const float* __restrict__ stats,
                                                            float* __restrict__ dx, size_t n4, int slabs) {
  const int n = blockIdx.y;
  float sgx = 0.f;
  for (int k = 0; k < slabs; ++k) sgx += part[((size_t)n * slabs + k) * 2];
  const float cnt = (float)(n4 * 4);
  const float mean = stats[2 * n], inv = stats[2 * n + 1];
  const float c = sgx * inv * inv * inv / (cnt - 1.f);
  const f32x4* xn = reinterpret_cast<const f32x4*>(x) + (size_t)n * n4;
  const f32x4* gn = reinterpret_cast<const f32x4*>(dy) + (size_t)n * n4;
  f32x4* on = reinterpret_cast<f32x4*>(dx) + (size_t)n * n4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = xn[i], g = gn[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = g[e] * inv - (v[e] - mean) * c;
    on[i] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------
// N4: uint8 NHWC [B, H, W, 3] -> fp32 NCHW [B, 3, H, W], (u - 127) / 128   (clis/train_parallel.py:194-195)
// one thread per 4 consecutive pixels of one image row segment: 12 bytes in, three 16-byte stores out
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void input_stage_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int B,
                                                          size_t hw) {
  const size_t hw4 = hw / 4, total = (size_t)B * hw4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw4, q = i - b * hw4;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (b * hw + q * 4) * 3);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
    const uint8_t px[12] = {(uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16), (uint8_t)(w0 >> 24),
                            (uint8_t)w1, (uint8_t)(w1 >> 8), (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24),
                            (uint8_t)w2, (uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 o;
#pragma unroll
      for (int p = 0; p < 4; ++p) o[p] = ((float)px[p * 3 + c] - 127.0f) * 0.0078125f;
      reinterpret_cast<f32x4*>(dst + (b * 3 + c) * hw)[q] = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Loss-guided sampling (diffusion posterior sampling, Chung et al. 2023): the two per-pixel passes around the
// autograd call through the denoiser, on [B, chw] fp32 images.
//   seed:   w = k v m,  k = scale / (clip == 2 ? thr[b] : 1),  m = (clip == 0 || |x0 scale| < 1 - 2^-21) ? 1 : 0
//           direct = a[b] w (the x_t term of the affine x0),  seed = bcoef[b] w (what goes back through the denoiser)
//   apply:  x -= zeta[b] (direct + jt); a sample with zeta[b] == 0 keeps its bits (neither read nor written)
// v is the gradient of the loss in image units; x0 is what the step kernel returned (after its threshold and division by
// scale): where the clamp acted x0 = +-fl(1 / scale), and fl(fl(1 / scale) scale) is 1 or one ulp below it when scale
// is no power of two (0.99999994), so "clipped" is |x0 scale| >= 1 - 2^-21 (four ulps): the threshold is differentiated
// as a clamp.
// ---------------------------------------------------------------------------------------------------------
constexpr float kGuideUnclipped = 1.f - 4.76837158203125e-7f;   // 1 - 2^-21
__global__ __launch_bounds__(256) void guide_seed_kernel(const float* __restrict__ v, const float* __restrict__ x0,
                                                         const float* __restrict__ a, const float* __restrict__ bcoef,
                                                         const float* __restrict__ thr, float scale, int clip,
                                                         float* __restrict__ direct, float* __restrict__ seed, int B,
                                                         size_t chw4) {
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const int b = (int)(i / chw4);
    const float k = clip == 2 ? scale / thr[b] : scale;
    const float ka = a[b] * k, kb = bcoef[b] * k;
    const f32x4 g = reinterpret_cast<const f32x4*>(v)[i];
    f32x4 d, s;
    if (clip) {
      const f32x4 x = reinterpret_cast<const f32x4*>(x0)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float w = fabsf(x[e] * scale) < kGuideUnclipped ? g[e] : 0.f;
        d[e] = ka * w; s[e] = kb * w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) { d[e] = ka * g[e]; s[e] = kb * g[e]; }
    }
    reinterpret_cast<f32x4*>(direct)[i] = d;
    reinterpret_cast<f32x4*>(seed)[i] = s;
  });
}

__global__ __launch_bounds__(256) void guide_apply_kernel(float* __restrict__ x, const float* __restrict__ direct,
                                                          const float* __restrict__ jt, const float* __restrict__ zeta,
                                                          int B, size_t chw4) {
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const float z = zeta[i / chw4];
    if (z == 0.f) return;
    f32x4 g = direct ? reinterpret_cast<const f32x4*>(direct)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    if (jt) g += reinterpret_cast<const f32x4*>(jt)[i];
    f32x4 o = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] -= z * g[e];
    reinterpret_cast<f32x4*>(x)[i] = o;
  });
}

// Perturbed-attention guidance (Ahn et al. 2024), the combine in front of the step kernel:
//   out = (pu ? pu + w (p - pu) : p) + s (p - pp)
// 16-byte loads and stores over the first n / 4 groups, the last n % 4 elements one by one.  Every thread reads its
// elements before it writes them, so out may alias pred.
__device__ __forceinline__ float pag_combine_one(float p, float pu, bool has_u, float pp, float w, float s) {
  const float base = has_u ? pu + w * (p - pu) : p;
  return base + s * (p - pp);
}
__global__ __launch_bounds__(256) void pag_combine_kernel(const float* pred, const float* pred_uncond, const float* pred_pert,
                                                          float w, float s, float* out, size_t n) {
  const size_t n4 = n / 4;
  const bool has_u = pred_uncond != nullptr;
  for_each_vec4(n4, [&](size_t i) {
    const f32x4 p = reinterpret_cast<const f32x4*>(pred)[i];
    const f32x4 pp = reinterpret_cast<const f32x4*>(pred_pert)[i];
    const f32x4 pu = has_u ? reinterpret_cast<const f32x4*>(pred_uncond)[i] : p;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pag_combine_one(p[e], pu[e], has_u, pp[e], w, s);
    reinterpret_cast<f32x4*>(out)[i] = o;
  });
  const size_t tail = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tail < n) out[tail] = pag_combine_one(pred[tail], has_u ? pred_uncond[tail] : 0.f, has_u, pred_pert[tail], w, s);
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_rng_advance(unsigned long long* state, unsigned long long blocks, void* stream) {
  MDM_CHECK_ARG(state);
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<RngState*>(state), blocks);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_randn(float* out, size_t n, const unsigned long long* rng_state, int rng_stream, void* stream) {
  MDM_CHECK_ARG(out && rng_state && n % 4 == 0);
  hipLaunchKernelGGL(randn_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out,
                     reinterpret_cast<const RngState*>(rng_state), (uint32_t)rng_stream, n / 4);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sampler_step(const float* x_t, const float* pred, const float* pred_uncond, float guidance,
                                const float* gamma, const float* gamma_last, const float* noise,
                                const float* noise_gate, const float* thr, const unsigned long long* rng_state,
                                int rng_stream, float* x0_out, float* x_last_out, int B, size_t chw, int pred_type,
                                int mode, float ddim_eta, int need_noise, int clip, float image_scale, void* stream) {
  MDM_CHECK_ARG(x_t && pred && gamma && gamma_last && x0_out);
  MDM_CHECK_ARG(B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2 && (mode == 0 || mode == 1) && clip >= 0 && clip <= 3);
  MDM_CHECK_ARG(clip == 3 || x_last_out);
  MDM_CHECK_ARG(clip != 2 || thr);
  MDM_CHECK_ARG(image_scale > 0.f);
  StepArgs a;
  a.x_t = x_t; a.pred = pred; a.pred_uncond = pred_uncond; a.guidance = guidance;
  a.gamma = gamma; a.gamma_last = gamma_last; a.noise = noise; a.noise_gate = noise_gate; a.thr = thr;
  a.rng = reinterpret_cast<const RngState*>(rng_state); a.rng_stream = (uint32_t)rng_stream;
  a.x0_out = x0_out; a.x_last_out = x_last_out;
  a.chw4 = chw / 4; a.B = B; a.ptype = pred_type == 2 ? PT_V : PT_EPS; a.mode = mode; a.eta = ddim_eta;
  a.need_noise = need_noise; a.clip = clip; a.scale = image_scale;
  MDM_CHECK_ARG(!need_noise || (mode == 1 && ddim_eta <= 0.f) || noise || rng_state);
  hipLaunchKernelGGL(sampler_step_kernel, dim3(stream_blocks((size_t)B * a.chw4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sampler_step_2m(const float* x_t, const float* pred, const float* pred_uncond, float guidance,
                                   const float* gamma, const float* gamma_last, const float* gamma_prev,
                                   const float* order_gate, const float* thr, const float* x0_prev, float* x0_out,
                                   float* x_last_out, int B, size_t chw, int pred_type, int clip, float image_scale,
                                   void* stream) {
  MDM_CHECK_ARG(x_t && pred && gamma && gamma_last && x0_out && x_last_out);
  MDM_CHECK_ARG(B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2 && clip >= 0 && clip <= 2);
  MDM_CHECK_ARG(clip != 2 || thr);
  MDM_CHECK_ARG(image_scale > 0.f);
  MDM_CHECK_ARG(!(order_gate && x0_prev) || gamma_prev);   // second order needs the gamma x0_prev was formed at
  MDM_CHECK_ARG(x_last_out != x0_out && x_last_out != x0_prev);
  Step2MArgs a;
  a.x_t = x_t; a.pred = pred; a.pred_uncond = pred_uncond; a.guidance = guidance;
  a.gamma = gamma; a.gamma_last = gamma_last; a.gamma_prev = gamma_prev; a.order_gate = order_gate; a.thr = thr;
  a.x0_prev = x0_prev; a.x0_out = x0_out; a.x_last_out = x_last_out;
  a.chw4 = chw / 4; a.B = B; a.ptype = pred_type == 2 ? PT_V : PT_EPS; a.clip = clip; a.scale = image_scale;
  hipLaunchKernelGGL(sampler_step_2m_kernel, dim3(stream_blocks((size_t)B * a.chw4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sampler_known_blend(float* x, const float* known, const float* mask, const float* gamma, float inv_scale,
                                       const float* noise, const unsigned long long* rng_state, int rng_stream, int B,
                                       int C, size_t hw, void* stream) {
  MDM_CHECK_ARG(x && known && mask && gamma && B > 0 && C > 0 && hw > 0);
  MDM_CHECK_ARG(hw % 4 == 0);
  MDM_CHECK_ARG(noise || rng_state);
  MDM_CHECK_ARG(x != known && x != noise);
  hipLaunchKernelGGL(known_blend_kernel, dim3(stream_blocks((size_t)B * C * (hw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, known, mask, gamma, inv_scale, noise,
                     reinterpret_cast<const RngState*>(rng_state), (uint32_t)rng_stream, B, C, hw / 4);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sampler_jump(const float* x_s, const float* gamma_t, const float* gamma_s, const float* noise,
                                const float* jump_gate, const unsigned long long* rng_state, int rng_stream,
                                float* x_t_out, int B, size_t chw, void* stream) {
  MDM_CHECK_ARG(x_s && gamma_t && gamma_s && x_t_out && B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(noise || rng_state);
  MDM_CHECK_ARG(x_t_out != noise);
  hipLaunchKernelGGL(jump_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x_s, gamma_t, gamma_s, noise, jump_gate,
                     reinterpret_cast<const RngState*>(rng_state), (uint32_t)rng_stream, x_t_out, B, chw / 4);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_guide_seed(const float* v, const float* x0, const float* a, const float* b, const float* thr,
                              float image_scale, int clip, float* direct, float* seed, int B, size_t chw, void* stream) {
  MDM_CHECK_ARG(v && a && b && direct && seed && B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(clip >= 0 && clip <= 2);
  MDM_CHECK_ARG(clip == 0 || x0);
  MDM_CHECK_ARG(clip != 2 || thr);
  MDM_CHECK_ARG(image_scale > 0.f);
  MDM_CHECK_ARG(direct != seed && direct != v && seed != v && direct != x0 && seed != x0);
  hipLaunchKernelGGL(guide_seed_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), v, x0, a, b, thr, image_scale, clip, direct, seed, B, chw / 4);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_guide_apply(float* x, const float* direct, const float* jt, const float* zeta, int B, size_t chw,
                               void* stream) {
  MDM_CHECK_ARG(x && zeta && (direct || jt) && B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(x != direct && x != jt);
  hipLaunchKernelGGL(guide_apply_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, direct, jt, zeta, B, chw / 4);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_pag_combine(const float* pred, const float* pred_uncond, const float* pred_pert, float guidance,
                               float pag_scale, float* out, size_t n, void* stream) {
  MDM_CHECK_ARG(pred && pred_pert && out && n > 0);
  MDM_CHECK_ARG(out != pred_uncond && out != pred_pert);   // out may alias pred only
  hipLaunchKernelGGL(pag_combine_kernel, dim3(stream_blocks((n + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), pred, pred_uncond, pred_pert, guidance, pag_scale, out, n);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_noise_images(const float* images, const float* eps, const float* gamma, float inv_scale, float* x_t,
                                float* eps_out, const unsigned long long* rng_state, int rng_stream, int B, size_t chw,
                                void* stream) {
  MDM_CHECK_ARG(images && gamma && x_t && B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(eps || (rng_state && eps_out));
  hipLaunchKernelGGL(noise_images_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), images, eps, gamma, inv_scale, x_t, eps_out,
                     reinterpret_cast<const RngState*>(rng_state), (uint32_t)rng_stream, B, chw / 4);
  MDM_LAUNCH_STATUS();
}

static inline int loss_slabs(int B, size_t chw4) {
  int s = (512 + B - 1) / B;
  const size_t max_s = (chw4 + 1023) / 1024;
  if ((size_t)s > max_s) s = (int)max_s;
  return s < 1 ? 1 : (s > 256 ? 256 : s);
}

extern "C" int mdm_diffusion_loss_plan(int B, size_t chw, size_t* ws_bytes) {
  MDM_CHECK_ARG(ws_bytes && B > 0 && chw % 4 == 0);
  *ws_bytes = (size_t)B * loss_slabs(B, chw / 4) * sizeof(float);
  return 0;
}

extern "C" int mdm_diffusion_loss_fwd(const float* x_t, const float* pred, const float* images, const float* eps,
                                      const float* gamma, float inv_scale, float* loss, float* ws, int B, size_t chw,
                                      int pred_type, int target_type, void* stream) {
  MDM_CHECK_ARG(x_t && pred && images && eps && gamma && loss && ws && B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2 && target_type >= 0 && target_type <= 2);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int slabs = loss_slabs(B, chw / 4);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(slabs, B), dim3(256), 0, st, x_t, pred, images, eps, gamma, inv_scale, ws,
                     chw / 4, pred_type == 2 ? PT_V : PT_EPS, target_type == 2 ? PT_V : PT_EPS);
  hipLaunchKernelGGL(loss_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, ws, loss, B, slabs, 1.0f / (float)chw);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_diffusion_loss_bwd(const float* x_t, const float* pred, const float* images, const float* eps,
                                      const float* gamma, const float* gloss, float inv_scale, float* dpred, int B,
                                      size_t chw, int pred_type, int target_type, void* stream) {
  MDM_CHECK_ARG(x_t && pred && images && eps && gamma && gloss && dpred && B > 0 && chw > 0 && chw % 4 == 0);
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x_t, pred, images, eps, gamma, gloss, inv_scale, dpred, B,
                     chw / 4, pred_type == 2 ? PT_V : PT_EPS, target_type == 2 ? PT_V : PT_EPS, 2.0f / (float)chw);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_avgpool(const float* x, float* y, int N, int C, int H, int W, int r, void* stream) {
  MDM_CHECK_ARG(x && y && N > 0 && C > 0 && r >= 1 && H % r == 0 && W % r == 0);
  const size_t total = (size_t)N * C * (H / r) * (W / r);
  hipLaunchKernelGGL(avgpool_kernel, dim3(stream_blocks(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y,
                     (size_t)N * C, H, W, r);
  MDM_LAUNCH_STATUS();
}

static inline int std_slabs(int N, size_t n4) {
  int s = (512 + N - 1) / N;
  const size_t max_s = (n4 + 1023) / 1024;
  if ((size_t)s > max_s) s = (int)max_s;
  return s < 1 ? 1 : (s > STD_SLABS ? STD_SLABS : s);
}

/* ws: fp32 [N][64][2] */
extern "C" int mdm_sample_std_fwd(const float* x, float* y, float* stats, float* ws, int N, size_t chw, void* stream) {
  MDM_CHECK_ARG(x && y && stats && ws && N > 0 && chw >= 8 && chw % 4 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int slabs = std_slabs(N, chw / 4);
  hipLaunchKernelGGL(std_partial_kernel, dim3(slabs, N), dim3(256), 0, st, x, (const float*)nullptr, ws, chw / 4);
  hipLaunchKernelGGL(std_apply_kernel, dim3(slabs, N), dim3(256), 0, st, x, ws, y, stats, chw / 4, slabs);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sample_std_bwd(const float* dy, const float* x, const float* stats, float* dx, float* ws, int N,
                                  size_t chw, void* stream) {
  MDM_CHECK_ARG(dy && x && stats && dx && ws && N > 0 && chw >= 8 && chw % 4 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int slabs = std_slabs(N, chw / 4);
  hipLaunchKernelGGL(std_partial_kernel, dim3(slabs, N), dim3(256), 0, st, x, dy, ws, chw / 4);
  hipLaunchKernelGGL(std_bwd_apply_kernel, dim3(slabs, N), dim3(256), 0, st, dy, x, ws, stats, dx, chw / 4, slabs);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_input_stage(const void* u8_nhwc, float* out_nchw, int B, int H, int W, void* stream) {
  MDM_CHECK_ARG(u8_nhwc && out_nchw && B > 0 && H > 0 && W > 0);
  const size_t hw = (size_t)H * W;
  MDM_CHECK_ARG(hw % 4 == 0 && ((size_t)u8_nhwc & 3) == 0);
  hipLaunchKernelGGL(input_stage_kernel, dim3(stream_blocks((size_t)B * hw / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint8_t*>(u8_nhwc), out_nchw, B, hw);
  MDM_LAUNCH_STATUS();
}


// ---------------------------------------------------------------------------------------------------------
// Dropout (reference models/unet.py:208,234: nn.Dropout between norm2 + SiLU and conv2 of a ResNet block).
// y[i] = keep(i) ? x[i] / (1 - p) : 0 with keep(i) = (Philox word of element i) >= p * 2^32: a pure function of
// (seed, offset, i), so backward regenerates the same mask from the two integers instead of storing it.  The same
// launch serves both directions (dx = dy masked and scaled the same way).  8 elements per thread = two Philox blocks.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, size_t n8, unsigned thresh,
                                                      float scale, unsigned long long seed, unsigned long long offset) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    float v[8];
    if constexpr (sizeof(T) == 2) {
      Chunk<T> c;
      c.load(x + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = c.v[e];
    } else {
      Chunk<T> c0, c1;
      c0.load(x + i * 8); c1.load(x + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = c0.v[e]; v[4 + e] = c1.v[e]; }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t c[4];
      dropout_words(c, seed, offset + 2 * i + h);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * h + e] = c[e] >= thresh ? v[4 * h + e] * scale : 0.f;
    }
    if constexpr (sizeof(T) == 2) {
      Chunk<T> c;
#pragma unroll
      for (int e = 0; e < 8; ++e) c.v[e] = v[e];
      c.store(y + i * 8);
    } else {
      Chunk<T> c0, c1;
#pragma unroll
      for (int e = 0; e < 4; ++e) { c0.v[e] = v[e]; c1.v[e] = v[4 + e]; }
      c0.store(y + i * 8); c1.store(y + i * 8 + 4);
    }
  }
}

extern "C" int mdm_dropout(const void* x, void* y, size_t n, float p, unsigned long long seed, unsigned long long offset,
                           int dtype, void* stream) {
  MDM_CHECK_ARG(x && y && n % 8 == 0 && p >= 0.f && p < 1.f);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  if (n == 0) return 0;
  const size_t n8 = n / 8;
  unsigned thresh;
  float scale;
  dropout_params(p, &thresh, &scale);
  const unsigned blocks = (unsigned)((n8 + 255) / 256 > 8192 ? 8192 : (n8 + 255) / 256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == DT_F32) hipLaunchKernelGGL(dropout_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)x, (float*)y, n8, thresh, scale, seed, offset);
  else hipLaunchKernelGGL(dropout_kernel<bf16>, dim3(blocks), dim3(256), 0, st, (const bf16*)x, (bf16*)y, n8, thresh, scale, seed, offset);
  MDM_LAUNCH_STATUS();
}
