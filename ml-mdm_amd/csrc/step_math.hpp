// The arithmetic of one reverse step on one element, shared by the kernels that must agree on it bit for bit: the step
// kernel of diffusion_ops.hip (mdm_sampler_step) and the noise-map kernel of invert.hip (mdm_sampler_noise_map), which
// solves that step for its noise.  Both call step_row() once per sample and step_mean() once per element, so both
// compile the same expressions.
#pragma once
#include "common.hpp"

namespace mdm {

enum { PT_EPS = 0, PT_V = 2 };   // PredictionType: DDPM (0) and DDIM (1) both predict eps; V_PREDICTION = 2

// x0 from the model output (samplers.py:347-367)
__device__ __forceinline__ float x0_of(float xt, float pred, float sg, float s1g, int ptype) {
  return ptype == PT_V ? xt * sg - pred * s1g : (xt - pred * s1g) / sg;
}

// classifier-free guidance combine p_u + w (p_c - p_u) (samplers.py:445-456)
__device__ __forceinline__ f32x4 guided(f32x4 p, f32x4 pu, float w) { return pu + w * (p - pu); }

// what a sample's gammas give a step from gamma g to gamma gl; beta_t is the variance of the step's noise (the DDPM
// posterior's, times eta^2 under DDIM(eta > 0)): the noise factor is sqrtf(beta_t)
struct StepRow { float g, gl, sg, s1g, sgl, alpha, beta, beta_t; };

__device__ __forceinline__ StepRow step_row(float g, float gl, int mode, float eta) {
  StepRow r;
  r.g = g; r.gl = gl;
  r.sg = sqrtf(g); r.s1g = sqrtf(1.f - g); r.sgl = sqrtf(gl);
  r.alpha = g / gl; r.beta = 1.f - r.alpha;
  r.beta_t = r.beta * (1.f - gl) / (1.f - g);
  if (mode == 1 && eta > 0.f) r.beta_t *= eta * eta;
  return r;
}

// the guided prediction p at x_t -> the thresholded x0 (x0: clip 3 = the unclipped x0 * scale) and, returned, the mean
// of the step: mode 0 = ancestral DDPM posterior mean, 1 = DDIM(eta).  clip: 0 none, 1 CLIP, 2 DYNAMIC (thr)
__device__ __forceinline__ float step_mean(const StepRow& r, float xt, float p, float thr, int ptype, int mode, float eta,
                                           int clip, float scale, float& x0) {
  float v = x0_of(xt, p, r.sg, r.s1g, ptype);
  if (clip == 1) v = fminf(fmaxf(v * scale, -1.f), 1.f) / scale;
  else if (clip == 2) v = fminf(fmaxf(v * scale, -thr), thr) / thr / scale;
  else if (clip == 3) v = v * scale;
  x0 = v;
  float x;
  if (mode == 0) {
    x = v * r.beta * r.sgl / (1.f - r.g) + xt * sqrtf(r.alpha) * (1.f - r.gl) / (1.f - r.g);
  } else {
    const float eps = (xt - v * r.sg) / r.s1g;
    x = v * r.sgl + eps * sqrtf(eta > 0.f ? 1.f - r.gl - r.beta_t : 1.f - r.gl);
  }
  return x;
}

template <typename F>
__device__ __forceinline__ void for_each_vec4(size_t total4, F f) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) f(i);
}

}  // namespace mdm

// the grid of a streaming kernel over n 16-byte groups: one group per thread, at most 4096 blocks of 256
static inline int stream_blocks(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
