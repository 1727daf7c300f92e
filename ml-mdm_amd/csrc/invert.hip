// Image inversion around the denoiser, on fp32 [B, chw] images (not in the reference): the two per-pixel passes that take a
// GIVEN image back to the noise that reproduces it.  include/mdm_hip_ext.h has the definitions.
//
//   mdm_sampler_invert_step   the preimage of one DDIM(0) step with the prediction held fixed: the body of the fixed-point
//                             iteration of DDIM inversion (Song et al. 2021; Pan et al. 2023; Garibi et al. 2024)
//   mdm_sampler_noise_map     the noise z that makes the ancestral step x_t -> x_s land on a given x_s (edit-friendly DDPM
//                             inversion, Huberman-Spiegelglas et al. 2024): z = (x_s - mu) / sigma with mu and sigma those of
//                             mdm_sampler_step -- the same __device__ functions (step_math.hpp), so the same arithmetic
//
// Streaming kernels: 16-byte accesses, one vec4 per thread and grid stride, per-sample gammas read per vec4 (a broadcast
// load, L1-resident), no atomics, no workspace.  Bytes per element: 12 (x, p, out) to 16 (+ p_u) for the first, 16 to 20
// for the second.
#include "common.hpp"
#include "step_math.hpp"

namespace mdm {

// alpha = sqrt(gamma), sigma = sqrt(1 - gamma); s the cleaner node (g_s > g_t).
//   eps:  x_t = (alpha_t / alpha_s) x_s + c p,     c = sigma_t - alpha_t sigma_s / alpha_s
//   v:    x_t = (x_s - d p) / (alpha_s alpha_t + sigma_s sigma_t),     d = sigma_s alpha_t - alpha_s sigma_t
// c and d are differences of nearly equal products between neighbouring nodes; from (sigma_t alpha_s)^2 - (alpha_t sigma_s)^2
// = g_s - g_t they are quotients without cancellation (the way the 2M kernel takes its lambda differences).
__global__ __launch_bounds__(256) void sampler_invert_step_kernel(const float* __restrict__ x_s, const float* __restrict__ pred,
                                                                  const float* __restrict__ pred_uncond, float guidance,
                                                                  const float* __restrict__ gamma_s,
                                                                  const float* __restrict__ gamma_t, float* __restrict__ x_t,
                                                                  int B, size_t chw4, int ptype) {
  for_each_vec4((size_t)B * chw4, [&](size_t i) {
    const int b = (int)(i / chw4);
    const float gs = gamma_s[b], gt = gamma_t[b];
    const float as = sqrtf(gs), ss = sqrtf(1.f - gs), at = sqrtf(gt), st = sqrtf(1.f - gt);
    const float cross = st * as + at * ss;   // > 0 wherever g_t < 1
    float cx, cp;
    if (ptype == PT_V) {
      const float inv = 1.f / (as * at + ss * st);
      cx = inv;
      cp = (gs - gt) / cross * inv;          // -d / (alpha_s alpha_t + sigma_s sigma_t)
    } else {
      cx = at / as;
      cp = (gs - gt) / (cross * as);
    }
    const f32x4 xs = reinterpret_cast<const f32x4*>(x_s)[i];
    f32x4 p = reinterpret_cast<const f32x4*>(pred)[i];
    if (pred_uncond) p = guided(p, reinterpret_cast<const f32x4*>(pred_uncond)[i], guidance);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = cx * xs[e] + cp * p[e];
    reinterpret_cast<f32x4*>(x_t)[i] = o;
  });
}

struct NoiseMapArgs {
  const float* x_t; const float* x_s; const float* pred; const float* pred_uncond; float guidance;
  const float* gamma; const float* gamma_last; const float* thr; float* z_out;
  size_t chw4; int B; int ptype, mode; float eta; int clip; float scale;
};

__global__ __launch_bounds__(256) void sampler_noise_map_kernel(NoiseMapArgs a) {
  for_each_vec4((size_t)a.B * a.chw4, [&](size_t i) {
    const int b = (int)(i / a.chw4);
    const StepRow r = step_row(a.gamma[b], a.gamma_last[b], a.mode, a.eta);
    const float sigma = sqrtf(r.beta_t);   // the step kernel's noise factor
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (sigma > 0.f) {   // sigma == 0 (gamma_last == 1: the last step adds no noise): z = 0, nothing else is read
      const f32x4 xt = reinterpret_cast<const f32x4*>(a.x_t)[i];
      const f32x4 xs = reinterpret_cast<const f32x4*>(a.x_s)[i];
      f32x4 p = reinterpret_cast<const f32x4*>(a.pred)[i];
      if (a.pred_uncond) p = guided(p, reinterpret_cast<const f32x4*>(a.pred_uncond)[i], a.guidance);
      const float thr = a.clip == 2 ? a.thr[b] : 1.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x0;
        const float mu = step_mean(r, xt[e], p[e], thr, a.ptype, a.mode, a.eta, a.clip, a.scale, x0);
        z[e] = (xs[e] - mu) / sigma;
      }
    }
    reinterpret_cast<f32x4*>(a.z_out)[i] = z;
  });
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_sampler_invert_step(const float* x_s, const float* pred, const float* pred_uncond, float guidance,
                                       const float* gamma_s, const float* gamma_t, float* x_t_out, int B, size_t chw,
                                       int pred_type, void* stream) {
  MDM_CHECK_ARG(x_s && pred && gamma_s && gamma_t && x_t_out);
  MDM_CHECK_ARG(B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2);
  MDM_CHECK_ARG(x_t_out != x_s && x_t_out != pred && x_t_out != pred_uncond);   // (__restrict__ above)
  hipLaunchKernelGGL(sampler_invert_step_kernel, dim3(stream_blocks((size_t)B * (chw / 4))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x_s, pred, pred_uncond, guidance, gamma_s, gamma_t, x_t_out, B,
                     chw / 4, pred_type == 2 ? PT_V : PT_EPS);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_sampler_noise_map(const float* x_t, const float* x_s, const float* pred, const float* pred_uncond,
                                     float guidance, const float* gamma, const float* gamma_last, const float* thr,
                                     float* z_out, int B, size_t chw, int pred_type, int mode, float ddim_eta, int clip,
                                     float image_scale, void* stream) {
  MDM_CHECK_ARG(x_t && x_s && pred && gamma && gamma_last && z_out);
  MDM_CHECK_ARG(B > 0 && chw > 0 && chw % 4 == 0);
  MDM_CHECK_ARG(pred_type >= 0 && pred_type <= 2 && (mode == 0 || mode == 1) && clip >= 0 && clip <= 2);
  MDM_CHECK_ARG(mode == 0 || ddim_eta > 0.f);   // DDIM(0) adds no noise: there is no map to solve for
  MDM_CHECK_ARG(clip != 2 || thr);
  MDM_CHECK_ARG(image_scale > 0.f);
  MDM_CHECK_ARG(z_out != x_t && z_out != x_s && z_out != pred && z_out != pred_uncond);
  NoiseMapArgs a;
  a.x_t = x_t; a.x_s = x_s; a.pred = pred; a.pred_uncond = pred_uncond; a.guidance = guidance;
  a.gamma = gamma; a.gamma_last = gamma_last; a.thr = thr; a.z_out = z_out;
  a.chw4 = chw / 4; a.B = B; a.ptype = pred_type == 2 ? PT_V : PT_EPS; a.mode = mode; a.eta = ddim_eta; a.clip = clip;
  a.scale = image_scale;
  hipLaunchKernelGGL(sampler_noise_map_kernel, dim3(stream_blocks((size_t)B * a.chw4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  MDM_LAUNCH_STATUS();
}
