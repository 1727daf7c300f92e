// Inference-only T5 v1.1 / flan encoder (language_models/factory.py:14-38, 84-101: T5Encoder.forward =
// T5ForConditionalGeneration.encoder, eval mode) over PACKED tokens: the T valid tokens of a [B, S] batch, row after
// row, each with its original position.  Everything between the seven projections (the existing GEMM) lives here:
//   t5_rms_kernel      embedding gather + first RMSNorm | residual add + RMSNorm | final RMSNorm + scatter to [B, S, D]
//   t5_gated_gelu_kernel   gelu_new(u[:, :F]) * u[:, F:]
//   t5_attn_kernel     softmax(q k^T + bias[h, pos_k - pos_q]) v per (sequence, head), no 1/sqrt(d); the input
//                      gradients are in text_encoder_bwd.hip
// The residual stream is fp32 (the reference's autocast leaves the residual adds in fp32); T is the storage type of the
// GEMM operands.  Norm statistics, scores and the softmax are fp32.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

enum { RMS_EMBED = 0, RMS_ADD = 1, RMS_FINAL = 2 };

__device__ __forceinline__ void store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store4(bf16* p, const f32x4& v) {
  bf16x4 t = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<bf16x4*>(p) = t;
}
__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const bf16* p) {
  const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
}

// One row per wave, four rows per block; a lane walks the row in 16-byte fp32 chunks (D % 4 == 0).  Two passes over the
// row: the first forms x (+ delta), stores it back to the fp32 stream and accumulates sum x^2; the second re-reads the
// 8 KB row (L1 / L2) and writes w * x * rsqrt(mean + eps).
//   RMS_EMBED  x[r] = table[clamp(ids[r])];                  h[r] = rms(x[r])              rows = T
//   RMS_ADD    x[r] += delta[r] (delta may be null);         h[r] = rms(x[r])              rows = T
//   RMS_FINAL  s = src[r]; out[r] = s < 0 ? 0 : rms(x[s] + delta[s])   (fp32, x not written)   rows = B * S
template <typename T, int MODE>
__global__ __launch_bounds__(256) void t5_rms_kernel(const int* __restrict__ idx, const float* __restrict__ table,
                                                     float* __restrict__ x, const T* __restrict__ delta,
                                                     const float* __restrict__ w, T* __restrict__ h,
                                                     float* __restrict__ out, int rows, int D, int vocab, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nc = D >> 2;
  if constexpr (MODE == RMS_FINAL) {
    const int s = idx[r];
    float* o = out + (size_t)r * D;
    if (s < 0) {
      for (int c = lane; c < nc; c += 64) store4(o + 4 * c, f32x4{0.f, 0.f, 0.f, 0.f});
      return;
    }
    const float* xr = x + (size_t)s * D;
    const T* dr = delta ? delta + (size_t)s * D : nullptr;
    float ss = 0.f;
    for (int c = lane; c < nc; c += 64) {
      f32x4 v = load4(xr + 4 * c);
      if (dr) v += load4(dr + 4 * c);
      ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)D + eps);
    for (int c = lane; c < nc; c += 64) {
      f32x4 v = load4(xr + 4 * c);
      if (dr) v += load4(dr + 4 * c);
      store4(o + 4 * c, load4(w + 4 * c) * (v * rs));
    }
    return;
  } else {
    float* xr = x + (size_t)r * D;
    float ss = 0.f;
    if constexpr (MODE == RMS_EMBED) {
      int id = idx[r];
      id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
      const float* e = table + (size_t)id * D;
      for (int c = lane; c < nc; c += 64) {
        const f32x4 v = load4(e + 4 * c);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        store4(xr + 4 * c, v);
      }
    } else {
      const T* dr = delta ? delta + (size_t)r * D : nullptr;
      for (int c = lane; c < nc; c += 64) {
        f32x4 v = load4(xr + 4 * c);
        if (dr) {
          v += load4(dr + 4 * c);
          store4(xr + 4 * c, v);
        }
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      }
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)D + eps);
    T* hr = h + (size_t)r * D;
    // a lane re-reads only the chunks it wrote itself: no cross-lane ordering is needed
    for (int c = lane; c < nc; c += 64) store4(hr + 4 * c, load4(w + 4 * c) * (load4(xr + 4 * c) * rs));
  }
}

// gelu_new as T5 v1.1 defines it (tanh form; NOT the erf GELU of common.hpp)
__device__ __forceinline__ float gelu_new_f(float u) {
  return 0.5f * u * (1.f + tanhf(0.7978845608028654f * (u + 0.044715f * u * u * u)));
}

// y[t, f] = gelu_new(u[t, f]) * u[t, F + f]; u is the output of the one GEMM over Wi0 | Wi1.  16-byte chunks.
template <typename T>
__global__ void t5_gated_gelu_kernel(const T* __restrict__ u, T* __restrict__ y, size_t rows, int F) {
  constexpr int EPV = Tr<T>::EPV;
  const int k = F / EPV;
  const size_t total = rows * k;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / k;
    const int c = (int)(i - t * k);
    Chunk<T> a, b;
    a.load(u + t * 2 * F + (size_t)c * EPV);
    b.load(u + t * 2 * F + F + (size_t)c * EPV);
#pragma unroll
    for (int e = 0; e < EPV; ++e) a.v[e] = gelu_new_f(a.v[e]) * b.v[e];
    a.store(y + i * EPV);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Relative-bias self-attention forward over packed, variable-length sequences; head dim 64.
//
// Work item = (sequence b, head h, tile of 16 queries), ONE WAVE each; a 256-thread block holds four consecutive items
// of one head, so the short rows of a caption batch (10-40 tokens = 1-3 tiles) share blocks instead of each occupying
// one.  The block's only shared state is the head's bias table over r = pos_k - pos_q in [-(S-1), S-1] (2S-1 floats in
// LDS, read once per score); after the barrier behind its load the waves are independent (a wave whose tile lies beyond
// its row's end leaves).
//
// Per wave, keys stream in tiles of 32 with a running max / sum (any row length; one or two iterations for <= 64):
//   S^T = K Q^T  as two 16 x 16 tiles: lane (c = l & 15, g = l >> 4) holds query c, keys 16 t + 4 g + i (t = 0, 1; i < 4)
//                -- a query's 32 scores sit in 4 lanes x 8 registers: the row max / sum are 8 register ops + 2 shuffles
//                and the statistics stay on the query's own lanes;
//   O^T = V^T P^T: the 8 probabilities a lane holds ARE its B fragment (column = query c, reduction slots (g, j)) under
//                the slot order  key(g, j) = 16 (j >> 2) + 4 g + (j & 3)  -- no transposition of P, in either dtype;
//                the accumulator is lane (c, g) -> query c, channels 16 n + 4 g + i: rescaling uses the lane's own
//                statistics and the output is written in 8 / 16-byte pieces.
//   V^T  is the A fragment (row = channel, reduction slots = keys): V is key-major in memory, so each wave transposes
//        its 32 x 64 tile through a private LDS image [64 channels][32 slots (+ pad)] -- 16-byte global loads, scalar
//        LDS writes to the slot of each key, one vector LDS read per fragment.  Rows are padded by 16 bytes, which
//        spreads the 16 channel rows of a fragment read over the banks.
// Q and K fragments are read straight from global memory (8 consecutive channels per lane = one 16 / 32-byte load).
// Loads of keys beyond the row's end are clamped to its last token (finite data) and their scores set to -inf.
// LSE: also write lse[h, query] = running max + log(running sum), what the backward (text_encoder_bwd.hip) recomputes the
// probabilities from; `out` is the same bits either way.
template <typename T, bool LSE>
__global__ __launch_bounds__(256) void t5_attn_kernel(const T* __restrict__ qkv, const int* __restrict__ seq_start,
                                                      const int* __restrict__ pos, const float* __restrict__ bias,
                                                      T* __restrict__ out, float* __restrict__ lse, int B, int Ttot, int S,
                                                      int qtiles, int H) {
  constexpr int D = 64, KT = 32;
  constexpr int VS = KT + 16 / (int)sizeof(T);          // slots per channel row of the V^T image, padded by 16 bytes
  __shared__ float tab[1024];
  __shared__ __attribute__((aligned(16))) T vt_all[4][D * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y;
  const int nrel = 2 * S - 1;
  for (int i = tid; i < nrel; i += 256) tab[i] = bias[(size_t)h * nrel + i];
  __syncthreads();

  const int item = blockIdx.x * 4 + wave;
  const int b = item / qtiles, qt = item - b * qtiles;
  if (b >= B) return;
  const int t0 = seq_start[b];
  int t1 = seq_start[b + 1];
  t1 = t1 > Ttot ? Ttot : t1;
  const int len = t1 - t0;
  if (t0 < 0 || len <= 0 || qt * 16 >= len) return;

  T* vt = vt_all[wave];
  const int c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)3 * H * D;                   // row stride of qkv
  const T* qb = qkv + (size_t)h * D;
  const T* kb = qb + (size_t)H * D;
  const T* vb = kb + (size_t)H * D;

  const int qi = qt * 16 + c;                            // this lane's query (clamped for loads)
  const int qrow = t0 + (qi < len ? qi : len - 1);
  const int qpos = pos[qrow];
  Frag<T> qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const T* p = qb + (size_t)qrow * rs + ks * 32 + g * 8;
    qf[ks].load_lds(reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p + 4));
  }

  f32x4 o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  for (int k0 = 0; k0 < len; k0 += KT) {
    // ---- scores of 32 keys
    float s[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kk = k0 + t * 16 + c;                    // A row = key c of this 16-key tile
      const T* kr = kb + (size_t)(t0 + (kk < len ? kk : len - 1)) * rs;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Frag<T> kf;
        const T* p = kr + ks * 32 + g * 8;
        kf.load_lds(reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p + 4));
        mma16(acc, kf, qf[ks]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kj = k0 + t * 16 + g * 4 + i;          // the key of acc[i] (row of S^T)
        const bool ok = kj < len;
        int rel = pos[t0 + (ok ? kj : len - 1)] - qpos + (S - 1);
        rel = rel < 0 ? 0 : (rel > nrel - 1 ? nrel - 1 : rel);
        s[t * 4 + i] = ok ? acc[i] + tab[rel] : -INFINITY;
      }
    }
    // ---- stage V^T of these keys: chunk ci -> key ci / CPR, channels (ci % CPR) * EPV ...
    constexpr int EPV = Tr<T>::EPV, CPR = D / EPV;
#pragma unroll
    for (int it = 0; it < KT * CPR / 64; ++it) {
      const int ci = it * 64 + lane;
      const int key = ci / CPR, dc = (ci % CPR) * EPV;
      const int kk = k0 + key;
      Chunk<T> v;
      v.load(vb + (size_t)(t0 + (kk < len ? kk : len - 1)) * rs + dc);
      const int slot = ((key & 15) >> 2) * 8 + (key >> 4) * 4 + (key & 3);
#pragma unroll
      for (int e = 0; e < EPV; ++e) vt[(dc + e) * VS + slot] = from_f32<T>(v.v[e]);
    }
    // ---- running softmax (statistics of query c: registers + the 4 lanes c, c + 16, c + 32, c + 48)
    float tm = s[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) tm = fmaxf(tm, s[i]);
    tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);                       // finite: key k0 is valid in every iteration
    const float alpha = __expf(m - mn);                  // first iteration: exp(-inf) = 0
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s[i] = __expf(s[i] - mn);
      ps += s[i];
    }
    l = l * alpha + ps;
    m = mn;
    Frag<T> pf;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) pf.v[i] = (bf16)s[i];
    } else {
      pf.lo = f32x4{s[0], s[1], s[2], s[3]};
      pf.hi = f32x4{s[4], s[5], s[6], s[7]};
    }
    // the wave's own LDS writes above must have landed before its reads below (LDS serves a wave in order; the wait and
    // the clobber keep the compiler from moving either side)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      Frag<T> vf;
      const T* p = vt + (n * 16 + c) * VS + g * 8;
      vf.load_lds(reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p + 4));
      o[n] *= alpha;
      mma16(o[n], vf, pf);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the next tile overwrites the image
    __builtin_amdgcn_wave_barrier();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi < len) {
    const float inv = 1.f / l;
    T* orow = out + (size_t)(t0 + qi) * H * D + (size_t)h * D;
#pragma unroll
    for (int n = 0; n < 4; ++n) store4(orow + n * 16 + g * 4, o[n] * inv);
    if constexpr (LSE) {
      if (g == 0) lse[(size_t)h * Ttot + t0 + qi] = m + logf(l);
    }
  }
}

}  // namespace mdm

using namespace mdm;

#define MDM_T5_DISPATCH(dtype, ...)                                                 \
  if ((dtype) == DT_F32) { typedef float TT; __VA_ARGS__; }                         \
  else if ((dtype) == DT_BF16) { typedef bf16 TT; __VA_ARGS__; }                    \
  else { MDM_CHECK_ARG(false); }

extern "C" int mdm_t5_embed_rms(const int* ids, const float* table, const float* ln_w, float* x, void* h, int T, int D,
                                int vocab, float eps, int dtype, void* stream) {
  MDM_CHECK_ARG(ids && table && ln_w && x && h);
  MDM_CHECK_ARG(T > 0 && D > 0 && D % 8 == 0 && vocab > 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL((t5_rms_kernel<TT, RMS_EMBED>), dim3((T + 3) / 4), dim3(256), 0, st, ids, table, x,
                                            (const TT*)nullptr, ln_w, (TT*)h, (float*)nullptr, T, D, vocab, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_add_rms(float* x, const void* delta, const float* ln_w, void* h, int T, int D, float eps, int dtype,
                              void* stream) {
  MDM_CHECK_ARG(x && ln_w && h);
  MDM_CHECK_ARG(T > 0 && D > 0 && D % 8 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL((t5_rms_kernel<TT, RMS_ADD>), dim3((T + 3) / 4), dim3(256), 0, st, (const int*)nullptr,
                                            (const float*)nullptr, x, (const TT*)delta, ln_w, (TT*)h, (float*)nullptr, T, D, 0, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_final_rms(const float* x, const void* delta, const float* ln_w, const int* src, float* out, int R,
                                int D, float eps, int dtype, void* stream) {
  MDM_CHECK_ARG(x && ln_w && src && out);
  MDM_CHECK_ARG(R > 0 && D > 0 && D % 8 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL((t5_rms_kernel<TT, RMS_FINAL>), dim3((R + 3) / 4), dim3(256), 0, st, src,
                                            (const float*)nullptr, const_cast<float*>(x), (const TT*)delta, ln_w, (TT*)nullptr, out,
                                            R, D, 0, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_gated_gelu(const void* u, void* y, int T, int F, int dtype, void* stream) {
  MDM_CHECK_ARG(u && y && T > 0 && F > 0 && F % 8 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t total = (size_t)T * (F / (dtype == DT_F32 ? 4 : 8));
  size_t nb = (total + 255) / 256;
  nb = nb > 16384 ? 16384 : nb;
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL(t5_gated_gelu_kernel<TT>, dim3((unsigned)nb), dim3(256), 0, st, (const TT*)u, (TT*)y,
                                            (size_t)T, F));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_attn_fwd(const void* qkv, const int* seq_start, const int* pos, const float* bias_table, void* out,
                               int B, int T, int S, int max_len, int H, int d, int dtype, void* stream) {
  MDM_CHECK_ARG(qkv && seq_start && pos && bias_table && out);
  MDM_CHECK_ARG(d == 64);                                   // the only head dim of the T5 family; anything else: no kernel
  MDM_CHECK_ARG(B > 0 && T > 0 && H > 0 && H <= 65535);
  MDM_CHECK_ARG(S >= 1 && S <= 512 && max_len >= 1 && max_len <= S);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int qtiles = (max_len + 15) / 16;
  const long long items = (long long)B * qtiles;
  MDM_CHECK_ARG(items < (1ll << 30));
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL((t5_attn_kernel<TT, false>), dim3((unsigned)((items + 3) / 4), H), dim3(256), 0, st,
                                            (const TT*)qkv, seq_start, pos, bias_table, (TT*)out, (float*)nullptr, B, T, S, qtiles,
                                            H));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_attn_fwd_lse(const void* qkv, const int* seq_start, const int* pos, const float* bias_table, void* out,
                                   float* lse, int B, int T, int S, int max_len, int H, int d, int dtype, void* stream) {
  MDM_CHECK_ARG(qkv && seq_start && pos && bias_table && out && lse);
  MDM_CHECK_ARG(d == 64);
  MDM_CHECK_ARG(B > 0 && T > 0 && H > 0 && H <= 65535);
  MDM_CHECK_ARG(S >= 1 && S <= 512 && max_len >= 1 && max_len <= S);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int qtiles = (max_len + 15) / 16;
  const long long items = (long long)B * qtiles;
  MDM_CHECK_ARG(items < (1ll << 30));
  MDM_T5_DISPATCH(dtype, hipLaunchKernelGGL((t5_attn_kernel<TT, true>), dim3((unsigned)((items + 3) / 4), H), dim3(256), 0, st,
                                            (const TT*)qkv, seq_start, pos, bias_table, (TT*)out, lse, B, T, S, qtiles, H));
  MDM_LAUNCH_STATUS();
}
