// Input gradients of the frozen T5 encoder of text_encoder.hip (textual inversion: the only trainable thing is a few
// rows of the embedding, so the backward is a chain of INPUT gradients -- no weight gradient, no bias-table gradient).
// Everything between the seven input-gradient projections (the existing GEMM) lives here:
//   t5_attn_bwd_q_kernel / t5_attn_bwd_kv_kernel   dQ | dK, dV of softmax(q k^T + bias) v from the saved log-sum-exp
//   t5_gated_gelu_bwd_kernel                       du of y = gelu_new(u[:, :F]) * u[:, F:]
//   t5_rms_bwd_kernel                              dx (+)= input gradient of h = w * x * rsqrt(mean(x^2) + eps)
//   t5_embed_slots_kernel                          embedding gather + first RMSNorm with learned rows overriding ids
//   t5_embed_bwd_kernel                            dlearned[j] = sum of dx0 over the tokens of slot j, in token order
// The conventions are the forward's: fp32 residual stream, statistics and softmax; T is the storage type of the GEMM
// operands.  No atomics: every output element is produced by one lane in a fixed order, so two runs agree in every bit
// and a sequence's gradients do not depend on the rest of the batch.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

__device__ __forceinline__ void bstore4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void bstore4(bf16* p, const f32x4& v) {
  bf16x4 t = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<bf16x4*>(p) = t;
}
__device__ __forceinline__ f32x4 bload4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 bload4(const bf16* p) {
  const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
}

// sum over the 8 reduction slots a lane holds of a[j] * b[j], fp32
__device__ __forceinline__ float frag_dot(const Frag<bf16>& a, const Frag<bf16>& b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (float)a.v[j] * (float)b.v[j];
  return s;
}
__device__ __forceinline__ float frag_dot(const Frag<float>& a, const Frag<float>& b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += a.lo[j] * b.lo[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) s += a.hi[j] * b.hi[j];
  return s;
}
// the 8 fp32 values a lane holds of a 32-wide tile of the score matrix, as the B fragment of the next product
template <typename T> __device__ __forceinline__ void frag_of(Frag<T>& f, const float (&s)[8]);
template <> __device__ __forceinline__ void frag_of<bf16>(Frag<bf16>& f, const float (&s)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f.v[i] = (bf16)s[i];
}
template <> __device__ __forceinline__ void frag_of<float>(Frag<float>& f, const float (&s)[8]) {
  f.lo = f32x4{s[0], s[1], s[2], s[3]};
  f.hi = f32x4{s[4], s[5], s[6], s[7]};
}
// 8 consecutive channels of a row as a fragment, straight from global memory
template <typename T> __device__ __forceinline__ void frag_row(Frag<T>& f, const T* p) {
  f.load_lds(reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p + 4));
}

// The wave's own LDS writes must have landed before its reads, and its reads must be done before the image is written
// again (LDS serves a wave in order; the wait and the clobber keep the compiler from moving either side).
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Transposed image [64 channels][32 slots (+ pad)] of 32 rows of a row-major [*, 64] operand, as the forward stages V^T:
// row j of the tile (clamped to the sequence's last token) lands in slot ((j & 15) >> 2) * 8 + (j >> 4) * 4 + (j & 3),
// the reduction slot in which the lanes hold that row's score.  base points at (token 0 of the tensor, channel 0 of
// the head); stride is the tensor's row stride in elements.
template <typename T, int VS>
__device__ __forceinline__ void stage_transposed(T* img, const T* base, size_t stride, int t0, int len, int j0, int lane) {
  constexpr int D = 64, KT = 32, EPV = Tr<T>::EPV, CPR = D / EPV;
#pragma unroll
  for (int it = 0; it < KT * CPR / 64; ++it) {
    const int ci = it * 64 + lane;
    const int row = ci / CPR, dc = (ci % CPR) * EPV;
    const int jj = j0 + row;
    Chunk<T> v;
    v.load(base + (size_t)(t0 + (jj < len ? jj : len - 1)) * stride + dc);
    const int slot = ((row & 15) >> 2) * 8 + (row >> 4) * 4 + (row & 3);
#pragma unroll
    for (int e = 0; e < EPV; ++e) img[(dc + e) * VS + slot] = from_f32<T>(v.v[e]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Attention backward, pass 1: dQ.  The forward's layout: one wave per (sequence, head, tile of 16 queries), keys stream
// in tiles of 32.  Lane (c = l & 15, g = l >> 4) holds query c and keys 16 t + 4 g + i:
//   S^T  = K Q^T,  dP^T = V dO^T    (A = the key tile's rows of K / V from global memory, B = the wave's Q / dO)
//   P    = exp(S + bias - lse[query]),   dS = P (dP - delta[query]),   delta = rowsum(dO o O)  (the lane's 16 channels
//          of its query + 2 shuffles)
//   dQ^T += K^T dS^T               (A = the transposed K image in LDS, B = the lane's 8 dS values as they are)
// Keys beyond the row's end: loads clamped to the last token, P = 0.
template <typename T>
__global__ __launch_bounds__(256) void t5_attn_bwd_q_kernel(const T* __restrict__ qkv, const T* __restrict__ out,
                                                            const float* __restrict__ lse, const T* __restrict__ dout,
                                                            const int* __restrict__ seq_start, const int* __restrict__ pos,
                                                            const float* __restrict__ bias, T* __restrict__ dqkv, int B,
                                                            int Ttot, int S, int qtiles, int H) {
  constexpr int D = 64, KT = 32;
  constexpr int VS = KT + 16 / (int)sizeof(T);
  __shared__ float tab[1024];
  __shared__ __attribute__((aligned(16))) T img_all[4][D * VS];
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

  T* img = img_all[wave];
  const int c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)3 * H * D, os = (size_t)H * D;
  const T* qb = qkv + (size_t)h * D;
  const T* kb = qb + (size_t)H * D;
  const T* vb = kb + (size_t)H * D;

  const int qi = qt * 16 + c;
  const int qrow = t0 + (qi < len ? qi : len - 1);
  const int qpos = pos[qrow];
  const float ls = lse[(size_t)h * Ttot + qrow];
  Frag<T> qf[2], dof[2];
  float dl = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    Frag<T> of;
    frag_row(qf[ks], qb + (size_t)qrow * rs + ks * 32 + g * 8);
    frag_row(dof[ks], dout + (size_t)qrow * os + (size_t)h * D + ks * 32 + g * 8);
    frag_row(of, out + (size_t)qrow * os + (size_t)h * D + ks * 32 + g * 8);
    dl += frag_dot(dof[ks], of);
  }
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);

  f32x4 dq[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < len; k0 += KT) {
    float ds[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kk = k0 + t * 16 + c;                    // A row = key c of this 16-key tile
      const size_t kr = (size_t)(t0 + (kk < len ? kk : len - 1)) * rs;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Frag<T> kf, vf;
        frag_row(kf, kb + kr + ks * 32 + g * 8);
        frag_row(vf, vb + kr + ks * 32 + g * 8);
        mma16(acc, kf, qf[ks]);
        mma16(accp, vf, dof[ks]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kj = k0 + t * 16 + g * 4 + i;          // the key of acc[i]
        const bool ok = kj < len;
        int rel = pos[t0 + (ok ? kj : len - 1)] - qpos + (S - 1);
        rel = rel < 0 ? 0 : (rel > nrel - 1 ? nrel - 1 : rel);
        const float p = ok ? __expf(acc[i] + tab[rel] - ls) : 0.f;
        ds[t * 4 + i] = p * (accp[i] - dl);
      }
    }
    stage_transposed<T, VS>(img, kb, rs, t0, len, k0, lane);
    Frag<T> dsf;
    frag_of<T>(dsf, ds);
    wave_lds_fence();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      Frag<T> kf;
      frag_row(kf, img + (n * 16 + c) * VS + g * 8);
      mma16(dq[n], kf, dsf);
    }
    wave_lds_fence();
  }
  if (qi < len) {
    T* drow = dqkv + (size_t)(t0 + qi) * rs + (size_t)h * D;
#pragma unroll
    for (int n = 0; n < 4; ++n) bstore4(drow + n * 16 + g * 4, dq[n]);
  }
}

// Pass 2: dK and dV.  One wave per (sequence, head, tile of 16 keys); queries stream in tiles of 32.  Lane (c, g) holds
// key c and queries 16 t + 4 g + i:
//   S  = Q K^T,  dP = dO V^T        (A = the query tile's rows of Q / dO from global memory, B = the wave's K / V)
//   delta of the tile's 32 queries: each query's row sum on the lanes that loaded its dO, through 32 floats of LDS
//   P, dS as in pass 1 (lse and delta now per register, the key per lane)
//   dV^T += dO^T P                  (A = the transposed dO image, B = the lane's 8 P values)
//   dK^T += Q^T dS                  (A = the transposed Q image -- the same LDS, after the dV product -- B = dS)
// Queries beyond the row's end: loads clamped, P = 0.  Recomputing S here rather than exchanging it removes every sum
// across waves.
template <typename T>
__global__ __launch_bounds__(256) void t5_attn_bwd_kv_kernel(const T* __restrict__ qkv, const T* __restrict__ out,
                                                             const float* __restrict__ lse, const T* __restrict__ dout,
                                                             const int* __restrict__ seq_start, const int* __restrict__ pos,
                                                             const float* __restrict__ bias, T* __restrict__ dqkv, int B,
                                                             int Ttot, int S, int ktiles, int H) {
  constexpr int D = 64, QT = 32;
  constexpr int VS = QT + 16 / (int)sizeof(T);
  __shared__ float tab[1024];
  __shared__ float dl_all[4][QT];
  __shared__ __attribute__((aligned(16))) T img_all[4][D * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y;
  const int nrel = 2 * S - 1;
  for (int i = tid; i < nrel; i += 256) tab[i] = bias[(size_t)h * nrel + i];
  __syncthreads();

  const int item = blockIdx.x * 4 + wave;
  const int b = item / ktiles, kt = item - b * ktiles;
  if (b >= B) return;
  const int t0 = seq_start[b];
  int t1 = seq_start[b + 1];
  t1 = t1 > Ttot ? Ttot : t1;
  const int len = t1 - t0;
  if (t0 < 0 || len <= 0 || kt * 16 >= len) return;

  T* img = img_all[wave];
  float* dls = dl_all[wave];
  const int c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)3 * H * D, os = (size_t)H * D;
  const T* qb = qkv + (size_t)h * D;
  const T* kb = qb + (size_t)H * D;
  const T* vb = kb + (size_t)H * D;
  const T* ob = out + (size_t)h * D;
  const T* dob = dout + (size_t)h * D;

  const int ki = kt * 16 + c;
  const int krow = t0 + (ki < len ? ki : len - 1);
  const int kpos = pos[krow];
  Frag<T> kf[2], vf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    frag_row(kf[ks], kb + (size_t)krow * rs + ks * 32 + g * 8);
    frag_row(vf[ks], vb + (size_t)krow * rs + ks * 32 + g * 8);
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) dk[n] = dv[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int q0 = 0; q0 < len; q0 += QT) {
    f32x4 acc[2], accp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int qq = q0 + t * 16 + c;                    // A row = query c of this 16-query tile
      const int qr = t0 + (qq < len ? qq : len - 1);
      acc[t] = accp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      float dl = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Frag<T> qf, dof, of;
        frag_row(qf, qb + (size_t)qr * rs + ks * 32 + g * 8);
        frag_row(dof, dob + (size_t)qr * os + ks * 32 + g * 8);
        frag_row(of, ob + (size_t)qr * os + ks * 32 + g * 8);
        mma16(acc[t], qf, kf[ks]);
        mma16(accp[t], dof, vf[ks]);
        dl += frag_dot(dof, of);
      }
      dl += __shfl_xor(dl, 16, 64);
      dl += __shfl_xor(dl, 32, 64);
      if (g == 0) dls[t * 16 + c] = dl;
    }
    wave_lds_fence();
    float p[8], ds[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qj = q0 + t * 16 + g * 4 + i;          // the query of acc[t][i]
        const bool ok = qj < len;
        const int qr = t0 + (ok ? qj : len - 1);
        int rel = kpos - pos[qr] + (S - 1);
        rel = rel < 0 ? 0 : (rel > nrel - 1 ? nrel - 1 : rel);
        const float pp = ok ? __expf(acc[t][i] + tab[rel] - lse[(size_t)h * Ttot + qr]) : 0.f;
        p[t * 4 + i] = pp;
        ds[t * 4 + i] = pp * (accp[t][i] - dls[t * 16 + g * 4 + i]);
      }
    }
    Frag<T> pf, dsf;
    frag_of<T>(pf, p);
    frag_of<T>(dsf, ds);
    stage_transposed<T, VS>(img, dob, os, t0, len, q0, lane);
    wave_lds_fence();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      Frag<T> af;
      frag_row(af, img + (n * 16 + c) * VS + g * 8);
      mma16(dv[n], af, pf);
    }
    wave_lds_fence();
    stage_transposed<T, VS>(img, qb, rs, t0, len, q0, lane);
    wave_lds_fence();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      Frag<T> af;
      frag_row(af, img + (n * 16 + c) * VS + g * 8);
      mma16(dk[n], af, dsf);
    }
    wave_lds_fence();
  }
  if (ki < len) {
    T* drow = dqkv + (size_t)(t0 + ki) * rs + (size_t)H * D + (size_t)h * D;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      bstore4(drow + n * 16 + g * 4, dk[n]);
      bstore4(drow + (size_t)H * D + n * 16 + g * 4, dv[n]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// gelu_new and its derivative (tanh form, the forward's constants): with z = k (a + 0.044715 a^3), t = tanh z,
//   gelu(a) = 0.5 a (1 + t),   gelu'(a) = 0.5 (1 + t) + 0.5 a (1 - t^2) k (1 + 3 * 0.044715 a^2)
template <typename T>
__global__ void t5_gated_gelu_bwd_kernel(const T* __restrict__ u, const T* __restrict__ dy, T* __restrict__ du, size_t rows,
                                         int F) {
  constexpr int EPV = Tr<T>::EPV;
  const int k = F / EPV;
  const size_t total = rows * k;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / k;
    const int c = (int)(i - t * k);
    Chunk<T> a, b, d, da, db;
    a.load(u + t * 2 * F + (size_t)c * EPV);
    b.load(u + t * 2 * F + F + (size_t)c * EPV);
    d.load(dy + i * EPV);
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      const float x = a.v[e];
      const float th = tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x));
      const float ge = 0.5f * x * (1.f + th);
      const float dg = 0.5f * (1.f + th) + 0.5f * x * (1.f - th * th) * 0.7978845608028654f * (1.f + 0.134145f * x * x);
      da.v[e] = d.v[e] * b.v[e] * dg;
      db.v[e] = d.v[e] * ge;
    }
    da.store(du + t * 2 * F + (size_t)c * EPV);
    db.store(du + t * 2 * F + F + (size_t)c * EPV);
  }
}

// One row per wave, four rows per block; a lane walks the row in chunks of 4 channels (D % 4 == 0), as t5_rms_kernel:
// 16 bytes of the fp32 operands (x, w, dout, dx), 8 bytes of the bf16 ones (delta, dh, dxt).  First pass: sum x^2 and
// sum w dh x; second pass: g = rs (w dh) - x rs^3 / D sum(w dh x).
//   FINAL = false   x is the saved fp32 row r, dh the storage-type gradient of the norm's output; dx[r] += g
//   FINAL = true    x = xs[r] + delta[r] (the forward's final norm forms the same sum), dh = row flat[r] of the fp32
//                   [B * S, D] output gradient (a gather); dx[r] = g
// dxt (storage type, or null): a copy of the updated dx row -- the operand of the next input-gradient GEMM.
template <typename T, bool FINAL>
__global__ __launch_bounds__(256) void t5_rms_bwd_kernel(const float* __restrict__ xs, const T* __restrict__ delta,
                                                         const float* __restrict__ w, const T* __restrict__ dh,
                                                         const float* __restrict__ dout, const int* __restrict__ flat,
                                                         float* __restrict__ dx, T* __restrict__ dxt, int rows, int D,
                                                         float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nc = D >> 2;
  const float* xr = xs + (size_t)r * D;
  const T* dr = (FINAL && delta) ? delta + (size_t)r * D : nullptr;
  const T* gh = FINAL ? nullptr : dh + (size_t)r * D;
  const float* go = FINAL ? dout + (size_t)flat[r] * D : nullptr;
  float ss = 0.f, dot = 0.f;
  for (int c = lane; c < nc; c += 64) {
    f32x4 v = bload4(xr + 4 * c);
    if (dr) v += bload4(dr + 4 * c);
    const f32x4 wg = bload4(w + 4 * c) * (FINAL ? bload4(go + 4 * c) : bload4(gh + 4 * c));
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    dot += wg[0] * v[0] + wg[1] * v[1] + wg[2] * v[2] + wg[3] * v[3];
  }
  const float rsv = rsqrtf(wave_sum(ss) / (float)D + eps);
  const float coef = rsv * rsv * rsv * (wave_sum(dot) / (float)D);
  float* dxr = dx + (size_t)r * D;
  for (int c = lane; c < nc; c += 64) {
    f32x4 v = bload4(xr + 4 * c);
    if (dr) v += bload4(dr + 4 * c);
    const f32x4 wg = bload4(w + 4 * c) * (FINAL ? bload4(go + 4 * c) : bload4(gh + 4 * c));
    f32x4 gx = wg * rsv - v * coef;
    if constexpr (!FINAL) gx += bload4(dxr + 4 * c);
    bstore4(dxr + 4 * c, gx);
    if (dxt) bstore4(dxt + (size_t)r * D + 4 * c, gx);
  }
}

// mdm_t5_embed_rms with an override: slot_of_id[id] >= 0 reads row slot of `learned` instead of the vocabulary table.
// Ids are clamped to [0, n_ids); an id in [vocab, n_ids) without a slot (the host refuses it) reads the table's last row.
template <typename T>
__global__ __launch_bounds__(256) void t5_embed_slots_kernel(const int* __restrict__ ids, const float* __restrict__ table,
                                                             const int* __restrict__ slot_of_id,
                                                             const float* __restrict__ learned, float* __restrict__ x,
                                                             const float* __restrict__ w, T* __restrict__ h, int rows, int D,
                                                             int vocab, int n_ids, int P, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nc = D >> 2;
  int id = ids[r];
  id = id < 0 ? 0 : (id >= n_ids ? n_ids - 1 : id);
  const int slot = slot_of_id[id];
  const float* e = (slot >= 0 && slot < P) ? learned + (size_t)slot * D : table + (size_t)(id >= vocab ? vocab - 1 : id) * D;
  float* xr = x + (size_t)r * D;
  float ss = 0.f;
  for (int c = lane; c < nc; c += 64) {
    const f32x4 v = bload4(e + 4 * c);
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    bstore4(xr + 4 * c, v);
  }
  const float rs = rsqrtf(wave_sum(ss) / (float)D + eps);
  T* hr = h + (size_t)r * D;
  for (int c = lane; c < nc; c += 64) bstore4(hr + 4 * c, bload4(w + 4 * c) * (bload4(xr + 4 * c) * rs));
}

// dlearned[j, 4 c ...] = sum over tokens[slot_start[j] ... slot_start[j + 1]) of dx0[token], one thread per (slot, chunk)
// walking the slot's list in order: a sequential fp32 sum in ascending token order.
__global__ void t5_embed_bwd_kernel(const float* __restrict__ dx0, const int* __restrict__ slot_start,
                                    const int* __restrict__ tokens, float* __restrict__ dlearned, int P, int D, int n, int T) {
  const int nc = D >> 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * nc) return;
  const int j = i / nc, c = i - j * nc;
  int a = slot_start[j], e = slot_start[j + 1];
  a = a < 0 ? 0 : a;
  e = e > n ? n : e;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int k = a; k < e; ++k) {
    const int t = tokens[k];
    if (t >= 0 && t < T) s += bload4(dx0 + (size_t)t * D + 4 * c);
  }
  bstore4(dlearned + (size_t)j * D + 4 * c, s);
}

}  // namespace mdm

using namespace mdm;

#define MDM_T5B_DISPATCH(dtype, ...)                                                \
  if ((dtype) == DT_F32) { typedef float TT; __VA_ARGS__; }                         \
  else if ((dtype) == DT_BF16) { typedef bf16 TT; __VA_ARGS__; }                    \
  else { MDM_CHECK_ARG(false); }

extern "C" int mdm_t5_attn_bwd(const void* qkv, const void* out, const float* lse, const void* dout, const int* seq_start,
                               const int* pos, const float* bias_table, void* dqkv, int B, int T, int S, int max_len, int H,
                               int d, int dtype, void* stream) {
  MDM_CHECK_ARG(qkv && out && lse && dout && seq_start && pos && bias_table && dqkv);
  MDM_CHECK_ARG(d == 64);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(B > 0 && T > 0 && H > 0 && H <= 65535);
  MDM_CHECK_ARG(S >= 1 && S <= 512 && max_len >= 1 && max_len <= S);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int tiles = (max_len + 15) / 16;
  const long long items = (long long)B * tiles;
  MDM_CHECK_ARG(items < (1ll << 30));
  const dim3 grid((unsigned)((items + 3) / 4), H);
  MDM_T5B_DISPATCH(dtype, {
    hipLaunchKernelGGL(t5_attn_bwd_q_kernel<TT>, grid, dim3(256), 0, st, (const TT*)qkv, (const TT*)out, lse, (const TT*)dout,
                       seq_start, pos, bias_table, (TT*)dqkv, B, T, S, tiles, H);
    hipLaunchKernelGGL(t5_attn_bwd_kv_kernel<TT>, grid, dim3(256), 0, st, (const TT*)qkv, (const TT*)out, lse, (const TT*)dout,
                       seq_start, pos, bias_table, (TT*)dqkv, B, T, S, tiles, H);
  });
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_gated_gelu_bwd(const void* u, const void* dy, void* du, int T, int F, int dtype, void* stream) {
  MDM_CHECK_ARG(u && dy && du && T > 0 && F > 0 && F % 8 == 0);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t total = (size_t)T * (F / (dtype == DT_F32 ? 4 : 8));
  size_t nb = (total + 255) / 256;
  nb = nb > 16384 ? 16384 : nb;
  MDM_T5B_DISPATCH(dtype, hipLaunchKernelGGL(t5_gated_gelu_bwd_kernel<TT>, dim3((unsigned)nb), dim3(256), 0, st, (const TT*)u,
                                             (const TT*)dy, (TT*)du, (size_t)T, F));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_rms_bwd(const float* x, const float* ln_w, const void* dh, float* dx, void* dx_lo, int T, int D,
                              float eps, int dtype, void* stream) {
  MDM_CHECK_ARG(x && ln_w && dh && dx);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(T > 0 && D > 0 && D % 8 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5B_DISPATCH(dtype, hipLaunchKernelGGL((t5_rms_bwd_kernel<TT, false>), dim3((T + 3) / 4), dim3(256), 0, st, x,
                                             (const TT*)nullptr, ln_w, (const TT*)dh, (const float*)nullptr, (const int*)nullptr,
                                             dx, (TT*)dx_lo, T, D, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_final_rms_bwd(const float* x, const void* delta, const float* ln_w, const float* dout, const int* flat,
                                    float* dx, void* dx_lo, int T, int D, float eps, int dtype, void* stream) {
  MDM_CHECK_ARG(x && ln_w && dout && flat && dx);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(T > 0 && D > 0 && D % 8 == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5B_DISPATCH(dtype, hipLaunchKernelGGL((t5_rms_bwd_kernel<TT, true>), dim3((T + 3) / 4), dim3(256), 0, st, x,
                                             (const TT*)delta, ln_w, (const TT*)nullptr, dout, flat, dx, (TT*)dx_lo, T, D, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_embed_rms_slots(const int* ids, const float* table, const int* slot_of_id, const float* learned,
                                      const float* ln_w, float* x, void* h, int T, int D, int vocab, int n_ids, int P,
                                      float eps, int dtype, void* stream) {
  MDM_CHECK_ARG(ids && table && slot_of_id && learned && ln_w && x && h);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(T > 0 && D > 0 && D % 8 == 0 && vocab > 0 && n_ids >= vocab && P > 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MDM_T5B_DISPATCH(dtype, hipLaunchKernelGGL(t5_embed_slots_kernel<TT>, dim3((T + 3) / 4), dim3(256), 0, st, ids, table,
                                             slot_of_id, learned, x, ln_w, (TT*)h, T, D, vocab, n_ids, P, eps));
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_t5_embed_bwd(const float* dx0, const int* slot_start, const int* tokens, float* dlearned, int P, int D,
                                int n, int T, void* stream) {
  MDM_CHECK_ARG(dx0 && slot_start && dlearned && (tokens || n == 0));
  MDM_CHECK_ARG(P > 0 && D > 0 && D % 4 == 0 && n >= 0 && T > 0);
  MDM_CHECK_ARG((long long)P * (D / 4) < (1ll << 30));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int total = P * (D / 4);
  hipLaunchKernelGGL(t5_embed_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, st, dx0, slot_start, tokens, dlearned, P, D,
                     n, T);
  MDM_LAUNCH_STATUS();
}
