// Prompt-to-prompt attention control (Hertz et al. 2022): the two preparation kernels in front of the attention entry points
// the library already has.  An EDITED batch row r computes with the attention maps of its SOURCE row s:
//   out_h[r] = A_h(g_s ? s : r) v_h[r] + P_h(s) V'_h[r] + P_h(r) V''_h[r]
//   V'[r][i, :]  = g_c sum_{j live in r} M_r[i, j] v_c[r][j, :]        (i: a source token, j: an edit token)
//   V''[r][j, :] = (g_c D_r[j] + 1 - g_c) v_c[r][j, :]
// The text term of mdm_attn_fwd is a softmax of its own over the S text keys, so mixing the probabilities over the token axis
// is linear in v_c: (P M) v_c = P (M v_c).  No attention kernel is new:
//   mdm_ctrl_gather_qkv   [R, L, 3C] with q, k of row (g_s ? s : r) and v of row r -> mdm_attn_fwd without text keys;
//                         the source's q in the q columns of a second [R, L, 3C]   -> mdm_attn_cross_bias with kv_a
//   mdm_ctrl_mix_kv       kv_a[r] = (k_c[s] | V'[r]),  kv_b[r] = (k_c[r] | V''[r]) -> two mdm_attn_cross_bias launches
// The gates are device floats that SELECT (0: off, anything else: on), so one captured graph serves a trajectory.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

constexpr int CM_THREADS = 64;   // a thread owns one 16-byte chunk of the C channels
constexpr int CM_TI = 8;         // source tokens per block: every v_c row is loaded once for 8 output rows

// grid (ceil(C / EPV / 64), ceil(S / 8), R).  M rows, D, the mask and both row tables are uniform over a block.
template <typename T>
__global__ __launch_bounds__(CM_THREADS) void ctrl_mix_kv_kernel(const T* __restrict__ kvc, const int* __restrict__ own,
                                                                const int* __restrict__ src, const float* __restrict__ M,
                                                                int ld, const float* __restrict__ D,
                                                                const float* __restrict__ mask, const float* __restrict__ gate,
                                                                T* __restrict__ kv_a, T* __restrict__ kv_b, int N, int S, int C) {
  constexpr int EPV = Tr<T>::EPV;
  const int c = (blockIdx.x * CM_THREADS + threadIdx.x) * EPV;
  if (c >= C) return;
  const int r = blockIdx.z, i0 = blockIdx.y * CM_TI;
  const int ro = own[r], rs = src[r];
  if ((unsigned)ro >= (unsigned)N || (unsigned)rs >= (unsigned)N) return;   // a row table that leaves the batch: nothing is read
  const bool on = gate[0] != 0.f;
  const size_t row2 = 2 * (size_t)C;
  const T* kv_o = kvc + (size_t)ro * S * row2;
  const T* kv_s = kvc + (size_t)rs * S * row2;
  const float* Mr = M + (size_t)r * S * ld;
  const float* mk = mask ? mask + (size_t)ro * S : nullptr;
  const int ni = min(CM_TI, S - i0);

  float acc[CM_TI][EPV];
#pragma unroll
  for (int ii = 0; ii < CM_TI; ++ii)
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[ii][e] = 0.f;
  if (on) {
    for (int j = 0; j < S; ++j) {   // ascending j: the order of the sum is fixed
      if (mk && mk[j] == 0.f) continue;   // a masked edit token: neither its M column nor its v_c row is read
      Chunk<T> v;
      v.load(kv_o + (size_t)j * row2 + C + c);
#pragma unroll
      for (int ii = 0; ii < CM_TI; ++ii) {
        if (ii < ni) {
          const float m = Mr[(size_t)(i0 + ii) * ld + j];
#pragma unroll
          for (int e = 0; e < EPV; ++e) acc[ii][e] = fmaf(m, v.v[e], acc[ii][e]);
        }
      }
    }
  }
#pragma unroll
  for (int ii = 0; ii < CM_TI; ++ii) {
    if (ii >= ni) break;
    const int i = i0 + ii;
    const size_t o = ((size_t)r * S + i) * row2 + c;
    const size_t in_o = (size_t)i * row2 + c;
    // the key halves: bit for bit
    *reinterpret_cast<uint4*>(kv_a + o) = *reinterpret_cast<const uint4*>(kv_s + in_o);
    *reinterpret_cast<uint4*>(kv_b + o) = *reinterpret_cast<const uint4*>(kv_o + in_o);
    Chunk<T> va;
#pragma unroll
    for (int e = 0; e < EPV; ++e) va.v[e] = acc[ii][e];
    va.store(kv_a + o + C);   // gate off: exact zeros
    if (on) {
      const float d = D[(size_t)r * S + i];
      Chunk<T> vb;
      vb.load(kv_o + in_o + C);
#pragma unroll
      for (int e = 0; e < EPV; ++e) vb.v[e] *= d;
      vb.store(kv_b + o + C);
    } else {   // gate off: v_c bit for bit
      *reinterpret_cast<uint4*>(kv_b + o + C) = *reinterpret_cast<const uint4*>(kv_o + in_o + C);
    }
  }
}

// one 16-byte chunk per thread with a grid stride over the R * L * 3C / EPV chunks of the gathered tensor
template <int ESIZE>
__global__ __launch_bounds__(256) void ctrl_gather_qkv_kernel(const uint4* __restrict__ qkv, const int* __restrict__ own,
                                                             const int* __restrict__ src, const float* __restrict__ gate,
                                                             uint4* __restrict__ qkv_self, uint4* __restrict__ q_src, int N,
                                                             int R, int L, int C) {
  const int cc = C / (16 / ESIZE);   // chunks per C channels
  const size_t row = 3 * (size_t)cc, per = (size_t)L * row, total = (size_t)R * per;
  const bool on = gate[0] != 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / per);
    const size_t in_row = i - (size_t)r * per;
    const int col = (int)(in_row % row);
    const int ro = own[r], rs = src[r];
    if ((unsigned)ro >= (unsigned)N || (unsigned)rs >= (unsigned)N) continue;
    const bool v_part = col >= 2 * cc;
    qkv_self[i] = qkv[(size_t)((v_part || !on) ? ro : rs) * per + in_row];
    if (col < cc) q_src[i] = qkv[(size_t)rs * per + in_row];
  }
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_ctrl_mix_kv(const void* kvc, const int* own_rows, const int* src_rows, const float* M, int m_ld,
                               const float* D, const float* mask, const float* gate, void* kv_a, void* kv_b, int N, int R,
                               int S, int C, int dtype, void* stream) {
  MDM_CHECK_ARG(kvc && own_rows && src_rows && M && D && gate && kv_a && kv_b);
  MDM_CHECK_ARG(N > 0 && R > 0 && R <= 65535 && S > 0 && C > 0);
  MDM_CHECK_ARG(m_ld >= S && m_ld % 4 == 0);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int epv = dtype == DT_BF16 ? 8 : 4;
  MDM_CHECK_ARG(C % epv == 0);
  MDM_CHECK_ARG(((uintptr_t)kvc | (uintptr_t)kv_a | (uintptr_t)kv_b) % 16 == 0);
  MDM_CHECK_ARG(kv_a != kv_b && kv_a != kvc && kv_b != kvc);
  const int tiles = (S + CM_TI - 1) / CM_TI;
  MDM_CHECK_ARG(tiles <= 65535);
  const dim3 grid((C / epv + CM_THREADS - 1) / CM_THREADS, tiles, R);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(ctrl_mix_kv_kernel<bf16>, grid, dim3(CM_THREADS), 0, st, (const bf16*)kvc, own_rows, src_rows, M, m_ld,
                       D, mask, gate, (bf16*)kv_a, (bf16*)kv_b, N, S, C);
  else
    hipLaunchKernelGGL(ctrl_mix_kv_kernel<float>, grid, dim3(CM_THREADS), 0, st, (const float*)kvc, own_rows, src_rows, M,
                       m_ld, D, mask, gate, (float*)kv_a, (float*)kv_b, N, S, C);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_ctrl_gather_qkv(const void* qkv, const int* own_rows, const int* src_rows, const float* gate,
                                   void* qkv_self, void* q_src, int N, int R, int L, int C, int dtype, void* stream) {
  MDM_CHECK_ARG(qkv && own_rows && src_rows && gate && qkv_self && q_src);
  MDM_CHECK_ARG(N > 0 && R > 0 && L > 0 && C > 0);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int epv = dtype == DT_BF16 ? 8 : 4;
  MDM_CHECK_ARG(C % epv == 0);
  MDM_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)qkv_self | (uintptr_t)q_src) % 16 == 0);
  MDM_CHECK_ARG(qkv_self != qkv && q_src != qkv && qkv_self != q_src);
  const size_t total = (size_t)R * L * 3 * (C / epv);
  size_t blocks = (total + 255) / 256;
  const size_t cap = (size_t)device_cus() * 16;
  if (blocks > cap) blocks = cap;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(ctrl_gather_qkv_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)qkv, own_rows,
                       src_rows, gate, (uint4*)qkv_self, (uint4*)q_src, N, R, L, C);
  else
    hipLaunchKernelGGL(ctrl_gather_qkv_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)qkv, own_rows,
                       src_rows, gate, (uint4*)qkv_self, (uint4*)q_src, N, R, L, C);
  MDM_LAUNCH_STATUS();
}
