// Low-rank adapters (LoRA, Hu et al. 2021) on the 1x1 / linear projections of the attention layers:
//   y = W x + b + s * B (A x),   A [r, Cin], B [Cout, r], s = alpha / r,  r <= 64
// The base term is the ordinary convolution launch; this file holds the rank-r arithmetic beside it.  With r <= 64
// against M = 16 384 ... 262 144 rows all of it is HBM-bound streaming with a few MFMAs per byte, so none of it shares
// the tile GEMMs of gemm_conv.hip (they would pad r to a 64-wide tile and fill a quarter of the chip):
//   lora_down_kernel     T[M, r]  = X[M, C] A^T          X read once, T written once
//   lora_up_add_kernel   Y[M, N] (+)= s T[M, r] B^T      one read-modify-write pass over Y
//   lora_wgrad_kernel    D[r, C] (+)= s P[M, r]^T Q[M, C]   P, Q read once; split over M into fp32 slabs, summed in
//   + lora_wgrad_reduce_kernel                            a fixed order (no float atomics: deterministic)
// All three form their products on the MFMA pipe through the fragments of common.hpp (bf16: v_mfma_f32_16x16x32_bf16,
// fp32: exact v_mfma_f32_16x16x4_f32), accumulate in fp32, and pad r to the 32-deep / 16-wide MFMA shape in registers:
// the caller passes r = 4 as it is.  Guarded loads are branch-free (clamped address + select) and no loop holds a
// store: every wave loads, computes, and stores once at its end.
#include "common.hpp"

namespace mdm {
namespace {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// 8 consecutive elements of T at p as an MFMA fragment; !ok -> zeros (the load then reads `safe`, a mapped address)
__device__ __forceinline__ void ldg_frag8(Frag<bf16>& f, const bf16* p, bool ok, const bf16* safe) {
  const uint4 t = *reinterpret_cast<const uint4*>(ok ? p : safe);
  uint4 u = uint4{ok ? t.x : 0u, ok ? t.y : 0u, ok ? t.z : 0u, ok ? t.w : 0u};
  f.v = *reinterpret_cast<bf16x8*>(&u);
}
__device__ __forceinline__ void ldg_frag8(Frag<float>& f, const float* p, bool ok, const float* safe) {
  const float* q = ok ? p : safe;
  const f32x4 a = *reinterpret_cast<const f32x4*>(q), b = *reinterpret_cast<const f32x4*>(q + 4);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f.lo = ok ? a : z;
  f.hi = ok ? b : z;
}

// the same fragment over a reduction dimension that is a multiple of 4 only (the rank): `n` = 8, 4 or <= 0 valid
// elements from p on, loaded as two halves (8 bytes each for bf16: a row of r = 4 is 8-byte aligned, not 16)
__device__ __forceinline__ void ldg_frag44(Frag<bf16>& f, const bf16* p, int n, const bf16* safe) {
  const bool ok0 = n >= 4, ok1 = n >= 8;
  const u32x2 a = *reinterpret_cast<const u32x2*>(ok0 ? p : safe), b = *reinterpret_cast<const u32x2*>(ok1 ? p + 4 : safe);
  uint4 u = uint4{ok0 ? a.x : 0u, ok0 ? a.y : 0u, ok1 ? b.x : 0u, ok1 ? b.y : 0u};
  f.v = *reinterpret_cast<bf16x8*>(&u);
}
__device__ __forceinline__ void ldg_frag44(Frag<float>& f, const float* p, int n, const float* safe) {
  const bool ok0 = n >= 4, ok1 = n >= 8;
  const f32x4 a = *reinterpret_cast<const f32x4*>(ok0 ? p : safe), b = *reinterpret_cast<const f32x4*>(ok1 ? p + 4 : safe);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f.lo = ok0 ? a : z;
  f.hi = ok1 ? b : z;
}

// 8 scalars (reduction index = the slow dimension in memory) as a fragment
__device__ __forceinline__ void frag_of(Frag<bf16>& f, const bf16 (&e)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = e[j];
}
__device__ __forceinline__ void frag_of(Frag<float>& f, const float (&e)[8]) {
  f.lo = f32x4{e[0], e[1], e[2], e[3]};
  f.hi = f32x4{e[4], e[5], e[6], e[7]};
}

// 8 consecutive elements of T <-> fp32
__device__ __forceinline__ void ld8(float (&v)[8], const bf16* p) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
__device__ __forceinline__ void ld8(float (&v)[8], const float* p) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}
__device__ __forceinline__ void st8(bf16* p, const float (&v)[8]) {
  bf16x8 t;
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = (bf16)v[i];
  *reinterpret_cast<bf16x8*>(p) = t;
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ void st4(bf16* p, const f32x4& v) {
  *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

// ---------------------------------------------------------------------------------------------------------------------
// T[M, r] = X[M, C] A^T.  A block owns 32 rows of X; its four waves take the 32-deep k-steps of C in turn (wave w: steps
// w, w + 4, ...: the four 64-byte pieces a row contributes per round are one contiguous 256 bytes), each with the A
// fragments of its own steps -- A (<= 64 x 3072) is re-read per block through L2, X comes from HBM exactly once.  The
// four partial tiles meet in LDS and are summed in wave order.  MFMA operands: A rows first, X rows second, so that a
// lane ends up with 4 consecutive ranks of one row of T: one 8- / 16-byte store.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DOWN_RT = 2;   // 16-row tiles of X per block

template <typename T, int NT>   // NT: 16-row tiles of A (r <= 16 NT)
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ X, const T* __restrict__ A, T* __restrict__ Tout,
                                                        int M, int C, int r) {
  __shared__ f32x4 part[4][DOWN_RT * NT][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int m0 = blockIdx.x * (16 * DOWN_RT);
  f32x4 acc[DOWN_RT][NT];
#pragma unroll
  for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ksteps = (C + 31) / 32;
  for (int ks = w; ks < ksteps; ks += 4) {
    const int k = ks * 32 + quad * 8;
    const bool kok = k < C;   // C % 8 == 0: a chunk is inside or outside as a whole
    Frag<T> xf[DOWN_RT], af[NT];
#pragma unroll
    for (int rt = 0; rt < DOWN_RT; ++rt) {
      const int m = m0 + rt * 16 + l15;
      ldg_frag8(xf[rt], X + (size_t)m * C + k, kok && m < M, X);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 16 + l15;
      ldg_frag8(af[t], A + (size_t)n * C + k, kok && n < r, A);
    }
#pragma unroll
    for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
      for (int t = 0; t < NT; ++t) mma16(acc[rt][t], af[t], xf[rt]);   // [rank n][row m]
  }
#pragma unroll
  for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) part[w][rt * NT + t][lane] = acc[rt][t];
  __syncthreads();
  for (int idx = threadIdx.x; idx < DOWN_RT * NT * 64; idx += 256) {
    const int tile = idx >> 6, ln = idx & 63;
    const f32x4 s = ((part[0][tile][ln] + part[1][tile][ln]) + part[2][tile][ln]) + part[3][tile][ln];
    const int m = m0 + (tile / NT) * 16 + (ln & 15);
    const int n = (tile % NT) * 16 + (ln >> 4) * 4;
    if (m < M && n < r) st4(Tout + (size_t)m * r + n, s);   // r % 4 == 0: the four ranks are inside together
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Y[M, N] (+)= s T[M, r] B^T.  A wave owns 32 rows x 128 columns of Y and nothing else: it requests its 8 chunks of Y,
// the T fragments of its rows and the B fragments of its columns, forms the rank-r product (one or two 32-deep MFMA
// steps, r padded with zeros), adds in fp32 and stores -- no loop, so no load ever queues behind a store.  The rows of B
// are dealt to the first MFMA operand in the order n = 8 (i / 4) + 4 h + i % 4 (h: which of the two MFMAs of a 32-column
// group), which leaves every lane with 8 CONSECUTIVE columns of one row: a 16-byte chunk of Y for bf16 tensors.
// B == 0 gives acc == 0 and y + 0.0f rounds back to y: bit-identical without a special case.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int UP_RT = 2, UP_U = 4;   // wave tile: 16 UP_RT rows x 32 UP_U columns

template <typename T, int KS, bool ACC>   // KS: 32-deep steps over r (r <= 32 KS)
__global__ __launch_bounds__(256) void lora_up_add_kernel(T* __restrict__ Y, const T* __restrict__ Tm, const T* __restrict__ B,
                                                          int M, int N, int r, float s, int ncol, int ntiles) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int wid = blockIdx.x * 4 + w;
  if (wid >= ntiles) return;   // wave-uniform; the kernel has no barrier
  const int m0 = (wid / ncol) * (16 * UP_RT), n0 = (wid % ncol) * (32 * UP_U);

  float y[UP_RT][UP_U][8];
  bool yok[UP_RT][UP_U];
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
    for (int u = 0; u < UP_U; ++u) {
      const int m = m0 + rt * 16 + l15, n = n0 + u * 32 + quad * 8;
      yok[rt][u] = m < M && n < N;   // N % 8 == 0
      if (ACC) {
        ld8(y[rt][u], yok[rt][u] ? Y + (size_t)m * N + n : Y);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) y[rt][u][i] = 0.f;
      }
    }
  Frag<T> tf[UP_RT][KS];
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int m = m0 + rt * 16 + l15, k = ks * 32 + quad * 8;
      ldg_frag44(tf[rt][ks], Tm + (size_t)m * r + k, m < M ? r - k : 0, Tm);
    }
#pragma unroll
  for (int u = 0; u < UP_U; ++u) {
    f32x4 acc[UP_RT][2];
#pragma unroll
    for (int rt = 0; rt < UP_RT; ++rt) acc[rt][0] = acc[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      Frag<T> bf[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = n0 + u * 32 + (l15 >> 2) * 8 + h * 4 + (l15 & 3), k = ks * 32 + quad * 8;
        ldg_frag44(bf[h], B + (size_t)n * r + k, n < N ? r - k : 0, B);
      }
#pragma unroll
      for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
        for (int h = 0; h < 2; ++h) mma16(acc[rt][h], bf[h], tf[rt][ks]);   // [column 8 quad + 4 h + i][row l15]
    }
#pragma unroll
    for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y[rt][u][i] += s * acc[rt][0][i];
        y[rt][u][4 + i] += s * acc[rt][1][i];
      }
  }
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
    for (int u = 0; u < UP_U; ++u) {
      const int m = m0 + rt * 16 + l15, n = n0 + u * 32 + quad * 8;
      if (yok[rt][u]) st8(Y + (size_t)m * N + n, y[rt][u]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// D[r, C] (+)= s P[M, r]^T Q[M, C]: the reduction runs over rows, the slow dimension of both operands.  A wave owns
// 16 chunks of columns of Q (128 bf16 / 64 fp32) and a slab of rows.  Per 32 rows a lane loads 8 rows x one chunk of Q
// (16 lanes side by side: 256 contiguous bytes per row) and transposes the 8 x EPV block in registers (Blk, common.hpp):
// column c of the block is the fragment of MFMA c, whose 16 output columns are therefore 16 l + c.  P's fragments are 8
// strided scalars per lane (P is M x r: small next to Q, and shared by every column group through L2).  The slab's
// partial [r, 128] goes to the fp32 workspace with 16-byte stores; lora_wgrad_reduce_kernel sums the slabs in order.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T> struct QBlk;
template <> struct QBlk<bf16> {
  Blk<bf16> b;
  __device__ __forceinline__ void load(int j, const bf16* p, bool ok) { b.load_row_sel(j, p, ok); }
  __device__ __forceinline__ void frag(Frag<bf16>& f, int c) const {
    uint4 u = b.col(c);
    f.v = *reinterpret_cast<bf16x8*>(&u);
  }
};
template <> struct QBlk<float> {
  Blk<float> a, b;
  __device__ __forceinline__ void load(int j, const float* p, bool ok) {
    if (j < 4) a.load_row_sel(j, p, ok); else b.load_row_sel(j - 4, p, ok);
  }
  __device__ __forceinline__ void frag(Frag<float>& f, int c) const {
    uint4 u = a.col(c), v = b.col(c);
    f.lo = *reinterpret_cast<f32x4*>(&u);
    f.hi = *reinterpret_cast<f32x4*>(&v);
  }
};

template <typename T, int NT>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const T* __restrict__ P, const T* __restrict__ Q, float* __restrict__ ws,
                                                         int M, int r, int C, int rows_per_split, int ngroups, int ntiles) {
  constexpr int EPV = Tr<T>::EPV;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int wid = blockIdx.x * 4 + w;
  if (wid >= ntiles) return;   // wave-uniform; no barrier below
  const int sp = wid / ngroups;
  const int c0 = (wid % ngroups) * (16 * EPV) + l15 * EPV;
  const bool cok = c0 < C;     // C % 8 == 0
  const int mb = sp * rows_per_split;
  const int me = mb + rows_per_split < M ? mb + rows_per_split : M;
  f32x4 acc[NT][EPV];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < EPV; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m = mb; m < me; m += 32) {
    QBlk<T> qb;
    T pe[NT][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int mm = m + quad * 8 + j;
      const bool ok = cok && mm < me;
      qb.load(j, ok ? Q + (size_t)mm * C + c0 : Q, ok);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int mm = m + quad * 8 + j, n = t * 16 + l15;
        const bool ok = mm < me && n < r;
        const T v = *(ok ? P + (size_t)mm * r + n : P);
        pe[t][j] = ok ? v : (T)0.f;
      }
    Frag<T> pf[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) frag_of(pf[t], pe[t]);
#pragma unroll
    for (int c = 0; c < EPV; ++c) {
      Frag<T> qf;
      qb.frag(qf, c);
#pragma unroll
      for (int t = 0; t < NT; ++t) mma16(acc[t][c], pf[t], qf);   // [rank 16 t + 4 quad + i][column c0 + c]
    }
  }
  if (!cok) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = t * 16 + quad * 4 + i;
      if (n < r) {
        float* o = ws + ((size_t)sp * r + n) * C + c0;
#pragma unroll
        for (int c = 0; c < EPV; c += 4)
          *reinterpret_cast<f32x4*>(o + c) = f32x4{acc[t][c][i], acc[t][c + 1][i], acc[t][c + 2][i], acc[t][c + 3][i]};
      }
    }
}

__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ D, size_t n4,
                                                                int nsplit, float s, int accumulate) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4* w4 = reinterpret_cast<const f32x4*>(ws);
  f32x4* d4 = reinterpret_cast<f32x4*>(D);
  f32x4 base = {0.f, 0.f, 0.f, 0.f};
  if (accumulate) base = d4[i];
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < nsplit; ++sp) sum += w4[(size_t)sp * n4 + i];   // fixed order
  d4[i] = base + s * sum;
}

inline bool lora_rank_ok(int r) { return r >= 4 && r <= 64 && r % 4 == 0; }

// rows per slab of the weight-gradient split: at least 128 (four k-steps per wave), doubled until the launch is at most
// 4096 waves and 256 slabs (the workspace stays a fraction of the operands)
inline void lora_wgrad_split(int M, int C, int dtype, int* rows_per_split, int* nsplit, int* ngroups) {
  const int cw = 16 * (dtype == DT_F32 ? 4 : 8);
  const int groups = (C + cw - 1) / cw;
  int rps = 128;
  while ((long long)((M + rps - 1) / rps) * groups > 4096 || (M + rps - 1) / rps > 256) rps *= 2;
  *rows_per_split = rps;
  *nsplit = (M + rps - 1) / rps;
  *ngroups = groups;
}

// =====================================================================================================================
// The same three products for a 3x3 (stride 1, padding 1) adapter on an NHWC activation [N, H, W, C]:
//   y = conv3x3(x, W) + b + s B conv3x3(x, A),   A [r, Cin, 3, 3] (the 3x3 sits on the down-projection), B [Cout, r]
//   lora_down_conv3x3_kernel     T[M, r]     = sum_tap X[m + shift(tap)][C] A[:, tap, :]^T        a packed [r][9][C]
//   lora_up_add_conv3x3_kernel   Y[M, N] (+)= s sum_tap T[m + shift(tap)][r] B[:, tap, :]^T      b packed [N][9][r]
//   lora_wgrad_conv3x3_kernel    D[r][9][C] (+)= s sum_m P[m][r]^T Q[m + shift(tap)][C]          + the reduce kernel above
// with M = N H W rows, tap = 3 ky + kx and shift(tap) = (ky - 1) W + (kx - 1) rows.  A pixel's position in its own image
// is (y, x) = ((m / W) % H, m % W); a tap whose (y + ky - 1, x + kx - 1) lies outside [0, H) x [0, W) contributes zeros --
// that one test covers the image's four borders AND the neighbouring images of the batch, and whenever it passes the
// shifted row lies in the same image, hence inside the buffer.  Where it fails the lane reads `safe` (the buffer's first
// element) and selects zeros: branch-free, and no out-of-range address is formed into a load.  The shifted rows are
// re-read through L2 (a row is used by 9 taps of 3 neighbouring rows: the working set of a block is 3 image rows) rather
// than staged as a halo in LDS: the kernels have a few MFMAs per byte and no reuse inside a block beyond those 9 taps.
// =====================================================================================================================

// the two 4-element halves of a fragment from two addresses of their own (each n-th of a 32-deep step may belong to
// another tap, hence another row); !ok -> zeros, read from `safe`
__device__ __forceinline__ void ldg_frag4x2(Frag<bf16>& f, const bf16* p0, bool ok0, const bf16* p1, bool ok1, const bf16* safe) {
  const u32x2 a = *reinterpret_cast<const u32x2*>(ok0 ? p0 : safe), b = *reinterpret_cast<const u32x2*>(ok1 ? p1 : safe);
  uint4 u = uint4{ok0 ? a.x : 0u, ok0 ? a.y : 0u, ok1 ? b.x : 0u, ok1 ? b.y : 0u};
  f.v = *reinterpret_cast<bf16x8*>(&u);
}
__device__ __forceinline__ void ldg_frag4x2(Frag<float>& f, const float* p0, bool ok0, const float* p1, bool ok1, const float* safe) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(ok0 ? p0 : safe), b = *reinterpret_cast<const f32x4*>(ok1 ? p1 : safe);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f.lo = ok0 ? a : z;
  f.hi = ok1 ? b : z;
}

// Blocks b and b + 8 share an XCD and its L2 (observed dealing, for speed only): the blocks of one XCD get a contiguous range
// of tiles, so that the rows a tile re-reads from its neighbours (+-(W + 1) rows) sit in the L2 that fetched them.
// Bijective for any number of blocks n.
__device__ __forceinline__ int xcd_tile(int b, int n) {
  const int q = n >> 3, rem = n & 7, x = b & 7;
  return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + (b >> 3);
}

// T[M, r] = sum_tap X[m + shift(tap)] A[:, tap, :]^T: lora_down_kernel with the k-steps running over 9 x ceil(C / 32)
// (tap-major), dealt to the four waves in turn.  X comes from HBM once and 8 more times from L2; A [r][9][C] per block
// through L2.
template <typename T, int NT>
__global__ __launch_bounds__(256) void lora_down_conv3x3_kernel(const T* __restrict__ X, const T* __restrict__ A, T* __restrict__ Tout,
                                                                int M, int H, int W, int C, int r) {
  __shared__ f32x4 part[4][DOWN_RT * NT][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int m0 = xcd_tile(blockIdx.x, gridDim.x) * (16 * DOWN_RT);
  int px[DOWN_RT], py[DOWN_RT];
#pragma unroll
  for (int rt = 0; rt < DOWN_RT; ++rt) {
    const int m = m0 + rt * 16 + l15;
    px[rt] = m % W;
    py[rt] = (m / W) % H;
  }
  f32x4 acc[DOWN_RT][NT];
#pragma unroll
  for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kpt = (C + 31) / 32;   // k-steps per tap
  const int ksteps = 9 * kpt;
  for (int ks = w; ks < ksteps; ks += 4) {
    const int tap = ks / kpt;
    const int k = (ks - tap * kpt) * 32 + quad * 8;
    const int ky = tap / 3, dy = ky - 1, dx = tap - 3 * ky - 1;
    const bool kok = k < C;   // C % 8 == 0: a chunk is inside or outside as a whole
    Frag<T> xf[DOWN_RT], af[NT];
#pragma unroll
    for (int rt = 0; rt < DOWN_RT; ++rt) {
      const int m = m0 + rt * 16 + l15;
      const bool ok = kok && m < M && (unsigned)(py[rt] + dy) < (unsigned)H && (unsigned)(px[rt] + dx) < (unsigned)W;
      const size_t row = ok ? (size_t)(m + dy * W + dx) : 0;
      ldg_frag8(xf[rt], X + row * C + k, ok, X);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 16 + l15;
      ldg_frag8(af[t], A + ((size_t)n * 9 + tap) * C + k, kok && n < r, A);
    }
#pragma unroll
    for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
      for (int t = 0; t < NT; ++t) mma16(acc[rt][t], af[t], xf[rt]);   // [rank n][row m]
  }
#pragma unroll
  for (int rt = 0; rt < DOWN_RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) part[w][rt * NT + t][lane] = acc[rt][t];
  __syncthreads();
  for (int idx = threadIdx.x; idx < DOWN_RT * NT * 64; idx += 256) {
    const int tile = idx >> 6, ln = idx & 63;
    const f32x4 s = ((part[0][tile][ln] + part[1][tile][ln]) + part[2][tile][ln]) + part[3][tile][ln];
    const int m = m0 + (tile / NT) * 16 + (ln & 15);
    const int n = (tile % NT) * 16 + (ln >> 4) * 4;
    if (m < M && n < r) st4(Tout + (size_t)m * r + n, s);
  }
}

// Y[M, N] (+)= s sum_tap T[m + shift(tap)] B[:, tap, :]^T.  The reduction index is k = tap r + j, 9 r long and
// contiguous in the packed B [N][9][r]; it is cut into 32-deep MFMA steps WITHOUT padding each tap: a lane's fragment is
// two runs of 4 (r % 4 == 0: a run never straddles two taps), each with the tap, hence the shifted row of T, of its own.
// r = 4 takes 2 steps (36 of 64 slots used), not 9.  The wave tile is lora_up_add_kernel's (32 rows x 128 columns, the
// same dealing of B's rows so that a lane owns 8 consecutive columns); the k-steps are a loop of loads and MFMAs only,
// and Y is read (ACC), added to and stored once behind it.
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void lora_up_add_conv3x3_kernel(T* __restrict__ Y, const T* __restrict__ Tm, const T* __restrict__ B,
                                                                  int M, int H, int W, int N, int r, float s, int ncol, int ntiles) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int wid = xcd_tile(blockIdx.x, gridDim.x) * 4 + w;
  if (wid >= ntiles) return;   // wave-uniform; the kernel has no barrier
  const int m0 = (wid / ncol) * (16 * UP_RT), n0 = (wid % ncol) * (32 * UP_U);
  int px[UP_RT], py[UP_RT];
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt) {
    const int m = m0 + rt * 16 + l15;
    px[rt] = m % W;
    py[rt] = (m / W) % H;
  }
  f32x4 acc[UP_RT][UP_U][2];
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
    for (int u = 0; u < UP_U; ++u) acc[rt][u][0] = acc[rt][u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int rpt = r >> 2;       // runs of 4 per tap
  const int K = 9 * r;
  const int ksteps = (K + 31) / 32;
  for (int ks = 0; ks < ksteps; ++ks) {
    const int k = ks * 32 + quad * 8;
    const T* tp[2];
    int tdy[2], tdx[2];
    bool tin[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int run = (k >> 2) + h;
      tin[h] = run < 9 * rpt;
      const int tap = tin[h] ? run / rpt : 0;
      const int ky = tap / 3;
      tdy[h] = ky - 1;
      tdx[h] = tap - 3 * ky - 1;
      tp[h] = Tm + (run - tap * rpt) * 4;
    }
    Frag<T> tf[UP_RT];
#pragma unroll
    for (int rt = 0; rt < UP_RT; ++rt) {
      const int m = m0 + rt * 16 + l15;
      bool ok[2];
      size_t row[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ok[h] = tin[h] && m < M && (unsigned)(py[rt] + tdy[h]) < (unsigned)H && (unsigned)(px[rt] + tdx[h]) < (unsigned)W;
        row[h] = ok[h] ? (size_t)(m + tdy[h] * W + tdx[h]) : 0;
      }
      ldg_frag4x2(tf[rt], tp[0] + row[0] * r, ok[0], tp[1] + row[1] * r, ok[1], Tm);
    }
#pragma unroll
    for (int u = 0; u < UP_U; ++u) {
      if (n0 + u * 32 >= N) continue;   // wave-uniform: a column group past N has nothing to form
      Frag<T> bf[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = n0 + u * 32 + (l15 >> 2) * 8 + h * 4 + (l15 & 3);
        ldg_frag44(bf[h], B + (size_t)n * K + k, n < N ? K - k : 0, B);
      }
#pragma unroll
      for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
        for (int h = 0; h < 2; ++h) mma16(acc[rt][u][h], bf[h], tf[rt]);   // [column 8 quad + 4 h + i][row l15]
    }
  }
#pragma unroll
  for (int rt = 0; rt < UP_RT; ++rt)
#pragma unroll
    for (int u = 0; u < UP_U; ++u) {
      const int m = m0 + rt * 16 + l15, n = n0 + u * 32 + quad * 8;
      const bool yok = m < M && n < N;   // N % 8 == 0
      float y[8];
      if (ACC) {
        ld8(y, yok ? Y + (size_t)m * N + n : Y);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y[i] += s * acc[rt][u][0][i];
        y[4 + i] += s * acc[rt][u][1][i];
      }
      if (yok) st8(Y + (size_t)m * N + n, y);
    }
}

// D[r][9][C] (+)= s sum_m P[m]^T Q[m + shift(tap)]: lora_wgrad_kernel with the tap as one more dimension of the grid.  A
// wave owns a slab of rows, one tap and 16 chunks of columns; the 9 waves of a (slab, column group) sit side by side in
// the grid and read the same rows of Q, shifted by at most W + 1 rows: Q comes from HBM once and from L2 for the rest.
// (y, x) of the lane's first row takes two divisions per 32 rows; the 7 rows behind it are counted up.
template <typename T, int NT>
__global__ __launch_bounds__(256) void lora_wgrad_conv3x3_kernel(const T* __restrict__ P, const T* __restrict__ Q, float* __restrict__ ws,
                                                                 int M, int H, int W, int r, int C, int rows_per_split, int ngroups,
                                                                 int ntiles) {
  constexpr int EPV = Tr<T>::EPV;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int wid = xcd_tile(blockIdx.x, gridDim.x) * 4 + w;
  if (wid >= ntiles) return;   // wave-uniform; no barrier below
  const int sp = wid / (9 * ngroups), rem = wid - sp * (9 * ngroups);
  const int tap = rem % 9;
  const int c0 = (rem / 9) * (16 * EPV) + l15 * EPV;
  const bool cok = c0 < C;     // C % 8 == 0
  const int ky = tap / 3, dy = ky - 1, dx = tap - 3 * ky - 1;
  const int mb = sp * rows_per_split;
  const int me = mb + rows_per_split < M ? mb + rows_per_split : M;
  f32x4 acc[NT][EPV];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < EPV; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m = mb; m < me; m += 32) {
    QBlk<T> qb;
    T pe[NT][8];
    int x = (m + quad * 8) % W, y = ((m + quad * 8) / W) % H;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int mm = m + quad * 8 + j;
      const bool ok = cok && mm < me && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
      qb.load(j, ok ? Q + (size_t)(mm + dy * W + dx) * C + c0 : Q, ok);
      if (++x == W) {
        x = 0;
        if (++y == H) y = 0;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int mm = m + quad * 8 + j, n = t * 16 + l15;
        const bool ok = mm < me && n < r;
        const T v = *(ok ? P + (size_t)mm * r + n : P);
        pe[t][j] = ok ? v : (T)0.f;
      }
    Frag<T> pf[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) frag_of(pf[t], pe[t]);
#pragma unroll
    for (int c = 0; c < EPV; ++c) {
      Frag<T> qf;
      qb.frag(qf, c);
#pragma unroll
      for (int t = 0; t < NT; ++t) mma16(acc[t][c], pf[t], qf);   // [rank 16 t + 4 quad + i][column c0 + c]
    }
  }
  if (!cok) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = t * 16 + quad * 4 + i;
      if (n < r) {
        float* o = ws + (((size_t)sp * r + n) * 9 + tap) * C + c0;
#pragma unroll
        for (int c = 0; c < EPV; c += 4)
          *reinterpret_cast<f32x4*>(o + c) = f32x4{acc[t][c][i], acc[t][c + 1][i], acc[t][c + 2][i], acc[t][c + 3][i]};
      }
    }
}

// the 3x3 form's split: the same rule with 9 waves (one per tap) for every (slab, column group)
inline void lora_wgrad_conv3x3_split(int M, int C, int dtype, int* rows_per_split, int* nsplit, int* ngroups) {
  const int cw = 16 * (dtype == DT_F32 ? 4 : 8);
  const int groups = (C + cw - 1) / cw;
  int rps = 128;
  while ((long long)((M + rps - 1) / rps) * groups * 9 > 4096 || (M + rps - 1) / rps > 256) rps *= 2;
  *rows_per_split = rps;
  *nsplit = (M + rps - 1) / rps;
  *ngroups = groups;
}

// N H W rows of an NHWC activation as an int (the kernels index rows with 32 bits), or 0 if the geometry is not valid
inline int lora_conv_rows(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const long long m = (long long)N * H * W;
  return m < (1ll << 30) ? (int)m : 0;   // row + shift and 32-row tile arithmetic stay far inside int
}

}  // namespace
}  // namespace mdm

using namespace mdm;

extern "C" int mdm_lora_down(const void* x, const void* a, void* t, int M, int C, int r, int dtype, void* stream) {
  MDM_CHECK_ARG(x && a && t);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((M + 16 * DOWN_RT - 1) / (16 * DOWN_RT));
  const int nt = (r + 15) / 16;
#define MDM_LORA_DOWN(TT, NT) \
  hipLaunchKernelGGL((lora_down_kernel<TT, NT>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)a, (TT*)t, M, C, r)
  if (dtype == DT_F32) {
    if (nt == 1) MDM_LORA_DOWN(float, 1); else if (nt == 2) MDM_LORA_DOWN(float, 2); else MDM_LORA_DOWN(float, 4);
  } else {
    if (nt == 1) MDM_LORA_DOWN(bf16, 1); else if (nt == 2) MDM_LORA_DOWN(bf16, 2); else MDM_LORA_DOWN(bf16, 4);
  }
#undef MDM_LORA_DOWN
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_lora_up_add(void* y, const void* t, const void* b, int M, int N, int r, float s, int accumulate, int dtype,
                               void* stream) {
  MDM_CHECK_ARG(y && t && b);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(M >= 1 && N >= 8 && N % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int ncol = (N + 32 * UP_U - 1) / (32 * UP_U);
  const long long tiles = (long long)((M + 16 * UP_RT - 1) / (16 * UP_RT)) * ncol;
  MDM_CHECK_ARG(tiles < (1ll << 31));
  const int ntiles = (int)tiles;
  const dim3 grid((ntiles + 3) / 4);
#define MDM_LORA_UP(TT, KS, ACC)                                                                                     \
  hipLaunchKernelGGL((lora_up_add_kernel<TT, KS, ACC>), grid, dim3(256), 0, st, (TT*)y, (const TT*)t, (const TT*)b, M, N, r, \
                     s, ncol, ntiles)
#define MDM_LORA_UP_T(TT)                                                        \
  do {                                                                           \
    if (r <= 32) { if (accumulate) MDM_LORA_UP(TT, 1, true); else MDM_LORA_UP(TT, 1, false); } \
    else { if (accumulate) MDM_LORA_UP(TT, 2, true); else MDM_LORA_UP(TT, 2, false); }         \
  } while (0)
  if (dtype == DT_F32) MDM_LORA_UP_T(float); else MDM_LORA_UP_T(bf16);
#undef MDM_LORA_UP_T
#undef MDM_LORA_UP
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_lora_wgrad_plan(int M, int r, int C, int dtype, int* splits_out, size_t* ws_bytes) {
  MDM_CHECK_ARG(splits_out && ws_bytes);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  int rps, nsplit, groups;
  lora_wgrad_split(M, C, dtype, &rps, &nsplit, &groups);
  *splits_out = nsplit;
  *ws_bytes = (size_t)nsplit * r * C * sizeof(float);
  return 0;
}

extern "C" int mdm_lora_wgrad(const void* p, const void* q, float* d, float* ws, int M, int r, int C, float s, int accumulate,
                              int dtype, void* stream) {
  MDM_CHECK_ARG(p && q && d && ws);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rps, nsplit, groups;
  lora_wgrad_split(M, C, dtype, &rps, &nsplit, &groups);
  const int ntiles = nsplit * groups;
  const dim3 grid((ntiles + 3) / 4);
  const int nt = (r + 15) / 16;
#define MDM_LORA_WG(TT, NT)                                                                                          \
  hipLaunchKernelGGL((lora_wgrad_kernel<TT, NT>), grid, dim3(256), 0, st, (const TT*)p, (const TT*)q, ws, M, r, C, rps, groups, \
                     ntiles)
  if (dtype == DT_F32) {
    if (nt == 1) MDM_LORA_WG(float, 1); else if (nt == 2) MDM_LORA_WG(float, 2); else MDM_LORA_WG(float, 4);
  } else {
    if (nt == 1) MDM_LORA_WG(bf16, 1); else if (nt == 2) MDM_LORA_WG(bf16, 2); else MDM_LORA_WG(bf16, 4);
  }
#undef MDM_LORA_WG
  const size_t n4 = (size_t)r * C / 4;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, d, n4, nsplit, s, accumulate);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_lora_down_conv3x3(const void* x, const void* a, void* t, int N, int H, int W, int C, int r, int dtype,
                                     void* stream) {
  MDM_CHECK_ARG(x && a && t);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int M = lora_conv_rows(N, H, W);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((M + 16 * DOWN_RT - 1) / (16 * DOWN_RT));
  const int nt = (r + 15) / 16;
#define MDM_LORA_DOWN3(TT, NT) \
  hipLaunchKernelGGL((lora_down_conv3x3_kernel<TT, NT>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)a, (TT*)t, M, H, W, C, r)
  if (dtype == DT_F32) {
    if (nt == 1) MDM_LORA_DOWN3(float, 1); else if (nt == 2) MDM_LORA_DOWN3(float, 2); else MDM_LORA_DOWN3(float, 4);
  } else {
    if (nt == 1) MDM_LORA_DOWN3(bf16, 1); else if (nt == 2) MDM_LORA_DOWN3(bf16, 2); else MDM_LORA_DOWN3(bf16, 4);
  }
#undef MDM_LORA_DOWN3
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_lora_up_add_conv3x3(void* y, const void* t, const void* b, int N, int H, int W, int Cout, int r, float s,
                                       int accumulate, int dtype, void* stream) {
  MDM_CHECK_ARG(y && t && b);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int M = lora_conv_rows(N, H, W);
  MDM_CHECK_ARG(M >= 1 && Cout >= 8 && Cout % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int ncol = (Cout + 32 * UP_U - 1) / (32 * UP_U);
  const long long tiles = (long long)((M + 16 * UP_RT - 1) / (16 * UP_RT)) * ncol;
  MDM_CHECK_ARG(tiles < (1ll << 31));
  const int ntiles = (int)tiles;
  const dim3 grid((ntiles + 3) / 4);
#define MDM_LORA_UP3(TT, ACC)                                                                                          \
  hipLaunchKernelGGL((lora_up_add_conv3x3_kernel<TT, ACC>), grid, dim3(256), 0, st, (TT*)y, (const TT*)t, (const TT*)b, M, H, \
                     W, Cout, r, s, ncol, ntiles)
  if (dtype == DT_F32) {
    if (accumulate) MDM_LORA_UP3(float, true); else MDM_LORA_UP3(float, false);
  } else {
    if (accumulate) MDM_LORA_UP3(bf16, true); else MDM_LORA_UP3(bf16, false);
  }
#undef MDM_LORA_UP3
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_lora_wgrad_conv3x3_plan(int N, int H, int W, int r, int C, int dtype, int* splits_out, size_t* ws_bytes) {
  MDM_CHECK_ARG(splits_out && ws_bytes);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int M = lora_conv_rows(N, H, W);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  int rps, nsplit, groups;
  lora_wgrad_conv3x3_split(M, C, dtype, &rps, &nsplit, &groups);
  *splits_out = nsplit;
  *ws_bytes = (size_t)nsplit * r * 9 * C * sizeof(float);
  return 0;
}

extern "C" int mdm_lora_wgrad_conv3x3(const void* p, const void* q, float* d, float* ws, int N, int H, int W, int r, int C,
                                      float s, int accumulate, int dtype, void* stream) {
  MDM_CHECK_ARG(p && q && d && ws);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int M = lora_conv_rows(N, H, W);
  MDM_CHECK_ARG(M >= 1 && C >= 8 && C % 8 == 0);
  MDM_CHECK_ARG(lora_rank_ok(r));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rps, nsplit, groups;
  lora_wgrad_conv3x3_split(M, C, dtype, &rps, &nsplit, &groups);
  const int ntiles = nsplit * groups * 9;
  const dim3 grid((ntiles + 3) / 4);
  const int nt = (r + 15) / 16;
#define MDM_LORA_WG3(TT, NT)                                                                                           \
  hipLaunchKernelGGL((lora_wgrad_conv3x3_kernel<TT, NT>), grid, dim3(256), 0, st, (const TT*)p, (const TT*)q, ws, M, H, W, r, \
                     C, rps, groups, ntiles)
  if (dtype == DT_F32) {
    if (nt == 1) MDM_LORA_WG3(float, 1); else if (nt == 2) MDM_LORA_WG3(float, 2); else MDM_LORA_WG3(float, 4);
  } else {
    if (nt == 1) MDM_LORA_WG3(bf16, 1); else if (nt == 2) MDM_LORA_WG3(bf16, 2); else MDM_LORA_WG3(bf16, 4);
  }
#undef MDM_LORA_WG3
  const size_t n4 = (size_t)r * 9 * C / 4;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, d, n4, nsplit, s, accumulate);
  MDM_LAUNCH_STATUS();
}
