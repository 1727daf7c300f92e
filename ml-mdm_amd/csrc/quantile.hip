// The per-sample threshold of the dynamic threshold functions (Imagen: ratio 0.995, cap 100; DeepFloyd IF: 0.95, 1.5):
// thr[b] = clamp(quantile_q |x[b, :]|, cmin, cmax), the quantile by torch.quantile's rule (linear interpolation between the
// order statistics a[lo], a[hi] around the fp32 rank q (n - 1)), found EXACTLY by a radix select instead of a sort.
//   key = bits(x) & 0x7fffffff: unsigned order on the key is value order on |x| (-0.0 is 0, inf above every finite value,
//   the NaN patterns above inf).  The 31 key bits are refined over three levels, 12 + 11 + 8 bits:
//     level 1   histogram of key >> 19 over every element                                   (4096 bins)
//     level 2   histogram of (key >> 8) & 0x7ff over the elements whose 12-bit prefix holds the rank  (2048 bins)
//     level 3   histogram of key & 0xff over the elements whose 23-bit prefix holds the rank          (256 bins)
//   Both ranks lo and hi are carried through the levels, each with a prefix and a histogram of its own from level 2 on: where
//   they fall into the same bin (almost always) the second histogram stays empty, where they do not -- a[hi] the smallest
//   key of another level-one bin -- it is what finds a[hi].
// Five launches: zero the row histograms; one grid-stride pass over x per level, a block-private LDS histogram merged into
// the row's histogram in the workspace with integer atomics (non-empty bins only); the finish, one block per row.  The blocks
// of levels 2 and 3 each find the prefix for themselves from the histogram of the level before (block 0 of the row leaves
// prefix and residual rank in the workspace for the next launch).  Integer counts do not depend on arrival order and the
// selection is exact: a row's result depends on nothing but the row, and two runs are bit-identical.  No float atomics.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"
#include "../../include/mdm_hip_dev.h"

#include <math.h>

namespace mdm {

constexpr int AQ_T = 256;
constexpr int AQ_B1 = 4096, AQ_B2 = 2048, AQ_B3 = 256;   // bins per level: 12 + 11 + 8 = 31 key bits
constexpr int AQ_S1 = 19, AQ_S2 = 8;                      // key >> AQ_S1: level-1 bin; key >> AQ_S2: the 23-bit prefix
// level 1 counts every element, and neighbouring pixels share a bin: each lane adds runs of equal bins among its four
// elements as one add, and odd and even lanes keep histograms of their own (interleaved: different LDS banks)
constexpr int AQ_COPIES = 2;
constexpr size_t AQ_BLOCK_ELEMS = 16384;                  // elements of a row per block at least (64 per thread)
constexpr int AQ_MAX_BLOCKS = 2048;                       // over all rows
constexpr int AQ_MAX_ROW_BLOCKS = 512;                    // of one row: every block adds its bins to the same row histogram
// a row's workspace in 32-bit words: level-1 histogram, two level-2 and two level-3 histograms (rank lo, rank hi), state
constexpr int AQ_H1 = 0, AQ_H2 = AQ_H1 + AQ_B1, AQ_H3 = AQ_H2 + 2 * AQ_B2, AQ_ST = AQ_H3 + 2 * AQ_B3, AQ_ROW = AQ_ST + 16;
enum { ST_NAN = 0, ST_P1A, ST_R1A, ST_P1B, ST_R1B, ST_P2A, ST_R2A, ST_P2B, ST_R2B };
constexpr unsigned AQ_INF = 0x7f800000u;
static_assert(AQ_ROW % 4 == 0 && AQ_H2 % 4 == 0 && AQ_H3 % 4 == 0, "the histograms are read 16 bytes at a time");

__device__ __forceinline__ unsigned aq_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// f(const unsigned (&key)[W]) over the block's share of the row: W = 4 elements per 16-byte load (VEC: n % 4 == 0 and an
// aligned row) or 1; four loads in flight per thread
template <bool VEC, typename F>
__device__ __forceinline__ void aq_for_keys(const float* __restrict__ row, size_t n, F&& f) {
  constexpr int W = VEC ? 4 : 1;
  const size_t cnt = VEC ? n / 4 : n, stride = (size_t)gridDim.x * AQ_T;
  size_t i = (size_t)blockIdx.x * AQ_T + threadIdx.x;
  auto load = [&](size_t j, unsigned (&k)[W]) {
    if constexpr (VEC) {
      const f32x4 v = reinterpret_cast<const f32x4*>(row)[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = aq_key(v[e]);
    } else {
      k[0] = aq_key(row[j]);
    }
  };
  for (; i + 3 * stride < cnt; i += 4 * stride) {
    unsigned k[4][W];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(i + u * stride, k[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) f(k[u]);
  }
  for (; i < cnt; i += stride) {
    unsigned k[W];
    load(i, k);
    f(k);
  }
}

// h[bin] += 1 for every lane with `on`; where 16 lanes or more are on and all of them name the same bin (a flat image
// region, a row of ties) one lane adds their number instead of up to 64 adds to one LDS word
__device__ __forceinline__ void aq_wave_add(unsigned* h, unsigned bin, bool on) {
  const unsigned long long m = __ballot(on);
  if (m == 0ull) return;
  if (__popcll(m) < 16) {   // a few scattered matches, the usual case: not worth the exchange below
    if (on) atomicAdd(&h[bin], 1u);
    return;
  }
  const int leader = __ffsll((long long)m) - 1;
  const unsigned b0 = (unsigned)__shfl((int)bin, leader, 64);
  if (__ballot(on && bin == b0) == m) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[b0], (unsigned)__popcll(m));
  } else if (on) {
    atomicAdd(&h[bin], 1u);
  }
}

// the bins of a row histogram (NB counts, 16-byte aligned) that hold ranks r0 and r1 (0-based, in ascending key order), and
// the ranks within them.  Every thread of the block calls; sh: 8 words of LDS.  A rank past the histogram's total: bin 0.
struct AqSel {
  unsigned bin[2], res[2];
};
template <int NB>
__device__ __forceinline__ AqSel aq_select(const unsigned* __restrict__ hist, unsigned r0, unsigned r1, unsigned* sh) {
  constexpr int PER = NB / AQ_T;
  static_assert(PER == 1 || PER % 4 == 0, "bins per thread");
  unsigned c[PER];
  if constexpr (PER == 1) {
    c[0] = hist[threadIdx.x];
  } else {
#pragma unroll
    for (int j = 0; j < PER; j += 4) {
      const uint4 v = reinterpret_cast<const uint4*>(hist)[(threadIdx.x * PER + j) / 4];
      c[j] = v.x; c[j + 1] = v.y; c[j + 2] = v.z; c[j + 3] = v.w;
    }
  }
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) s += c[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();   // sh may still be read from the call before
  if (lane == 63) sh[wave] = inc;
  if (threadIdx.x < 4) sh[4 + threadIdx.x] = 0u;
  __syncthreads();
  unsigned ex = inc - s;
  for (int w = 0; w < wave; ++w) ex += sh[w];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const unsigned r = q ? r1 : r0;
    if (r >= ex && r - ex < s) {   // exactly one thread
      unsigned a = r - ex;
      bool found = false;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (!found) {
          if (a < c[j]) {
            sh[4 + 2 * q] = (unsigned)(threadIdx.x * PER + j);
            sh[5 + 2 * q] = a;
            found = true;
          } else {
            a -= c[j];
          }
        }
      }
    }
  }
  __syncthreads();
  AqSel o;
  o.bin[0] = sh[4]; o.res[0] = sh[5]; o.bin[1] = sh[6]; o.res[1] = sh[7];
  return o;
}

// h (LDS) -> the row histogram, non-empty bins only
__device__ __forceinline__ void aq_merge(const unsigned* h, unsigned* __restrict__ g, int nb) {
  for (int i = threadIdx.x; i < nb; i += AQ_T) {
    const unsigned c = h[i];
    if (c) atomicAdd(&g[i], c);
  }
}

// grid (AQ_ROW / 4 / AQ_T rounded up, B)
__global__ __launch_bounds__(AQ_T) void aq_zero_kernel(unsigned* __restrict__ ws) {
  const int i = blockIdx.x * AQ_T + threadIdx.x;
  if (i < AQ_ROW / 4) reinterpret_cast<uint4*>(ws + (size_t)blockIdx.y * AQ_ROW)[i] = uint4{0u, 0u, 0u, 0u};
}

// grid (blocks per row, B) for the three passes
template <bool VEC>
__global__ __launch_bounds__(AQ_T) void aq_level1_kernel(const float* __restrict__ x, unsigned* __restrict__ ws, size_t n) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ unsigned h[AQ_B1 * AQ_COPIES];
  const float* row = x + (size_t)blockIdx.y * n;
  unsigned* wr = ws + (size_t)blockIdx.y * AQ_ROW;
  for (int i = threadIdx.x; i < AQ_B1 * AQ_COPIES; i += AQ_T) h[i] = 0u;
  __syncthreads();
  const unsigned cp = threadIdx.x & (AQ_COPIES - 1);
  bool nan = false;
  aq_for_keys<VEC>(row, n, [&](const unsigned (&k)[W]) {
    unsigned cur = k[0] >> AQ_S1, c = 1u;
    nan |= k[0] > AQ_INF;
#pragma unroll
    for (int e = 1; e < W; ++e) {
      const unsigned b = k[e] >> AQ_S1;
      nan |= k[e] > AQ_INF;
      if (b == cur) {
        ++c;
      } else {
        atomicAdd(&h[cur * AQ_COPIES + cp], c);
        cur = b;
        c = 1u;
      }
    }
    atomicAdd(&h[cur * AQ_COPIES + cp], c);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < AQ_B1; i += AQ_T) {
    unsigned c = 0u;
#pragma unroll
    for (int j = 0; j < AQ_COPIES; ++j) c += h[i * AQ_COPIES + j];
    if (c) atomicAdd(&wr[AQ_H1 + i], c);
  }
  if (__any(nan) && (threadIdx.x & 63) == 0) atomicOr(&wr[AQ_ST + ST_NAN], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(AQ_T) void aq_level2_kernel(const float* __restrict__ x, unsigned* __restrict__ ws, size_t n,
                                                         unsigned lo, unsigned hi) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ unsigned h[2 * AQ_B2];
  __shared__ unsigned sh[8];
  const float* row = x + (size_t)blockIdx.y * n;
  unsigned* wr = ws + (size_t)blockIdx.y * AQ_ROW;
  for (int i = threadIdx.x; i < 2 * AQ_B2; i += AQ_T) h[i] = 0u;
  const AqSel s = aq_select<AQ_B1>(wr + AQ_H1, lo, hi, sh);   // (its barriers publish the zeroes)
  const unsigned pa = s.bin[0], pb = s.bin[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    wr[AQ_ST + ST_P1A] = pa; wr[AQ_ST + ST_R1A] = s.res[0];
    wr[AQ_ST + ST_P1B] = pb; wr[AQ_ST + ST_R1B] = s.res[1];
  }
  aq_for_keys<VEC>(row, n, [&](const unsigned (&k)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const unsigned p = k[e] >> AQ_S1, bin = (k[e] >> AQ_S2) & (AQ_B2 - 1);
      aq_wave_add(h, p == pa ? bin : bin + AQ_B2, p == pa || p == pb);
    }
  });
  __syncthreads();
  aq_merge(h, wr + AQ_H2, 2 * AQ_B2);
}

// prefix and residual rank of both ranks after the level whose two histograms are `hist`, `hist + NB`, from those before it
template <int NB>
__device__ __forceinline__ void aq_refine(const unsigned* __restrict__ hist, unsigned& pa, unsigned& ra, unsigned& pb,
                                          unsigned& rb, int bits, unsigned* sh) {
  const bool same = pa == pb;   // block-uniform
  AqSel s = aq_select<NB>(hist, ra, same ? rb : ra, sh);
  if (!same) {
    const AqSel t = aq_select<NB>(hist + NB, rb, rb, sh);
    s.bin[1] = t.bin[0];
    s.res[1] = t.res[0];
  }
  pa = (pa << bits) | s.bin[0]; ra = s.res[0];
  pb = (pb << bits) | s.bin[1]; rb = s.res[1];
}

template <bool VEC>
__global__ __launch_bounds__(AQ_T) void aq_level3_kernel(const float* __restrict__ x, unsigned* __restrict__ ws, size_t n) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ unsigned h[2 * AQ_B3];
  __shared__ unsigned sh[8];
  const float* row = x + (size_t)blockIdx.y * n;
  unsigned* wr = ws + (size_t)blockIdx.y * AQ_ROW;
  for (int i = threadIdx.x; i < 2 * AQ_B3; i += AQ_T) h[i] = 0u;
  unsigned pa = wr[AQ_ST + ST_P1A], ra = wr[AQ_ST + ST_R1A], pb = wr[AQ_ST + ST_P1B], rb = wr[AQ_ST + ST_R1B];
  aq_refine<AQ_B2>(wr + AQ_H2, pa, ra, pb, rb, 11, sh);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    wr[AQ_ST + ST_P2A] = pa; wr[AQ_ST + ST_R2A] = ra;
    wr[AQ_ST + ST_P2B] = pb; wr[AQ_ST + ST_R2B] = rb;
  }
  aq_for_keys<VEC>(row, n, [&](const unsigned (&k)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const unsigned p = k[e] >> AQ_S2, bin = k[e] & (AQ_B3 - 1);
      aq_wave_add(h, p == pa ? bin : bin + AQ_B3, p == pa || p == pb);
    }
  });
  __syncthreads();
  aq_merge(h, wr + AQ_H3, 2 * AQ_B3);
}

// grid (B): the two order statistics, torch.lerp's two-sided form, the clamp
__global__ __launch_bounds__(AQ_T) void aq_finish_kernel(const unsigned* __restrict__ ws, float w, float cmin, float cmax,
                                                         float* __restrict__ thr, float* __restrict__ stats) {
  __shared__ unsigned sh[8];
  const unsigned* wr = ws + (size_t)blockIdx.x * AQ_ROW;
  unsigned pa = wr[AQ_ST + ST_P2A], ra = wr[AQ_ST + ST_R2A], pb = wr[AQ_ST + ST_P2B], rb = wr[AQ_ST + ST_R2B];
  aq_refine<AQ_B3>(wr + AQ_H3, pa, ra, pb, rb, 8, sh);
  if (threadIdx.x == 0) {
    const float alo = __uint_as_float(pa), ahi = __uint_as_float(pb);
    const float d = ahi - alo;
    float t = w < 0.5f ? alo + w * d : ahi - d * (1.f - w);
    if (wr[AQ_ST + ST_NAN]) t = __uint_as_float(0x7fc00000u);
    if (t < cmin) t = cmin;   // a NaN passes both
    if (t > cmax) t = cmax;
    thr[blockIdx.x] = t;
    if (stats != nullptr) {
      stats[2 * blockIdx.x] = alo;
      stats[2 * blockIdx.x + 1] = ahi;
    }
  }
}

static inline size_t aq_ws_bytes(int B) { return (size_t)B * AQ_ROW * sizeof(unsigned); }

static int aq_check_shape(int B, size_t n) {
  MDM_CHECK_ARG(B >= 1 && B <= 65535);
  MDM_CHECK_ARG(n >= 1 && n < ((size_t)1 << 31));
  return 0;
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_abs_quantile_plan(int B, size_t n, size_t* ws_bytes) {
  MDM_CHECK_ARG(ws_bytes != nullptr);
  if (aq_check_shape(B, n) != 0) return -1;
  *ws_bytes = aq_ws_bytes(B);
  return 0;
}

// stages: bit 0 the zeroing launch, bits 1 .. 3 the pass of that level, bit 4 the finish
static int aq_run(const float* x, void* ws, size_t ws_bytes, int B, size_t n, float q, float cmin, float cmax, float* thr,
                  float* stats, void* stream, unsigned stages) {
  MDM_CHECK_ARG(x != nullptr);
  MDM_CHECK_ARG(ws != nullptr);
  MDM_CHECK_ARG(thr != nullptr || !(stages & 16u));
  if (aq_check_shape(B, n) != 0) return -1;
  MDM_CHECK_ARG(q >= 0.f && q <= 1.f);   // NaN fails
  MDM_CHECK_ARG(cmin <= cmax);           // NaN fails; -inf / +inf: no clamp
  MDM_CHECK_ARG(ws_bytes >= aq_ws_bytes(B));
  MDM_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  MDM_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0);
  // torch.quantile's rank, in fp32 as torch forms it; above 2^24 it is an integer (lo == hi, w == 0)
  const float rank = q * (float)(n - 1);
  const double last = (double)(n - 1);
  const double fl = fmin(floor((double)rank), last), ce = fmin(ceil((double)rank), last);
  const unsigned lo = (unsigned)fl, hi = (unsigned)ce;
  const float w = rank - floorf(rank);
  const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  size_t blocks = (n + AQ_BLOCK_ELEMS - 1) / AQ_BLOCK_ELEMS;
  const size_t cap = AQ_MAX_BLOCKS / B > 1 ? AQ_MAX_BLOCKS / B : 1;
  if (blocks > cap) blocks = cap;
  if (blocks > (size_t)AQ_MAX_ROW_BLOCKS) blocks = AQ_MAX_ROW_BLOCKS;
  const dim3 grid((unsigned)blocks, B), blk(AQ_T);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned* w32 = reinterpret_cast<unsigned*>(ws);
  if (stages & 1u) hipLaunchKernelGGL(aq_zero_kernel, dim3((AQ_ROW / 4 + AQ_T - 1) / AQ_T, B), blk, 0, st, w32);
  if (vec) {
    if (stages & 2u) hipLaunchKernelGGL(aq_level1_kernel<true>, grid, blk, 0, st, x, w32, n);
    if (stages & 4u) hipLaunchKernelGGL(aq_level2_kernel<true>, grid, blk, 0, st, x, w32, n, lo, hi);
    if (stages & 8u) hipLaunchKernelGGL(aq_level3_kernel<true>, grid, blk, 0, st, x, w32, n);
  } else {
    if (stages & 2u) hipLaunchKernelGGL(aq_level1_kernel<false>, grid, blk, 0, st, x, w32, n);
    if (stages & 4u) hipLaunchKernelGGL(aq_level2_kernel<false>, grid, blk, 0, st, x, w32, n, lo, hi);
    if (stages & 8u) hipLaunchKernelGGL(aq_level3_kernel<false>, grid, blk, 0, st, x, w32, n);
  }
  if (stages & 16u) hipLaunchKernelGGL(aq_finish_kernel, dim3(B), blk, 0, st, w32, w, cmin, cmax, thr, stats);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_abs_quantile(const float* x, void* ws, size_t ws_bytes, int B, size_t n, float q, float cmin, float cmax,
                                float* thr, float* stats, void* stream) {
  return aq_run(x, ws, ws_bytes, B, n, q, cmin, cmax, thr, stats, stream, 31u);
}

// development aid (include/mdm_hip_dev.h): one launch of the five by itself
extern "C" int mdm_dev_abs_quantile_stage(const float* x, void* ws, size_t ws_bytes, int B, size_t n, float q, int stage,
                                          void* stream) {
  MDM_CHECK_ARG(stage >= 0 && stage <= 3);
  return aq_run(x, ws, ws_bytes, B, n, q, 0.f, 0.f, nullptr, nullptr, stream, 1u << stage);
}
