// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024) on the up path's skip concat:
//   out[n, p, 0:C1/2]   = h[n, p, :C1/2] * m[n, p]      m = b (v1), or 1 + (b - 1) hm[n, p] (v2, "structure")
//   out[n, p, C1/2:C1]  = h[n, p, C1/2:]                 bit for bit
//   out[n, p, C1:C1+C2] = r + (s - 1) / (H W) * sum_k coef_k[n, c] phi_k(y, x)
// The last line is the Fourier filter of the paper at its threshold 1 (the 2 x 2 centre of the shifted spectrum scaled
// by s) in closed form: the four bins are the DC term and the first harmonic along y, along x and along the diagonal,
// i.e. seven real modes phi = {1, cos t1, sin t1, cos t2, sin t2, cos t3, sin t3}, t1 = 2 pi y / H, t2 = 2 pi x / W,
// t3 = t1 + t2, with coef_k = sum_p r phi_k.  No FFT.
// Two launches (mdm_hip_ext.h): mdm_freeu_stats reads r once (and h once for v2), mdm_freeu_apply is mdm_concat's
// forward with both transforms fused.  cos / sin come from a per-row / per-column table in LDS (H + W sincos per block)
// and the angle-addition formulas.  Sums over pixels go through per-slab partials summed in slab order: no atomics,
// two runs are bit-identical.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

constexpr int FU_THREADS = 256;
constexpr int FU_TAB = 1024;   // H + W table entries (8 KB of LDS)
constexpr int FU_UNROLL = 4;   // pixels a thread has in flight per trip of its pixel loop

// tab[0, H) = (cos, sin)(2 pi y / H), tab[H, H + W) = (cos, sin)(2 pi x / W)
__device__ __forceinline__ void fu_fill_table(float2* tab, int H, int W) {
  for (int i = threadIdx.x; i < H + W; i += FU_THREADS) {
    const int num = i < H ? i : i - H, den = i < H ? H : W;
    float s, c;
    sincospif((float)(2 * num) / (float)den, &s, &c);
    tab[i] = make_float2(c, s);
  }
  __syncthreads();
}

// a 16-byte chunk held in registers -> its EPV values as fp32
__device__ __forceinline__ void fu_unpack(const uint4& w, Chunk<float>& v) {
  const f32x4 t = __builtin_bit_cast(f32x4, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) v.v[i] = t[i];
}
__device__ __forceinline__ void fu_unpack(const uint4& w, Chunk<bf16>& v) {
  const bf16x8 t = __builtin_bit_cast(bf16x8, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) v.v[i] = (float)t[i];
}

// phi_1 .. phi_6 at pixel p (phi_0 = 1)
__device__ __forceinline__ void fu_phi(const float2* tab, int H, int W, int p, float (&f)[6]) {
  const int y = p / W, x = p - y * W;
  const float2 a = tab[y], b = tab[H + x];
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
  f[4] = a.x * b.x - a.y * b.y;
  f[5] = a.y * b.x + a.x * b.y;
}

// Block = tx channel chunks x (256 / tx) pixel lanes; grid = (chunk blocks, pixel slabs, N).  Thread (cx, py) sums its
// chunk over the pixels p0 + py, p0 + py + ty, ... of slab blockIdx.y; the pixel lanes are then summed by shuffles and
// through LDS in a fixed order.  dst[((n * slabs + slab) * 7 + k) * C2 + c]: coef itself when there is one slab, the partials otherwise.
template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_stats_kernel(const T* __restrict__ r, float* __restrict__ dst, int H,
                                                                 int W, int C2, int tx, int slab_px) {
  constexpr int EPV = Tr<T>::EPV;
  __shared__ float2 tab[FU_TAB];
  __shared__ float red[FU_THREADS * EPV];
  fu_fill_table(tab, H, W);
  const int ty = FU_THREADS / tx, cx = threadIdx.x % tx, py = threadIdx.x / tx;
  const int col = blockIdx.x * tx + cx, ncol = C2 / EPV;
  const int slab = blockIdx.y, slabs = gridDim.y, n = blockIdx.z, HW = H * W;
  const int p0 = slab * slab_px, p1 = min(HW, p0 + slab_px);
  float acc[7][EPV];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[k][e] = 0.f;
  if (col < ncol) {
    const T* base = r + (size_t)n * HW * C2 + (size_t)col * EPV;
    // FU_UNROLL pixels per trip, their loads issued together; the sums still run in pixel order
    for (int p = p0 + py; p < p1; p += FU_UNROLL * ty) {
      uint4 raw[FU_UNROLL];
#pragma unroll
      for (int u = 0; u < FU_UNROLL; ++u)
        if (p + u * ty < p1) raw[u] = *reinterpret_cast<const uint4*>(base + (size_t)(p + u * ty) * C2);
#pragma unroll
      for (int u = 0; u < FU_UNROLL; ++u) {
        if (p + u * ty >= p1) break;
        Chunk<T> v;
        fu_unpack(raw[u], v);
        float f[6];
        fu_phi(tab, H, W, p + u * ty, f);
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          acc[0][e] += v.v[e];
#pragma unroll
          for (int k = 1; k < 7; ++k) acc[k][e] = fmaf(v.v[e], f[k - 1], acc[k][e]);
        }
      }
    }
  }
  // The sum over the pixel lanes, in a fixed order: inside a wave a butterfly over the lanes that share cx (xor offsets
  // tx, 2 tx, ... < 64; a wave is one pixel lane when tx == 64), then the four waves through LDS, wave 0 first.  Lanes
  // [0, tx) of a wave hold its sums for cx = lane; red[w * per + cx * EPV + e], per = tx * EPV <= FU_THREADS * EPV / 4.
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < EPV; ++e)
      for (int o = tx; o < 64; o <<= 1) acc[k][e] += __shfl_xor(acc[k][e], o, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, per = tx * EPV;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    if (lane < tx) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) red[wv * per + lane * EPV + e] = acc[k][e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < per; i += FU_THREADS) {
      const int c = blockIdx.x * per + i;   // the channel: chunk column blockIdx.x * tx + i / EPV, element i % EPV
      if (c < C2)
        dst[(((size_t)n * slabs + slab) * 7 + k) * C2 + c] = ((red[i] + red[per + i]) + red[2 * per + i]) + red[3 * per + i];
    }
    __syncthreads();
  }
}

// coef[n, j] = sum over slabs, in slab order, of part[n, slab, j]   (j over the 7 * C2 entries of a sample)
__global__ __launch_bounds__(FU_THREADS) void freeu_coef_reduce_kernel(const float* __restrict__ part,
                                                                       float* __restrict__ coef, int slabs, size_t per,
                                                                       size_t total) {
  for (size_t i = (size_t)blockIdx.x * FU_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * FU_THREADS) {
    const size_t n = i / per, j = i - n * per;
    float t = 0.f;
    for (int s = 0; s < slabs; ++s) t += part[(n * slabs + s) * per + j];
    coef[i] = t;
  }
}

// mu[m] = mean over the C1 channels of pixel m: lp lanes (a power of two <= 64) per pixel, 256 / lp pixels per block
template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_mean_kernel(const T* __restrict__ h, float* __restrict__ mu, size_t M,
                                                                int C1, int lp) {
  constexpr int EPV = Tr<T>::EPV;
  const int k1 = C1 / EPV, ppb = FU_THREADS / lp, g = threadIdx.x / lp, l = threadIdx.x % lp;
  const float inv = 1.f / (float)C1;
  for (size_t m0 = (size_t)blockIdx.x * ppb; m0 < M; m0 += (size_t)gridDim.x * ppb) {
    const size_t m = m0 + g;
    float sum = 0.f;
    if (m < M) {
      for (int j = l; j < k1; j += lp) {
        Chunk<T> v;
        v.load(h + m * C1 + (size_t)j * EPV);
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < EPV; ++e) t += v.v[e];
        sum += t;
      }
    }
    for (int o = lp >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (m < M && l == 0) mu[m] = sum * inv;
  }
}

// mm[2 n] = min, mm[2 n + 1] = max of mu[n, :] -- one block per sample (min / max do not depend on the order)
__global__ __launch_bounds__(FU_THREADS) void freeu_minmax_kernel(const float* __restrict__ mu, float* __restrict__ mm,
                                                                  int HW) {
  __shared__ float s[2 * FU_THREADS / 64];
  const int n = blockIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int p = threadIdx.x; p < HW; p += FU_THREADS) {
    const float v = mu[(size_t)n * HW + p];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = -wave_max(-mn);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    s[2 * (threadIdx.x >> 6)] = mn;
    s[2 * (threadIdx.x >> 6) + 1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FU_THREADS / 64; ++w) {
      mn = fminf(mn, s[2 * w]);
      mx = fmaxf(mx, s[2 * w + 1]);
    }
    mm[2 * n] = mn;
    mm[2 * n + 1] = mx;
  }
}

// The concat with both transforms.  Geometry as freeu_stats_kernel over the (C1 + C2) / EPV output chunks: a thread keeps
// its chunk column over the pixels of its slab, so a skip column reads its 7 coefficients once.  g = (s - 1) / (H W);
// g == 0 copies the skip raw.  mu == nullptr: v1.
template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_apply_kernel(const T* __restrict__ h, const T* __restrict__ r,
                                                                 T* __restrict__ out, const float* __restrict__ coef,
                                                                 const float* __restrict__ mu, const float* __restrict__ mm,
                                                                 int H, int W, int C1, int C2, int tx, int slab_px, float b,
                                                                 float g) {
  constexpr int EPV = Tr<T>::EPV;
  __shared__ float2 tab[FU_TAB];
  fu_fill_table(tab, H, W);
  const int ty = FU_THREADS / tx, cx = threadIdx.x % tx, py = threadIdx.x / tx;
  const int k1 = C1 / EPV, kh = k1 / 2, k = (C1 + C2) / EPV;
  const int col = blockIdx.x * tx + cx, n = blockIdx.z, HW = H * W;
  const int p0 = blockIdx.y * slab_px, p1 = min(HW, p0 + slab_px);
  if (col >= k) return;
  T* o = out + (size_t)n * HW * (C1 + C2) + (size_t)col * EPV;
  const size_t ldo = (size_t)(C1 + C2);
  if (col >= k1) {
    const int c0 = (col - k1) * EPV;
    const T* src = r + (size_t)n * HW * C2 + c0;
    if (g == 0.f) {
      for (int p = p0 + py; p < p1; p += ty)
        *reinterpret_cast<uint4*>(o + p * ldo) = *reinterpret_cast<const uint4*>(src + (size_t)p * C2);
      return;
    }
    float cf[7][EPV];
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
      for (int e = 0; e < EPV; ++e) cf[q][e] = g * coef[((size_t)n * 7 + q) * C2 + c0 + e];
    for (int p = p0 + py; p < p1; p += FU_UNROLL * ty) {
      uint4 raw[FU_UNROLL];
#pragma unroll
      for (int u = 0; u < FU_UNROLL; ++u)
        if (p + u * ty < p1) raw[u] = *reinterpret_cast<const uint4*>(src + (size_t)(p + u * ty) * C2);
#pragma unroll
      for (int u = 0; u < FU_UNROLL; ++u) {
        const int pu = p + u * ty;
        if (pu >= p1) break;
        Chunk<T> v;
        fu_unpack(raw[u], v);
        float f[6];
        fu_phi(tab, H, W, pu, f);
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          float t = cf[0][e];
#pragma unroll
          for (int q = 1; q < 7; ++q) t = fmaf(cf[q][e], f[q - 1], t);
          v.v[e] += t;
        }
        v.store(o + pu * ldo);
      }
    }
  } else if (col < kh) {
    const T* src = h + (size_t)n * HW * C1 + (size_t)col * EPV;
    float mn = 0.f, mx = 0.f;
    if (mu) { mn = mm[2 * n]; mx = mm[2 * n + 1]; }
    const bool map = mu && mx > mn;   // max == min: hm = 1, the v1 scale
    for (int p = p0 + py; p < p1; p += ty) {
      Chunk<T> v;
      v.load(src + (size_t)p * C1);
      const float m = map ? fmaf(b - 1.f, (mu[(size_t)n * HW + p] - mn) / (mx - mn), 1.f) : b;
#pragma unroll
      for (int e = 0; e < EPV; ++e) v.v[e] *= m;
      v.store(o + p * ldo);
    }
  } else {
    const T* src = h + (size_t)n * HW * C1 + (size_t)col * EPV;
    for (int p = p0 + py; p < p1; p += ty)
      *reinterpret_cast<uint4*>(o + p * ldo) = *reinterpret_cast<const uint4*>(src + (size_t)p * C1);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct FuGeom {
  int tx, colblocks, slabs, slab_px;
};
// ncol chunk columns, HW pixels, N samples: about 1024 blocks where the shape has them, every pixel lane of a slab with
// at least 4 pixels.  A function of the shape alone: the plan, the statistics and the apply launch agree on it.
static FuGeom fu_geom(int ncol, int HW, int N) {
  FuGeom q;
  q.tx = 1;
  while (q.tx < ncol && q.tx < 64) q.tx <<= 1;
  while (q.tx > 8 && ncol % q.tx) q.tx >>= 1;   // 96 columns: 3 full blocks of 32, not 2 of 64 with one half idle
  q.colblocks = (ncol + q.tx - 1) / q.tx;
  const long long base = (long long)q.colblocks * N;
  long long want = (1024 + base - 1) / base;
  if (want > 65535) want = 65535;
  const int min_px = (FU_THREADS / q.tx) * FU_UNROLL;
  const int even = (int)((HW + want - 1) / want);
  q.slab_px = even > min_px ? even : min_px;
  q.slabs = (HW + q.slab_px - 1) / q.slab_px;
  return q;
}

struct FuLayout {
  size_t coef, part, mu, mm, total;   // offsets in floats; part == 0: one slab, no partials
  FuGeom stats;
};
static inline size_t fu_up4(size_t v) { return (v + 3) & ~(size_t)3; }
static FuLayout fu_layout(int N, int H, int W, int C2, int epv, int structure) {
  FuLayout L;
  L.stats = fu_geom(C2 / epv, H * W, N);
  size_t at = 0;
  L.coef = at; at += (size_t)N * 7 * C2;
  L.part = 0;
  if (L.stats.slabs > 1) { L.part = at; at += (size_t)N * L.stats.slabs * 7 * C2; }
  L.mu = L.mm = 0;
  if (structure) {
    L.mu = at; at += fu_up4((size_t)N * H * W);
    L.mm = at; at += fu_up4((size_t)2 * N);
  }
  L.total = at;
  return L;
}

}  // namespace mdm

using namespace mdm;

#define FU_DISPATCH_T(dtype, ...)                                      \
  if ((dtype) == DT_F32) { typedef float TT; __VA_ARGS__; }            \
  else { typedef bf16 TT; __VA_ARGS__; }

static int fu_check_shape(int N, int H, int W, int C1, int C2, int dtype) {
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  const int epv = dtype == DT_F32 ? 4 : 8;
  MDM_CHECK_ARG(N >= 1 && N <= 65535);
  MDM_CHECK_ARG(H >= 2 && W >= 2 && H + W <= FU_TAB);
  MDM_CHECK_ARG(C1 >= 2 * epv && C1 % (2 * epv) == 0);
  MDM_CHECK_ARG(C2 >= epv && C2 % epv == 0);
  return 0;
}

extern "C" int mdm_freeu_plan(int N, int H, int W, int C1, int C2, int dtype, int structure, size_t* ws_bytes) {
  MDM_CHECK_ARG(ws_bytes);
  if (fu_check_shape(N, H, W, C1, C2, dtype) != 0) return -1;
  *ws_bytes = fu_layout(N, H, W, C2, dtype == DT_F32 ? 4 : 8, structure).total * sizeof(float);
  return 0;
}

extern "C" int mdm_freeu_stats(const void* h, const void* r, void* ws, size_t ws_bytes, int N, int H, int W, int C1, int C2,
                               int structure, int dtype, void* stream) {
  MDM_CHECK_ARG(r && ws && (h || !structure));
  if (fu_check_shape(N, H, W, C1, C2, dtype) != 0) return -1;
  const int epv = dtype == DT_F32 ? 4 : 8;
  const FuLayout L = fu_layout(N, H, W, C2, epv, structure);
  MDM_CHECK_ARG(ws_bytes >= L.total * sizeof(float));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* f = reinterpret_cast<float*>(ws);
  const FuGeom q = L.stats;
  float* dst = q.slabs > 1 ? f + L.part : f + L.coef;
  FU_DISPATCH_T(dtype, hipLaunchKernelGGL(freeu_stats_kernel<TT>, dim3(q.colblocks, q.slabs, N), dim3(FU_THREADS), 0, st,
                                          (const TT*)r, dst, H, W, C2, q.tx, q.slab_px));
  if (q.slabs > 1) {
    const size_t per = (size_t)7 * C2, total = per * N;
    const size_t nb = (total + FU_THREADS - 1) / FU_THREADS;
    hipLaunchKernelGGL(freeu_coef_reduce_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(FU_THREADS), 0, st,
                       (const float*)(f + L.part), f + L.coef, q.slabs, per, total);
  }
  if (structure) {
    const size_t M = (size_t)N * H * W;
    int lp = 1;
    while (lp < C1 / epv && lp < 64) lp <<= 1;
    const size_t ppb = FU_THREADS / lp, nb = (M + ppb - 1) / ppb;
    FU_DISPATCH_T(dtype, hipLaunchKernelGGL(freeu_mean_kernel<TT>, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(FU_THREADS),
                                            0, st, (const TT*)h, f + L.mu, M, C1, lp));
    hipLaunchKernelGGL(freeu_minmax_kernel, dim3(N), dim3(FU_THREADS), 0, st, (const float*)(f + L.mu), f + L.mm, H * W);
  }
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_freeu_apply(const void* h, const void* r, const void* ws, size_t ws_bytes, void* out, int N, int H, int W,
                               int C1, int C2, float b, float s, int structure, int dtype, void* stream) {
  MDM_CHECK_ARG(h && r && ws && out && out != h && out != r);
  if (fu_check_shape(N, H, W, C1, C2, dtype) != 0) return -1;
  MDM_CHECK_ARG(b > 0.f && b <= 3.0e38f && s >= 0.f && s <= 3.0e38f);   // finite; NaN fails both
  const int epv = dtype == DT_F32 ? 4 : 8;
  const FuLayout L = fu_layout(N, H, W, C2, epv, structure);
  MDM_CHECK_ARG(ws_bytes >= L.total * sizeof(float));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float* f = reinterpret_cast<const float*>(ws);
  const FuGeom q = fu_geom((C1 + C2) / epv, H * W, N);
  const float g = (s - 1.f) / (float)(H * W);
  const float* mu = structure ? f + L.mu : nullptr;
  const float* mm = structure ? f + L.mm : nullptr;
  FU_DISPATCH_T(dtype, hipLaunchKernelGGL(freeu_apply_kernel<TT>, dim3(q.colblocks, q.slabs, N), dim3(FU_THREADS), 0, st,
                                          (const TT*)h, (const TT*)r, (TT*)out, f + L.coef, mu, mm, H, W, C1, C2, q.tx,
                                          q.slab_px, b, g));
  MDM_LAUNCH_STATUS();
}
