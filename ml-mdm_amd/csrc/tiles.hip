// Tiled (MultiDiffusion, Bar-Tal et al., ICML 2023) sampling: the two image-side kernels around the denoiser call of a step.
//   mdm_tiles_gather   canvas x [B, C, H, W] -> the model's rows [reps, B, T, C, h, w]: every window of every image, once
//                      per block of the model batch ([uncond | cond | perturbed]) -- reads each element once, stores it
//                      `reps` times, so it also does what torch.cat([x] * reps) does for the untiled samplers
//   mdm_tiles_merge    predictions p [R, T, C, h, w] -> canvas [R, C, H, W]: the weighted mean of the windows over a pixel
// The windows form a separable grid: along an axis of length L with window `win` and stride `s` there are
// n = ceil((L - win) / s) + 1 of them at offsets o_i = min(i s, L - win) -- the last one clamped to the border.  Windows
// 0 .. n - 2 sit at i s < L - win, so the ones over a position y are the run  max(0, floor((y - win) / s) + 1) ..
// min(floor(y / s), n - 2)  plus window n - 1 where y >= L - win: arithmetic on (y, win, s, L), no offset table.
// fp32 NCHW throughout.  Consecutive lanes take consecutive x; 16 bytes per lane where every row start that occurs is
// 16-byte aligned (w, W, sx, W - w multiples of 4 and aligned bases), 4 bytes otherwise.  Each output element gathers its
// own terms in window order (i ascending, then j): no atomics, no workspace, no dependence on the batch.  Forward only.
#include "common.hpp"
#include "../../include/mdm_hip.h"
#include "../../include/mdm_hip_ext.h"

namespace mdm {

constexpr int TL_THREADS = 256;

struct TlAxis {
  int n;      // windows along the axis
  int win;    // window length
  int s;      // stride
  int last;   // offset of window n - 1: L - win
};

static TlAxis tl_axis(int L, int win, int s) {
  TlAxis a;
  a.n = (L - win + s - 1) / s + 1;
  a.win = win;
  a.s = s;
  a.last = L - win;
  return a;
}

__device__ __forceinline__ int tl_offset(const TlAxis& a, int i) {
  const int o = i * a.s;
  return o < a.last ? o : a.last;
}

// the windows over position y, in ascending order: m-th of them (m < count) is window tl_window(a, lo, run, m)
__device__ __forceinline__ int tl_cover(const TlAxis& a, int y, int& lo, int& run) {
  lo = y < a.win ? 0 : (y - a.win) / a.s + 1;
  int hi = y / a.s;
  if (hi > a.n - 2) hi = a.n - 2;
  run = hi >= lo ? hi - lo + 1 : 0;
  return run + (y >= a.last ? 1 : 0);
}
__device__ __forceinline__ int tl_window(const TlAxis& a, int lo, int run, int m) { return m < run ? lo + m : a.n - 1; }

__device__ __forceinline__ float tl_ramp(int pos, int win) {
  const int up = pos + 1, down = win - pos;
  return (float)(up < down ? up : down);
}

template <int V> struct TlVec;
template <> struct TlVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  __device__ __forceinline__ void store(float* p) const {
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  }
};
template <> struct TlVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};

// grid (ceil(C h (w / V) / 256), T, B): one lane per V consecutive elements of a window row
template <int V>
__global__ __launch_bounds__(TL_THREADS) void tiles_gather_kernel(const float* __restrict__ x, float* __restrict__ out, int B,
                                                                  int C, int H, int W, TlAxis ay, TlAxis ax, int reps,
                                                                  unsigned per_window) {
  const unsigned e = blockIdx.x * (unsigned)TL_THREADS + threadIdx.x;
  if (e >= per_window) return;
  const int h = ay.win, w = ax.win;
  const unsigned wv = (unsigned)w / V;
  const int b0 = (int)(e % wv) * V;
  const unsigned t = e / wv;
  const int a = (int)(t % (unsigned)h), c = (int)(t / (unsigned)h);
  const int k = blockIdx.y, b = blockIdx.z, T = ay.n * ax.n;
  const int oy = tl_offset(ay, k / ax.n), ox = tl_offset(ax, k % ax.n);
  TlVec<V> val;
  val.load(x + (((size_t)b * C + c) * H + (size_t)(oy + a)) * W + (size_t)(ox + b0));
  const size_t hw = (size_t)h * w;
  const size_t in_window = (size_t)c * hw + (size_t)a * w + (size_t)b0;
  for (int rep = 0; rep < reps; ++rep)
    val.store(out + (((size_t)rep * B + b) * T + k) * C * hw + in_window);
}

// grid (ceil(C H (W / V) / 256), R): one lane per V consecutive canvas elements.  On the vector path every offset is a
// multiple of 4, so the four elements of a lane lie under the same windows.
template <int V, bool RAMP>
__global__ __launch_bounds__(TL_THREADS) void tiles_merge_kernel(const float* __restrict__ p, float* __restrict__ out, int C,
                                                                 int H, int W, TlAxis ay, TlAxis ax, unsigned per_row) {
  const unsigned e = blockIdx.x * (unsigned)TL_THREADS + threadIdx.x;
  if (e >= per_row) return;
  const int h = ay.win, w = ax.win;
  const unsigned Wv = (unsigned)W / V;
  const int x0 = (int)(e % Wv) * V;
  const unsigned t = e / Wv;
  const int y = (int)(t % (unsigned)H), c = (int)(t / (unsigned)H);
  const size_t r = blockIdx.y;
  const int T = ay.n * ax.n;
  const size_t hw = (size_t)h * w;
  const float* pr = p + r * T * C * hw + (size_t)c * hw;
  float* dst = out + ((r * C + c) * H + (size_t)y) * W + (size_t)x0;
  int ylo, yrun, xlo, xrun;
  const int ny = tl_cover(ay, y, ylo, yrun), nx = tl_cover(ax, x0, xlo, xrun);
  TlVec<V> val;
  if (ny * nx == 1) {   // one window over the pixel: its value, bit for bit
    const int i = tl_window(ay, ylo, yrun, 0), j = tl_window(ax, xlo, xrun, 0);
    val.load(pr + (size_t)(i * ax.n + j) * C * hw + (size_t)(y - tl_offset(ay, i)) * w + (size_t)(x0 - tl_offset(ax, j)));
    val.store(dst);
    return;
  }
  float num[V], den[V];
#pragma unroll
  for (int q = 0; q < V; ++q) num[q] = den[q] = 0.f;
  for (int my = 0; my < ny; ++my) {
    const int i = tl_window(ay, ylo, yrun, my);
    const int a = y - tl_offset(ay, i);
    const float wy = RAMP ? tl_ramp(a, h) : 1.f;
    for (int mx = 0; mx < nx; ++mx) {
      const int j = tl_window(ax, xlo, xrun, mx);
      const int b0 = x0 - tl_offset(ax, j);
      val.load(pr + (size_t)(i * ax.n + j) * C * hw + (size_t)a * w + (size_t)b0);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const float wt = RAMP ? wy * tl_ramp(b0 + q, w) : 1.f;   // integers below 2^24: exact
        num[q] = RAMP ? fmaf(wt, val.v[q], num[q]) : num[q] + val.v[q];
        den[q] += wt;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < V; ++q) val.v[q] = num[q] / den[q];
  val.store(dst);
}

static inline bool tl_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// every row start that a 16-byte access can meet is 16-byte aligned
static inline bool tl_vector_ok(const void* a, const void* b, int W, int w, int sx) {
  return tl_aligned(a) && tl_aligned(b) && w % 4 == 0 && W % 4 == 0 && sx % 4 == 0 && (W - w) % 4 == 0;
}

static int tl_check_geometry(int C, int H, int W, int h, int w, int sy, int sx) {
  MDM_CHECK_ARG(C >= 1 && H >= 1 && W >= 1);
  MDM_CHECK_ARG(h >= 1 && h <= H && w >= 1 && w <= W);
  MDM_CHECK_ARG(sy >= 1 && sy <= h && sx >= 1 && sx <= w);   // every pixel under a window
  MDM_CHECK_ARG((size_t)C * H * W < ((size_t)1 << 31));      // the in-image index of a lane is 32 bits
  return 0;
}

}  // namespace mdm

using namespace mdm;

extern "C" int mdm_tiles_gather(const float* x, float* out, int B, int C, int H, int W, int h, int w, int sy, int sx,
                                int reps, void* stream) {
  MDM_CHECK_ARG(x && out && x != out);
  MDM_CHECK_ARG(B >= 1 && B <= 65535 && reps >= 1);
  if (tl_check_geometry(C, H, W, h, w, sy, sx) != 0) return -1;
  const TlAxis ay = tl_axis(H, h, sy), ax = tl_axis(W, w, sx);
  MDM_CHECK_ARG((size_t)ay.n * ax.n <= 65535);
  const bool vec = tl_vector_ok(x, out, W, w, sx);
  const unsigned per_window = (unsigned)((size_t)C * h * (vec ? w / 4 : w));
  const dim3 grid((per_window + TL_THREADS - 1) / TL_THREADS, ay.n * ax.n, B);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(tiles_gather_kernel<4>, grid, dim3(TL_THREADS), 0, st, x, out, B, C, H, W, ay, ax, reps, per_window);
  else
    hipLaunchKernelGGL(tiles_gather_kernel<1>, grid, dim3(TL_THREADS), 0, st, x, out, B, C, H, W, ay, ax, reps, per_window);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_tiles_merge(const float* p, float* out, int R, int C, int H, int W, int h, int w, int sy, int sx,
                               int blend, void* stream) {
  MDM_CHECK_ARG(p && out && p != out);
  MDM_CHECK_ARG(R >= 1 && R <= 65535);
  MDM_CHECK_ARG(blend == 0 || blend == 1);
  if (tl_check_geometry(C, H, W, h, w, sy, sx) != 0) return -1;
  // ramp: the largest weight, ceil(h / 2) ceil(w / 2), is an exact integer in fp32
  MDM_CHECK_ARG(blend == 0 || (size_t)((h + 1) / 2) * ((w + 1) / 2) <= ((size_t)1 << 24));
  const TlAxis ay = tl_axis(H, h, sy), ax = tl_axis(W, w, sx);
  MDM_CHECK_ARG((size_t)ay.n * ax.n <= 65535);
  const bool vec = tl_vector_ok(p, out, W, w, sx);
  const unsigned per_row = (unsigned)((size_t)C * H * (vec ? W / 4 : W));
  const dim3 grid((per_row + TL_THREADS - 1) / TL_THREADS, R);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define MDM_TL_MERGE(V, RAMP) \
  hipLaunchKernelGGL((tiles_merge_kernel<V, RAMP>), grid, dim3(TL_THREADS), 0, st, p, out, C, H, W, ay, ax, per_row)
  if (vec) {
    if (blend) MDM_TL_MERGE(4, true); else MDM_TL_MERGE(4, false);
  } else {
    if (blend) MDM_TL_MERGE(1, true); else MDM_TL_MERGE(1, false);
  }
#undef MDM_TL_MERGE
  MDM_LAUNCH_STATUS();
}
