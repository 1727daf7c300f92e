// Input gradient of the stem convolution (conv_in: 3x3, stride 1, zero padding 1, 1..8 real input channels padded to a
// chunk in the forward pass) -- the last kernel on the way back to the model's own input x_t.
//
//   dx[n, ci, y, x] = sum over (sy, sx) in {-1, 0, 1}^2 and co of  dy[n, y + sy, x + sx, co] * w[co, ci, 1 - sy, 1 - sx]
//
// The problem's floor is reading dy once, and it has next to nothing for the matrix pipe: Cin = 3 output columns fill
// nothing of an MFMA tile, and the generic implicit GEMM would fetch nine shifted copies of dy through L2, write a padded
// NHWC tensor of the compute dtype and need a layout pass behind it (the argument of conv3x3_direct_kernel in
// gemm_conv.hip for the narrow outer levels).  So, per block of 256 threads:
//   * an 8 x 32 pixel tile, one output pixel per thread; the channels of dy go through LDS in slices of 128 bytes
//     (64 bf16 / 32 fp32): the 10 x 34 halo tile of a slice is staged ONCE, zeros written for out-of-image pixels, and
//     the nine shifted views are read from it as 16-byte LDS reads.  Pixel stride 144 bytes = 36 banks: the 16 lanes
//     of a ds_read_b128 group hold 16 different pixel indices mod 16 and 36 l mod 64 = 4 (9 l mod 16) is a bijection there,
//     so every group covers the 64 banks once.  10 * 34 * 144 = 48960 bytes, three blocks per CU.
//   * the filter is read straight from the FORWARD pack w_fwd [Cout][9][Cin_pad] (so the values are rounded exactly as the
//     forward operator rounds them and the kernel is its exact transpose): the address of a (co, tap) row is the same
//     for every lane, the loads are wave-uniform (scalar loads through the constant cache) and the products are VALU FMAs
//     with a uniform operand -- no LDS traffic for the weights, no vector registers.
//   * fp32 accumulators, fixed order (channel slice -> tap -> channel), no atomics: deterministic.
//   * the result is stored directly as fp32 NCHW [N, Cin, H, W], 128-byte runs per wave row; nothing of the compute dtype
//     is materialised and the gradient of x_t is not rounded on its last step.
// Bytes: N H W Cout elements of dy read once (+ the 340 / 256 halo overlap, which neighbouring blocks find in L2),
// 4 N H W Cin written = Cin / Cout (x 2 for bf16) of the read.
// What limits THIS form, by counting (nothing here is a measurement): per pixel 9 Cout Cin fp32 FMAs with a scalar operand
// plus 9 Cout bf16 -> fp32 unpacks of dy, i.e. at Cin = 3 in bf16 about 36 VALU lane-operations per 2 bytes of dy --
// roughly twice the read-once HBM time at the VALU peak, whatever Cout is -- and 9 * 64 scalar 16-byte loads per wave and
// slice.  The kernel is VALU-limited, not HBM-limited: its GB/s over the read-once byte count is expected at about half
// the streaming rate.  The padded-column MFMA form (dy as the A operand, the filter as a 16-column B operand) would
// move the products to the matrix pipe; it is the follow-up if this kernel ever shows in a profile.
#include "common.hpp"

namespace mdm {

constexpr int ST_TH = 8, ST_TW = 32;                       // pixel tile (one pixel per thread)
constexpr int ST_HH = ST_TH + 2, ST_HW = ST_TW + 2;         // with the one-pixel halo
constexpr int ST_SLICE = 128;                               // bytes of channels per pixel in LDS
constexpr int ST_PIX = ST_SLICE + 16;                       // padded pixel stride (bytes)

template <typename T> __device__ __forceinline__ float stem_w(const uint32_t* q, int ci);
template <> __device__ __forceinline__ float stem_w<float>(const uint32_t* q, int ci) { return __uint_as_float(q[ci]); }
template <> __device__ __forceinline__ float stem_w<bf16>(const uint32_t* q, int ci) {
  const uint32_t u = q[ci >> 1];
  return __uint_as_float((ci & 1) ? (u & 0xffff0000u) : (u << 16));
}

template <typename T, int CIN>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ w,
                                                         float* __restrict__ dx, int H, int W, int Cout, int tiles_x,
                                                         int tiles_y) {
  constexpr int EPV = Tr<T>::EPV;
  constexpr int CINP = (CIN + EPV - 1) / EPV * EPV;         // channels of a (co, tap) row of the forward pack
  constexpr int WQ = CINP * (int)sizeof(T) / 4;             // 32-bit words of such a row (4 or 8)
  constexpr int CK = ST_SLICE / (int)sizeof(T);             // channels per slice
  __shared__ __attribute__((aligned(16))) char tile[ST_HH * ST_HW * ST_PIX];

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int bx = b % tiles_x; b /= tiles_x;
  const int by = b % tiles_y;
  const int n = b / tiles_y;
  const int y0 = by * ST_TH, x0 = bx * ST_TW;
  const int ty = tid >> 5, tx = tid & 31;

  float acc[CIN];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;

  for (int c0 = 0; c0 < Cout; c0 += CK) {
    const int ck = min(CK, Cout - c0);                      // a multiple of EPV (Cout is)
    const int nch = ck / EPV;                               // 16-byte chunks of this slice
    if (c0) __syncthreads();                                // everyone is done with the slice before
    for (int idx = tid; idx < ST_HH * ST_HW * 8; idx += 256) {
      const int pix = idx >> 3, ch = idx & 7;
      if (ch >= nch) continue;
      const int hy = pix / ST_HW, hx = pix - hy * ST_HW;
      const int gy = y0 + hy - 1, gx = x0 + hx - 1;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < H && gx >= 0 && gx < W)
        v = *reinterpret_cast<const uint4*>(dy + (((size_t)n * H + gy) * W + gx) * Cout + c0 + ch * EPV);
      *reinterpret_cast<uint4*>(tile + pix * ST_PIX + ch * 16) = v;
    }
    __syncthreads();
#pragma unroll
    for (int sy = 0; sy < 3; ++sy) {
#pragma unroll
      for (int sx = 0; sx < 3; ++sx) {
        const char* p = tile + ((ty + sy) * ST_HW + tx + sx) * ST_PIX;
        const int tap = (2 - sy) * 3 + (2 - sx);            // the forward tap that carried x[y, x] into y[y + sy - 1, x + sx - 1]
        for (int g = 0; g < nch; ++g) {
          Chunk<T> v;
          v.load(reinterpret_cast<const T*>(p + g * 16));
          const uint32_t* wq = reinterpret_cast<const uint32_t*>(w) + ((size_t)(c0 + g * EPV) * 9 + tap) * WQ;
#pragma unroll
          for (int j = 0; j < EPV; ++j) {
            uint32_t q[WQ];
#pragma unroll
            for (int k = 0; k < WQ; ++k) q[k] = wq[(size_t)j * 9 * WQ + k];   // wave-uniform address
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) acc[ci] = fmaf(v.v[j], stem_w<T>(q, ci), acc[ci]);
          }
        }
      }
    }
  }
  const int y = y0 + ty, x = x0 + tx;
  if (y < H && x < W) {
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) dx[(((size_t)n * CIN + ci) * H + y) * W + x] = acc[ci];
  }
}

}  // namespace mdm

using namespace mdm;

template <typename T>
static void stem_dgrad_launch(const void* dy, const void* w, float* dx, int N, int H, int W, int Cout, int Cin,
                              hipStream_t st) {
  const int tx = (W + ST_TW - 1) / ST_TW, ty = (H + ST_TH - 1) / ST_TH;
  const dim3 grid((unsigned)((size_t)tx * ty * N)), block(256);
#define MDM_STEM_CASE(C)                                                                                          \
  case C:                                                                                                         \
    hipLaunchKernelGGL((stem_dgrad_kernel<T, C>), grid, block, 0, st, (const T*)dy, (const T*)w, dx, H, W, Cout, tx, ty); \
    break
  switch (Cin) {
    MDM_STEM_CASE(1); MDM_STEM_CASE(2); MDM_STEM_CASE(3); MDM_STEM_CASE(4);
    MDM_STEM_CASE(5); MDM_STEM_CASE(6); MDM_STEM_CASE(7); MDM_STEM_CASE(8);
  }
#undef MDM_STEM_CASE
}

extern "C" int mdm_conv3x3_stem_dgrad(const void* dy, const void* w_fwd, float* dx_nchw, int N, int H, int W, int Cout,
                                      int Cin, int dtype, void* stream) {
  MDM_CHECK_ARG(dy && w_fwd && dx_nchw);
  MDM_CHECK_ARG(N > 0 && H > 0 && W > 0);
  MDM_CHECK_ARG(Cin >= 1 && Cin <= 8);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(Cout > 0 && Cout % (dtype == DT_F32 ? 4 : 8) == 0);
  const size_t tiles = (size_t)((W + ST_TW - 1) / ST_TW) * ((H + ST_TH - 1) / ST_TH) * (size_t)N;
  MDM_CHECK_ARG(tiles <= 0x7fffffffu);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == DT_F32) stem_dgrad_launch<float>(dy, w_fwd, dx_nchw, N, H, W, Cout, Cin, st);
  else stem_dgrad_launch<bf16>(dy, w_fwd, dx_nchw, N, H, W, Cout, Cin, st);
  MDM_LAUNCH_STATUS();
}
