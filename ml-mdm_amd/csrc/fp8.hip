// MXFP8 (OCP MX, E4M3 codes + one E8M0 scale byte per 32 consecutive K elements) sampling path for the plain-GEMM layers of
// SelfAttention: qkv, proj_out and the two FFN convolutions (reference models/unet.py:296-313).  Inference only.
//
//   mx8_quant_kernel   rows [M, K] (bf16 / fp32) -> codes [M, Kp] + scales [M, Kp / 32], Kp = K rounded up to 128
//   mx8_gemm_kernel    Y[M, N] = A W^T (+ bias) (+ GELU) (+ residual) on v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation;
//                      the output is bf16, or (EMIT) the MXFP8 form of the bf16-rounded value -- the SAME encoder as the
//                      quantiser's (mx8_encode8), so the fused form equals mx8_quant(bf16 output) bit for bit
//
// Format: amax = the block's largest magnitude, e = clamp(floor(log2 amax) - 8, -127, 127), scale byte
// s = e + 127 (amax == 0: s = 127), code = RNE_e4m3fn(clamp(x 2^-e, -448, 448)).  floor(log2 amax) is the exponent field of the
// fp32 amax: a subnormal amax (field 0) gives e <= -135, i.e. the clamp, as the real logarithm does.
//
// MFMA shape: 16x16x128 rather than 32x32x64 -- it keeps the accumulator-to-row-chunk staging of conv_gemm_bl_kernel, whose
// epilogue this kernel copies, and 4 x 4 tiles per wave give every loaded fragment four uses.  Operand map, found on the
// device and pinned by the exact-data test of tests/test_fp8_gpu.py (NOT 32 contiguous K per lane): lane l, register r of
// the 8, byte b holds X[row l & 15][k = 64 (r >> 2) + 16 (l >> 4) + 4 (r & 3) + b] -- two 16-byte pieces, one from each
// half of the 128 -- and the scale of K block kb = k / 32 is read from the scale VGPR (byte picked by op_sel) of lane
// 16 kb + row.  So lane (row, g = l >> 4) loads the 16-byte chunks g and 4 + g of its row and supplies the scale byte of
// block g.  D[row = 4 (l >> 4) + i][col = l & 15] as for every 16x16 MFMA.  As in conv_gemm_bl_kernel the WEIGHT fragment is
// the first operand: a lane then owns 4 consecutive output channels of one pixel.
//
// Structure: 128 x 128 x 128 tile, 4 waves (2 x 2, 64 x 64 each), two LDS stages filled by global_load_lds (16-byte copies
// for the codes, 4-byte copies for the tile's 128 + 128 scale dwords), one barrier per k-tile.  The XOR swizzle of the
// 128-byte LDS rows sits on the SOURCE address (the DMA writes lane-linear).  Deterministic: no split-K.
//
// The 3x3 convolutions of ResNet (reference models/unet.py:223-238) run on the same kernel as an implicit GEMM (CONV): the
// k-loop walks 9 taps x Kp / 128 tiles, tap outer, and for tap (dy, dx) tile row m = (b, y, x) takes its 128-byte code row and
// its scale dword from row m + dy W + dx of the SAME quantised activation (blocks run along the channels of one pixel, so one
// quantisation serves all nine taps) -- a row gather on the per-lane DMA source address, nothing else changes.  A tap outside
// the image, tested on (y, x) and never on the flat index, reads the ZERO ROW: row M of the activation, codes 0 / scale 127,
// written by the quantiser itself (mdm_mx8_quant_zrow).  The weight is [Cout 9, Kp] with row o 9 + ky 3 + kx.
#include <climits>

#include "common.hpp"

#include "../../include/mdm_hip.h"

namespace mdm {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive elements of one MX block per lane, 4 adjacent lanes per block: codes of this lane's 8 elements and the
// block's scale byte (identical in the 4 lanes).  Every lane of the wave must call it (cross-lane reduce).
__device__ __forceinline__ void mx8_encode8(const float (&v)[8], uint2& codes, unsigned& sbyte) {
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(v[j]));
  am = fmaxf(am, __shfl_xor(am, 1, 64));
  am = fmaxf(am, __shfl_xor(am, 2, 64));
  const int field = (int)((__float_as_uint(am) >> 23) & 0xffu);
  int e = field - 135;               // floor(log2 amax) - 8
  e = e < -127 ? -127 : e;           // (the upper clamp cannot bind: field <= 254)
  if (am == 0.f) e = 0;
  sbyte = (unsigned)(e + 127);
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);   // 2^-e, exact
  float t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = __builtin_amdgcn_fmed3f(v[j] * inv, -448.f, 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], w1, true);
  codes = uint2{(unsigned)w0, (unsigned)w1};
}
// the 4 scale bytes of 128 consecutive elements (16 adjacent lanes, lane & 15 == 0 first) as one dword; valid in that lane
__device__ __forceinline__ unsigned mx8_gather_scales(unsigned sbyte) {
  const int lane = threadIdx.x & 63;
  const unsigned s1 = __shfl(sbyte, lane + 4, 64), s2 = __shfl(sbyte, lane + 8, 64), s3 = __shfl(sbyte, lane + 12, 64);
  return sbyte | (s1 << 8) | (s2 << 16) | (s3 << 24);
}

template <typename T>
__global__ __launch_bounds__(256) void mx8_quant_kernel(const T* __restrict__ x, unsigned char* __restrict__ q,
                                                        unsigned char* __restrict__ s, int M, int Msrc, int K, int Kp) {
  const int cpr = Kp >> 3;                                   // 8-element pieces per padded row: a multiple of 16
  const size_t total = (size_t)M * cpr;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = idx < total;                            // uniform over each group of 16 lanes
  const size_t row = valid ? idx / cpr : 0;
  const int k = valid ? (int)(idx - row * cpr) * 8 : 0;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (valid && k < K && row < (size_t)Msrc) {                // K % 8 == 0: a piece is inside the row or in the padding; rows
                                                             // Msrc .. M - 1 have no source: code 0, scale 127 (the zero row)
    const T* src = x + row * K + k;
    if constexpr (sizeof(T) == 2) {
      Chunk<bf16> c;
      c.load(src);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = c.v[j];
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    }
  }
  uint2 codes;
  unsigned sb;
  mx8_encode8(v, codes, sb);
  const unsigned sw = mx8_gather_scales(sb);
  if (valid) {
    *reinterpret_cast<uint2*>(q + row * Kp + k) = codes;
    if ((threadIdx.x & 15) == 0) *reinterpret_cast<unsigned*>(s + row * (Kp >> 5) + (k >> 5)) = sw;
  }
}

struct Mx8GemmArgs {
  const unsigned char *qa, *sa, *qw, *sw;
  const float* bias;
  const bf16* res;
  bf16* y;
  unsigned char *q_out, *s_out;
  int M, N, Kp, act;
  int H, W;   // CONV: the image; M = batch H W pixels, qa / sa hold M + 1 rows (the zero row last), qw / sw 9 N rows
};

constexpr int MX_BM = 128, MX_BN = 128;
constexpr int MX_A_BYTES = MX_BM * 128, MX_B_BYTES = MX_BN * 128;
constexpr int MX_SC_BYTES = (MX_BM + MX_BN) * 4;
constexpr int MX_STAGE = MX_A_BYTES + MX_B_BYTES + MX_SC_BYTES;
constexpr int MX_SMEM = 2 * MX_STAGE;
constexpr int MX_PITCH = MX_BN * 2 + 16;     // staged bf16 output rows, padded by one chunk
static_assert(MX_BM * MX_PITCH <= MX_SMEM, "the staged output tile must fit the k-loop's LDS");

template <bool EMIT, bool CONV>
__global__ __launch_bounds__(256) void mx8_gemm_kernel(const Mx8GemmArgs p) {
  static_assert(!(EMIT && CONV), "the 3x3 form has no emitting epilogue");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int quad = lane >> 4, l16 = lane & 15;
  const int tiles_n = (p.N + MX_BN - 1) / MX_BN;
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (t / tiles_n) * MX_BM, n0 = (t % tiles_n) * MX_BN;
  const int sb_row = p.Kp >> 5;              // scale bytes per row

  // ---- loader: thread (row = tid >> 3, slot = tid & 7) of pass j fills physical 16-byte slot `slot` of tile row
  // row + 32 j with the logical chunk slot ^ (row & 7).  Rows past the edge re-read the last row (never stored).
  const int lrow = tid >> 3;
  const int lchunk = (tid & 7) ^ (lrow & 7);
  const unsigned char* a_src[4];
  const unsigned char* b_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = min(m0 + lrow + 32 * j, p.M - 1), n = min(n0 + lrow + 32 * j, p.N - 1);
    a_src[j] = p.qa + (size_t)m * p.Kp + lchunk * 16;
    b_src[j] = p.qw + (size_t)n * p.Kp + lchunk * 16;
  }
  // CONV: the pixel (y, x) of this thread's four code rows and of its scale row; a row past M gets y = -2, so that no tap of
  // it is ever inside the image and it reads the zero row (it is never stored)
  int ry[4], rx[4], sy = -2, sx = 0;
  if constexpr (CONV) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + lrow + 32 * j, q = m / p.W;
      rx[j] = m - q * p.W;
      ry[j] = m < p.M ? q % p.H : -2;
    }
    if (tid < MX_BM && m0 + tid < p.M) {
      const int q = (m0 + tid) / p.W;
      sx = m0 + tid - q * p.W;
      sy = q % p.H;
    }
  }
  // the tile's scales: one dword (4 blocks = 128 k) per row; threads 0..127 the A rows, 128..255 the W rows
  const unsigned char* sc_src = tid < MX_BM ? p.sa + (size_t)min(m0 + tid, p.M - 1) * sb_row
                                            : p.sw + (size_t)min(n0 + tid - MX_BM, p.N - 1) * sb_row;
  // CONV: the sources of tap ky 3 + kx -- row m + dy W + dx where (y + dy, x + dx) is inside the image, else the zero row M
#define MDM_SET_TAP(tap)                                                                                  \
  {                                                                                                       \
    const int dy = (tap) / 3 - 1, dx = (tap) - ((tap) / 3) * 3 - 1;                                       \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
      const bool in = (unsigned)(ry[j] + dy) < (unsigned)p.H && (unsigned)(rx[j] + dx) < (unsigned)p.W;   \
      const int m = in ? m0 + lrow + 32 * j + dy * p.W + dx : p.M;                                        \
      const int n = min(n0 + lrow + 32 * j, p.N - 1);                                                     \
      a_src[j] = p.qa + (size_t)m * p.Kp + lchunk * 16;                                                   \
      b_src[j] = p.qw + ((size_t)n * 9 + (tap)) * p.Kp + lchunk * 16;                                     \
    }                                                                                                     \
    if (tid < MX_BM) {                                                                                    \
      const bool in = (unsigned)(sy + dy) < (unsigned)p.H && (unsigned)(sx + dx) < (unsigned)p.W;         \
      sc_src = p.sa + (size_t)(in ? m0 + tid + dy * p.W + dx : p.M) * sb_row;                             \
    } else {                                                                                              \
      sc_src = p.sw + ((size_t)min(n0 + tid - MX_BM, p.N - 1) * 9 + (tap)) * sb_row;                      \
    }                                                                                                     \
  }
  const int wave_lds = __builtin_amdgcn_readfirstlane(wave * 1024);
  const int wave_sc = __builtin_amdgcn_readfirstlane(wave * 256);
#define MDM_GLDS(src, lds_ptr, bytes)                                                                     \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),                  \
                                   (__attribute__((address_space(3))) void*)(lds_ptr), bytes, 0, 0)
#define MDM_STAGE_TILE(stage, kt)                                                                         \
  {                                                                                                       \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) MDM_GLDS(a_src[j] + (size_t)(kt) * 128, (stage) + j * 4096 + wave_lds, 16); \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                         \
      MDM_GLDS(b_src[j] + (size_t)(kt) * 128, (stage) + MX_A_BYTES + j * 4096 + wave_lds, 16);             \
    MDM_GLDS(sc_src + (size_t)(kt) * 4, (stage) + MX_A_BYTES + MX_B_BYTES + wave_sc, 4);                   \
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ktiles = p.Kp >> 7;
  const int ntiles = CONV ? 9 * ktiles : ktiles;
  int tap_n = 0, kk_n = 0;                           // CONV: the tap and the k-tile within it of the tile being staged
  if constexpr (CONV) MDM_SET_TAP(0);
  MDM_STAGE_TILE(smem, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA of tile 0 has landed before any wave reads it
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const char* cur = smem + (kt & 1) * MX_STAGE;
    if (kt + 1 < ntiles) {
      if constexpr (CONV) {
        if (++kk_n == ktiles) {
          kk_n = 0;
          ++tap_n;
          MDM_SET_TAP(tap_n);
        }
        MDM_STAGE_TILE(smem + ((kt + 1) & 1) * MX_STAGE, kk_n);
      } else {
        MDM_STAGE_TILE(smem + ((kt + 1) & 1) * MX_STAGE, kt + 1);
      }
    }
    const char* As = cur;
    const char* Bs = cur + MX_A_BYTES;
    const unsigned* sc = reinterpret_cast<const unsigned*>(cur + MX_A_BYTES + MX_B_BYTES);
    i32x8 af[4], bfr[4];
    int asc[4], bsc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ra = wm * 64 + i * 16 + l16, rb = wn * 64 + i * 16 + l16;
      // registers 0-3: k = 16 quad .. + 15, registers 4-7: k = 64 + 16 quad .. + 15 (the instruction's K map, see above)
      const i32x4 a0 = *reinterpret_cast<const i32x4*>(As + lds_chunk_off(ra, quad));
      const i32x4 a1 = *reinterpret_cast<const i32x4*>(As + lds_chunk_off(ra, 4 + quad));
      const i32x4 b0 = *reinterpret_cast<const i32x4*>(Bs + lds_chunk_off(rb, quad));
      const i32x4 b1 = *reinterpret_cast<const i32x4*>(Bs + lds_chunk_off(rb, 4 + quad));
      af[i] = i32x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      bfr[i] = i32x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      asc[i] = (int)((sc[ra] >> (8 * quad)) & 0xffu);
      bsc[i] = (int)((sc[MX_BM + rb] >> (8 * quad)) & 0xffu);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bfr[j], af[i], acc[i][j], 0, 0, 0, bsc[j], 0, asc[i]);
    // retire this wave's LDS-DMA of tile kt + 1 explicitly (as gemm_conv.hip does: the barrier alone is a compiler choice);
    // the barrier then publishes it and fences the reads of tile kt
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#undef MDM_STAGE_TILE
#undef MDM_SET_TAP
#undef MDM_GLDS

  // ---- epilogue: bf16(acc + bias) staged through LDS as rows of the output tile (a lane owns 4 consecutive channels of
  // one pixel: 8-byte writes), read back as 16-byte chunks of complete rows -> GELU -> + residual -> bf16 / MXFP8
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = wn * 64 + j * 16 + quad * 4;
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && n0 + nl < p.N) b = *reinterpret_cast<const f32x4*>(p.bias + n0 + nl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ml = wm * 64 + i * 16 + l16;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16)(acc[i][j][e] + b[e]);
      *reinterpret_cast<bf16x4*>(smem + ml * MX_PITCH + nl * 2) = o;
    }
  }
  __syncthreads();
  constexpr int NCH = MX_BM * 16 / 256;   // staged chunks per thread
  uint4 raw[NCH], rr[NCH];
  const bool has_res = p.res != nullptr;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int idx = tid + i * 256;
    const int row = idx >> 4, ch = idx & 15;
    raw[i] = *reinterpret_cast<const uint4*>(smem + row * MX_PITCH + ch * 16);
    const int m = m0 + row, n = n0 + ch * 8;
    rr[i] = uint4{0u, 0u, 0u, 0u};
    if (has_res && m < p.M && n < p.N) rr[i] = *reinterpret_cast<const uint4*>(p.res + (size_t)m * p.N + n);
  }
  const int np = tiles_n * MX_BN;         // EMIT: the padded width of the emitted rows (the next GEMM's Kp)
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int idx = tid + i * 256;
    const int row = idx >> 4, ch = idx & 15;
    const int m = m0 + row, n = n0 + ch * 8;
    const bool inside = m < p.M && n < p.N;
    Chunk<bf16> c;
    c.load(reinterpret_cast<const bf16*>(&raw[i]));
    if (p.act == MDM_ACT_GELU) gelu_vec<bf16, 8>(c.v);
    if (has_res) {
      Chunk<bf16> r;
      r.load(reinterpret_cast<const bf16*>(&rr[i]));
#pragma unroll
      for (int e = 0; e < 8; ++e) c.v[e] += r.v[e];
    }
    if constexpr (!EMIT) {
      if (inside) c.store(p.y + (size_t)m * p.N + n);
    } else {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = n < p.N ? (float)(bf16)c.v[e] : 0.f;   // columns N .. np - 1 are padding: code 0, scale 127
      uint2 codes;
      unsigned sb;
      mx8_encode8(v, codes, sb);
      const unsigned sw = mx8_gather_scales(sb);
      if (m < p.M) {
        *reinterpret_cast<uint2*>(p.q_out + (size_t)m * np + n) = codes;
        if (ch == 0) *reinterpret_cast<unsigned*>(p.s_out + (size_t)m * (np >> 5) + (n0 >> 5)) = sw;
      }
    }
  }
}

}  // namespace mdm

using namespace mdm;

// (models/unet.py:296-313: the operands of the qkv / proj_out / FFN projections in MXFP8)
// rows 0 .. Msrc - 1 from x, rows Msrc .. Mout - 1 zero (code 0, scale 127)
static int mx8_quant_launch(const void* x, int dtype, int Msrc, int Mout, int K, int Kp, void* q_out, void* s_out, void* stream) {
  MDM_CHECK_ARG(x != nullptr && q_out != nullptr && s_out != nullptr);
  MDM_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16);
  MDM_CHECK_ARG(Msrc >= 1 && Mout >= Msrc && K >= 8 && K % 8 == 0 && Kp == (K + 127) / 128 * 128);
  const int M = Mout;
  const size_t total = (size_t)M * (size_t)(Kp / 8);
  const size_t nb = (total + 255) / 256;
  MDM_CHECK_ARG(nb < (size_t)1 << 31);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(mx8_quant_kernel<bf16>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16*)x, (unsigned char*)q_out,
                       (unsigned char*)s_out, M, Msrc, K, Kp);
  else
    hipLaunchKernelGGL(mx8_quant_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)x, (unsigned char*)q_out,
                       (unsigned char*)s_out, M, Msrc, K, Kp);
  MDM_LAUNCH_STATUS();
}

extern "C" int mdm_mx8_quant(const void* x, int dtype, int M, int K, int Kp, void* q_out, void* s_out, void* stream) {
  return mx8_quant_launch(x, dtype, M, M, K, Kp, q_out, s_out, stream);
}

// (models/unet.py:223-238: the activation of conv1 / conv2 with the zero row its out-of-image taps read, in the same launch)
extern "C" int mdm_mx8_quant_zrow(const void* x, int dtype, int M, int K, int Kp, void* q_out, void* s_out, void* stream) {
  MDM_CHECK_ARG(M >= 1 && M < INT_MAX);
  return mx8_quant_launch(x, dtype, M, M + 1, K, Kp, q_out, s_out, stream);
}

// (models/unet.py:296-313: qkv :298, proj_out :310, the FFN pair :311-312)
extern "C" int mdm_mx8_gemm(const void* qa, const void* sa, const void* qw, const void* sw, const float* bias,
                            const void* residual, void* y, void* q_out, void* s_out, int M, int N, int Kp, int act,
                            void* stream) {
  MDM_CHECK_ARG(qa != nullptr && sa != nullptr && qw != nullptr && sw != nullptr);
  MDM_CHECK_ARG(M >= 1 && N >= 32 && N % 32 == 0 && Kp >= 128 && Kp % 128 == 0);
  MDM_CHECK_ARG(act == MDM_ACT_NONE || act == MDM_ACT_GELU);
  const bool emit = q_out != nullptr;
  MDM_CHECK_ARG(emit ? (s_out != nullptr && y == nullptr) : (y != nullptr && s_out == nullptr));
  const size_t tiles = (size_t)((M + MX_BM - 1) / MX_BM) * (size_t)((N + MX_BN - 1) / MX_BN);
  MDM_CHECK_ARG(tiles < (size_t)1 << 31);
  Mx8GemmArgs p;
  p.qa = (const unsigned char*)qa; p.sa = (const unsigned char*)sa;
  p.qw = (const unsigned char*)qw; p.sw = (const unsigned char*)sw;
  p.bias = bias; p.res = (const bf16*)residual; p.y = (bf16*)y;
  p.q_out = (unsigned char*)q_out; p.s_out = (unsigned char*)s_out;
  p.M = M; p.N = N; p.Kp = Kp; p.act = act; p.H = p.W = 0;
  hipStream_t st = (hipStream_t)stream;
  if (emit) {
    ensure_dynamic_lds(mx8_gemm_kernel<true, false>, MX_SMEM);
    hipLaunchKernelGGL((mx8_gemm_kernel<true, false>), dim3((unsigned)tiles), dim3(256), MX_SMEM, st, p);
  } else {
    ensure_dynamic_lds(mx8_gemm_kernel<false, false>, MX_SMEM);
    hipLaunchKernelGGL((mx8_gemm_kernel<false, false>), dim3((unsigned)tiles), dim3(256), MX_SMEM, st, p);
  }
  MDM_LAUNCH_STATUS();
}

// (models/unet.py:223-238: conv1 :225 and conv2 :236 of ResNet, stride 1, zero padding 1)
extern "C" int mdm_mx8_conv3x3(const void* qa, const void* sa, const void* qw, const void* sw, const float* bias,
                               const void* residual, void* y, int N, int H, int W, int Cin, int Cout, void* stream) {
  MDM_CHECK_ARG(qa != nullptr && sa != nullptr && qw != nullptr && sw != nullptr && y != nullptr);
  MDM_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && Cin >= 32 && Cin % 32 == 0 && Cout >= 32 && Cout % 32 == 0);
  const size_t pixels = (size_t)N * (size_t)H * (size_t)W;
  // a shifted row index m + dy W + dx and the zero row M are formed in int
  MDM_CHECK_ARG(pixels + (size_t)W + MX_BM + 1 < (size_t)INT_MAX && (size_t)Cout * 9 < (size_t)INT_MAX);
  const int M = (int)pixels;
  const size_t tiles = (size_t)((M + MX_BM - 1) / MX_BM) * (size_t)((Cout + MX_BN - 1) / MX_BN);
  MDM_CHECK_ARG(tiles < (size_t)1 << 31);
  Mx8GemmArgs p;
  p.qa = (const unsigned char*)qa; p.sa = (const unsigned char*)sa;
  p.qw = (const unsigned char*)qw; p.sw = (const unsigned char*)sw;
  p.bias = bias; p.res = (const bf16*)residual; p.y = (bf16*)y;
  p.q_out = nullptr; p.s_out = nullptr;
  p.M = M; p.N = Cout; p.Kp = (Cin + 127) / 128 * 128; p.act = MDM_ACT_NONE; p.H = H; p.W = W;
  ensure_dynamic_lds(mx8_gemm_kernel<false, true>, MX_SMEM);
  hipLaunchKernelGGL((mx8_gemm_kernel<false, true>), dim3((unsigned)tiles), dim3(256), MX_SMEM, (hipStream_t)stream, p);
  MDM_LAUNCH_STATUS();
}
