/* libmdm_hip -- development / profiling aids.  NOT part of the drop-in boundary (include/mdm_hip.h): nothing here
 * replaces a reference call site; bench.py and tools/ use these to label per-launch timings. */
#ifndef MDM_HIP_DEV_H_
#define MDM_HIP_DEV_H_
#ifdef __cplusplus
extern "C" {
#endif

/* name (as a profiler prints it, without arguments) of the GEMM-class kernel the calling thread launched last */
const char* mdm_last_gemm_kernel(void);
/* host-only: block tile (BM * 1000 + BN) mdm_conv_fwd will use for (M, Cout, dtype) */
int mdm_conv_fwd_tile(int M, int Cout, int dtype);
/* host-only: 128 or 256 (square output tile edge) mdm_conv_wgrad will use */
int mdm_conv_wgrad_tile(int M, int Cout, int K, int dtype);

/* development knobs of the GEMM kernels (0 in the product; host-side state of the calling process, never read from the
 * environment inside an entry point).  Any other index is an argument error.
 *   0  1 = the LDS-DMA of conv_gemm_bl_kernel fetches nothing (timing only: what the k-loop costs without memory).  Its
 *      uniform branch also keeps the compiler's register allocation of the 3x3 instantiations (see conv_args.hpp)
 *   2  force the forward tile of conv_gemm_bl_kernel (128128 / 256192 / 256256; tools/kbench.py KB_TILE)
 *   3  force the weight-gradient tile edge (128 / 256, 0 = cost model) wherever the kernel of that edge is eligible (256:
 *      bf16, Cout >= 192 and K >= 192; elsewhere the cost model still decides).  Read by the one function behind
 *      mdm_conv_wgrad_plan, mdm_conv_wgrad_tile, the launch and the workspace size, and by the grouped launch's tile
 *      choice, so they stay consistent; set it before the plan call and leave it until after mdm_conv_wgrad_reduce.  Any
 *      other value is an argument error (tests/conv_variant_cases.py: the 256-edge kernels at test size)
 *   8  1 = the narrow weight gradients (64 output channels, >= 262144 pixels) go back to the split GEMM (no wgrad_direct_kernel:
 *      the reference of tests/test_ops_gpu.py's direct-kernel test) */
int mdm_dev_set_knob(int idx, int value);
/* attention backward kernel choice: 0 = by shape, 1 = always the split (dQ + dK/dV) kernels on 16x16x32 MFMAs, 2 = the
 * one-block-per-head kernel whenever the shape allows (tests), 3 = as 2 but the 16x16x32 one, 4 = the streaming kernels on
 * 32x32x16 MFMAs (csrc/attn32.hpp) whenever the shape allows */
int mdm_dev_set_attn_bwd(int mode);
/* names of the kernel(s) the calling thread's last mdm_attn_fwd / mdm_attn_bwd launched, as "attn_fwd_kernel<bf16,96,2>"; a
 * two-kernel backward is joined with '+'.  Written where the launch is made, so a knob that the shape does not allow shows as
 * the kernel that ran instead (tests/attn_variant_cases.py) */
const char* mdm_last_attn_kernel(void);
/* queries per wave of the bf16 attention forward: 0 = by shape and CU count (the product), 1 = always 16 (QT = 1), 2 = always
 * 32 (QT = 2).  The fp32 and DT_F32_SPLIT forwards have one instantiation and ignore it.  Any other value is -1 */
int mdm_dev_set_attn_fwd(int mode);
/* GroupNorm backward, two-kernel path (images too large for the register-resident kernel): bytes of x + dy, in MiB,
 * above which the batch is walked in chunks of samples so that the second kernel's reads still find them in the Infinity
 * Cache (default 160; 0 = chunk whenever the batch allows it -- the tests; negative = never) */
int mdm_dev_set_gn_chunk_mb(int mb);
/* bytes per element of the operand a bf16 MDM_ACT_GELU launch leaves for its backward: 1 (the product: the byte code of
 * gelu', include/mdm_hip.h) or 2 (a variant library built with -DMDM_FFN_AUX_BF16 for in-call A/B: the bf16 pre-activation) */
int mdm_dev_ffn_aux_bytes(void);
/* phase time stamps of attn_bwd_small32_kernel: a device buffer of [blocks][8][16] 64-bit words (tools/attn_debug.py), or
 * null (the default) */
int mdm_dev_set_attn_dbg(void* buf);
/* one launch of mdm_abs_quantile (include/mdm_hip_ext.h) by itself, for the rate of each level (tools/thr_bench.py): stage 0 =
 * the zeroing of the workspace, 1 .. 3 = the pass of that level, on a workspace in the state the stages before it left.
 * Arguments and checks as mdm_abs_quantile. */
int mdm_dev_abs_quantile_stage(const float* x, void* ws, size_t ws_bytes, int B, size_t n, float q, int stage, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_DEV_H_ */
