/* libmdm_hip -- entry points beyond the drop-in boundary (include/mdm_hip.h): capabilities the reference does not have
 * and that replace none of its call sites.  Same conventions as mdm_hip.h (return 0 or a negative code, mdm_last_error(),
 * dtype codes, a hipStream_t as void*); pure additions, so MDM_HIP_ABI_VERSION is untouched. */
#ifndef MDM_HIP_EXT_H_
#define MDM_HIP_EXT_H_
#ifdef __cplusplus
extern "C" {
#endif

/* mdm_attn_cross_bias -- the text cross-attention term with an additive bias on its logits, added onto `base`: what
 * regional prompts ("a red car" on the left) and token weights ("(snow:1.4)" = bias log 1.4) come to on this model, where
 * the text term is a softmax of its own over the S text keys (mdm_attn_fwd).
 *   out[b, l, :] = base[b, l, :] + softmax_s( q . k_c / sqrt(d) + bias[b, l, s] ; live keys ) v_c        [B, L, C], C = H * d
 * qkv [B, L, 3C] (only q is read, unless base points into it), kvc [B, S, 2C] and mask [B, S] of 0/1 floats or NULL as
 * for mdm_attn_cross_addv.  bias: fp32 [B, L, bias_ld], bias_ld >= S and bias_ld % 4 == 0, 16-byte aligned, shared by all
 * heads; columns [S, bias_ld) are never used and may hold anything.  A key is live where mask != 0 and bias > -1e30:
 * a bias <= -1e30 (-inf included; NaN too) excludes the key exactly as mask == 0 does.  (A finite bias below about
 * -6.9e29 is out of the exponent's range and also counts as excluded.)  A query with no live key gets base bit for bit.
 * base: [B, L, base_ld] of the compute dtype, base_ld >= C and % 4 == 0 -- base == out with base_ld == C adds in place
 * (onto the self part that mdm_attn_fwd with kvc == NULL wrote); base == v of qkv with base_ld == 3C gives the perturbed
 * rows of perturbed-attention guidance.  base may alias out exactly (every lane reads its elements before it stores
 * them), not overlap it otherwise.  Scores, softmax and accumulation in fp32; d in {32, 64, 96, 128}, any S >= 1.
 * dtype: MDM_F32, MDM_BF16, or MDM_F32_SPLIT, which runs the exact-fp32 products.  With a zero bias and base == v the
 * result is mdm_attn_cross_addv's bit for bit.  No workspace, no atomics, deterministic, forward only. */
int mdm_attn_cross_bias(const void* qkv, const void* kvc, const float* mask, const float* bias, int bias_ld,
                        const void* base, int base_ld, void* out, int B, int L, int S, int H, int d, int dtype,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_EXT_H_ */
