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

/* mdm_attn_cross_maps -- the probabilities of that text cross-attention term, averaged over the heads and accumulated:
 *   acc[b, l, s] += w / H * sum_h softmax_s( q_h . k_c,h / sqrt(d) (+ bias[b, l, s]) ; live keys )       w = w_host * (*w_dev)
 * what mdm_attn_fwd / mdm_attn_cross_addv / mdm_attn_cross_bias multiply into v_c and never write: per-token heat maps.
 * qkv [B, L, 3C] (only q is read), kvc [B, S, 2C] (only k_c is read), mask [B, S] of 0/1 floats or NULL, bias as for
 * mdm_attn_cross_bias or NULL (fp32 [B, L, bias_ld], bias_ld >= S and % 4 == 0, 16-byte aligned; columns [S, bias_ld)
 * are never used and may hold anything).  A key is live where mask != 0 and bias > -1e30; a query with no live key adds 0.
 * acc: fp32 [B, L, acc_ld], query-major like the bias, acc_ld >= S and % 4 == 0, 16-byte aligned; columns [S, acc_ld)
 * are neither read nor written.  w_dev: a device float or NULL (= 1); w == 0 launches blocks that return before they
 * load anything, acc untouched bit for bit -- one captured graph serves a trajectory in which only some steps record.
 * The exponent is that of the sister kernels ((s c2) rounded, + bias log2(e), - max), so a single live key has
 * probability exactly 1; the probabilities are fp32 in every mode and scaled by nothing but w / H.  dtype: MDM_F32,
 * MDM_BF16, or MDM_F32_SPLIT, which runs the exact-fp32 products; d in {32, 64, 96, 128}, H <= 64, any L, any S >= 1.
 * One launch: the heads are looped inside the block and every acc element is read once and written once by the lane that
 * owns it.  No workspace, no atomics, deterministic, a batch row's result independent of B, forward only. */
int mdm_attn_cross_maps(const void* qkv, const void* kvc, const float* mask, const float* bias, int bias_ld, float* acc,
                        int acc_ld, float w_host, const float* w_dev, int B, int L, int S, int H, int d, int dtype,
                        void* stream);

/* mdm_attn_cross_maps_bwd -- the gradient of those maps with respect to q (attention-map guidance: a loss on the maps,
 * Attend-and-Excite for one, moves x_t).  With dacc = d loss / d acc of one mdm_attn_cross_maps launch of weight w:
 *   P_h        = the probabilities exactly as mdm_attn_cross_maps forms them, without a bias (the same exponent,
 *                (s c2) rounded and then - max; a key is live where key < S and mask != 0)
 *   delta_h[l] = sum_s P_h[l, s] dacc[b, l, s]
 *   dS_h       = P_h o (dacc - delta_h)
 *   dq[b, l, h d + c] = w / (H sqrt(d)) sum_s dS_h[l, s] k_c[b, s, h d + c]
 * (w / H is applied once, to the finished sum, so dacc enters the products unscaled.)
 * qkv [B, L, 3C] (only q is read), kvc [B, S, 2C] (only k_c is read), mask [B, S] of 0/1 floats or NULL.  dacc: fp32
 * [B, L, dacc_ld], query-major like acc, dacc_ld >= S and % 4 == 0, 16-byte aligned; its columns [S, dacc_ld) and the
 * entries of keys that are not live are selected away, never computed on: they may hold NaN.  dq: the compute dtype, row
 * (b, l) at dq + b * dq_bs + l * dq_rs elements, C of them written (dq_rs >= C, dq_rs and dq_bs % 4 == 0, dq aligned to
 * four elements): dq_rs = 3C, dq_bs = L * 3C writes straight into the q columns of a qkv-shaped gradient, and nothing
 * outside those columns is touched.  A query with no live key gets exact zeros; a single live key gives exact zeros too.
 * No bias: a biased map has no backward here.  Gradients to k_c are not formed.
 * dtype: MDM_F32, MDM_BF16 (dS rounded to bf16 for the second product, as the attention backward does), or MDM_F32_SPLIT,
 * which runs the exact-fp32 products; accumulation in fp32; d in {32, 64, 96, 128}, any L, any S >= 1, any H with
 * B * H <= 65535.  One block per 64 queries of one (batch, head): S <= 64 is one key tile with everything in registers,
 * beyond that two sweeps over the key tiles.  Every dq element is written once by the lane that owns it: no workspace, no
 * atomics, deterministic, a batch row's result independent of B.  Invalid arguments: a negative status, nothing launched. */
int mdm_attn_cross_maps_bwd(const void* qkv, const void* kvc, const float* mask, const float* dacc, int dacc_ld, float w,
                            void* dq, size_t dq_bs, int dq_rs, int B, int L, int S, int H, int d, int dtype, void* stream);

/* FreeU (Si et al., CVPR 2024) fused into the up path's skip concat: backbone h [N, H, W, C1], skip r [N, H, W, C2], NHWC,
 * of dtype MDM_F32 or MDM_BF16 (the fp32-split mode has fp32 tensors: MDM_F32), arithmetic in fp32 ->
 *   out[.., 0:C1/2]   = h[.., :C1/2] * m       m = b, or with `structure` (FreeU v2)  1 + (b - 1) hm[n, y, x],
 *                                              hm = (mu - min mu) / (max mu - min mu), mu = mean of h over all C1 channels,
 *                                              min / max over the pixels of sample n; max == min: hm = 1 (m = b)
 *   out[.., C1/2:C1]  = h[.., C1/2:]           bit for bit
 *   out[.., C1:C1+C2] = r + (s - 1) / (H W) * sum_k coef_k[n, c] phi_k(y, x),   coef_k = sum_{y, x} r phi_k,
 *       phi = {1, cos t1, sin t1, cos t2, sin t2, cos t3, sin t3}, t1 = 2 pi y / H, t2 = 2 pi x / W, t3 = t1 + t2
 * -- the Fourier filter of the paper at threshold 1 (rows H/2 - 1 .. H/2 and columns W/2 - 1 .. W/2 of the shifted
 * spectrum scaled by s) in closed form; exact for H, W >= 2.  s == 1 copies r bit for bit, b == 1 copies h bit for bit.
 * Limits: H, W >= 2, H + W <= 1024, N <= 65535, C1 % 16 == 0 and C2 % 8 == 0 for bf16, C1 % 8 == 0 and C2 % 4 == 0 for
 * fp32; b finite and > 0, s finite and >= 0.
 * mdm_freeu_plan (host-only): the bytes of the fp32 workspace both launches share.
 * mdm_freeu_stats: reads r once -> coef [N, 7, C2] in ws (per-slab partials summed in slab order); with `structure`
 *   reads h once -> mu [N, H W] and the per-sample min / max in ws.  h may be NULL without `structure`.
 * mdm_freeu_apply: mdm_concat's forward with both transforms, from the ws that mdm_freeu_stats filled for the same
 *   tensors and the same `structure`.  out must not alias h or r.
 * No allocation, no host sync, no atomics: capturable, and two runs are bit-identical.  Forward only. */
int mdm_freeu_plan(int N, int H, int W, int C1, int C2, int dtype, int structure, size_t* ws_bytes);
int mdm_freeu_stats(const void* h, const void* r, void* ws, size_t ws_bytes, int N, int H, int W, int C1, int C2,
                    int structure, int dtype, void* stream);
int mdm_freeu_apply(const void* h, const void* r, const void* ws, size_t ws_bytes, void* out, int N, int H, int W, int C1,
                    int C2, float b, float s, int structure, int dtype, void* stream);

/* Projected and rescaled classifier-free guidance: the combine in front of mdm_sampler_step / mdm_sampler_step_2m, which
 * then get pred_uncond = NULL and guidance = 1 (the place of mdm_pag_combine).  APG (Sadat, Hilliges, Weber, ICLR 2025),
 * CFG rescale (Lin, Liu, Li, Yang, WACV 2024, section 3.4) and the guidance interval (Kynkaanniemi et al., NeurIPS 2024)
 * as a device gate.  fp32 [B, chw] tensors, gamma [B]; per sample, with x0 = a x_t + be p (pred_type 2, V: a = sqrt(g),
 * be = -sqrt(1 - g); 0 / 1, eps: a = 1 / sqrt(g), be = -sqrt(1 - g) / sqrt(g)):
 *   D = a x_t + be p_c ;  E = be (p_c - p_u) + momentum run_prev  (run_prev taken as 0 where it is NULL or run_gate is off)
 *   run_out = E   (before the cap)
 *   s = min(1, norm_threshold / (image_scale sqrt(<E, E> / chw)))   (norm_threshold == 0, or a zero E: s = 1)
 *   c = <E, D> / <D, D>   (<D, D> == 0: c = 0)
 *   p_g = p_c + (guidance - 1) s (E - (1 - eta) c D) / be
 *   out = p_g (rescale std(p_c) / std(p_g) + 1 - rescale)   (population std over chw; rescale == 0 or std(p_g) == 0: out = p_g)
 * eta = 1, norm_threshold = 0, no run buffers and rescale = 0: plain classifier-free guidance up to rounding.
 * norm_threshold caps the RMS of the update in IMAGE units (the paper's L2 radius r = norm_threshold sqrt(chw)), so one
 * value serves every scale of a nested model.  be == 0 (gamma == 1): out = p_c.
 * run_gate, w_gate: DEVICE float[1], NULL = on; they select.  run_gate off: run_prev is not read.  w_gate off (outside the
 * guidance interval): out = p_c bit for bit, x_t / p_u / ws are not read, and the history passes through -- run_out =
 * run_prev bit for bit (0 where run_gate is off too).  So one captured graph serves a whole trajectory.
 * mdm_cfg_plan (host-only): the bytes of the fp32 workspace both launches share -- per sample and per slab of the image 3
 *   sums, 9 with the rescale (the Gram matrix of (p_c, E, D) and their plain sums: the variance of p_g follows from them,
 *   there is no second pass over the images).
 * mdm_cfg_stats: reads x_t, p_c, p_u (and run_prev) once; writes the per-slab sums and, if run_out is given, E.  run_out may
 *   alias run_prev, nothing else.  run_out == NULL: no momentum (run_prev must be NULL too).  |momentum| < 1.
 * mdm_cfg_combine: adds every sample's slab sums in a fixed order in fp64, forms the coefficients in fp64 and writes out.
 *   `run`: the run_out that mdm_cfg_stats wrote for this step (E is read from it, pred_uncond is not read), or NULL (E is
 *   formed from pred_uncond again).  Same tensors, gates, gamma, B, chw, pred_type and rescale > 0 as the statistics call.
 *   out may alias pred, nothing else.  rescale in [0, 1], norm_threshold >= 0, image_scale > 0, eta and guidance finite.
 * Limits: chw % 4 == 0, 1 <= B <= 65535, 16-byte aligned tensors.  The slab geometry depends on chw alone: a sample's result
 * does not depend on the rest of the batch.  No allocation, no host sync, no atomics: capturable, and two runs are
 * bit-identical. */
int mdm_cfg_plan(int B, size_t chw, int rescale_on, size_t* ws_bytes);
int mdm_cfg_stats(const float* x_t, const float* pred, const float* pred_uncond, const float* gamma, const float* run_prev,
                  float* run_out, const float* run_gate, const float* w_gate, float momentum, int rescale_on, void* ws,
                  size_t ws_bytes, int B, size_t chw, int pred_type, void* stream);
int mdm_cfg_combine(const float* x_t, const float* pred, const float* pred_uncond, const float* gamma, const float* run,
                    const float* w_gate, const void* ws, size_t ws_bytes, float* out, float guidance, float eta,
                    float norm_threshold, float rescale, float image_scale, int B, size_t chw, int pred_type, void* stream);

/* Tiled sampling (MultiDiffusion, Bar-Tal et al., ICML 2023): the denoiser of a step runs on overlapping windows of a canvas
 * larger than its training size, and the windows' predictions are averaged where they overlap.  fp32 NCHW tensors.
 * Geometry, per axis (canvas L, window win, stride s): n = ceil((L - win) / s) + 1 windows at offsets min(i s, L - win) --
 * the last one is clamped to the border.  ny x nx windows, window k = i nx + j, T = ny nx.
 * mdm_tiles_gather: x [B, C, H, W] -> out [reps, B, T, C, h, w]; row (rep B + b) T + k is window k of image b, the same for
 *   every rep (the blocks [uncond | cond | perturbed] of the model batch).  Every element is a copy, bit for bit.
 * mdm_tiles_merge: p [R, T, C, h, w] -> out [R, C, H, W],
 *     out[r, c, y, x] = sum_k wt_k p[r, k, c, y - oy_k, x - ox_k] / sum_k wt_k     over the windows k that contain (y, x),
 *   accumulated in fp32 in window order (i ascending, then j).  blend 0 (uniform): wt = 1.  blend 1 (ramp): at position
 *   (a, b) of the window wt = min(a + 1, h - a) min(b + 1, w - b), a tent; needs ceil(h / 2) ceil(w / 2) <= 2^24.  A pixel
 *   under exactly one window gets that window's value bit for bit.  out must not alias p.  R is the whole model batch.
 * Both: 1 <= h <= H, 1 <= w <= W, 1 <= sy <= h, 1 <= sx <= w (so every pixel lies under a window), reps >= 1, B, R, T <=
 * 65535, C H W < 2^31.  The windows over a pixel are found by arithmetic on (y, x, h, w, sy, sx, H, W): no offset table.
 * 16-byte accesses where w, W, sx and W - w are multiples of 4 and both tensors are 16-byte aligned, 4-byte ones otherwise.
 * No allocation, no workspace, no host sync, no atomics: capturable, two runs are bit-identical, and a row's bits do not
 * depend on the rows beside it.  Invalid arguments: a negative status, nothing launched.  Forward only. */
int mdm_tiles_gather(const float* x, float* out, int B, int C, int H, int W, int h, int w, int sy, int sx, int reps,
                     void* stream);
int mdm_tiles_merge(const float* p, float* out, int R, int C, int H, int W, int h, int w, int sy, int sx, int blend,
                    void* stream);

/* The per-sample threshold of the dynamic threshold functions: thr[b] = clamp(quantile_q |x[b, :]|, cmin, cmax), the
 * quantile by torch.quantile's rule, found exactly by a radix select on the bit patterns of the magnitudes -- no sort, and
 * no limit of 2^24 values per row.  x: fp32 [B, n], contiguous.  For a row, with a = |x| sorted ascending:
 *   rank = q (n - 1) IN FP32 ;  lo = floor(rank) ;  hi = min(ceil(rank), n - 1) ;  w = rank - lo
 *   quant = w < 0.5 ? a[lo] + w (a[hi] - a[lo]) : a[hi] - (a[hi] - a[lo]) (1 - w) ;  thr = clamp(quant, cmin, cmax)
 * (above 2^24 the fp32 rank is an integer: lo == hi, w == 0; the rule is the same).  A row that holds a NaN: thr = NaN.  +-inf
 * are ordinary largest values and the interpolation is applied as written (inf - inf: NaN, as torch); -0.0 counts as 0.
 * cmin = -inf, cmax = +inf: no clamp.  stats [B, 2] or NULL: a[lo] and a[hi] bit for bit (of a NaN, its pattern without the
 * sign).
 * The key bits(x) & 0x7fffffff orders as |x| does; the prefix that holds each of the two ranks is refined over three levels
 * of 12 + 11 + 8 bits, each one pass over x: block-private LDS histograms, merged into the row's histogram in ws with integer
 * atomics.  Only the first pass counts every element.  16-byte loads where n % 4 == 0 and x is 16-byte aligned, 4-byte loads
 * otherwise: same result.  Integer counts and an exact selection: a row's thr and stats depend on nothing but the row (not on
 * B, not on the other rows), and two runs are bit-identical.  No float atomics.
 * mdm_abs_quantile_plan (host-only): the bytes of ws -- per row 34 880 (the histograms of the three levels).
 * ws: 16-byte aligned; it may hold anything on entry (the entry zeroes what it needs in a launch of its own) and is free again
 * when the last launch has run.  Five launches for any B and n; no allocation, no host sync, no memset: capturable.
 * Limits: 1 <= n < 2^31, 1 <= B <= 65535, 0 <= q <= 1, cmin <= cmax.  Invalid arguments: a negative status, nothing launched. */
int mdm_abs_quantile_plan(int B, size_t n, size_t* ws_bytes);
int mdm_abs_quantile(const float* x, void* ws, size_t ws_bytes, int B, size_t n, float q, float cmin, float cmax, float* thr,
                     float* stats, void* stream);

/* Input gradients of the frozen T5 encoder (textual inversion: csrc/text_encoder_bwd.hip).  Packed tokens, dtypes and
 * tensors as the mdm_t5_* forward entries of mdm_hip.h: dtype MDM_F32 or MDM_BF16 is the storage type of the GEMM-operand
 * tensors (void*); the residual stream, its gradient, lse and the statistics are fp32.  No weight and no bias-table gradient.
 * No allocation, no workspace, no host sync, NO atomics: two runs are bit-identical, and the gradients of a sequence do not
 * depend on what else is in the batch.  Invalid arguments: a negative status, nothing launched.
 *   mdm_t5_attn_fwd_lse   mdm_t5_attn_fwd with one more output, lse fp32 [H, T]: the log of the softmax denominator per
 *                      (head, packed query), running max included.  out: the bits of mdm_t5_attn_fwd.
 *   mdm_t5_attn_bwd    qkv [T, 3 H 64], out and dout [T, H 64], lse -> dqkv [T, 3 H 64], every element written.  Per
 *                      (sequence, head):  P = exp(q k^T + bias[h][pos_k - pos_q + S - 1] - lse),  delta = rowsum(dout o out),
 *                      dV = P^T dout,  dS = P o (dout V^T - delta),  dQ = dS K,  dK = dS^T Q.  No 1 / sqrt(d).  Two launches
 *                      (a wave per 16 queries for dQ, a wave per 16 keys for dK and dV, each recomputing the scores);
 *                      products on MFMA, bf16 16x16x32 or exact fp32.  d == 64, S <= 512, rows of any length from 0 to S.
 *   mdm_t5_gated_gelu_bwd  u [T, 2F], dy [T, F] -> du [T, 2F]:  du[:, :F] = dy u[:, F:] gelu_new'(u[:, :F]),
 *                      du[:, F:] = dy gelu_new(u[:, :F])  (tanh form, the forward's constants).  F % 8 == 0.
 *   mdm_t5_rms_bwd     the input gradient of h = w o x rsqrt(mean(x^2) + eps), ADDED into the fp32 stream gradient:
 *                      dx[t] += rs (w o dh) - x rs^3 / D sum(w o dh o x), x the saved fp32 row [T, D], dh [T, D] of dtype.
 *                      dx_lo (dtype [T, D], or NULL): a copy of the updated dx, the operand of the next GEMM.
 *   mdm_t5_final_rms_bwd   the same for mdm_t5_final_rms: x + delta (delta may be NULL) is the normed row, the gradient of
 *                      packed row t is row flat[t] of dout fp32 [B S, D] (a gather), and dx[t] is WRITTEN.
 *   mdm_t5_embed_rms_slots  mdm_t5_embed_rms with an override: slot_of_id (int32 [n_ids], -1 or a row of learned fp32
 *                      [P, D]) is looked up first; a hit reads learned[slot] instead of table[id].  n_ids >= vocab; ids in
 *                      [vocab, n_ids) must hit a slot.  With no hit: the bits of mdm_t5_embed_rms.
 *   mdm_t5_embed_bwd   dlearned[j] = sum over k in [slot_start[j], slot_start[j + 1]) of dx0[tokens[k]], sequentially in
 *                      that order (the host lists a slot's packed tokens ascending); dx0 fp32 [T, D], tokens int32 [n],
 *                      slot_start int32 [P + 1].  Every slot is written, one without tokens with zeros.  D % 4 == 0. */
int mdm_t5_attn_fwd_lse(const void* qkv, const int* seq_start, const int* pos, const float* bias_table, void* out, float* lse,
                        int B, int T, int S, int max_len, int H, int d, int dtype, void* stream);
int mdm_t5_attn_bwd(const void* qkv, const void* out, const float* lse, const void* dout, const int* seq_start, const int* pos,
                    const float* bias_table, void* dqkv, int B, int T, int S, int max_len, int H, int d, int dtype,
                    void* stream);
int mdm_t5_gated_gelu_bwd(const void* u, const void* dy, void* du, int T, int F, int dtype, void* stream);
int mdm_t5_rms_bwd(const float* x, const float* ln_w, const void* dh, float* dx, void* dx_lo, int T, int D, float eps,
                   int dtype, void* stream);
int mdm_t5_final_rms_bwd(const float* x, const void* delta, const float* ln_w, const float* dout, const int* flat, float* dx,
                         void* dx_lo, int T, int D, float eps, int dtype, void* stream);
int mdm_t5_embed_rms_slots(const int* ids, const float* table, const int* slot_of_id, const float* learned, const float* ln_w,
                           float* x, void* h, int T, int D, int vocab, int n_ids, int P, float eps, int dtype, void* stream);
int mdm_t5_embed_bwd(const float* dx0, const int* slot_start, const int* tokens, float* dlearned, int P, int D, int n, int T,
                     void* stream);

/* mdm_sampler_step_sa -- one step of SA-Solver (Xue et al., NeurIPS 2023, "SA-Solver: Stochastic Adams Solver for Fast
 * Sampling of Diffusion Models") on fp32 NCHW [B, chw] images, per scale and per sample: an exponential Adams-Bashforth
 * predictor and an Adams-Moulton corrector on the data prediction, with a noise level tau between the probability-flow ODE
 * (tau = 0) and the reverse SDE (tau = 1).  alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda = log(alpha / sigma); a step
 * from node a (gamma) to node b (gamma_last), h = lambda_b - lambda_a > 0, kappa = 1 + tau^2; m_j the guided, thresholded x0
 * formed at node j (guidance combine, x0 and clip 0 / 1 / 2 exactly as mdm_sampler_step_2m); l_j the Lagrange basis over the
 * nodes' offsets s_j = lambda_j - lambda_a:
 *   x_b = (sigma_b / sigma_a) e^{-tau^2 h} x_a + alpha_b sum_j c_j m_j + sigma_b sqrt(-expm1(-2 tau^2 h)) z
 *   c_j = kappa int_0^h e^{-kappa (h - s)} l_j(s) ds                       (sum_j c_j = -expm1(-kappa h))
 * Predictor of order p <= 3: nodes a, a-1, .., a-p+1.  Corrector of order k <= 3: the step a-1 -> a once more, now that m_a
 * is known, over nodes a, .., a-k+1 with the same x_{a-1} term and the same noise -- so it is a difference,
 *   x_a <- x_a - psum_a + alpha_a sum_j c^c_j m_j,      psum_a = alpha_a sum_j c^p_j m_j  stored by the launch before,
 * and whatever was done to x_a after that launch (a known-region blend) survives it.  One launch at node a:
 *   m_a from (x_t, pred) ; correct x_t ; predict x_b -> x_last_out ; psum <- psum_b ; h1 <- h0, h0 <- m_a ; x0_out <- m_a
 * h0 / h1: m_{a-1} / m_{a-2}, formed at gamma_h0 / gamma_h1 ([B] each).  h0, h1 and psum are updated IN PLACE; a thread reads
 * its elements before it writes them, and x0_out may be h0 itself.  x_last_out aliases nothing.
 * gate: DEVICE float[4] = {predictor order, corrector order, tau, tau of the step the corrector redoes}, so that one captured
 * graph serves every step.  (The fourth entry is there because tau may differ between neighbouring steps, tau_interval, and the
 * corrector's coefficients belong to the step before.)  The orders are clamped to [1, max_predictor] and [0, max_corrector],
 * the host's ceilings, which also say which buffers must be given: gamma_h0 for max_predictor >= 2 or max_corrector >= 1, h0
 * for either >= 2, h1 and gamma_h1 for either >= 3, psum for max_corrector >= 1 (NULL otherwise: then not written either).
 * The gate SELECTS: history and gammas behind an order that is off are not read, NaN in them reaches no output.
 * A sample with gamma_last == 1 (the last step, h = inf) takes predictor order 1, tau = 0 and no corrector whatever the gate
 * says: x_last_out = x0_out = m_a bit for bit, no logarithm is evaluated, no history is read, no normal is drawn.
 * z: noise[] if given, else drawn in the kernel from rng_state / rng_stream (Philox, element i as mdm_sampler_step and
 * mdm_randn; the caller advances the state); with neither, tau counts as 0.  With tau == 0 neither is read.
 * Coefficients: on the device, in fp64, once per block (a block works on one sample): lambda differences as
 * log1p((g_b - g_a) / (g_a (1 - g_b))) / 2, the moments of the integral by their series below kappa h = 1 and by the recurrence
 * phi_n = 1 - (n / x) phi_{n-1} above -- 1e-6 relative or better against quadrature for h in [1e-4, 8].
 * chw % 4 == 0, 16-byte accesses, no allocation, no workspace, no host sync, no atomics: capturable, two runs are bit-identical,
 * and a row's bits do not depend on the rows beside it.  Invalid host arguments (a ceiling outside 1..3 / 0..3, a missing or
 * aliased buffer): a negative status, nothing launched.  What lives on the device is not checked: gamma_last > gamma is the
 * caller's to keep wherever the sample is not on its last step. */
int mdm_sampler_step_sa(const float* x_t, const float* pred, const float* pred_uncond, float guidance, const float* gamma,
                        const float* gamma_last, const float* gamma_h0, const float* gamma_h1, const float* gate,
                        const float* thr, const float* noise, const unsigned long long* rng_state, int rng_stream, float* h0,
                        float* h1, float* psum, float* x0_out, float* x_last_out, int B, size_t chw, int pred_type, int clip,
                        float image_scale, int max_predictor, int max_corrector, void* stream);

/* Image inversion: taking a GIVEN image back to the noise that reproduces it, on fp32 NCHW [B, chw] images, per scale and per
 * sample.  alpha = sqrt(gamma), sigma = sqrt(1 - gamma); p = pred_uncond ? pred_uncond + guidance (pred - pred_uncond) : pred.
 *
 * mdm_sampler_invert_step -- the preimage of one DDIM(0) step with the prediction held fixed: from x_s at the CLEANER node
 * (gamma_s > gamma_t) the x_t for which mdm_sampler_step(mode 1, eta 0, clip 0) with the same p returns x_s,
 *   pred_type 0, 1 (eps):  x_t = (alpha_t / alpha_s) (x_s - sigma_s p) + sigma_t p
 *   pred_type 2 (v):       x_t = (x_s - (sigma_s alpha_t - alpha_s sigma_t) p) / (alpha_s alpha_t + sigma_s sigma_t)
 * DDIM inversion with fixed-point refinement (Song et al. 2021; Pan et al. 2023; Garibi et al. 2024) evaluates p at the
 * iterate and applies this to the same x_s again.  The small coefficients are formed without cancellation:
 * sigma_s alpha_t - alpha_s sigma_t = (gamma_t - gamma_s) / (sigma_s alpha_t + alpha_s sigma_t), and for eps the coefficient
 * of p is (gamma_s - gamma_t) / ((sigma_t alpha_s + alpha_t sigma_s) alpha_s).  gamma_s == 1 (the image itself) is allowed;
 * gamma_t < 1.  No threshold: a clamp has no inverse.  x_t_out aliases nothing.
 *
 * mdm_sampler_noise_map -- the noise of one ancestral step solved for (edit-friendly DDPM inversion, Huberman-Spiegelglas et
 * al. 2024): z = (x_s - mu) / sigma, where mu is what mdm_sampler_step computes from (x_t, p) before it adds noise -- the same
 * guidance combine, x0, clip 0 / 1 / 2 (2: thr[b], from mdm_sampler_step(clip 3) and mdm_abs_quantile) and mode 0 / 1, by the
 * same device functions -- and sigma its noise factor, so that mdm_sampler_step(noise = z) maps x_t to x_s.  A sample whose
 * sigma is 0 (gamma_last == 1) gets z = 0.  mode 1 needs ddim_eta > 0.  z_out aliases nothing.
 *
 * Both: chw % 4 == 0, 16-byte accesses, one vec4 per thread with a grid stride, no allocation, no workspace, no host sync,
 * no atomics: capturable, two runs are bit-identical, and a row's bits do not depend on the rows beside it.  Invalid host
 * arguments: a negative status, nothing launched. */
int mdm_sampler_invert_step(const float* x_s, const float* pred, const float* pred_uncond, float guidance,
                            const float* gamma_s, const float* gamma_t, float* x_t_out, int B, size_t chw, int pred_type,
                            void* stream);
int mdm_sampler_noise_map(const float* x_t, const float* x_s, const float* pred, const float* pred_uncond, float guidance,
                          const float* gamma, const float* gamma_last, const float* thr, float* z_out, int B, size_t chw,
                          int pred_type, int mode, float ddim_eta, int clip, float image_scale, void* stream);

/* Prompt-to-prompt attention control (Hertz et al. 2022): an EDITED batch row r computes with the attention maps of its
 * SOURCE row s.  The text term of mdm_attn_fwd is a softmax of its own over the S text keys, so mixing its probabilities
 * over the token axis is linear in v_c -- (P_s M) v_c = P_s (M v_c) -- and the controlled layer is
 *   out_h[r] = A_h(g_s ? s : r) v_h[r] + P_h(s) V'_h[r] + P_h(r) V''_h[r]
 *   V'[r][i, :]  = g_c sum_{j live in r} M[r][i, j] v_c[r][j, :]     (i: a source token, j: an edit token; live: mask != 0)
 *   V''[r][j, :] = (g_c D[r][j] + 1 - g_c) v_c[r][j, :]
 * with the entry points above: mdm_attn_fwd without text keys on what mdm_ctrl_gather_qkv wrote, then mdm_attn_cross_bias
 * twice in place with a zero bias -- (the source's q, kv_a, the source's mask) and (the row's own q, kv_b, its own mask).
 * own_rows, src_rows: DEVICE int32 [R], the absolute batch rows r and s of the R edited rows; an entry outside [0, N)
 * makes the kernel skip that row (nothing is read or written for it).  gate: a DEVICE float, 0 = off, anything else = on;
 * it selects, so one captured graph serves a trajectory.
 *
 * mdm_ctrl_mix_kv -- kvc [N, S, 2C] (k_c | v_c) -> kv_a, kv_b [R, S, 2C] of the same dtype:
 *   kv_a[r] = (k_c[s] | V'[r]),  kv_b[r] = (k_c[r] | V''[r]);  both key halves are copies, bit for bit.
 * M: fp32 [R, S, m_ld], m_ld >= S and % 4 == 0 (row = source token, column = edit token); its columns [S, m_ld) and the
 * columns of masked edit tokens are never read and may hold anything.  D: fp32 [R, S].  mask: [N, S] of 0/1 floats or NULL.
 * V' is accumulated in fp32 by FMAs over j ascending and rounded once; V'' is one product, rounded once.  Gate off: V' is
 * exact zeros and V'' is v_c[r] bit for bit.  One block per (8 source tokens, 64 16-byte channel chunks, row): a row's bits
 * do not depend on R.  C % 8 == 0 (bf16) / % 4 == 0 (fp32), 16-byte aligned tensors, R <= 65535.
 *
 * mdm_ctrl_gather_qkv -- qkv [N, L, 3C] -> qkv_self [R, L, 3C]: q and k columns of row (gate ? s : r), v columns of row r;
 * q_src [R, L, 3C]: the q columns of row s (its k and v columns are NOT written: mdm_attn_cross_bias with base == out
 * reads q only).  Copies of 16 bytes, bit for bit.
 *
 * Both: dtype MDM_F32 (the fp32-split mode has fp32 tensors) or MDM_BF16.  No allocation, no workspace, no host sync, no
 * atomics: capturable, and two runs are bit-identical.  Outputs alias neither each other nor the input.  Invalid host
 * arguments: a negative status, nothing launched.  Forward only. */
int mdm_ctrl_mix_kv(const void* kvc, const int* own_rows, const int* src_rows, const float* M, int m_ld, const float* D,
                    const float* mask, const float* gate, void* kv_a, void* kv_b, int N, int R, int S, int C, int dtype,
                    void* stream);
int mdm_ctrl_gather_qkv(const void* qkv, const int* own_rows, const int* src_rows, const float* gate, void* qkv_self,
                        void* q_src, int N, int R, int L, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_EXT_H_ */
