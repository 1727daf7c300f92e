"""The variant ledger of csrc/attention.hip + csrc/attn32.hpp: one row per kernel instantiation mdm_attn_fwd / mdm_attn_bwd
can launch, with the smallest shape that reaches it, the development knobs that force it (mdm_dev_set_attn_fwd /
mdm_dev_set_attn_bwd), the exact string mdm_last_attn_kernel() returns afterwards and the edges the shape exercises -- plus
the operands, the fp64 reference and the per-element gates every row is held to.

Host-only (torch on the CPU): tests/test_attn_variants_host.py checks the ledger and the gates themselves,
tests/test_attn_variants_gpu.py launches every row.

The operation (per batch element b and head h; scale = 1 / sqrt(d), the reference's d^-1/4 on q and on k):
    s_ij = scale q_i . k_j        p = softmax_j(s) over the live keys        o = p v        lse_i = log sum_j exp(s_ij)
    out = o_self + o_cross        (two separate softmaxes; a text key is dead where mask == 0, so -0.0 is dead and 0.5 / -1
                                   are live; a sample with no live text key has o_cross = 0 and lse_cross = -inf: what
                                   attn_fwd_kernel computes -- l = 0 gives inv = 0 and m ln 2 + __logf(0) = -inf)
    delta_i = do_i . o_i  (of that softmax)     dp_ij = do_i . v_j     ds = p (dp - delta)
    dq_i = scale sum_j ds_ij k_j  (both softmaxes)     dk_j = scale sum_i ds_ij q_i     dv_j = sum_i p_ij do_i

The gates
---------
Every output is compared element by element with the fp64 reference:  |got - ref| <= bound, the bound built from fp64
reference quantities only (never from the kernel's output).  U = 2^-8 is one bf16 rounding to nearest, relative: bf16
keeps 8 significant bits, so values in [2^e, 2^(e+1)) are 2^(e-7) apart and a rounding moves one by up to 2^(e-8), which is
2^-8 of a value at the bottom of the binade (1 + 2^-8 rounds to 1) and 2^-9 only of one at its top -- 2^-9 |v| is NOT a bound
a correctly rounding store can keep.  EPS32 = 2^-24 one fp32 rounding.  For fp32 tensors U is replaced by EPS32 throughout and dd = 2 d (the products of the fp32
MFMAs are rounded too); for bf16 dd = d (a product of two bf16 values is exact in fp32).  ACC(n) = 2 (n + 16) EPS32 is the
relative error of an fp32 sum of n terms (the factor 2: MFMA-internal accumulation may truncate, as in
tests/conv_variant_cases.py; + 16: the alpha rescales of the running sums, one per 64-key tile).  Lk = number of keys.

The rounding points, counted in the source (lines of csrc/attention.hip; the kernels of attn32.hpp and
attn_bwd_small_kernel state "same arithmetic ... and rounding points" and were read against the same list):

lse   m_run ln 2 + __logf(l) (attn_fwd_kernel, the `LSE[...] =` store).  The logit is an fp32 sum of d exact products:
      |ds_ij| <= dd EPS32 2 scale sum_c |q_ic k_jc|; the exponent fmaf(s, c2, -m_new) is one rounding of a value of size
      R_i log2 e (R_i = spread of the row's live logits), v_exp_f32 is good to 1 ulp; l is an fp32 sum of Lk positive terms;
      __logf = v_log_f32 (1 ulp) times ln 2; m ln 2 and the final sum round once each:
          B_lse_i = EPS32 (2 dd scale max_j sum_c |q_ic k_jc|  +  R_i + 4  +  2 (Lk + 16)  +  4 (|m_i| + |lse_i - m_i| + |lse_i|))
      A softmax weight e_ij / l_i therefore has relative error  d_i = 2 B_lse_i  in the forward (numerator and sum), and
      the recomputed weight of the backward, 2^(s c2 - lse log2 e) from the STORED lse, has  dp_i = 2 B_lse_i + 8 EPS32
      (|lse_i| + max_j |s_ij|)  (attn32.hpp forms s - lse / scale in the fp32 accumulator: both magnitudes round).
out   P is rounded to bf16 for the PV product (frag_from_acc_x) while l sums the unrounded values: U A_i per softmax with
      A_ic = sum_j p_ij |v_jc|; the softmax weights carry d_i and the PV sum ACC(Lk): (d_i + ACC) A_i; out_cross is staged as
      bf16 (`dst[i] = from_f32<T>(val[i])` under `if (OC && ...)`): U |oc|; the final store rounds self + float(oc): U |out|.
          B_oc  = U |oc| + (U + d_i + ACC) A_cross          B_out = U |out| + B_oc + (U + d_i + ACC) A_self
delta attn_bwd_dq_kernel forms delta_self = sum_c do (out - oc), delta_cross = sum_c do oc from the STORED bf16 tensors:
          dD_self_i = sum_c |do_ic| (U |out_ic| + (U + d_i + ACC) A_self_ic)  +  ACC(d) sum_c |do_ic| (|out_ic| + |oc_ic|)
          dD_cross_i = sum_c |do_ic| B_oc_ic  +  ACC(d) sum_c |do_ic oc_ic|
      (oc cancels in out - oc up to the final store's rounding, which is the U |out| term.)
ds    p (dp - delta) is rounded to bf16 for the second product (frag_from_acc<T>(dsf...)); dp is an fp32 sum of d products:
          W_ij = (U + dp_i + ACC(Lk)) |ds_ij| + p_ij (dD_i + ACC(dd) sum_c |do_ic v_jc|)
dq    = scale sum_j ds_ij k_j, stored as bf16:   B_dq_i = scale sum_j W_ij |k_j| (both softmaxes) + U |dq_i|
dk    the transpose:                             B_dk_j = scale sum_i W_ij |q_i| + U |dk_j|
dv    P rounded to bf16 (frag_from_acc<T>(pf...)):  B_dv_j = sum_i (U + dp_i + ACC(L)) p_ij |do_i| + U |dv_j|
One overall factor SLACK = 2 covers the second-order terms.  An element whose bound is 0 (a dead key's gradient, dK with
q = 0) must be exact.

Two operand kinds per row:
random   normals rounded to the row's dtype, q / k at scale 1.2 (peaked) or 0.3 (flat: the regime of a fresh model, where the
         old one-number gate is weakest); one query of head 0 spiked against one self key in a later tile and one query of
         the last head against the last text key, so the online-softmax rescale stays in.
uniform  q = 0, k random, v and dout small integers.  Every live key has weight exactly 1 / n: lse = ln n (within B_lse),
         dK = 0 EXACTLY, bf16 dV = bf16(bf16(1 / n) sum_i do_i) EXACTLY (uniform_dv_candidates), and the bf16 out is one rounding of the fp64 mean:  |out - mean| <= HU(mean) + 4 EPS32 (|o_self| +
         |o_cross|), HU(x) = 2^(floor(log2 |x|) - 8) = half the bf16 spacing at x: exactly what one rounding to nearest can
         move x by (between 2^-9 |x| and 2^-8 |x|; the tightest bound a correct store meets) -- plus HU(o_cross) where the
         number of live text keys is no power of two (then the staged bf16 out_cross is a rounding of its own; with a power
         of two sum v / n is exact in 8 bits, |sum v| <= 3 * 77 < 256).
"""
import math
import re

import torch

U = 2.0 ** -8
EPS32 = 2.0 ** -24
SLACK = 2.0
KINDS = ("random", "uniform")

# ---- edges -------------------------------------------------------------------------------------------------------------
QB2 = ">= 2 query blocks, the last one partial"
KODD = "odd number of 64-key tiles"
KRAG = "partial last 64-key tile"
TXT = "text keys"
TXT2 = "two text tiles, the last one partial"
BH8 = "B*H % 8 != 0 with more than one block per head"
OVER = "B*H > CUs"
L16 = "L < 16"
MASKS = ("none", "partial", "one", "values", "dead")


class Row:
    """``shape``: (B, L, S, H) or a function of the CU count returning it; ``fwd`` / ``bwd``: mdm_dev_set_attn_fwd /
    mdm_dev_set_attn_bwd.  ``entry`` 'fwd' launches mdm_attn_fwd only; 'bwd' launches the forward with the product's choice
    (its outputs are the backward's inputs, and are gated too) and then mdm_attn_bwd.  ``name``: what mdm_last_attn_kernel()
    returns after the row's entry."""

    def __init__(self, id, entry, dtype, d, shape, mask, flat, name, edges=(), fwd=0, bwd=0, note=""):
        assert entry in ("fwd", "bwd") and dtype in ("bf16", "float") and mask in MASKS
        self.id, self.entry, self.dtype, self.d, self.shape, self.mask, self.flat = id, entry, dtype, d, shape, mask, flat
        self.name, self.edges, self.fwd, self.bwd, self.note = name, tuple(edges), fwd, bwd, note

    def dims(self, cus=256):
        return self.shape(cus) if callable(self.shape) else self.shape

    @property
    def writes_delta(self):
        """the one-block-per-head kernels keep delta in LDS; the two-kernel paths hand it over through the workspace"""
        return "+" in self.name

    def __repr__(self):
        return self.id


def launch_rule(entry, dtype, d, fwd, bwd, B, L, S, H, cus):
    """attn_fwd_launch / attn_bwd_launch of csrc/attention.hip, transcribed: the name of what they launch"""
    if entry == "fwd":
        if dtype != "bf16":
            return "attn_fwd_kernel<float,%d,2>" % d
        by_shape = -(-L // 128) * B * H * 2 <= cus and L > 64
        qt = 1 if (fwd == 1 or (fwd == 0 and by_shape)) else 2
        return "attn_fwd_kernel<bf16,%d,%d>" % (d, qt)
    pair = "attn_bwd_dq_kernel<%s,%d,%d>+attn_bwd_dkv_kernel<%s,%d,%d>" % (dtype, d, 1 if d >= 96 else 2, dtype, d, 2 if (dtype == "bf16" and d <= 64) else 1)
    if dtype != "bf16":
        return pair
    split_only, force_small = bwd in (1, 4), bwd in (2, 3)
    if d in (64, 96) and L <= 256 and S <= 32 and not split_only and bwd != 3:
        return "attn_bwd_small32_kernel<%d>" % d
    if d == 64 and ((L > 256 and bwd == 0) or bwd == 4) and S <= 32:
        return "attn_bwd_dq32_kernel<64>+attn_bwd_dkv32_kernel<64>"
    if L <= 256 and S <= 64 and (B * H >= cus or force_small) and not split_only:
        return "attn_bwd_small_kernel<%d>" % d
    return pair


FW = "attn_fwd_kernel<%s,%d,%d>"
P16 = lambda t, d: launch_rule("bwd", t, d, 0, 1, 1, 1, 0, 1, 256)   # the 16x16x32 pair of (dtype, d)
SM = "attn_bwd_small_kernel<%d>"
S32 = "attn_bwd_small32_kernel<%d>"
P32 = "attn_bwd_dq32_kernel<64>+attn_bwd_dkv32_kernel<64>"

ROWS = [
    # ---- forward, bf16: QT (16 x QT queries per wave) forced, every d; L in (128, 192) or (256, 320): 3 / 5 key tiles, the
    # last one partial, and a partial last block of 64 / 128 queries ------------------------------------------------------
    Row("fwd_qt1_d32", "fwd", "bf16", 32, (1, 129, 20, 3), "partial", False, FW % ("bf16", 32, 1), (QB2, KODD, KRAG, TXT, BH8), fwd=1),
    Row("fwd_qt1_d64", "fwd", "bf16", 64, (1, 136, 77, 7), "none", True, FW % ("bf16", 64, 1), (QB2, KODD, KRAG, TXT, TXT2, BH8), fwd=1),
    Row("fwd_qt1_d96", "fwd", "bf16", 96, (3, 300, 33, 3), "dead", False, FW % ("bf16", 96, 1), (QB2, KODD, KRAG, TXT, BH8), fwd=1),
    Row("fwd_qt1_d128", "fwd", "bf16", 128, (2, 136, 3, 2), "values", True, FW % ("bf16", 128, 1), (QB2, KODD, KRAG, TXT), fwd=1),
    Row("fwd_qt2_d32", "fwd", "bf16", 32, (3, 136, 65, 3), "one", True, FW % ("bf16", 32, 2), (QB2, KODD, KRAG, TXT, TXT2, BH8), fwd=2),
    Row("fwd_qt2_d64", "fwd", "bf16", 64, (1, 300, 32, 7), "partial", False, FW % ("bf16", 64, 2), (QB2, KODD, KRAG, TXT, BH8), fwd=2),
    Row("fwd_qt2_d96", "fwd", "bf16", 96, (2, 136, 64, 2), "dead", True, FW % ("bf16", 96, 2), (QB2, KODD, KRAG, TXT), fwd=2,
        note="the instantiation of a batch-64 train step's 16x16 level"),
    Row("fwd_qt2_d128", "fwd", "bf16", 128, (1, 129, 1, 3), "none", False, FW % ("bf16", 128, 2), (QB2, KODD, KRAG, TXT, BH8), fwd=2),
    # the remaining L and S edges of the two forward families
    Row("fwd_qt1_L1", "fwd", "bf16", 64, (2, 1, 3, 2), "one", True, FW % ("bf16", 64, 1), (L16, KRAG, TXT), fwd=1),
    Row("fwd_qt1_L15", "fwd", "bf16", 96, (2, 15, 0, 3), "none", False, FW % ("bf16", 96, 1), (L16, KRAG), fwd=1),
    Row("fwd_qt1_L33", "fwd", "bf16", 32, (2, 33, 33, 2), "dead", True, FW % ("bf16", 32, 1), (KRAG, TXT), fwd=1),
    Row("fwd_qt1_L64", "fwd", "bf16", 128, (1, 64, 64, 2), "values", False, FW % ("bf16", 128, 1), (TXT,), fwd=1),
    Row("fwd_qt1_L65", "fwd", "bf16", 64, (1, 65, 65, 9), "partial", False, FW % ("bf16", 64, 1), (QB2, KRAG, TXT, TXT2, BH8), fwd=1),
    Row("fwd_qt1_L200", "fwd", "bf16", 96, (1, 200, 20, 7), "partial", True, FW % ("bf16", 96, 1), (QB2, KRAG, TXT, BH8), fwd=1),
    Row("fwd_qt1_L256", "fwd", "bf16", 32, (1, 256, 32, 3), "values", False, FW % ("bf16", 32, 1), (TXT, BH8), fwd=1),
    Row("fwd_qt1_L320", "fwd", "bf16", 128, (1, 320, 1, 3), "none", True, FW % ("bf16", 128, 1), (KODD, TXT, BH8), fwd=1),
    Row("fwd_qt1_L1000", "fwd", "bf16", 64, (1, 1000, 77, 2), "partial", True, FW % ("bf16", 64, 1), (QB2, KRAG, TXT, TXT2), fwd=1),
    Row("fwd_qt2_L1", "fwd", "bf16", 32, (2, 1, 1, 2), "none", False, FW % ("bf16", 32, 2), (L16, KRAG, TXT), fwd=2),
    Row("fwd_qt2_L15", "fwd", "bf16", 128, (2, 15, 20, 2), "dead", True, FW % ("bf16", 128, 2), (L16, KRAG, TXT), fwd=2),
    Row("fwd_qt2_L33", "fwd", "bf16", 96, (1, 33, 3, 3), "values", False, FW % ("bf16", 96, 2), (KRAG, TXT), fwd=2),
    Row("fwd_qt2_L64", "fwd", "bf16", 64, (2, 64, 0, 2), "none", True, FW % ("bf16", 64, 2), (), fwd=2),
    Row("fwd_qt2_L65", "fwd", "bf16", 96, (2, 65, 64, 2), "one", False, FW % ("bf16", 96, 2), (KRAG, TXT), fwd=2),
    Row("fwd_qt2_L200", "fwd", "bf16", 32, (1, 200, 33, 9), "partial", True, FW % ("bf16", 32, 2), (QB2, KRAG, TXT, BH8), fwd=2),
    Row("fwd_qt2_L256", "fwd", "bf16", 96, (1, 256, 32, 7), "partial", False, FW % ("bf16", 96, 2), (TXT, BH8), fwd=2),
    Row("fwd_qt2_L320", "fwd", "bf16", 64, (1, 320, 77, 3), "values", False, FW % ("bf16", 64, 2), (QB2, KODD, TXT, TXT2, BH8), fwd=2),
    Row("fwd_qt2_L1000", "fwd", "bf16", 64, (1, 1000, 20, 2), "one", True, FW % ("bf16", 64, 2), (QB2, KRAG, TXT), fwd=2),
    # ---- forward, fp32 (one instantiation per d; the knob does not apply) ------------------------------------------------
    Row("fwd_f32_d32", "fwd", "float", 32, (1, 136, 20, 3), "partial", True, FW % ("float", 32, 2), (QB2, KODD, KRAG, TXT, BH8)),
    Row("fwd_f32_d64", "fwd", "float", 64, (2, 129, 77, 2), "dead", False, FW % ("float", 64, 2), (QB2, KODD, KRAG, TXT, TXT2), fwd=1,
        note="fwd = 1 is set and must be ignored: the fp32 forward has no QT = 1 instantiation"),
    Row("fwd_f32_d96", "fwd", "float", 96, (1, 300, 0, 3), "none", True, FW % ("float", 96, 2), (QB2, KODD, KRAG, BH8)),
    Row("fwd_f32_d128", "fwd", "float", 128, (1, 15, 3, 2), "values", False, FW % ("float", 128, 2), (L16, KRAG, TXT)),
    Row("fwd_f32_L1", "fwd", "float", 64, (2, 1, 1, 2), "none", True, FW % ("float", 64, 2), (L16, KRAG, TXT)),
    Row("fwd_f32_L33", "fwd", "float", 32, (1, 33, 32, 3), "one", False, FW % ("float", 32, 2), (KRAG, TXT)),
    Row("fwd_f32_L64", "fwd", "float", 96, (1, 64, 33, 2), "partial", True, FW % ("float", 96, 2), (TXT,)),
    Row("fwd_f32_L65", "fwd", "float", 128, (2, 65, 64, 2), "dead", False, FW % ("float", 128, 2), (KRAG, TXT)),
    Row("fwd_f32_L200", "fwd", "float", 64, (1, 200, 65, 7), "partial", True, FW % ("float", 64, 2), (QB2, KRAG, TXT, TXT2, BH8)),
    Row("fwd_f32_L256", "fwd", "float", 32, (1, 256, 20, 2), "values", False, FW % ("float", 32, 2), (TXT,)),
    Row("fwd_f32_L320", "fwd", "float", 96, (1, 320, 3, 9), "none", True, FW % ("float", 96, 2), (QB2, KODD, TXT, BH8)),
    Row("fwd_f32_L1000", "fwd", "float", 64, (1, 1000, 0, 2), "none", True, FW % ("float", 64, 2), (QB2, KRAG)),
    # ---- forward, the product's rule (knob 0): QT = 1 iff ceil(L / 128) B H 2 <= CUs and L > 64 --------------------------
    Row("fwd_rule_fills", "fwd", "bf16", 96, lambda cus: (cus // 4, 129, 0, 1), "none", True, FW % ("bf16", 96, 1), (QB2, KODD, KRAG)),
    Row("fwd_rule_over", "fwd", "bf16", 96, lambda cus: (cus // 4 + 1, 129, 0, 1), "none", True, FW % ("bf16", 96, 2), (QB2, KODD, KRAG)),
    Row("fwd_rule_L64", "fwd", "bf16", 64, (1, 64, 20, 2), "partial", False, FW % ("bf16", 64, 2), (TXT,)),
    Row("fwd_rule_L65", "fwd", "bf16", 64, (1, 65, 20, 2), "partial", False, FW % ("bf16", 64, 1), (QB2, KRAG, TXT)),
    # ---- backward, the two streaming kernels on 16x16x32 MFMAs: bf16 (bwd = 1) and fp32, every d (DQ_QT = 2 below d = 96,
    # KV_KT = 2 for bf16 at d <= 64) -----------------------------------------------------------------------------------
    Row("bwd16_bf16_d32", "bwd", "bf16", 32, (1, 129, 20, 3), "partial", False, P16("bf16", 32), (QB2, KODD, KRAG, TXT, BH8), bwd=1),
    Row("bwd16_bf16_d64", "bwd", "bf16", 64, (1, 200, 77, 7), "none", True, P16("bf16", 64), (QB2, KRAG, TXT, TXT2, BH8), bwd=1),
    Row("bwd16_bf16_d96", "bwd", "bf16", 96, (3, 136, 33, 3), "dead", False, P16("bf16", 96), (QB2, KODD, KRAG, TXT, BH8), bwd=1),
    Row("bwd16_bf16_d128", "bwd", "bf16", 128, (2, 65, 65, 2), "values", True, P16("bf16", 128), (QB2, KRAG, TXT, TXT2), bwd=1),
    Row("bwd16_bf16_L1", "bwd", "bf16", 96, (2, 1, 1, 2), "none", True, P16("bf16", 96), (L16, KRAG, TXT), bwd=1),
    Row("bwd16_bf16_L15", "bwd", "bf16", 32, (2, 15, 0, 3), "none", False, P16("bf16", 32), (L16, KRAG), bwd=1),
    Row("bwd16_bf16_L33", "bwd", "bf16", 128, (2, 33, 3, 2), "dead", False, P16("bf16", 128), (KRAG, TXT), bwd=1),
    Row("bwd16_bf16_L64", "bwd", "bf16", 64, (2, 64, 64, 2), "one", True, P16("bf16", 64), (TXT,), bwd=1),
    Row("bwd16_bf16_L256", "bwd", "bf16", 96, (1, 256, 32, 9), "values", False, P16("bf16", 96), (TXT, BH8), bwd=1),
    Row("bwd16_bf16_L320", "bwd", "bf16", 128, (1, 320, 64, 3), "partial", True, P16("bf16", 128), (KODD, TXT, BH8), bwd=1),
    Row("bwd16_bf16_L1000", "bwd", "bf16", 32, (1, 1000, 3, 2), "one", True, P16("bf16", 32), (QB2, KRAG, TXT), bwd=1),
    Row("bwd16_f32_d32", "bwd", "float", 32, (1, 200, 20, 3), "values", True, P16("float", 32), (QB2, KRAG, TXT, BH8)),
    Row("bwd16_f32_d64", "bwd", "float", 64, (2, 129, 33, 2), "dead", False, P16("float", 64), (QB2, KODD, KRAG, TXT)),
    Row("bwd16_f32_d96", "bwd", "float", 96, (1, 136, 0, 3), "none", False, P16("float", 96), (QB2, KODD, KRAG, BH8)),
    Row("bwd16_f32_d128", "bwd", "float", 128, (1, 65, 65, 7), "partial", True, P16("float", 128), (QB2, KRAG, TXT, TXT2, BH8)),
    Row("bwd16_f32_L15", "bwd", "float", 64, (2, 15, 1, 2), "none", True, P16("float", 64), (L16, KRAG, TXT)),
    Row("bwd16_f32_L1", "bwd", "float", 128, (2, 1, 3, 2), "one", False, P16("float", 128), (L16, KRAG, TXT)),
    Row("bwd16_f32_L33", "bwd", "float", 96, (2, 33, 32, 2), "dead", True, P16("float", 96), (KRAG, TXT)),
    Row("bwd16_f32_L64", "bwd", "float", 32, (1, 64, 64, 3), "partial", False, P16("float", 32), (TXT,)),
    Row("bwd16_f32_L256", "bwd", "float", 64, (1, 256, 77, 9), "none", True, P16("float", 64), (TXT, TXT2, BH8)),
    Row("bwd16_f32_L320", "bwd", "float", 32, (1, 320, 0, 2), "none", False, P16("float", 32), (QB2, KODD)),
    Row("bwd16_f32_L1000", "bwd", "float", 64, (1, 1000, 20, 2), "values", True, P16("float", 64), (QB2, KRAG, TXT)),
    # ---- backward, one block per head on 16x16x32 MFMAs (bwd = 2; at d = 64 / 96 bwd = 3, or more than 32 text keys) ------
    Row("small_d32", "bwd", "bf16", 32, (3, 200, 64, 3), "dead", False, SM % 32, (KRAG, TXT), bwd=2),
    Row("small_d64", "bwd", "bf16", 64, (2, 256, 32, 2), "partial", True, SM % 64, (TXT,), bwd=3),
    Row("small_d96", "bwd", "bf16", 96, (1, 129, 33, 7), "values", False, SM % 96, (KODD, KRAG, TXT), bwd=2,
        note="33 text keys: one more than attn_bwd_small32_kernel takes, so bwd = 2 reaches the 16x16 kernel at d = 96"),
    Row("small_d128", "bwd", "bf16", 128, (2, 65, 20, 2), "one", True, SM % 128, (KRAG, TXT), bwd=2),
    Row("small_L1", "bwd", "bf16", 128, (2, 1, 3, 2), "dead", True, SM % 128, (L16, KRAG, TXT), bwd=2),
    Row("small_L15", "bwd", "bf16", 64, (2, 15, 1, 3), "none", False, SM % 64, (L16, KRAG, TXT), bwd=3),
    Row("small_L33", "bwd", "bf16", 32, (1, 33, 0, 3), "none", True, SM % 32, (KRAG,), bwd=2),
    Row("small_L64", "bwd", "bf16", 96, (1, 64, 64, 2), "partial", False, SM % 96, (TXT,), bwd=3),
    Row("small_over", "bwd", "bf16", 32, lambda cus: (cus + 8, 33, 3, 1), "values", True, SM % 32, (OVER, KRAG, TXT)),
    # ---- backward, one block per head on 32x32x16 MFMAs (attn32.hpp; the product's choice at d = 64 / 96, L <= 256, S <= 32)
    Row("small32_d64", "bwd", "bf16", 64, (2, 200, 20, 2), "dead", False, S32 % 64, (KRAG, TXT)),
    Row("small32_d96", "bwd", "bf16", 96, (1, 256, 32, 3), "partial", True, S32 % 96, (TXT,)),
    Row("small32_L1", "bwd", "bf16", 96, (2, 1, 1, 2), "none", False, S32 % 96, (L16, KRAG, TXT)),
    Row("small32_L15", "bwd", "bf16", 64, (2, 15, 3, 2), "dead", True, S32 % 64, (L16, KRAG, TXT)),
    Row("small32_L33", "bwd", "bf16", 96, (1, 33, 0, 3), "none", True, S32 % 96, (KRAG,)),
    Row("small32_L64", "bwd", "bf16", 64, (1, 64, 32, 7), "values", False, S32 % 64, (TXT,)),
    Row("small32_L65", "bwd", "bf16", 64, (1, 65, 20, 3), "one", True, S32 % 64, (KRAG, TXT)),
    Row("small32_L129", "bwd", "bf16", 96, (2, 129, 3, 2), "values", False, S32 % 96, (KODD, KRAG, TXT)),
    Row("small32_over", "bwd", "bf16", 64, lambda cus: (cus + 8, 33, 1, 1), "none", True, S32 % 64, (OVER, KRAG, TXT)),
    # ---- backward, the streaming kernels on 32x32x16 MFMAs (d = 64, S <= 32: L > 256 in the product, any L with bwd = 4) ---
    Row("bwd32_L320", "bwd", "bf16", 64, (1, 320, 32, 3), "partial", False, P32, (QB2, KODD, TXT, BH8)),
    Row("bwd32_L1000", "bwd", "bf16", 64, (1, 1000, 20, 2), "values", True, P32, (QB2, KRAG, TXT)),
    Row("bwd32_L300_dead", "bwd", "bf16", 64, (2, 300, 3, 2), "dead", True, P32, (QB2, KODD, KRAG, TXT)),
    Row("bwd32_L300_bh7", "bwd", "bf16", 64, (1, 300, 20, 7), "partial", False, P32, (QB2, KODD, KRAG, TXT, BH8)),
    Row("bwd32_L64", "bwd", "bf16", 64, (1, 64, 1, 3), "none", False, P32, (TXT,), bwd=4),
    Row("bwd32_L65", "bwd", "bf16", 64, (2, 65, 32, 2), "dead", True, P32, (KRAG, TXT), bwd=4),
    Row("bwd32_L129", "bwd", "bf16", 64, (1, 129, 0, 2), "none", True, P32, (KODD, KRAG), bwd=4),
    Row("bwd32_L1", "bwd", "bf16", 64, (2, 1, 1, 2), "none", True, P32, (L16, KRAG, TXT), bwd=4),
    Row("bwd32_L15", "bwd", "bf16", 64, (1, 15, 0, 3), "none", False, P32, (L16, KRAG), bwd=4),
    Row("bwd32_L33", "bwd", "bf16", 64, (2, 33, 20, 2), "one", False, P32, (KRAG, TXT), bwd=4),
    Row("bwd32_L200", "bwd", "bf16", 64, (1, 200, 32, 9), "partial", True, P32, (KRAG, TXT), bwd=4),
    Row("bwd32_L256", "bwd", "bf16", 64, (2, 256, 3, 2), "dead", False, P32, (TXT,), bwd=4),
    # ---- backward, the product's rule (knob 0), one row on each side of every branch -------------------------------------
    Row("rule_L256_d64", "bwd", "bf16", 64, (1, 256, 20, 2), "partial", False, S32 % 64, (TXT,)),
    Row("rule_L257_d64", "bwd", "bf16", 64, (1, 257, 20, 9), "partial", False, P32, (QB2, KODD, KRAG, TXT, BH8)),
    Row("rule_L256_d96", "bwd", "bf16", 96, (1, 256, 0, 2), "none", True, S32 % 96, ()),
    Row("rule_L257_d96", "bwd", "bf16", 96, (1, 257, 0, 2), "none", True, P16("bf16", 96), (QB2, KODD, KRAG),
        note="d = 96 has no streaming kernel on 32x32x16 MFMAs: L > 256 goes to the 16x16x32 pair"),
    Row("rule_S32", "bwd", "bf16", 64, (2, 129, 32, 2), "values", True, S32 % 64, (KODD, KRAG, TXT)),
    Row("rule_S33", "bwd", "bf16", 64, (2, 129, 33, 2), "values", True, P16("bf16", 64), (QB2, KODD, KRAG, TXT),
        note="33 text keys and fewer heads than CUs: neither one-block kernel, the 16x16x32 pair"),
    Row("rule_S33_fills", "bwd", "bf16", 96, lambda cus: (cus, 33, 33, 1), "partial", False, SM % 96, (KRAG, TXT)),
    Row("rule_S64_fills", "bwd", "bf16", 64, lambda cus: (cus, 33, 64, 1), "dead", True, SM % 64, (KRAG, TXT)),
    Row("rule_S65_fills", "bwd", "bf16", 64, lambda cus: (cus, 33, 65, 1), "dead", True, P16("bf16", 64), (KRAG, TXT, TXT2)),
    Row("rule_S77_d96", "bwd", "bf16", 96, (1, 136, 77, 3), "partial", False, P16("bf16", 96), (QB2, KODD, KRAG, TXT, TXT2, BH8), bwd=2,
        note="bwd = 2 is set: 77 text keys fit no one-block kernel, every mode runs the 16x16x32 pair"),
    Row("rule_mode4_d96", "bwd", "bf16", 96, (1, 300, 20, 3), "one", True, P16("bf16", 96), (QB2, KODD, KRAG, TXT, BH8), bwd=4,
        note="bwd = 4 at d = 96 falls through to the 16x16x32 pair"),
    Row("rule_below_d32", "bwd", "bf16", 32, lambda cus: (cus - 1, 33, 20, 1), "partial", False, P16("bf16", 32), (KRAG, TXT)),
    Row("rule_fills_d32", "bwd", "bf16", 32, lambda cus: (cus, 33, 20, 1), "partial", False, SM % 32, (KRAG, TXT)),
    Row("rule_below_d128", "bwd", "bf16", 128, lambda cus: (cus - 1, 15, 0, 1), "none", True, P16("bf16", 128), (L16, KRAG)),
    Row("rule_fills_d128", "bwd", "bf16", 128, lambda cus: (cus, 15, 0, 1), "none", True, SM % 128, (L16, KRAG)),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


# ---- operands ----------------------------------------------------------------------------------------------------------
def bf16r(t):
    """round to bf16 (to nearest even), keep the dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _seed(row, kind):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(row.id)) * 7 + KINDS.index(kind) * 3) % (2 ** 31)


def n_live_target(S):
    """live text keys of a 'partial' / 'values' / 'dead' sample: the largest power of two below S (S itself at S <= 2)"""
    return S if S <= 2 else 2 ** int(math.log2(S - 1))


def make_mask(row, B, S, gen):
    """[B, S] fp32 or None.  'partial': a power-of-two number of keys live (1.0), the rest 0.0; 'one': one live key per
    sample, the last key for sample 0; 'values': as 'partial' with live values 0.5, -1, 2, 1e-30 and dead keys -0.0 / +0.0 in turn;
    'dead': sample 0 has no live key (+0.0 / -0.0 in turn), the other samples as 'partial'."""
    if row.mask == "none" or S == 0:
        return None
    m = torch.zeros(B, S, dtype=torch.float32)
    for b in range(B):
        if row.mask == "one":
            m[b, (S - 1 + 5 * b) % S] = 1.0
            continue
        perm = torch.randperm(S, generator=gen)
        m[b, perm[:n_live_target(S)]] = 1.0
    if row.mask == "values":
        vals = torch.tensor([0.5, -1.0, 2.0, 1e-30])
        k = torch.arange(S)
        rank = (m == 0).cumsum(1)                                         # a sample's first, third, ... dead key is -0.0
        m = torch.where(m != 0, vals[(k % 4)].expand(B, S), torch.where(rank % 2 == 1, -torch.zeros(()), torch.zeros(())))
    if row.mask == "dead":
        k = torch.arange(S)
        m[0] = torch.where(k % 2 == 1, -torch.zeros(()), torch.zeros(()))
    return m


def operands(row, kind, cus=256):
    """{'qkv' [B, L, 3C], 'kvc' [B, S, 2C] or None, 'mask' [B, S] fp32 or None, 'dout' [B, L, C]} as fp64 CPU tensors whose
    values are representable in the row's dtype"""
    B, L, S, H = row.dims(cus)
    d, C = row.d, H * row.d
    gen = torch.Generator().manual_seed(_seed(row, kind))
    rnd = bf16r if row.dtype == "bf16" else (lambda t: t.float().double())
    f64 = torch.float64
    qkv = torch.randn(B, L, 3 * C, generator=gen, dtype=f64)
    kvc = torch.randn(B, S, 2 * C, generator=gen, dtype=f64) if S else None
    dout = torch.randn(B, L, C, generator=gen, dtype=f64)
    if kind == "random":
        sc = 0.3 if row.flat else 1.2
        qkv[..., :2 * C] *= sc
        qkv = rnd(qkv)
        iq = L // 2
        jk = (3 * L) // 4 if L <= 64 else max((3 * L) // 4, 64)          # a key of a tile after the first where there is one
        qkv[0, iq, :d] *= 6.0
        qkv[0, jk, C:C + d] = qkv[0, iq, :d] * 0.5
        if S:
            kvc[..., :C] *= sc
            kvc = rnd(kvc)
            i2 = L // 3
            qkv[B - 1, i2, C - d:C] *= 6.0
            kvc[B - 1, S - 1, C - d:C] = qkv[B - 1, i2, C - d:C] * 0.5
            kvc = rnd(kvc)
        qkv, dout = rnd(qkv), rnd(dout)
    else:
        ints = lambda shape: torch.randint(-3, 4, shape, generator=gen).double()
        qkv[..., :C] = 0.0
        qkv[..., 2 * C:] = ints((B, L, C))
        qkv = rnd(qkv)
        if S:
            kvc[..., C:] = ints((B, S, C))
            kvc = rnd(kvc)
        dout = ints((B, L, C))
    return {"qkv": qkv, "kvc": kvc, "mask": make_mask(row, B, S, gen), "dout": dout, "H": H, "d": d, "dtype": row.dtype}


# ---- the operation -----------------------------------------------------------------------------------------------------
def _heads(x, H, d, part):
    """[B, N, parts * C] -> part ``part`` as [B, H, N, d]"""
    B, N = x.shape[:2]
    C = H * d
    return x[..., part * C:(part + 1) * C].reshape(B, N, H, d).permute(0, 2, 1, 3)


def _merge(x):
    """[B, H, N, d] -> [B, N, H * d]"""
    B, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * d)


class Defect:
    """planted defects of tests/test_attn_variants_host.py (all off: the operation itself)"""
    lose_key = None        # self key index the forward and the backward leave out
    dup_query = None       # query row counted twice in dK / dV (self)
    live_dead = False      # the first dead text key of every sample is treated as live
    no_scale = False       # dQ / dK without the 1 / sqrt(d)
    delta_total = False    # delta_self from out instead of out - out_cross
    drop_rows = None       # (i0, i1): query rows left out of the dK / dV sums (self)
    nan_out_row = None     # out row left unwritten


def _softmax(q, k, scale, live):
    """logits s, e = exp(s - max), l = sum e and lse of one softmax: q [B, H, L, d], k [B, H, N, d], live [B, N] bool or None"""
    s = (q @ k.transpose(-1, -2)) * scale
    if live is not None:
        s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m0)
    l = e.sum(-1, keepdim=True)
    lse = (m0 + torch.log(l)).squeeze(-1)          # -inf where no key is live
    return s, e, l, lse


def attention(o, dtype=torch.float64, emulate=False, defect=None, backward=True):
    """The operation on operands ``o`` in ``dtype``.  ``emulate``: with the kernels' roundings (to the operands' dtype) at
    the counted rounding points -- P before PV, the staged out_cross, the final store, delta from the stored tensors, the
    backward's P and dS, the gradient stores.  Returns {'out', 'out_cross', 'lse_self', 'lse_cross', 'dq', 'dk', 'dv',
    'dkc', 'dvc'} ([B, L, C] / [B, H, L] / [B, S, C]; absent tensors are missing) and, without ``emulate``, 'aux'."""
    D = defect or Defect()
    H, d = o["H"], o["d"]
    scale = 1.0 / math.sqrt(d)
    if emulate:
        rnd = bf16r if o["dtype"] == "bf16" else (lambda t: t)
    else:
        rnd = lambda t: t
    c = lambda t: t.to(dtype)
    q, k, v = (c(_heads(o["qkv"], H, d, i)) for i in range(3))
    B, _, L, _ = q.shape
    has_c = o["kvc"] is not None
    live_s = None
    if D.lose_key is not None:
        live_s = torch.ones(B, L, dtype=torch.bool)
        live_s[:, D.lose_key] = False
    parts = [("self", k, v, live_s)]
    if has_c:
        S = o["kvc"].shape[1]
        live_c = (o["mask"] != 0) if o["mask"] is not None else torch.ones(B, S, dtype=torch.bool)
        if D.live_dead:
            live_c = live_c.clone()
            for b in range(B):
                dead = (~live_c[b]).nonzero()
                if len(dead):
                    live_c[b, dead[0]] = True
        parts.append(("cross", c(_heads(o["kvc"], H, d, 0)), c(_heads(o["kvc"], H, d, 1)), live_c))
    r, sm = {}, {}
    for name, kk, vv, live in parts:
        s, e, l, lse = _softmax(q, kk, scale, live)
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        oo = (rnd(e) @ vv) * inv
        sm[name] = dict(k=kk, v=vv, s=s, p=e * inv, lse=lse, o=oo, live=live)
        r["lse_" + name] = lse
    oc = rnd(sm["cross"]["o"]) if has_c else None
    out = rnd(sm["self"]["o"] + oc) if has_c else rnd(sm["self"]["o"])
    r["out"] = _merge(out).clone()
    if has_c:
        r["out_cross"] = _merge(oc)
    if D.nan_out_row is not None:
        r["out"][:, D.nan_out_row] = float("nan")
    if backward:
        do = c(_heads(o["dout"], H, d, 0))
        gs = 1.0 if D.no_scale else scale
        dq = torch.zeros_like(q)
        for name in sm:
            t = sm[name]
            if emulate or D.delta_total:   # from the stored tensors
                base = out if (name == "self" and D.delta_total) else (out - oc if (name == "self" and has_c) else (out if name == "self" else oc))
                delta = (do * base).sum(-1, keepdim=True)
            else:
                delta = (do * t["o"]).sum(-1, keepdim=True)
            if emulate:
                lse = t["lse"].unsqueeze(-1)
                p = torch.exp(t["s"] - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse))
                p = torch.where(torch.isinf(lse), torch.zeros_like(p), p)
            else:
                p = t["p"]
            dp = do @ t["v"].transpose(-1, -2)
            ds = p * (dp - delta)
            t["delta"], t["dp"], t["ds"] = delta, dp, ds
            dq = dq + rnd(ds) @ t["k"]
            pk, dsk, qk, dok = rnd(p), rnd(ds), q, do
            if name == "self" and D.drop_rows is not None:
                keep = torch.ones(L, dtype=torch.bool)
                keep[D.drop_rows[0]:D.drop_rows[1]] = False
                pk, dsk, qk, dok = pk[:, :, keep], dsk[:, :, keep], q[:, :, keep], do[:, :, keep]
            dk = dsk.transpose(-1, -2) @ qk
            dv = pk.transpose(-1, -2) @ dok
            if name == "self" and D.dup_query is not None:
                i = D.dup_query
                dk = dk + ds[:, :, i:i + 1].transpose(-1, -2) @ q[:, :, i:i + 1]
                dv = dv + p[:, :, i:i + 1].transpose(-1, -2) @ do[:, :, i:i + 1]
            r["dk" if name == "self" else "dkc"] = _merge(rnd(dk * gs))
            r["dv" if name == "self" else "dvc"] = _merge(rnd(dv))
        r["dq"] = _merge(rnd(dq * gs))
    if not emulate:
        r["aux"] = dict(sm=sm, q=q, do=c(_heads(o["dout"], H, d, 0)) if backward else None, scale=scale, out=out, oc=oc)
    return {k_: (v_.double() if torch.is_tensor(v_) else v_) for k_, v_ in r.items()}


# ---- reference and bounds ----------------------------------------------------------------------------------------------
def _acc(n):
    return 2.0 * (n + 16) * EPS32


class Expect:
    def __init__(self, ref, bound):
        self.ref, self.bnd = ref, bound

    def bound(self):
        return self.bnd


def reference(row, o, backward=None):
    """{tensor name: Expect} from the fp64 operation; the bounds of the module docstring"""
    backward = (row.entry == "bwd") if backward is None else backward
    r = attention(o, backward=backward)
    aux = r.pop("aux")
    bf = row.dtype == "bf16"
    u = U if bf else EPS32
    d = row.d
    dd = d if bf else 2 * d
    scale, q, sm = aux["scale"], aux["q"], aux["sm"]
    exp = {}
    for name, t in sm.items():
        N = t["k"].shape[2]
        s, live = t["s"], t["live"]
        sabs = (q.abs() @ t["k"].abs().transpose(-1, -2)) * scale
        if live is not None:
            sabs = sabs.masked_fill(~live[:, None, None, :], 0.0)
        fin = torch.isfinite(s)
        smax = torch.where(fin, s, torch.full_like(s, -1e300)).max(-1).values
        smin = torch.where(fin, s, torch.full_like(s, 1e300)).min(-1).values
        dead = ~fin.any(-1)
        z = torch.zeros_like(smax)
        smax, smin = torch.where(dead, z, smax), torch.where(dead, z, smin)
        lse = torch.where(dead, z, t["lse"])
        b_lse = EPS32 * (2 * dd * sabs.max(-1).values + (smax - smin) + 4 + 2 * (N + 16) + 4 * (smax.abs() + (lse - smax).abs() + lse.abs()))
        t["b_lse"] = b_lse
        t["d_fwd"] = 2 * b_lse
        t["d_bwd"] = 2 * b_lse + 8 * EPS32 * (lse.abs() + torch.maximum(smax.abs(), smin.abs()))
        t["A"] = t["p"] @ t["v"].abs()
        t["E"] = (u + t["d_fwd"].unsqueeze(-1) + _acc(N)) * t["A"]          # error of this softmax's o before any store
        exp["lse_" + name] = Expect(t["lse"], SLACK * torch.where(dead, z, b_lse))
    out, oc = aux["out"], aux["oc"]
    has_c = oc is not None
    b_oc = (u * oc.abs() + sm["cross"]["E"]) if has_c else None
    b_out = u * out.abs() + sm["self"]["E"] + (b_oc if has_c else 0.0)
    exp["out"] = Expect(r["out"], SLACK * _merge(b_out))
    if has_c:
        exp["out_cross"] = Expect(r["out_cross"], SLACK * _merge(b_oc))
    if backward:
        do = aux["do"]
        L = q.shape[2]
        osum = out.abs() + (oc.abs() if has_c else 0.0)
        dD = {"self": (do.abs() * (u * out.abs() + sm["self"]["E"])).sum(-1) + _acc(d) * (do.abs() * osum).sum(-1)}
        if has_c:
            dD["cross"] = (do.abs() * b_oc).sum(-1) + _acc(d) * (do.abs() * oc.abs()).sum(-1)
        b_dq = torch.zeros_like(q)
        for name, t in sm.items():
            N = t["k"].shape[2]
            dpabs = do.abs() @ t["v"].abs().transpose(-1, -2)
            dpr = t["d_bwd"].unsqueeze(-1)
            W = (u + dpr + _acc(max(N, L))) * t["ds"].abs() + t["p"] * (dD[name].unsqueeze(-1) + _acc(dd) * (dpabs + t["delta"].abs()))
            b_dq = b_dq + scale * (W @ t["k"].abs())
            b_dk = scale * (W.transpose(-1, -2) @ q.abs())
            b_dv = ((u + dpr + _acc(L)) * t["p"]).transpose(-1, -2) @ do.abs()
            kn, vn = ("dk", "dv") if name == "self" else ("dkc", "dvc")
            exp[kn] = Expect(r[kn], SLACK * (_merge(b_dk) + u * r[kn].abs()))
            exp[vn] = Expect(r[vn], SLACK * (_merge(b_dv) + u * r[vn].abs()))
        exp["dq"] = Expect(r["dq"], SLACK * (_merge(b_dq) + u * r["dq"].abs()))
    exp["_aux"] = aux
    return exp


def half_ulp(x, dtype="bf16"):
    """half the spacing of the row's dtype at |x| (0 at 0): what one rounding to nearest moves x by, at most"""
    bits = 8 if dtype == "bf16" else 24
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-300)))
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(e - bits))


def n_live(o):
    """(self keys, [B] live text keys or None)"""
    L = o["qkv"].shape[1]
    if o["kvc"] is None:
        return L, None
    S = o["kvc"].shape[1]
    return L, ((o["mask"] != 0).sum(1) if o["mask"] is not None else torch.full((o["qkv"].shape[0],), S))


def uniform_expect(row, o, exp):
    """the exact conditions of the uniform kind: {'lse_self', 'lse_cross': (value [B], None) , 'out': Expect with the
    one-rounding bound}.  lse = ln(n_live) (-inf for a dead sample); out = mean of v over the live keys."""
    aux = exp["_aux"]
    L, nc = n_live(o)
    res = {"lse_self": torch.full_like(exp["lse_self"].ref, math.log(L))}
    o_self, oc = aux["sm"]["self"]["o"], aux["oc"]
    bound = half_ulp(aux["out"], row.dtype) + 4 * EPS32 * (o_self.abs() + (oc.abs() if oc is not None else 0.0))
    if nc is not None:
        res["lse_cross"] = torch.log(nc.double())[:, None, None].expand_as(exp["lse_cross"].ref)
        pow2 = (nc & (nc - 1)) == 0                     # (0 counts: a dead sample's cross term is exactly 0)
        bound = bound + torch.where(pow2, 0.0, 1.0)[:, None, None, None] * half_ulp(oc, row.dtype)
    res["out"] = Expect(exp["out"].ref, _merge(bound))
    return res


def uniform_dv_candidates(row, o):
    """bf16 rows of the uniform kind: what dV / dVc must hold EXACTLY.  Every live key has the same weight for every query:
    the backward recomputes 2^(0 - lse log2 e) from lse = __logf(n) -- within 2e-6 of 1 / n (1 ulp of v_log_f32 on |ln n| < 7,
    the product with log2 e, 1 ulp of v_exp_f32) -- and rounds it to bf16: pt, ONE value for the whole softmax.  dout holds
    integers |.| <= 3, so every product pt * do is exact and every partial sum is pt times an integer below 2^11: 8 + 11 bits,
    exact in fp32 in any order.  So dV_jc = bf16(pt * sum_i do_ic) for a live key, 0 for a dead one -- and a query row counted
    twice or left out changes the integer.  pt = bf16(1 / n); where 1 / n lies within 2^-16 of the middle between two bf16
    values both are admitted.  Returns {'dv': [candidates [B, N, C]], 'dvc': [...]}; a (batch, head) must match ONE of them."""
    assert row.dtype == "bf16"
    H, d = o["H"], o["d"]
    B, L = o["qkv"].shape[:2]
    T = o["dout"].sum(1, keepdim=True)                                     # [B, 1, C]
    L_, nc = n_live(o)
    sets = {"dv": (torch.full((B,), float(L)), torch.ones(B, L, dtype=torch.bool))}
    if nc is not None:
        live = (o["mask"] != 0) if o["mask"] is not None else torch.ones(B, o["kvc"].shape[1], dtype=torch.bool)
        sets["dvc"] = (nc.double(), live)
    out = {}
    for name, (n, live) in sets.items():
        cands = []
        for f in (1.0 - 2.0 ** -16, 1.0, 1.0 + 2.0 ** -16):
            pt = bf16r(torch.where(n > 0, f / n.clamp_min(1), torch.zeros_like(n)).double())
            e = bf16r(pt[:, None, None] * T) * live[:, :, None]
            if not any(bool((e == c).all()) for c in cands):
                cands.append(e)
        out[name] = cands
    return out


def heads_without_exact_match(got, cands, H):
    """number of (batch, head) pairs whose [N, d] block equals none of the candidates' blocks"""
    B, N, C = got.shape
    ok = torch.zeros(B, H, dtype=torch.bool)
    for c in cands:
        ok |= (got.double() == c).reshape(B, N, H, C // H).all(3).all(1)
    return int((~ok).sum())


# ---- gates -------------------------------------------------------------------------------------------------------------
def bound_ratio(got, e):
    """(worst |got - ref| / bound, number of elements over the bound); an element with bound 0 must be exact; where the
    reference is -inf (lse of a dead sample) the value must be -inf"""
    got, ref = got.double(), e.ref
    same_inf = torch.isinf(ref) & (got == ref)
    diff = torch.where(same_inf, torch.zeros_like(ref), (got - ref).abs())
    bound = e.bound()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, bound)
    inf = torch.full_like(diff, float("inf"))
    ratio = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), inf))
    ratio = torch.where(torch.isnan(diff), inf, ratio)
    if ratio.numel() == 0:
        return 0.0, 0
    return float(ratio.max()), int((ratio > 1).sum())


def old_relerr(got, ref):
    """the gate of tests/test_ops_gpu.py: max |a - b| / max |b|"""
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


def old_gate_passes(got, ref, tol=3e-2):
    """test_attention's three numbers: out, dqkv as a whole (dQ, dK, dV together) and dkvc as a whole"""
    ok = old_relerr(got["out"], ref["out"]) < tol
    if "dq" in ref:
        cat = lambda r: torch.cat([r["dq"], r["dk"], r["dv"]], -1)
        ok = ok and old_relerr(cat(got), cat(ref)) < tol
        if "dkc" in ref:
            catc = lambda r: torch.cat([r["dkc"], r["dvc"]], -1)
            ok = ok and old_relerr(catc(got), catc(ref)) < tol
    return ok


# ---- the name formats of the source ------------------------------------------------------------------------------------
def note_kernel_formats(source_text):
    """the distinct format strings of the MDM_NOTE_ATTN(...) lines"""
    return sorted(set(re.findall(r'MDM_NOTE_ATTN\("([^"]+)"', source_text)))


def format_regex(fmt):
    return re.compile("^" + re.escape(fmt).replace("%d", r"\d+").replace("%s", r"[a-z0-9_]+") + "$")
