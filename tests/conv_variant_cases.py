"""The variant ledger of csrc/gemm_conv.hip: one row per kernel variant the file can launch for bf16 tensors, with the
smallest shape that reaches it, the development knobs that force it, the exact string mdm_last_gemm_kernel() returns
afterwards and the edges the shape exercises -- plus the operands, fp64 references and gates the rows are held to.

Host-only (torch on the CPU; nothing here touches a GPU): tests/test_conv_variants_host.py checks the ledger and the
gates themselves, tests/test_conv_variants_gpu.py launches every row.

The gates
---------
Operands are bf16-representable (bias: fp32, as the kernels read it); the reference is F.conv2d in fp64 on them, its
fp64 autograd for the gradients.

* integer data: every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact in ANY order
  and the kernel must reproduce ``bf16(bf16(sum + bias) + res)`` (what conv_epilogue / splitk_epilogue_kernel compute)
  -- respectively the fp64 value itself for the fp32 weight / bias gradients -- with ZERO differing elements.
* random data, elementwise: with u = 2^-8 (one bf16 rounding is within u |v| -- half of it under round-to-nearest)
    bf16 output, residual :  |got - ref| <= u (1 + u) |pre| + u |ref| + A
    bf16 output, none     :  |got - ref| <= u |ref| + A
    fp32 output (dw, db)  :  |got - ref| <= A
  ``pre`` = fp64 value before the residual, ``A = f * L * 2^-24 * (|a| (*) |b| + |bias|)`` = worst-case error of L fp32
  additions (each within 2^-24 of the running sum of magnitudes), computed by the same fp64 operation on absolute
  values; f = 2 covers MFMA-internal accumulation that may truncate instead of rounding to nearest.  L = reduction
  length (K for y and dx, the pixel count M for dw and db).  Derivation of the first line: the kernel rounds
  s = fl(sum + bias) to bf16: |bf16(s) - pre| <= u |pre| + (1 + u) A0 with A0 the accumulation error; the second rounding
  adds u |bf16(s) + res| <= u |ref| + u (u |pre| + ...): together u (1 + u) |pre| + u |ref| + A up to terms of order u A0,
  which the factor 2 of A absorbs.
"""
import re

import torch
import torch.nn.functional as F

U = 2.0 ** -8          # relative spacing bound of one bf16 rounding
EPS32 = 2.0 ** -24     # unit round-off of fp32
INT_LIMIT = 2 ** 24

# entry -> (what is computed, the convolution is over the 2x nearest-upsampled input)
ENTRIES = {
    "fwd": ("y", False),               # mdm_conv_fwd_ws on the forward pack
    "dgrad": ("dx", False),            # mdm_conv_fwd_ws on the input-gradient pack (transposed = 1 for stride 2)
    "s2_dgrad": ("dx", False),         # mdm_conv_s2_dgrad_res (sub-pixel input gradient of a stride-2 3x3 convolution)
    "up_fwd": ("y", True),             # mdm_conv_up_fwd
    "up_dgrad": ("dx", True),          # mdm_conv_up_dgrad on the 2x2-blocked output gradient
    "linear_grouped": ("y", False),    # mdm_linear_grouped
    "wgrad": ("dw", False),            # mdm_conv_wgrad + mdm_conv_wgrad_reduce
    "wgrad_blocked": ("dw", True),     # mdm_conv_wgrad_blocked + mdm_conv_wgrad_reduce + mdm_upconv_wfold
    "wgrad_grouped": ("dw", False),    # mdm_conv_wgrad_grouped
}

# name formats of gemm_conv.hip that no bf16 launch produces (fp32 tensors only: tests/test_ops_gpu.py holds them to 2e-5)
FP32_ONLY_FORMATS = ("conv_wgrad_kernel<float, %d>",)


class Row:
    """``shape``: (N, H, W, Cin, Cout, ksize, stride) of the convolution whose forward / input gradient / weight gradient
    the entry computes (up_* and wgrad_blocked: H, W of the LOW-resolution input; the grouped entries: N = rows, H = W = 1),
    or a function of the CU count returning it.  ``knobs``: {index: value} for mdm_dev_set_knob."""

    def __init__(self, id, entry, shape, name, edges, knobs=None, res=False, bias=True, groups=1, splitk=False,
                 round_once=False, wgrid=False, a_factor=2.0, reachable=True, note=""):
        self.id, self.entry, self.shape, self.name, self.edges = id, entry, shape, name, tuple(edges)
        self.knobs = dict(knobs or {})
        self.kind, self.up = ENTRIES[entry]
        self.res = res                # y / dx: a residual is added in the epilogue
        self.bias = bias              # y: bias given; dw: want_bias
        self.groups = groups
        self.splitk = splitk          # a workspace sized by mdm_conv_fwd_plan is passed
        self.round_once = round_once  # Cout % 8 != 0: the scalar branch of conv_epilogue rounds sum + bias + res ONCE
        self.wgrid = wgrid            # random weights on a 1/64 grid in [-1, 1] (see operands)
        self.a_factor = a_factor      # the factor f of A (2 unless the row's note derives another)
        self.reachable = reachable
        self.note = note

    def dims(self, cus=256):
        return self.shape(cus) if callable(self.shape) else self.shape

    def gemm(self, cus=256):
        """(M, N, K) of the GEMM the entry launches"""
        N, H, W, Cin, Cout, ks, stride = self.dims(cus)
        Ho, Wo = out_hw(H, W, ks, stride)
        e = self.entry
        if e in ("fwd", "linear_grouped"):
            return N * Ho * Wo, Cout, ks * ks * Cin
        if e == "dgrad":
            return N * H * W, Cin, ks * ks * Cout
        if e == "s2_dgrad":
            return N * Ho * Wo, 4 * Cin, 4 * Cout
        if e == "up_fwd":
            return N * H * W, 4 * Cout, 4 * Cin
        if e == "up_dgrad":
            return N * H * W, Cin, 16 * Cout
        if e == "wgrad_blocked":
            return N * H * W, 4 * Cout, 9 * Cin
        return N * Ho * Wo, Cout, ks * ks * Cin      # wgrad, wgrad_grouped: (reduction M, Cout, K)

    def __repr__(self):
        return self.id


def out_hw(H, W, ks, stride):
    return (H, W) if ks == 1 else ((H - 1) // stride + 1, (W - 1) // stride + 1)


def _persistent128(ks):
    # 5 column tiles (Cout = 520), so many 128-row tiles that 128x128 tiles outnumber the 2 x CUs resident blocks
    return lambda cus: (3, ((2 * cus) // 5 * 128) // 24 + 2, 8, 64, 520, ks, 1)


def _persistent256(ks):
    # 2 column tiles (Cout = 264), so many 256-row tiles that 256x256 tiles outnumber the CUs (one resident block each)
    return lambda cus: (3, (cus // 2 * 256) // 24 + 2, 8, 64, 264, ks, 1)


GK = "conv_gemm_kernel<bf16, %d, %d, %d, %d, %d>"
BL = "conv_gemm_bl_kernel<%d, %d, %d, %d, %d%s>"
T128, T192, T256 = {2: 128128}, {2: 256192}, {2: 256256}
PR, PC, C8, BB, IB = "partial row tile", "partial column tile", "Cout % 8 != 0", "batch boundary in a row tile", "image borders in a tile"
K1, KODD, KRAG = "single k-tile", "odd number of k-tiles", "ragged last k-tile"
TAIL, SPL = "reduction tail < 64 rows", "split count > 1"
ONCE = ("Cout % 8 != 0 takes the scalar branch of conv_epilogue, which adds bias and residual to the fp32 sum and rounds "
        "ONCE (the chunked branch rounds sum + bias first): the expected value is bf16(sum + bias + res).  Unreachable "
        "through mdm_hip.ops, which pads Cout to a multiple of 8.")
GRID = ("the pack sums the 3x3 taps that fall on one low-resolution pixel and rounds the SUM to bf16; random weights are "
        "drawn from the grid k / 64, |k| <= 64, whose sums of up to four are bf16-exact, so the kernel and the reference "
        "see the same operands")

ROWS = [
    # ---- conv_gemm_kernel<bf16, ...>: K % 64 != 0, the small-Cout tiles, the transposed stride-2 input gradient --------
    Row("gk32_3x3_fwd", "fwd", (5, 7, 5, 24, 20, 3, 1), GK % (128, 32, 4, 1, 1), (PR, PC, C8, BB, IB, KRAG), res=True, round_once=True, note=ONCE),
    Row("gk32_1x1_fwd", "fwd", (2, 9, 7, 40, 32, 1, 1), GK % (128, 32, 4, 1, 0), (PR, BB, K1, KRAG), res=True),
    Row("gk32_1x1_dgrad", "dgrad", (2, 9, 7, 32, 40, 1, 1), GK % (128, 32, 4, 1, 0), (PR, BB, K1, KRAG)),
    Row("gk64_3x3_fwd", "fwd", (2, 12, 11, 24, 52, 3, 1), GK % (128, 64, 2, 2, 1), (PR, PC, C8, BB, IB, KRAG), res=True, round_once=True, note=ONCE),
    Row("gk64_1x1_fwd", "fwd", (2, 12, 11, 72, 64, 1, 1), GK % (128, 64, 2, 2, 0), (PR, BB, KRAG)),
    Row("gk64_3x3_dgrad", "dgrad", (2, 12, 11, 64, 40, 3, 1), GK % (128, 64, 2, 2, 1), (PR, BB, IB, KRAG)),
    Row("gk128_3x3_fwd", "fwd", (3, 10, 12, 40, 132, 3, 1), GK % (128, 128, 2, 2, 1), (PR, PC, C8, BB, IB, KRAG), res=True, round_once=True, note=ONCE),
    Row("gk128_1x1_fwd", "fwd", (3, 10, 12, 72, 136, 1, 1), GK % (128, 128, 2, 2, 0), (PR, PC, BB, KRAG), res=True),
    Row("gk128_3x3_dgrad", "dgrad", (3, 10, 12, 136, 40, 3, 1), GK % (128, 128, 2, 2, 1), (PR, PC, BB, IB, KRAG)),
    Row("gk128_1x1_dgrad", "dgrad", (3, 10, 12, 136, 72, 1, 1), GK % (128, 128, 2, 2, 0), (PR, PC, BB, KRAG)),
    Row("gk256_3x3_fwd", "fwd", (3, 10, 12, 40, 264, 3, 1), GK % (256, 256, 2, 4, 1), (PR, PC, BB, IB, KRAG), T256, res=True),
    Row("gk256_1x1_fwd", "fwd", (3, 10, 12, 72, 264, 1, 1), GK % (256, 256, 2, 4, 0), (PR, PC, BB, KRAG), T256),
    Row("gk256_3x3_dgrad", "dgrad", (3, 10, 12, 264, 40, 3, 1), GK % (256, 256, 2, 4, 1), (PR, PC, BB, IB, KRAG), T256),
    Row("gk32_t2_dgrad", "dgrad", (2, 12, 10, 24, 40, 3, 2), GK % (128, 32, 4, 1, 2), (PR, PC, BB, IB, KRAG)),
    Row("gk128_t2_dgrad", "dgrad", (2, 12, 10, 136, 40, 3, 2), GK % (128, 128, 2, 2, 2), (PR, PC, BB, IB, KRAG)),
    Row("gk256_t2_dgrad", "dgrad", (2, 12, 10, 264, 64, 3, 2), GK % (256, 256, 2, 4, 2), (PR, PC, IB, KODD), T256),
    # ---- conv_gemm_bl_kernel: K % 64 == 0 ------------------------------------------------------------------------------
    Row("bl128s4_3x3_fwd", "fwd", (3, 10, 12, 64, 136, 3, 1), BL % (128, 128, 2, 2, 1, ", 4 stages"), (PR, PC, BB, IB, KODD), res=True),
    Row("bl128s4_1x1_fwd", "fwd", (3, 10, 12, 64, 132, 1, 1), BL % (128, 128, 2, 2, 0, ", 4 stages"), (PR, PC, C8, BB, K1), res=True, round_once=True, note=ONCE),
    Row("bl128s4_3x3_dgrad", "dgrad", (3, 10, 12, 136, 128, 3, 1), BL % (128, 128, 2, 2, 1, ", 4 stages"), (PR, PC, BB, IB)),
    Row("bl128s4_1x1_dgrad", "dgrad", (3, 10, 12, 136, 192, 1, 1), BL % (128, 128, 2, 2, 0, ", 4 stages"), (PR, PC, BB, KODD)),
    Row("bl128s4_s2_fwd", "fwd", (2, 18, 22, 64, 200, 3, 2), BL % (128, 128, 2, 2, 1, ", 4 stages"), (PR, PC, BB, IB, KODD, "stride 2"), res=True),
    Row("bl128p_1x1_fwd", "fwd", _persistent128(1), BL % (128, 128, 2, 2, 0, ""), (PR, PC, BB, K1, "a block's second tile"), T128, res=True),
    Row("bl128p_3x3_fwd", "fwd", _persistent128(3), BL % (128, 128, 2, 2, 1, ""), (PR, PC, BB, IB, KODD, "a block's second tile"), T128),
    Row("bl192_3x3_fwd", "fwd", (3, 10, 12, 64, 200, 3, 1), BL % (256, 192, 2, 4, 1, ""), (PR, PC, BB, IB, KODD), T192, res=True),
    Row("bl192_1x1_fwd", "fwd", (3, 10, 12, 128, 200, 1, 1), BL % (256, 192, 2, 4, 0, ""), (PR, PC, BB), T192),
    Row("bl192_3x3_dgrad", "dgrad", (3, 10, 12, 200, 64, 3, 1), BL % (256, 192, 2, 4, 1, ""), (PR, PC, BB, IB, KODD), T192),
    Row("bl256_3x3_fwd", "fwd", (2, 12, 12, 256, 264, 3, 1), BL % (256, 256, 2, 4, 1, ""), (PR, PC, BB, IB), T256, res=True),
    Row("bl256_1x1_fwd", "fwd", (3, 10, 12, 192, 264, 1, 1), BL % (256, 256, 2, 4, 0, ""), (PR, PC, BB, KODD), T256, res=True),
    Row("bl256_1x1_dgrad", "dgrad", (3, 10, 12, 264, 192, 1, 1), BL % (256, 256, 2, 4, 0, ""), (PR, PC, BB, KODD), T256),
    Row("bl256_s2_fwd", "fwd", (2, 18, 22, 64, 264, 3, 2), BL % (256, 256, 2, 4, 1, ""), (PR, PC, BB, IB, KODD, "stride 2"), T256),
    Row("bl256p_1x1_fwd", "fwd", _persistent256(1), BL % (256, 256, 2, 4, 0, ""), (PR, PC, BB, K1, "a block's second tile"), T256, res=True),
    Row("bl256p_3x3_fwd", "fwd", _persistent256(3), BL % (256, 256, 2, 4, 1, ""), (PR, PC, BB, IB, KODD, "a block's second tile"), T256),
    # split-K (27 resp. 25 k-tiles over 4 ranges: 7 + 7 + 7 + 6 resp. 7 + 7 + 7 + 4)
    Row("splitk_3x3_fwd", "fwd", (2, 9, 7, 192, 136, 3, 1), BL % (128, 128, 2, 2, 1, ", splitk x4"), (PR, PC, BB, IB, KODD, "uneven k ranges"), res=True, splitk=True),
    Row("splitk_1x1_fwd", "fwd", (2, 9, 7, 1600, 136, 1, 1), BL % (128, 128, 2, 2, 0, ", splitk x4"), (PR, PC, BB, KODD, "uneven k ranges"), splitk=True,
        note="Cin = 1600: a 1x1 problem needs >= 24 k-tiles before the plan splits it"),
    # sel4: the sub-pixel forms of the resampling convolutions
    Row("sel4_128_s2dgrad", "s2_dgrad", (3, 20, 12, 128, 64, 3, 2), BL % (128, 128, 2, 2, 1, ", sel4"), (PR, BB, IB)),
    Row("sel4_128_s2dgrad_res", "s2_dgrad", (3, 20, 12, 128, 64, 3, 2), BL % (128, 128, 2, 2, 1, ", sel4"), (PR, BB, IB), res=True),
    Row("sel4_192_s2dgrad_res", "s2_dgrad", (3, 20, 12, 384, 64, 3, 2), BL % (256, 192, 2, 4, 1, ", sel4"), (PR, BB, IB), res=True),
    Row("sel4_256_s2dgrad", "s2_dgrad", (3, 20, 12, 256, 64, 3, 2), BL % (256, 256, 2, 4, 1, ", sel4"), (PR, BB, IB)),
    Row("sel4_128_up_fwd", "up_fwd", (3, 9, 7, 64, 128, 3, 1), BL % (128, 128, 2, 2, 1, ", sel4"), (PR, BB, IB), wgrid=True, note=GRID),
    Row("sel4_192_up_fwd", "up_fwd", (3, 9, 7, 64, 192, 3, 1), BL % (256, 192, 2, 4, 1, ", sel4"), (PR, BB, IB), wgrid=True, note=GRID),
    Row("sel4_256_up_fwd", "up_fwd", (3, 9, 7, 64, 256, 3, 1), BL % (256, 256, 2, 4, 1, ", sel4"), (PR, BB, IB), wgrid=True, note=GRID),
    Row("sel4_128_up_dgrad", "up_dgrad", (3, 9, 7, 192, 64, 3, 1), BL % (128, 128, 2, 2, 1, ", sel4"), (PR, PC, BB, IB), wgrid=True, note=GRID),
    Row("sel4_192_up_dgrad", "up_dgrad", (3, 9, 7, 320, 64, 3, 1), BL % (256, 192, 2, 4, 1, ", sel4"), (PR, PC, BB, IB), T192, wgrid=True, note=GRID),
    Row("sel4_256_up_dgrad", "up_dgrad", (3, 9, 7, 320, 64, 3, 1), BL % (256, 256, 2, 4, 1, ", sel4"), (PR, PC, BB, IB), T256, wgrid=True, note=GRID),
    # grouped linear layers
    Row("grouped128", "linear_grouped", (150, 1, 1, 128, 200, 1, 1), BL % (128, 128, 2, 2, 0, ", grouped"), (PR, PC), groups=3),
    Row("grouped192", "linear_grouped", (150, 1, 1, 128, 200, 1, 1), BL % (256, 192, 2, 4, 0, ", grouped"), (PR, PC), T192, groups=3),
    Row("grouped256", "linear_grouped", (150, 1, 1, 192, 264, 1, 1), BL % (256, 256, 2, 4, 0, ", grouped"), (PR, PC, KODD), T256, groups=4),
    # ---- the direct kernels: their size gates (>= 65536 resp. >= 262144 pixels) make these the only large rows ----------
    Row("direct_32_32", "fwd", (2, 128, 256, 32, 32, 3, 1), "conv3x3_direct_kernel<32, 32, 8, 64, 2>", (BB, IB), res=True),
    Row("direct_32_64", "fwd", (2, 128, 256, 32, 64, 3, 1), "conv3x3_direct_kernel<32, 64, 8, 64, 4>", (BB, IB)),
    Row("direct_64_32", "fwd", (2, 128, 256, 64, 32, 3, 1), "conv3x3_direct_kernel<64, 32, 8, 32, 2>", (BB, IB), res=True),
    Row("direct_64_64", "fwd", (2, 128, 256, 64, 64, 3, 1), "conv3x3_direct_kernel<64, 64, 8, 32, 4>", (BB, IB)),
    Row("direct_64_32_dgrad", "dgrad", (2, 128, 256, 32, 64, 3, 1), "conv3x3_direct_kernel<64, 32, 8, 32, 2>", (BB, IB)),
    Row("wgrad_direct", "wgrad", (4, 256, 256, 64, 64, 3, 1), "wgrad_direct_kernel<64, 9, 8>", (BB, IB, SPL)),
    # ---- weight gradients ----------------------------------------------------------------------------------------------
    Row("wg_tr128_3x3", "wgrad", (3, 14, 15, 72, 72, 3, 1), "conv_wgrad_tr_kernel<1, 0>", (PR, PC, BB, IB, TAIL, SPL)),
    Row("wg_tr128_3x3_nobias", "wgrad", (3, 14, 15, 72, 72, 3, 1), "conv_wgrad_tr_kernel<1, 0>", (PR, PC, BB, IB, TAIL, SPL), bias=False),
    Row("wg_tr256_3x3", "wgrad", (3, 14, 15, 72, 200, 3, 1), "conv_wgrad_tr_kernel<1, 1>", (PR, PC, BB, IB, TAIL, SPL), {3: 256}),
    Row("wg_tr128_s2", "wgrad", (3, 28, 30, 64, 72, 3, 2), "conv_wgrad_tr_kernel<1, 0>", (PR, PC, BB, IB, TAIL, SPL, "stride 2")),
    Row("wg_tr256_s2", "wgrad", (3, 28, 30, 64, 200, 3, 2), "conv_wgrad_tr_kernel<1, 1>", (PR, PC, BB, IB, TAIL, SPL, "stride 2"), {3: 256}, bias=False),
    Row("wg_tr128_1x1", "wgrad", (5, 9, 14, 64, 136, 1, 1), "conv_wgrad_tr_kernel<0, 0>", (), reachable=False,
        note="a 1x1 weight gradient leaves conv_wgrad_bl_kernel only when an operand exceeds 0x7F000000 bytes (wgrad_bl_ok): "
             "over a billion elements, no test-sized shape"),
    Row("wg_tr256_1x1", "wgrad", (5, 9, 14, 200, 264, 1, 1), "conv_wgrad_tr_kernel<0, 1>", (), {3: 256}, reachable=False,
        note="as wg_tr128_1x1"),
    Row("wg_bl128_3x3", "wgrad", (19, 4, 8, 64, 72, 3, 1), "conv_wgrad_bl_kernel<1, 0>", (PR, PC, BB, IB, TAIL, SPL)),
    Row("wg_bl256_3x3", "wgrad", (19, 4, 8, 64, 200, 3, 1), "conv_wgrad_bl_kernel<1, 1>", (PR, PC, BB, IB, TAIL, SPL), {3: 256}, bias=False),
    Row("wg_bl128_1x1", "wgrad", (5, 9, 14, 64, 136, 1, 1), "conv_wgrad_bl_kernel<0, 0>", (PR, PC, TAIL, SPL)),
    Row("wg_bl128_1x1_nobias", "wgrad", (5, 9, 14, 64, 136, 1, 1), "conv_wgrad_bl_kernel<0, 0>", (PR, PC, TAIL, SPL), bias=False),
    Row("wg_bl256_1x1", "wgrad", (5, 9, 14, 200, 264, 1, 1), "conv_wgrad_bl_kernel<0, 1>", (PR, PC, TAIL, SPL), {3: 256}),
    Row("wg_blocked128", "wgrad_blocked", (31, 4, 8, 256, 256, 3, 1), "conv_wgrad_bl_kernel<1, 0>", (BB, IB, TAIL, SPL), {3: 128}),
    Row("wg_blocked256", "wgrad_blocked", (31, 4, 8, 256, 256, 3, 1), "conv_wgrad_bl_kernel<1, 1>", (BB, IB, TAIL, SPL), {3: 256}),
    Row("wg_grouped128", "wgrad_grouped", (150, 1, 1, 136, 200, 1, 1), "conv_wgrad_bl_kernel<0, 0>", (PR, PC, TAIL), groups=3),
    Row("wg_grouped128_forced", "wgrad_grouped", (150, 1, 1, 200, 264, 1, 1), "conv_wgrad_bl_kernel<0, 0>", (PR, PC, TAIL), {3: 128}, groups=3, bias=False),
    Row("wg_grouped256", "wgrad_grouped", (150, 1, 1, 200, 264, 1, 1), "conv_wgrad_bl_kernel<0, 1>", (PR, PC, TAIL), groups=3),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
KINDS = ("int", "impulse", "random")


# ---- operands ----------------------------------------------------------------------------------------------------------
def bf16r(t):
    """round to bf16 (to nearest even), keep the dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _seed(row, kind, g):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(row.id)) * 7 + KINDS.index(kind) * 3 + g * 1009) % (2 ** 31)


def _impulse_mask(N, H, W):
    """1 at the four corners of image 0 and at the first and last pixel of a sample in the middle of the batch"""
    m = torch.zeros(N, 1, H, W, dtype=torch.float64)
    for h, w in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m[0, 0, h, w] = 1
    m[N // 2, 0, 0, 0] = 1
    m[N // 2, 0, H - 1, W - 1] = 1
    return m


def operands(row, kind, cus=256, g=0):
    """fp64 CPU operands of group ``g`` of a row (NCHW / OIHW): x, w, b (or None), res (or None: y / dx rows with a
    residual), dy (dx / dw rows).  'int' and 'impulse': small integers; 'random': normal, rounded to bf16 (bias: fp32)."""
    N, H, W, Cin, Cout, ks, stride = row.dims(cus)
    up = 2 if row.up else 1
    Ho, Wo = out_hw(H * up, W * up, ks, stride)
    gen = torch.Generator().manual_seed(_seed(row, kind, g))
    f64 = torch.float64
    o = {"stride": stride, "up": row.up}
    if kind == "random":
        o["x"] = bf16r(torch.randn(N, Cin, H, W, generator=gen, dtype=f64))
        if row.wgrid:
            o["w"] = (torch.randn(Cout, Cin, ks, ks, generator=gen, dtype=f64) * 24).round().clamp(-64, 64) / 64
        else:
            o["w"] = bf16r(torch.randn(Cout, Cin, ks, ks, generator=gen, dtype=f64) / (Cin * ks * ks) ** 0.5)
        o["b"] = torch.randn(Cout, generator=gen, dtype=f64).float().double()
        o["dy"] = bf16r(torch.randn(N, Cout, Ho, Wo, generator=gen, dtype=f64))
        rshape = (N, Cout, Ho, Wo) if row.kind == "y" else (N, Cin, H, W)
        o["res"] = bf16r(torch.randn(rshape, generator=gen, dtype=f64))
    else:
        def ints(shape, lo, hi, half_zero):
            t = torch.randint(lo, hi + 1, shape, generator=gen).double()
            if half_zero:
                t = t * (torch.rand(shape, generator=gen) < 0.5)
            return t
        o["x"] = ints((N, Cin, H, W), -3, 3, True)
        # the weight differs per (tap, input channel mod 7, output channel mod 11): a swapped or shifted tap shows
        tap = torch.arange(ks * ks).view(1, 1, ks, ks)
        ci = torch.arange(Cin).view(1, Cin, 1, 1) % 7
        co = torch.arange(Cout).view(Cout, 1, 1, 1) % 11
        o["w"] = ((tap * 5 + ci * 3 + co + g) % 7 - 3).double()
        o["b"] = ((torch.arange(Cout) * 5 + g) % 23 - 11).double()
        o["dy"] = ints((N, Cout, Ho, Wo), -3, 3, True)
        rshape = (N, Cout, Ho, Wo) if row.kind == "y" else (N, Cin, H, W)
        o["res"] = ints(rshape, -9, 9, False)
        if kind == "impulse":   # the activation operand is zero but for single pixels (all of their channels)
            if row.kind == "dx":
                o["dy"] = torch.randint(1, 4, (N, Cout, Ho, Wo), generator=gen).double() * _impulse_mask(N, Ho, Wo)
            else:
                o["x"] = torch.randint(1, 4, (N, Cin, H, W), generator=gen).double() * _impulse_mask(N, H, W)
    if not (row.kind == "y" and row.bias):
        o["b"] = None
    if not (row.res and row.kind in ("y", "dx")):
        o["res"] = None
    return o


# ---- the operation, in any precision -----------------------------------------------------------------------------------
def _conv(x, w, b, stride, up):
    if up:
        x = F.interpolate(x, scale_factor=2)
    return F.conv2d(x, w, b, stride=stride, padding=(w.shape[-1] - 1) // 2)


def compute(kind, o, dtype=torch.float64, absolute=False):
    """{'y'} / {'dx'} / {'dw', 'db'} of the row's operation BEFORE any residual, in ``dtype``; ``absolute``: on the
    operands' magnitudes (the sum of absolute products that A and the 2^24 condition need)"""
    c = (lambda t: None if t is None else (t.abs() if absolute else t).to(dtype))
    x, w, b, dy = c(o["x"]), c(o["w"]), c(o["b"]), c(o["dy"])
    if kind == "y":
        return {"y": _conv(x, w, b, o["stride"], o["up"])}
    if kind == "dx":
        x = x.clone().requires_grad_()
        return {"dx": torch.autograd.grad(_conv(x, w, None, o["stride"], o["up"]), x, dy)[0]}
    if o["up"]:
        x = F.interpolate(x, scale_factor=2)
    # (the weight-gradient node of F.conv2d's autograd, without running the forward first)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=o["stride"], padding=(w.shape[-1] - 1) // 2)
    return {"dw": dw, "db": dy.sum((0, 2, 3))}


def reduction_length(row, cus=256):
    """L of A: additions behind one output element"""
    N, H, W, Cin, Cout, ks, stride = row.dims(cus)
    up = 2 if row.up else 1
    if row.kind == "y":
        return ks * ks * Cin + 1
    if row.kind == "dx":
        return ks * ks * Cout * up * up
    Ho, Wo = out_hw(H * up, W * up, ks, stride)
    return N * Ho * Wo


class Expect:
    """per output: ref (fp64, with the residual), pre (before it), A, whether it is stored as bf16"""

    def __init__(self, ref, pre, A, is_bf16, has_res):
        self.ref, self.pre, self.A, self.is_bf16, self.has_res = ref, pre, A, is_bf16, has_res

    def bound(self):
        if not self.is_bf16:
            return self.A
        if self.has_res:
            return U * (1 + U) * self.pre.abs() + U * self.ref.abs() + self.A
        return U * self.ref.abs() + self.A


def reference(row, o, cus=256):
    """{output: Expect} of one group's operands, from the fp64 operation and the same operation on absolute values"""
    pre = compute(row.kind, o)
    mag = compute(row.kind, o, absolute=True)
    L = reduction_length(row, cus)
    out = {}
    for k, v in pre.items():
        if k == "db" and not row.bias:
            continue
        res = o["res"] if k in ("y", "dx") else None
        A = row.a_factor * L * EPS32 * mag[k]
        out[k] = Expect(v if res is None else v + res, v, A, k in ("y", "dx"), res is not None)
        out[k].mag = mag[k]
    return out


def int_condition(exp):
    """largest magnitude any fp32 partial sum of the integer problem can reach (must stay below 2^24)"""
    return max(float(max(e.mag.max(), e.ref.abs().max())) for e in exp.values())


def int_expected(row, e):
    """what a kernel with exact fp32 accumulation must store"""
    if not e.is_bf16:
        return e.ref
    if not e.has_res or row.round_once:
        return bf16r(e.ref)
    return bf16r(bf16r(e.pre) + (e.ref - e.pre))


def emulate(row, o, dtype=torch.float32):
    """CPU emulation of the kernels' arithmetic: the operation in fp32, then the epilogue's bf16 roundings"""
    got = compute(row.kind, o, dtype)
    out = {}
    for k, v in got.items():
        if k == "db" and not row.bias:
            continue
        if k in ("y", "dx"):
            out[k] = epilogue(row, v, o["res"])
        else:
            out[k] = v.double()
    return out


def epilogue(row, s, res):
    """fp32 sum (+ bias) -> the stored bf16 value, as fp64"""
    s = s.float()
    if res is None:
        return bf16r(s).double()
    if row.round_once:
        return bf16r(s + res.float()).double()
    return bf16r(bf16r(s) + res.float()).double()


# ---- gates -------------------------------------------------------------------------------------------------------------
def int_mismatches(got, want):
    """number of elements that differ (a NaN differs)"""
    return int((~(got.double() == want)).sum())


def bound_ratio(got, e):
    """(worst |got - ref| / bound, number of elements over the bound); an element with bound 0 must be exact"""
    diff = (got.double() - e.ref).abs()
    bound = e.bound()
    ratio = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    ratio = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), ratio)
    return float(ratio.max()), int((ratio > 1).sum())


def old_relerr(got, ref):
    """the gate of tests/test_ops_gpu.py: max |a - b| / max |b|"""
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


# ---- the name formats of the source ------------------------------------------------------------------------------------
def note_kernel_formats(source_text):
    """the distinct format strings of the MDM_NOTE_KERNEL(...) lines"""
    fmts = re.findall(r'MDM_NOTE_KERNEL\("([^"]+)"', source_text)
    return sorted(set(fmts))


def format_regex(fmt):
    return re.compile("^" + re.escape(fmt).replace("%d", r"\d+").replace("%s", r".+") + "$")
