"""Shared by tests/test_fp8_conv_host.py (CPU) and tests/test_fp8_conv_gpu.py (GPU): the fp64 restatement of the MXFP8 3x3
convolution (csrc/fp8.hip, CONV form of mx8_gemm_kernel) on the operand format of tests/fp8_cases.py,
its integer-data operands, and the fake-quant oracle that also covers the ResNet convolutions.

The restatement is the kernel's row indexing written down independently: the activation is [M = N H W, Kp] rows of one pixel
each, the weight [Cout 9, Kp] with row o 9 + ky 3 + kx, and the output is a sum over nine GEMMs on rows shifted by
dy W + dx, a row taking part only where (y + dy, x + dx) lies inside the image -- tested on (y, x), not on the flat index.
tests/test_fp8_conv_host.py pins it to ``F.conv2d(..., padding=1)``."""
import torch

import fp8_cases as FC
import parity_cases as PC
import unet_oracle as O

# (N, H, W, Cin, Cout), each the smallest that exercises one way to go wrong:
#   (2, 5, 3, 32, 32)     M = 30, one ragged tile; every pixel touches a border; an image seam inside the tile; Kp 3/4 padding
#   (2, 1, 4, 32, 32)     H = 1: six of the nine taps are never valid
#   (1, 8, 8, 288, 96)    288 -> Kp 384: three k-tiles per tap, the last mostly padding; Cout ragged in its N tile
#   (3, 9, 7, 256, 160)   M = 189: two M tiles with the seam mid-tile and a ragged end; two N tiles; two k-tiles per tap
CONV_SHAPES = [(2, 5, 3, 32, 32), (2, 1, 4, 32, 32), (1, 8, 8, 288, 96), (3, 9, 7, 256, 160)]
CONV_SUFFIXES = ("conv1", "conv2", "conv3")


def pad_k(q, s):
    """codes [R, K], scale bytes [R, K / 32] -> the padded form [R, Kp], [R, Kp / 32] (code 0, scale 127), Kp = K up to 128"""
    R, K = q.shape
    Kp = FC.round_up(K, 128)
    qp = torch.zeros(R, Kp, dtype=torch.uint8)
    sp = torch.full((R, Kp // 32), 127, dtype=torch.uint8)
    qp[:, :K], sp[:, : K // 32] = q, s
    return qp, sp


def with_zero_row(q, s):
    """the activation as the kernel takes it: one more row, codes 0 and scales 127"""
    return (torch.cat([q, torch.zeros(1, q.shape[1], dtype=torch.uint8)]),
            torch.cat([s, torch.full((1, s.shape[1]), 127, dtype=torch.uint8)]))


def conv_ref(qa, sa, qw, sw, shape):
    """fp64 [N, H, W, Cout]: the sum over nine shifted-row GEMMs on the dequantised operands; qa / sa hold N H W rows (a
    zero row behind them is ignored: invalid taps simply do not take part here), qw / sw the Cout 9 weight rows"""
    N, H, W = shape
    M = N * H * W
    a = FC.dequant_ref(qa[:M], sa[:M])
    cout = qw.shape[0] // 9
    w = FC.dequant_ref(qw, sw).reshape(cout, 9, -1)
    m = torch.arange(M)
    x, y = m % W, (m // W) % H
    out = torch.zeros(M, cout, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dy, dx = ky - 1, kx - 1
            ok = (y + dy >= 0) & (y + dy < H) & (x + dx >= 0) & (x + dx < W)
            out[ok] += a[m[ok] + dy * W + dx] @ w[:, ky * 3 + kx].t()
    return out.reshape(N, H, W, cout)


def as_conv2d_operands(qa, sa, qw, sw, shape, cin):
    """the same dequantised operands in torch's layouts: x [N, Cin, H, W], w [Cout, Cin, 3, 3] (fp64)"""
    N, H, W = shape
    x = FC.dequant_ref(qa[: N * H * W], sa[: N * H * W])[:, :cin].reshape(N, H, W, cin).permute(0, 3, 1, 2)
    w = FC.dequant_ref(qw, sw)[:, :cin].reshape(-1, 3, 3, cin).permute(0, 3, 1, 2)
    return x.contiguous(), w.contiguous()


def exact_operands(N, H, W, cin, cout):
    """``FC.exact_case(M, 9 Cout, Cin)`` (codes in -4 .. 4, seven power-of-two scales per operand) padded to Kp"""
    qa, sa, qw, sw = FC.exact_case(N * H * W, 9 * cout, cin)
    return pad_k(qa, sa) + pad_k(qw, sw)


def quant_weight_3x3(w):
    """w (Cout, Cin, 3, 3) -> (codes, scale bytes) of [Cout 9, Cin]: row o 9 + ky 3 + kx, blocks over input channels"""
    return FC.quant_ref(w.permute(0, 2, 3, 1).reshape(w.shape[0] * 9, w.shape[1]))


# ---- fake-quant oracle ----------------------------------------------------------------------------------------------------
def fake_quant_conv(real_conv, suffixes):
    """a replacement for ``unet_oracle._conv``: the convolutions whose name ends in one of ``suffixes`` see their input
    quantised and dequantised per pixel over channels, and their weight per (output channel, tap) over input channels --
    the weight is permuted to (O, ky, kx, I) first (flattening (O, I, ky, kx) as ``fp8_cases.fake_quant_conv`` does is right
    for 1x1 only).  The input of ``ffn.3`` is rounded through bf16 first, as there."""

    def conv(sd, name, x, stride=1):
        if not name.endswith(suffixes):
            return real_conv(sd, name, x, stride)
        w = sd[name + ".weight"]
        B, C, H, W = x.shape
        if name.endswith("ffn.3"):
            x = x.to(torch.bfloat16).to(x.dtype)
        x2 = FC.fake_quant(x.permute(0, 2, 3, 1).reshape(-1, C)).reshape(B, H, W, C).permute(0, 3, 1, 2)
        co, ci, kh, kw = w.shape
        w2 = FC.fake_quant(w.permute(0, 2, 3, 1).reshape(co * kh * kw, ci)).reshape(co, kh, kw, ci).permute(0, 3, 1, 2)
        sd2 = {name + ".weight": w2}
        if name + ".bias" in sd:
            sd2[name + ".bias"] = sd[name + ".bias"]
        return real_conv(sd2, name, x2, stride)

    return conv


def oracle_fake_quant_run(name, dtype, monkeypatch, attention=False):
    """the oracle's forward with conv1 / conv2 / conv3 of every ResNet (and, with ``attention``, the four attention-layer
    projections) fake-quantised (no gradients)"""
    suffixes = CONV_SUFFIXES + (FC.FAKE_QUANT_SUFFIXES if attention else ())
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(O, "_conv", fake_quant_conv(O._conv, suffixes))
        return PC.oracle_run(name, dtype, with_grad=False)[0]
