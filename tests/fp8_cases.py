"""Shared by tests/test_fp8_host.py (CPU) and tests/test_fp8_gpu.py (GPU): the fp64 / torch restatement of the MXFP8
quantiser (OCP MX, E4M3 codes + one E8M0 scale byte per 32 consecutive K elements), its inverse, the
GEMM reference on dequantised operands, and a fake-quant form of the oracle.

The restatement shares nothing with csrc/fp8.hip: floor(log2) comes from ``torch.frexp`` in fp64, the codes from torch's
own ``float8_e4m3fn`` cast (after the explicit clamp: the cast alone makes NaN above 464)."""
import torch
import torch.nn.functional as F

import parity_cases as PC
import unet_oracle as O

QUANT_SHAPES = [(1, 32), (5, 96), (80, 256), (33, 1024)]
# (M, N, K): one tile; a ragged column tile (N = 96) with K = 3 k-tiles; a partial row tile past 256 with the mini FFN's K
GEMM_SHAPES = [(16, 32, 128), (80, 96, 384), (272, 256, 1024)]
FAKE_QUANT_SUFFIXES = ("qkv", "proj_out", "ffn.1", "ffn.3")


def round_up(v, m):
    return (v + m - 1) // m * m


def quant_ref(x):
    """x [M, K] (any float dtype, CPU) -> (codes uint8 [M, Kp], scale bytes uint8 [M, Kp / 32]), Kp = K rounded up to 128"""
    x = x.detach().double()
    M, K = x.shape
    Kp = round_up(K, 128)
    xp = torch.zeros(M, Kp, dtype=torch.float64)
    xp[:, :K] = x
    b = xp.reshape(M, Kp // 32, 32)
    amax = b.abs().amax(-1)
    _, ex = torch.frexp(amax)                      # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex.to(torch.int64) - 1 - 8, torch.zeros_like(ex, dtype=torch.int64)).clamp(-127, 127)
    scaled = (b * torch.exp2(-e.double()).unsqueeze(-1)).clamp(-448.0, 448.0)
    codes = scaled.float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(M, Kp)
    return codes, (e + 127).to(torch.uint8)


def dequant_ref(codes, scales):
    """-> fp64 [M, Kp]"""
    v = codes.view(torch.float8_e4m3fn).double()
    return v * torch.exp2(scales.double() - 127.0).repeat_interleave(32, dim=1)


def fake_quant(x):
    """x [M, K] -> dequant(quant(x)) [M, K] in x's dtype (every MXFP8 value is a bf16 value: 4 significant bits)"""
    q, s = quant_ref(x)
    return dequant_ref(q, s)[:, : x.shape[1]].to(x.dtype)


def gemm_ref(qa, sa, qw, sw):
    """fp64 A W^T on the dequantised operands"""
    return dequant_ref(qa, sa) @ dequant_ref(qw, sw).t()


def exact_case(M, N, K):
    """integer codes in {-4 .. 4} (half of them zero) and power-of-two scales in [2^-3, 2^3] that differ from block to block
    and row to row, A and W built differently; row 1 of A is one-hot per block.  Every product and every partial sum is an
    integer multiple of 2^-6 below 2^18 in magnitude (checked by the caller): exact in fp32 in any summation order."""
    g = torch.Generator().manual_seed(1000 + M + N + K)
    nb = K // 32
    a = torch.randint(-4, 5, (M, K), generator=g).double() * (torch.rand(M, K, generator=g) < 0.5)
    w = torch.randint(-4, 5, (N, K), generator=g).double() * (torch.rand(N, K, generator=g) < 0.5)
    row = min(1, M - 1)
    a[row] = 0
    for blk in range(nb):
        a[row, 32 * blk + (7 * blk + 3) % 32] = 1.0
    r, c, kb = torch.arange(M).unsqueeze(1), torch.arange(N).unsqueeze(1), torch.arange(nb).unsqueeze(0)
    sa = ((5 * r + 3 * kb) % 7 - 3 + 127).to(torch.uint8)
    sw = ((3 * c + kb + 2) % 7 - 3 + 127).to(torch.uint8)
    qa = a.float().to(torch.float8_e4m3fn).view(torch.uint8)
    qw = w.float().to(torch.float8_e4m3fn).view(torch.uint8)
    return qa, sa, qw, sw


def gelu_ref(v):
    return F.gelu(v)          # the exact (erf) form; the kernels' polynomial is gated at the bf16 op gate


# ---- fake-quant oracle ----------------------------------------------------------------------------------------------------
def fake_quant_conv(real_conv):
    """a replacement for ``unet_oracle._conv``: the 1x1 convolutions named ``*qkv``, ``*proj_out``, ``*ffn.1`` and ``*ffn.3``
    see input (per pixel, over channels) and weight (per output channel, over input channels) quantised and dequantised;
    the FFN hidden tensor (the input of ``ffn.3``) is rounded through bf16 first, as the first GEMM's epilogue emits it"""

    def conv(sd, name, x, stride=1):
        if not name.endswith(FAKE_QUANT_SUFFIXES):
            return real_conv(sd, name, x, stride)
        w = sd[name + ".weight"]
        B, C, H, W = x.shape
        if name.endswith("ffn.3"):
            x = x.to(torch.bfloat16).to(x.dtype)
        x2 = fake_quant(x.permute(0, 2, 3, 1).reshape(-1, C)).reshape(B, H, W, C).permute(0, 3, 1, 2)
        w2 = fake_quant(w.reshape(w.shape[0], -1)).reshape(w.shape)
        sd2 = {name + ".weight": w2}
        if name + ".bias" in sd:
            sd2[name + ".bias"] = sd[name + ".bias"]
        return real_conv(sd2, name, x2, stride)

    return conv


def oracle_fake_quant_run(name, dtype, monkeypatch):
    """the oracle's forward with the four projections fake-quantised (no gradients)"""
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(O, "_conv", fake_quant_conv(O._conv))
        return PC.oracle_run(name, dtype, with_grad=False)[0]
