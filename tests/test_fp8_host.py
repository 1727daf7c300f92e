"""CPU: the MXFP8 restatement of tests/fp8_cases.py against hand-written vectors, its round trip, the exported symbols,
the static scans of the new kernels, and the host logic of ``mdm_hip.fp8`` (attach / detach, refusals) on CPU-built mini
models."""
import os
import shutil

import pytest
import torch
import torch.nn as nn

import fp8_cases as FC
import parity_cases as PC
import stub_models as SM
from mdm_hip import fp8, lora, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_zero_block_and_padding():
    x = torch.zeros(2, 96)
    x[1, 64:96] = torch.arange(32, dtype=torch.float32) - 16.0          # amax 16 = 2^4: e = -4, 16 * 2^4 = 256
    q, s = FC.quant_ref(x)
    assert q.shape == (2, 128) and s.shape == (2, 4) and q.dtype == s.dtype == torch.uint8
    assert int(q[0].max()) == 0 and s[0].tolist() == [127, 127, 127, 127]      # zero blocks: scale 127, codes 0
    assert s[1].tolist() == [127, 127, 127 - 4, 127] and int(q[1, 96:].max()) == 0   # K = 96: the 4th block is padding
    # -16 -> -256 = -(2^8): sign 1, exponent field 15, mantissa 0 = 0xF8;  -15 -> -240 = -1.875 * 2^7: 0xF7;  1 -> 16 = 2^4: 0x58
    assert q[1, 64].item() == 0xF8 and q[1, 65].item() == 0xF7 and q[1, 64 + 17].item() == 0x58 and q[1, 64 + 16].item() == 0
    assert torch.equal(FC.dequant_ref(q, s)[:, :96], x.double())        # these values are exact in e4m3


def test_saturating_block():
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 480.0, -500.0, 1.0, -2.0       # amax 500: floor(log2) = 8, e = 0; 480, 500 in (448, 512)
    q, s = FC.quant_ref(x)
    assert s[0, 0].item() == 127
    assert q[0, :4].tolist() == [0x7E, 0xFE, 0x38, 0xC0]                # +-448 (never the NaN code 0x7F), 1.0, -2.0
    q2, s2 = FC.quant_ref(x / 2)                                        # amax 250: e = -1, the same scaled values
    assert s2[0, 0].item() == 126 and q2[0, :4].tolist() == [0x7E, 0xFE, 0x38, 0xC0]


def test_exponent_clamps():
    tiny = torch.zeros(1, 32)
    tiny[0, 5] = 2.0 ** -140                                            # an fp32 subnormal: floor(log2) - 8 = -148 -> -127
    q, s = FC.quant_ref(tiny)
    assert s[0, 0].item() == 0 and int(q.max()) == 0                    # 2^-140 * 2^127 = 2^-13 rounds to 0 (half the least code: 2^-10)
    big = torch.zeros(1, 32)
    big[0, 0], big[0, 1] = 2.0 ** 127, -(2.0 ** 120)
    q, s = FC.quant_ref(big)
    assert s[0, 0].item() == 127 + 119 and q[0, 0].item() == 0x78 and q[0, 1].item() == 0xC0   # 2^8 and -(2^1)
    small = torch.zeros(1, 32)
    small[0, 0] = 2.0 ** -126                                           # e = -134 -> -127: 2^-126 * 2^127 = 2
    q, s = FC.quant_ref(small)
    assert s[0, 0].item() == 0 and q[0, 0].item() == 0x40


@pytest.mark.parametrize("M,K", FC.QUANT_SHAPES)
def test_quant_of_dequant_is_the_identity(M, K):
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
    q, s = FC.quant_ref(x)
    assert not bool((q & 0x7F).eq(0x7F).any())                          # no NaN code
    back = FC.dequant_ref(q, s)[:, :K]
    q2, s2 = FC.quant_ref(back)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # the format's error: e4m3 has 3 mantissa bits, the block's largest value sits in [256, 512) of the code range
    rel = float((back - x.double()).norm() / x.double().norm())
    print("[mx8 restatement M=%d K=%d] rel-L2 of the round trip %.3e" % (M, K, rel))
    assert rel < 2.0 ** -4


def test_exact_case_is_exact_in_fp32():
    for M, N, K in FC.GEMM_SHAPES:
        qa, sa, qw, sw = FC.exact_case(M, N, K)
        a, w = FC.dequant_ref(qa, sa), FC.dequant_ref(qw, sw)
        assert float((a.abs() @ w.abs().t()).max()) < 2.0 ** 18         # every partial sum, in any order
        assert torch.equal((a * 64).round(), a * 64) and not torch.equal(a[:N, :], w[:M, :])
        assert len(set(sa.flatten().tolist())) == 7 and len(set(sw.flatten().tolist())) == 7


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_symbols_resolve_and_abi_stays_6():
    from mdm_hip import _lib

    L = _lib.lib()
    names = {p[0] for p in _lib.header_prototypes()}
    for n in ("mdm_mx8_quant", "mdm_mx8_gemm"):
        assert n in names and hasattr(L, n)
    assert L.mdm_abi_version() == _lib.ABI_VERSION == 6 and "fp8.hip" in _lib.SOURCES
    # invalid arguments are reported, not executed
    assert L.mdm_mx8_quant(None, 1, 4, 32, 128, None, None, None) < 0
    assert L.mdm_mx8_gemm(None, None, None, None, None, None, None, None, None, 16, 32, 128, 0, None) < 0


def test_new_kernels_pass_the_static_scans():
    """tools/mfma_hazard_scan.py over csrc/fp8.hip: no early read of an MFMA result on any path, no spilled registers past
    the cap, and no vector load between the wide stores of the GEMM's epilogue"""
    import importlib.util
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("mfma_hazard_scan", os.path.join(ROOT, "tools", "mfma_hazard_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = sys.argv
    sys.argv = ["mfma_hazard_scan.py", "fp8.hip"]
    try:
        assert mod.main() == 0
    finally:
        sys.argv = old


def test_ops_refuse_cpu_tensors():
    from mdm_hip import _lib

    with pytest.raises(_lib.MdmHipError):
        ops.mx8_quant(torch.randn(4, 32))
    with pytest.raises(_lib.MdmHipError):
        ops.packed_weight_mx8(nn.Conv2d(32, 32, 1).weight, None)


# ---- attach / detach ----------------------------------------------------------------------------------------------------------
def _attn_layers(model):
    from mdm_hip.unet import SelfAttention

    return [(n, m) for n, m in model.named_modules() if isinstance(m, SelfAttention)]


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested", "mini_nested2"])
def test_attach_sets_handles_and_detach_clears_them(name):
    model, _, _ = PC.build_module(name)
    layers = _attn_layers(model)
    assert layers and all(m._fp8 is None for _, m in layers)
    sd_before = {k: v.clone() for k, v in model.state_dict().items()}
    epoch = ops.adapter_epoch()
    h = fp8.attach(model)
    assert ops.adapter_epoch() > epoch                                  # a GraphedSampler captures anew
    assert sorted(n for n, _, _ in h.layers) == sorted(n for n, _ in layers)
    if name != "mini_unet":
        assert any(n.startswith("inner_unet.") for n, _, _ in h.layers)    # inner nets included
    for _, m in layers:
        assert m._fp8 is not None and m._fp8.on("qkv") and m._fp8.on("proj_out") and m._fp8.on("ffn") == (m.ffn is not None)
        assert "_fp8" not in m._modules and "_fp8" not in m._parameters and "_fp8" not in m._buffers
    sd = model.state_dict()
    assert list(sd.keys()) == list(sd_before.keys()) and all(torch.equal(sd[k], v) for k, v in sd_before.items())
    assert all(p.requires_grad for p in model.parameters())            # nothing is frozen: training is simply not the fp8 path
    epoch = ops.adapter_epoch()
    h.detach()
    assert ops.adapter_epoch() > epoch and all(m._fp8 is None for _, m in layers)
    with pytest.raises(RuntimeError):
        h.detach()
    # a subset of targets
    h2 = fp8.attach(model, targets=("ffn",))
    assert all(m._fp8.on("ffn") and not m._fp8.on("qkv") for _, m in layers if m.ffn is not None)
    h2.detach()


def test_refusals():
    model, _, _ = PC.build_module("mini_unet")
    layers = _attn_layers(model)
    with pytest.raises(ValueError, match="targets"):
        fp8.attach(model, targets=("qkv", "kv_cond"))
    with pytest.raises(ValueError, match="targets"):
        fp8.attach(model, targets=())
    with pytest.raises(ValueError, match="no attention"):
        fp8.attach(SM.StubUNet())
    # 1. channel counts: a layer whose projection is not a multiple of 32 wide is named
    name, layer = layers[0]
    keep = layer.qkv
    layer.qkv = nn.Conv2d(layer.channels, 3 * layer.channels + 8, 1)
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + r"\.qkv"):
        fp8.attach(model)
    layer.qkv = keep
    assert all(m._fp8 is None for _, m in layers)                       # a refused attach leaves the model alone
    # 2. unmerged LoRA adapters
    ad = lora.attach(model, rank=4)
    with pytest.raises(RuntimeError, match=r"merge\(\) first"):
        fp8.attach(model)
    ad.detach()
    # 3. a second handle
    h = fp8.attach(model)
    with pytest.raises(RuntimeError, match="already"):
        fp8.attach(model)
    h.detach()


def test_lora_refuses_fp8_layers():
    """the other direction of refusal 2: adapters cannot appear, or come back out of the masters, under an fp8 handle"""
    model, _, _ = PC.build_module("mini_unet")
    h = fp8.attach(model)
    with pytest.raises(RuntimeError, match="fp8"):
        lora.attach(model, rank=4)
    assert all(m._lora is None for _, m in _attn_layers(model))
    ad = lora.attach(model, rank=4, targets=(), conv_targets=("conv1",))   # the ResNet convolutions are not fp8: allowed
    ad.detach()
    h.detach()
    ad = lora.attach(model, rank=4)
    ad.merged = True                                                    # as after merge() (the fold itself runs on the GPU)
    h = fp8.attach(model)
    with pytest.raises(RuntimeError, match="fp8"):
        ad.unmerge()
    h.detach()
