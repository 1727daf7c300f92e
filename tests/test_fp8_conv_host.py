"""CPU: the restatement of the MXFP8 3x3 convolution (tests/fp8_conv_cases.py) against ``F.conv2d``, the exactness of its
integer-data cases, the exported symbols and the static scans of the file that holds the kernel, and the host logic of
``mdm_hip.fp8.attach(conv_targets=...)`` (handles, ``min_channels``, refusals) on CPU-built mini models."""
import os
import shutil

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fp8_cases as FC
import fp8_conv_cases as CC
import parity_cases as PC
import stub_models as SM
from mdm_hip import fp8, lora, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,cin,cout", CC.CONV_SHAPES)
def test_restatement_is_conv2d(N, H, W, cin, cout):
    """nine shifted-row GEMMs with (y, x) validity == conv2d(padding=1) in fp64: on the integer operands bit for bit (every
    partial sum is exact), on random quantised operands to fp64 rounding"""
    qa, sa, qw, sw = CC.exact_operands(N, H, W, cin, cout)
    x, w = CC.as_conv2d_operands(qa, sa, qw, sw, (N, H, W), cin)
    ref = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1)
    got = CC.conv_ref(qa, sa, qw, sw, (N, H, W))
    assert got.shape == (N, H, W, cout) and torch.equal(got, ref)
    assert torch.equal(CC.conv_ref(*CC.with_zero_row(qa, sa), qw, sw, (N, H, W)), got)    # a zero row behind changes nothing
    g = torch.Generator().manual_seed(N + H + W + cin)
    qa, sa = FC.quant_ref(torch.randn(N * H * W, cin, generator=g))
    qw, sw = CC.quant_weight_3x3(torch.randn(cout, cin, 3, 3, generator=g))
    x, w = CC.as_conv2d_operands(qa, sa, qw, sw, (N, H, W), cin)
    ref = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1)
    got = CC.conv_ref(qa, sa, qw, sw, (N, H, W))
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_weight_rows_are_tap_major_within_an_output_channel():
    w = torch.arange(2 * 32 * 9, dtype=torch.float32).reshape(2, 32, 3, 3)
    q, s = CC.quant_weight_3x3(w)
    back = FC.dequant_ref(q, s)[:, :32]
    assert q.shape == (18, 128) and s.shape == (18, 4)
    for o, ky, kx in ((0, 0, 0), (0, 2, 1), (1, 1, 2)):
        assert torch.equal(back[o * 9 + ky * 3 + kx], FC.dequant_ref(*FC.quant_ref(w[o, :, ky, kx].reshape(1, 32)))[0, :32])


def test_exact_cases_are_exact_in_fp32():
    """every partial sum of every output is an integer multiple of 2^-6 below 2^18: exact in fp32 in any summation order, so
    the kernel's output must be THE bf16 rounding of the fp64 value"""
    maxima = []
    for N, H, W, cin, cout in CC.CONV_SHAPES:
        qa, sa, qw, sw = CC.exact_operands(N, H, W, cin, cout)
        x, w = CC.as_conv2d_operands(qa, sa, qw, sw, (N, H, W), cin)
        top = float(F.conv2d(x.abs(), w.abs(), padding=1).max())
        maxima.append(top)
        assert top < 2.0 ** 18
        assert torch.equal((x * 8).round(), x * 8) and torch.equal((w * 8).round(), w * 8)     # products: multiples of 2^-6
        y64 = F.conv2d(x, w, padding=1)
        y32 = F.conv2d(x.float(), w.float(), padding=1)
        assert torch.equal(y32.double(), y64) and torch.equal((y64 * 64).round(), y64 * 64)
        # a dropped output must not hide behind a zero: none is zero, bar ONE element of 256 in the H = 1 case
        assert int((y64 == 0).sum()) == (1 if (N, H, W) == (2, 1, 4) else 0)
        assert len(set(sa.flatten().tolist())) >= 7 and len(set(sw.flatten().tolist())) >= 7
    print("[mx8 conv exact cases] max of conv2d(|x|, |w|): %s" % maxima)
    assert [round(v) for v in maxima] == [8256, 3812, 26005, 25762]


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_symbols_resolve_and_abi_stays_6():
    from mdm_hip import _lib

    L = _lib.lib()
    names = {p[0] for p in _lib.header_prototypes()}
    for n in ("mdm_mx8_quant_zrow", "mdm_mx8_conv3x3"):
        assert n in names and hasattr(L, n)
    assert L.mdm_abi_version() == _lib.ABI_VERSION == 6
    # invalid arguments are reported, not executed
    assert L.mdm_mx8_quant_zrow(None, 1, 4, 32, 128, None, None, None) < 0
    one = ctypes_buffer()
    assert L.mdm_mx8_conv3x3(None, None, None, None, None, None, None, 1, 4, 4, 32, 32, None) < 0
    assert L.mdm_mx8_conv3x3(one, one, one, one, None, None, one, 1, 4, 4, 48, 32, None) < 0     # Cin % 32
    assert L.mdm_mx8_conv3x3(one, one, one, one, None, None, one, 1, 4, 4, 32, 40, None) < 0     # Cout % 32
    assert L.mdm_mx8_conv3x3(one, one, one, one, None, None, one, 1, 0, 4, 32, 32, None) < 0     # H < 1
    assert L.mdm_mx8_conv3x3(one, one, one, one, None, None, one, 65536, 256, 128, 32, 32, None) < 0   # N H W past int


def ctypes_buffer():
    """a non-null pointer for the argument checks (never dereferenced: every call above is refused before a launch)"""
    import ctypes

    buf = ctypes.create_string_buffer(16)
    ctypes_buffer.keep = buf
    return ctypes.addressof(buf)


def test_the_conv_kernel_passes_the_static_scans():
    """tools/mfma_hazard_scan.py over csrc/fp8.hip, which holds the 3x3 form: no early read of an MFMA result, no spilled
    registers past the cap, no vector load between the wide stores of the epilogue -- and the 3x3
    instantiation is among the kernels the scan saw"""
    import importlib.util
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("mfma_hazard_scan", os.path.join(ROOT, "tools", "mfma_hazard_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = []
    real = mod.loads_between_wide_stores

    def spy(path):
        seen.append(open(path).read())
        return real(path)

    mod.loads_between_wide_stores = spy
    old = sys.argv
    sys.argv = ["mfma_hazard_scan.py", "fp8.hip"]
    try:
        assert mod.main() == 0
    finally:
        sys.argv = old
    assert seen and "mx8_gemm_kernelILb0ELb1EE" in seen[0]                  # mx8_gemm_kernel<EMIT = false, CONV = true>


def test_ops_refuse_cpu_tensors():
    from mdm_hip import _lib

    with pytest.raises(_lib.MdmHipError):
        ops.mx8_quant_zrow(torch.randn(4, 32).to(torch.bfloat16))
    with pytest.raises(_lib.MdmHipError):
        ops.packed_weight_mx8_3x3(nn.Conv2d(32, 32, 3).weight, None)
    qa, sa, qw, sw = CC.exact_operands(1, 2, 2, 32, 32)
    qa, sa = CC.with_zero_row(qa, sa)
    with pytest.raises(_lib.MdmHipError):
        ops.mx8_conv3x3(ops.Mx8(qa, sa, 32), ops.Mx8(qw, sw, 32), (1, 2, 2))


# ---- attach / detach ----------------------------------------------------------------------------------------------------------
def _resnets(model):
    from mdm_hip.unet import ResNet

    return [(n, m) for n, m in model.named_modules() if isinstance(m, ResNet)]


def _attn_layers(model):
    from mdm_hip.unet import SelfAttention

    return [(n, m) for n, m in model.named_modules() if isinstance(m, SelfAttention)]


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested", "mini_nested2"])
def test_conv_targets_set_handles_and_detach_clears_them(name):
    model, _, _ = PC.build_module(name)
    blocks = _resnets(model)
    assert blocks and all(m._fp8 is None for _, m in blocks)
    sd_before = {k: v.clone() for k, v in model.state_dict().items()}
    # the defaults do what they did: attention layers only
    if _attn_layers(model):
        h = fp8.attach(model)
        assert h.convs == [] and all(m._fp8 is None for _, m in blocks)
        h.detach()
    targets = fp8.TARGETS if _attn_layers(model) else ()
    epoch = ops.adapter_epoch()
    h = fp8.attach(model, targets=targets, conv_targets=fp8.CONV_TARGETS)
    assert ops.adapter_epoch() > epoch
    assert sorted(n for n, _, _ in h.convs) == sorted(n for n, _ in blocks)
    assert len(h.layers) == len(_attn_layers(model)) and all(len(e) == 3 for e in h.layers)
    if name != "mini_unet":
        assert any(n.startswith("inner_unet.") for n, _, _ in h.convs)     # inner nets included
    for _, m in blocks:
        assert m._fp8 is not None and m._fp8.on("conv1") and m._fp8.on("conv2") and m._fp8.on("conv3") == hasattr(m, "conv3")
        assert "_fp8" not in m._modules and "_fp8" not in m._parameters and "_fp8" not in m._buffers
    assert any(hasattr(m, "conv3") for _, m in blocks) and not all(hasattr(m, "conv3") for _, m in blocks)
    sd = model.state_dict()
    assert list(sd.keys()) == list(sd_before.keys()) and all(torch.equal(sd[k], v) for k, v in sd_before.items())
    assert all(p.requires_grad for p in model.parameters())
    epoch = ops.adapter_epoch()
    h.detach()
    assert ops.adapter_epoch() > epoch and all(m._fp8 is None for _, m in blocks + _attn_layers(model))
    with pytest.raises(RuntimeError):
        h.detach()
    # a subset of conv targets, no attention targets
    h2 = fp8.attach(model, targets=(), conv_targets="conv2")
    assert h2.layers == [] and all(m._fp8.on("conv2") and not m._fp8.on("conv1") and not m._fp8.on("conv3") for _, m in blocks)
    assert all(m._fp8 is None for _, m in _attn_layers(model))
    h2.detach()


def test_min_channels_leaves_narrow_resnets_on_bf16():
    model, _, _ = PC.build_module("mini_unet")
    blocks = _resnets(model)
    width = {n: min(m.conv1.weight.shape[0], m.conv1.weight.shape[1]) for n, m in blocks}
    assert min(width.values()) == 32 and max(width.values()) >= 64
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS, min_channels=64)
    assert sorted(n for n, _, _ in h.convs) == sorted(n for n, w in width.items() if w >= 64)
    assert all((m._fp8 is None) == (width[n] < 64) for n, m in blocks)
    h.detach()
    with pytest.raises(ValueError, match="min_channels"):
        fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS, min_channels=4096)
    assert all(m._fp8 is None for _, m in blocks)


def test_conv_refusals_leave_the_model_alone():
    model, _, _ = PC.build_module("mini_unet")
    blocks, layers = _resnets(model), _attn_layers(model)

    def untouched():
        return all(m._fp8 is None for _, m in blocks + layers)

    with pytest.raises(ValueError, match="conv targets"):
        fp8.attach(model, conv_targets=("conv1", "conv4"))
    with pytest.raises(ValueError, match="conv_targets"):
        fp8.attach(model, targets=("conv1",))                           # a conv target among the attention targets
    with pytest.raises(ValueError, match="targets"):
        fp8.attach(model, targets=(), conv_targets=())
    with pytest.raises(ValueError, match="no ResNet"):
        fp8.attach(SM.StubUNet(), targets=(), conv_targets=fp8.CONV_TARGETS)
    assert untouched()
    # 1. channel counts: a targeted ResNet whose convolution is not a multiple of 32 wide is named
    name, block = blocks[0]
    keep = block.conv2
    block.conv2 = nn.Conv2d(keep.weight.shape[1], keep.weight.shape[0] + 8, 3, padding=1)
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + r"\.conv2"):
        fp8.attach(model, conv_targets=fp8.CONV_TARGETS)
    block.conv2 = keep
    assert untouched()
    # 2. unmerged LoRA conv adapters
    ad = lora.attach(model, rank=4, targets=(), conv_targets=("conv1",))
    with pytest.raises(RuntimeError, match=r"merge\(\) first"):
        fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    assert untouched()
    h = fp8.attach(model)                                               # attention targets only: the conv adapters do not matter
    h.detach()
    ad.detach()
    # 3. a second handle
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    with pytest.raises(RuntimeError, match="already"):
        fp8.attach(model)
    with pytest.raises(RuntimeError, match="already"):
        fp8.attach(model, targets=(), conv_targets=("conv1",))
    h.detach()
    assert untouched()


def test_attach_without_attention_layers_needs_no_attention_targets():
    """a net without attention (the outer nets of a nested model are such nets) takes conv targets alone"""
    from mdm_hip.unet import ResNet

    class OnlyResNets(nn.Module):
        def __init__(self):
            super().__init__()
            from mdm_hip.unet import ResNetConfig
            self.a = ResNet(16, ResNetConfig(num_channels=32, output_channels=64, num_groups_norm=32))

    net = OnlyResNets()
    with pytest.raises(ValueError, match="no attention"):
        fp8.attach(net, conv_targets=fp8.CONV_TARGETS)                  # the default attention targets were asked for
    assert net.a._fp8 is None
    h = fp8.attach(net, targets=(), conv_targets=fp8.CONV_TARGETS)
    assert h.layers == [] and [n for n, _, _ in h.convs] == ["a"] and net.a._fp8.on("conv3")
    h.detach()


def test_lora_refuses_fp8_resnets():
    """the other direction: conv adapters cannot appear, or come back out of the masters, under an fp8 handle on the ResNets"""
    model, _, _ = PC.build_module("mini_unet")
    blocks = _resnets(model)
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    with pytest.raises(RuntimeError, match="fp8"):
        lora.attach(model, rank=4, targets=(), conv_targets=("conv1",))
    assert all(m._lora is None for _, m in blocks)
    ad = lora.attach(model, rank=4)                                     # the attention layers are not fp8: allowed
    ad.detach()
    h.detach()
    ad = lora.attach(model, rank=4, targets=(), conv_targets=("conv1", "conv3"))
    ad.merged = True                                                    # as after merge() (the fold itself runs on the GPU)
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    with pytest.raises(RuntimeError, match="fp8"):
        ad.unmerge()
    h.detach()
