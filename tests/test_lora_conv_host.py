"""CPU: the host side of the conv adapters of ``mdm_hip.lora`` -- names, shapes, seeded values and their draw order, the
frozen base, the untouched vision-model state dict, attention adapters that do not depend on ``conv_targets``, a conv-only
attach on a net without attention, every refusal, the state-dict round trip, the four new symbols and the plan's arithmetic."""
import ctypes

import pytest
import torch
import torch.nn as nn

import lora_cases as LC
import lora_conv_cases as CC
import parity_cases as PC
import stub_models as SM
from mdm_hip import lora

NAMES = ["mini_unet", "mini_nested", "mini_nested2"]


def _params(ad):
    return dict(ad.named_parameters())


@pytest.mark.parametrize("name", NAMES)
def test_attach_names_shapes_init_freeze_and_detach(name):
    model, _, sd = PC.build_module(name)
    keys_before = list(model.state_dict().keys())
    flags_before = {k: p.requires_grad for k, p in model.named_parameters()}
    ad = lora.attach(model, rank=8, alpha=4, seed=3, conv_targets=lora.CONV_TARGETS, conv_rank=4, conv_alpha=2)
    assert lora.CONV_TARGETS == ("conv1", "conv2", "conv3")
    assert ad.scale == 0.5 and ad.conv_scale == 0.5 and not ad.merged
    want_attn = LC.expected_adapters(sd, LC.TARGETS, 8)
    want_conv = CC.expected_conv_adapters(model, CC.CONV_TARGETS, 4)
    got = {k: tuple(p.shape) for k, p in ad.named_parameters()}
    assert want_attn and want_conv and got == {**want_attn, **want_conv}
    assert any(len(s) == 4 for s in want_conv.values()) and any(k.endswith("conv3.lora_A") and len(s) == 2 for k, s in want_conv.items())
    assert any(".conv3." not in k and k.replace("conv1", "conv3") not in got for k in want_conv if ".conv1." in k)   # conv3 skipped where absent
    if name != "mini_unet":
        assert any(k.startswith("inner_unet.") for k in want_conv) and any(not k.startswith("inner_unet.") for k in want_conv)
    for k, p in ad.named_parameters():
        assert p.dtype == torch.float32 and p.requires_grad and p.device.type == "cpu"
        if k.endswith("lora_B"):
            assert float(p.detach().abs().max()) == 0.0
    # the draw: every attention adapter first (sorted layer names; qkv, kv_cond, proj_out), then the ResNets in sorted
    # name order, conv1, conv2, conv3, A ~ N(0, 1 / fan_in) with fan_in = 9 Cin (3x3) or Cin (conv3)
    g = torch.Generator().manual_seed(3)
    P = _params(ad)
    for layer in sorted({k.rsplit(".", 2)[0] for k in want_attn}):
        for t in LC.TARGETS:
            key = "%s.%s.lora_A" % (layer, t)
            if key in got:
                cin = got[key][1]
                assert torch.equal(P[key], torch.randn(8, cin, generator=g) / cin ** 0.5), key
    for layer in sorted({k.rsplit(".", 2)[0] for k in want_conv}):
        for t in CC.CONV_TARGETS:
            key = "%s.%s.lora_A" % (layer, t)
            if key in got:
                shape = got[key]
                fan_in = shape[1] * (9 if len(shape) == 4 else 1)
                assert torch.equal(P[key], torch.randn(shape, generator=g) / fan_in ** 0.5), key
    assert all(not p.requires_grad for p in model.parameters())
    assert list(model.state_dict().keys()) == keys_before
    assert not any(isinstance(m, type(ad)) for m in model.modules())
    sd_ad = ad.state_dict()
    assert int(sd_ad["conv_rank"]) == 4 and float(sd_ad["conv_alpha"]) == 2.0 and int(sd_ad["rank"]) == 8
    ad.detach()
    assert {k: p.requires_grad for k, p in model.named_parameters()} == flags_before
    assert all(getattr(m, "_lora", None) is None for m in model.modules())
    with pytest.raises(RuntimeError):
        ad.detach()
    # defaults: conv_rank = rank, conv_alpha = conv_rank
    ad2 = lora.attach(model, rank=8, alpha=4, seed=3, conv_targets=("conv2",))
    assert ad2.conv_scale == 1.0 and ad2.scale == 0.5
    assert all(p.shape[0] == 8 for k, p in ad2.named_parameters() if k.endswith("conv2.lora_A"))
    assert not any(".conv1." in k or ".conv3." in k for k, _ in ad2.named_parameters())


@pytest.mark.parametrize("name", NAMES)
def test_attention_adapters_do_not_depend_on_conv_targets(name):
    model, _, _ = PC.build_module(name)
    plain = lora.attach(model, rank=8, alpha=4, seed=3)
    plain_sd = {k: v.clone() for k, v in plain.state_dict().items()}
    assert not any(k.startswith("conv_") for k in plain_sd)                  # an attention-only state dict keeps today's keys
    plain.detach()
    both = lora.attach(model, rank=8, alpha=4, seed=3, conv_targets=lora.CONV_TARGETS, conv_rank=4)
    both_sd = both.state_dict()
    assert set(plain_sd) < set(both_sd)
    assert all(torch.equal(v, both_sd[k]) for k, v in plain_sd.items())


def test_conv_only_attach_on_a_model_without_attention():
    from mdm_hip.unet import ResNet, ResNetConfig

    class ConvOnly(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = ResNet(16, ResNetConfig(num_channels=8, output_channels=16, num_groups_norm=8))
            self.b = ResNet(16, ResNetConfig(num_channels=16, output_channels=16, num_groups_norm=8))

    net = ConvOnly()
    ad = lora.attach(net, targets=(), conv_targets=lora.CONV_TARGETS, conv_rank=4, seed=1)
    got = {k: tuple(p.shape) for k, p in ad.named_parameters()}
    assert got == {"a.conv1.lora_A": (4, 8, 3, 3), "a.conv1.lora_B": (16, 4), "a.conv2.lora_A": (4, 16, 3, 3), "a.conv2.lora_B": (16, 4),
                   "a.conv3.lora_A": (4, 8), "a.conv3.lora_B": (16, 4), "b.conv1.lora_A": (4, 16, 3, 3), "b.conv1.lora_B": (16, 4),
                   "b.conv2.lora_A": (4, 16, 3, 3), "b.conv2.lora_B": (16, 4)}
    assert net.a._lora is not None and net.b._lora is not None and all(not p.requires_grad for p in net.parameters())
    assert ad.targets == () and ad.conv_targets == lora.CONV_TARGETS
    ad.detach()
    assert net.a._lora is None and net.b._lora is None and all(p.requires_grad for p in net.parameters())
    # the outer nets of a nested model are such nets: a conv-only attach reaches them
    model, _, _ = PC.build_module("mini_nested")
    ad = lora.attach(model, targets=(), conv_targets=("conv1", "conv2"), conv_rank=4)
    names = [k for k, _ in ad.named_parameters()]
    assert any(not k.startswith("inner_unet.") for k in names) and not any(t in k for k in names for t in LC.TARGETS)


def test_refusals():
    model, _, _ = PC.build_module("mini_unet")
    with pytest.raises(ValueError, match="conv targets"):
        lora.attach(model, conv_targets=("conv1", "resample"))
    with pytest.raises(ValueError, match="conv targets"):
        lora.attach(model, conv_targets=("qkv",))
    for bad in (0, 3, 12, 128, 4.5, True):
        with pytest.raises(ValueError, match="conv rank"):
            lora.attach(model, conv_targets=("conv1",), conv_rank=bad)
    with pytest.raises(ValueError, match="non-empty"):
        lora.attach(model, targets=(), conv_targets=())
    with pytest.raises(ValueError, match="no attention"):
        lora.attach(SM.StubUNet(), conv_targets=("conv1",))
    with pytest.raises(ValueError, match="no ResNet"):
        lora.attach(SM.StubUNet(), targets=(), conv_targets=("conv1",))
    assert all(p.requires_grad for p in model.parameters()) and all(getattr(m, "_lora", None) is None for m in model.modules())
    # channels that are no multiple of 8: refused, and nothing stays attached
    from mdm_hip.unet import ResNet, ResNetConfig

    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = ResNet(16, ResNetConfig(num_channels=8, output_channels=8, num_groups_norm=4))
            self.b = ResNet(16, ResNetConfig(num_channels=8, output_channels=12, num_groups_norm=4))

    odd = Odd()
    with pytest.raises(ValueError, match="multiples of 8"):
        lora.attach(odd, targets=(), conv_targets=("conv1",))
    assert odd.a._lora is None and odd.b._lora is None and all(p.requires_grad for p in odd.parameters())
    ad = lora.attach(model, rank=16, conv_targets=("conv1",))
    with pytest.raises(RuntimeError, match="already"):
        lora.attach(model, targets=(), conv_targets=("conv2",))
    ad.detach()


def test_state_dict_round_trip_and_conv_rank_check():
    model, _, _ = PC.build_module("mini_nested")
    ad = lora.attach(model, rank=8, alpha=2, seed=5, conv_targets=lora.CONV_TARGETS, conv_rank=4, conv_alpha=1)
    LC.seeded_b(ad)
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    assert all(k in ("rank", "alpha", "conv_rank", "conv_alpha") or k.endswith(".lora_A") or k.endswith(".lora_B") for k in sd)
    ad.detach()
    fresh = lora.attach(model, rank=8, seed=99, conv_targets=lora.CONV_TARGETS, conv_rank=4)
    assert fresh.scale == 1.0 and fresh.conv_scale == 1.0
    fresh.load_state_dict(sd)
    assert fresh.scale == 0.25 and fresh.conv_scale == 0.25
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k
    fresh.detach()
    other = lora.attach(model, rank=8, conv_targets=lora.CONV_TARGETS, conv_rank=8)
    with pytest.raises(ValueError, match="conv rank"):
        other.load_state_dict(sd)


def test_symbols_resolve_plan_arithmetic_and_invalid_arguments():
    from mdm_hip import _lib

    L = _lib.lib()
    names = {p[0] for p in _lib.header_prototypes()}
    for n in ("mdm_lora_down_conv3x3", "mdm_lora_up_add_conv3x3", "mdm_lora_wgrad_conv3x3_plan", "mdm_lora_wgrad_conv3x3"):
        assert n in names and hasattr(L, n)
    assert L.mdm_abi_version() == _lib.ABI_VERSION == 6

    def plan(N, H, W, r, C, dt):
        sp, ws = ctypes.c_int(0), ctypes.c_size_t(0)
        rc = L.mdm_lora_wgrad_conv3x3_plan(N, H, W, r, C, dt, ctypes.byref(sp), ctypes.byref(ws))
        return rc, sp.value, ws.value

    def want(M, C, dt):
        """slabs of >= 128 rows, doubled until 9 waves (one per tap) x slabs x column groups <= 4096 and <= 256 slabs"""
        groups = -(-C // (16 * (4 if dt == 0 else 8)))
        rps = 128
        while -(-M // rps) * groups * 9 > 4096 or -(-M // rps) > 256:
            rps *= 2
        return -(-M // rps)

    for (N, H, W, r, C, dt) in [(5, 32, 32, 16, 64, 1), (5, 32, 32, 16, 64, 0), (1, 4, 4, 4, 8, 1), (64, 64, 64, 64, 768, 1),
                                (16, 256, 256, 4, 32, 1), (2, 5, 7, 8, 40, 0)]:
        rc, sp, ws = plan(N, H, W, r, C, dt)
        assert rc == 0 and sp == want(N * H * W, C, dt) and ws == sp * r * 9 * C * 4, (N, H, W, r, C, dt, sp, ws)
    assert plan(5, 32, 32, 16, 64, 1)[1] > 1 and plan(1, 4, 4, 4, 8, 1)[1] == 1
    # invalid arguments are reported, not executed
    assert plan(1, 4, 4, 5, 8, 1)[0] < 0 and plan(1, 4, 4, 4, 60, 1)[0] < 0 and plan(0, 4, 4, 4, 8, 1)[0] < 0
    assert plan(1, 4, 4, 128, 8, 1)[0] < 0 and plan(1, 4, 4, 4, 8, 2)[0] < 0 and plan(1 << 12, 1 << 12, 1 << 12, 4, 8, 1)[0] < 0
    assert L.mdm_lora_down_conv3x3(None, None, None, 1, 4, 4, 8, 4, 1, None) < 0
    assert L.mdm_lora_up_add_conv3x3(None, None, None, 1, 4, 4, 8, 4, 1.0, 1, 1, None) < 0
    assert L.mdm_lora_wgrad_conv3x3(None, None, None, None, 1, 4, 4, 4, 8, 1.0, 0, 1, None) < 0
    one = ctypes.c_void_p(1)    # non-null pointers: the geometry checks refuse before anything is launched
    assert L.mdm_lora_down_conv3x3(one, one, one, 1, 4, 4, 12, 4, 1, None) < 0
    assert L.mdm_lora_down_conv3x3(one, one, one, 1, 0, 4, 8, 4, 1, None) < 0
    assert L.mdm_lora_up_add_conv3x3(one, one, one, 1, 4, 4, 8, 6, 1.0, 1, 1, None) < 0
    assert L.mdm_lora_wgrad_conv3x3(one, one, one, one, 1, 4, 4, 4, 8, 1.0, 0, 7, None) < 0


def test_ops_refuse_cpu_tensors():
    from mdm_hip import _lib, ops

    x, a, t = torch.randn(1, 4, 4, 8), torch.randn(4, 9, 8), torch.randn(1, 4, 4, 4)
    with pytest.raises(_lib.MdmHipError):
        ops.lora_down_conv3x3(x, a)
    with pytest.raises(_lib.MdmHipError):
        ops.lora_up_add_conv3x3(x, t, torch.randn(8, 9, 4), 1.0)
    with pytest.raises(_lib.MdmHipError):
        ops.lora_wgrad_conv3x3(t, x, 1.0)
    with pytest.raises(_lib.MdmHipError):
        ops.lora_conv(torch.randn(1, 4, 4, 16), x, torch.randn(4, 8, 3, 3), torch.zeros(16, 4), 1.0)
    model, _, _ = PC.build_module("mini_nested")
    ad = lora.attach(model, targets=(), conv_targets=lora.CONV_TARGETS, conv_rank=4)
    with pytest.raises(_lib.MdmHipError):
        ad.merge()            # merging runs the kernel on GPU tensors: no CPU fallback
