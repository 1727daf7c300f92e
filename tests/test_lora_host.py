"""CPU: the host side of ``mdm_hip.lora`` -- where adapters attach, their shapes and seeded values, the frozen base, the
untouched vision-model state dict, every refusal, the state-dict round trip, the exported symbols -- and the plain
trainer path clipping every parameter its optimizer holds."""
import ctypes
import types

import pytest
import torch
import torch.nn as nn

import lora_cases as LC
import parity_cases as PC
import stub_models as SM
from mdm_hip import lora


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested", "mini_nested2"])
def test_attach_parameters_freeze_and_detach(name):
    model, _, sd = PC.build_module(name)
    keys_before = list(model.state_dict().keys())
    flags_before = {k: p.requires_grad for k, p in model.named_parameters()}
    ad = lora.attach(model, rank=8, alpha=4, seed=3)
    assert isinstance(ad, nn.Module) and ad.scale == 0.5 and not ad.merged
    want = LC.expected_adapters(sd, LC.TARGETS, 8)
    got = {k: tuple(p.shape) for k, p in ad.named_parameters()}
    assert want and got == want
    if name != "mini_unet":
        assert any(k.startswith("inner_unet.") for k in got)          # inner nets included
    assert any(".kv_cond." in k for k in got) and any(".qkv." in k for k in got) and any(".proj_out." in k for k in got)
    for k, p in ad.named_parameters():
        assert p.dtype == torch.float32 and p.requires_grad
        if k.endswith("lora_B"):
            assert float(p.detach().abs().max()) == 0.0
    # A: seeded normal, sigma = 1 / sqrt(Cin), drawn in sorted layer-name order, targets in the order qkv, kv_cond, proj_out
    g = torch.Generator().manual_seed(3)
    layers = sorted({k.rsplit(".", 2)[0] for k in got})
    for layer in layers:
        for t in LC.TARGETS:
            key = "%s.%s.lora_A" % (layer, t)
            if key in got:
                cin = got[key][1]
                assert torch.equal(dict(ad.named_parameters())[key], torch.randn(8, cin, generator=g) / cin ** 0.5)
    # the base is frozen, the vision model's state dict has the reference's keys and nothing else
    assert all(not p.requires_grad for p in model.parameters())
    assert list(model.state_dict().keys()) == keys_before
    assert not any(isinstance(m, type(ad)) for m in model.modules())
    # the same seed gives the same draw; another seed another
    ad.detach()
    assert {k: p.requires_grad for k, p in model.named_parameters()} == flags_before
    ad2 = lora.attach(model, rank=8, alpha=4, seed=3)
    assert all(torch.equal(p, dict(ad.named_parameters())[k]) for k, p in ad2.named_parameters())
    ad2.detach()
    ad3 = lora.attach(model, rank=8, seed=4, targets=("qkv",), freeze_base=False)
    assert ad3.scale == 1.0 and all(".qkv." in k for k, _ in ad3.named_parameters())
    assert {k: p.requires_grad for k, p in model.named_parameters()} == flags_before
    assert not all(torch.equal(p, dict(ad.named_parameters())[k]) for k, p in ad3.named_parameters() if k.endswith("lora_A"))


def test_detach_restores_flags_as_found():
    model, _, _ = PC.build_module("mini_unet")
    first = next(model.parameters())
    first.requires_grad = False
    ad = lora.attach(model, rank=4)
    ad.detach()
    flags = [p.requires_grad for p in model.parameters()]
    assert flags[0] is False and all(flags[1:])
    with pytest.raises(RuntimeError):
        ad.detach()


def test_refusals():
    model, _, _ = PC.build_module("mini_unet")
    with pytest.raises(ValueError, match="qkv"):
        lora.attach(model, targets=("qkv", "conv1"))
    with pytest.raises(ValueError, match="FFN"):
        lora.attach(model, targets=("ffn",))
    for bad in (0, 3, 12, 128, 16.5):
        with pytest.raises(ValueError, match="rank"):
            lora.attach(model, rank=bad)
    assert all(p.requires_grad for p in model.parameters())     # a refused attach leaves the model alone
    ad = lora.attach(model, rank=16)
    with pytest.raises(RuntimeError, match="already"):
        lora.attach(model, rank=16)
    ad.detach()
    with pytest.raises(ValueError, match="no attention"):
        lora.attach(nn.Sequential(nn.Conv2d(8, 8, 1)))
    with pytest.raises(ValueError, match="no attention"):
        lora.attach(SM.StubUNet())


def test_state_dict_round_trip_and_rank_check():
    model, _, _ = PC.build_module("mini_nested")
    ad = lora.attach(model, rank=8, alpha=2, seed=5)
    LC.seeded_b(ad)
    sd = ad.state_dict()
    assert int(sd["rank"]) == 8 and float(sd["alpha"]) == 2.0
    assert all(k in ("rank", "alpha") or k.endswith(".lora_A") or k.endswith(".lora_B") for k in sd)
    sd = {k: v.clone() for k, v in sd.items()}
    ad.detach()
    fresh = lora.attach(model, rank=8, seed=99)
    assert fresh.scale == 1.0
    fresh.load_state_dict(sd)
    assert fresh.scale == 0.25
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k
    fresh.detach()
    other = lora.attach(model, rank=16)
    with pytest.raises(ValueError, match="rank"):
        other.load_state_dict(sd)


def test_ops_refuse_cpu_tensors():
    from mdm_hip import _lib, ops

    x, a = torch.randn(16, 64), torch.randn(4, 64)
    with pytest.raises(_lib.MdmHipError):
        ops.lora_down(x, a)
    with pytest.raises(_lib.MdmHipError):
        ops.lora(torch.randn(16, 8), x, a, torch.zeros(8, 4), 1.0)
    model, _, _ = PC.build_module("mini_unet")
    ad = lora.attach(model, rank=4)
    with pytest.raises(_lib.MdmHipError):
        ad.merge()            # merging runs the kernel on GPU tensors: no CPU fallback


def test_symbols_resolve_and_abi_stays_6():
    from mdm_hip import _lib

    L = _lib.lib()
    names = {p[0] for p in _lib.header_prototypes()}
    for n in ("mdm_lora_down", "mdm_lora_up_add", "mdm_lora_wgrad_plan", "mdm_lora_wgrad"):
        assert n in names and hasattr(L, n)
    assert L.mdm_abi_version() == _lib.ABI_VERSION == 6 and "lora.hip" in _lib.SOURCES
    # the plan is host-only: slabs over M, an fp32 [r, C] slab each; (5000, 768) spans several
    sp, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    assert L.mdm_lora_wgrad_plan(5000, 16, 768, 1, ctypes.byref(sp), ctypes.byref(ws)) == 0
    assert sp.value > 1 and ws.value == sp.value * 16 * 768 * 4
    assert L.mdm_lora_wgrad_plan(16, 4, 64, 0, ctypes.byref(sp), ctypes.byref(ws)) == 0 and sp.value == 1
    # invalid arguments are reported, not executed
    assert L.mdm_lora_wgrad_plan(16, 5, 64, 1, ctypes.byref(sp), ctypes.byref(ws)) < 0
    assert L.mdm_lora_wgrad_plan(16, 4, 60, 1, ctypes.byref(sp), ctypes.byref(ws)) < 0
    assert L.mdm_lora_down(None, None, None, 16, 64, 4, 1, None) < 0


# ---- trainer: the plain path clips every parameter the optimizer holds --------------------------------------------------
class _StubWithOutsideParameter(SM.StubUNet):
    """a denoiser whose output also depends on a parameter that is NOT registered in the model (as adapters are not)"""

    def __init__(self, outside):
        super().__init__()
        self._outside = [outside]

    def forward(self, x_t, times, lm_outputs, lm_mask, micros={}):
        return super().forward(x_t, times, lm_outputs, lm_mask, micros) + self._outside[0] * torch.roll(x_t, 2, dims=-2)


def _stub_pipe(outside):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM")
    return D.Diffusion(_StubWithOutsideParameter(outside), D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


def _stub_sample():
    g = torch.Generator().manual_seed(7)
    return {"images": torch.rand(3, 3, 16, 16, generator=g) * 2 - 1, "lm_outputs": torch.randn(3, 5, 8, generator=g),
            "lm_mask": torch.ones(3, 5)}


@pytest.mark.parametrize("holds", ["outside_only", "model_and_outside", "model_only"])
def test_plain_path_clips_the_union_of_model_and_optimizer_parameters(holds):
    from mdm_hip import trainer

    clip = 0.05
    outside = nn.Parameter(torch.tensor(0.3))
    pipe = _stub_pipe(outside)
    w = pipe.model.vision_model.w
    held = {"outside_only": [outside], "model_and_outside": [w, outside], "model_only": [w]}[holds]
    # raw gradients of the same step (same seed -> same timesteps and noise), clipped by torch over the union
    torch.manual_seed(11)
    pipe.train()
    losses = pipe.get_loss(_stub_sample())[0]
    losses.mean().backward()
    union = [w] + ([outside] if holds != "model_only" else [])
    raw = {id(p): p.grad.clone() for p in [w, outside]}
    assert float(raw[id(outside)].abs()) > 0 and float(raw[id(w)].abs()) > 0
    norm_ref = torch.nn.utils.clip_grad_norm_(union, clip)
    want = {id(p): p.grad.clone() for p in [w, outside]}
    assert float(norm_ref) > clip          # the clip acts
    for p in (w, outside):
        p.grad = None
    before = {id(p): p.detach().clone() for p in [w, outside]}
    opt = torch.optim.SGD(held, lr=1.0)
    if holds == "model_only":
        assert not isinstance(trainer._clip_parameters(pipe, opt), list)     # the unchanged path: the model's own iterator
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
    torch.manual_seed(11)
    trainer.train_batch(pipe, _stub_sample(), opt, sched, None, types.SimpleNamespace(fp16=False, gradient_clip_norm=clip))
    assert getattr(opt, "_mdm_fused", None) is False
    assert abs(float(opt._mdm_grad_norm) - float(norm_ref)) <= 1e-6 * float(norm_ref)
    for p in held:      # SGD, lr 1: the step is the clipped gradient
        assert torch.allclose(before[id(p)] - p.detach(), want[id(p)], rtol=1e-5, atol=1e-9), holds
    for p in [w, outside]:
        if all(p is not h for h in held):
            assert torch.equal(p.detach(), before[id(p)])
