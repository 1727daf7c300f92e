"""GPU: whole-model parity of the HIP path (called through the C ABI) against
  * the CPU oracle run live on the same seeded weights/inputs (all outputs, all parameter grads)
  * the golden vectors produced by the real reference (tests/golden/*.pt)

Tolerances (rel-L2): fp32 mode outputs 1e-4, gradients 1e-3 (SURVEY.md section 8d parity gates;
oracle fp32-vs-fp64 noise is ~1e-6).  bf16 mode: every output and the aggregate parameter gradient must be
at least as close to the fp32 reference as the REFERENCE's own bf16-autocast run of the same case
(tests/golden/reference_bf16_error.pt, measured by oracle/make_golden.py on the real reference; 1.30e-2 for
the UNet-64 forward, the figure SURVEY.md section 8c quotes).  Measured values are printed (pytest -s).
"""
import os

import pytest
import torch

import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REF_BF16 = torch.load(os.path.join(GOLD, "reference_bf16_error.pt"))


def hip_run(name, dtype, with_grad=True):
    model, _, _ = PC.build_module(name)
    model = model.to("cuda:0")
    inp = PC.inputs(name)
    x = [t.cuda() for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].cuda()
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else torch.autocast("cuda", enabled=False)
    micros = {k: v.cuda() for k, v in inp["micros"].items()}
    with ctx:
        outs = model(x, inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), micros)
    grads = None
    if with_grad:
        PC.loss_of(outs, inp["gys"]).backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        assert all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
    return [o.detach().float().cpu() for o in PC.as_list(outs)], grads


@pytest.mark.parametrize("name", PC.ALL_CASES)
def test_fp32_matches_oracle_and_golden(name):
    """incl. (round 3) explicit micro-conditioning on both sides of the clamp (models/unet.py:920-933) and
    mixed-resolution batches bh < bl (models/nested_unet.py:186-212), two and three nesting levels"""
    outs, grads = hip_run(name, torch.float32)
    o_ref, g_ref = PC.oracle_run(name)
    gold = torch.load(os.path.join(GOLD, name + ".pt"), weights_only=False)
    for a, b, c in zip(outs, o_ref, gold["outputs"]):
        assert O.rel_l2(a, b) < 1e-4
        assert O.rel_l2(a, c) < 1e-4
    errs, floor = PC.grad_errors(grads, g_ref)
    worst = max((e, k) for k, e in errs.items())
    assert worst[0] < 1e-3, worst
    for k, n in gold["grad_norm"].items():
        assert abs(float(grads[k].double().norm()) - n) <= 1e-3 * max(n, floor), k


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested", "mini_nested2"])
def test_bf16_close_to_oracle(name):
    """bf16 mode vs the fp32 oracle: measured errors are printed; gate = the reference's own bf16-autocast error on the
    same case, per output and for the aggregate parameter gradient"""
    outs, grads = hip_run(name, torch.bfloat16)
    o_ref, g_ref = PC.oracle_run(name)
    errs = [O.rel_l2(a, b) for a, b in zip(outs, o_ref)]
    # aggregate gradient error over all parameters (individual tiny tensors are noisier)
    num = sum(float((grads[k].double().cpu() - g_ref[k].double()).pow(2).sum()) for k in g_ref)
    den = sum(float(g_ref[k].double().pow(2).sum()) for k in g_ref)
    agg = (num / den) ** 0.5
    bar = REF_BF16[name]
    print("[bf16 %s] forward rel-L2 %s (reference's own: %s), aggregate gradient rel-L2 %.3e (reference's own: %.3e)" % (
        name, ["%.3e" % e for e in errs], ["%.3e" % e for e in bar["fwd"]], agg, bar["grad_agg"]))
    assert all(e <= b for e, b in zip(errs, bar["fwd"])) and agg <= bar["grad_agg"]


def test_lm_head_bf16():
    """num_lm_head_layers > 0 under bf16 autocast (the fp32 run is held to the real reference's golden by
    test_fp32_matches_oracle_and_golden[mini_unet_lmhead*]): same order of error as the other bf16 cases"""
    outs, grads = hip_run("mini_unet_lmhead", torch.bfloat16)
    o_ref, g_ref = PC.oracle_run("mini_unet_lmhead")
    assert O.rel_l2(outs[0], o_ref[0]) < 1.5 * REF_BF16["mini_unet_masked"]["fwd"][0]
    head = [k for k in g_ref if k.startswith("lm_head.")]
    assert head and all(torch.isfinite(grads[k]).all() for k in head)
    num = sum(float((grads[k].double().cpu() - g_ref[k].double()).pow(2).sum()) for k in head)
    den = sum(float(g_ref[k].double().pow(2).sum()) for k in head)
    assert (num / den) ** 0.5 < 5e-2


def test_forward_is_deterministic():
    a, _ = hip_run("mini_unet", torch.float32, with_grad=False)
    b, _ = hip_run("mini_unet", torch.float32, with_grad=False)
    assert torch.equal(a[0], b[0])


def test_no_grad_inference_matches_training_forward():
    model, _, _ = PC.build_module("mini_unet")
    model = model.to("cuda:0").eval()
    inp = PC.inputs("mini_unet")
    with torch.no_grad():
        y = model(inp["x"].cuda(), inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda())
    ref, _ = hip_run("mini_unet", torch.float32, with_grad=False)
    assert torch.equal(y.float().cpu(), ref[0])


def _pipeline(name, net, threshold="CLIP"):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                              use_double_loss=True, no_use_residual=True))
    return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_four_step_sampling_and_loss_match_reference_pipeline(name):
    """Diffusion.sample() (4 DDIM steps) and get_loss() through the HIP denoiser vs the golden images / losses the
    real reference pipeline produced on CPU with the same seed (tests/golden/pipeline.pt).  Gate: 1e-3 rel-L2
    (BASELINE.json north_star: "sampled images within 1e-3 rel-L2 of reference")."""
    gold = torch.load(os.path.join(GOLD, "pipeline.pt"), weights_only=False)[name]
    model, _, _ = PC.build_module(name)
    pipe = _pipeline(name, model).to(torch.device("cuda:0"))
    inp = PC.inputs(name)
    side = 32 if name == "mini_nested" else 16
    smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda()}
    torch.manual_seed(23)
    with torch.no_grad():
        if name == "mini_nested":
            # the reference draws the low-resolution start noise with .normal_() on the sampling device
            # (samplers.py:669-676); replay its CPU draws and hand the pyramid to the sampler directly
            pipe.eval()
            hi = torch.randn(2, 3, side, side)
            lo = torch.randn(2, 3, side // 2, side // 2)
            img = pipe.sampler.sample(pipe.get_model(), [hi.cuda(), lo.cuda()], smp["lm_outputs"], smp["lm_mask"], {},
                                      resample_steps=True, num_inference_steps=4, ddim_eta=0)
        else:
            img = pipe.sample(2, smp, side, torch.device("cuda:0"), resample_steps=True, num_inference_steps=4, ddim_eta=0)
    assert O.rel_l2(img.cpu(), gold["sample"]) < 1e-3
    # train-step loss: replay, from the CPU generator, exactly the draws the reference made on CPU
    # (randint for the timesteps, randn_like for eps, then one normal_() per lower resolution)
    g = torch.Generator().manual_seed(29)
    smp["images"] = (torch.rand(2, 3, side, side, generator=g) * 2 - 1).cuda()
    torch.manual_seed(31)
    time = torch.randint(0, 1000, (2,))
    draws = [torch.randn(2, 3, side, side)] + ([torch.randn(2, 3, side // 2, side // 2)] if name == "mini_nested" else [])
    it = iter(draws)
    pipe.train()
    loss = pipe.get_loss(smp, time=time.cuda(), noise_fn=lambda like: next(it).to(like.device))[0]
    assert O.rel_l2(loss.float().cpu(), gold["loss"]) < 1e-3


def test_mixed_ratio_train_loss_matches_reference_pipeline():
    """NestedDiffusion.get_loss with the shipped yaml key ``mixed_ratio: '2:1'`` (cc12m_256x256.yaml:108) and explicit
    micro-conditioning, B = 3 (the 32x32 level runs on 2 samples, the 16x16 level on 3): per-sample losses and every
    parameter-gradient norm vs what the REAL reference pipeline + reference NestedUNet produced on CPU
    (tests/golden/pipeline.pt; reference diffusion.py:258-275, 374-381, models/nested_unet.py:186-212)."""
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    gold = torch.load(os.path.join(GOLD, "pipeline.pt"), weights_only=False)["mini_nested_mixed"]
    model, _, _ = PC.build_module("mini_nested")
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=True, rescale_signal=1)
    pipe = D.NestedDiffusion(model, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False, use_double_loss=True,
                                                            no_use_residual=True, mixed_ratio="2:1")).to(torch.device("cuda:0"))
    inp = PC.inputs("mini_nested_mixed")
    g = torch.Generator().manual_seed(37)
    smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda(), "scale": inp["micros"]["scale"].cuda(),
           "images": (torch.rand(3, 3, 32, 32, generator=g) * 2 - 1).cuda()}
    torch.manual_seed(41)   # replay the reference's CPU draws: timesteps, eps, then one normal_() per lower resolution
    time = torch.randint(0, 1000, (3,))
    it = iter([torch.randn(3, 3, 32, 32), torch.randn(3, 3, 16, 16)])
    pipe.train()
    loss = pipe.get_loss(smp, time=time.cuda(), noise_fn=lambda like: next(it).to(like.device))[0]
    assert O.rel_l2(loss.float().cpu(), gold["loss"]) < 1e-4
    loss.sum().backward()
    norms = sorted(gold["grad_norm"].values())
    floor = 1e-2 * norms[len(norms) // 2]
    for k, p in model.named_parameters():
        n = gold["grad_norm"][k]
        assert abs(float(p.grad.double().norm()) - n) <= 1e-3 * max(n, floor), k


def test_fused_train_step_matches_torch_optimizer():
    """TrainStep(fused=True): gradient sink + mdm_sumsq + mdm_adamw_ema_step  ==  autograd accumulation +
    clip_grad_norm_-style scaling + torch.optim.AdamW + EMA lerp, over 3 steps on the same batch / timesteps / noise."""
    from mdm_hip import ops
    from mdm_hip.trainer import TrainStep

    results = []
    for fused in (False, True):
        ops.set_grad_sink(None)
        model, _, _ = PC.build_module("mini_unet")
        pipe = _pipeline("mini_unet", model).to(torch.device("cuda:0"))
        step = TrainStep(pipe, bf16=False, lr=1e-3, clip_norm=0.5, ema_decay=0.9, fused=fused)
        inp = PC.inputs("mini_unet")
        g = torch.Generator().manual_seed(29)
        smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda(),
               "images": (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).cuda()}
        noise = torch.randn(2, 3, 16, 16, generator=g).cuda()
        losses = [step(smp, time=torch.tensor([100, 700]).cuda(), noise_fn=lambda like: noise) for _ in range(3)]
        params = {k: v.detach().float().cpu().clone() for k, v in model.named_parameters()}
        ema = {k: v.detach().float().cpu().clone() for k, v in step.ema_state().items()}
        results.append((losses, params, ema))
    ops.set_grad_sink(None)
    (l0, p0, e0), (l1, p1, e1) = results
    assert all(abs(a - b) <= 1e-4 * abs(a) + 1e-7 for a, b in zip(l0, l1)), (l0, l1)
    assert l0[2] < l0[0]
    # Adam normalises every gradient to +-lr, including the pure-rounding-noise gradients of parameters whose true
    # gradient is zero (conv bias in front of a 1-channel-per-group GroupNorm): those few tensors differ by O(lr)
    # between ANY two fp32 implementations, so the check is aggregate plus a loose per-tensor bound.
    def agg(a, b):
        num = sum(float((a[k].double() - b[k].double()).pow(2).sum()) for k in a)
        den = sum(float(b[k].double().pow(2).sum()) for k in a)
        return (num / den) ** 0.5

    assert agg(p1, p0) < 1e-4 and agg(e1, e0) < 1e-4
    for k in p0:
        assert O.rel_l2(p1[k], p0[k]) < 5e-3, k


def test_non_finite_step_is_skipped_on_the_device():
    """a NaN loss (here: a NaN in the images) must leave parameters, moments, EMA and the optimizer's step number untouched
    and clear the gradients -- decided on the device from the gradient norm, no host look at the loss mid-step
    (reference trainer.py:37-41 returns before backward)"""
    from mdm_hip import ops
    from mdm_hip.trainer import TrainStep

    ops.set_grad_sink(None)
    model, _, _ = PC.build_module("mini_unet")
    pipe = _pipeline("mini_unet", model).to(torch.device("cuda:0"))
    step = TrainStep(pipe, bf16=False, lr=1e-2, fused=True)
    inp = PC.inputs("mini_unet")
    g = torch.Generator().manual_seed(3)
    smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda(), "images": (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).cuda()}
    step(smp)
    p1, m1, e1 = step.flat_p.clone(), step.m.clone(), step.flat_ema.clone()
    bad = dict(smp, images=smp["images"].clone())
    bad["images"][0, 0, 0, 0] = float("nan")
    lv = step(bad)
    assert lv != lv
    assert torch.equal(step.flat_p, p1) and torch.equal(step.m, m1) and torch.equal(step.flat_ema, e1)
    assert float(step.reducer.flat.abs().max()) == 0.0 and int(step.step_dev) == 1 and step.steps == 1
    step(smp)
    ops.set_grad_sink(None)
    assert int(step.step_dev) == 2 and not torch.equal(step.flat_p, p1) and bool(torch.isfinite(step.flat_p).all())


def test_weights_are_repacked_after_an_optimizer_step():
    """the packed kernel-layout weights must follow parameter updates that do not bump Tensor._version"""
    from mdm_hip import ops
    from mdm_hip.trainer import TrainStep

    ops.set_grad_sink(None)
    model, _, _ = PC.build_module("mini_unet")
    pipe = _pipeline("mini_unet", model).to(torch.device("cuda:0"))
    step = TrainStep(pipe, bf16=False, lr=5e-2, fused=True)
    inp = PC.inputs("mini_unet")
    args = (inp["x"].cuda(), inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda())
    with torch.no_grad():
        y0 = model(*args).clone()
    g = torch.Generator().manual_seed(3)
    smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda(), "images": (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).cuda()}
    step(smp)
    with torch.no_grad():
        y1 = model(*args)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ops.set_grad_sink(None)
    assert O.rel_l2(y1, y0) > 1e-3                      # the update is visible through the kernels
    _, cfg, _ = PC.build_module("mini_unet")
    y_ref = O.model_forward(sd, cfg, inp["x"], inp["times"], inp["cond"], inp["mask"])
    assert O.rel_l2(y1.cpu(), y_ref) < 1e-4             # ... and it is exactly the updated parameters


def _full_gold(name):
    return torch.load(os.path.join(GOLD, "full_size.pt"), weights_only=False)[name]


def _agg_grad_err(grads, gold):
    """aggregate ||g - g_ref|| / ||g_ref|| over all parameters, estimated from the golden file's seeded random
    projections: E[<g - g_ref, probe>^2] = ||g - g_ref||^2 for a unit-variance probe, summed over ~700 tensors"""
    num = sum((float((grads[k].detach().double().cpu() * PC.probe_for(k, grads[k].shape)).sum()) - pr) ** 2
              for k, pr in gold["grad_probe"].items())
    den = sum(n * n for n in gold["grad_norm"].values())
    return (num / den) ** 0.5


@pytest.mark.parametrize("which", list(PC.FULL))
def test_full_size_architectures_match_reference(which):
    """The SHIPPED architectures at full size (BASELINE.json configs[0..4]: 461 M / 477 M / 481 M parameters), HIP
    path vs what the REAL reference produced on the same seeded weights / inputs (tests/golden/full_size.pt):
      fp32 mode: every output (1e-4) and -- unet64 (B=2), nested256 -- every parameter gradient through its norm and a
                 seeded random projection (2e-3 of max(norm, floor));
      bf16 mode: forward error and the aggregate gradient error are PRINTED and gated at the reference's own
                 bf16-autocast error on the same case (tests/golden/reference_bf16_error.pt; 1.30e-2 for the UNet-64
                 forward).
    nested1024 exercises the x / std input normalisation kernel of its 256 level (models/unet.py:871-872)."""
    gold = _full_gold(which)
    model, _ = PC.full_module(which)
    inp = PC.full_inputs(which)
    model = model.cuda()
    xs = [t.cuda() for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].cuda()
    args = (xs, inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda())
    with_grad = "grad_norm" in gold
    with torch.set_grad_enabled(with_grad):
        out = PC.as_list(model(*args))
    for i, (o, gd) in enumerate(zip(out, gold["outputs"])):
        PC.check_summary(o.float(), gd, "%s.out%d" % (which, i), 1e-4)
    if with_grad:
        PC.loss_of(out, inp["gys"]).backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        norms = sorted(gold["grad_norm"].values())
        floor = 1e-2 * norms[len(norms) // 2]
        bad = []
        for k, n in gold["grad_norm"].items():
            gk = grads[k].double().cpu()
            mine = float(gk.norm())
            probe = float((gk * PC.probe_for(k, gk.shape)).sum())
            if n < 0.1 * floor:
                # a gradient that is mathematically zero (bias of a conv in front of a 1-channel-per-group GroupNorm: the
                # outer 32-channel levels of the 1024 net) is rounding noise of a sum over up to 10^6 pixels on BOTH
                # sides; the two noises need not agree, they only have to be negligible: < 0.5 % of the median norm
                ok = mine <= 0.5 * floor
            else:
                ok = abs(mine - n) <= 2e-3 * max(n, floor) and abs(probe - gold["grad_probe"][k]) <= 8e-3 * max(n, floor)
            if not ok:
                bad.append((k, mine, n, probe, gold["grad_probe"][k]))
        assert not bad, (floor, bad[:8])
        agg32 = _agg_grad_err(grads, gold)
        model.zero_grad(set_to_none=True)
    # bf16 mode on the same input
    with torch.set_grad_enabled(with_grad), torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = PC.as_list(model(*args))
    errs = []
    for i, (o, gd) in enumerate(zip(out16, gold["outputs"])):
        st = max(1, o.shape[-1] // 64)
        errs.append(O.rel_l2(o.float()[..., ::st, ::st], gd["sub"]))
    bar = REF_BF16[which]
    msg = "[bf16 %s] forward rel-L2 vs reference fp32: %s (reference's own bf16 error: %s)" % (
        which, ", ".join("%.3e" % e for e in errs), ", ".join("%.3e" % e for e in bar["fwd"]))
    if with_grad:
        PC.loss_of(out16, inp["gys"]).backward()
        agg16 = _agg_grad_err({k: p.grad for k, p in model.named_parameters()}, gold)
        msg += "; aggregate parameter-gradient error fp32 %.2e, bf16 %.3e (reference's own: %.3e)" % (agg32, agg16, bar["grad_agg"])
    print(msg)
    assert all(e <= b for e, b in zip(errs, bar["fwd"])), msg
    if with_grad:
        assert agg32 < 5e-4 and agg16 <= bar["grad_agg"], msg


def test_config0_pipeline_at_full_size():
    """BASELINE.json configs[0] at its REAL size: cc12m_64x64 U-Net (461 M parameters), batch 2, 4 diffusion steps
    (DDIM eta=0), random text embeddings; Diffusion.sample() and get_loss() through the HIP denoiser and the fused
    sampler / loss kernels vs the images / losses the real reference pipeline produced on CPU.
    Gate: 1e-3 rel-L2 (north_star: "sampled images within 1e-3 rel-L2 of reference")."""
    gold = _full_gold("unet64")
    model, _ = PC.full_module("unet64")
    pipe = _pipeline("mini_unet", model).to(torch.device("cuda:0"))
    inp = PC.full_inputs("unet64")
    smp = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda()}
    torch.manual_seed(23)
    with torch.no_grad():
        img = pipe.sample(2, smp, 64, torch.device("cuda:0"), resample_steps=True, num_inference_steps=4, ddim_eta=0)
    e_img = O.rel_l2(img.cpu(), gold["sample"])
    g = torch.Generator().manual_seed(29)
    smp["images"] = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
    torch.manual_seed(31)
    time = torch.randint(0, 1000, (2,))
    eps = torch.randn(2, 3, 64, 64)
    pipe.train()
    loss = pipe.get_loss(smp, time=time.cuda(), noise_fn=lambda like: eps.to(like.device))[0]
    e_loss = O.rel_l2(loss.float().cpu(), gold["loss"])
    print("[configs[0], full size] 4-step sample rel-L2 %.3e, train loss rel-L2 %.3e" % (e_img, e_loss))
    assert e_img < 1e-3 and e_loss < 1e-3


def test_residual_gradient_with_two_consumers_under_async_wgrad():
    """ConvFn.backward hands `dy` on as the gradient of its residual input while the side stream still reads it for
    the weight gradient.  When that tensor has a second consumer the engine ACCUMULATES into the first gradient;
    it must not do so in place under the side stream's reads."""
    from mdm_hip import ops

    class Sink:
        def __init__(self, params):
            self.slots = {p.data_ptr(): torch.zeros_like(p) for p in params}

        def slot(self, p):
            return self.slots.get(p.data_ptr())

        def ready(self, p):
            pass

    g = torch.Generator().manual_seed(1)
    N, H, C = 8, 32, 256
    x0 = torch.randn(N, H, H, C, generator=g).cuda().to(torch.bfloat16)
    h0 = torch.randn(N, H, H, C, generator=g).cuda().to(torch.bfloat16)
    w = (torch.randn(C, C, 3, 3, generator=g) / 48).cuda().requires_grad_()
    b = torch.zeros(C).cuda().requires_grad_()
    res = []
    for async_on in (False, True):
        sink = Sink([w, b])
        ops.set_grad_sink(sink)
        ops.enable_async_wgrad(async_on)
        x = x0.clone().requires_grad_()
        h = h0.clone().requires_grad_()
        y = ops.conv(h, w, b, residual=x)          # dres = dy lands first in x's input buffer ...
        z = ops.silu(x)                            # ... and the second consumer's gradient is added to it
        for _ in range(6):                         # keep the side stream busy while the main stream moves on
            y = ops.conv(y, w, b, residual=x)
        (y.float().square().sum() * 1e-3 + z.float().sum()).backward()
        ops.join_side_stream()
        torch.cuda.synchronize()
        res.append((x.grad.clone(), sink.slots[w.data_ptr()].clone()))
    ops.set_grad_sink(None)
    ops.enable_async_wgrad(False)
    assert torch.equal(res[0][0], res[1][0])
    assert O.rel_l2(res[1][1], res[0][1]) < 1e-6   # same kernels, same summation order: the side stream only moves them


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_graph_replay_matches_eager(name):
    """GraphedDenoiser: hipGraph replay of the forward == eager forward, bit for bit, also after the inputs change"""
    from mdm_hip.graph import GraphedDenoiser

    model, _, _ = PC.build_module(name)
    model = model.cuda().eval()
    graphed = GraphedDenoiser(model)
    inp = PC.inputs(name)
    to_dev = lambda v: [t.cuda() for t in v] if isinstance(v, list) else v.cuda()
    with torch.no_grad():
        for shift in (0.0, 0.37):
            x = inp["x"]
            x = [t + shift for t in x] if isinstance(x, list) else x + shift
            times = inp["times"] - int(shift * 10)
            args = (to_dev(x), times.cuda(), inp["cond"].cuda() * (1 + shift), inp["mask"].cuda())
            eager = PC.as_list(model(*args))
            replay = PC.as_list(graphed(*args))
            for a, b in zip(eager, replay):
                assert torch.equal(a, b)
    assert len(graphed._graphs) == 1
    assert graphed.input_channels == 3


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
@pytest.mark.parametrize("mode", ["ddim", "ddpm_cfg", "ddpm_dynamic", "ddim_eta05", "ddpm_none"])
def test_graphed_sampler_matches_eager_sampler(name, mode):
    """GraphedSampler (one hipGraph replay per WHOLE denoise iteration: schedule lookup, denoiser, fused update of every
    scale, RNG / step-counter advance) == the eager sampler on the same start noise; DDPM mode draws its noise inside
    the step kernel from the same device generator state in both.  ``ddim_eta05``: noisy DDIM (eta-scaled beta_tilde with
    in-kernel noise and the noise gate); ``ddpm_none``: threshold NONE."""
    from mdm_hip.graph import GraphedSampler

    model, _, _ = PC.build_module(name)
    threshold = {"ddpm_dynamic": "DYNAMIC_IF", "ddpm_none": "NONE"}.get(mode, "CLIP")
    pipe = _pipeline(name, model, threshold=threshold).to(torch.device("cuda:0"))
    pipe.eval()
    inp = PC.inputs(name)
    cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
    if mode in ("ddim", "ddim_eta05"):
        kw = dict(ddim_eta=0 if mode == "ddim" else 0.5)
    else:
        kw = dict(ddim_eta=None, guidance_scale=2.5 if mode == "ddpm_cfg" else 1)
    if mode == "ddpm_cfg":
        cond, mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
    smp = {"lm_outputs": cond, "lm_mask": mask}
    side = 32 if name == "mini_nested" else 16
    g = torch.Generator().manual_seed(41)
    start = [torch.randn(2, 3, side, side, generator=g).cuda()]
    if name == "mini_nested":
        start.append(torch.randn(2, 3, side // 2, side // 2, generator=g).cuda())
    n = 5
    with torch.no_grad():
        pipe.sampler.use_device_rng(1234, "cuda:0")
        x0 = [t.clone() for t in start]
        eager = pipe.sampler.sample(pipe.get_model(), x0 if name == "mini_nested" else x0[0], cond, mask, {},
                                    resample_steps=True, num_inference_steps=n, **kw)
        gs = GraphedSampler(pipe, seed=1234)
        for rep in range(2):   # the second call replays the cached graph on fresh inputs
            out = gs.sample(2, smp, side, torch.device("cuda:0"), num_inference_steps=n, start_noise=start, seed=1234, **kw)
            assert O.rel_l2(out, eager) < 1e-6, rep
    pipe.sampler.device_rng = None
    assert len(gs._graphs) == 1


def test_graphed_sampler_passes_micro_conditioning_and_handles_one_step_schedules():
    """GraphedSampler.sample must hand the sample's micro-conditioning (``scale`` ...) to the denoiser
    like Diffusion.sample does (reference diffusion.py:194-196) -- different values, different images -- and a
    1-step schedule must survive the warm-up passes; without ``seed=`` the first call starts the generator at
    (seed, 0) like the eager sampler after use_device_rng(seed)."""
    from mdm_hip.graph import GraphedSampler

    model, _, _ = PC.build_module("mini_unet")
    pipe = _pipeline("mini_unet", model).to(torch.device("cuda:0"))
    pipe.eval()
    inp = PC.inputs("mini_unet")
    cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
    g = torch.Generator().manual_seed(41)
    start = torch.randn(2, 3, 16, 16, generator=g).cuda()
    outs = {}
    with torch.no_grad():
        for tag, micros in (("default", {}), ("scale", {"scale": torch.tensor([7.0, 40.0]).cuda()})):
            for n in (4, 1):
                pipe.sampler.use_device_rng(99, "cuda:0")
                eager = pipe.sampler.sample(pipe.get_model(), start.clone(), cond, mask, micros, resample_steps=True,
                                            num_inference_steps=n, ddim_eta=None)
                gs = GraphedSampler(pipe, seed=99)
                smp = dict({"lm_outputs": cond, "lm_mask": mask}, **micros)
                out = gs.sample(2, smp, 16, torch.device("cuda:0"), num_inference_steps=n, start_noise=start)   # no seed=
                assert O.rel_l2(out, eager) < 1e-6, (tag, n)
                outs[(tag, n)] = out
    pipe.sampler.device_rng = None
    assert O.rel_l2(outs[("scale", 4)], outs[("default", 4)]) > 1e-4


@pytest.mark.parametrize("name", ["nested1024_ddpm", "unet64_ddpm50", "unet64_ddim100", "nested1024_ddpm250"])
def test_long_horizon_sampling_matches_reference(name, tmp_path):
    """Long sampling runs at FULL size against the real reference pipeline (tests/golden/long_sampling.pt, made by
    oracle/make_golden.py long): BASELINE.json configs[4] -- the 64+256+1024 NestedUNet, ancestral DDPM (ddim_eta=1,
    generate_sample.py:546-551), 25 steps, B=1, weights round-tripped through UNet.save -> UNet.load -- the same over the
    demo's full 250 steps (configs[4] as stated; round 6) -- and the 64x64 U-Net over 50 DDPM / 100 DDIM steps.  The reference consumed, draw by draw, the host replay of the numbers the step
    kernel generates from DeviceRng(LONG_SEED) (oracle/philox_ref.py), so both sides see identical noise.
    Gate: 1e-3 rel-L2 in fp32 (north_star); the bf16-autocast error of the same run is printed."""
    import make_golden as MG
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    arch, B, steps, eta, skw = MG.LONG_CASES[name]
    gold = torch.load(os.path.join(GOLD, "long_sampling.pt"), weights_only=False)[name]
    src, sd = PC.full_module(arch)
    ck = str(tmp_path / "vis_model_synthetic.pth")
    src.save(ck, other_items={"batch_num": 7})
    del src
    model, _ = PC.full_module(arch, seed=3, param_seed=5)     # other values: everything must come from the file
    assert model.load(ck)["batch_num"] == 7
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    nested = len(PC.FULL[arch][1]) > 1
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", **skw)
    if nested:
        pipe = D.NestedDiffusion(model, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                use_double_loss=True, no_use_residual=True))
    else:
        pipe = D.Diffusion(model, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
    pipe = pipe.to(torch.device("cuda:0"))
    pipe.eval()
    inp = PC.full_inputs(arch)
    cond, mask = inp["cond"][:B].cuda(), inp["mask"][:B].cuda()
    start = [t.cuda() for t in MG.long_start_noise(name)]
    errs = {}
    from mdm_hip import ops

    for mode in ("fp32", "fp32x3", "bf16"):
        pipe.sampler.use_device_rng(MG.LONG_SEED, "cuda:0")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"), ops.fp32_split(mode == "fp32x3"):
            out = pipe.sampler.sample(pipe.get_model(), [t.clone() for t in start] if nested else start[0].clone(), cond, mask, {},
                                      resample_steps=True, num_inference_steps=steps, ddim_eta=eta)
        assert tuple(out.shape) == gold["shape"]
        if mode == "fp32":
            # the same number of noise draws as the reference made
            per_step = sum((t.numel() + 3) // 4 for t in start)
            assert int(pipe.sampler.device_rng.state[1]) == (gold["draws"] // len(start)) * per_step
            PC.check_summary(out.float(), gold["out"], "long." + name, 1e-3)
        if mode == "fp32x3":
            # fp32 tensors, bf16x3 products (MDM_F32_SPLIT): the mode the fp32 sampling bench legs time -- same gate
            PC.check_summary(out.float(), gold["out"], "long." + name, 1e-3)
        st = max(1, out.shape[-1] // 64)
        errs[mode] = O.rel_l2(out.float()[..., ::st, ::st], gold["out"]["sub"])
    pipe.sampler.device_rng = None
    print("[long sampling %s: %d steps, B=%d] rel-L2 vs the reference: fp32 %.3e, fp32 tensors / bf16x3 products %.3e, bf16 autocast %.3e"
          % (name, steps, B, errs["fp32"], errs["fp32x3"], errs["bf16"]))
    # measured (round 3): fp32 1.2e-6 / 6.7e-7 / 5.5e-7; bf16 autocast 8.2e-3 (nested-1024, 25 steps), 4.4e-3 (UNet-64, 50 / 100 steps)
    assert errs["bf16"] < 2.5e-2
