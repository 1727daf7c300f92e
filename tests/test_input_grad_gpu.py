"""GPU: autograd with respect to the model's own input on the HIP path, and loss-guided sampling on top of it.

  * mdm_conv3x3_stem_dgrad against fp64 autograd of F.conv2d on the dtype-rounded operands: integer data (0 differing
    elements), border impulses (exact), random data (rel-L2 <= 2e-5, the project's fp32 kernel gate), bit-identical reruns;
  * x.requires_grad_() on the mini models: input and conditioning gradients against the CPU oracle run on the same leaves
    (fp32: rel-L2 < 1e-3 per tensor; bf16: 1.5 x the oracle's own bf16-autocast error, computed here), bit-equality of
    outputs and parameter gradients with and without it, frozen parameters, recomputation, LoRA, the MXFP8 refusal;
  * Sampler.sample(guide=LossGuide(...)): 4 steps against the same sampler driven by the CPU oracle and torch autograd.

Measured values are printed (pytest -s)."""
import functools
import types

import pytest
import torch

import input_grad_cases as IG
import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float32]
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


# ---- the kernel ----------------------------------------------------------------------------------------------------
def _dgrad(dy, w):
    from mdm_hip import ops

    return ops.conv3x3_stem_dgrad(dy.to(DEV), w)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", IG.STEM_SHAPES, ids=_id)
def test_stem_dgrad_integer_data_is_exact(shape, dtype):
    """dy and w from {-2 .. 2}: every sum is below 2^24, fp32 accumulation is exact -> 0 differing elements"""
    dy, w = IG.stem_operands(shape, dtype, "int")
    dx = _dgrad(dy, w.to(DEV))
    ref = IG.stem_dgrad_reference(dy, w, dtype)
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (shape[0], shape[4], shape[1], shape[2]) and dx.is_contiguous()
    assert int((dx.cpu().double() != ref).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", IG.STEM_SHAPES, ids=_id)
def test_stem_dgrad_border_impulses(shape, dtype):
    """a one-hot dy at the four corners, an edge midpoint and the centre: dx is the flipped filter clipped by the image,
    zero elsewhere, exactly"""
    N, H, W, Cout, Cin = shape
    _, w = IG.stem_operands(shape, dtype, "rand")
    wd = w.to(DEV)
    for i, (py, px) in enumerate(IG.impulse_positions(H, W)):
        n, co = N - 1, (7 * i + 3) % Cout
        dy = torch.zeros(N, H, W, Cout, dtype=dtype)
        dy[n, py, px, co] = 1
        assert torch.equal(_dgrad(dy, wd).cpu(), IG.impulse_expected(w, dtype, shape, n, py, px, co)), (py, px)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", IG.STEM_SHAPES, ids=_id)
def test_stem_dgrad_random_data(shape, dtype):
    """inputs are dtype-exact and the output is fp32, so only the accumulation order differs: rel-L2 <= 2e-5 in both dtypes
    (sqrt(K) 2^-24 ~ 3e-6 at K = 2304 sits well inside); two runs are bit-identical"""
    dy, w = IG.stem_operands(shape, dtype, "rand")
    wd = w.to(DEV)
    a, b = _dgrad(dy, wd), _dgrad(dy, wd)
    err = O.rel_l2(a.cpu().double(), IG.stem_dgrad_reference(dy, w, dtype))
    print("[stem dgrad %s %s] rel-L2 vs fp64 %.3e" % (_id(shape), _id(dtype), err))
    assert err <= 2e-5
    assert torch.equal(a, b)


def test_stem_dgrad_limits():
    """more than 8 input channels on a padded stem keeps raising, and the message names the limit"""
    from mdm_hip import _lib, ops

    w = torch.randn(32, 9, 3, 3, device=DEV)
    x = torch.randn(1, 9, 8, 8, device=DEV, requires_grad=True)
    with pytest.raises(_lib.MdmHipError, match="at most 8 input"):
        ops.stem_conv(x, w, None, torch.bfloat16)


# ---- function and model --------------------------------------------------------------------------------------------
def _autocast(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)


def _hip(name, dtype, x_grad=True, cond_grad=False, frozen=False, setup=None, profile=False):
    """-> dict(outs, dx (list), dcond, grads, names): one forward + backward of the HIP module"""
    from mdm_hip import ops

    model = PC.build_module(name)[0].to(DEV)
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    handle = setup(model) if setup is not None else None
    inp = PC.inputs(name)
    xs = [t.to(DEV).requires_grad_(x_grad) for t in PC.as_list(inp["x"])]
    cond = inp["cond"].to(DEV).requires_grad_(cond_grad)
    micros = {k: v.to(DEV) for k, v in inp["micros"].items()}
    if profile:
        ops.profile_begin(shapes=True)
    try:
        with _autocast(dtype):
            outs = model(xs if isinstance(inp["x"], list) else xs[0], inp["times"].to(DEV), cond, inp["mask"].to(DEV), micros)
        PC.loss_of(outs, inp["gys"]).backward()
    finally:
        rec = ops.profile_end(1.0) if profile else None
    torch.cuda.synchronize()
    names = (list(rec["all_gemm_kernels"]) + list(rec["hbm_kernels"])) if rec else []
    del handle
    return dict(outs=[o.detach().float().cpu() for o in PC.as_list(outs)], dx=[t.grad for t in xs], dcond=cond.grad,
                grads={k: p.grad for k, p in model.named_parameters()}, names=names)


@functools.lru_cache(maxsize=None)
def _oracle(name, bf16=False):
    """the CPU oracle on the same leaves -> (input gradients hi -> lo, conditioning gradient); computed once per case"""
    _, cfg, sd = PC.build_module(name)
    inp = PC.inputs(name)
    xs = [t.clone().requires_grad_(True) for t in PC.as_list(inp["x"])]
    cond = inp["cond"].clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        outs = O.model_forward(sd, cfg, xs if isinstance(inp["x"], list) else xs[0], inp["times"], cond, inp["mask"], inp["micros"])
    PC.loss_of(outs, inp["gys"]).backward()
    return [t.grad.float() for t in xs], cond.grad.float()


@pytest.mark.parametrize("name", IG.MODEL_CASES)
def test_input_and_conditioning_gradients_fp32(name):
    """THE test that fails without the feature: x.requires_grad_() for every scale and cond.requires_grad_(), backward
    completes; rel-L2 < 1e-3 per tensor against the oracle (the project's gradient gate)"""
    r = _hip(name, torch.float32, x_grad=True, cond_grad=True)
    dx_ref, dc_ref = _oracle(name)
    errs = [O.rel_l2(a.cpu(), b) for a, b in zip(r["dx"], dx_ref)] + [O.rel_l2(r["dcond"].cpu(), dc_ref)]
    print("[input grad fp32 %s] rel-L2 vs oracle: x %s, cond %.3e" % (name, ["%.3e" % e for e in errs[:-1]], errs[-1]))
    assert all(g.dtype == torch.float32 and g.shape == x.shape for g, x in zip(r["dx"], dx_ref))
    assert max(errs) < 1e-3, errs


@pytest.mark.parametrize("name", IG.MODEL_CASES)
def test_input_and_conditioning_gradients_bf16(name):
    """bf16 mode.  Yardstick: the CPU oracle's own error when the same case runs under bf16 autocast, against its fp32 run
    (no recorded reference figure exists for input gradients); margin 1.5 x, as test_lm_head_bf16 takes for a quantity
    without a recorded figure -- the roundings fall in different places."""
    r = _hip(name, torch.bfloat16, x_grad=True, cond_grad=True)
    (dx_ref, dc_ref), (dx_bf, dc_bf) = _oracle(name), _oracle(name, True)
    errs = [O.rel_l2(a.cpu(), b) for a, b in zip(r["dx"], dx_ref)] + [O.rel_l2(r["dcond"].cpu(), dc_ref)]
    bars = [O.rel_l2(a, b) for a, b in zip(dx_bf, dx_ref)] + [O.rel_l2(dc_bf, dc_ref)]
    print("[input grad bf16 %s] rel-L2 vs fp32 oracle: x %s cond %.3e; the oracle's own under bf16 autocast: x %s cond %.3e" % (
        name, ["%.3e" % e for e in errs[:-1]], errs[-1], ["%.3e" % e for e in bars[:-1]], bars[-1]))
    assert all(torch.isfinite(g).all() for g in r["dx"])
    assert all(e <= 1.5 * b for e, b in zip(errs, bars)), (errs, bars)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("name", IG.MODEL_CASES)
def test_outputs_and_parameter_gradients_do_not_depend_on_input_grad(name, dtype):
    """bit-equality with the path that exists today: outputs and EVERY parameter gradient, with and without
    x.requires_grad (the same launches forward, the same weight-gradient launches backward)"""
    a, b = _hip(name, dtype, x_grad=False), _hip(name, dtype, x_grad=True)
    assert all(torch.equal(u, v) for u, v in zip(a["outs"], b["outs"]))
    assert a["grads"].keys() == b["grads"].keys() and all(g is not None for g in b["grads"].values())
    bad = [k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])]
    assert not bad, bad
    assert all(g is None for g in a["dx"]) and all(g is not None for g in b["dx"])


def test_fused_train_batch_does_not_depend_on_input_grad():
    """the same through trainer.train_batch, fused (gradient sink, side stream), one optimizer step on mini_unet: a forward
    pre-hook makes the denoiser's x_t require grad"""
    from mdm_hip import diffusion as D
    from mdm_hip import ops, samplers as S, trainer

    res = []
    for hook in (False, True):
        ops.set_grad_sink(None)
        model = PC.build_module("mini_unet")[0]
        scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM")
        pipe = D.Diffusion(model, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False)).to(torch.device(DEV))
        vm = pipe.model.vision_model
        seen = []
        if hook:
            vm.register_forward_pre_hook(lambda m, args: (seen.append(args[0]), (args[0].requires_grad_(True),) + tuple(args[1:]))[1])
        opt = torch.optim.AdamW(vm.parameters(), lr=1e-3, weight_decay=0, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
        inp = PC.inputs("mini_unet")
        g = torch.Generator().manual_seed(29)
        sample = {"lm_outputs": inp["cond"].to(DEV), "lm_mask": inp["mask"].to(DEV),
                  "images": (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(DEV)}
        torch.manual_seed(100)
        out = trainer.train_batch(pipe, sample, opt, sched, None, types.SimpleNamespace(fp16=True, gradient_clip_norm=0.5),
                                  grad_scaler=None, accumulate_gradient=False, num_grad_accumulations=1, ema_model=None)
        torch.cuda.synchronize()
        assert getattr(opt, "_mdm_fused", None) not in (None, False), getattr(opt, "_mdm_fused_reason", None)
        assert bool(seen) == hook
        if hook:   # the stem took ops.stem_conv inside the fused step: the gradient reached the denoiser's input
            assert seen[0].grad is not None and torch.isfinite(seen[0].grad).all() and float(seen[0].grad.abs().max()) > 0
        res.append((float(out[0]), {k: v.detach().clone() for k, v in vm.named_parameters()}))
        ops.set_grad_sink(None)
    assert res[0][0] == res[1][0]
    bad = [k for k in res[0][1] if not torch.equal(res[0][1][k], res[1][1][k])]
    assert not bad, bad


@pytest.mark.parametrize("name", IG.MODEL_CASES)
def test_frozen_parameters_launch_no_weight_gradient(name):
    """every parameter frozen: the input gradient is bit-identical to the one obtained with trainable parameters, every
    p.grad stays None and the profile records no launch whose name contains "wgrad" (it does with trainable parameters)"""
    dt = torch.bfloat16
    a = _hip(name, dt, cond_grad=True, profile=True)
    b = _hip(name, dt, cond_grad=True, frozen=True, profile=True)
    assert all(torch.equal(u, v) for u, v in zip(a["dx"], b["dx"])) and torch.equal(a["dcond"], b["dcond"])
    assert all(g is None for g in b["grads"].values())
    assert any("wgrad" in n for n in a["names"]) and any("stem_dgrad" in n for n in b["names"])
    assert not [n for n in b["names"] if "wgrad" in n]   # the GroupNorm row sums and the grouped launches are profiled too


def test_frozen_groupnorm_and_shared_linears_launch_nothing_for_their_parameters():
    """the two gates the model test cannot isolate.  GroupNorm with three samples and no gradient sink: trainable gamma /
    beta take per-sample rows and a fixed-order sum (profiled as "... rows sum (wgrad ...)"), deterministic over reruns;
    frozen ones keep the single launch.  SharedInputLinearsFn: the grouped weight-gradient launch goes when every layer of
    a width is frozen, and the input gradient keeps its bits."""
    from mdm_hip import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 8, 8, 64, generator=g).to(DEV, torch.bfloat16)
    dy = torch.randn(3, 8, 8, 64, generator=g).to(DEV, torch.bfloat16)

    def gn(trainable):
        gamma, beta = (torch.randn(64, generator=torch.Generator().manual_seed(6)).to(DEV).requires_grad_(trainable) for _ in range(2))
        xi = x.clone().requires_grad_(True)
        ops.profile_begin(shapes=True)
        try:
            ops.group_norm(xi, gamma, beta, 32, silu=True).backward(dy)
        finally:
            ops._prof, rec = None, ops._prof
        return xi.grad, gamma.grad, beta.grad, [r[1] for r in rec]

    a, b, c = gn(True), gn(True), gn(False)
    assert any("rows sum" in n for n in a[3]) and not any("wgrad" in n for n in c[3])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])                 # deterministic
    assert torch.equal(a[0], c[0]) and c[1] is None and c[2] is None

    xl = torch.randn(4, 128, generator=g).to(DEV, torch.bfloat16)
    dys = [torch.randn(4, n, generator=g).to(DEV, torch.bfloat16) for n in (64, 64, 128)]

    def lin(trainable):
        gw = torch.Generator().manual_seed(8)
        layers = [(torch.randn(n, 128, generator=gw).to(DEV).requires_grad_(trainable),
                   torch.randn(n, generator=gw).to(DEV).requires_grad_(trainable)) for n in (64, 64, 128)]
        assert ops.shared_input_linears_supported(xl, layers)
        xi = xl.clone().requires_grad_(True)
        ys = ops.shared_input_linears(xi, layers)
        ops.profile_begin(shapes=True)
        try:
            torch.autograd.backward(list(ys), dys)
        finally:
            ops._prof, rec = None, ops._prof
        return xi.grad, [w.grad for w, _ in layers], [r[1] for r in rec]

    t, f = lin(True), lin(False)
    assert sum("wgrad" in n for n in t[2]) == 2 and all(w is not None for w in t[1])   # one grouped launch per width
    assert not any("wgrad" in n for n in f[2]) and all(w is None for w in f[1])
    assert torch.equal(t[0], f[0])


def test_guide_seed_clip_detection_at_a_scale_that_does_not_round_trip():
    """mdm_guide_seed, image scale 3: the step kernel leaves +-fl(1 / 3) where it clipped, and fl(1 / 3) * 3 need not be 1"""
    from mdm_hip import ops

    s = 3.0
    raw = torch.linspace(-0.6, 0.6, 64).reshape(1, 1, 8, 8)
    x0 = ((raw * s).clamp(-1, 1) / s).to(DEV)                                  # what clip 1 of the step kernel stores
    v = torch.ones_like(x0)
    a, b = torch.tensor([2.0], device=DEV), torch.tensor([-0.5], device=DEV)
    direct, seed = ops.guide_seed(v, x0, a, b, clip="CLIP", image_scale=s)
    inside = ((raw * s).abs() < 1).to(DEV)
    assert 0 < int(inside.sum()) < 64
    assert torch.equal(direct, torch.where(inside, torch.full_like(v, 2.0 * s), torch.zeros_like(v)))
    assert torch.equal(seed, torch.where(inside, torch.full_like(v, -0.5 * s), torch.zeros_like(v)))
    d0, s0 = ops.guide_seed(v, None, a, b, clip="NONE", image_scale=s)
    assert torch.equal(d0, torch.full_like(v, 2.0 * s)) and torch.equal(s0, torch.full_like(v, -0.5 * s))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested2"])
def test_composes_with_recomputation_and_lora(name):
    """with enable_activation_recompute(True), and with unmerged LoRA adapters (B = 0: the adapted function is the plain
    one), the input gradient equals the plain one bit for bit"""
    import mdm_hip

    dt = torch.bfloat16
    plain = _hip(name, dt)
    mdm_hip.enable_activation_recompute(True)
    try:
        rec = _hip(name, dt)
    finally:
        mdm_hip.enable_activation_recompute(False)
    lo = _hip(name, dt, setup=lambda m: mdm_hip.lora.attach(m, rank=8, conv_targets=("conv1", "conv2")))
    assert all(torch.equal(u, v) for u, v in zip(plain["dx"], rec["dx"]))
    assert all(torch.equal(u, v) for u, v in zip(plain["dx"], lo["dx"]))
    assert all(torch.equal(u, v) for u, v in zip(plain["outs"], lo["outs"]))


def test_mxfp8_layers_stay_inference_only():
    from mdm_hip import _lib, fp8

    with pytest.raises(_lib.MdmHipError, match="inference-only"):
        _hip("mini_unet", torch.bfloat16, frozen=True, setup=lambda m: fp8.attach(m))


# ---- the sampler ---------------------------------------------------------------------------------------------------
def _pipelines(name, threshold="CLIP"):
    """(the HIP pipeline on the GPU, the same sampler around the CPU oracle)"""
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    model, cfg, sd = PC.build_module(name)

    def wrap(net):
        scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                               loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=nested,
                               rescale_signal=1 if nested else None)
        if nested:
            return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                  use_double_loss=True, no_use_residual=True))
        return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))

    hip, cpu = wrap(model).to(torch.device(DEV)), wrap(IG.OracleNet(sd, cfg, nested))
    hip.eval(), cpu.eval()
    return hip, cpu


def _sampling_inputs(name, guidance=1):
    inp = PC.inputs(name)
    side = 32 if name == "mini_nested" else 16
    g = torch.Generator().manual_seed(23)
    xs = [torch.randn(2, 3, side, side, generator=g)] + ([torch.randn(2, 3, side // 2, side // 2, generator=g)] if name == "mini_nested" else [])
    target = torch.rand(2, 3, side, side, generator=g) * 2 - 1
    m = (torch.rand(2, 1, side, side, generator=g) < 0.5).float()
    cond, mask = inp["cond"], inp["mask"]
    if guidance != 1:   # classifier-free guidance: [unconditional | conditional]
        cond, mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
    return xs, cond, mask, target, m


def _sample(pipe, xs, cond, mask, dev, **kw):
    x = [t.to(dev) for t in xs]
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        return pipe.sampler.sample(pipe.get_model(), x if len(x) > 1 else x[0], cond.to(dev), mask.to(dev), {},
                                   resample_steps=True, num_inference_steps=4, **kw).float().cpu()


@pytest.mark.parametrize("name,threshold,guidance", [("mini_unet", "CLIP", 1), ("mini_unet", "DYNAMIC", 1), ("mini_unet", "CLIP", 2.0),
                                                     ("mini_nested", "CLIP", 1)])
def test_guided_sampling_matches_cpu_oracle(name, threshold, guidance):
    """4 DDIM steps with a masked-MSE guide, fp32: the HIP denoiser and its input gradient against the same 4 steps with
    the CPU oracle as the model and torch autograd.  rel-L2 of the final x < 1e-3 (the sampling gate of DESIGN section 3)."""
    from mdm_hip import LossGuide

    hip, cpu = _pipelines(name, threshold)
    xs, cond, mask, target, m = _sampling_inputs(name, guidance)
    kw = dict(ddim_eta=0, guidance_scale=guidance)
    a = _sample(hip, xs, cond, mask, DEV, guide=LossGuide(IG.masked_mse(target.to(DEV), m.to(DEV)), scale=1.0), **kw)
    b = _sample(cpu, xs, cond, mask, "cpu", guide=LossGuide(IG.masked_mse(target, m), scale=1.0), **kw)
    plain = _sample(cpu, xs, cond, mask, "cpu", **kw)
    err, moved = O.rel_l2(a, b), O.rel_l2(b, plain)
    print("[guided sampling %s %s cfg %s] rel-L2 vs the CPU oracle %.3e (the guide moved the result by %.3e)" % (name, threshold, guidance, err, moved))
    assert moved > 1e-2          # the guide is not a bystander
    assert err < 1e-3


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_guided_sampling_properties(name):
    """scale = 0 is bit-identical to guide=None; a guided run is deterministic; guided + known_images keeps the known region
    exact; guided + solver="dpmpp_2m" runs and differs from unguided; the parameters are trainable again afterwards"""
    from mdm_hip import LossGuide

    hip, _ = _pipelines(name)
    xs, cond, mask, target, m = _sampling_inputs(name)
    fn = IG.masked_mse(target.to(DEV), m.to(DEV))
    run = lambda **kw: _sample(hip, xs, cond, mask, DEV, **kw)
    plain, zero = run(ddim_eta=0), run(ddim_eta=0, guide=LossGuide(fn, scale=0.0))
    assert torch.equal(plain, zero)
    g1, g2 = run(ddim_eta=0, guide=LossGuide(fn, scale=1.0)), run(ddim_eta=0, guide=LossGuide(fn, scale=1.0))
    assert torch.equal(g1, g2) and not torch.equal(g1, plain)
    assert float(fn(g1.to(DEV)).sum()) < float(fn(plain.to(DEV)).sum())
    known = (target * 0.5).to(DEV)
    km = torch.zeros(2, 1, *target.shape[2:], device=DEV)
    km[..., : target.shape[-1] // 2] = 1
    out = run(ddim_eta=0, guide=LossGuide(fn, scale=1.0), known_images=known, known_mask=km)
    half = target.shape[-1] // 2
    assert torch.equal(out[..., :half], known.cpu()[..., :half]) and not torch.equal(out[..., half:], known.cpu()[..., half:])
    s_plain, s_guided = run(solver="dpmpp_2m"), run(solver="dpmpp_2m", guide=LossGuide(fn, scale=1.0))
    assert torch.isfinite(s_guided).all() and not torch.equal(s_plain, s_guided)
    assert all(p.requires_grad for p in hip.parameters())


def test_graphed_sampler_refuses_a_guide():
    from mdm_hip import LossGuide
    from mdm_hip.graph import GraphedSampler

    hip, _ = _pipelines("mini_unet")
    xs, cond, mask, target, m = _sampling_inputs("mini_unet")
    with pytest.raises(NotImplementedError, match="hipGraph"):
        GraphedSampler(hip).sample(2, {"lm_outputs": cond.to(DEV), "lm_mask": mask.to(DEV)}, 16, torch.device(DEV),
                                   guide=LossGuide(IG.masked_mse(target, m)))
