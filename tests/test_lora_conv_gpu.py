"""GPU: the 3x3 adapter kernels (csrc/lora.hip) against torch's conv2d / conv_transpose2d / autograd in fp64 on the CPU, the
autograd op against torch, and models with attention AND conv adapters against the oracle run on the merged state dict
(tests/lora_conv_cases.py) -- plus the identities: B = 0 changes nothing, merged == unmerged, detach restores, the base stays
frozen, a conv-only attach trains the outer nets of a nested model, the trainer's plain path moves the adapters only, and
graphed sampling follows attach / merge.

Gates: the op gates of tests/lora_cases.py (max-abs error over the largest reference magnitude: 2e-5 fp32, 3e-2 bf16, inputs
rounded through the dtype on both sides); the model gates of DESIGN.md section 3 (rel-L2 1e-4 outputs, 1e-3 gradients in
fp32); bf16 models: the oracle's own error when run in bf16 on the CPU, times 1.5 (the rule of tests/test_lora_gpu.py).
Measured values are printed (pytest -s); DESIGN.md section 4.9 is where they are recorded.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import lora_cases as LC
import lora_conv_cases as CC
import parity_cases as PC
import unet_oracle as O
from lora_cases import TOL, q, relerr

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
DEV = "cuda:0"
RANK, ALPHA, CONV_RANK, CONV_ALPHA, SEED = 8, 4, 4, 2, 3
NAMES = ["mini_unet", "mini_nested", "mini_nested2"]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _d(t, dtype):
    return t.to(dtype).to(DEV)


# ---- kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C,r", CC.SHAPES)
def test_lora_down_conv3x3(dtype, N, H, W, C, r):
    from mdm_hip import ops

    g = _g(N + H + W + C + r)
    x = q(torch.randn(N, H, W, C, generator=g) + 0.2, dtype)       # a non-zero mean: a row read from a neighbour shows
    a = q(torch.randn(r, 9, C, generator=g) / (9 * C) ** 0.5, dtype)
    t = ops.lora_down_conv3x3(_d(x, dtype), _d(a, dtype))
    assert t.shape == (N, H, W, r) and t.dtype == dtype
    err = relerr(t.float(), CC.down_ref(x, a))
    print("[lora_down_conv3x3 %s N=%d H=%d W=%d C=%d r=%d] %.3e" % (dtype, N, H, W, C, r, err))
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [0.5, 2.0])
@pytest.mark.parametrize("N,H,W,C,r", CC.SHAPES)
def test_lora_up_add_conv3x3(dtype, N, H, W, C, r, s):
    from mdm_hip import ops

    g = _g(N + H + W + C + r + 1)
    y, t = q(torch.randn(N, H, W, C, generator=g) + 0.3, dtype), q(torch.randn(N, H, W, r, generator=g) + 0.2, dtype)
    b = q(torch.randn(C, 9, r, generator=g) / (9 * r) ** 0.5, dtype)
    yd, td, bd = _d(y, dtype), _d(t, dtype), _d(b, dtype)
    out = ops.lora_up_add_conv3x3(yd, td, bd, s)
    assert out.data_ptr() == yd.data_ptr()                      # in place
    err = relerr(out.float(), CC.up_add_ref(y, t, b, s))
    # accumulate = 0 overwrites without reading y: NaNs in the destination do not come through
    fresh = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=DEV)
    ops.lora_up_add_conv3x3(fresh, td, bd, s, accumulate=False)
    err0 = relerr(fresh.float(), CC.up_add_ref(torch.zeros(N, H, W, C), t, b, s))
    # the backward's use: the flipped pack of A [r, C, 3, 3] gives torch's conv_transpose2d
    a4 = q(torch.randn(r, C, 3, 3, generator=g) / (9 * C) ** 0.5, dtype)
    dx = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=DEV)
    ops.lora_up_add_conv3x3(dx, td, _d(CC.pack_a_flipped(a4), dtype), s, accumulate=False)
    err_t = relerr(dx.float(), CC.dx_ref(t, a4, s))
    print("[lora_up_add_conv3x3 %s N=%d H=%d W=%d C=%d r=%d s=%g] add %.3e, overwrite %.3e, transposed %.3e" % (
        dtype, N, H, W, C, r, s, err, err0, err_t))
    assert err < TOL[dtype] and err0 < TOL[dtype] and err_t < TOL[dtype]
    # B = 0 leaves y bit-identical
    y0 = _d(y, dtype)
    ops.lora_up_add_conv3x3(y0, td, torch.zeros_like(bd), s)
    assert torch.equal(y0, _d(y, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C,r", CC.WGRAD_SHAPES)
def test_lora_wgrad_conv3x3(dtype, N, H, W, C, r):
    from mdm_hip import ops

    g = _g(N + H + W + C + r + 2)
    p, qq = q(torch.randn(N, H, W, r, generator=g) + 0.2, dtype), q(torch.randn(N, H, W, C, generator=g) + 0.2, dtype)
    pd, qd = _d(p, dtype), _d(qq, dtype)
    s = 0.5
    ref = CC.wgrad_ref(p, qq, s)
    d = ops.lora_wgrad_conv3x3(pd, qd, s)
    assert d.shape == (r, 9, C) and d.dtype == torch.float32
    err = relerr(d, ref)
    print("[lora_wgrad_conv3x3 %s N=%d H=%d W=%d C=%d r=%d] %.3e" % (dtype, N, H, W, C, r, err))
    assert err < TOL[dtype]
    assert torch.equal(d, ops.lora_wgrad_conv3x3(pd, qd, s))    # deterministic: two runs are bit-identical
    base = torch.randn(r, 9, C, generator=g)
    acc = base.to(DEV)
    ops.lora_wgrad_conv3x3(pd, qd, s, out=acc)                  # accumulate = 1
    assert relerr(acc, base.double() + ref) < TOL[dtype]


@pytest.mark.parametrize("cout,cin,r", CC.MERGE_SHAPES)
def test_merge_unmerge_on_a_3x3_fp32_master(cout, cin, r):
    """W [Cout, Cin, 3, 3] += s (B @ A.view(r, 9 Cin)).view_as(W) through mdm_lora_up_add on the master viewed as
    [Cout, 9 Cin]; the bound of test_merge_unmerge_on_fp32_masters: 4 u max(|W0| + |s B A|), u = 2^-24"""
    from mdm_hip import ops

    g = _g(cout + r)
    w0 = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    a, b = torch.randn(r, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, torch.randn(cout, r, generator=g) * 0.05
    s = 0.5
    w, bd, atd = w0.to(DEV), b.to(DEV), a.reshape(r, -1).t().contiguous().to(DEV)
    ops.lora_up_add(w.view(cout, cin * 9), bd, atd, s)
    delta = s * (b.double() @ a.double().reshape(r, -1)).reshape(w0.shape)
    err = relerr(w, w0.double() + delta)
    ops.lora_up_add(w.view(cout, cin * 9), bd, atd, -s)
    back = float((w.cpu().double() - w0.double()).abs().max())
    bound = 4 * 2.0 ** -24 * float((w0.double().abs() + delta.abs()).max())
    print("[merge 3x3 %dx%d r=%d] merged %.3e, after unmerge %.3e (bound %.3e)" % (cout, cin, r, err, back, bound))
    assert err < 2e-5 and back <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,cin,cout,r", CC.AUTOGRAD_SHAPES)
def test_lora_conv_autograd_op(dtype, N, H, W, cin, cout, r):
    """ops.lora_conv adds into a base convolution's output in place; y, dX (base + low-rank part), dA, dB against torch's
    conv2d with the weight W + s B A"""
    from mdm_hip import ops

    g = _g(N + H + cin + r)
    s = 0.5
    x = q(torch.randn(N, H, W, cin, generator=g), dtype).double().requires_grad_()
    w = q(torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, dtype).double()
    a = q(torch.randn(r, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, dtype).double().requires_grad_()
    b = q(torch.randn(cout, r, generator=g) * 0.3, dtype).double().requires_grad_()
    gy = q(torch.randn(N, H, W, cout, generator=g), dtype)
    ref = CC.nhwc(F.conv2d(CC.nchw(x), w + s * (b @ a.reshape(r, -1)).reshape(w.shape), padding=1))
    (ref * gy.double()).sum().backward()
    xd = x.detach().to(dtype).to(DEV).requires_grad_()
    ad, bd = a.detach().float().to(DEV).requires_grad_(), b.detach().float().to(DEV).requires_grad_()
    y = ops.conv(xd, w.float().to(DEV), None)                           # the base convolution's fresh output
    out = ops.lora_conv(y, xd, ad, bd, s)
    assert out.data_ptr() == y.data_ptr()
    (out.float() * gy.to(DEV)).sum().backward()
    errs = dict(y=relerr(out.float(), ref), dx=relerr(xd.grad.float(), x.grad), dA=relerr(ad.grad, a.grad), dB=relerr(bd.grad, b.grad))
    print("[lora_conv op %s N=%d %dx%d %d->%d r=%d] %s" % (dtype, N, H, W, cin, cout, r, {k: "%.2e" % v for k, v in errs.items()}))
    assert ad.grad.dtype == torch.float32 and ad.grad.shape == a.shape and bd.grad.shape == b.shape
    assert all(v < TOL[dtype] for v in errs.values()), errs


# ---- model level --------------------------------------------------------------------------------------------------------
def _ctx(dtype):
    return torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else torch.autocast("cuda", enabled=False)


def _model(name):
    return PC.build_module(name)[0].to(DEV)


def _forward(model, name, dtype):
    inp = PC.inputs(name)
    x = [t.cuda() for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].cuda()
    with _ctx(dtype):
        return model(x, inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), {})


def _outs(model, name, dtype):
    with torch.no_grad():
        return [o.detach().float().cpu() for o in PC.as_list(_forward(model, name, dtype))]


def _attach(model, nonzero=True, **kw):
    from mdm_hip import lora

    args = dict(rank=RANK, alpha=ALPHA, seed=SEED, conv_targets=lora.CONV_TARGETS, conv_rank=CONV_RANK, conv_alpha=CONV_ALPHA)
    args.update(kw)
    ad = lora.attach(model, **args)
    if nonzero:
        LC.seeded_b(ad)
    return ad


def _hip_run(name, dtype):
    model = _model(name)
    ad = _attach(model)
    outs = _forward(model, name, dtype)
    PC.loss_of(outs, PC.inputs(name)["gys"]).backward()
    grads = {k: p.grad for k, p in ad.named_parameters()}
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape for p in ad.parameters())
    assert all(p.grad is None for p in model.parameters())                    # the base gets no gradient
    return [o.detach().float().cpu() for o in PC.as_list(outs)], grads


@functools.lru_cache(maxsize=None)
def _oracle(name, bf16=False):
    """the oracle on the merged state dict, computed once per case and shared (never modified by the tests)"""
    model = PC.build_module(name)[0]
    ad = _attach(model)
    return CC.oracle_lora_run(name, LC.adapter_values(ad), ad.scale, ad.conv_scale, torch.bfloat16 if bf16 else torch.float32)


@pytest.mark.parametrize("name", NAMES)
def test_model_fp32_matches_oracle_on_merged_weights(name):
    outs, grads = _hip_run(name, torch.float32)
    o_ref, g_ref = _oracle(name)
    fwd = [O.rel_l2(a, b) for a, b in zip(outs, o_ref)]
    errs, _ = PC.grad_errors(grads, g_ref)
    worst = max((e, k) for k, e in errs.items())
    worst_conv = max((e, k) for k, e in errs.items() if CC.is_conv_adapter(k))
    print("[lora+conv fp32 %s] forward rel-L2 %s, worst dA / dB rel-L2 %.3e (%s), worst conv adapter %.3e (%s)" % (
        name, ["%.3e" % e for e in fwd], worst[0], worst[1], worst_conv[0], worst_conv[1]))
    assert set(grads) == set(g_ref) and any(CC.is_conv_adapter(k) and g_ref[k].dim() == 4 for k in g_ref)
    assert all(e < 1e-4 for e in fwd) and worst[0] < 1e-3, (fwd, worst)


@pytest.mark.parametrize("name", NAMES)
def test_model_bf16_within_the_oracles_own_bf16_error(name):
    """product vs oracle-in-bf16, both against the fp32 oracle; the oracle-in-bf16 side is recorded in DESIGN.md section 4.9"""
    outs, grads = _hip_run(name, torch.bfloat16)
    o_ref, g_ref = _oracle(name)
    o_b, g_b = _oracle(name, True)
    fwd, fwd_bar = [O.rel_l2(a, b) for a, b in zip(outs, o_ref)], [O.rel_l2(a, b) for a, b in zip(o_b, o_ref)]
    agg, agg_bar = LC.agg_err(grads, g_ref), LC.agg_err(g_b, g_ref)
    worst, worst_bar = max(PC.grad_errors(grads, g_ref)[0].values()), max(PC.grad_errors(g_b, g_ref)[0].values())
    print("[lora+conv bf16 %s] forward rel-L2 %s (oracle in bf16: %s); dA / dB aggregate %.3e (%.3e), worst tensor %.3e (%.3e)" % (
        name, ["%.3e" % e for e in fwd], ["%.3e" % e for e in fwd_bar], agg, agg_bar, worst, worst_bar))
    assert all(e <= 1.5 * b for e, b in zip(fwd, fwd_bar)), (fwd, fwd_bar)
    assert agg <= 1.5 * agg_bar and worst <= 1.5 * worst_bar, (agg, agg_bar, worst, worst_bar)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_model_identities(name, dtype):
    model = _model(name)
    before = _outs(model, name, dtype)
    ad = _attach(model, nonzero=False)
    zero_b = _outs(model, name, dtype)
    assert all(torch.equal(a, b) for a, b in zip(zero_b, before))          # B = 0: bit for bit
    LC.seeded_b(ad)
    unmerged = _outs(model, name, dtype)
    assert max(O.rel_l2(a, b) for a, b in zip(unmerged, before)) > 1e-4       # the adapters act
    ad.merge()
    assert ad.merged
    merged = _outs(model, name, dtype)
    ad.unmerge()
    again = _outs(model, name, dtype)
    ad.detach()
    after = _outs(model, name, dtype)
    e_merge = max(relerr(a, b) for a, b in zip(merged, unmerged))
    e_again = max(relerr(a, b) for a, b in zip(again, unmerged))
    print("[lora+conv identities %s %s] merged vs unmerged %.3e, unmerged again %.3e" % (name, dtype, e_merge, e_again))
    assert e_merge < TOL[dtype] and e_again < TOL[dtype]
    # detach(): the unadapted outputs, within the rounding of W + d - d on the masters
    e_after = max(relerr(a, b) for a, b in zip(after, before))
    assert e_after < (2e-5 if dtype == torch.float32 else TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_detach_without_merge_restores_the_outputs_bit_for_bit(name, dtype):
    model = _model(name)
    before = _outs(model, name, dtype)
    ad = _attach(model)
    assert max(O.rel_l2(a, b) for a, b in zip(_outs(model, name, dtype), before)) > 1e-4
    ad.detach()
    assert all(torch.equal(a, b) for a, b in zip(_outs(model, name, dtype), before))


def test_conv_only_attach_trains_the_outer_net_of_a_nested_model():
    """targets=(): no attention adapter at all; the outer net (names not under inner_unet.) gets non-zero gradients"""
    name = "mini_nested"
    model = _model(name)
    ad = _attach(model, targets=())
    assert not any(t in k for k, _ in ad.named_parameters() for t in LC.TARGETS)
    PC.loss_of(_forward(model, name, torch.float32), PC.inputs(name)["gys"]).backward()
    outer = {k: p for k, p in ad.named_parameters() if not k.startswith("inner_unet.")}
    assert outer and any(p.dim() == 4 for p in outer.values())
    norms = {k: float(p.grad.abs().max()) for k, p in outer.items()}
    print("[lora conv-only mini_nested] outer-net adapter tensors %d, smallest max |grad| %.3e" % (len(outer), min(norms.values())))
    assert all(v > 0 for v in norms.values()), norms
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in ad.parameters())
    assert all(p.grad is None for p in model.parameters())
    # against the oracle on the merged state dict, conv adapters only
    o_ref, g_ref = CC.oracle_lora_run(name, LC.adapter_values(ad), ad.scale, ad.conv_scale)
    worst = max(PC.grad_errors({k: p.grad for k, p in ad.named_parameters()}, g_ref)[0].values())
    print("[lora conv-only mini_nested] worst dA / dB rel-L2 %.3e" % worst)
    assert worst < 1e-3


def _pipe(name, model):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(model, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                use_double_loss=True, no_use_residual=True)).to(torch.device(DEV))
    return D.Diffusion(model, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False)).to(torch.device(DEV))


@pytest.mark.parametrize("fp16", [False, True])
def test_train_batch_moves_the_conv_adapters_and_not_the_base(fp16):
    from mdm_hip import ops, trainer

    ops.set_grad_sink(None)
    model = PC.build_module("mini_unet")[0]
    pipe = _pipe("mini_unet", model)
    vm = pipe.model.vision_model
    ad = _attach(vm)
    base0 = {k: p.detach().clone() for k, p in vm.named_parameters()}
    ad0 = {k: p.detach().clone() for k, p in ad.named_parameters()}
    opt = torch.optim.AdamW(ad.parameters(), lr=1e-2, weight_decay=0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
    args = types.SimpleNamespace(fp16=fp16, gradient_clip_norm=0.05)
    inp = PC.inputs("mini_unet")
    g = _g(29)
    sample = {"lm_outputs": inp["cond"].cuda(), "lm_mask": inp["mask"].cuda(), "images": (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).cuda()}
    vals = []
    for i in range(3):
        torch.manual_seed(100 + i)
        vals.append(trainer.train_batch(pipe, sample, opt, sched, None, args)[0])
    torch.cuda.synchronize()
    print("[lora+conv train fp16=%s] losses %s, path: %s" % (fp16, vals, opt._mdm_fused_reason))
    assert opt._mdm_fused is False and opt._mdm_fused_reason == "vision model has no trainable parameters"
    assert all(torch.isfinite(torch.tensor(v)) for v in vals)
    assert all(torch.equal(p.detach(), base0[k]) for k, p in vm.named_parameters())          # bit-identical base
    moved = {k: not torch.equal(p.detach(), ad0[k]) for k, p in ad.named_parameters()}
    assert any(CC.is_conv_adapter(k) for k in moved) and all(moved.values()), [k for k, v in moved.items() if not v]


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_graphed_sampling_follows_attach_and_merge(name):
    from mdm_hip.graph import GraphedSampler

    model = PC.build_module(name)[0]
    pipe = _pipe(name, model)
    pipe.eval()
    vm = pipe.model.vision_model
    inp = PC.inputs(name)
    cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
    smp = {"lm_outputs": cond, "lm_mask": mask}
    side = 32 if name == "mini_nested" else 16
    g = _g(41)
    start = [torch.randn(2, 3, side, side, generator=g).cuda()]
    if name == "mini_nested":
        start.append(torch.randn(2, 3, side // 2, side // 2, generator=g).cuda())
    n = 4

    def eager():
        x0 = [t.clone() for t in start]
        return pipe.sampler.sample(pipe.get_model(), x0 if name == "mini_nested" else x0[0], cond, mask, {}, resample_steps=True,
                                   num_inference_steps=n, ddim_eta=0)

    def graphed(gs):
        return gs.sample(2, smp, side, torch.device(DEV), num_inference_steps=n, start_noise=start, ddim_eta=0)

    with torch.no_grad():
        gs = GraphedSampler(pipe, seed=1)
        plain = graphed(gs)                                   # captured BEFORE attach
        assert O.rel_l2(plain, eager()) < 1e-6
        ad = _attach(vm, targets=())                          # conv adapters only: every change below is theirs
        e_un = eager()
        assert O.rel_l2(e_un, plain) > 1e-3                   # the adapters change the images
        g_un = graphed(gs)                                    # the stale graph is not replayed: captured anew
        assert O.rel_l2(g_un, e_un) < 1e-6 and len(gs._graphs) == 1
        assert O.rel_l2(graphed(gs), e_un) < 1e-6 and len(gs._graphs) == 1       # ... and that one replays
        ad.merge()
        e_m = eager()
        assert relerr(e_m, e_un) < 1e-3                       # merged weights sample the same images (fp32 round-off over 4 steps)
        assert O.rel_l2(graphed(gs), e_m) < 1e-6 and len(gs._graphs) == 1       # a graph captured before merge() is refreshed
        fresh = GraphedSampler(pipe, seed=1)
        assert O.rel_l2(graphed(fresh), e_m) < 1e-6
        ad.unmerge()
        ad.detach()
        assert O.rel_l2(graphed(gs), plain) < 1e-4 and len(gs._graphs) == 1
