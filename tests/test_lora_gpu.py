"""GPU: the LoRA kernels (csrc/lora.hip) against fp64 restatements, the autograd op against torch, and the model with
adapters against the oracle run on the merged state dict (tests/lora_cases.py) -- plus the identities that make the
feature safe to use: B = 0 changes nothing, merged == unmerged, detach restores, the base stays frozen, the trainer's
plain path trains the adapters only, and graphed sampling follows attach / merge.

Op gates are those of tests/test_ops_gpu.py (max-abs error over the largest reference magnitude: 2e-5 fp32, 3e-2 bf16,
inputs rounded through the dtype on both sides); model gates those of DESIGN.md section 3 (rel-L2 1e-4 outputs, 1e-3
gradients in fp32).  Measured values are printed (pytest -s).

bf16 model gate: the oracle's OWN error when it is run with bf16 tensors on the CPU (computed here; independent code),
times 1.5 -- the oracle rounds at other places than the fused epilogues do.
"""
import functools
import types

import pytest
import torch

import lora_cases as LC
import parity_cases as PC
import unet_oracle as O
from lora_cases import TOL, q, relerr

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
DEV = "cuda:0"
RANK, ALPHA, SEED = 8, 4, 3


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,r", LC.DOWN_SHAPES)
def test_lora_down(dtype, M, C, r):
    from mdm_hip import ops

    g = _g(M + C + r)
    x, a = q(torch.randn(M, C, generator=g), dtype), q(torch.randn(r, C, generator=g) / C ** 0.5, dtype)
    t = ops.lora_down(x.to(dtype).to(DEV), a.to(dtype).to(DEV))
    assert t.shape == (M, r) and t.dtype == dtype
    err = relerr(t.float(), LC.down_ref(x, a))
    print("[lora_down %s M=%d C=%d r=%d] %.3e" % (dtype, M, C, r, err))
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [0.5, 2.0])
@pytest.mark.parametrize("M,N,r", LC.UP_SHAPES)
def test_lora_up_add(dtype, M, N, r, s):
    from mdm_hip import ops

    g = _g(M + N + r)
    y, t = q(torch.randn(M, N, generator=g) + 0.3, dtype), q(torch.randn(M, r, generator=g), dtype)
    b = q(torch.randn(N, r, generator=g) / r ** 0.5, dtype)
    yd, td, bd = y.to(dtype).to(DEV), t.to(dtype).to(DEV), b.to(dtype).to(DEV)
    out = ops.lora_up_add(yd, td, bd, s)
    assert out.data_ptr() == yd.data_ptr()                      # in place
    err = relerr(out.float(), LC.up_add_ref(y, t, b, s))
    print("[lora_up_add %s M=%d N=%d r=%d s=%g] %.3e" % (dtype, M, N, r, s, err))
    assert err < TOL[dtype]
    # accumulate = 0 overwrites without reading y (the backward's dX): NaNs in the destination do not come through
    fresh = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
    ops.lora_up_add(fresh, td, bd, s, accumulate=False)
    assert relerr(fresh.float(), LC.up_add_ref(torch.zeros(M, N), t, b, s)) < TOL[dtype]
    # B = 0 leaves y bit-identical
    y0 = y.to(dtype).to(DEV)
    ops.lora_up_add(y0, td, torch.zeros_like(bd), s)
    assert torch.equal(y0, y.to(dtype).to(DEV))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,r", LC.WGRAD_SHAPES)
def test_lora_wgrad(dtype, M, C, r):
    from mdm_hip import ops

    g = _g(M + C + r + 1)
    p, qq = q(torch.randn(M, r, generator=g), dtype), q(torch.randn(M, C, generator=g), dtype)
    pd, qd = p.to(dtype).to(DEV), qq.to(dtype).to(DEV)
    s = 0.5
    ref = LC.wgrad_ref(p, qq, s)
    d = ops.lora_wgrad(pd, qd, s)
    assert d.shape == (r, C) and d.dtype == torch.float32
    err = relerr(d, ref)
    print("[lora_wgrad %s M=%d C=%d r=%d] %.3e" % (dtype, M, C, r, err))
    assert err < TOL[dtype]
    assert torch.equal(d, ops.lora_wgrad(pd, qd, s))            # deterministic: two runs are bit-identical
    base = torch.randn(r, C, generator=g)
    acc = base.to(DEV)
    ops.lora_wgrad(pd, qd, s, out=acc)                          # accumulate = 1
    assert relerr(acc, base.double() + ref) < TOL[dtype]


@pytest.mark.parametrize("cout,cin,r", LC.MERGE_SHAPES)
def test_merge_unmerge_on_fp32_masters(cout, cin, r):
    """W += s B A through mdm_lora_up_add (t = B, b = A^T) against fp64; W -= s B A afterwards returns to W0 within two
    roundings of the merged magnitude: |W2 - W0| <= |W0 + d| u + |W0| u with u = 2^-24, gated at 4 u max(|W0| + |s B A|)"""
    from mdm_hip import ops

    g = _g(cout + r)
    w0 = torch.randn(cout, cin, generator=g) / cin ** 0.5
    a, b = torch.randn(r, cin, generator=g) / cin ** 0.5, torch.randn(cout, r, generator=g) * 0.05
    s = 0.5
    w, bd, atd = w0.to(DEV), b.to(DEV), a.t().contiguous().to(DEV)
    ops.lora_up_add(w, bd, atd, s)
    delta = s * (b.double() @ a.double())
    err = relerr(w, w0.double() + delta)
    ops.lora_up_add(w, bd, atd, -s)
    back = float((w.cpu().double() - w0.double()).abs().max())
    bound = 4 * 2.0 ** -24 * float((w0.double().abs() + delta.abs()).max())
    print("[merge %dx%d r=%d] merged %.3e, after unmerge %.3e (bound %.3e)" % (cout, cin, r, err, back, bound))
    assert err < 2e-5 and back <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,cin,cout,r", LC.AUTOGRAD_SHAPES)
def test_lora_autograd_op(dtype, M, cin, cout, r):
    """ops.lora adds into a base projection's output in place; dX (base + low-rank part), dA, dB against torch fp32"""
    from mdm_hip import ops

    g = _g(M + r)
    s = 0.5
    x = q(torch.randn(M, cin, generator=g), dtype).requires_grad_()
    w = q(torch.randn(cout, cin, generator=g) / cin ** 0.5, dtype)
    a = q(torch.randn(r, cin, generator=g) / cin ** 0.5, dtype).requires_grad_()
    b = q(torch.randn(cout, r, generator=g) * 0.3, dtype).requires_grad_()
    gy = q(torch.randn(M, cout, generator=g), dtype)
    ref = x @ w.t() + s * (x @ a.t()) @ b.t()
    (ref * gy).sum().backward()
    xd = x.detach().to(dtype).to(DEV).requires_grad_()
    ad, bd = a.detach().to(DEV).requires_grad_(), b.detach().to(DEV).requires_grad_()
    y = xd @ w.to(dtype).to(DEV).t()                          # a fresh non-leaf output, as a convolution's is
    out = ops.lora(y, xd, ad, bd, s)
    assert out.data_ptr() == y.data_ptr()
    (out.float() * gy.to(DEV)).sum().backward()
    errs = dict(y=relerr(out.float(), ref), dx=relerr(xd.grad.float(), x.grad), dA=relerr(ad.grad, a.grad), dB=relerr(bd.grad, b.grad))
    print("[lora op %s M=%d %d->%d r=%d] %s" % (dtype, M, cin, cout, r, {k: "%.2e" % v for k, v in errs.items()}))
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


def _attach(model, nonzero=True):
    from mdm_hip import lora

    ad = lora.attach(model, rank=RANK, alpha=ALPHA, seed=SEED)
    if nonzero:
        LC.seeded_b(ad)
    return ad


def _hip_run(name, dtype):
    model = _model(name)
    ad = _attach(model)
    outs = _forward(model, name, dtype)
    PC.loss_of(outs, PC.inputs(name)["gys"]).backward()
    grads = {k: p.grad for k, p in ad.named_parameters()}
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values())
    return [o.detach().float().cpu() for o in PC.as_list(outs)], grads, model


@functools.lru_cache(maxsize=None)
def _oracle(name, bf16=False):
    """the oracle on the merged state dict, computed once per case and shared (never modified by the tests)"""
    model = PC.build_module(name)[0]
    ad = _attach(model)
    return LC.oracle_lora_run(name, LC.adapter_values(ad), ad.scale, torch.bfloat16 if bf16 else torch.float32)


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_model_fp32_matches_oracle_on_merged_weights(name):
    outs, grads, _ = _hip_run(name, torch.float32)
    o_ref, g_ref = _oracle(name)
    fwd = [O.rel_l2(a, b) for a, b in zip(outs, o_ref)]
    errs, _ = PC.grad_errors(grads, g_ref)
    worst = max((e, k) for k, e in errs.items())
    print("[lora fp32 %s] forward rel-L2 %s, worst dA / dB rel-L2 %.3e (%s)" % (name, ["%.3e" % e for e in fwd], worst[0], worst[1]))
    assert set(grads) == set(g_ref) and all(e < 1e-4 for e in fwd) and worst[0] < 1e-3, (fwd, worst)


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_model_bf16_within_the_oracles_own_bf16_error(name):
    """Measured on an MI355X (product vs oracle-in-bf16, both against the fp32 oracle): see DESIGN.md section 4.9."""
    outs, grads, _ = _hip_run(name, torch.bfloat16)
    o_ref, g_ref = _oracle(name)
    o_b, g_b = _oracle(name, True)
    fwd, fwd_bar = [O.rel_l2(a, b) for a, b in zip(outs, o_ref)], [O.rel_l2(a, b) for a, b in zip(o_b, o_ref)]
    agg, agg_bar = LC.agg_err(grads, g_ref), LC.agg_err(g_b, g_ref)
    worst, worst_bar = max(PC.grad_errors(grads, g_ref)[0].values()), max(PC.grad_errors(g_b, g_ref)[0].values())
    print("[lora bf16 %s] forward rel-L2 %s (oracle in bf16: %s); dA / dB aggregate %.3e (%.3e), worst tensor %.3e (%.3e)" % (
        name, ["%.3e" % e for e in fwd], ["%.3e" % e for e in fwd_bar], agg, agg_bar, worst, worst_bar))
    assert all(e <= 1.5 * b for e, b in zip(fwd, fwd_bar)), (fwd, fwd_bar)
    assert agg <= 1.5 * agg_bar and worst <= 1.5 * worst_bar, (agg, agg_bar, worst, worst_bar)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
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
    e_after = max(relerr(a, b) for a, b in zip(after, before))
    print("[lora identities %s %s] merged vs unmerged %.3e, unmerged again %.3e, detached vs before %.3e" % (name, dtype, e_merge, e_again, e_after))
    assert e_merge < TOL[dtype] and e_again < TOL[dtype]
    assert e_after < (2e-5 if dtype == torch.float32 else TOL[dtype])


def test_frozen_base_gets_no_gradient_and_ffn_launches_no_weight_gradient(monkeypatch):
    from mdm_hip import ops

    calls = {"launch": 0, "sink": 0}
    real_launch, real_sink = ops._wgrad_launch, ops._wgrad_into_sink

    def launch(*a, **k):
        calls["launch"] += 1
        return real_launch(*a, **k)

    def sink(*a, **k):
        calls["sink"] += 1
        return real_sink(*a, **k)

    monkeypatch.setattr(ops, "_wgrad_launch", launch)
    monkeypatch.setattr(ops, "_wgrad_into_sink", sink)
    ops.set_grad_sink(None)
    name = "mini_unet"
    model = _model(name)
    assert any(m.ffn is not None for m in model.modules() if hasattr(m, "ffn")), "the case must have FFN layers"
    PC.loss_of(_forward(model, name, torch.float32), PC.inputs(name)["gys"]).backward()
    trainable = dict(calls)
    assert trainable["launch"] > 0
    model.zero_grad(set_to_none=True)
    ad = _attach(model)
    calls.update(launch=0, sink=0)
    PC.loss_of(_forward(model, name, torch.float32), PC.inputs(name)["gys"]).backward()
    torch.cuda.synchronize()
    print("[lora frozen base] weight-gradient launches: trainable %s, frozen + adapters %s" % (trainable, calls))
    assert calls == {"launch": 0, "sink": 0}              # convolutions, linears and FFN layers alike
    assert all(p.grad is None for p in model.parameters())
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in ad.parameters())


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
def test_train_batch_trains_the_adapters_only(fp16):
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
    # the clipped norm of the first step against torch's over the adapter gradients of the same step (same seed)
    torch.manual_seed(100)
    pipe.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=fp16):
        losses, _, _, _, _, weights = pipe.get_loss(sample)
        trainer._loss_of(losses, weights).backward()
    norm_ref = float(torch.nn.utils.clip_grad_norm_(list(ad.parameters()), 1e9))
    assert all(p.grad is None for p in vm.parameters())
    opt.zero_grad()
    vals = []
    for i in range(3):
        torch.manual_seed(100 + i)
        vals.append(trainer.train_batch(pipe, sample, opt, sched, None, args)[0])
        if i == 0:
            norm = float(opt._mdm_grad_norm)
    torch.cuda.synchronize()
    print("[lora train fp16=%s] losses %s, clipped norm %.6e (torch over the adapter gradients: %.6e), path: %s" % (
        fp16, vals, norm, norm_ref, opt._mdm_fused_reason))
    assert opt._mdm_fused is False and opt._mdm_fused_reason == "vision model has no trainable parameters"
    assert all(torch.isfinite(torch.tensor(v)) for v in vals)
    assert abs(norm - norm_ref) <= 1e-5 * norm_ref
    assert all(torch.equal(p.detach(), base0[k]) for k, p in vm.named_parameters())          # bit-identical base
    assert all(not torch.equal(p.detach(), ad0[k]) for k, p in ad.named_parameters())        # every adapter tensor moved


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
        ad = _attach(vm)
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
