"""GPU: activation recomputation for the ResNet blocks (``ops.enable_activation_recompute``).
  * kernel: ``mdm_gn_reapply`` against ``mdm_gn_fwd`` (both of its kernel families, tests/recompute_cases.py), and with
    dropout against ``mdm_dropout(mdm_gn_fwd(...))`` -- 0 differing elements;
  * function: ``ops.gn_conv`` against the composed stored path group_norm -> dropout -> conv with pass-through outputs,
    FiLM and a residual -- the output and every gradient equal in every bit (after the stored path has been shown to repeat
    itself bit for bit on the case);
  * model: the mini U-Net and the mini nested model with the switch on meet the gates of tests/test_model_gpu.py (that
    module's own tests are called under the switch: no gate is restated here) and equal the switch-off run bit for bit, with
    dropout (and the same dropout counter afterwards), with conv LoRA adapters (the stored-path fallback), through
    ``trainer.train_batch`` on both of its paths in fp32 and bf16 (and once with the deferred 1x1 weight-gradient queue
    active); and the forward holds at least the analytic bytes of every recomputed activation less.
Exactness rests on N = 2: dgamma / dbeta are summed over samples with atomics, and a two-term sum has one order.  The one
larger case runs where those sums are per-sample rows reduced in a fixed order, and first shows that the stored path repeats."""
import gc
import types

import pytest
import torch

import parity_cases as PC
import recompute_cases as RC
from recompute_cases import count_gn_conv, ndiff, recompute

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
SEED, OFF = 0x1234567887654321, 977   # a dropout triple with high seed bits and a counter that is no multiple of anything


# ---- kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", RC.KERNEL_CASES, ids=lambda c: "N%d_%dx%d_C%d_G%d" % c[:5])
def test_reapply_equals_gn_fwd_in_every_bit(case, dtype):
    from mdm_hip import ops

    N, H, W, C, G, fam16, fam32 = case
    fam = fam32 if dtype == torch.float32 else fam16
    assert RC.family(H * W, C, G, dtype) == fam
    for act in (0, 1):
        for film in (False, True):
            x, gamma, beta, fl = [t if t is None else t.to(DEV) for t in RC.kernel_inputs(N, H, W, C, G, dtype, film, seed=act)]
            y, coef = RC.gn_fwd_raw(x, gamma, beta, fl, G, act)
            z = ops.gn_reapply(x, coef, silu=bool(act))
            n = ndiff(z, y)
            print("[gn_reapply %s %s family=%s act=%d film=%d] differing elements: %d of %d" % (
                dtype, case[:5], fam, act, film, n, y.numel()))
            assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0
            assert n == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", RC.DROPOUT_CASES, ids=lambda c: "N%d_%dx%d_C%d_G%d" % c[:5])
def test_reapply_with_dropout_equals_dropout_of_gn_fwd(case, dtype):
    from mdm_hip import ops

    N, H, W, C, G = case[:5]
    p = RC.DROPOUT_P
    for act, film in ((1, True), (1, False), (0, True)):
        x, gamma, beta, fl = [t if t is None else t.to(DEV) for t in RC.kernel_inputs(N, H, W, C, G, dtype, film, seed=2 + act)]
        y, coef = RC.gn_fwd_raw(x, gamma, beta, fl, G, act)
        yd = RC.dropout_raw(y, p, SEED, OFF)
        z = ops.gn_reapply(x, coef, silu=bool(act), p=p, seed=SEED, offset=OFF)
        n = ndiff(z, yd)
        dropped = float((yd == 0).float().mean())
        print("[gn_reapply+dropout %s %s act=%d film=%d] differing elements: %d of %d (dropped %.3f)" % (
            dtype, case[:5], act, film, n, y.numel(), dropped))
        assert 0.02 < dropped < 0.25      # the mask is there (p = 0.1) ...
        assert ndiff(yd, y) > 0           # ... and changes the tensor
        assert n == 0


def test_gn_reapply_rejects_a_malformed_coef():
    """[N, C, 2] fp32 on x's device, or MdmHipError: the kernel would read a wrong one out of bounds"""
    from mdm_hip import _lib, ops

    x = torch.randn(2, 4, 4, 32, device=DEV)
    for bad in (torch.zeros(2, 32, device=DEV), torch.zeros(2, 16, 2, device=DEV), torch.zeros(1, 32, 2, device=DEV),
                torch.zeros(2, 32, 2, device=DEV, dtype=torch.bfloat16), torch.zeros(2, 32, 2)):
        with pytest.raises(_lib.MdmHipError, match="coef must be"):
            ops.gn_reapply(x, bad)
    # a non-contiguous view of the right shape is made contiguous, not misread
    base = torch.randn(2, 32, 4, device=DEV)
    view = base[:, :, ::2]
    assert not view.is_contiguous()
    assert ndiff(ops.gn_reapply(x, view), ops.gn_reapply(x, view.contiguous())) == 0


# ---- function -----------------------------------------------------------------------------------------------------------
def _function_run(fused, H, W, cin, cout, G, dtype, p, passthrough, res_kind):
    """one forward + backward of norm(+FiLM)+SiLU -> dropout -> 3x3 conv (+bias, +residual) -> (outputs, gradients)"""
    from mdm_hip import ops

    g = RC.gen(H * 100 + W * 10 + cin + cout + G)
    N = 2
    x = (torch.randn(N, H, W, cin, generator=g) + 0.2).to(dtype).to(DEV).requires_grad_()
    gamma = (torch.randn(cin, generator=g) * 0.3 + 1).to(DEV).requires_grad_()
    beta = (torch.randn(cin, generator=g) * 0.3).to(DEV).requires_grad_()
    film = (torch.randn(N, 2 * cin, generator=g) * 0.3).to(dtype).to(DEV).requires_grad_()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV).requires_grad_()
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV).requires_grad_()
    res = (torch.randn(N, H, W, cout, generator=g)).to(dtype).to(DEV).requires_grad_() if res_kind == "tensor" else None
    gy = torch.randn(N, H, W, cout, generator=g).to(DEV)
    g1, g2 = torch.randn(N, H, W, cin, generator=g).to(DEV), torch.randn(N, H, W, cin, generator=g).to(DEV)
    ops.set_dropout_rng_state((SEED, OFF))
    if fused:
        out = ops.gn_conv(x, gamma, beta, G, w, b, film=film, passthrough=passthrough, p=p, residual=res)
    else:
        out = ops.group_norm(x, gamma, beta, G, film=film, silu=True, passthrough=passthrough)
        out = list(out) if passthrough else [out]
        out[0] = ops.conv(ops.dropout(out[0], p, True), w, b, residual=res)
    out = list(out) if isinstance(out, (tuple, list)) else [out]
    loss = (out[0].float() * gy).sum()
    if passthrough:
        loss = loss + (out[1].float() * g1).sum()
    if passthrough == 2:
        loss = loss + (out[2].float() * g2).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {"dx": x.grad, "dW": w.grad, "db": b.grad, "dfilm": film.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    if res is not None:
        grads["dres"] = res.grad
    assert all(v is not None for v in grads.values()), [k for k, v in grads.items() if v is None]
    return out[0].detach(), grads, ops.get_dropout_rng_state()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, RC.DROPOUT_P])
@pytest.mark.parametrize("case", RC.FUNCTION_CASES, ids=lambda c: "%dx%d_%dto%d_G%d" % c)
def test_gn_conv_equals_the_stored_path_in_every_bit(case, p, dtype):
    H, W, cin, cout, G = case
    for passthrough, res_kind in ((2, "tensor"), (1, "tensor"), (0, None)):
        a = _function_run(False, H, W, cin, cout, G, dtype, p, passthrough, res_kind)
        a2 = _function_run(False, H, W, cin, cout, G, dtype, p, passthrough, res_kind)
        # precondition: the stored path repeats itself bit for bit on this case
        assert ndiff(a[0], a2[0]) == 0 and all(ndiff(a[1][k], a2[1][k]) == 0 for k in a[1]), "the stored path is not deterministic here"
        f = _function_run(True, H, W, cin, cout, G, dtype, p, passthrough, res_kind)
        diffs = {"y": ndiff(f[0], a[0])}
        diffs.update({k: ndiff(f[1][k], a[1][k]) for k in a[1]})
        print("[gn_conv %s %s p=%g passthrough=%d] differing elements %s" % (dtype, case, p, passthrough, diffs))
        assert all(float(v.float().abs().max()) > 0 for v in a[1].values())
        assert all(v == 0 for v in diffs.values()), diffs
        assert f[2] == a[2]   # the dropout counter moved once, in forward, by the same amount


def test_gn_conv_with_a_frozen_weight_needs_no_reapply():
    """needs_input_grad as ConvFn honours it: a frozen weight skips the weight gradient, and then nothing reads h"""
    from mdm_hip import ops

    g = RC.gen(5)
    x = torch.randn(2, 8, 8, 32, generator=g).to(DEV).requires_grad_()
    gamma, beta = torch.ones(32, device=DEV), torch.zeros(32, device=DEV)
    w = (torch.randn(32, 32, 3, 3, generator=g) / 17).to(DEV)
    b = torch.zeros(32, device=DEV)
    calls = []
    orig = ops.gn_reapply
    ops.gn_reapply = lambda *a, **kw: calls.append(1) or orig(*a, **kw)
    try:
        res = []
        for fused in (False, True):
            xx = x.detach().clone().requires_grad_()
            y = ops.gn_conv(xx, gamma, beta, 8, w, b) if fused else ops.conv(ops.group_norm(xx, gamma, beta, 8, silu=True), w, b)
            y.float().square().sum().backward()
            res.append((y.detach(), xx.grad))
        assert calls == []
        assert ndiff(res[0][0], res[1][0]) == 0 and ndiff(res[0][1], res[1][1]) == 0
        w.requires_grad_()
        ops.gn_conv(x, gamma, beta, 8, w, b).float().square().sum().backward()
        assert calls == [1] and w.grad is not None
    finally:
        ops.gn_reapply = orig


# ---- model --------------------------------------------------------------------------------------------------------------
MODELS = ["mini_unet", "mini_nested"]


def _resnets(model):
    from mdm_hip.unet import ResNet

    return [m for m in model.modules() if isinstance(m, ResNet)]


def _set_dropout(model, p):
    import copy

    for m in _resnets(model):
        m.config = copy.copy(m.config)
        m.config.dropout = p


def _model_run(name, dtype, on, dropout=0.0, adapters=None):
    """one forward + backward of a mini model -> (outputs, gradients, dropout counter, gn_conv calls)"""
    from mdm_hip import lora, ops

    model = PC.build_module(name)[0].to(DEV)
    if dropout:
        _set_dropout(model, dropout)
    ad = None
    if adapters is not None:
        ad = lora.attach(model, rank=8, alpha=4, seed=3, conv_targets=adapters, conv_rank=4, conv_alpha=2)
        import lora_cases as LC
        LC.seeded_b(ad)
    inp = PC.inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    ops.set_dropout_rng_state((SEED, 0))
    with recompute(on), count_gn_conv() as cnt, torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
        PC.loss_of(outs, inp["gys"]).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in (ad if ad is not None else model).named_parameters()}
    assert all(v is not None for v in grads.values())
    return [o.detach() for o in PC.as_list(outs)], grads, ops.get_dropout_rng_state(), cnt.calls


def _assert_same(a, b, what):
    bad = [i for i, (u, v) in enumerate(zip(a[0], b[0])) if ndiff(u, v)]
    assert not bad, (what, "outputs", bad)
    bad = [k for k in a[1] if ndiff(a[1][k], b[1][k])]
    assert not bad, (what, "gradients", bad[:8], len(bad))


@pytest.mark.parametrize("name", MODELS)
def test_switch_on_meets_the_model_gates(name):
    """the gates and goldens of tests/test_model_gpu.py, by running its own tests with the switch on"""
    import test_model_gpu as TM

    with recompute(True), count_gn_conv() as cnt:
        TM.test_fp32_matches_oracle_and_golden(name)
        n32 = cnt.calls
        TM.test_bf16_close_to_oracle(name)
    print("[recompute gates %s] gn_conv calls: fp32 %d, bf16 %d" % (name, n32, cnt.calls - n32))
    assert n32 > 0 and cnt.calls == 2 * n32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", MODELS)
def test_switch_on_equals_switch_off_in_every_bit(name, dtype):
    off = _model_run(name, dtype, False)
    on = _model_run(name, dtype, True)
    assert off[3] == 0 and on[3] == 2 * len(_resnets(PC.build_module(name)[0]))   # every conv1 and conv2 took the fused path
    _assert_same(on, off, (name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", MODELS)
def test_dropout_is_replayed_and_its_counter_moves_once(name, dtype):
    from mdm_hip import ops

    plain = _model_run(name, dtype, False)
    off = _model_run(name, dtype, False, dropout=0.1)
    on = _model_run(name, dtype, True, dropout=0.1)
    assert any(ndiff(u, v) for u, v in zip(off[0], plain[0]))   # the dropout acts
    assert on[3] > 0
    _assert_same(on, off, (name, dtype, "dropout"))
    assert on[2] == off[2] and on[2][0] == SEED and on[2][1] > 0
    ops.seed_dropout(torch.initial_seed())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("targets,fused_calls_per_block", [(("conv1", "conv2", "conv3"), 0), (("conv1",), 1)])
@pytest.mark.parametrize("name", MODELS)
def test_unmerged_conv_adapters_keep_the_stored_path(name, targets, fused_calls_per_block, dtype):
    """adapted convolutions fall back (their adapter's backward reads h); an unadapted conv2 beside an adapted conv1 still
    takes the fused path -- with the base frozen, so nothing re-applies h at all.  The nested model's outer net is ResNet
    convolutions only: conv adapters are all it can have."""
    off = _model_run(name, dtype, False, adapters=targets)
    on = _model_run(name, dtype, True, adapters=targets)
    assert on[3] == fused_calls_per_block * len(_resnets(PC.build_module(name)[0]))
    assert all(float(v.abs().max()) > 0 for v in off[1].values())
    _assert_same(on, off, (name, dtype, targets))


def _train_pipe(name):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    model = PC.build_module(name)[0]
    if nested:
        pipe = D.NestedDiffusion(model, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                use_double_loss=True, no_use_residual=True))
    else:
        pipe = D.Diffusion(model, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
    return pipe.to(torch.device(DEV))


def _train_steps(name, mode, fp16, on, batch=2, steps=2):
    """``steps`` optimizer steps of trainer.train_batch on a fresh pipeline -> (losses, parameters, Adam first moments,
    gn_conv calls, queued 1x1 weight gradients); mode: "fused" (gradient sink, side-stream and deferred weight gradients) |
    "plain" (autograd accumulation, torch optimizer)"""
    from mdm_hip import ops, trainer

    ops.set_grad_sink(None)
    pipe = _train_pipe(name)
    vm = pipe.model.vision_model
    opt = torch.optim.AdamW(vm.parameters(), lr=1e-3, weight_decay=0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
    ema = trainer.ModelEma(vm, decay=0.9, warmup_steps=1)
    if mode == "plain":
        opt._mdm_fused = False
    args = types.SimpleNamespace(fp16=fp16, gradient_clip_norm=0.5)
    inp = PC.inputs(name)
    reps = batch // 2
    side = 32 if name == "mini_nested" else 16
    g = RC.gen(29)
    sample = {"lm_outputs": inp["cond"].repeat(reps, 1, 1).to(DEV), "lm_mask": inp["mask"].repeat(reps, 1).to(DEV),
              "images": (torch.rand(batch, 3, side, side, generator=g) * 2 - 1).to(DEV)}
    queued, orig_q = [0], ops._queue_wgrad

    def counting(*a, **kw):
        queued[0] += 1
        return orig_q(*a, **kw)

    ops._queue_wgrad = counting
    losses = []
    try:
        with recompute(on), count_gn_conv() as cnt:
            for i in range(steps):
                torch.manual_seed(100 + i)   # the timesteps and the noise of the step
                losses.append(float(trainer.train_batch(pipe, sample, opt, sched, None, args, ema_model=ema)[0]))
        torch.cuda.synchronize()
        fused = getattr(opt, "_mdm_fused", None)
        assert (fused not in (None, False)) == (mode == "fused"), getattr(opt, "_mdm_fused_reason", None)
        params = {k: v.detach().float().cpu().clone() for k, v in vm.named_parameters()}
        moments = {k: opt.state[v]["exp_avg"].detach().float().cpu().clone() for k, v in vm.named_parameters()}
    finally:
        ops._queue_wgrad = orig_q
        ops.set_grad_sink(None)
        ops.enable_async_wgrad(False)
        ops.enable_deferred_wgrad(False)
    return losses, params, moments, cnt.calls, queued[0]


def _assert_same_training(on, off, what):
    assert off[3] == 0 and on[3] > 0, what
    assert on[0] == off[0], (what, on[0], off[0])
    for which, a, b in (("parameters", on[1], off[1]), ("moments", on[2], off[2])):
        bad = [k for k in b if ndiff(a[k], b[k])]
        assert not bad, (what, which, bad[:8], len(bad))


@pytest.mark.parametrize("mode", ["fused", "plain"])
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_train_batch_is_unchanged_by_the_switch(name, fp16, mode):
    """two optimizer steps of trainer.train_batch -- the fused path with the gradient sink and the side-stream weight
    gradients, and the plain path -- switch on against off at N = 2: same losses, same parameters, same Adam moments, bit
    for bit.  A recomputed h released before the side stream has read it shows here."""
    off = _train_steps(name, mode, fp16, False)
    on = _train_steps(name, mode, fp16, True)
    print("[recompute train_batch %s %s %s] losses off %s on %s, gn_conv calls %d" % (
        name, "bf16" if fp16 else "fp32", mode, off[0], on[0], on[3]))
    _assert_same_training(on, off, (name, fp16, mode))


def test_train_batch_with_the_deferred_weight_gradient_queue_active():
    """the bf16 fused step at a batch where the 1x1 weight gradients are queued for grouped launches (M >= 4096 pixels: the
    mini nested model's 32 x 32 level at N = 8) and the GroupNorm parameter gradients go out as per-sample rows -- the
    state a real run is in, next to the recomputed h.  Nothing on this path sums over samples with atomics (rows, slabs and
    grouped launches are fixed-order), which is first shown by two switch-off runs that must agree in every bit."""
    name = "mini_nested"
    off = _train_steps(name, "fused", True, False, batch=8)
    off2 = _train_steps(name, "fused", True, False, batch=8)
    print("[recompute train_batch queue] queued 1x1 weight gradients per run: %d, losses %s" % (off[4], off[0]))
    assert off[4] > 0, "no 1x1 weight gradient was queued: the case does not reach the deferred path"
    assert off2[0] == off[0] and not [k for k in off[1] if ndiff(off2[1][k], off[1][k])], "the stored path is not deterministic here"
    on = _train_steps(name, "fused", True, True, batch=8)
    assert on[4] == off[4]
    _assert_same_training(on, off, (name, "bf16", "fused", "N=8"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", MODELS)
def test_forward_holds_the_recomputed_activations_less(name, dtype):
    """memory_allocated() right after forward, loss alive: off - on >= sum of the bytes of every h that is re-applied"""
    model = PC.build_module(name)[0].to(DEV)
    inp = PC.inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    args = (x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    held = {}
    for on in (False, True, False, True):   # the first pair is the warm-up (packed weights, workspaces)
        with recompute(on), count_gn_conv() as cnt, torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            # unreachable cycles that earlier tests left (whole models: gigabytes) are freed HERE, not by a collection that
            # happens to run during the forward and would be booked as memory the forward gave back
            gc.collect()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            loss = PC.loss_of(model(*args), inp["gys"])
            torch.cuda.synchronize()
            held[on] = torch.cuda.memory_allocated() - base
            loss.backward()
        model.zero_grad(set_to_none=True)
        del loss
        analytic = cnt.bytes if on else 0
    saved = held[False] - held[True]
    print("[recompute memory %s %s] held after forward: off %d B, on %d B, saved %d B, analytic sum of recomputed h %d B" % (
        name, dtype, held[False], held[True], saved, analytic))
    assert analytic > 0
    assert saved >= analytic
