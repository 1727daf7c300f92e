"""CPU: projected and rescaled classifier-free guidance without a GPU -- ``CFG`` validation, the torch ``cfg_combine``
against the fp64 restatement of tests/cfg_cases.py, the identities of the definition in fp64, the CPU samplers on stub
models (cfg=None is today's output, the momentum history per trajectory, the interval, the refusals) and the new C-ABI
entries."""
import ctypes

import pytest
import torch

import cfg_cases as CC
import dpm_cases as DC
import stub_models as SM

GATE = 2e-5   # max-abs over max-abs: the project's fp32 per-kernel gate


def test_cfg_validation():
    import mdm_hip
    from mdm_hip import guidance

    assert mdm_hip.CFG is guidance.CFG and "CFG" in mdm_hip.__all__ and mdm_hip.guidance is guidance
    c = mdm_hip.CFG()
    assert (c.eta, c.norm_threshold, c.momentum, c.rescale, c.interval) == (1.0, 0.0, 0.0, 0.0, None)
    c = mdm_hip.CFG(eta=0, norm_threshold=2.5, momentum=-0.5, rescale=0.7, interval=(0.2, 0.8))
    assert c.key() == ("cfg", 0.0, 2.5, -0.5, 0.7, (0.2, 0.8)) and hash(c.key()) is not None
    assert c.on(200, 1000) and c.on(800, 1000) and not c.on(199, 1000) and not c.on(801, 1000)
    assert mdm_hip.CFG().on(1, 1000)
    for bad in (dict(eta=float("nan")), dict(eta=float("inf")), dict(norm_threshold=-1e-3), dict(norm_threshold=float("nan")),
                dict(momentum=1.0), dict(momentum=-1.0), dict(momentum=float("nan")), dict(rescale=-0.1), dict(rescale=1.01),
                dict(interval=(0.8, 0.2)), dict(interval=0.5), dict(interval=(0.1, float("nan")))):
        with pytest.raises(ValueError, match="CFG"):
            mdm_hip.CFG(**bad)
    mdm_hip.CFG(eta=-0.5, momentum=0.99, rescale=1.0, interval=(0.3, 0.3))   # legal edges


def _torch_combine(shape, opt, pt, dtype):
    from mdm_hip import guidance

    i = CC.inputs(shape)
    kw = CC.OPTIONS[opt]
    t = lambda v: v.to(dtype)
    return guidance.cfg_combine(t(i["x_t"]), t(i["p_c"]), t(i["p_u"]), t(i["gamma"]), pt, CC.W,
                                run_prev=t(i["run"]) if kw.get("momentum") else None, **kw)


@pytest.mark.parametrize("pt", CC.PRED_TYPES)
@pytest.mark.parametrize("opt", list(CC.OPTIONS))
def test_torch_combine_matches_the_fp64_restatement(opt, pt):
    """fp32 within the fp32 gate, fp64 to 1e-12; the momentum state alike"""
    worst = 0.0
    for shape in CC.SHAPES:
        want, want_run, _ = CC.reference(shape, opt, pt)
        for dtype, gate in ((torch.float32, GATE), (torch.float64, 1e-12)):
            got, run = _torch_combine(shape, opt, pt, dtype)
            err = CC.maxerr(got, want)
            assert got.dtype == dtype and torch.isfinite(got).all() and err < gate, (shape, dtype, err)
            assert (run is None) == (want_run is None)
            if run is not None:
                assert CC.maxerr(run, want_run) < gate
            if dtype == torch.float32:
                worst = max(worst, err)
    print("%s %s: fp32 torch ops against fp64, worst %.2e" % (opt, pt, worst))


def test_the_cap_is_active_in_some_rows_and_idle_in_others():
    for pt in CC.PRED_TYPES:
        s = CC.reference((3, 3, 5, 4), "cap-mixed", pt)[2]["s"]
        assert float(s[0]) == 1.0 and float(s[1]) < 1.0 and float(s[2]) < 1.0
        assert float(CC.reference((3, 3, 5, 4), "all", pt)[2]["s"].max()) < 1.0


@pytest.mark.parametrize("pt", CC.PRED_TYPES)
def test_identities_in_fp64(pt):
    from mdm_hip import guidance

    shape = (3, 3, 160, 136)
    i = {k: v.double() for k, v in CC.inputs(shape).items()}
    x, pc, pu, g, run = i["x_t"], i["p_c"], i["p_u"], i["gamma"], i["run"]
    a, be = CC.coeffs(g.reshape(-1, 1, 1, 1), pt)
    D = a * x + be * pc
    dot = lambda u, v: (u * v).flatten(1).sum(1)
    comb = lambda **kw: guidance.cfg_combine(x, pc, pu, g, pt, CC.W, **kw)
    # the defaults are plain classifier-free guidance
    plain = pu + CC.W * (pc - pu)
    assert CC.maxerr(comb()[0], plain) < 1e-12 and comb()[1] is None
    # eta = 0: the update of x0 is orthogonal to the conditional x0
    x0_g = a * x + be * comb(eta=0.0)[0]
    assert float((dot(x0_g - D, D).abs() / (dot(D, D) * dot(x0_g - D, x0_g - D)).sqrt()).max()) < 1e-12
    # a capped update has the cap's RMS, in image units: here at image scale 2 and eta = 1, where u = s dD
    thr, sc = 0.05, 2.0
    p_g = comb(norm_threshold=thr, image_scale=sc)[0]
    u = be * (p_g - pc) / (CC.W - 1)
    rms = sc * (dot(u, u) / pc[0].numel()).sqrt()
    assert float((rms - thr).abs().max()) < 1e-12 * thr
    assert abs(CC.paper_radius(thr, pc[0].numel()) - float(sc * dot(u, u).sqrt()[0])) < 1e-9
    # rescale = 1: the guided prediction has the conditional one's std
    sd = lambda t: t.flatten(1).var(1, unbiased=False).sqrt()
    assert float((sd(comb(rescale=1.0)[0]) / sd(pc) - 1).abs().max()) < 1e-12
    assert float((sd(comb()[0]) / sd(pc) - 1).abs().min()) > 0.5   # ... which plain guidance at w = 7.5 is far from
    # momentum: run is the update before the cap, history included
    p, r = comb(momentum=-0.5, norm_threshold=0.01, run_prev=run)
    assert CC.maxerr(r, be * (pc - pu) - 0.5 * run) < 1e-12
    assert torch.equal(comb(momentum=-0.5)[1], be * (pc - pu))   # no history: run_prev counts as 0
    # guidance off: the operands themselves
    p, r = comb(momentum=-0.5, rescale=0.7, run_prev=run, on=False)
    assert p is pc and r is run
    w, _, _ = CC.cfg_ref(x, pc, pu, g, pt, CC.W, momentum=-0.5, rescale=0.7, run_prev=run, on=False)
    assert torch.equal(w, pc)
    # degenerate inputs follow the definition and stay finite
    assert torch.equal(guidance.cfg_combine(x, pc, pc, g, pt, CC.W, eta=0.0, norm_threshold=0.1, rescale=0.7)[0], pc)
    z = torch.zeros_like(pc)
    p = guidance.cfg_combine(z, z, pu, g, pt, CC.W, eta=0.0, rescale=0.7)[0]    # D_c == 0: c = 0; std(p_c) = 0
    assert torch.isfinite(p).all() and CC.maxerr(p, 0.3 * (1 - CC.W) * pu) < 1e-12
    half = torch.full_like(pc, 0.5)
    assert torch.equal(guidance.cfg_combine(x, half, half, g, pt, CC.W, rescale=1.0)[0], half)   # a constant p_g: factor 1


# ---- the CPU samplers ------------------------------------------------------------------------------------------------------
B, S, D = 2, 5, 8
W = 7.5


def _sc(**kw):
    from mdm_hip import samplers as S_

    base = dict(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM",
                threshold_function="CLIP")
    base.update(kw)
    return S_.SamplerConfig(**base)


def _pipe(nested, **kw):
    from mdm_hip import diffusion as Df

    if nested:
        cfg = Df.NestedDiffusionConfig(sampler_config=_sc(schedule_shifted=True, rescale_signal=1, **kw),
                                       use_vdm_loss_weights=False, use_double_loss=True, no_use_residual=True)
        return Df.NestedDiffusion(SM.StubNestedUNet(), cfg)
    return Df.Diffusion(SM.StubUNet(), Df.DiffusionConfig(sampler_config=_sc(**kw), use_vdm_loss_weights=False))


def _inputs(nested, seed=0):
    g = torch.Generator().manual_seed(seed)
    lm = torch.randn(B, S, D, generator=g)
    lm = torch.cat([torch.zeros_like(lm), lm])
    mask = torch.ones(2 * B, S)
    side = 32 if nested else 16
    x = torch.randn(B, 3, side, side, generator=g)
    xs = [x, torch.randn(B, 3, side // 4, side // 4, generator=g)] if nested else x
    return xs, lm, mask


def _run(pipe, xs, lm, mask, n=4, w=W, **kw):
    x = [t.clone() for t in xs] if isinstance(xs, list) else xs.clone()
    kw.setdefault("ddim_eta", 0)
    if kw.get("solver"):
        kw.pop("ddim_eta")
    with torch.no_grad():
        return pipe.sampler.sample(pipe.get_model(), x, lm, mask, {}, resample_steps=True, num_inference_steps=n,
                                   guidance_scale=w, **kw)


class Recorder:
    """wraps ``Sampler._cfg_scales`` of one sampler: (on, history present, number of scales) per call"""

    def __init__(self, monkeypatch, smp):
        self.calls = []
        inner = smp._cfg_scales

        def wrapped(cfg, x_t, pcs, pus, g_t, image_scales, guidance_scale, state=None, on=True, gates=None):
            self.calls.append((bool(on), state is not None and state.get("cfg_run") is not None, len(x_t)))
            return inner(cfg, x_t, pcs, pus, g_t, image_scales, guidance_scale, state, on, gates)

        monkeypatch.setattr(smp, "_cfg_scales", wrapped)


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
def test_cfg_none_and_guidance_one_change_no_bit(nested, monkeypatch):
    import mdm_hip

    pipe = _pipe(nested)
    xs, lm, mask = _inputs(nested)
    rec = Recorder(monkeypatch, pipe.sampler)
    full = mdm_hip.CFG(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7)
    for kw in (dict(), dict(ddim_eta=None), dict(solver="dpmpp_2m")):
        torch.manual_seed(3)
        base = _run(pipe, xs, lm, mask, **kw)
        torch.manual_seed(3)
        assert torch.equal(_run(pipe, xs, lm, mask, cfg=None, **kw), base)
        # the defaults are plain guidance up to rounding, and do go through the combine
        torch.manual_seed(3)
        same = _run(pipe, xs, lm, mask, cfg=mdm_hip.CFG(), **kw)
        assert CC.rel_l2(same, base) < 1e-5 and len(rec.calls) == 4
        rec.calls.clear()
        torch.manual_seed(3)
        moved = _run(pipe, xs, lm, mask, cfg=full, **kw)
        assert torch.isfinite(moved).all() and CC.maxerr(moved, base) > 1e-3
        rec.calls.clear()
    # guidance_scale == 1: cfg is a no-op, nothing is combined
    one = _run(pipe, xs, lm[B:], mask[B:], w=1)
    assert torch.equal(_run(pipe, xs, lm[B:], mask[B:], w=1, cfg=full), one) and not rec.calls


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
def test_momentum_history_starts_empty_with_every_trajectory(nested, monkeypatch):
    import mdm_hip

    pipe = _pipe(nested)
    xs, lm, mask = _inputs(nested, seed=1)
    rec = Recorder(monkeypatch, pipe.sampler)
    cfg = mdm_hip.CFG(momentum=-0.5, eta=0.0)
    scales = 2 if nested else 1
    a = _run(pipe, xs, lm, mask, cfg=cfg)
    assert rec.calls == [(True, False, scales)] + [(True, True, scales)] * 3
    rec.calls.clear()
    assert torch.equal(_run(pipe, xs, lm, mask, cfg=cfg), a)   # nothing of the first trajectory is left
    assert rec.calls == [(True, False, scales)] + [(True, True, scales)] * 3
    assert CC.maxerr(a, _run(pipe, xs, lm, mask, cfg=mdm_hip.CFG(eta=0.0))) > 1e-4   # the momentum acts
    # a late start (t=) starts without history too; so does every get_xt_minus_1 call without a state dict
    rec.calls.clear()
    with torch.no_grad():
        pipe.sampler.sample(pipe.get_model(), xs, lm, mask, {}, resample_steps=True, num_inference_steps=4, ddim_eta=0,
                            guidance_scale=W, cfg=cfg, t=600)
    assert rec.calls == [(True, False, scales), (True, True, scales)]
    # known images with resample = 2: every denoiser call updates the history, the repeats included
    rec.calls.clear()
    top = xs[0] if nested else xs
    known = [0.5 * torch.ones_like(top), None] if nested else 0.5 * torch.ones_like(top)
    m = torch.zeros(B, 1, *top.shape[2:])
    m[..., : top.shape[-1] // 2] = 1
    _run(pipe, xs, lm, mask, n=3, cfg=cfg, known_images=known, known_mask=[m, None] if nested else m, resample=2)
    assert rec.calls == [(True, False, scales)] + [(True, True, scales)] * 4


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
def test_interval_turns_guidance_off_exactly_outside_it(nested, monkeypatch):
    import mdm_hip

    pipe = _pipe(nested)
    smp = pipe.sampler
    xs, lm, mask = _inputs(nested, seed=2)
    rec = Recorder(monkeypatch, smp)
    steps = [int(t) for t in smp.set_timesteps(6)[:-1]]
    lo, hi = 0.25, 0.7
    want = [lo <= t / 1000 <= hi for t in steps]
    assert True in want and False in want and not want[0] and not want[-1]
    scales = 2 if nested else 1
    out = _run(pipe, xs, lm, mask, n=6, cfg=mdm_hip.CFG(momentum=-0.5, interval=(lo, hi)))
    assert [c[0] for c in rec.calls] == want
    first = want.index(True)
    assert [c[1] for c in rec.calls] == [i > first for i in range(len(want))]   # the history begins with the first guided step
    # an interval that holds no step: the conditional prediction alone drives every step
    off = _run(pipe, xs, lm, mask, n=6, cfg=mdm_hip.CFG(rescale=0.7, interval=(2.0, 3.0)))
    cond = _run(pipe, xs, lm[B:], mask[B:], n=6, w=1)
    assert CC.maxerr(off, cond) < 1e-6 and CC.maxerr(out, cond) > 1e-3
    # the whole schedule: the same as no interval
    assert torch.equal(_run(pipe, xs, lm, mask, cfg=mdm_hip.CFG(eta=0.0, interval=(0.0, 1.0))),
                       _run(pipe, xs, lm, mask, cfg=mdm_hip.CFG(eta=0.0)))


@pytest.mark.parametrize("fn", ["NONE", "CLIP", "DYNAMIC", "DYNAMIC_IF"])
@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
def test_only_the_prediction_handed_to_the_step_changes(fn, pred):
    """every threshold function and both prediction types: the sampler with cfg= is the sampler without it run on a model
    whose predictions are already combined -- here a wrapper that returns the fp64 restatement's p_g in both halves"""
    import mdm_hip
    from mdm_hip import diffusion as Df

    pipe = _pipe(False, threshold_function=fn, prediction_type=pred)
    smp, model = pipe.sampler, pipe.get_model()
    xs, lm, mask = _inputs(False, seed=4)
    opts = dict(eta=0.25, norm_threshold=0.1, rescale=0.7)

    class Combined(torch.nn.Module):
        input_channels, conditions = 3, None

        def forward(self, x_t, times, lm_outputs, lm_mask, micros={}):
            pu, pc = model.vision_model(x_t, times, lm_outputs, lm_mask, micros).chunk(2)
            g = smp.gammas[times[:B] + 1]
            p_g = CC.cfg_ref(x_t[:B], pc, pu, g, pred, W, **opts)[0].to(pc.dtype)
            return torch.cat([p_g, p_g])

    got = _run(pipe, xs, lm, mask, cfg=mdm_hip.CFG(**opts))
    want = _run(Df.Diffusion(Combined(), Df.DiffusionConfig(sampler_config=_sc(threshold_function=fn, prediction_type=pred),
                                                            use_vdm_loss_weights=False)), xs, lm, mask)
    assert torch.isfinite(got).all() and CC.rel_l2(got, want) < 1e-5
    assert CC.rel_l2(got, _run(pipe, xs, lm, mask)) > 10 * 1e-5   # ... and it is not the plain combine (the stub's text term is small)


def test_identical_predictions_leave_the_trajectory_alone():
    """fp64, the closed-form Gaussian denoiser ignores the text: p_u == p_c, every correction is exactly zero"""
    import mdm_hip
    from mdm_hip import diffusion as Df
    from mdm_hip import samplers as S_

    smp = S_.Sampler(_sc(threshold_function="NONE")).double()
    model = Df.Model(DC.GaussianDenoiser(smp.gammas))
    x = torch.randn(B, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    lm, mask = torch.zeros(2 * B, S, D, dtype=torch.float64), torch.ones(2 * B, S, dtype=torch.float64)
    run = lambda **kw: smp.sample(model, x.clone(), lm, mask, {}, resample_steps=True, num_inference_steps=5,
                                  solver="dpmpp_2m", guidance_scale=W, **kw)
    with torch.no_grad():
        assert torch.equal(run(cfg=mdm_hip.CFG(eta=0.0, norm_threshold=0.1, momentum=-0.5, rescale=0.7)), run())


def test_refusals():
    import inspect

    import mdm_hip
    from mdm_hip.graph import GraphedSampler
    from mdm_hip.samplers import SampleOptions

    pipe = _pipe(False)
    smp, model = pipe.sampler, pipe.get_model()
    xs, lm, mask = _inputs(False)
    guide = mdm_hip.LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=W)
    with pytest.raises(NotImplementedError, match="Jacobian"):
        smp.sample(model, xs, lm, mask, {}, guide=guide, cfg=mdm_hip.CFG(), **kw)
    with pytest.raises(NotImplementedError, match="Jacobian"):
        smp.get_xt_minus_1(model, 700, xs, lm, mask, guide=guide, cfg=mdm_hip.CFG(), guidance_scale=W)
    with pytest.raises(NotImplementedError, match="perturbed-attention"):
        smp.sample(model, xs, lm, mask, {}, pag_scale=1.0, cfg=mdm_hip.CFG(), **kw)
    with pytest.raises(NotImplementedError, match="perturbed-attention"):
        smp.get_xt_minus_1(model, 700, xs, lm, mask, pag_scale=1.0, cfg=mdm_hip.CFG(), guidance_scale=W)
    with pytest.raises(ValueError, match="mdm_hip.CFG"):
        smp.sample(model, xs, lm, mask, {}, cfg=dict(eta=0), **kw)
    c = mdm_hip.CFG()
    c.rescale = 2.0   # changed after construction: caught where it is used
    with pytest.raises(ValueError, match="rescale"):
        smp.sample(model, xs, lm, mask, {}, cfg=c, **kw)
    # the keyword reaches GraphedSampler.sample through its **options: the fields of SampleOptions, with their defaults
    sig = inspect.signature(GraphedSampler.sample).parameters
    assert sig["options"].kind is inspect.Parameter.VAR_KEYWORD and SampleOptions().cfg is None
    with pytest.raises(NotImplementedError, match="perturbed-attention"):
        GraphedSampler(pipe).sample(B, {"lm_outputs": lm, "lm_mask": mask}, 16, torch.device("cpu"), guidance_scale=W,
                                    pag_scale=1.0, cfg=mdm_hip.CFG())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_refuse_bad_arguments():
    from mdm_hip import _lib

    assert len(_lib.header_prototypes()) == 85 and _lib.ABI_VERSION == 6 and "guidance.hip" in _lib.SOURCES
    ext = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert ext["mdm_cfg_plan"][1] == ["B", "chw", "rescale_on", "ws_bytes"] and ext["mdm_cfg_plan"][0][1] is ctypes.c_size_t
    assert ext["mdm_cfg_stats"][1] == ["x_t", "pred", "pred_uncond", "gamma", "run_prev", "run_out", "run_gate", "w_gate",
                                       "momentum", "rescale_on", "ws", "ws_bytes", "B", "chw", "pred_type", "stream"]
    assert ext["mdm_cfg_combine"][1] == ["x_t", "pred", "pred_uncond", "gamma", "run", "w_gate", "ws", "ws_bytes", "out",
                                         "guidance", "eta", "norm_threshold", "rescale", "image_scale", "B", "chw",
                                         "pred_type", "stream"]
    L = _lib.lib()
    for name in ("mdm_cfg_plan", "mdm_cfg_stats", "mdm_cfg_combine"):
        assert getattr(L, name).argtypes == ext[name][0]
    ws = ctypes.c_size_t(0)
    plan = lambda *a: L.mdm_cfg_plan(*a, ctypes.byref(ws))
    assert plan(1, 12, 0) == 0 and ws.value == 3 * 4
    assert plan(1, 12, 1) == 0 and ws.value == 9 * 4
    assert plan(4, 3 * 64 * 64, 1) == 0 and ws.value == 4 * 6 * 9 * 4            # 3072 groups of 16 bytes: 6 slabs of 512
    one = ws.value // 4
    assert plan(1, 3 * 64 * 64, 1) == 0 and ws.value == one                       # the slabs of a sample do not depend on B
    assert plan(1, 3 * 1024 * 1024, 0) == 0 and ws.value == 512 * 3 * 4          # one sample still fills the chip
    assert plan(1, 14, 0) < 0 and plan(1, 0, 0) < 0 and plan(0, 12, 0) < 0 and plan(65536, 12, 0) < 0
    assert L.mdm_cfg_plan(1, 12, 0, None) < 0
    # argument checks come before any launch
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    x, pc, pu, g, run, out, wsp = (ctypes.c_void_p(base + 256 * k) for k in range(7))
    stats = lambda **kw: L.mdm_cfg_stats(*[dict(dict(x_t=x, pred=pc, pred_uncond=pu, gamma=g, run_prev=None, run_out=None,
                                                     run_gate=None, w_gate=None, momentum=0.0, rescale_on=0, ws=wsp, ws_bytes=12,
                                                     B=1, chw=12, pred_type=2, stream=None), **kw)[k]
                                           for k in ext["mdm_cfg_stats"][1]])
    comb = lambda **kw: L.mdm_cfg_combine(*[dict(dict(x_t=x, pred=pc, pred_uncond=pu, gamma=g, run=None, w_gate=None, ws=wsp,
                                                      ws_bytes=12, out=out, guidance=7.5, eta=1.0, norm_threshold=0.0,
                                                      rescale=0.0, image_scale=1.0, B=1, chw=12, pred_type=2, stream=None),
                                                 **kw)[k] for k in ext["mdm_cfg_combine"][1]])
    assert stats(chw=14) < 0 and stats(B=0) < 0 and stats(ws_bytes=8) < 0 and stats(rescale_on=1) < 0   # 9 sums need 36 bytes
    assert stats(pred_uncond=None) < 0 and stats(run_prev=run) < 0 and stats(run_out=pc, momentum=0.5) < 0
    assert stats(run_out=run, momentum=1.0) < 0 and stats(pred_type=3) < 0
    assert stats(x_t=ctypes.c_void_p(base + 4)) < 0
    assert comb(chw=14) < 0 and comb(B=0) < 0 and comb(ws_bytes=8) < 0 and comb(rescale=0.5) < 0
    assert comb(out=x) < 0 and comb(out=pu) < 0 and comb(run=run, out=run) < 0 and comb(pred_uncond=None) < 0
    assert comb(rescale=1.5) < 0 and comb(norm_threshold=-1.0) < 0 and comb(eta=float("nan")) < 0 and comb(image_scale=0.0) < 0
    assert b"guidance.hip" in L.mdm_last_error()
