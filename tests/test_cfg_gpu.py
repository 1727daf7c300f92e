"""GPU: projected and rescaled classifier-free guidance on the HIP path -- mdm_cfg_stats + mdm_cfg_combine against the fp64
restatement of tests/cfg_cases.py (the fp32 per-kernel gate of DESIGN section 3), their exact properties (gates, batch
independence, reproducibility, aliasing), degenerate inputs, refused arguments, the mini models' eager sampler against a
loop restated here, eager against graphed bit for bit, and bf16 autocast against the plain path's own bf16 error."""
import ctypes
import functools

import pytest
import torch

import cfg_cases as CC
import parity_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-5   # max-abs over max-abs, fp32 (test_pag_gpu.GATE["fp32"])


def _dev(i):
    return {k: v.to(DEV) for k, v in i.items()}


def _combine(i, pt, opt, w=CC.W, history=True, **more):
    """ops.cfg_combine on the device copies ``i`` of CC.inputs under the options ``opt`` -> (p_g, run)"""
    from mdm_hip import ops

    kw = dict(opt)
    kw.update(more)
    if kw.get("momentum") and history and "run_prev" not in kw:
        kw["run_prev"] = i["run"]
    return ops.cfg_combine(i["x_t"], i["p_c"], i["p_u"], i["gamma"], pt, w, **kw)


# ---- the kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", CC.PRED_TYPES)
@pytest.mark.parametrize("opt", list(CC.OPTIONS))
def test_kernels_match_the_fp64_restatement(opt, pt):
    worst = 0.0
    for shape in CC.SHAPES:
        i = _dev(CC.inputs(shape))
        want, want_run, _ = CC.reference(shape, opt, pt)
        got, run = _combine(i, pt, CC.OPTIONS[opt])
        err = CC.maxerr(got, want)
        err_run = CC.maxerr(run, want_run) if want_run is not None else 0.0
        print("%s %s %s: p_g %.2e, run %.2e" % (shape, opt, pt, err, err_run))
        assert (run is None) == (want_run is None)
        assert torch.isfinite(got).all() and err < GATE and err_run < GATE
        assert torch.equal(i["p_c"].cpu(), CC.inputs(shape)["p_c"])   # the inputs are left alone
        worst = max(worst, err, err_run)
    print("%s %s: worst %.2e" % (opt, pt, worst))


FULL = dict(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7)


@pytest.mark.parametrize("pt", CC.PRED_TYPES)
def test_gates_select(pt):
    """w_gate off: out == pred and run_out == run_prev; run_gate off: NaN-filled run_prev is never read"""
    off, on = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    for shape in ((3, 3, 5, 4), (3, 3, 160, 136)):
        i = _dev(CC.inputs(shape))
        want, want_run = _combine(i, pt, FULL)
        # gates that are on change nothing
        got, run = _combine(i, pt, FULL, run_gate=on, w_gate=on)
        assert torch.equal(got, want) and torch.equal(run, want_run)
        # guidance off: the conditional prediction and the history, bit for bit -- in place and into other buffers
        got, run = _combine(i, pt, FULL, run_gate=on, w_gate=off)
        assert torch.equal(got, i["p_c"]) and torch.equal(run, i["run"])
        buf, hist = i["p_c"].clone(), i["run"].clone()
        got, run = _combine(i, pt, FULL, run_prev=hist, run_out=hist, w_gate=off, out=torch.full_like(buf, 7.0))
        assert torch.equal(got, i["p_c"]) and run.data_ptr() == hist.data_ptr() and torch.equal(hist, i["run"])
        # ... and with NaNs wherever an operand must not be read
        nan = torch.full_like(i["p_c"], float("nan"))
        j = dict(i, x_t=nan, p_u=nan)
        got, run = _combine(j, pt, FULL, w_gate=off)
        assert torch.equal(got, i["p_c"]) and torch.equal(run, i["run"])
        got, run = _combine(j, pt, FULL, run_prev=nan, run_gate=off, w_gate=off)
        assert torch.equal(got, i["p_c"]) and torch.equal(run, torch.zeros_like(run))   # no history passes through as none
        # no history: garbage in run_prev behind a closed gate == no run_prev at all
        zero, zero_run = _combine(i, pt, FULL, history=False)
        got, run = _combine(i, pt, FULL, run_prev=nan, run_gate=off)
        assert torch.equal(got, zero) and torch.equal(run, zero_run) and torch.isfinite(got).all()
        got, run = _combine(i, pt, FULL, run_prev=torch.zeros_like(nan))
        assert torch.equal(got, zero) and torch.equal(run, zero_run)
        assert not torch.equal(zero, want)   # ... and the history does act


@pytest.mark.parametrize("opt", ["all", "rescale1"])
def test_a_row_does_not_depend_on_its_batch_and_runs_repeat(opt):
    for shape in ((3, 3, 5, 4), (3, 3, 64, 64), (3, 3, 160, 136)):
        i = _dev(CC.inputs(shape))
        for pt in CC.PRED_TYPES:
            got, run = _combine(i, pt, CC.OPTIONS[opt])
            again, run2 = _combine(i, pt, CC.OPTIONS[opt])
            assert torch.equal(got, again) and (run is None or torch.equal(run, run2))
            for b in range(shape[0]):
                row = {k: v[b:b + 1].contiguous() for k, v in i.items()}
                one, one_run = _combine(row, pt, CC.OPTIONS[opt])
                assert torch.equal(one[0], got[b]), (shape, pt, b)
                assert run is None or torch.equal(one_run[0], run[b])


@pytest.mark.parametrize("pt", CC.PRED_TYPES)
def test_aliasing_gives_the_same_bits(pt):
    for shape in ((3, 3, 5, 4), (1, 3, 256, 256)):
        i = _dev(CC.inputs(shape))
        want, want_run = _combine(i, pt, FULL)
        buf, hist = i["p_c"].clone(), i["run"].clone()
        j = dict(i, p_c=buf)
        got, run = _combine(j, pt, FULL, run_prev=hist, run_out=hist, out=buf)
        assert got.data_ptr() == buf.data_ptr() and run.data_ptr() == hist.data_ptr()
        assert torch.equal(buf, want) and torch.equal(hist, want_run)


def test_degenerate_inputs_stay_finite_and_follow_the_definition():
    from mdm_hip import ops

    shape = (3, 3, 160, 136)
    i = _dev(CC.inputs(shape))
    z, half = torch.zeros_like(i["p_c"]), torch.full_like(i["p_c"], 0.5)
    for pt in CC.PRED_TYPES:
        # p_u == p_c: no update, whatever the options
        got, _ = ops.cfg_combine(i["x_t"], i["p_c"], i["p_c"], i["gamma"], pt, CC.W, eta=0.0, norm_threshold=0.1, rescale=0.7)
        assert torch.equal(got, i["p_c"])
        # D_c == 0 (x_t and p_c zero): c = 0; std(p_c) = 0 pulls the result to (1 - rescale) p_g
        got, _ = ops.cfg_combine(z, z, i["p_u"], i["gamma"], pt, CC.W, eta=0.0, rescale=0.7)
        want, _, info = CC.cfg_ref(z, z, i["p_u"], i["gamma"], pt, CC.W, eta=0.0, rescale=0.7)
        assert torch.isfinite(got).all() and float(info["c"].abs().max()) == 0.0 and CC.maxerr(got, want) < GATE
        # a constant p_g under the rescale: std(p_g) == 0, the factor is 1
        got, _ = ops.cfg_combine(i["x_t"], half, half, i["gamma"], pt, CC.W, rescale=1.0)
        assert torch.equal(got, half)
        # an all-zero problem
        got, run = ops.cfg_combine(z, z, z, i["gamma"], pt, CC.W, run_prev=z, **FULL)
        assert torch.equal(got, z) and torch.equal(run, z)


def test_invalid_arguments_return_a_status_and_launch_nothing():
    from mdm_hip import _lib, ops

    L = _lib.lib()
    x, pc, pu = (torch.randn(2, 12, device=DEV) for _ in range(3))
    g = torch.tensor([0.5, 0.5], device=DEV)
    out = torch.full_like(pc, 3.0)
    ws = torch.full((64,), 5.0, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    size = ctypes.c_size_t(0)
    assert L.mdm_cfg_plan(2, 12, 1, ctypes.byref(size)) == 0 and size.value == 2 * 9 * 4
    stats = lambda B=2, chw=12, wsb=256, resc=1: L.mdm_cfg_stats(p(x), p(pc), p(pu), p(g), None, None, None, None, 0.0, resc, p(ws),
                                                                 wsb, B, chw, 2, ops._stream())
    comb = lambda B=2, chw=12, wsb=256, resc=0.7: L.mdm_cfg_combine(p(x), p(pc), p(pu), p(g), None, None, p(ws), wsb, p(out), 7.5, 1.0,
                                                                    0.0, resc, 1.0, B, chw, 2, ops._stream())
    assert stats(chw=10) < 0 and stats(B=0) < 0 and stats(wsb=size.value - 4) < 0
    assert comb(chw=10) < 0 and comb(B=0) < 0 and comb(wsb=size.value - 4) < 0
    torch.cuda.synchronize()
    assert float(ws.min()) == 5.0 and float(out.min()) == 3.0 == float(out.max())   # nothing ran
    assert stats() == 0 and comb() == 0
    torch.cuda.synchronize()
    want, _, _ = CC.cfg_ref(x.view(2, 3, 2, 2), pc.view(2, 3, 2, 2), pu.view(2, 3, 2, 2), g, "V_PREDICTION", 7.5, rescale=0.7)
    assert CC.maxerr(out.view(2, 3, 2, 2), want) < GATE
    with pytest.raises(_lib.MdmHipError, match="multiple of 4"):
        ops.cfg_combine(x[:, :10].reshape(2, 10, 1, 1), pc[:, :10].reshape(2, 10, 1, 1), pu[:, :10].reshape(2, 10, 1, 1), g,
                        "V_PREDICTION", 7.5)
    with pytest.raises(_lib.MdmHipError, match="momentum"):
        ops.cfg_combine(x, pc, pu, g, "V_PREDICTION", 7.5, run_prev=pu)
    with pytest.raises(_lib.MdmHipError, match="float\\[1\\]"):
        ops.cfg_combine(x, pc, pu, g, "V_PREDICTION", 7.5, w_gate=torch.ones(2, device=DEV))


def test_one_norm_threshold_bites_at_the_same_rms_on_every_scale():
    """a nested sampler whose scales carry image scales 1 and 2: the cap is an RMS in image units, so both scales' updates
    end at norm_threshold -- an L2 radius would have to differ by the factor 2 x sqrt(4) between them"""
    import mdm_hip
    from mdm_hip import samplers as S

    smp = S.NestedSampler(S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                          loss_target_type="DDPM")).to(DEV)
    thr, scales = 0.05, [1.0, 2.0]
    ins = [_dev(CC.inputs((3, 3, 32, 32), seed=1)), _dev(CC.inputs((3, 3, 16, 16), seed=2))]
    g = [i["gamma"] for i in ins]
    outs = smp._cfg_scales(mdm_hip.CFG(norm_threshold=thr), [i["x_t"] for i in ins], [i["p_c"] for i in ins],
                           [i["p_u"] for i in ins], g, scales, CC.W)
    for i, p_g, sc in zip(ins, outs, scales):
        _, be = CC.coeffs(i["gamma"].double().reshape(-1, 1, 1, 1), "V_PREDICTION")
        u = be * (p_g.double() - i["p_c"].double()) / (CC.W - 1)
        rms = sc * u.flatten(1).pow(2).mean(1).sqrt()
        _, _, info = CC.cfg_ref(i["x_t"], i["p_c"], i["p_u"], i["gamma"], "V_PREDICTION", CC.W, norm_threshold=thr, image_scale=sc)
        active = info["s"].to(DEV) < 1
        print("image scale %g: rms of the update %s, cap active %s" % (sc, rms.tolist(), active.tolist()))
        assert bool(active.any()) and float((rms[active] / thr - 1).abs().max()) < 1e-5
        assert bool((rms[~active] < thr).all())


# ---- the samplers --------------------------------------------------------------------------------------------------------
RNG_SEED = 21
W = 2.0


def _pipeline(name, net):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                              use_double_loss=True, no_use_residual=True))
    return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


class Setup:
    """one mini pipeline on the GPU, its text inputs [uncond | cond], eager and graphed runs from given noise"""

    def __init__(self, name, w):
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested, self.w = name, name == "mini_nested", w
        self.pipe = _pipeline(name, PC.build_module(name)[0]).to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].to(DEV), inp["mask"].to(DEV)
        self.cond, self.mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.sample = {"lm_outputs": self.cond, "lm_mask": self.mask}
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, self.side, self.side, generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, self.side // 2, self.side // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, n=4, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, guidance_scale=self.w, **kw)

    def graphed(self, xs, n=4, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, self.side, torch.device(DEV), num_inference_steps=n, start_noise=xs,
                                  seed=RNG_SEED, guidance_scale=self.w, **kw)


@functools.lru_cache(maxsize=None)
def _setup(name, w=W):
    return Setup(name, w)


def _fresh(name, w=W):
    from mdm_hip.graph import GraphedSampler

    s = _setup(name, w)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    return s


def _cfg(**kw):
    import mdm_hip

    return mdm_hip.CFG(**dict(FULL, **kw))


def _restated(s, xs, n, solver, cfg):
    """The loop of ``Sampler._sample`` written out: the HIP model on [uncond | cond], the torch ``cfg_combine`` with the
    momentum history kept here, and the sampler's torch step formulas (a custom clip_fn keeps GPU tensors off the step
    kernels)."""
    from mdm_hip import guidance

    smp, model = s.pipe.sampler, s.pipe.get_model()
    clip = lambda x0, sc: smp.clip_sample(x0, sc)
    steps = smp.set_timesteps(n)
    xs = [x.clone() for x in xs]
    B = xs[0].shape[0]
    image_scales = smp._scale_info(model)[1]
    x0_prev = g_prev = None
    runs = [None] * len(xs)
    with torch.no_grad():
        for i in range(n):
            t = torch.full((2 * B,), int(steps[i]) - 1, dtype=torch.long, device=DEV)
            xin = [torch.cat([x] * 2) for x in xs]
            preds = model(xin if s.nested else xin[0], t, s.cond, s.mask, {})
            preds = list(preds) if s.nested else [preds[0]]
            g_t, g_s = smp._scale_gammas(model, int(steps[i]), B), smp._scale_gammas(model, int(steps[i + 1]), B)
            second = solver is not None and 0 < i < n - 1
            x0s = []
            for k, p in enumerate(preds):
                pu, pc = p.float().chunk(2)
                comb, runs[k] = guidance.cfg_combine(xs[k], pc, pu, g_t[k], smp._config.prediction_type, s.w,
                                                     image_scale=image_scales[k], run_prev=runs[k],
                                                     on=cfg.on(int(steps[i]), smp.n_steps), **cfg.options())
                if solver is None:
                    x0, xs[k], _ = smp.get_prediction_xt_last(xs[k], comb, g_t[k], g_s[k], clip_fn=clip, ddim_eta=0,
                                                             image_scale=image_scales[k], return_eps=False)
                else:
                    x0, xs[k] = smp.get_prediction_xt_last_2m(xs[k], comb, g_t[k], g_s[k], g_prev=g_prev[k] if second else None,
                                                             x0_prev=x0_prev[k] if second else None, second_order=second,
                                                             clip_fn=clip, image_scale=image_scales[k])
                x0s.append(x0)
            x0_prev, g_prev = x0s, g_t
        return smp._postprocess(xs if s.nested else xs[0], clip=True)


@pytest.mark.parametrize("solver,n", [(None, 4), ("dpmpp_2m", 3)], ids=["ddim0", "dpmpp_2m"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_eager_sampler_matches_the_restated_loop(name, solver, n):
    """fp32, rel-L2 1e-5 -- the measure every sampler comparison of this suite uses; and cfg moves the image"""
    s = _setup(name)
    xs = s.start(41)
    kw = dict(solver=solver) if solver else dict(ddim_eta=0)
    cfg = _cfg()
    out = s.eager(xs, n=n, cfg=cfg, **kw)
    want = _restated(s, xs, n, solver, cfg)
    err, worst = CC.rel_l2(out, want), CC.maxerr(out, want)
    plain = s.eager(xs, n=n, **kw)
    print("%s %s: rel-L2 %.2e (max-abs over max-abs %.2e) against the restated loop; cfg moves the image by %.2e against "
          "plain guidance" % (name, solver, err, worst, CC.maxerr(out, plain)))
    assert torch.isfinite(out).all() and err < 1e-5
    assert CC.maxerr(out, plain) > 1e-3


@pytest.mark.parametrize("name,kw,opts", [
    ("mini_unet", dict(ddim_eta=0), dict()),
    ("mini_nested", dict(solver="dpmpp_2m"), dict()),
    ("mini_unet", dict(ddim_eta=0), dict(interval=(0.1, 0.7))),        # 4 steps from t = 801, 601, 400, 200: the first is out
    ("mini_nested", dict(ddim_eta=0, late=600), dict()),               # starts at t = 400
    ("mini_unet", dict(known=True, resample=2), dict(interval=(0.3, 1.0))),   # ancestral DDPM with a known half, the last step out
    ("mini_unet", dict(ddim_eta=0, regions=True, freeu=True), dict()),
], ids=["unet-ddim0", "nested-dpmpp_2m", "unet-interval", "nested-late-start", "unet-ddpm-known-resample", "unet-regions-freeu"])
def test_graphed_sampler_equals_eager_sampler(name, kw, opts):
    """bit for bit, with momentum throughout; also on a second call through the cached graph with other noise, which shows
    that the momentum buffers and the gates are armed anew"""
    import freeu_cases as FC
    import mdm_hip
    import region_cases as RC

    s = _fresh(name)
    cfg = _cfg(**opts)
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed)
        more, gmore = dict(kw), {}
        if more.pop("known", False):
            g = torch.Generator().manual_seed(seed)
            m = torch.zeros(2, 1, s.side, s.side, device=DEV)
            m[..., : s.side // 2] = 1
            more.update(known_images=(torch.randn(2, 3, s.side, s.side, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)
        if more.pop("regions", False):
            more.update(regions=RC.model_regions(name, DEV))
        if more.pop("freeu", False):
            more.update(freeu=mdm_hip.FreeU(b=FC.MODEL_B, s=FC.MODEL_S))
        late = more.pop("late", None)
        emore = dict(more, t=late) if late is not None else more
        gmore = dict(more, start_step=late) if late is not None else more
        want, out = s.eager(xs, cfg=cfg, **emore), s.graphed(xs, cfg=cfg, **gmore)
        print("%s %s %s call %d: rel-L2 %.2e, max-abs %.2e" % (name, sorted(kw), opts, rep, CC.rel_l2(out, want),
                                                             float((out - want).abs().max())))
        assert torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
    plain = s.graphed(xs, **gmore)
    assert len(s.gs._graphs) == 2 and CC.maxerr(out, plain) > 1e-3


def test_graph_key_holds_the_cfg_values():
    import mdm_hip

    s = _fresh("mini_unet")
    xs = s.start(44)
    a = s.graphed(xs, ddim_eta=0, cfg=_cfg())
    assert len(s.gs._graphs) == 1
    b = s.graphed(xs, ddim_eta=0, cfg=_cfg(rescale=0.5))
    assert len(s.gs._graphs) == 2 and not torch.equal(a, b)
    c = s.graphed(xs, ddim_eta=0, cfg=_cfg(interval=(0.0, 0.5)))
    assert len(s.gs._graphs) == 3 and not torch.equal(a, c)
    assert torch.equal(s.graphed(xs, ddim_eta=0, cfg=_cfg()), a) and len(s.gs._graphs) == 3   # the same values: a replay
    assert torch.equal(s.graphed(xs, ddim_eta=0, cfg=_cfg(rescale=0.5)), b) and len(s.gs._graphs) == 3
    plain = s.graphed(xs, ddim_eta=0)
    assert len(s.gs._graphs) == 4
    assert torch.equal(s.graphed(xs, ddim_eta=0, cfg=None), plain) and len(s.gs._graphs) == 4
    assert torch.equal(s.eager(xs, ddim_eta=0, cfg=None), s.eager(xs, ddim_eta=0))
    with pytest.raises(NotImplementedError, match="perturbed-attention"):
        s.graphed(xs, ddim_eta=0, cfg=_cfg(), pag_scale=1.0)
    # guidance 1: cfg is a no-op and adds no graph
    s1 = _fresh("mini_unet", 1)
    s1.cond, s1.mask = s1.cond[2:], s1.mask[2:]
    s1.sample = {"lm_outputs": s1.cond, "lm_mask": s1.mask}
    one = s1.graphed(xs, ddim_eta=0)
    assert torch.equal(s1.graphed(xs, ddim_eta=0, cfg=_cfg()), one) and len(s1.gs._graphs) == 1
    assert torch.equal(s1.eager(xs, ddim_eta=0, cfg=_cfg()), s1.eager(xs, ddim_eta=0))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_bf16_autocast_error_is_that_of_the_plain_path(name):
    """bf16 against fp32 from the same noise, rel-L2: the cfg run's error stays below 2x the plain-guidance run's -- the
    yardstick is the existing path.  2x: the two are different trajectories of a random-weight mini model (the analogous
    PAG / regions ratios measured 0.91 - 1.02 and 0.95 - 0.97)."""
    s = _setup(name)
    xs = s.start(45)
    cfg = _cfg()
    errs = {}
    for tag, kw in (("plain", dict()), ("cfg", dict(cfg=cfg))):
        ref = s.eager(xs, ddim_eta=0, **kw)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            low = s.eager(xs, ddim_eta=0, **kw)
        assert torch.isfinite(low).all()
        errs[tag] = CC.rel_l2(low, ref)
    print("%s bf16 against fp32: plain guidance %.3e, cfg %.3e (ratio %.2f)" % (name, errs["plain"], errs["cfg"],
                                                                              errs["cfg"] / errs["plain"]))
    assert errs["cfg"] < 2 * errs["plain"]
