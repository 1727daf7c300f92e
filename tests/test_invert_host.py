"""CPU: image inversion -- the torch-op path of ``Sampler.invert`` (DDIM inversion with fixed-point refinement),
``Sampler.noise_maps`` (edit-friendly DDPM inversion) and the ``step_noise=`` replay.  The reference has neither, so the
yardsticks are tests/invert_cases.py (both formulas restated in fp64, closed-form Gaussian denoisers) and the identities
that tie the new code to the reverse step pinned to the reference's goldens: ``invert_step`` undoes DDIM(0), and a replay of
the maps passes through the stored noisy copies."""
import pytest
import torch

import dpm_cases as DC
import invert_cases as IC
import stub_models as SM


def maxerr(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


def sc(**kw):
    from mdm_hip import samplers as S

    base = dict(num_diffusion_steps=32, schedule_type="COSINE", prediction_type="V_PREDICTION", loss_target_type="DDPM",
                threshold_function="NONE")
    base.update(kw)
    return S.SamplerConfig(**base)


# (gamma_s, gamma_t) per sample: the image itself as the cleaner node, a wide step, and two ADJACENT nodes of the 1000-step
# linear schedule, where sigma_s alpha_t - alpha_s sigma_t cancels to a few digits if it is taken as a difference
def gamma_pairs():
    from mdm_hip import samplers as S

    lin = S.gammas_linear_beta(1000, 0.0001, 0.02)
    gs = torch.tensor([1.0, 0.9, lin[500], lin[1]], dtype=torch.float64)
    gt = torch.tensor([0.97, 0.3, lin[501], lin[2]], dtype=torch.float64)
    return gs, gt


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
@pytest.mark.parametrize("guided", [False, True])
def test_torch_formulas_match_the_fp64_restatement(pred, guided):
    """``samplers.invert_step`` and ``Sampler.get_noise_map`` on fp64 CPU tensors == tests/invert_cases.py, 1e-12"""
    from mdm_hip import samplers as S

    gen = torch.Generator().manual_seed(2)
    gs, gt = gamma_pairs()
    B = gs.numel()
    rnd = lambda: torch.randn(B, 3, 6, 6, generator=gen, dtype=torch.float64)
    x, pc, pu = rnd() * 1.2, rnd(), rnd()
    w = 2.5 if guided else 1.0
    got = S.invert_step(x, pc, gs, gt, pred, pu if guided else None, w)
    ref = IC.invert_step_ref(x, pc, gs, gt, pred, pu if guided else None, w)
    e = maxerr(got, ref) / float(ref.abs().max())
    print("invert_step %s: %.2e" % (pred, e))
    assert e <= 1e-12
    # the noise map: a step from the noisier gt to gs (gs == 1 in row 0: sigma == 0, z = 0)
    for thr, scale in (("NONE", None), ("CLIP", 2.0)):
        for eta in (None, 0.6):
            smp = S.Sampler(sc(prediction_type=pred, threshold_function=thr, rescale_signal=scale)).double()
            x_s = rnd()
            z = smp.get_noise_map(x, x_s, pc, gt.reshape(-1, 1, 1, 1), gs.reshape(-1, 1, 1, 1), clip_fn=smp.clip_sample,
                                  ddim_eta=eta, image_scale=scale, pred_uncond=pu if guided else None, guidance_scale=w)
            zr = IC.noise_map_ref(x, x_s, pc, gt, gs, pred_type=pred, thr=thr, image_scale=scale or 1.0,
                                  pred_uncond=pu if guided else None, guidance=w, ddim_eta=eta)
            e = maxerr(z, zr) / float(zr.abs().max())
            print("noise_map %s %s eta=%s: %.2e" % (pred, thr, eta, e))
            assert e <= 1e-12
            assert float(z[0].abs().max()) == 0.0   # gamma_last == 1
            # ... and it is the noise that lands the step on x_s
            _, back, _ = smp.get_prediction_xt_last(x, pc, gt.reshape(-1, 1, 1, 1), gs.reshape(-1, 1, 1, 1), clip_fn=smp.clip_sample,
                                                    need_noise=True, ddim_eta=eta, input_noise=z, image_scale=scale,
                                                    return_eps=False, pred_uncond=pu if guided else None, guidance_scale=w)
            assert maxerr(back[1:], x_s[1:]) <= 1e-12 * max(1.0, float(x_s.abs().max()))


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
def test_one_step_identity(pred):
    """random x_t, p: DDIM(0) by ``get_prediction_xt_last`` (no threshold), then ``invert_step`` with the same p -> x_t again
    within 1e-12, also from gamma_s = 1 and between adjacent nodes of the 1000-step linear schedule"""
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(prediction_type=pred)).double()
    gen = torch.Generator().manual_seed(4)
    gs, gt = gamma_pairs()
    B = gs.numel()
    x_t = torch.randn(B, 3, 6, 6, generator=gen, dtype=torch.float64) * 1.1
    p = torch.randn(B, 3, 6, 6, generator=gen, dtype=torch.float64)
    _, x_s, _ = smp.get_prediction_xt_last(x_t, p, gt.reshape(-1, 1, 1, 1), gs.reshape(-1, 1, 1, 1),
                                           clip_fn=lambda x, s: x, ddim_eta=0, return_eps=False)
    assert maxerr(x_s, IC.ddim0_ref(x_t, p, gt, gs, pred)) <= 1e-12
    back = S.invert_step(x_s, p, gs, gt, pred)
    errs = [maxerr(back[b], x_t[b]) for b in range(B)]
    print(pred, ["%.1e" % e for e in errs])
    assert max(errs) <= 1e-12


def _gaussian(pred):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(prediction_type=pred)).double()
    den = DC.GaussianDenoiser if pred == "V_PREDICTION" else IC.GaussianEpsDenoiser
    img = (DC.MU + DC.S * torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).clamp(-1, 1)
    return smp, D.Model(den(smp.gammas)), img


def _round_trip(smp, model, img, K):
    kw = dict(num_inference_steps=16, resample_steps=True)
    x_t, t = smp.invert(model, img, None, None, {}, iterations=K, **kw)
    assert t == int(smp.set_timesteps(16)[0])
    return maxerr(smp.sample(model, x_t, None, None, {}, ddim_eta=0, t=t, **kw), img)


@pytest.mark.parametrize("pred,factor", [("V_PREDICTION", 8.0), ("DDPM", 2.0)])
def test_gaussian_round_trip_converges(pred, factor):
    """cosine schedule, 32 diffusion steps, 16 inference steps, no threshold, fp64: invert(iterations=K) then
    sample(ddim_eta=0) against the image.  Every extra iteration K = 1..4 divides the error by >= 8 (v) / >= 2 (eps);
    measured: v 17.7, 17.0, 16.5 (5.0e-2, 2.8e-3, 1.7e-4, 1.0e-5); eps 5.7, 4.5, 3.6."""
    smp, model, img = _gaussian(pred)
    errs = [_round_trip(smp, model, img, K) for K in (1, 2, 3, 4)]
    print(pred, ["%.2e" % e for e in errs], ["%.1f" % (a / b) for a, b in zip(errs, errs[1:])])
    for a, b in zip(errs, errs[1:]):
        assert a >= factor * b, (pred, errs)


def test_gaussian_round_trip_is_exact_at_twelve_iterations():
    """v-prediction, K = 12: the fixed point is the exact preimage, <= 1e-12 (measured 3.1e-15)"""
    e = _round_trip(*_gaussian("V_PREDICTION"), 12)
    print("K = 12: %.2e" % e)
    assert e <= 1e-12


def test_invert_stops_at_t_like_partial_diffusion():
    smp, model, img = _gaussian("V_PREDICTION")
    steps = smp.set_timesteps(16)
    x_t, t = smp.invert(model, img, None, None, {}, iterations=2, num_inference_steps=16, resample_steps=True, t=20)
    assert t == int(steps[steps <= 20][0])
    x0, t0 = smp.invert(model, img, None, None, {}, num_inference_steps=16, resample_steps=True, t=0)
    assert t0 == 0 and torch.equal(x0, img)
    full, tf = smp.invert(model, img, None, None, {}, iterations=1)   # every step of the schedule
    assert tf == smp.n_steps and full.shape == img.shape


# ---- noise maps ------------------------------------------------------------------------------------------------------
def _pipe(kind, thr):
    from mdm_hip import diffusion as D

    if kind == "nested":
        cfg = D.NestedDiffusionConfig(sampler_config=sc(threshold_function=thr, schedule_shifted=True, rescale_signal=1),
                                      use_vdm_loss_weights=False, use_double_loss=True, no_use_residual=True)
        pipe = D.NestedDiffusion(SM.StubNestedUNet(), cfg)
    elif kind == "gaussian":
        pipe = D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=sc(threshold_function=thr), use_vdm_loss_weights=False))
        pipe.model.vision_model = DC.GaussianDenoiser(pipe.sampler.gammas)
    else:
        pipe = D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=sc(threshold_function=thr), use_vdm_loss_weights=False))
    pipe.sampler.double()
    pipe.model.double()
    return pipe


def _inputs(B=3):
    g = torch.Generator().manual_seed(7)
    lm = torch.randn(2 * B, 5, 8, generator=g, dtype=torch.float64)
    img = torch.rand(B, 3, 16, 16, generator=g, dtype=torch.float64) * 2 - 1
    return img, lm, torch.ones(2 * B, 5, dtype=torch.float64)


def _noise_fn(seed=11):
    gen = torch.Generator().manual_seed(seed)
    return lambda x: torch.randn(x.shape, generator=gen, dtype=x.dtype)


SCHED = dict(num_inference_steps=8, resample_steps=True)


@pytest.mark.parametrize("kind", ["stub", "gaussian", "nested"])
@pytest.mark.parametrize("thr", ["NONE", "CLIP"])
@pytest.mark.parametrize("eta", [None, 0.7])
def test_replay_hits_every_stored_node(kind, thr, eta):
    """noise_maps under guidance 3, then sample(step_noise=maps, return_sequence=True): entry i of the sequence is the stored
    noisy copy of node i within 1e-12 (fp64) -- whatever the threshold function, because the maps absorb it"""
    pipe = _pipe(kind, thr)
    smp, model = pipe.sampler, pipe.get_model()
    img, lm, mask = _inputs()
    x_start, maps, nodes = smp.noise_maps(model, img, lm, mask, {}, guidance_scale=3.0, ddim_eta=eta, noise_fn=_noise_fn(),
                                          return_nodes=True, **SCHED)
    steps = smp.set_timesteps(8)
    assert len(maps) == len(steps) - 1 and len(nodes) == len(steps) - 1
    if kind != "nested":
        assert maps[-1] is None and all(m is not None for m in maps[:-1])   # the last step adds no noise: no map
    else:   # NestedSampler._noisy_step: noise unless the step starts at time 1; the step to gamma = 1 has sigma = 0: z = 0
        assert all(float(z.abs().max()) == 0.0 for z in maps[-1])
    seq = smp.sample(model, x_start, lm, mask, {}, guidance_scale=3.0, ddim_eta=eta, step_noise=maps, return_sequence=True,
                     **SCHED)
    top = lambda v: v[0] if isinstance(v, (list, tuple)) else v
    errs = [maxerr(top(seq[i]), top(smp._postprocess(n)) if i else top(n)) for i, n in enumerate(nodes)]
    print(kind, thr, eta, "%.2e" % max(errs))
    assert max(errs) <= 1e-12 * max(1.0, max(float(top(n).abs().max()) for n in nodes))
    # the same maps under another guidance scale still pass through the first stored node after x_start only by chance:
    # another conditioning gives another image
    other = smp.sample(model, x_start, lm.flip(0) * 1.5, mask, {}, guidance_scale=3.0, ddim_eta=eta, step_noise=maps, **SCHED)
    same = smp.sample(model, x_start, lm, mask, {}, guidance_scale=3.0, ddim_eta=eta, step_noise=maps, **SCHED)
    if kind != "gaussian":   # (the Gaussian denoiser ignores its conditioning)
        assert maxerr(other, same) > 1e-3


def test_noise_maps_draw_order_is_documented():
    """nodes in sampling order, scales hi -> lo: one noise_fn call each, and nothing for node 0"""
    pipe = _pipe("nested", "NONE")
    img, lm, mask = _inputs()
    calls = []
    inner = _noise_fn()

    def fn(x):
        calls.append(tuple(x.shape[-2:]))
        return inner(x)

    pipe.sampler.noise_maps(pipe.get_model(), img, lm, mask, {}, guidance_scale=3.0, noise_fn=fn, **SCHED)
    assert calls == [(16, 16), (4, 4)] * 8


@pytest.mark.parametrize("kind", ["stub", "nested"])
def test_step_noise_none_changes_no_bit(kind):
    pipe = _pipe(kind, "CLIP")
    smp, model = pipe.sampler, pipe.get_model()
    img, lm, mask = _inputs()
    x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    outs = []
    for kw in ({}, dict(step_noise=None)):
        torch.manual_seed(3)
        outs.append(smp.sample(model, x, lm, mask, {}, guidance_scale=3.0, **SCHED, **kw))
    assert torch.equal(outs[0], outs[1])


def test_replay_does_not_advance_the_generator():
    pipe = _pipe("stub", "CLIP")
    smp, model = pipe.sampler, pipe.get_model()
    img, lm, mask = _inputs()
    x_start, maps = smp.noise_maps(model, img, lm, mask, {}, guidance_scale=3.0, noise_fn=_noise_fn(), **SCHED)
    torch.manual_seed(9)
    before = torch.get_rng_state()
    smp.sample(model, x_start, lm, mask, {}, guidance_scale=3.0, step_noise=maps, **SCHED)
    assert torch.equal(before, torch.get_rng_state())


def test_pipeline_invert_and_sample_from():
    """Diffusion.invert -> Inverted -> Diffusion.sample_from, both methods, with a late start (t=)"""
    import mdm_hip
    from mdm_hip import diffusion as D

    smp, model, img = _gaussian("V_PREDICTION")
    pipe = D.Diffusion(model.vision_model, D.DiffusionConfig(sampler_config=sc(), use_vdm_loss_weights=False))
    pipe.sampler.double()
    sample = {"lm_outputs": None, "lm_mask": None}
    inv = pipe.invert(img, None, None, torch.device("cpu"), method="ddim", iterations=12, t=20, **{**SCHED, "num_inference_steps": 16})
    assert isinstance(inv, mdm_hip.Inverted) and inv.step_noise is None and inv.t == 19 and inv.num_inference_steps == 16
    assert maxerr(pipe.sample_from(inv, sample, torch.device("cpu")), img) <= 1e-12
    inv = pipe.invert(img, None, None, torch.device("cpu"), method="ddpm", noise_fn=_noise_fn(), t=20, **SCHED)
    steps = pipe.sampler.set_timesteps(8)
    assert inv.method == "ddpm" and inv.t == int(steps[steps <= 20][0]) and len(inv.step_noise) == int((steps <= 20).sum()) - 1
    out = pipe.sample_from(inv, sample, torch.device("cpu"))
    # the last step is a plain denoise from the least noisy copy: for Gaussian data that is the posterior mean, not the image
    assert out.shape == img.shape and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        pipe.invert(img, None, None, torch.device("cpu"), method="null-text")


def test_refusals():
    from mdm_hip import samplers as S
    import mdm_hip

    pipe = _pipe("stub", "CLIP")
    smp, model = pipe.sampler, pipe.get_model()
    img, lm, mask = _inputs()
    x_start, maps = smp.noise_maps(model, img, lm, mask, {}, guidance_scale=3.0, noise_fn=_noise_fn(), **SCHED)
    run = lambda **kw: smp.sample(model, x_start, lm, mask, {}, guidance_scale=3.0, **{**SCHED, **kw})
    for kw in (dict(step_noise=maps, solver="dpmpp_2m"), dict(step_noise=maps, solver="sa"), dict(step_noise=maps, ddim_eta=0),
               dict(step_noise=maps, ddim_eta=-1.0),
               dict(step_noise=maps, resample=2, known_images=img, known_mask=torch.ones(3, 1, 16, 16, dtype=torch.float64)),
               dict(step_noise=maps[:-1]), dict(step_noise=maps, num_inference_steps=6), dict(step_noise=maps, t=10),
               dict(step_noise=[None] * len(maps)), dict(step_noise=[[m[0][:, :, :8]] if m else None for m in maps]),
               dict(step_noise=[[m[0], m[0]] if m else None for m in maps]), dict(step_noise=maps[0][0])):
        with pytest.raises(ValueError):
            run(**kw)
    guide = S.LossGuide(lambda x0: (x0 ** 2).mean(dim=(1, 2, 3)))
    mg = S.MapGuide(lambda m: None, 1.0)
    tiles = mdm_hip.Tiles(8)
    inv = lambda **kw: smp.invert(model, img, lm, mask, {}, guidance_scale=3.0, **SCHED, **kw)
    nm = lambda **kw: smp.noise_maps(model, img, lm, mask, {}, guidance_scale=3.0, **SCHED, **kw)
    for name, kw in (("guide", dict(guide=guide)), ("map_guide", dict(map_guide=mg)), ("tiles", dict(tiles=tiles)),
                     ("known_images", dict(known_images=img))):
        for fn in (inv, nm):
            with pytest.raises(NotImplementedError) as e:
                fn(**kw)
            assert name in str(e.value)
    for name, kw in (("cfg", dict(cfg=mdm_hip.CFG(rescale=0.5))), ("pag_scale", dict(pag_scale=1.0))):
        with pytest.raises(NotImplementedError) as e:
            inv(**kw)
        assert name in str(e.value)
    x, m = nm(cfg=mdm_hip.CFG(rescale=0.5), noise_fn=_noise_fn())   # noise_maps takes the combined prediction
    assert not torch.equal(m[0][0], maps[0][0])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            inv(iterations=bad)
    with pytest.raises(ValueError):
        nm(ddim_eta=0)
    with pytest.raises(ValueError):
        nm(t=-1)
    with pytest.raises(ValueError):
        nm(t=0)
    with pytest.raises(ValueError):
        smp.get_noise_map(x_start, x_start, x_start, smp.read_gamma(torch.full((3,), 5)), smp.read_gamma(torch.full((3,), 4)),
                          ddim_eta=0.0)


def test_cfg_prediction_reaches_the_maps():
    """noise_maps(cfg=) hands ``get_noise_map`` what the step is handed: a replay with the same cfg= hits the stored nodes"""
    import mdm_hip

    pipe = _pipe("stub", "CLIP")
    smp, model = pipe.sampler, pipe.get_model()
    img, lm, mask = _inputs()
    cfg = mdm_hip.CFG(rescale=0.5, momentum=-0.3)
    x_start, maps, nodes = smp.noise_maps(model, img, lm, mask, {}, guidance_scale=3.0, noise_fn=_noise_fn(), cfg=cfg,
                                          return_nodes=True, **SCHED)
    seq = smp.sample(model, x_start, lm, mask, {}, guidance_scale=3.0, step_noise=maps, cfg=cfg, return_sequence=True, **SCHED)
    errs = [maxerr(seq[i], n[0]) for i, n in enumerate(nodes)]
    assert max(errs) <= 1e-12 * max(1.0, max(float(n[0].abs().max()) for n in nodes))
