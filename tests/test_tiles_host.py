"""Tiled (MultiDiffusion) sampling on the host: the window geometry, the torch ``gather`` / ``merge`` of mdm_hip/tiling.py
against the fp64 definition of tests/tiles_cases.py, the rows the denoiser sees, tiled against untiled sampling with a
pointwise stub denoiser (they must agree: rel-L2 1e-5, the suite's sampler measure), the refusals and their place behind the
existing checks, validation, and non-square start noise."""
import types

import pytest
import torch

import tiles_cases as TC

B, S, D = 2, 5, 8
# the fp32 torch restatement against the fp64 definition, max-abs over max |p|: a bound stated for the cases of TC.TABLE.
# Every case, the later ones too, is held to the derived gate TC.merge_gate (roundings counted, doubled).
TORCH_MERGE_BOUND = 8e-8


def _sampler(nested=False):
    from mdm_hip import samplers as SM

    cfg = SM.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP")
    return (SM.NestedSampler if nested else SM.Sampler)(cfg)


def _text(rows=2 * B):
    g = torch.Generator().manual_seed(0)
    return torch.randn(rows, S, D, generator=g), (torch.rand(rows, S, generator=g) < 0.7).float()


# ---- geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_offsets_are_those_of_the_table_and_every_pixel_is_covered(case):
    import mdm_hip

    _, H, W, h, w, sy, sx = case
    tiles = mdm_hip.Tiles((h, w), (sy, sx))
    oy, ox = tiles.offsets(H, W)
    assert (oy, ox) == TC.OFFSETS[case]
    assert oy == [min(i * sy, H - h) for i in range(-((h - H) // sy) + 1)]
    assert ox == [min(j * sx, W - w) for j in range(-((w - W) // sx) + 1)]
    assert [(y, x) for y in oy for x in ox] == TC.window_offsets(case) and tiles.count(H, W) == len(oy) * len(ox)
    _, count = TC.merged(case, 1, "uniform")
    assert int(count.min()) >= 1


def test_defaults_and_scales():
    import mdm_hip

    t = mdm_hip.Tiles(64)
    assert (t.window, t.stride, t.blend) == ((64, 64), (32, 32), "uniform")
    assert mdm_hip.Tiles((5, 1)).stride == (2, 1)
    assert mdm_hip.Tiles(64, 32, "ramp").graph_key() == ("tiles", (64, 64), (32, 32), "ramp")
    low = mdm_hip.Tiles((32, 16), (16, 8), "ramp").at(4)
    assert (low.window, low.stride, low.blend) == ((8, 4), (4, 2), "ramp")
    # the clamped offsets divide too: the same grid at every scale
    top = mdm_hip.Tiles(32, 16).check(32, 56, [1, 2])
    assert [o // 2 for o in top.offsets(32, 56)[1]] == top.at(2).offsets(16, 28)[1] == [0, 8, 12]
    assert torch.equal(mdm_hip.Tiles((3, 4), blend="ramp").weight(), torch.tensor([[1., 2, 2, 1], [2, 4, 4, 2], [1, 2, 2, 1]]))


def test_validation_errors():
    import mdm_hip

    for bad in (dict(window=0), dict(window=(4, 0)), dict(window=8, stride=0), dict(window=8, stride=9),
                dict(window=(8, 4), stride=(4, 5)), dict(window=8, blend="cosine"), dict(window=(8, 8, 8)), dict(window=2.5)):
        with pytest.raises(ValueError):
            mdm_hip.Tiles(**bad)
    t = mdm_hip.Tiles(8, 4)
    with pytest.raises(ValueError, match="larger than the canvas"):
        t.offsets(8, 7)
    with pytest.raises(ValueError, match="larger than the canvas"):
        t.check(4, 16)
    for canvas, ratios in (((16, 30), [1, 4]), ((16, 18), [1, 4])):
        with pytest.raises(ValueError, match="multiples of the largest nesting ratio"):
            t.check(*canvas, ratios)
    with pytest.raises(ValueError, match="multiples of the largest nesting ratio"):
        mdm_hip.Tiles(8, 2).check(16, 32, [1, 4])
    t.check(16, 32, [1, 2, 4])
    # ... and from sample(): a nested canvas that does not divide
    smp, stub = _sampler(True), TC.PointwiseStub(True)
    lm, mask = _text(B)
    with pytest.raises(ValueError, match="multiples of the largest nesting ratio"):
        smp.sample(stub, [torch.randn(B, 3, 8, 11), torch.randn(B, 3, 4, 5)], lm, mask, {}, resample_steps=True,
                   num_inference_steps=2, ddim_eta=0, tiles=mdm_hip.Tiles(8, 4))
    assert stub.calls == 0


# ---- the torch ops -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reps", TC.REPS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_torch_gather_is_the_definition(case, reps):
    import mdm_hip
    from mdm_hip import tiling

    _, H, W, h, w, sy, sx = case
    x, _ = TC.inputs(case, reps)
    got = tiling.gather(x, mdm_hip.Tiles((h, w), (sy, sx)), reps)
    assert torch.equal(got, TC.gather_ref(x, case, reps))


@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("reps", TC.REPS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_torch_merge_matches_the_fp64_definition(case, reps, blend):
    import mdm_hip
    from mdm_hip import tiling

    _, H, W, h, w, sy, sx = case
    tiles = mdm_hip.Tiles((h, w), (sy, sx), blend)
    _, p = TC.inputs(case, reps)
    want, count = TC.merged(case, reps, blend)
    got = tiling.merge(p, tiles, H, W)
    err = float((got.double() - want).abs().max() / p.abs().max())
    print("%s reps %d %s: %.2e (covering up to %d)" % (TC.case_id(case), reps, blend, err, int(count.max())))
    assert got.dtype == torch.float32 and err < TC.merge_gate(int(count.max()))
    assert err <= TORCH_MERGE_BOUND or case not in TC.TABLE
    # a pixel under one window holds that window's value bit for bit; one window: out == p
    single = (count == 1).expand_as(got)
    assert torch.equal(got[single], want.float()[single])
    if tiles.count(H, W) == 1:
        assert torch.equal(got, p)


# ---- what the denoiser sees ----------------------------------------------------------------------------------------------
def test_rows_are_blocks_by_images_by_windows_and_the_conditioning_is_repeated_once_per_call(monkeypatch):
    import mdm_hip
    from mdm_hip import tiling

    made = []
    inner = tiling.cond_rows
    monkeypatch.setattr(tiling, "cond_rows", lambda *a: made.append(a[0]) or inner(*a))
    smp, stub = _sampler(), TC.RecordingStub()
    lm, mask = _text()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, 8, 12, generator=g)
    micros = {"scale": torch.tensor([10.0, 20.0, 30.0, 40.0]), "flag": 7}
    tiles = mdm_hip.Tiles(8, 4)
    T = 2
    assert tiles.offsets(8, 12) == ([0], [0, 4])
    out = smp.sample(stub, x, lm, mask, micros, resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=2.0,
                     pag_scale=1.5, tiles=tiles)
    assert out.shape == x.shape and len(stub.calls) == 3 and made == [T]
    each = lambda v: v.repeat_interleave(T, dim=0)
    blocks = lambda v: torch.cat([v, v[-B:]])   # [uncond | cond | perturbed = cond]
    first = stub.calls[0]
    wins = torch.stack([x[..., 0:8], x[..., 4:12]], dim=1).reshape(B * T, 3, 8, 8)
    assert torch.equal(first["x"], torch.cat([wins] * 3))
    for call in stub.calls:
        assert call["x"].shape == (3 * B * T, 3, 8, 8) and call["pag_rows"] == B * T
        assert torch.equal(call["lm"], each(blocks(lm))) and torch.equal(call["mask"], each(blocks(mask)))
        assert torch.equal(call["micros"]["scale"], each(blocks(micros["scale"]))) and call["micros"]["flag"] == 7
        assert call["t"].shape == (3 * B * T,) and len(set(call["t"].tolist())) == 1
        # within a block, row b T + k is window k of image b: the three blocks hold the same windows
        a, b, c = call["x"].chunk(3)
        assert torch.equal(a, b) and torch.equal(a, c)
    # a single step: the rows are made in that call
    smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, guidance_scale=2.0, pag_scale=1.5, tiles=tiles)
    assert made == [T, T] and torch.equal(stub.calls[-1]["lm"], each(blocks(lm)))


def SM_options(**kw):
    from mdm_hip.samplers import SampleOptions

    return SampleOptions(**kw)


def test_extras_are_those_of_window_zero():
    import mdm_hip

    smp, stub = _sampler(), TC.PointwiseStub()
    lm, mask = _text()
    x = torch.randn(B, 3, 8, 12, generator=torch.Generator().manual_seed(4))
    pcs, pus, extras, pps = smp._forward_model_raw(stub, [x], torch.full((B,), 5), lm, mask, {}, 2.0,
                                                   SM_options(tiles=mdm_hip.Tiles(8, 4)))
    assert pcs[0].shape == pus[0].shape == x.shape and pps is None
    assert extras.shape == (B, 3, 8, 8) and bool((extras == 1).all())


# ---- tiled sampling equals untiled sampling where the denoiser is pointwise ------------------------------------------------
def _canvas(nested):
    g = torch.Generator().manual_seed(11)
    if nested:
        return [torch.randn(B, 3, 16, 30, generator=g), torch.randn(B, 3, 8, 15, generator=g)]
    return torch.randn(B, 3, 10, 13, generator=g)


@pytest.mark.parametrize("guidance", ["plain", "cfg"])
@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("solver,n", [(None, 4), ("dpmpp_2m", 3)], ids=["ddim0", "dpmpp_2m"])
def test_tiled_equals_untiled_for_a_pointwise_denoiser(solver, n, nested, blend, guidance):
    import mdm_hip

    smp, stub = _sampler(nested), TC.PointwiseStub(nested)
    lm, mask = _text()
    x = _canvas(nested)
    tiles = mdm_hip.Tiles(8, 4, blend) if nested else mdm_hip.Tiles((6, 8), (4, 5), blend)
    kw = dict(resample_steps=True, num_inference_steps=n, guidance_scale=2.0)
    kw.update(dict(solver=solver) if solver else dict(ddim_eta=0))
    if guidance == "cfg":
        kw.update(cfg=mdm_hip.CFG(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7))
    want = smp.sample(stub, x, lm, mask, {}, **kw)
    got = smp.sample(stub, x, lm, mask, {}, tiles=tiles, **kw)
    err = TC.rel_l2(got, want)
    print("rel-L2 %.2e" % err)
    assert got.shape == want.shape == (B, 3) + tuple((x[0] if nested else x).shape[2:])
    assert torch.isfinite(got).all() and err < 1e-5
    assert stub.calls == 2 * n
    # tiles=None is the call without the keyword; one window equal to the canvas changes no bit
    assert torch.equal(smp.sample(stub, x, lm, mask, {}, tiles=None, **kw), want)
    H, W = (x[0] if nested else x).shape[2:]
    assert torch.equal(smp.sample(stub, x, lm, mask, {}, tiles=mdm_hip.Tiles((H, W), (H, W), blend), **kw), want)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _refusals():
    import mdm_hip

    guide = mdm_hip.LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    tiles = mdm_hip.Tiles(8, 4)
    graphed_guide = (NotImplementedError,
                     "GraphedSampler does not take guide=: loss-guided sampling calls an arbitrary user function and an "
                     "autograd pass through the denoiser every step, and neither can be captured in a hipGraph; use the eager "
                     "Sampler.sample(..., guide=...)")
    no_tiles = (ValueError, "tiles = 8 (wanted a mdm_hip.Tiles)")
    eta = (ValueError, "cfg = {'eta': 0} (wanted a mdm_hip.CFG)")
    pair = (ValueError, "freeu = (1.4, 0.2) (wanted a mdm_hip.FreeU)")
    pag_cfg = (NotImplementedError,
               "pag_scale != 0 together with cfg=: mdm_pag_combine adds the perturbed-attention term to the plain combine; "
               "projecting, capping and rescaling an update of three predictions is not implemented")
    regions_tiles = (NotImplementedError,
                     "regions= together with tiles=: the bias is laid out per query position of the whole canvas, and "
                     "cropping it per window is not implemented")
    return {
        "guide x tiles": (dict(guide=guide, tiles=tiles),
                          (NotImplementedError, "guide= together with tiles=: the window kernels (mdm_tiles_gather, "
                                                "mdm_tiles_merge) have no backward, so the guide's input gradient cannot pass "
                                                "them"), graphed_guide),
        "regions x tiles": (dict(regions=rp, tiles=tiles), regions_tiles, regions_tiles),
        "tiles type": (dict(tiles=8), no_tiles, no_tiles),
        # the checks for tiles come after all the existing ones
        "cfg type before tiles": (dict(cfg=dict(eta=0), tiles=8), eta, eta),
        "freeu type before tiles": (dict(freeu=(1.4, 0.2), regions=rp, tiles=tiles), pair, pair),
        "pag x cfg before tiles": (dict(pag_scale=1.0, cfg=mdm_hip.CFG(), regions=rp, tiles=tiles), pag_cfg, pag_cfg),
        "tiles type before its pairs": (dict(regions=rp, tiles=8), no_tiles, no_tiles),
    }


REFUSALS = ["guide x tiles", "regions x tiles", "tiles type", "cfg type before tiles", "freeu type before tiles",
            "pag x cfg before tiles", "tiles type before its pairs"]


@pytest.mark.parametrize("name", REFUSALS)
def test_every_entry_point_refuses_alike(name):
    from mdm_hip.graph import GraphedSampler

    assert sorted(REFUSALS) == sorted(_refusals())
    options, eager, graphed = _refusals()[name]
    smp, stub = _sampler(), TC.RecordingStub()
    lm, mask = _text()
    x = torch.randn(B, 3, 8, 8)
    gs = GraphedSampler(types.SimpleNamespace(sampler=smp))   # refuses before it asks its pipeline for anything
    calls = {
        "sample": (eager, lambda: smp.sample(stub, x, lm, mask, {}, resample_steps=True, num_inference_steps=2, ddim_eta=0,
                                             guidance_scale=2.0, **options)),
        "get_xt_minus_1": (eager, lambda: smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, guidance_scale=2.0, **options)),
        "graphed": (graphed, lambda: gs.sample(B, {"lm_outputs": lm, "lm_mask": mask}, 8, torch.device("cpu"),
                                               guidance_scale=2.0, **options)),
    }
    for where, ((cls, message), call) in calls.items():
        with pytest.raises(cls) as err:
            call()
        assert type(err.value) is cls and str(err.value) == message, where
    assert not stub.calls


# ---- start noise -------------------------------------------------------------------------------------------------------------
def test_image_side_may_be_a_pair_and_an_int_draws_what_it_drew():
    from mdm_hip import diffusion as DF

    noise = DF.Diffusion.get_noise(None, 2, 3, (4, 6), "cpu")
    assert noise.shape == (2, 3, 4, 6)
    assert DF.Diffusion.get_noise(None, 2, 3, [5, 2], "cpu").shape == (2, 3, 5, 2)
    torch.manual_seed(5)
    a = DF.Diffusion.get_noise(None, 2, 3, 8, "cpu")
    torch.manual_seed(5)
    assert torch.equal(a, torch.randn(2, 3, 8, 8))
    torch.manual_seed(5)
    assert torch.equal(DF.Diffusion.get_noise(None, 2, 3, (8, 8), "cpu"), a)


def test_output_inner_follows_a_non_square_canvas():
    """the nested sampler's ``output_inner`` lays every scale, resized to the canvas, side by side: H x (scales W)"""
    import mdm_hip

    smp, stub = _sampler(True), TC.PointwiseStub(True)
    lm, mask = _text()
    x = _canvas(True)
    H, W = x[0].shape[2:]
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0, tiles=mdm_hip.Tiles(8, 4))
    plain = smp.sample(stub, x, lm, mask, {}, **kw)
    inner = smp.sample(stub, x, lm, mask, {}, output_inner=True, **kw)
    assert plain.shape == (B, 3, H, W) and inner.shape == (B, 3, H, 2 * W) and torch.equal(inner[..., W:], plain)
    x0, x_t, _ = smp.sample(stub, x, lm, mask, {}, output_inner=True, yield_full=True, **kw)
    assert x0.shape == x_t.shape == (B, 3, H, 2 * W) and torch.equal(x_t, inner)


def test_diffusion_sample_takes_a_canvas():
    """``Diffusion.sample(..., image_side=(H, W), tiles=...)`` end to end on the CPU with the pointwise stub as the pipeline's
    model; the nested sampler's lower-scale start noise follows the canvas"""
    import mdm_hip
    from mdm_hip import diffusion as DF

    for nested in (False, True):
        stub = TC.PointwiseStub(nested)
        stub.input_channels, stub.conditions = 3, None
        pipe = types.SimpleNamespace(sampler=_sampler(nested), get_model=lambda: stub, eval=lambda: None,
                                     get_micro_conditioning=lambda sample: {})
        pipe.get_noise = lambda *a: DF.Diffusion.get_noise(pipe, *a)
        lm, mask = _text(B)
        out = DF.Diffusion.sample(pipe, B, {"lm_outputs": lm, "lm_mask": mask}, (8, 14), "cpu", resample_steps=True,
                                  num_inference_steps=2, ddim_eta=0, tiles=mdm_hip.Tiles(8, 4))
        assert out.shape == (B, 3, 8, 14) and torch.isfinite(out).all() and stub.calls == 2
