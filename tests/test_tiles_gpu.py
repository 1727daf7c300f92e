"""GPU: tiled (MultiDiffusion) sampling on the HIP path -- mdm_tiles_gather (copies: 0 differing elements) and mdm_tiles_merge
(max-abs over max |p| below (n_cover + 3) 2^-23) against the fp64 definition of tests/tiles_cases.py, their exact identities,
refused arguments, the mini models' eager sampler on a canvas against a loop restated here, eager against graphed bit for
bit, tiles=None and a single window against the present sampler bit for bit, and bf16 autocast against the untiled path's
own bf16 error."""
import functools

import pytest
import torch

import parity_cases as PC
import tiles_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tiles(case, blend="uniform"):
    import mdm_hip

    _, H, W, h, w, sy, sx = case
    return mdm_hip.Tiles((h, w), (sy, sx), blend)


def _merge(p, case, blend, **kw):
    from mdm_hip import ops

    _, H, W, h, w, sy, sx = case
    return ops.tiles_merge(p, H, W, (h, w), (sy, sx), blend, **kw)


# ---- the kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reps", TC.REPS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_gather_copies_every_window(case, reps):
    from mdm_hip import ops

    _, H, W, h, w, sy, sx = case
    x, _ = TC.inputs(case, reps)
    got = ops.tiles_gather(x.to(DEV), (h, w), (sy, sx), reps)
    want = TC.gather_ref(x, case, reps)
    assert got.shape == want.shape and int((got.cpu() != want).sum()) == 0
    assert torch.equal(ops.tiles_gather(x.to(DEV), (h, w), (sy, sx), reps), got)


@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("reps", TC.REPS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_merge_matches_the_fp64_definition(case, reps, blend):
    _, p = TC.inputs(case, reps)
    want, count = TC.merged(case, reps, blend)
    n_cover = int(count.max())
    dp = p.to(DEV)
    got = _merge(dp, case, blend)
    err = float((got.cpu().double() - want).abs().max() / p.abs().max())
    print("%s reps %d %s: %.2e, gate %.2e (covering up to %d)" % (TC.case_id(case), reps, blend, err, TC.merge_gate(n_cover),
                                                                  n_cover))
    assert got.shape == want.shape and torch.isfinite(got).all() and err < TC.merge_gate(n_cover)
    assert torch.equal(dp.cpu(), p)   # the input is left alone
    # singly covered pixels are their window's value bit for bit
    single = (count == 1).expand_as(want)
    assert torch.equal(got.cpu()[single], want.float()[single])
    # repeat runs are bit-identical, and a row's bits do not depend on R
    assert torch.equal(_merge(dp, case, blend), got)
    T = len(TC.window_offsets(case))
    for r in (0, got.shape[0] - 1):
        assert torch.equal(_merge(dp[r * T:(r + 1) * T].contiguous(), case, blend)[0], got[r])


@pytest.mark.parametrize("blend", TC.BLENDS)
def test_one_window_and_equal_windows(blend):
    from mdm_hip import ops

    p = torch.randn(4, 3, 16, 20, generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(ops.tiles_merge(p, 16, 20, (16, 20), (16, 20), blend), p)      # one window: out == p
    assert torch.equal(ops.tiles_merge(p, 16, 20, (16, 20), (3, 4), blend), p)
    assert torch.equal(ops.tiles_gather(p, (16, 20), (8, 10), 2), torch.cat([p, p]))
    # the same prediction in every window: that value, within the gate
    for case in TC.CASES:
        B, H, W, h, w, sy, sx = case
        T = len(TC.window_offsets(case))
        _, count = TC.merged(case, 1, blend)
        vals = torch.randn(B, 3, 1, 1, generator=torch.Generator().manual_seed(5))
        rows = vals.repeat_interleave(T, dim=0).expand(B * T, 3, h, w).contiguous().to(DEV)
        got = _merge(rows, case, blend).cpu()
        err = float((got - vals).abs().max() / vals.abs().max())
        assert err < TC.merge_gate(int(count.max())), (case, err)


def _off_by_one_float(t):
    """a copy of ``t`` on the device whose first element sits 4 bytes past a 16-byte boundary: contiguous, misaligned"""
    buf = torch.empty(t.numel() + 1, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("case", [TC.CASES[2], TC.CASES[7]], ids=TC.case_id)
def test_misaligned_tensors_take_the_scalar_path_to_the_same_bits(case):
    """shapes that allow 16-byte accesses, bases that do not: input, output, both"""
    from mdm_hip import ops

    _, H, W, h, w, sy, sx = case
    x, p = TC.inputs(case, 3)
    rows = ops.tiles_gather(x.to(DEV), (h, w), (sy, sx), 3)
    assert torch.equal(ops.tiles_gather(_off_by_one_float(x), (h, w), (sy, sx), 3), rows)
    out = _off_by_one_float(torch.zeros_like(rows))
    assert torch.equal(ops.tiles_gather(x.to(DEV), (h, w), (sy, sx), 3, out=out), rows)
    assert torch.equal(ops.tiles_gather(_off_by_one_float(x), (h, w), (sy, sx), 3, out=out), rows)
    for blend in TC.BLENDS:
        want = _merge(p.to(DEV), case, blend)
        assert torch.equal(_merge(_off_by_one_float(p), case, blend), want)
        out = _off_by_one_float(torch.zeros_like(want))
        assert torch.equal(_merge(p.to(DEV), case, blend, out=out), want)
        assert torch.equal(_merge(_off_by_one_float(p), case, blend, out=out), want)


def test_invalid_arguments_return_a_status_and_launch_nothing():
    from mdm_hip import _lib, ops

    L = _lib.lib()
    B, Cc, H, W, h, w, sy, sx = 2, 3, 8, 12, 8, 8, 4, 4
    T = 2
    x = torch.randn(B, Cc, H, W, device=DEV)
    rows = torch.full((2 * B * T, Cc, h, w), 3.0, device=DEV)
    canvas = torch.full((2 * B, Cc, H, W), 5.0, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()

    def gather(x=x, out=rows, B=B, C=Cc, H=H, W=W, h=h, w=w, sy=sy, sx=sx, reps=2):
        return L.mdm_tiles_gather(ptr(x), ptr(out), B, C, H, W, h, w, sy, sx, reps, ops._stream())

    def merge(p=rows, out=canvas, R=2 * B, C=Cc, H=H, W=W, h=h, w=w, sy=sy, sx=sx, blend=0):
        return L.mdm_tiles_merge(ptr(p), ptr(out), R, C, H, W, h, w, sy, sx, blend, ops._stream())

    for bad in (dict(h=9), dict(w=13), dict(h=0), dict(sy=0), dict(sx=0), dict(sy=9), dict(sx=9), dict(H=0), dict(C=0)):
        assert gather(**bad) < 0 and merge(**bad) < 0, bad
    assert gather(reps=0) < 0 and gather(B=0) < 0 and gather(x=None) < 0 and gather(out=None) < 0 and gather(out=x) < 0
    assert merge(R=0) < 0 and merge(blend=2) < 0 and merge(p=None) < 0 and merge(out=None) < 0 and merge(out=rows) < 0
    torch.cuda.synchronize()
    assert float(rows.min()) == 3.0 == float(rows.max()) and float(canvas.min()) == 5.0 == float(canvas.max())   # nothing ran
    assert gather() == 0 and merge() == 0
    torch.cuda.synchronize()
    case = (B, H, W, h, w, sy, sx)
    assert torch.equal(rows.cpu(), TC.gather_ref(x.cpu(), case, 2))
    want, _ = TC.merge_ref(rows.cpu(), case, "uniform")
    assert float((canvas.cpu().double() - want).abs().max() / rows.abs().max()) < TC.merge_gate(2)
    with pytest.raises(_lib.MdmHipError, match="tiles"):
        ops.tiles_gather(x, (9, 8), (4, 4))
    with pytest.raises(_lib.MdmHipError, match="not rows of"):
        ops.tiles_merge(rows[:3], H, W, (h, w), (sy, sx))
    with pytest.raises(_lib.MdmHipError, match="fp32"):
        ops.tiles_gather(x.double(), (h, w), (sy, sx))
    with pytest.raises(_lib.MdmHipError, match="unknown blend 'cosine'"):
        ops.tiles_merge(rows, H, W, (h, w), (sy, sx), "cosine")


# ---- the samplers --------------------------------------------------------------------------------------------------------
RNG_SEED = 21
W_GUIDE = 2.0
CANVAS = {"mini_unet": ((16, 36), 16, 8), "mini_nested": ((32, 56), 32, 16)}   # canvas, window, stride


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

    def __init__(self, name):
        import mdm_hip
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested, self.w = name, name == "mini_nested", W_GUIDE
        self.pipe = _pipeline(name, PC.build_module(name)[0]).to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].to(DEV), inp["mask"].to(DEV)
        self.cond, self.mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.sample = {"lm_outputs": self.cond, "lm_mask": self.mask}
        self.canvas, window, stride = CANVAS[name]
        self.side = window
        self.tiles = lambda blend="uniform": mdm_hip.Tiles(window, stride, blend)
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed, canvas=None):
        H, W = canvas or self.canvas
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, H, W, generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, H // 2, W // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, n=4, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, guidance_scale=self.w, **kw)

    def graphed(self, xs, n=4, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, tuple(xs[0].shape[2:]), torch.device(DEV), num_inference_steps=n,
                                  start_noise=xs, seed=RNG_SEED, guidance_scale=self.w, **kw)


@functools.lru_cache(maxsize=None)
def _setup(name):
    return Setup(name)


def _fresh(name):
    from mdm_hip.graph import GraphedSampler

    s = _setup(name)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    return s


def _restated(s, xs, n, solver, tiles):
    """The loop of ``Sampler._sample`` under ``tiles=`` written out: the HIP model on every window by itself, sliced out of
    the canvases of every scale, on [uncond | cond]; the torch ``tiling.merge`` of the windows' predictions; and the sampler's
    torch step formulas on the whole canvas (a custom clip_fn keeps GPU tensors off the step kernels)."""
    from mdm_hip import tiling

    smp, model = s.pipe.sampler, s.pipe.get_model()
    clip = lambda x0, sc: smp.clip_sample(x0, sc)
    steps = smp.set_timesteps(n)
    xs = [x.clone() for x in xs]
    B = xs[0].shape[0]
    ratios, image_scales = smp._scale_info(model)
    H, W = xs[0].shape[2:]
    (h, w), (sy, sx) = tiles.window, tiles.stride
    offs = TC.window_offsets((B, H, W, h, w, sy, sx))
    x0_prev = g_prev = None
    with torch.no_grad():
        for i in range(n):
            t = torch.full((2 * B,), int(steps[i]) - 1, dtype=torch.long, device=DEV)
            per_window = []
            for y, u in offs:
                win = [torch.cat([x[:, :, y // r:(y + h) // r, u // r:(u + w) // r]] * 2).contiguous() for x, r in zip(xs, ratios)]
                preds = model(win if s.nested else win[0], t, s.cond, s.mask, {})
                per_window.append([p.float() for p in (preds if s.nested else [preds[0]])])
            g_t, g_s = smp._scale_gammas(model, int(steps[i]), B), smp._scale_gammas(model, int(steps[i + 1]), B)
            second = solver is not None and 0 < i < n - 1
            x0s = []
            for k, r in enumerate(ratios):
                rows = torch.stack([pw[k] for pw in per_window], dim=1).flatten(0, 1)   # row: (block, image), then window
                pu, pc = tiling.merge(rows, tiles.at(r), H // r, W // r).chunk(2)
                if solver is None:
                    x0, xs[k], _ = smp.get_prediction_xt_last(xs[k], pc, g_t[k], g_s[k], clip_fn=clip, ddim_eta=0,
                                                             image_scale=image_scales[k], return_eps=False, pred_uncond=pu,
                                                             guidance_scale=s.w)
                else:
                    x0, xs[k] = smp.get_prediction_xt_last_2m(xs[k], pc, g_t[k], g_s[k], g_prev=g_prev[k] if second else None,
                                                             x0_prev=x0_prev[k] if second else None, second_order=second,
                                                             clip_fn=clip, image_scale=image_scales[k], pred_uncond=pu,
                                                             guidance_scale=s.w)
                x0s.append(x0)
            x0_prev, g_prev = x0s, g_t
        return smp._postprocess(xs if s.nested else xs[0], clip=True)


@pytest.mark.parametrize("solver,n", [(None, 4), ("dpmpp_2m", 3)], ids=["ddim0", "dpmpp_2m"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_eager_sampler_matches_the_restated_loop(name, solver, n):
    """fp32, rel-L2 1e-5 -- the measure every sampler comparison of this suite uses; and the option acts: the tiled image is
    not the one the model makes of the whole canvas in one piece"""
    s = _setup(name)
    xs = s.start(41)
    kw = dict(solver=solver) if solver else dict(ddim_eta=0)
    for blend in TC.BLENDS:
        out = s.eager(xs, n=n, tiles=s.tiles(blend), **kw)
        want = _restated(s, xs, n, solver, s.tiles(blend))
        err = TC.rel_l2(out, want)
        print("%s %s %s: rel-L2 %.2e against the restated loop" % (name, solver, blend, err))
        assert out.shape == (2, 3) + s.canvas and torch.isfinite(out).all() and err < 1e-5
    whole = s.eager(xs, n=n, **kw)
    moved = float((out - whole).abs().max() / whole.abs().max())
    print("%s %s: tiled against the whole canvas in one piece: %.2e" % (name, solver, moved))
    assert moved > 1e-3


@pytest.mark.parametrize("name,kw", [
    ("mini_unet", dict(ddim_eta=0)),
    ("mini_nested", dict(solver="dpmpp_2m", blend="ramp")),
    ("mini_unet", dict(ddim_eta=0, pag_scale=1.5, freeu=True, blend="ramp")),
    ("mini_unet", dict(cfg=True, known=True)),    # ancestral DDPM, projected guidance with momentum, a known half
    ("mini_nested", dict(ddim_eta=0, pag_scale=1.5, pag_layers="all")),
], ids=["unet-ddim0", "nested-dpmpp_2m-ramp", "unet-pag-freeu-ramp", "unet-ddpm-cfg-known", "nested-pag"])
def test_graphed_sampler_equals_eager_sampler(name, kw):
    """bit for bit; also on a second call through the cached graph with other noise"""
    import mdm_hip

    s = _fresh(name)
    H, W = s.canvas
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed)
        more = dict(kw)
        tiles = s.tiles(more.pop("blend", "uniform"))
        if more.pop("known", False):
            g = torch.Generator().manual_seed(seed)
            m = torch.zeros(2, 1, H, W, device=DEV)
            m[..., : W // 2] = 1
            more.update(known_images=(torch.randn(2, 3, H, W, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)
        if more.pop("freeu", False):
            more.update(freeu=mdm_hip.FreeU(b=(1.4, 1.4), s=(0.2, 0.2)))
        if more.pop("cfg", False):
            more.update(cfg=mdm_hip.CFG(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7))
        want, out = s.eager(xs, tiles=tiles, **more), s.graphed(xs, tiles=tiles, **more)
        print("%s %s call %d: rel-L2 %.2e, max-abs %.2e" % (name, sorted(kw), rep, TC.rel_l2(out, want),
                                                          float((out - want).abs().max())))
        assert out.shape == (2, 3, H, W) and torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
    # another blend or stride captures anew, and the graph key holds the tiles
    other = s.graphed(xs, tiles=mdm_hip.Tiles(tiles.window, tiles.window, tiles.blend), **more)
    assert len(s.gs._graphs) == 2 and not torch.equal(other, out)
    assert all(any(isinstance(c, tuple) and c and c[0] == "tiles" for c in key) for key in s.gs._graphs)


def test_graphed_start_noise_follows_the_canvas():
    s = _fresh("mini_nested")
    with torch.no_grad():
        out = s.gs.sample(2, s.sample, s.canvas, torch.device(DEV), num_inference_steps=2, ddim_eta=0, guidance_scale=s.w,
                          tiles=s.tiles())
    assert out.shape == (2, 3) + s.canvas and torch.isfinite(out).all()
    (key,) = s.gs._graphs
    assert key[0] == ((2, 3, 32, 56), (2, 3, 16, 28))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_no_tiles_and_one_window_change_no_bit(name):
    """on the square input the model was made for: tiles=None is the call without the keyword, and one window equal to the
    canvas is the present sampler bit for bit -- eager and graphed"""
    import mdm_hip

    s = _fresh(name)
    xs = s.start(43, (s.side, s.side))
    for kw in (dict(ddim_eta=0), dict(solver="dpmpp_2m", pag_scale=1.5, pag_layers="all")):
        for run in (s.eager, s.graphed):
            want = run(xs, **kw)
            assert torch.equal(run(xs, tiles=None, **kw), want), (run.__name__, kw)
            for blend in TC.BLENDS:
                one = run(xs, tiles=mdm_hip.Tiles(s.side, s.side, blend), **kw)
                assert torch.equal(one, want), (run.__name__, kw, blend)
    keys = list(s.gs._graphs)
    assert len(keys) == 6 and sum(any(isinstance(c, tuple) and c and c[0] == "tiles" for c in k) for k in keys) == 4


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_bf16_autocast_error_is_that_of_the_untiled_path(name):
    """bf16 against fp32 from the same noise, rel-L2: the tiled run on the canvas stays within 1.25 x the untiled run on
    the square input -- the yardstick is the existing path"""
    s = _setup(name)
    errs = {}
    for tag, xs, kw in (("untiled", s.start(45, (s.side, s.side)), dict()), ("tiled", s.start(45), dict(tiles=s.tiles()))):
        ref = s.eager(xs, ddim_eta=0, **kw)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            low = s.eager(xs, ddim_eta=0, **kw)
        assert torch.isfinite(low).all()
        errs[tag] = TC.rel_l2(low, ref)
    print("%s bf16 against fp32: untiled %.3e, tiled %.3e (ratio %.2f)" % (name, errs["untiled"], errs["tiled"],
                                                                         errs["tiled"] / errs["untiled"]))
    assert errs["tiled"] <= 1.25 * errs["untiled"]
