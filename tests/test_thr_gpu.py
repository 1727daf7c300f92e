"""GPU: the dynamic-threshold quantile as a radix select (mdm_abs_quantile) -- the two order statistics against the sort-based
definition of tests/thr_cases.py with 0 differing bits and the threshold within 2 ulp of its fp64 evaluation on every case
of the table; independence of the batch, reproducibility, a dirty workspace and the two load paths bit for bit; rows longer
than ``torch.quantile`` takes; the samplers' step with ``torch.quantile`` taken away; and GraphedSampler against the eager
sampler bit for bit."""
import ctypes
import functools

import pytest
import torch

import parity_cases as PC
import thr_cases as TH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP_GATE = 2   # a[hi] - a[lo], its product with the weight, the sum: three roundings of at most 1/2 ulp each


def _on_device(kind, n, q):
    """[1, n] on the GPU; "misaligned": x[1:] of an aligned buffer (4-byte loads)"""
    x = TH.row(kind, n, q)
    if kind != "misaligned":
        return x.to(DEV)[None]
    buf = torch.empty(n + 1, device=DEV)
    buf[1:] = x.to(DEV)
    out = buf[1:][None]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---- the kernel against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TH.KINDS)
def test_statistics_and_threshold_match_the_definition(kind):
    from mdm_hip import ops

    got, differ_torch, cases = [], 0, 0
    for n in TH.NS:
        for q in TH.QS:
            x = _on_device(kind, n, q)
            thr, stats = ops.abs_quantile(x, q, *TH.CLAMP[q], return_stats=True)
            tq = torch.quantile(x.abs(), q, dim=1).clamp(min=TH.CLAMP[q][0], max=TH.CLAMP[q][1])
            got.append((n, q, thr, stats, tq))
    worst = 0.0
    for n, q, thr, stats, tq in got:
        want_stats, want_thr = TH.expected(kind, n, q)
        assert TH.bits_differ(stats, want_stats) == 0, (kind, n, q, stats.cpu(), want_stats)
        assert torch.equal(thr.cpu().isnan(), want_thr.isnan()), (kind, n, q, thr.cpu(), want_thr)
        off = float(TH.ulps_off(thr, want_thr).max())
        worst = max(worst, off)
        assert off <= ULP_GATE, (kind, n, q, thr.cpu(), want_thr)
        cases += 1
        differ_torch += int(TH.bits_differ(thr.nan_to_num(0.0), tq.nan_to_num(0.0)) != 0)
    print("%s: %d cases, worst %.2f ulp from the fp64 evaluation; %d differ from torch.quantile on the device"
          % (kind, cases, worst, differ_torch))
    if kind == "nan1":
        assert all(bool(thr.isnan().all()) for _, _, thr, _, _ in got)
    if kind == "small":
        assert all(float(thr) == 1.0 for _, _, thr, _, _ in got)
    if kind == "big":
        assert all(float(thr) == TH.CLAMP[q][1] for _, q, thr, _, _ in got)


def test_no_clamp_and_the_ends_of_the_range():
    """cmin / cmax None: the quantile itself; q = 0 and q = 1: the smallest and the largest magnitude"""
    from mdm_hip import ops

    x = _on_device("normal", 4099, 0.95)
    a = x.abs().sort(dim=1).values
    for q, idx in ((0.0, 0), (1.0, -1)):
        thr, stats = ops.abs_quantile(x, q, return_stats=True)
        assert TH.bits_differ(thr, a[:, idx]) == 0 and TH.bits_differ(stats, a[:, [idx, idx]]) == 0
    want_stats, want = TH.definition(x.cpu(), 0.5, float("-inf"), float("inf"))
    thr, stats = ops.abs_quantile(x, 0.5, return_stats=True)
    assert TH.bits_differ(stats, want_stats) == 0 and float(TH.ulps_off(thr, want).max()) <= ULP_GATE
    assert 0.1 < float(thr) < 1.0   # below cmin = 1: nothing was clamped


# ---- independence, reproducibility, the two load paths ---------------------------------------------------------------------
BATCH_KINDS = ("normal", "eighths", "two_bins", "split_mixed", "zeros")


@functools.lru_cache(maxsize=None)
def _batch(n=12288, q=0.95):
    return torch.stack([TH.row(k, n, q) for k in BATCH_KINDS]).to(DEV), q


def test_a_row_alone_equals_the_row_in_a_batch_and_two_runs_agree():
    from mdm_hip import ops

    x, q = _batch()
    thr, stats = ops.abs_quantile(x, q, 1, 1.5, return_stats=True)
    thr2, stats2 = ops.abs_quantile(x, q, 1, 1.5, return_stats=True)
    assert TH.bits_differ(thr, thr2) == 0 and TH.bits_differ(stats, stats2) == 0
    for b in range(x.shape[0]):
        t1, s1 = ops.abs_quantile(x[b:b + 1], q, 1, 1.5, return_stats=True)
        assert TH.bits_differ(t1, thr[b:b + 1]) == 0 and TH.bits_differ(s1, stats[b:b + 1]) == 0, BATCH_KINDS[b]
    want_stats, _ = TH.definition(x.cpu(), q, 1, 1.5)
    assert TH.bits_differ(stats, want_stats) == 0


def test_a_dirty_workspace_changes_nothing():
    from mdm_hip import _lib, ops

    x, q = _batch()
    B, n = x.shape
    L = _lib.lib()
    nbytes = ctypes.c_size_t(0)
    assert L.mdm_abs_quantile_plan(B, n, ctypes.byref(nbytes)) == 0
    outs = []
    for fill in (0, -1):   # -1: every byte 0xFF
        ws = torch.full((nbytes.value // 4,), fill, dtype=torch.int32, device=DEV)
        thr, stats = torch.empty(B, device=DEV), torch.empty(B, 2, device=DEV)
        _lib.check(L.mdm_abs_quantile(x.data_ptr(), ws.data_ptr(), nbytes.value, B, n, q, 1.0, 1.5, thr.data_ptr(),
                                      stats.data_ptr(), ops._stream()), "mdm_abs_quantile")
        outs.append((thr, stats))
    assert TH.bits_differ(outs[0][0], outs[1][0]) == 0 and TH.bits_differ(outs[0][1], outs[1][1]) == 0
    thr, stats = ops.abs_quantile(x, q, 1, 1.5, return_stats=True)
    assert TH.bits_differ(outs[1][0], thr) == 0 and TH.bits_differ(outs[1][1], stats) == 0
    # stats is optional
    thr0 = torch.empty(B, device=DEV)
    ws = torch.empty(nbytes.value // 4, dtype=torch.int32, device=DEV)
    _lib.check(L.mdm_abs_quantile(x.data_ptr(), ws.data_ptr(), nbytes.value, B, n, q, 1.0, 1.5, thr0.data_ptr(), None,
                                  ops._stream()), "mdm_abs_quantile")
    assert TH.bits_differ(thr0, thr) == 0


@pytest.mark.parametrize("n", [768, 12288, 65536 + 4])
def test_scalar_path_equals_vector_path(n):
    from mdm_hip import ops

    q = 0.995
    for kind in ("normal", "eighths"):
        x = TH.row(kind, n, q).to(DEV)
        buf = torch.empty(n + 1, device=DEV)
        buf[1:] = x
        a = ops.abs_quantile(x[None], q, 1, 100, return_stats=True)
        b = ops.abs_quantile(buf[1:][None], q, 1, 100, return_stats=True)
        assert buf[1:].data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
        assert TH.bits_differ(a[0], b[0]) == 0 and TH.bits_differ(a[1], b[1]) == 0


# ---- large rows ----------------------------------------------------------------------------------------------------------------
def _sorted_stats(x, q):
    a = x.abs().sort(dim=1).values
    lo, hi, _ = TH.ranks(x.shape[1], q)
    return torch.stack([a[:, lo], a[:, hi]], dim=1)


@pytest.mark.parametrize("kind", ["normal", "eighths"])
def test_rows_longer_than_torch_quantile_takes(kind):
    from mdm_hip import ops

    n = 2 ** 24 + 4
    x = torch.randn(1, n, device=DEV, generator=torch.Generator(DEV).manual_seed(3)) * 1.3
    if kind == "eighths":
        x = torch.round(x * 8) / 8
    with pytest.raises(RuntimeError, match="too large"):
        torch.quantile(x.abs(), 0.95, dim=1)
    for q in TH.QS:
        thr, stats = ops.abs_quantile(x, q, *TH.CLAMP[q], return_stats=True)
        want = _sorted_stats(x, q)
        assert TH.bits_differ(stats, want) == 0, (q, stats, want)
        assert TH.bits_differ(thr, want[:, 0].clamp(*TH.CLAMP[q])) == 0   # lo == hi above 2^24


def test_two_rows_of_the_nested_top_scale():
    from mdm_hip import ops

    x = torch.randn(2, 3 * 2 ** 20, device=DEV, generator=torch.Generator(DEV).manual_seed(4)) * 0.8
    x[1] = torch.round(x[1] * 8) / 8
    for q in TH.QS:
        thr, stats = ops.abs_quantile(x, q, *TH.CLAMP[q], return_stats=True)
        assert TH.bits_differ(stats, _sorted_stats(x, q)) == 0
        _, want = TH.definition(x, q, *TH.CLAMP[q])
        assert float(TH.ulps_off(thr, want).max()) <= ULP_GATE


# ---- the step --------------------------------------------------------------------------------------------------------------------
def _sampler(thr, pred="V_PREDICTION"):
    from mdm_hip import samplers as S

    return S.Sampler(S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type=pred,
                                     loss_target_type="DDPM", threshold_function=thr)).to(DEV)


def _no_quantile(*a, **kw):
    raise AssertionError("torch.quantile was called on the HIP path")


@pytest.mark.parametrize("fn", ["DYNAMIC", "DYNAMIC_IF"])
def test_step_takes_its_threshold_from_the_kernel(fn, monkeypatch):
    from mdm_hip import ops

    smp = _sampler(fn)
    g = torch.Generator().manual_seed(11)
    x_t, pred = (torch.randn(3, 3, 16, 20, generator=g).to(DEV) * 1.3), torch.randn(3, 3, 16, 20, generator=g).to(DEV)
    t = torch.tensor([700, 31, 999], device=DEV)
    gam, gl = smp.read_gamma(t), smp.read_gamma(t - 25)
    monkeypatch.setattr(torch, "quantile", _no_quantile)
    thr_out = []
    x0, x_last, _ = smp.get_prediction_xt_last(x_t, pred, gam, gl, clip_fn=smp.clip_sample, ddim_eta=0, return_eps=False,
                                               thr_out=thr_out)
    assert torch.isfinite(x0).all() and torch.isfinite(x_last).all()
    x0s, _ = ops.sampler_step(x_t, pred, gam, gl, smp._config.prediction_type, ddim_eta=0, clip="X0_ONLY")
    ratio, vmax = {"DYNAMIC": (0.995, 100), "DYNAMIC_IF": (0.95, 1.5)}[fn]
    assert thr_out[0].shape == (3,) and TH.bits_differ(thr_out[0], ops.abs_quantile(x0s, ratio, 1, vmax)) == 0
    _, want = TH.definition(x0s.reshape(3, -1), ratio, 1, vmax)
    assert float(TH.ulps_off(thr_out[0], want).max()) <= ULP_GATE
    # clip_sample on a GPU tensor takes the same kernel
    got = smp.clip_sample(x0s, 1)
    s = thr_out[0].reshape(-1, 1, 1, 1)
    assert torch.equal(got, torch.clamp(x0s, -s, s) / s)


@pytest.mark.parametrize("fn", ["DYNAMIC", "DYNAMIC_IF"])
def test_step_on_an_image_above_2_to_24_values(fn):
    """[1, 3, 2368, 2368]: 16 822 272 values.  x0 of both updates against the clamp restated in torch ops with the threshold
    of the sort-based definition, to 1e-6 of max |x0|"""
    smp = _sampler(fn)
    gen = torch.Generator(DEV).manual_seed(12)
    shape = (1, 3, 2368, 2368)
    assert 3 * 2368 * 2368 > 2 ** 24
    # x0 = sqrt(g) x_t - sqrt(1 - g) pred has standard deviation 0.6: both quantiles lie inside their clamps
    x_t, pred = torch.randn(shape, device=DEV, generator=gen) * 0.6, torch.randn(shape, device=DEV, generator=gen) * 0.6
    t = torch.tensor([400], device=DEV)
    gam, gl = smp.read_gamma(t), smp.read_gamma(t - 50)
    ratio, vmax = {"DYNAMIC": (0.995, 100), "DYNAMIC_IF": (0.95, 1.5)}[fn]
    x0u = gam.sqrt() * x_t - (1 - gam).sqrt() * pred   # V_PREDICTION
    _, thr = TH.definition(x0u.reshape(1, -1), ratio, 1, vmax)
    s = thr.float().reshape(-1, 1, 1, 1)
    assert 1 < float(s) < vmax
    want = torch.clamp(x0u, -s, s) / s
    del x0u
    x0, x_last, _ = smp.get_prediction_xt_last(x_t, pred, gam, gl, clip_fn=smp.clip_sample, ddim_eta=0, return_eps=False)
    err = float((x0 - want).abs().max() / want.abs().max())
    x0_2m, x_last_2m = smp.get_prediction_xt_last_2m(x_t, pred, gam, gl, clip_fn=smp.clip_sample)
    err_2m = float((x0_2m - want).abs().max() / want.abs().max())
    print("%s: x0 max-abs / max |x0| %.2e (first order) %.2e (2M)" % (fn, err, err_2m))
    assert x0.shape == shape and torch.isfinite(x_last).all() and torch.isfinite(x_last_2m).all()
    assert err <= 1e-6 and err_2m <= 1e-6


# ---- capture and composition ---------------------------------------------------------------------------------------------------
RNG_SEED = 21
W_GUIDE = 2.0
CANVAS = {"mini_unet": ((16, 36), 16, 8), "mini_nested": ((32, 56), 32, 16)}   # canvas, window, stride (tests/tiles_cases.py)


class Setup:
    """one mini pipeline with a dynamic threshold on the GPU, text inputs [uncond | cond], eager and graphed runs from given
    noise (the protocol of the tiled-sampling tests)"""

    def __init__(self, name, threshold):
        from mdm_hip import diffusion as D
        from mdm_hip import samplers as S
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested = name, name == "mini_nested"
        scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                               loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=self.nested,
                               rescale_signal=1 if self.nested else None)
        net = PC.build_module(name)[0]
        if self.nested:
            pipe = D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                  use_double_loss=True, no_use_residual=True))
        else:
            pipe = D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
        self.pipe = pipe.to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].to(DEV), inp["mask"].to(DEV)
        self.cond, self.mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.sample = {"lm_outputs": self.cond, "lm_mask": self.mask}
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed, hw):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, hw[0], hw[1], generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, hw[0] // 2, hw[1] // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, n, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, guidance_scale=W_GUIDE, **kw)

    def graphed(self, xs, n, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, tuple(xs[0].shape[2:]), torch.device(DEV), num_inference_steps=n,
                                  start_noise=xs, seed=RNG_SEED, guidance_scale=W_GUIDE, **kw)


@pytest.mark.parametrize("name,threshold,kw", [
    ("mini_unet", "DYNAMIC_IF", dict(ddim_eta=0)),
    ("mini_nested", "DYNAMIC_IF", dict(ddim_eta=0)),
    ("mini_unet", "DYNAMIC", dict(solver="dpmpp_2m")),
    ("mini_unet", "DYNAMIC_IF", dict(ddim_eta=0, tiles=True)),
], ids=["unet-if", "nested-if", "unet-dynamic-dpmpp_2m", "unet-if-tiles"])
def test_graphed_sampler_equals_eager_sampler(name, threshold, kw, monkeypatch):
    """bit for bit, also on a second call through the cached graph with other noise; ``torch.quantile`` is not there"""
    import mdm_hip

    monkeypatch.setattr(torch, "quantile", _no_quantile)
    s = Setup(name, threshold)
    more = dict(kw)
    hw = (s.side, s.side)
    if more.pop("tiles", False):
        hw, window, stride = CANVAS[name]
        more.update(tiles=mdm_hip.Tiles(window, stride, "uniform"))
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed, hw)
        want, out = s.eager(xs, 4, **more), s.graphed(xs, 4, **more)
        print("%s %s call %d: max-abs %.2e" % (name, sorted(kw), rep, float((out - want).abs().max())))
        assert out.shape == (2, 3) + tuple(hw) and torch.isfinite(out).all() and torch.equal(out, want)
        assert len(s.gs._graphs) == 1
