"""GPU: SA-Solver on the HIP path -- the mdm_sampler_step_sa kernel against the fp64 restatement of tests/sa_cases.py
(coefficients by quadrature), its bit-for-bit properties, and the eager sampler against the torch-op path and against
GraphedSampler on the mini models.  Image quality under random weights is not judged anywhere here."""
import math

import pytest
import torch

import parity_cases as PC
import sa_cases as SC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RNG_SEED = 21
W_GUIDE = 2.0
CANVAS = {"mini_unet": ((16, 36), 16, 8), "mini_nested": ((32, 56), 32, 16)}   # canvas, window, stride (tests/tiles_cases.py)
NAN = float("nan")


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _sampler(pred="V_PREDICTION", thr="CLIP", **kw):
    from mdm_hip import samplers as S

    return S.Sampler(S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type=pred,
                                     loss_target_type="DDPM", threshold_function=thr, **kw))


def _pt():
    from mdm_hip import samplers as S

    return S.PredictionType.V_PREDICTION


def _gamma(lams):
    """gamma = sigmoid(2 lambda) as the fp32 values the kernel is given"""
    return torch.sigmoid(2 * torch.tensor(lams, dtype=torch.float64)).float()


# per sample: lambda of the node, the step h, h1 = lambda_a - lambda_{a-1}, h2 -- the noisy end, the middle and the clean end
# of the schedule (DEEPFLOYD spans lambda of about -10 .. 5), uneven spacing with ratios up to 3
NODES = [(-5.0, 0.6, 0.3, 0.6), (0.0, 0.25, 0.5, 0.2), (3.5, 1.2, 1.8, 1.8)]


def _case(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    r = lambda: torch.randn(*shape, generator=g)
    c = dict(x_t=r() * 1.3, pc=r(), pu=r(), h0=torch.rand(*shape, generator=g) * 2 - 1, h1=torch.rand(*shape, generator=g) * 2 - 1,
             psum=r() * 0.3, z=r())
    nodes = (NODES * B)[:B]
    c["g"] = _gamma([n[0] for n in nodes])
    c["gl"] = _gamma([n[0] + n[1] for n in nodes])
    c["g0"] = _gamma([n[0] - n[2] for n in nodes])
    c["g1"] = _gamma([n[0] - n[2] - n[3] for n in nodes])
    return c


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


ORDERS = [(p, c) for p in (1, 2, 3) for c in (0, 1, 2, 3)]


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
@pytest.mark.parametrize("thr", ["NONE", "CLIP", "DYNAMIC", "DYNAMIC_IF"])
@pytest.mark.parametrize("cfg,scale", [(1.0, None), (3.0, 2.0)])
@pytest.mark.parametrize("shape", [(3, 3, 20, 20), (2, 3, 4, 4)])
def test_kernel_matches_the_fp64_restatement(pred, thr, cfg, scale, shape):
    """Sampler.get_prediction_xt_last_sa on GPU tensors (one mdm_sampler_step_sa launch; the dynamic thresholds add the x0
    launch and the quantile) == the update restated in fp64 with quadrature coefficients, within 1e-4 of the largest value:
    predictor 1-3 x corrector 0-3 x tau 0 / 0.5 / 1 with given noise, one sample each at the noisy end, the middle and
    the clean end.  The history is moved on: h0 <- x0, h1 <- the h0 given, bit for bit."""
    smp = _sampler(pred, thr).to(DEV)
    c = _case(shape)
    d = _dev(c)
    taus = (0.0, 0.5, 1.0) if shape[2] == 20 else (0.5,)
    m = SC.x0_of(c["x_t"], c["pc"], c["g"], pred, thr, scale or 1.0, c["pu"] if cfg != 1 else None, cfg)
    worst = 0.0
    for p, k in ORDERS:
        for tau in taus:
            gate = (p, k, tau, 0.5 if k else 0.0)
            h0, h1, ps = d["h0"].clone(), d["h1"].clone(), d["psum"].clone()
            x0, xl, _ = smp.get_prediction_xt_last_sa(d["x_t"], d["pc"], d["g"], d["gl"], gate=gate, h0=h0, h1=h1, psum=ps,
                                                      g_h0=d["g0"], g_h1=d["g1"], input_noise=d["z"], clip_fn=smp.clip_sample,
                                                      image_scale=scale, pred_uncond=d["pu"] if cfg != 1 else None,
                                                      guidance_scale=cfg)
            rl, rs = SC.sa_single(c["x_t"], m, c["g"], c["gl"], gate, c["h0"], c["h1"], c["g0"], c["g1"], c["psum"], c["z"])
            errs = relerr(x0, m), relerr(xl, rl), relerr(ps, rs)
            worst = max(worst, *errs)
            assert max(errs) < 1e-4, (gate, errs)
            assert torch.equal(h0, x0) and torch.equal(h1, d["h0"])
    print("worst error %.2e" % worst)


def _probe():
    """every (h, r1, r2) of the grid as one sample of ONE launch; v prediction, no clip, x_t = 0 so that m = -sigma pred"""
    grid = [(h, r1, r2) for h in (1e-4, 1e-3, 1e-2, 0.1, 0.999, 1.0, 2.0, 4.0, 8.0) for r1 in (1 / 3, 1.0, 3.0) for r2 in (1 / 3, 1.0, 3.0)
            if r1 * h * (1 + r2) <= 20]
    la = [1.0 if h < 8 else -3.5 for h, _, _ in grid]
    g = _gamma(la)
    gl = _gamma([a + h for a, (h, _, _) in zip(la, grid)])
    g0 = _gamma([a - r1 * h for a, (h, r1, _) in zip(la, grid)])
    g1 = _gamma([a - r1 * h * (1 + r2) for a, (h, r1, r2) in zip(la, grid)])
    return grid, g, gl, g0, g1, _gamma([a + min(r1 * h, 0.5) for a, (h, r1, _) in zip(la, grid)])


@pytest.mark.parametrize("tau", [0.0, 0.5, 1.0])
def test_device_coefficients_match_quadrature(tau):
    """the coefficients the kernel forms on the device, read back through unit inputs (x_t = 0; one of m, h0, h1 is 1, the
    others 0): 1e-6 relative against quadrature for h in [1e-4, 8], ratios 1/3 .. 3, orders 1-3, predictor and corrector"""
    from mdm_hip import ops

    worst = 0.0
    for order in (1, 2, 3):
        grid, g, gl, g0, g1, gl_c = _probe()
        B = len(grid)
        shape = (B, 1, 2, 2)
        zeros, ones = torch.zeros(shape, device=DEV), torch.ones(shape, device=DEV)
        # m = 1: x_t = 0 and pred = -1 / sigma gives m = fl(...) close to 1; it is read back and divided out
        pred_one = (-1 / (1 - g.double()).sqrt()).float().reshape(-1, 1, 1, 1).expand(shape).contiguous().to(DEV)
        dv = lambda v: v.to(DEV)
        for which in range(order):
            pred = pred_one if which == 0 else zeros
            h0 = ones.clone() if which == 1 else zeros.clone()
            h1 = ones.clone() if which == 2 else zeros.clone()
            # predictor alone
            psum = zeros.clone()
            x0, xl = ops.sampler_step_sa(zeros, pred, dv(g), dv(gl), _pt(), (order, 0, tau, 0.0), h0=h0.clone(),
                                         h1=h1.clone(), psum=psum, g_h0=dv(g0), g_h1=dv(g1), noise=zeros, clip="NONE")
            # corrector of this order (its step a-1 -> a is r1 h of the grid) in front of a first-order step a -> b of about the
            # same length, so that the predictor's term does not swamp it: x_last = cx (alpha_a c^c_j v) + alpha_b c^p_0 m
            x0c, xlc = ops.sampler_step_sa(zeros, pred, dv(g), dv(gl_c), _pt(), (1, order, 0.0, tau), h0=h0.clone(),
                                           h1=h1.clone(), psum=zeros.clone(), g_h0=dv(g0), g_h1=dv(g1), clip="NONE")
            for b, (h, r1, r2) in enumerate(grid):
                ga, gb, gp, gpp, gc = (float(v[b]) for v in (g, gl, g0, g1, gl_c))
                la, lb, lp = SC.lam(ga), SC.lam(gb), SC.lam(gp)
                lpp = SC.lam(gpp) if order == 3 else 0.0
                v = float(x0[b, 0, 0, 0]) if which == 0 else 1.0
                want = SC.quad_coeffs([0.0, lp - la, lpp - la][:order], lb - la, tau)[which]
                got = float(xl[b, 0, 0, 0]) / (math.sqrt(gb) * v)
                wantc = SC.quad_coeffs([la - lp, 0.0, lpp - lp][:order], la - lp, tau)[which]
                cx = math.sqrt((1 - gc) / (1 - ga))
                first = math.sqrt(gc) * -math.expm1(-(SC.lam(gc) - la)) * (v if which == 0 else 0.0)
                gotc = (float(xlc[b, 0, 0, 0]) - first) / (cx * math.sqrt(ga) * v)
                e, ec = abs(got - want) / abs(want), abs(gotc - wantc) / abs(wantc)
                worst = max(worst, e, ec)
                assert e < 1e-6 and ec < 1e-6, (order, which, grid[b], got, want, gotc, wantc)
    print("tau=%g: worst relative error %.2e" % (tau, worst))


def _step(d, gate, smp=None, **kw):
    from mdm_hip import ops

    args = dict(h0=d["h0"].clone(), h1=d["h1"].clone(), psum=d["psum"].clone(), g_h0=d["g0"], g_h1=d["g1"], noise=d["z"],
                pred_uncond=d["pu"], guidance_scale=2.0)
    args.update(kw)
    x0, xl = ops.sampler_step_sa(d["x_t"], d["pc"], d["g"], d["gl"], _pt(), gate, **args)
    return x0, xl, args["h0"], args["h1"], args["psum"]


def test_last_step_is_x0_bit_for_bit():
    """gamma_last == 1 with NaN in h0 / h1 / psum and their gammas, whatever the gate says: x_last == x0, finite, equal to
    the first-order step's x0; no normal is drawn"""
    d = _dev(_case((3, 3, 20, 20)))
    d["gl"] = torch.ones(3, device=DEV)
    for k in ("h0", "h1", "psum", "g0", "g1"):
        d[k] = torch.full_like(d[k], NAN)
    ref, _, *_ = _step(d, (1, 0, 0.0, 0.0), max_predictor=1, max_corrector=0, h0=None, h1=None, psum=None, g_h0=None, g_h1=None)
    for gate in ((1, 0, 0.0, 0.0), (3, 3, 1.0, 1.0), torch.tensor([3.0, 3.0, 1.0, 1.0], device=DEV)):
        x0, xl, h0, _, _ = _step(d, gate)
        assert torch.isfinite(xl).all() and torch.equal(xl, x0) and torch.equal(x0, ref) and torch.equal(h0, x0)


def test_gated_off_orders_ignore_nan_history():
    """the gates select: NaN behind an order that is off reaches no output"""
    d = _dev(_case((3, 3, 20, 20)))
    nan = lambda k: torch.full_like(d[k], NAN)
    # first order, no corrector: nothing of the state is read
    want = _step(d, (1, 0, 0.5, 0.0), max_predictor=1, max_corrector=0, h0=None, h1=None, psum=None, g_h0=None, g_h1=None)
    got = _step(d, (1, 0, 0.5, 0.0), h0=nan("h0"), h1=nan("h1"), psum=nan("psum"), g_h0=nan("g0"), g_h1=nan("g1"))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.isfinite(got[4]).all()
    # second order with a first-order corrector: h1 and its gamma are not read, h0 only by the predictor
    want = _step(d, (2, 1, 0.5, 0.5), max_predictor=2, max_corrector=1, h1=None, g_h1=None)
    got = _step(d, (2, 1, 0.5, 0.5), h1=nan("h1"), g_h1=nan("g1"))
    assert torch.equal(got[1], want[1]) and torch.equal(got[4], want[4]) and torch.isfinite(got[1]).all()
    # a device gate is clamped to the host's ceilings
    hi = _step(d, torch.tensor([3.0, 3.0, 0.5, 0.5], device=DEV), max_predictor=2, max_corrector=1, h1=None, g_h1=None)
    assert torch.equal(hi[1], want[1])


@pytest.mark.parametrize("gate", [(3, 3, 0.5, 0.5), (1, 0, 0.0, 0.0)])
def test_aliasing_repeats_and_rows(gate):
    """x0_out aliasing h0 == separate buffers; a repeat run is identical; a row alone equals that row in its batch; a
    device gate equals the host gate -- all bit for bit"""
    d = _dev(_case((3, 3, 20, 20), seed=9))
    a = _step(d, gate)
    hist = d["h0"].clone()
    b = _step(d, gate, h0=hist, x0_out=hist)
    assert b[0] is hist or b[0].data_ptr() == hist.data_ptr()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, v in zip(a, _step(d, gate)):
        assert torch.equal(u, v)
    for u, v in zip(a, _step(d, torch.tensor(gate, dtype=torch.float32, device=DEV))):
        assert torch.equal(u, v)
    for r in range(3):
        row = {k: v[r:r + 1].contiguous() for k, v in d.items()}
        for u, v in zip(a, _step(row, gate)):
            assert torch.equal(u[r:r + 1], v)


def test_noise_and_the_generator():
    """in-kernel noise == noise= filled by mdm_randn from the same state (the kernel's element numbering is that of
    mdm_sampler_step: batch row and all); tau == 0 leaves the generator untouched, tau > 0 advances it by numel / 4 blocks"""
    from mdm_hip import ops
    from mdm_hip import samplers as S

    d = _dev(_case((3, 3, 20, 20)))
    gate = (3, 3, 0.7, 0.7)
    z = ops.DeviceRng(77, DEV, offset=5).randn(d["x_t"].shape, stream_id=0)
    given = _step(d, gate, noise=z)
    rng = ops.DeviceRng(77, DEV, offset=5)
    drawn = _step(d, gate, noise=None, rng=rng)
    assert torch.equal(given[1], drawn[1]) and int(rng.state[1]) == 5   # the operator itself advances nothing
    assert not torch.equal(given[1], _step(d, (3, 3, 0.0, 0.7))[1])
    smp = _sampler().to(DEV).use_device_rng(77, DEV)
    before = smp.device_rng.state.clone()
    kw = dict(h0=d["h0"].clone(), h1=d["h1"].clone(), psum=d["psum"].clone(), g_h0=d["g0"], g_h1=d["g1"], clip_fn=smp.clip_sample)
    smp.get_prediction_xt_last_sa(d["x_t"], d["pc"], d["g"], d["gl"], gate=(3, 3, 0.0, 0.0), **kw)
    assert torch.equal(smp.device_rng.state, before)
    smp.get_prediction_xt_last_sa(d["x_t"], d["pc"], d["g"], d["gl"], gate=gate, **kw)
    assert int(smp.device_rng.state[1]) == d["x_t"].numel() // 4
    assert S.SASolver(tau=0.0).tau == 0


def test_invalid_arguments_launch_nothing():
    """a status, and h0 / h1 / psum / x0_out as they were"""
    from mdm_hip import _lib, ops

    d = _dev(_case((2, 3, 4, 4)))
    mark = lambda: torch.full_like(d["x_t"], 7.0)
    bad = [dict(max_predictor=4), dict(max_predictor=0), dict(max_corrector=4), dict(max_corrector=-1),
           dict(h1=None), dict(psum=None), dict(g_h0=None), dict(g_h1=None), dict(h0=None), dict(clip="DYNAMIC")]
    for kw in bad:
        bufs = dict(h0=mark(), h1=mark(), psum=mark(), x0_out=mark())
        args = dict(bufs, g_h0=d["g0"], g_h1=d["g1"], noise=d["z"])
        args.update(kw)
        with pytest.raises(_lib.MdmHipError):
            ops.sampler_step_sa(d["x_t"], d["pc"], d["g"], d["gl"], _pt(), (3, 3, 0.5, 0.5), **args)
        assert all(bool((v == 7.0).all()) for v in bufs.values()), kw
    for alias in ("h1", "psum"):   # aliased state
        bufs = dict(h0=mark(), h1=mark(), psum=mark())
        bufs[alias] = bufs["h0"]
        with pytest.raises(_lib.MdmHipError):
            ops.sampler_step_sa(d["x_t"], d["pc"], d["g"], d["gl"], _pt(), (3, 3, 0.5, 0.5), g_h0=d["g0"], g_h1=d["g1"],
                                noise=d["z"], **bufs)
        assert all(bool((v == 7.0).all()) for v in bufs.values())
    with pytest.raises(ValueError):   # a host gate outside 0 .. 3
        ops.sampler_step_sa(d["x_t"], d["pc"], d["g"], d["gl"], _pt(), (4, 0, 0.0, 0.0))
    with pytest.raises(ValueError):
        ops.sampler_step_sa(d["x_t"], d["pc"], d["g"], d["gl"], _pt(), (1, 0, -1.0, 0.0))
    # chw must be a multiple of 4, as for mdm_sampler_step_2m: [2, 3, 5, 7] is refused with a status
    e = _dev(_case((2, 3, 5, 7)))
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_step_sa(e["x_t"], e["pc"], e["g"], e["gl"], _pt(), (1, 0, 0.0, 0.0), max_predictor=1, max_corrector=0)
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_step_2m(e["x_t"], e["pc"], e["g"], e["gl"], _pt())


# ---- the samplers on the mini models ---------------------------------------------------------------------------------
class Setup:
    def __init__(self, name, threshold="CLIP"):
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

    def start(self, seed, hw=None):
        hw = hw or (self.side, self.side)
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, hw[0], hw[1], generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, hw[0] // 2, hw[1] // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, n=6, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, guidance_scale=W_GUIDE, **kw)

    def graphed(self, xs, n=6, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, tuple(xs[0].shape[2:]), torch.device(DEV), num_inference_steps=n,
                                  start_noise=xs, seed=RNG_SEED, guidance_scale=W_GUIDE, **kw)


def _solvers():
    from mdm_hip import samplers as S

    return {"33": S.SASolver(3, 3), "22tau1": S.SASolver(2, 2, tau=1.0), "33interval": S.SASolver(3, 3, tau=0.8, tau_interval=(0.3, 0.7))}


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
@pytest.mark.parametrize("which", ["33", "22tau1"])
def test_eager_sampler_matches_the_torch_op_loop(name, which, monkeypatch):
    """6 steps (orders 1, 2, 3, 3, 3, 1): the eager sampler on the kernel == the same loop on the torch ops of
    get_prediction_xt_last_sa (held to the fp64 restatement by tests/test_sa_solver_host.py), given the same noises;
    the project's 1e-5 rel-L2 gate for restated loops"""
    from mdm_hip import samplers as S

    s = Setup(name)
    solver = _solvers()[which]
    xs = s.start(41)
    g = torch.Generator().manual_seed(5)
    noises = [torch.randn(x.shape, generator=g).to(DEV) for _ in range(6) for x in xs]

    def source():
        it = iter(noises)
        return lambda x: next(it)

    out = s.eager(xs, solver=solver, solver_noise_fn=source())
    monkeypatch.setattr(S.Sampler, "_on_hip", lambda self, x_t, clip_fn: False)
    want = s.eager(xs, solver=solver, solver_noise_fn=source())
    err = O.rel_l2(out, want)
    print("%s %s: rel-L2 %.2e" % (name, which, err))
    assert err < 1e-5 and torch.isfinite(out).all()


GRAPH_CASES = [
    ("mini_unet", "33", {}), ("mini_nested", "33", {}), ("mini_unet", "22tau1", {}), ("mini_nested", "22tau1", {}),
    ("mini_unet", "33interval", {}), ("mini_nested", "33interval", {}),
    ("mini_unet", "22tau1", dict(cfg=True)), ("mini_nested", "33interval", dict(known=True)),
    ("mini_unet", "33", dict(tiles=True)), ("mini_nested", "22tau1", dict(pag=True)),
    ("mini_unet", "33interval", dict(dynamic=True)),
]


@pytest.mark.parametrize("name,which,kw", GRAPH_CASES, ids=["%s-%s%s" % (n, w, "".join("-" + k for k in kw)) for n, w, kw in GRAPH_CASES])
def test_graphed_sampler_equals_eager_sampler(name, which, kw):
    """6 steps, bit for bit, also on a second call with other noise through the cached graph (which must not see the first
    call's history): the gate of every step and the two history times come from device tables, h0 / h1 / psum live in static
    buffers; with tau > 0 both draw from the device generator in the same order; with cfg=, known_images, tiles, PAG and a
    dynamic threshold"""
    import mdm_hip

    s = Setup(name, "DYNAMIC_IF" if kw.get("dynamic") else "CLIP")
    solver = _solvers()[which]
    more, hw = dict(solver=solver), (s.side, s.side)
    if kw.get("tiles"):
        hw, window, stride = CANVAS[name]
        more.update(tiles=mdm_hip.Tiles(window, stride, "uniform"))
    if kw.get("cfg"):
        more.update(cfg=mdm_hip.CFG(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7))
    if kw.get("pag"):
        more.update(pag_scale=1.5)
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed, hw)
        if kw.get("known"):
            g = torch.Generator().manual_seed(seed)
            m = torch.zeros(2, 1, *hw, device=DEV)
            m[..., : hw[1] // 2] = 1
            more.update(known_images=(torch.randn(2, 3, *hw, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)
        want, out = s.eager(xs, **more), s.graphed(xs, **more)
        print("%s %s %s call %d: max-abs %.2e" % (name, which, sorted(kw), rep, float((out - want).abs().max())))
        assert out.shape == (2, 3) + tuple(hw) and torch.isfinite(out).all() and torch.equal(out, want)
        assert len(s.gs._graphs) == 1
    if solver.tau == 0:   # nothing drew: the generator is where the seed put it
        ent = next(iter(s.gs._graphs.values()))
        assert int(ent["rng"].state[1]) == 0


def test_graphed_late_start_and_graph_key():
    """partial_diffusion(graphed=...) restarts the order count at the first replayed row, as the eager sampler does; the
    solver's fields are part of the graph key, "sa" is SASolver(); guide= and resample > 1 are refused"""
    from mdm_hip import samplers as S

    s = Setup("mini_unet")
    xs = s.start(41)
    img = torch.tanh(xs[0])
    kw = dict(resample_steps=True, num_inference_steps=6, guidance_scale=W_GUIDE, solver=S.SASolver(3, 3, tau=0.5), seed=3)
    with torch.no_grad():
        s.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        want = s.pipe.partial_diffusion(img, 600, s.cond, s.mask, torch.device(DEV), **kw)
        out = s.pipe.partial_diffusion(img, 600, s.cond, s.mask, torch.device(DEV), graphed=s.gs, **kw)
    assert torch.equal(out, want)
    a = s.graphed(xs, solver="sa")
    assert torch.equal(a, s.graphed(xs, solver=S.SASolver())) and len(s.gs._graphs) == 2
    s.graphed(xs, solver=S.SASolver(3, 2))
    assert len(s.gs._graphs) == 3
    with pytest.raises(NotImplementedError):
        s.graphed(xs, solver="sa", guide=S.LossGuide(lambda x0: (x0 ** 2).mean(dim=(1, 2, 3))))
    with pytest.raises(ValueError):
        s.graphed(xs, solver="sa", known_images=img, resample=2)
    with pytest.raises(ValueError):
        s.graphed(xs, solver="sa", ddim_eta=0.0)
