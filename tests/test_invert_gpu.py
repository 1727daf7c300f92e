"""GPU: image inversion -- the two kernels of csrc/invert.hip against the fp64 restatements of tests/invert_cases.py, the
replay identity that ties the noise-map kernel to the step kernel, and ``Sampler.invert`` / ``Sampler.noise_maps`` /
``step_noise=`` on the mini models: the eager paths against the same loops on the package's torch ops around the CPU oracle
(tests/test_invert_host.py holds those to the fp64 restatement), and ``GraphedSampler`` against the eager paths bit for bit."""
import pytest
import torch

import dpm_cases as DC
import input_grad_cases as IG
import invert_cases as IC
import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_GUIDE = 3.0
N = 4   # inference steps of the sampler tests
# The schedule of the tests that compare ``invert`` with a restated loop: the first four steps of 32 (nodes 0, 30, 61, 91, 121
# of 1000).  Chosen on the CPU oracle ALONE, by two measurements that do not involve the code under test (guidance 3, the
# image of ``Setup.image``), so that a comparison at the 1e-5 gate says something about the code and not about the loop:
# (a) the fixed-point iteration has to be a contraction there, or K = 3 is not nearer the preimage than K = 1 and any rounding
#     grows: |x(K+1) - x(K)| for K = 1, 2, 3 reads 1.7, 0.37, 0.09 (mini_unet) and 3.6, 1.1, 0.33 (mini_nested); over 4 steps of
#     the whole schedule (to t = 801) it reads 28, 24, 31 and 38, 43, 45 -- these random-weight nets do not converge there;
# (b) relative noise of 3.1e-6 on every denoiser output -- what ``smoke()`` reads for the HIP model against this oracle --
#     has to move the oracle loop's own result by less than a third of the gate: 1.1e-6 / 1.2e-6 (mini_unet, K = 1 / 3) and
#     2.4e-6 / 2.8e-6 (mini_nested); over the whole schedule it moves it by 6.4e-6 / 2.2e-5 and 1.1e-5 / 7.2e-5, which is
#     what the HIP loop then differs by (measured on MI355X: 7.5e-6 / 2.2e-5 and 1.0e-5 / 7.5e-5).
INV = dict(num_inference_steps=32, resample_steps=True, t=130)

# [2,3,8,8]; [3,3,4,4]: 12 float4 per row, so row boundaries fall inside a wave; [2,3,1024,1024]: 1572864 float4 against
# the launch's 4096 blocks x 256 threads = 1048576, so the grid-stride loop runs twice for half of the threads
SHAPES = [(2, 3, 8, 8), (3, 3, 4, 4), (2, 3, 1024, 1024)]
BIG = SHAPES[-1]


def _pt(pred):
    from mdm_hip import samplers as S

    return S.PredictionType[pred]


def _case(shape, seed=3):
    """distinct per-sample gammas: (cleaner, noisier) = (1, .97) -- the image itself --, a wide step, a narrow one"""
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    rnd = lambda s=1.0: torch.randn(shape, generator=g) * s
    gs = torch.tensor([0.9, 1.0, 0.5])[:B]
    gt = torch.tensor([0.3, 0.97, 0.45])[:B]
    return dict(x=rnd(1.2), y=rnd(1.1), pc=rnd(), pu=rnd(), gs=gs, gt=gt)


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _relmax(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


# every combination at the two small shapes; the large one once: the loop bound does not depend on the arithmetic
INVERT_CASES = [(shape, pred, guided) for shape in SHAPES[:2] for pred in ("V_PREDICTION", "DDPM") for guided in (False, True)]
INVERT_CASES.append((BIG, "V_PREDICTION", True))
MAP_CASES = [(shape, pred, thr, scale, guided, eta) for shape in SHAPES[:2] for pred in ("V_PREDICTION", "DDPM")
             for thr, scale in (("NONE", 1.0), ("CLIP", 2.0), ("DYNAMIC", 1.0)) for guided, eta in ((False, None), (True, None), (True, 0.7))]
MAP_CASES.append((BIG, "V_PREDICTION", "CLIP", 2.0, True, None))
_ids = lambda cases: ["-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c) for c in cases]


@pytest.mark.parametrize("shape,pred,guided", INVERT_CASES, ids=_ids(INVERT_CASES))
def test_invert_kernel_matches_the_fp64_restatement(shape, pred, guided):
    """1e-4 of the largest value (the project's gate for the step kernels); measured on MI355X: 4.5e-8 .. 1.8e-7 over the cases"""
    from mdm_hip import ops

    c = _case(shape)
    d = _dev(c)
    kw = dict(pred_uncond=d["pu"], guidance_scale=W_GUIDE) if guided else {}
    out = ops.sampler_invert_step(d["x"], d["pc"], d["gs"], d["gt"], _pt(pred), **kw)
    ref = IC.invert_step_ref(c["x"], c["pc"], c["gs"], c["gt"], pred, c["pu"] if guided else None, W_GUIDE)
    e = _relmax(out, ref)
    print("invert_step %s %s guided=%s: %.2e of the largest value" % (shape, pred, guided, e))
    assert e <= 1e-4
    assert torch.equal(out, ops.sampler_invert_step(d["x"], d["pc"], d["gs"], d["gt"], _pt(pred), **kw))   # repeat runs
    for b in range(shape[0]):   # a row alone has the bits it has in its batch
        kb = dict(pred_uncond=d["pu"][b:b + 1], guidance_scale=W_GUIDE) if guided else {}
        one = ops.sampler_invert_step(d["x"][b:b + 1], d["pc"][b:b + 1], d["gs"][b:b + 1], d["gt"][b:b + 1], _pt(pred), **kb)
        assert torch.equal(one[0], out[b]), b


def _map_args(c, pred, thr, scale, guided, eta):
    """-> (keywords of ops.sampler_noise_map / ops.sampler_step, keywords of the fp64 restatement)"""
    pu = c["pu"] if guided else None
    kw = dict(ddim_eta=eta, clip=thr, image_scale=scale, guidance_scale=W_GUIDE if guided else 1.0)
    if thr == "DYNAMIC":   # the per-sample threshold the three-stage path hands the kernel: the clamped quantile of |x0 scale|
        x0 = IC.x0_ref(c["x"].double(), IC.guided(c["pc"], pu, W_GUIDE), DC._col(c["gt"]), pred) * scale
        kw["thr"] = torch.quantile(x0.reshape(x0.shape[0], -1).abs(), 0.995, dim=1).clamp(min=1, max=100).float().to(DEV)
    ref = dict(pred_type=pred, thr=thr, image_scale=scale, pred_uncond=pu, guidance=W_GUIDE, ddim_eta=eta)
    return kw, ref


@pytest.mark.parametrize("shape,pred,thr,scale,guided,eta", MAP_CASES, ids=_ids(MAP_CASES))
def test_noise_map_kernel_and_one_step_replay(shape, pred, thr, scale, guided, eta):
    """z against the fp64 restatement, 1e-4 of the largest value (measured on MI355X: 6.0e-8 .. 1.4e-7); then
    ``sampler_step(noise=z)`` against x_s: |x - x_s| <= 2^-21 max(1, |x_s|, |mu|) per element -- four roundings of 2^-24 (the
    subtraction, the division, the product, the sum) on quantities bounded by |x_s| + |mu|, times two for contraction
    differences between the two kernels; fp32 numpy reads 2.3 x 2^-24.  Measured on MI355X: 1.6 .. 3.6 x 2^-24 of that
    maximum (0.20 .. 0.45 of the gate) over the cases."""
    from mdm_hip import ops

    c = _case(shape)
    d = _dev(c)
    kw, rkw = _map_args(c, pred, thr, scale, guided, eta)
    if guided:
        kw["pred_uncond"] = d["pu"]
    # a step from the noisier gt to the cleaner gs; row 1 goes to gamma = 1: sigma = 0, z = 0
    z = ops.sampler_noise_map(d["x"], d["y"], d["pc"], d["gt"], d["gs"], _pt(pred), **kw)
    ref = IC.noise_map_ref(c["x"], c["y"], c["pc"], c["gt"], c["gs"], **rkw)
    e = _relmax(z, ref)
    print("noise_map %s %s %s guided=%s eta=%s: %.2e of the largest value" % (shape, pred, thr, guided, eta, e))
    assert e <= 1e-4
    assert float(z[1].abs().max()) == 0.0
    assert torch.equal(z, ops.sampler_noise_map(d["x"], d["y"], d["pc"], d["gt"], d["gs"], _pt(pred), **kw))
    for b in range(shape[0]):
        kb = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in kw.items()}
        one = ops.sampler_noise_map(d["x"][b:b + 1], d["y"][b:b + 1], d["pc"][b:b + 1], d["gt"][b:b + 1], d["gs"][b:b + 1],
                                    _pt(pred), **kb)
        assert torch.equal(one[0], z[b]), b
    # the replay: the step kernel with noise = z lands on x_s
    _, xl = ops.sampler_step(d["x"], d["pc"], d["gt"], d["gs"], _pt(pred), need_noise=True, noise=z, **kw)
    mu, sigma = IC.posterior_ref(c["x"], c["pc"], c["gt"], c["gs"], **rkw)
    on = (sigma > 0).reshape(-1)
    bound = 2.0 ** -21 * torch.maximum(torch.ones_like(mu), torch.maximum(c["y"].double().abs(), mu.abs()))
    err = (xl.double().cpu() - c["y"].double()).abs()
    worst = float((err / bound)[on].max())
    print("  replay: worst |x - x_s| = %.2f x 2^-21 max(1, |x_s|, |mu|)  (%.2f x 2^-24)" % (worst, worst * 8))
    assert worst <= 1.0


def test_bad_arguments_return_a_negative_status():
    from mdm_hip import _lib, ops
    from mdm_hip.ops import _p, _stream

    d = _dev(_case((2, 3, 4, 4)))
    L = _lib.lib()
    out = torch.full_like(d["x"], 7.0)
    inv = lambda **k: L.mdm_sampler_invert_step(*[k.get(n, v) for n, v in (
        ("x", _p(d["x"])), ("p", _p(d["pc"])), ("pu", None), ("w", 1.0), ("gs", _p(d["gs"])), ("gt", _p(d["gt"])), ("out", _p(out)),
        ("B", 2), ("chw", 48), ("pt", 2), ("st", _stream()))])
    assert inv() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    for bad in (dict(x=None), dict(p=None), dict(gs=None), dict(gt=None), dict(out=None), dict(B=0), dict(chw=0), dict(chw=46),
                dict(pt=3), dict(pt=-1), dict(out=_p(d["x"])), dict(out=_p(d["pc"]))):
        assert inv(**bad) < 0, bad
    nm = lambda **k: L.mdm_sampler_noise_map(*[k.get(n, v) for n, v in (
        ("x", _p(d["x"])), ("y", _p(d["y"])), ("p", _p(d["pc"])), ("pu", None), ("w", 1.0), ("g", _p(d["gt"])), ("gl", _p(d["gs"])),
        ("thr", None), ("out", _p(out)), ("B", 2), ("chw", 48), ("pt", 2), ("mode", 0), ("eta", 0.0), ("clip", 1), ("scale", 1.0),
        ("st", _stream()))])
    assert nm() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    for bad in (dict(x=None), dict(y=None), dict(p=None), dict(g=None), dict(gl=None), dict(out=None), dict(B=-1), dict(chw=50),
                dict(pt=5), dict(mode=2), dict(mode=1, eta=0.0), dict(mode=1, eta=-0.5), dict(clip=3), dict(clip=2), dict(scale=0.0),
                dict(out=_p(d["y"]))):
        assert nm(**bad) < 0, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_noise_map(d["x"], d["y"], d["pc"], d["gt"], d["gs"], _pt("DDPM"), ddim_eta=0.0)
    e = _dev(_case((2, 3, 5, 7)))
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_invert_step(e["x"], e["pc"], e["gs"], e["gt"], _pt("DDPM"))


# ---- the samplers on the mini models ---------------------------------------------------------------------------------
class Setup:
    def __init__(self, name, threshold="CLIP"):
        from mdm_hip import diffusion as D
        from mdm_hip import samplers as S
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested = name, name == "mini_nested"
        model, cfg, sd = PC.build_module(name)

        def wrap(net):
            scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                   loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=self.nested,
                                   rescale_signal=1 if self.nested else None)
            if self.nested:
                return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                      use_double_loss=True, no_use_residual=True))
            return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))

        self.pipe, self.cpu = wrap(model).to(torch.device(DEV)), wrap(IG.OracleNet(sd, cfg, self.nested))
        self.pipe.eval(), self.cpu.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"], inp["mask"]
        self.cond1, self.mask1 = cond, mask
        self.cond, self.mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe)
        self.sched = dict(num_inference_steps=N, resample_steps=True)

    def image(self, seed=5):
        return torch.tanh(torch.randn(2, 3, self.side, self.side, generator=torch.Generator().manual_seed(seed)))

    def sample(self, dev=DEV, cond=None):
        cond = self.cond if cond is None else cond
        return {"lm_outputs": cond.to(dev), "lm_mask": self.mask.to(dev)}

    def on(self, pipe, dev):
        return pipe.sampler, pipe.get_model(), self.cond.to(dev), self.mask.to(dev)


def _lists(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


@pytest.fixture(scope="module", params=["mini_unet", "mini_nested"])
def setup(request):
    return Setup(request.param)


@pytest.mark.parametrize("K", [1, 3])
def test_eager_invert_matches_the_cpu_oracle_loop(setup, K):
    """``Sampler.invert`` on the GPU (HIP model, invert kernel) == the same loop on the torch ops around the CPU oracle,
    rel-L2 <= 1e-5 (the project's gate for restated loops).

    The schedule is ``INV`` (the comment there says how it was chosen).  Measured on MI355X: mini_unet 1.1e-6 (K = 1) /
    1.2e-6 (K = 3); mini_nested 1.3e-6, 2.3e-6 (the two scales, K = 1) / 1.5e-6, 2.6e-6 (K = 3)."""
    s = setup
    img = s.image()
    smp, model, cond, mask = s.on(s.pipe, DEV)
    x_t, t = smp.invert(model, img.to(DEV), cond, mask, {}, iterations=K, guidance_scale=W_GUIDE, **INV)
    csmp, cmodel, ccond, cmask = s.on(s.cpu, "cpu")
    want, tw = csmp.invert(cmodel, img, ccond, cmask, {}, iterations=K, guidance_scale=W_GUIDE, **INV)
    assert t == tw == 121
    errs = [O.rel_l2(a.cpu(), b) for a, b in zip(_lists(x_t), _lists(want))]
    print("%s invert K=%d vs the CPU oracle loop: rel-L2 %s" % (s.name, K, ["%.2e" % e for e in errs]))
    assert all(bool(torch.isfinite(a).all()) for a in _lists(x_t))
    assert max(errs) <= 1e-5


@pytest.mark.parametrize("K", [1, 3])
def test_eager_invert_matches_the_torch_op_loop_on_the_same_model(setup, K, monkeypatch):
    """the invert kernel in the loop == the torch ops of ``samplers.invert_step`` in the same loop around the same (HIP)
    model, rel-L2 <= 1e-5, on the schedule ``INV``.  Measured on MI355X: mini_unet 8.6e-7 / 1.2e-6
    (K = 1 / 3); mini_nested 1.0e-6, 1.8e-6 / 1.5e-6, 2.6e-6"""
    from mdm_hip import samplers as S

    s = setup
    img = s.image().to(DEV)
    smp, model, cond, mask = s.on(s.pipe, DEV)
    x_t, _ = smp.invert(model, img, cond, mask, {}, iterations=K, guidance_scale=W_GUIDE, **INV)
    monkeypatch.setattr(S.Sampler, "_on_hip", lambda self, x_t, clip_fn: False)
    want, _ = smp.invert(model, img, cond, mask, {}, iterations=K, guidance_scale=W_GUIDE, **INV)
    errs = [O.rel_l2(a, b) for a, b in zip(_lists(x_t), _lists(want))]
    print("%s invert K=%d vs the torch-op loop on the same model: rel-L2 %s" % (s.name, K, ["%.2e" % e for e in errs]))
    assert max(errs) <= 1e-5


@pytest.mark.parametrize("K", [1, 3])
def test_graphed_invert_equals_eager_invert(setup, K):
    """``GraphedSampler.invert`` == the eager result bit for bit, also with another image through the cached graph and with
    ``t=`` (fewer replays of the same graph); over the whole schedule in 4 steps, and on the schedule ``INV``"""
    s = setup
    smp, model, cond, mask = s.on(s.pipe, DEV)
    a, ta = smp.invert(model, s.image().to(DEV), cond, mask, {}, iterations=K, guidance_scale=W_GUIDE, **INV)
    b, tb = s.gs.invert(s.image().to(DEV), s.sample(), torch.device(DEV), iterations=K, num_inference_steps=INV["num_inference_steps"],
                        guidance_scale=W_GUIDE, t=INV["t"])
    assert ta == tb == 121 and all(torch.equal(p, q) for p, q in zip(_lists(a), _lists(b)))
    graphs = len(s.gs._graphs)
    for seed, tt in ((5, None), (6, None), (5, 600)):
        im = s.image(seed).to(DEV)
        a, ta = smp.invert(model, im, cond, mask, {}, iterations=K, guidance_scale=W_GUIDE, t=tt, **s.sched)
        b, tb = s.gs.invert(im, s.sample(), torch.device(DEV), iterations=K, num_inference_steps=N, guidance_scale=W_GUIDE, t=tt)
        assert ta == tb and all(torch.equal(p, q) for p, q in zip(_lists(a), _lists(b))), (seed, tt)
    assert len(s.gs._graphs) == graphs + 1


def _device_draws(s, seed, n_nodes):
    """the normals ``noise_maps`` draws on the device, regenerated in its documented order -- one ``ops.DeviceRng(seed)``, the
    nodes in sampling order, the scales hi -> lo, advanced by numel each -- as a ``noise_fn`` for the CPU loop"""
    from mdm_hip import ops

    rng = ops.DeviceRng(seed, DEV)
    sides = [s.side, s.side // 2] if s.nested else [s.side]
    draws = [rng.randn((2, 3, side, side)).cpu() for _ in range(n_nodes) for side in sides]   # (randn advances by numel)
    it = iter(draws)
    return lambda x: next(it)


def test_noise_maps_match_the_cpu_oracle_loop(setup):
    """``Sampler.noise_maps`` on the GPU == the same loop on the torch ops around the CPU oracle given the same draws (which
    checks the documented draw order too), rel-L2 <= 1e-5 per map.  Measured on MI355X: 2.5e-6 .. 3.9e-6 (both models)"""
    s = setup
    img = s.image()
    smp, model, cond, mask = s.on(s.pipe, DEV)
    kw = dict(guidance_scale=W_GUIDE, **s.sched)
    x_start, maps = smp.noise_maps(model, img.to(DEV), cond, mask, {}, seed=9, **kw)
    csmp, cmodel, ccond, cmask = s.on(s.cpu, "cpu")
    w_start, w_maps = csmp.noise_maps(cmodel, img, ccond, cmask, {}, noise_fn=_device_draws(s, 9, N), **kw)
    assert len(maps) == len(w_maps) == N
    for a, b in zip(_lists(x_start), _lists(w_start)):
        assert O.rel_l2(a.cpu(), b) <= 1e-6
    errs = []
    for i, (m, w) in enumerate(zip(maps, w_maps)):
        assert (m is None) == (w is None)
        for a, b in zip(m or [], w or []):
            errs.append(O.rel_l2(a.cpu(), b) if float(b.abs().max()) > 0 else float(a.abs().max()))
            print("%s map %d %s: rel-L2 %.2e" % (s.name, i, tuple(a.shape), errs[-1]))
    assert max(errs) <= 1e-5


def test_replay_reproduces_every_node_eager_and_graphed(setup):
    """the eager replay (guidance 3, CLIP) passes through every stored copy, rel-L2 <= 1e-5 (measured on MI355X: 0, 4.7e-8, 2.9e-6, 6.4e-6 /
    0, 4.7e-8, 2.1e-6, 5.0e-6 over the four nodes of mini_unet / mini_nested);
    the graphed replay == the eager one bit for bit, also with other map values through the cached graph; another prompt
    gives another image"""
    s = setup
    img = s.image()
    smp, model, cond, mask = s.on(s.pipe, DEV)
    kw = dict(guidance_scale=W_GUIDE, **s.sched)
    x_start, maps, nodes = smp.noise_maps(model, img.to(DEV), cond, mask, {}, seed=9, return_nodes=True, **kw)
    seq = smp.sample(model, x_start, cond, mask, {}, step_noise=maps, return_sequence=True, **kw)
    for i, n in enumerate(nodes):
        got = _lists(seq[i])[0]
        e = O.rel_l2(got, _lists(smp._postprocess(n))[0] if i else n[0])
        print("%s replay node %d: rel-L2 %.2e" % (s.name, i, e))
        assert e <= 1e-5
    graphs = len(s.gs._graphs)
    other = smp.noise_maps(model, s.image(6).to(DEV), cond, mask, {}, seed=10, **kw)
    for xs, mp in ((x_start, maps), other):
        want = smp.sample(model, [x.clone() for x in xs] if s.nested else xs.clone(), cond, mask, {}, step_noise=mp, **kw)
        out = s.gs.sample(2, s.sample(), s.side, torch.device(DEV), num_inference_steps=N, start_noise=_lists(xs),
                          guidance_scale=W_GUIDE, step_noise=mp)
        assert torch.equal(out, want)
    assert len(s.gs._graphs) == graphs + 1
    # another prompt edits: the same maps, another image
    edit = s.gs.sample(2, s.sample(cond=s.cond.flip(1)), s.side, torch.device(DEV), num_inference_steps=N,
                       start_noise=_lists(x_start), guidance_scale=W_GUIDE, step_noise=maps)
    assert len(s.gs._graphs) == graphs + 1 and not torch.equal(edit, out)
    with pytest.raises(ValueError):
        s.gs.sample(2, s.sample(), s.side, torch.device(DEV), num_inference_steps=N, start_noise=_lists(x_start),
                    guidance_scale=W_GUIDE, step_noise=maps, solver="dpmpp_2m")
    with pytest.raises(ValueError):
        s.gs.sample(2, s.sample(), s.side, torch.device(DEV), num_inference_steps=N, start_noise=_lists(x_start),
                    guidance_scale=W_GUIDE, step_noise=maps[:-1])


def test_pipeline_round_trip_through_the_graph(setup):
    """Diffusion.invert / sample_from with graphed= equal the eager pair bit for bit, both methods, with a late start"""
    s = setup
    img = s.image().to(DEV)
    dev = torch.device(DEV)
    for method, kw in (("ddim", dict(iterations=2)), ("ddpm", dict(seed=4))):
        a = s.pipe.invert(img, s.cond.to(DEV), s.mask.to(DEV), dev, method=method, guidance_scale=W_GUIDE, t=800, **kw, **s.sched)
        b = s.pipe.invert(img, s.cond.to(DEV), s.mask.to(DEV), dev, method=method, graphed=s.gs, guidance_scale=W_GUIDE, t=800,
                          **kw, **s.sched)
        assert a.t == b.t and all(torch.equal(p, q) for p, q in zip(_lists(a.x_t), _lists(b.x_t)))
        want = s.pipe.sample_from(a, s.sample(), dev, guidance_scale=W_GUIDE)
        out = s.pipe.sample_from(b, s.sample(), dev, graphed=s.gs, guidance_scale=W_GUIDE)
        assert torch.equal(out, want) and bool(torch.isfinite(out).all())


def test_attn_maps_recorded_during_invert(setup):
    """one step, one iteration: the recorder sees the one denoiser call of ``invert`` -- the image itself at the first node's
    time -- and holds what ``attn_maps.record`` holds for the same inputs; the graphed call records the same bits"""
    import mdm_hip
    from mdm_hip import attn_maps as AM

    s = setup
    smp, model = s.pipe.sampler, s.pipe.get_model()
    cond, mask = s.cond1.to(DEV), s.mask1.to(DEV)
    img = s.image().to(DEV)
    rec = mdm_hip.AttnMaps(cond.shape[1], 2)
    with torch.no_grad():
        smp.invert(model, img, cond, mask, {}, attn_maps=rec, num_inference_steps=1, resample_steps=True)
        t = int(smp.set_timesteps(1)[0])
        xs = [img] + ([torch.nn.functional.avg_pool2d(img, 2)] if s.nested else [])
        want = mdm_hip.AttnMaps(cond.shape[1], 2)
        with AM.record(model.vision_model, want):
            model(xs if s.nested else xs[0], torch.full((2,), t - 1, dtype=torch.long, device=DEV), cond, mask, {})
    assert rec.counts() == want.counts() and sum(rec.counts().values()) > 0
    for key, m in want.maps().items():
        assert torch.equal(rec.maps()[key], m), key
    grec = mdm_hip.AttnMaps(cond.shape[1], 2)
    s.gs.invert(img, {"lm_outputs": cond, "lm_mask": mask}, torch.device(DEV), num_inference_steps=1, attn_maps=grec)
    assert grec.counts() == want.counts()
    for key, m in want.maps().items():
        assert torch.equal(grec.maps()[key], m), key
    # K = 3: the recorder sees the last iteration of each step only
    rec3 = mdm_hip.AttnMaps(cond.shape[1], 2)
    smp.invert(model, img, cond, mask, {}, attn_maps=rec3, iterations=3, num_inference_steps=1, resample_steps=True)
    assert rec3.counts() == want.counts()


def test_bf16_reproduction(setup):
    """under bf16 autocast: extract the maps, replay them, and compare every replayed node with its stored copy; the error
    (printed) must not exceed what bf16 does to plain DDPM sampling of the same model and steps -- its rel-L2 against the
    fp32 run from the same start and the same device draws, measured here"""
    s = setup
    smp, model, cond, mask = s.on(s.pipe, DEV)
    kw = dict(guidance_scale=W_GUIDE, **s.sched)
    bf16 = lambda: torch.autocast("cuda", dtype=torch.bfloat16)
    with torch.no_grad(), bf16():
        x_start, maps, nodes = smp.noise_maps(model, s.image().to(DEV), cond, mask, {}, seed=9, return_nodes=True, **kw)
        seq = smp.sample(model, x_start, cond, mask, {}, step_noise=maps, return_sequence=True, **kw)
    errs = [O.rel_l2(_lists(seq[i])[0].float(), (_lists(smp._postprocess(n))[0] if i else n[0]).float()) for i, n in enumerate(nodes)]
    runs = []
    for ctx in (bf16, lambda: torch.autocast("cuda", enabled=False)):
        smp.use_device_rng(21, DEV)
        with torch.no_grad(), ctx():
            runs.append(smp.sample(model, [x.clone() for x in x_start] if s.nested else x_start.clone(), cond, mask, {}, **kw))
    smp.device_rng = None
    plain = O.rel_l2(runs[0].float(), runs[1].float())
    print("%s bf16: reproduction rel-L2 per node %s; plain DDPM sampling bf16 vs fp32 %.2e" % (s.name, ["%.2e" % e for e in errs], plain))
    assert max(errs) <= plain
