"""GPU: image-conditioned sampling on the HIP path -- the mdm_sampler_known_blend / mdm_sampler_jump kernels against the
fp64 restatements of tests/inpaint_cases.py and the host replay of the device generator (oracle/philox_ref.py), then the
eager sampler and GraphedSampler on the mini models: exact identities (zero mask, full mask, known half), eager against
graphed, the per-scale noise level, the late start and the super-resolution form."""
import functools

import pytest
import torch
import torch.nn.functional as F

import inpaint_cases as IC
import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6   # of the largest value: two fp32 multiply-adds
# (3, 3, 8, 8): 144 vec4s, one partial block; (3, 3, 20, 12): 540 vec4s, a partial last block, planes of 60 vec4s (no multiple
# of the wave) and rows of 3; (2, 3, 1024, 1024): 6.3 M elements, above the 4096 x 256 x 4 that one sweep of the launch
# covers, so the grid-stride loop runs more than once
SHAPES = [(3, 3, 8, 8), (3, 3, 20, 12), (2, 3, 1024, 1024)]
MASKS = ["zero", "one", "binary", "fractional"]
INV = 0.5


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _gammas(B):
    """per sample: the middle of the DEEPFLOYD schedule (t = 500, 80) ... and 1.0 for the last sample"""
    from mdm_hip import samplers as S

    g = S.gammas_squaredcos_cap_v2(1000)
    return torch.tensor([g[500], g[80], 1.0][-B:], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs of one shape, made once and never written: x, known, injected noise, gammas (the last one is 1.0)"""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 1.3
    known = torch.rand(*shape, generator=g) * 2.4 - 1.2
    noise = torch.randn(*shape, generator=g)
    return x, known, noise, _gammas(shape[0])


def _mask(kind, shape, seed=1):
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "zero":
        return torch.zeros(B, 1, H, W)
    if kind == "one":
        return torch.ones(B, 1, H, W)
    m = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
    if kind == "fractional":   # zeros, ones and fractions side by side, also within one 16-byte group
        f = torch.rand(B, 1, H, W, generator=g)
        m = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.4, f, m)
    return m


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_known_blend_matches_the_fp64_restatement(shape, kind):
    from mdm_hip import ops

    x, known, noise, gam = _case(shape)
    mask = _mask(kind, shape)
    want = IC.blend(x, known, mask, gam, INV, noise)
    xd = x.to(DEV).clone()
    out = ops.sampler_known_blend(xd, known.to(DEV), mask.to(DEV), gam.to(DEV), inv_scale=INV, noise=noise.to(DEV))
    assert out.data_ptr() == xd.data_ptr()   # in place
    out = xd.cpu()
    err = relerr(out, want)
    print("%s %s: %.2e" % (shape, kind, err))
    assert err < TOL
    m = mask.expand_as(x)
    assert torch.equal(out[m == 0], x[m == 0])                       # untouched, bit for bit
    last = torch.zeros_like(m, dtype=torch.bool)
    last[-1] = m[-1] == 1                                            # gamma == 1 there
    assert torch.equal(out[last], (known * INV)[last])               # the known image itself


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_jump_matches_the_fp64_restatement(shape):
    """... and the gate selects (off: x_s itself, bit for bit), and x_t_out may alias x_s"""
    from mdm_hip import ops

    x, _, noise, g_s = _case(shape)
    g_t = g_s * torch.tensor([0.6, 0.93, 0.4][-shape[0]:])
    xd, nd, gtd, gsd = x.to(DEV), noise.to(DEV), g_t.to(DEV), g_s.to(DEV)
    out = ops.sampler_jump(xd, gtd, gsd, noise=nd)
    err = relerr(out, IC.jump(x, g_t, g_s, noise))
    print("%s: %.2e" % (shape, err))
    assert err < TOL and torch.equal(xd.cpu(), x)
    on, off = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    assert torch.equal(ops.sampler_jump(xd, gtd, gsd, noise=nd, gate=on), out)
    assert torch.equal(ops.sampler_jump(xd, gtd, gsd, noise=nd, gate=off), xd)
    for gate, want in ((on, out), (off, xd), (None, out)):
        buf = xd.clone()
        assert ops.sampler_jump(buf, gtd, gsd, noise=nd, gate=gate, out=buf).data_ptr() == buf.data_ptr()
        assert torch.equal(buf, want)
    same = ops.sampler_jump(xd, gsd, gsd, noise=nd)   # a = 1: no noise, whatever max(1 - a, 0) rounds to
    assert relerr(same, x) < TOL


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_in_kernel_noise_of_both_entries(shape):
    """drawn in the kernel from DeviceRng(seed, offset) on stream 1 == the injected-noise result for the host replay of
    (seed, offset, stream 1): a function of position only, also under a mask (bound: the one of
    test_in_kernel_noise_of_the_sampler_step)"""
    import philox_ref as P
    from mdm_hip import ops

    x, known, _, gam = _case(shape)
    mask = _mask("fractional", shape).to(DEV)
    gam = (gam * 0.9).to(DEV)
    rng = ops.DeviceRng(77, DEV, offset=5)
    nz = torch.from_numpy(P.normals(x.numel(), 77, 5, 1).reshape(shape)).to(DEV)
    a = ops.sampler_known_blend(x.to(DEV).clone(), known.to(DEV), mask, gam, inv_scale=INV, rng=rng)
    b = ops.sampler_known_blend(x.to(DEV).clone(), known.to(DEV), mask, gam, inv_scale=INV, noise=nz)
    assert relerr(a, b) < 1e-5
    c = ops.sampler_jump(x.to(DEV), gam * 0.5, gam, rng=rng)
    d = ops.sampler_jump(x.to(DEV), gam * 0.5, gam, noise=nz)
    assert relerr(c, d) < 1e-5
    assert int(rng.state[1].item()) == 5   # the wrappers do not advance the generator
    e = ops.sampler_jump(x.to(DEV), gam * 0.5, gam, rng=rng, gate=torch.zeros(1, device=DEV))
    assert torch.equal(e.cpu(), x)


def test_ops_argument_checks():
    from mdm_hip import _lib, ops

    x, known, noise, gam = [v.to(DEV) for v in _case(SHAPES[0])]
    mask = torch.ones(3, 1, 8, 8, device=DEV)
    with pytest.raises(_lib.MdmHipError, match="mask"):
        ops.sampler_known_blend(x.clone(), known, mask.expand(3, 3, 8, 8).contiguous(), gam, noise=noise)
    with pytest.raises(_lib.MdmHipError, match="noise= or rng="):
        ops.sampler_known_blend(x.clone(), known, mask, gam)
    with pytest.raises(_lib.MdmHipError):   # in place: no silent copy of a strided x
        ops.sampler_known_blend(x.transpose(2, 3), known, mask, gam, noise=noise)
    with pytest.raises(_lib.MdmHipError, match="multiple of 4"):
        ops.sampler_known_blend(x[..., :5, :5].contiguous(), known[..., :5, :5].contiguous(), mask[..., :5, :5].contiguous(), gam,
                                noise=noise[..., :5, :5].contiguous())
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_jump(x, gam[:2], gam, noise=noise)
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_jump(x, gam, gam, noise=noise.cpu())


# ---- the samplers on the mini models ---------------------------------------------------------------------
SOLVERS = {"ddpm": {}, "ddim0": dict(ddim_eta=0), "dpmpp_2m": dict(solver="dpmpp_2m")}
RNG_SEED = 21


def _pipeline(name, net, threshold="CLIP"):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                              use_double_loss=True, no_use_residual=True))
    return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


class Setup:
    """one mini pipeline on the GPU with its inputs; ``eager`` / ``graphed`` run 6 steps from the same start noise, the
    ancestral noise of DDPM from the device generator at (RNG_SEED, 0) on both sides"""

    def __init__(self, name, mode):
        from mdm_hip.graph import GraphedSampler

        model, _, _ = PC.build_module(name)
        self.name, self.nested = name, name == "mini_nested"
        self.pipe = _pipeline(name, model, threshold="DYNAMIC_IF" if mode == "dynamic" else "CLIP").to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
        self.kw = dict(guidance_scale=2.5 if mode == "cfg" else 1)
        if mode == "cfg":
            cond, mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.cond, self.mask = cond, mask
        self.sample = {"lm_outputs": cond, "lm_mask": mask}
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, self.side, self.side, generator=g).cuda()]
        if self.nested:
            xs.append(torch.randn(2, 3, self.side // 2, self.side // 2, generator=g).cuda())
        return xs

    def known(self, seed=3, which="half"):
        g = torch.Generator().manual_seed(seed)
        known = (torch.randn(2, 3, self.side, self.side, generator=g) * 0.8).cuda()   # some values beyond [-1, 1]
        m = torch.zeros(2, 1, self.side, self.side, device=DEV)
        if which == "half":
            m[..., : self.side // 2] = 1
        elif which == "one":
            m.fill_(1)
        return known, m

    def eager(self, xs, n=6, model=None, **more):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(model or self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, **dict(self.kw, **more))

    def graphed(self, xs, n=6, **more):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, self.side, torch.device(DEV), num_inference_steps=n, start_noise=xs,
                                  seed=RNG_SEED, **dict(self.kw, **more))


@functools.lru_cache(maxsize=None)
def _setup(name, mode="plain"):
    return Setup(name, mode)


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_zero_full_and_half_masks(name, solver):
    """eager and graphed: an all-zero mask == the same call without known images, bit for bit; an all-one mask ==
    clip(known); a half mask: the known half is the known image, the other half is generated"""
    s = _setup(name)
    xs, kw = s.start(41), SOLVERS[solver]
    half = s.side // 2
    for run in (s.eager, s.graphed):
        free = run(xs, **kw)
        known, zero = s.known(which="zero")
        assert torch.equal(run(xs, known_images=known, known_mask=zero, **kw), free), run.__name__
        _, one = s.known(which="one")
        full = run(xs, known_images=known, known_mask=one, **kw)
        e_full = float((full - known.clamp(-1, 1)).abs().max())
        _, m = s.known()
        out = run(xs, known_images=known, known_mask=m, known_seed=9, **kw)
        e_half = float((out[..., :half] - known.clamp(-1, 1)[..., :half]).abs().max())
        print("%s %s %s: full mask off by %.2e, known half by %.2e" % (name, solver, run.__name__, e_full, e_half))
        assert e_full < TOL and e_half < TOL
        assert torch.isfinite(out).all()
        assert float((out[..., half:] - known.clamp(-1, 1)[..., half:]).abs().max()) > 1e-2
        assert not torch.equal(out[..., half:], free[..., half:])   # the free half follows the known one


@pytest.mark.parametrize("mode", ["plain", "cfg", "dynamic"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_graphed_sampler_matches_eager_sampler(name, mode):
    """ancestral DDPM, a half mask, resample 1 and 2: GraphedSampler (static known buffers, a second static generator,
    repeated table rows and the gated jump) == the eager sampler, also on a second call with other start noise, another
    known image and another known_seed through the cached graph.  Graphs are added only when ``resample`` or the presence
    of known images changes."""
    from mdm_hip.graph import GraphedSampler

    s = _setup(name, mode)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    _, m = s.known()
    for count, resample in ((1, 1), (2, 2)):
        for rep, (seed, kseed) in enumerate(((41, 0), (42, 1234567))):
            xs = s.start(seed)
            known, _ = s.known(seed=seed)
            kw = dict(known_images=known, known_mask=m, resample=resample, known_seed=kseed)
            want, out = s.eager(xs, **kw), s.graphed(xs, **kw)
            err = O.rel_l2(out, want)
            print("%s %s resample %d call %d: rel-L2 %.2e" % (name, mode, resample, rep, err))
            assert err < 1e-6, (resample, rep)
            assert len(s.gs._graphs) == count
    assert O.rel_l2(s.graphed(xs), s.eager(xs)) < 1e-6 and len(s.gs._graphs) == 3
    s.graphed(xs, known_images=known, known_mask=torch.ones_like(m))
    assert len(s.gs._graphs) == 3
    if s.nested:   # a scale without a known image is another graph
        s.graphed(xs, known_images=[known, None])
        assert len(s.gs._graphs) == 4
    with pytest.raises(ValueError):
        s.graphed(xs, resample=2)
    with pytest.raises(ValueError):
        s.graphed(xs, known_images=known, resample=2, solver="dpmpp_2m")


class Recorder:
    """the model as the sampler sees it, recording the state every denoiser call receives (all scales: return_sequence
    shows the top one only)"""

    def __init__(self, model):
        self.model, self.vision_model, self.seen = model, model.vision_model, []

    def __call__(self, x_t, *a, **k):
        self.seen.append([x.clone() for x in x_t])
        return self.model(x_t, *a, **k)


def test_every_scale_is_held_at_its_own_level():
    """mini_nested, full mask: after every step but the last, at every scale, (x - sqrt(g_s) known_i) / sqrt(1 - g_s) is
    the host replay of the known generator -- g_s that scale's SHIFTED target gamma, the draws in launch order (per
    iteration top scale, then inner scale), 1e-4 of the largest value"""
    import philox_ref as P

    s = _setup("mini_nested")
    xs = s.start(41)
    known, one = s.known(which="one")
    rec = Recorder(s.pipe.get_model())
    kseed = 0x1234_5678_9A
    seq = s.eager(xs, model=rec, known_images=known, known_mask=one, known_seed=kseed, ddim_eta=0, return_sequence=True)
    assert len(rec.seen) == 6 and len(seq) == 7
    smp = s.pipe.sampler
    steps = smp.set_timesteps(6)
    ks = [known, F.avg_pool2d(known, 2)]
    shifts = [2, 1]   # nest_ratio + [1]: SNR / 2 at the top scale
    offset = 0
    for j in range(1, 6):
        for i in range(2):
            x = rec.seen[j][i].double().cpu()
            g = IC.shifted(smp.gammas[steps[j]].double().cpu(), shifts[i])
            got = (x - g.sqrt() * ks[i].double().cpu()) / (1 - g).sqrt()
            want = torch.from_numpy(P.normals(x.numel(), kseed, offset, 1).reshape(x.shape)).double()
            offset += x.numel() // 4
            err = float((got - want).abs().max() / want.abs().max())
            print("step %d scale %d: %.2e" % (j, i, err))
            assert err < 1e-4, (j, i)
        assert torch.equal(seq[j], rec.seen[j][0])
    assert float((seq[-1] - known.clamp(-1, 1)).abs().max()) < TOL


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_late_start(name, solver):
    """start_step in the middle of a 6-step schedule: GraphedSampler replays only the remaining rows == the eager
    sampler with t=...; for dpmpp_2m the first replayed row is first order (no history) for this call only -- a full
    trajectory through the same graph afterwards is second order there again"""
    s = _setup(name)
    xs, kw = s.start(43), SOLVERS[solver]
    t0 = int(s.pipe.sampler.set_timesteps(6)[3])
    for t in (t0, t0 + 5):   # on a step of the schedule, and between two
        want, out = s.eager(xs, t=t, **kw), s.graphed(xs, start_step=t, **kw)
        err = O.rel_l2(out, want)
        print("%s %s from t=%d: rel-L2 %.2e" % (name, solver, t, err))
        assert err < 1e-6
    assert O.rel_l2(s.graphed(xs, **kw), s.eager(xs, **kw)) < 1e-6
    known, m = s.known()
    kn = dict(known_images=known, known_mask=m, known_seed=5)
    assert O.rel_l2(s.graphed(xs, start_step=t0, **kn, **kw), s.eager(xs, t=t0, **kn, **kw)) < 1e-6


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_partial_diffusion(name):
    """t = 0 returns clip(images); a mid t equals the sampler started on ops.noise_images of the same seed (per scale: the
    pooled image, its own gamma, the generator advanced in between); graphed=... replays the same steps"""
    from mdm_hip import ops

    s = _setup(name)
    dev = torch.device(DEV)
    images, _ = s.known(seed=8)
    smp = s.pipe.sampler
    kw = dict(resample_steps=True, num_inference_steps=6, ddim_eta=0)
    with torch.no_grad():
        assert torch.equal(s.pipe.partial_diffusion(images, 0, s.cond, s.mask, dev, **kw), images.clamp(-1, 1))
        t0 = int(smp.set_timesteps(6)[3])
        out = s.pipe.partial_diffusion(images, t0 + 3, s.cond, s.mask, dev, seed=17, **kw)
        rng = ops.DeviceRng(17, DEV)
        pyr = [images] + ([ops.avgpool(images, 2)] if s.nested else [])
        gam = smp._scale_gammas(s.pipe.get_model(), t0, 2)
        xs = []
        for img, g in zip(pyr, gam):
            xs.append(ops.noise_images(img, g, rng=rng)[0])
            rng.advance(img.numel())
        want = smp.sample(s.pipe.get_model(), xs if s.nested else xs[0], s.cond, s.mask, {}, t=t0, **kw)
        assert relerr(out, want) < TOL
        gr = s.pipe.partial_diffusion(images, t0 + 3, s.cond, s.mask, dev, seed=17, graphed=s.gs, **kw)
        assert torch.equal(s.pipe.partial_diffusion(images, 0, s.cond, s.mask, dev, graphed=s.gs, **kw), images.clamp(-1, 1))
    assert O.rel_l2(gr, want) < 1e-6
    assert not torch.equal(out, images.clamp(-1, 1)) and torch.isfinite(out).all()


def test_super_resolution_of_a_given_low_resolution_image():
    """mini_nested, known_images=[None, low]: the inner scale of the result carries ``low``, the top scale is generated
    and unmasked; eager and graphed agree"""
    s = _setup("mini_nested")
    xs = s.start(44)
    low = (torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(6)) * 0.6).cuda()
    up = F.interpolate(low.clamp(-1, 1), 32, mode="bilinear")
    free = s.eager(xs, ddim_eta=0, output_inner=True)
    out = s.eager(xs, ddim_eta=0, known_images=[None, low], output_inner=True)
    assert tuple(out.shape) == (2, 3, 32, 64)   # [inner scale upsampled | top scale]
    assert float((out[..., :32] - up).abs().max()) < TOL and float((free[..., :32] - up).abs().max()) > 1e-2
    assert torch.isfinite(out).all() and not torch.equal(out[..., 32:], free[..., 32:])
    top = s.graphed(xs, ddim_eta=0, known_images=[None, low])
    assert O.rel_l2(top, out[..., 32:]) < 1e-6
