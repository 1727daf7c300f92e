"""CPU: image-conditioned sampling (``known_images`` / ``known_mask`` / ``resample`` and ``Diffusion.partial_diffusion``) --
the torch-op path of mdm_hip.samplers, which is what CPU tensors take and what the GPU kernels are compared with
(tests/test_inpaint_gpu.py).  The reference has neither feature, so the yardsticks are tests/inpaint_cases.py: the two
per-pixel formulas, the pyramid rule and a reference loop restated in fp64, plus exact identities (the known region of the
result IS the known image; an all-zero mask changes nothing; the denoiser is called (n - 1) r + 1 times)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import dpm_cases as DC
import inpaint_cases as IC
import stub_models as SM

TOL = 1e-6   # of the largest value: two fp32 multiply-adds (the form of bound of the 2M host test)


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def sc(**kw):
    from mdm_hip import samplers as S

    base = dict(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                loss_target_type="DDPM", threshold_function="CLIP")
    base.update(kw)
    return S.SamplerConfig(**base)


class CountingStub(SM.StubUNet):
    calls = 0

    def forward(self, *a, **k):
        self.calls += 1
        return super().forward(*a, **k)


class CountingNestedStub(SM.StubNestedUNet):
    calls = 0

    def forward(self, *a, **k):
        self.calls += 1
        return super().forward(*a, **k)


def _pipe(kind, pred="V_PREDICTION"):
    """-> (pipeline, top side, per-scale (ratio, scale factor of the schedule shift, inv_scale)) for the three sampler
    configurations: plain, rescaled signal (rescale_signal = 2) and nested with a shifted schedule"""
    from mdm_hip import diffusion as D

    if kind == "nested":
        cfg = D.NestedDiffusionConfig(sampler_config=sc(prediction_type=pred, schedule_shifted=True, rescale_signal=1),
                                      use_vdm_loss_weights=False, use_double_loss=True, no_use_residual=True)
        return D.NestedDiffusion(CountingNestedStub(), cfg), 32, [(1, 4, 1.0), (4, 1, 1.0)]
    rs = 2 if kind == "rescaled" else None
    pipe = D.Diffusion(CountingStub(), D.DiffusionConfig(sampler_config=sc(prediction_type=pred, rescale_signal=rs),
                                                         use_vdm_loss_weights=False))
    return pipe, 16, [(1, 1, 0.5 if rs else 1.0)]


def _known(B, side, seed=11, frac=False):
    """a known image with values beyond [-1, 1] (the output is clipped) and a left-half mask"""
    g = torch.Generator().manual_seed(seed)
    known = torch.randn(B, 3, side, side, generator=g) * 0.8
    mask = torch.zeros(B, 1, side, side)
    mask[..., : side // 2] = 1
    if frac:
        mask[..., side // 2: side // 2 + 2] = torch.rand(B, 1, side, 2, generator=g)
    return known, mask


class NoiseTape:
    """known_noise_fn that records what it hands out, in launch order"""

    def __init__(self, seed=5):
        self.g, self.tape = torch.Generator().manual_seed(seed), []

    def __call__(self, x):
        self.tape.append(torch.randn(x.shape, generator=self.g, dtype=x.dtype))
        return self.tape[-1]


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
@pytest.mark.parametrize("kind", ["plain", "rescaled", "nested"])
def test_blend_and_jump_match_the_fp64_restatement(pred, kind):
    """The torch-formula blend and jump as the sampler applies them -- each scale with its own (shifted) target gamma and
    1 / image_scale -- against inpaint_cases.blend / jump, at mid-schedule times and at the last step (gamma = 1); then
    through ``_sample``: the first state of a known-region trajectory is the blend of the first state of the free one."""
    pipe, side, scales = _pipe(kind, pred)
    smp, model = pipe.sampler, pipe.get_model()
    B = 3
    known, mask = _known(B, side, frac=True)
    tape = NoiseTape()
    kr = smp._known_region(model, torch.zeros(B, 3, side, side), known, mask, 0, tape)
    ks, ms = IC.pyramid(known, mask, [r for r, _, _ in scales])
    gen = torch.Generator().manual_seed(2)
    for t, s in [(700, 500), (31, 1), (1, 0)]:
        xs = [torch.randn(B, 3, side // r, side // r, generator=gen) * 1.3 for r, _, _ in scales]
        g_t, g_s = smp._scale_gammas(model, t, B), smp._scale_gammas(model, s, B)
        tape.tape.clear()
        out = kr.blend(xs, g_s)
        back = kr.jump(out, g_t, g_s)
        for i, (r, shift, inv) in enumerate(scales):
            gt, gs = IC.shifted(smp.gammas[t].double(), shift), IC.shifted(smp.gammas[s].double(), shift)
            if s == 0:
                assert float(gs) == 1.0 and bool((g_s[i] == 1).all())
            want = IC.blend(xs[i], ks[i], ms[i], gs.expand(B), inv, tape.tape[i])
            e1 = relerr(out[i], want)
            e2 = relerr(back[i], IC.jump(out[i], gt.expand(B), gs.expand(B), tape.tape[len(scales) + i]))
            print("%s %s t=%d->%d scale %d: blend %.2e jump %.2e" % (kind, pred, t, s, i, e1, e2))
            assert e1 < TOL and e2 < TOL
            assert torch.equal(out[i][(ms[i] == 0).expand_as(xs[i])], xs[i][(ms[i] == 0).expand_as(xs[i])])
            if s == 0:   # gamma = 1: the known image itself, whatever the noise
                sel = (ms[i] == 1).expand_as(xs[i])
                assert torch.equal(out[i][sel], (kr.images[i] * inv)[sel]) and relerr(kr.images[i], ks[i]) < TOL
    # through the sampling loop (top scale): DDIM(0) is deterministic, so the free trajectory's first state is the x_s
    # the known-region one blends.  The nested sampler draws its start pyramid from torch's generator: same seed.
    x_T = torch.randn(B, 3, side, side, generator=gen)
    lm = torch.zeros(B, 2, 4)
    kw = dict(resample_steps=True, num_inference_steps=4, ddim_eta=0, return_sequence=True)
    tape = NoiseTape()
    torch.manual_seed(3)
    free = smp.sample(model, x_T, lm, None, {}, **kw)
    torch.manual_seed(3)
    held = smp.sample(model, x_T, lm, None, {}, known_images=known, known_mask=mask, known_noise_fn=tape, **kw)
    steps = smp.set_timesteps(4)
    r, shift, inv = scales[0]
    want = IC.blend(free[1] * inv, known, mask, IC.shifted(smp.gammas[steps[1]].double(), shift).expand(B), inv, tape.tape[0])
    assert relerr(held[1] * inv, want) < TOL   # the sequence is in output units: x * image_scale


def test_pyramid_rule():
    """a 16x16 mask with ONE unknown pixel gives, at ratio 2, exactly one unknown 8x8 pixel; known low-resolution
    pixels are the block means of the known image; fractions of the top mask count as unknown below"""
    from mdm_hip import samplers as S

    g = torch.Generator().manual_seed(1)
    known = torch.randn(2, 3, 16, 16, generator=g)
    mask = torch.ones(2, 1, 16, 16)
    mask[:, :, 5, 9] = 0
    ks, ms = S.known_pyramid(known, mask, [1, 2])
    assert ms[0] is mask and ks[0] is known
    assert tuple(ms[1].shape) == (2, 1, 8, 8) and int((ms[1] == 0).sum()) == 2 and bool((ms[1][:, :, 2, 4] == 0).all())
    assert set(ms[1].unique().tolist()) == {0.0, 1.0}
    assert torch.equal(ks[1], F.avg_pool2d(known, 2))
    mask[:, :, 12, 0] = 0.75
    for r in (2, 4):
        ks, ms = S.known_pyramid(known, mask, [1, r])
        rk, rm = IC.pyramid(known, mask, [1, r])
        assert torch.equal(ms[1].double(), rm[1]) and relerr(ks[1], rk[1]) < TOL
    assert float(S.known_pyramid(known, mask, [1, 2])[1][1][0, 0, 6, 0]) == 0.0


def _run(pipe, side, B=3, seed=13, **kw):
    g = torch.Generator().manual_seed(7)
    sample = {"lm_outputs": torch.randn(B, 5, 8, generator=g), "lm_mask": torch.ones(B, 5)}
    torch.manual_seed(seed)
    with torch.no_grad():
        return pipe.sample(B, sample, side, torch.device("cpu"), resample_steps=True, num_inference_steps=4, **kw)


SOLVERS = {"ddpm": {}, "ddim0": dict(ddim_eta=0), "dpmpp_2m": dict(solver="dpmpp_2m")}


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("kind", ["plain", "rescaled", "nested"])
def test_known_half_of_the_result_is_the_known_image(solver, kind):
    """stub denoiser, 4 steps, half-image mask: the known half of the output equals clip(known, -1, 1), the other half
    is generated; an all-zero mask changes nothing, bit for bit (the known-region noise never comes from torch's
    global generator, which draws the ancestral noise here); one denoiser call per step"""
    pipe, side, _ = _pipe(kind)
    known, mask = _known(3, side)
    net = pipe.get_model().vision_model
    net.calls = 0
    out = _run(pipe, side, known_images=known, known_mask=mask, **SOLVERS[solver])
    assert net.calls == 4
    half = side // 2
    err = float((out[..., :half] - known.clamp(-1, 1)[..., :half]).abs().max())
    print("%s %s: known half off by %.2e" % (kind, solver, err))
    assert err < TOL
    assert torch.isfinite(out).all() and float((out[..., half:] - known.clamp(-1, 1)[..., half:]).abs().max()) > 1e-2
    free = _run(pipe, side, **SOLVERS[solver])
    assert torch.equal(_run(pipe, side, known_images=known, known_mask=torch.zeros_like(mask), **SOLVERS[solver]), free)
    assert not torch.equal(out, free)   # the keywords are no longer swallowed


@pytest.mark.parametrize("kind", ["plain", "nested"])
def test_resampling_calls_the_denoiser_n_minus_1_times_r_plus_1(kind):
    pipe, side, _ = _pipe(kind)
    known, mask = _known(3, side)
    net = pipe.get_model().vision_model
    for extra in ({}, dict(ddim_eta=0)):
        net.calls = 0
        out = _run(pipe, side, known_images=known, known_mask=mask, resample=3, **extra)
        assert net.calls == (4 - 1) * 3 + 1
        assert float((out[..., : side // 2] - known.clamp(-1, 1)[..., : side // 2]).abs().max()) < TOL
    assert not torch.equal(out, _run(pipe, side, known_images=known, known_mask=mask, ddim_eta=0))


@pytest.mark.parametrize("resample", [1, 2])
def test_sampling_loop_matches_the_reference_loop(resample):
    """fp64 sampler, exact Gaussian denoiser, DDIM(0), injected known-region normals: every state of the trajectory ==
    inpaint_cases.reference_loop -- blend after every step at the step's target gamma, r repetitions with a jump in
    between on all steps but the last, one normal per blend then one per jump"""
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(threshold_function="NONE")).double()
    model = D.Model(DC.GaussianDenoiser(smp.gammas))
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    known, mask = _known(2, 8, frac=True)
    known, mask = known.double() * 0.5, mask.double()
    n = 5
    steps = [int(s) for s in smp.set_timesteps(n)]
    tape = NoiseTape()
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, resample_steps=True, num_inference_steps=n, ddim_eta=0,
                         return_sequence=True, known_images=known, known_mask=mask, resample=resample, known_noise_fn=tape)
    assert len(tape.tape) == n + (n - 1) * (resample - 1) * 2 and len(seq) == n + 1
    want = IC.reference_loop(x_T, smp.gammas, steps, DC.gaussian_v, known, mask, tape.tape, resample)
    for a, b in zip(seq[1:-1], want[:-1]):
        assert relerr(a, b) < 1e-9
    assert relerr(seq[-1], want[-1].clamp(-1, 1)) < 1e-9


def test_nested_list_form_is_super_resolution():
    """known_images=[None, low]: the inner scale of the result carries ``low``, the top scale is generated; a None mask
    beside a given image means all ones"""
    pipe, side, _ = _pipe("nested")
    low = torch.randn(3, 3, side // 4, side // 4, generator=torch.Generator().manual_seed(2)) * 0.5
    out = _run(pipe, side, known_images=[None, low], ddim_eta=0, output_inner=True)
    up = F.interpolate(low.clamp(-1, 1), side, mode="bilinear")
    assert tuple(out.shape) == (3, 3, side, 2 * side)   # [inner upsampled | top]
    assert float((out[..., :side] - up).abs().max()) < TOL
    free = _run(pipe, side, ddim_eta=0, output_inner=True)
    assert torch.isfinite(out).all() and float((free[..., :side] - up).abs().max()) > 1e-2


def test_partial_diffusion_on_cpu():
    """t = 0 returns clip(images); a mid t starts at the first schedule step <= t from images noised to THAT step's gamma
    and equals ``sample(t=...)`` on the same noised images"""
    pipe, side, _ = _pipe("plain")
    g = torch.Generator().manual_seed(4)
    images = torch.randn(3, 3, side, side, generator=g) * 0.7
    lm, lmm = torch.randn(3, 5, 8, generator=g), torch.ones(3, 5)
    noise = torch.randn(3, 3, side, side, generator=g)
    kw = dict(resample_steps=True, num_inference_steps=6, ddim_eta=0)
    with torch.no_grad():
        assert torch.equal(pipe.partial_diffusion(images, 0, lm, lmm, torch.device("cpu"), **kw), images.clamp(-1, 1))
        steps = pipe.sampler.set_timesteps(6)
        t0 = int(steps[3])
        net = pipe.get_model().vision_model
        net.calls = 0
        out = pipe.partial_diffusion(images, t0 + 7, lm, lmm, torch.device("cpu"), noise_fn=lambda x: noise, **kw)
        assert net.calls == 3
        gam = pipe.sampler.gammas[t0]
        x_t = gam.sqrt() * images + (1 - gam).sqrt() * noise
        want = pipe.sampler.sample(pipe.get_model(), x_t, lm, lmm, {}, t=t0, **kw)
    assert torch.equal(out, want)


def test_argument_errors():
    from mdm_hip import _lib, ops

    pipe, side, _ = _pipe("plain")
    known, mask = _known(3, side)
    with pytest.raises(ValueError, match="known_images"):
        _run(pipe, side, resample=2)
    with pytest.raises(ValueError, match="history"):
        _run(pipe, side, known_images=known, known_mask=mask, resample=2, solver="dpmpp_2m")
    with pytest.raises(ValueError):   # raised at the call, not at the generator's first next()
        pipe.sampler.sample(pipe.get_model(), torch.zeros(3, 3, side, side), None, None, {}, yield_output=True, resample=2)
    for bad in (mask[:, 0], mask.expand(3, 3, side, side), mask[..., :-1], mask[:2]):
        with pytest.raises(ValueError, match="mask"):
            _run(pipe, side, known_images=known, known_mask=bad)
    with pytest.raises(ValueError, match="known image"):
        _run(pipe, side, known_images=known[..., :-4], known_mask=mask)
    with pytest.raises(ValueError, match="without known_images"):
        _run(pipe, side, known_mask=mask)
    with pytest.raises(ValueError, match="multiple of 4"):   # H * W % 4: the blend kernel works on 16-byte groups
        _run(pipe, 5, known_images=torch.zeros(3, 3, 5, 5))
    # the operators: shapes are checked first, and they have no CPU path
    x = torch.zeros(3, 3, 8, 8)
    g1 = torch.full((3,), 0.5)
    with pytest.raises(_lib.MdmHipError, match="mask"):
        ops.sampler_known_blend(x, x.clone(), torch.ones(3, 3, 8, 8), g1, noise=x.clone())
    with pytest.raises(_lib.MdmHipError, match="multiple of 4"):
        ops.sampler_known_blend(x[..., :5, :5].contiguous(), x[..., :5, :5].contiguous(), torch.ones(3, 1, 5, 5), g1, noise=x[..., :5, :5].contiguous())
    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.sampler_known_blend(x, x.clone(), torch.ones(3, 1, 8, 8), g1, noise=x.clone())
    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.sampler_jump(x, g1, g1, noise=x.clone())
    # the C entries refuse before they launch (the pointers are never followed)
    L = _lib.lib()
    buf = ctypes.addressof(ctypes.create_string_buffer(64))
    assert L.mdm_sampler_known_blend(buf, buf + 16, buf + 32, buf + 48, 1.0, buf + 32, None, 1, 1, 3, 25, None) < 0
    assert b"hw % 4" in L.mdm_last_error()
    assert L.mdm_sampler_known_blend(buf, buf + 16, buf + 32, buf + 48, 1.0, None, None, 1, 1, 3, 16, None) < 0
    assert L.mdm_sampler_jump(buf, buf + 16, buf + 16, None, None, None, 1, buf, 1, 48, None) < 0
    assert L.mdm_sampler_jump(buf, buf + 16, buf + 16, buf + 32, None, None, 1, buf, 1, 50, None) < 0


def test_new_entries_are_declared_and_exported():
    from mdm_hip import _lib

    names = [p[0] for p in _lib.header_prototypes()]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("mdm_sampler_known_blend", "mdm_sampler_jump"):
        assert n in names and hasattr(handle, n)
    assert _lib.lib().mdm_abi_version() == _lib.ABI_VERSION == 6
