"""CPU: loss-guided sampling (``LossGuide``) on the stub denoiser in float64 -- the step's gradient against autograd through
a fully differentiable restatement (tests/input_grad_cases.py), the DPS step size, what is left alone, the refusals, the
new C ABI entries -- and the static scans of the stem input-gradient kernel's file."""
import os
import subprocess
import sys

import pytest
import torch

import input_grad_cases as IG
import stub_models as SM
from mdm_hip import LossGuide, _lib
from mdm_hip import diffusion as D
from mdm_hip import samplers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SIDE = 3, 8


def _pipe(prediction, threshold, rescale=None, nested=False):
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type=prediction,
                           loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=nested,
                           rescale_signal=1 if nested else rescale)
    if nested:
        pipe = D.NestedDiffusion(SM.StubNestedUNet(), D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                              use_double_loss=True, no_use_residual=True))
    else:
        pipe = D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
    pipe.model.double()
    pipe.eval()
    return pipe


def _data(cfg_guidance, side=SIDE):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 3, side, side, generator=g, dtype=torch.float64) * 1.3   # some x0 beyond the clip bound
    lm = torch.randn(2 * B if cfg_guidance else B, 4, 6, generator=g, dtype=torch.float64)
    mask = torch.ones(lm.shape[0], 4, dtype=torch.float64)
    target = torch.rand(B, 3, side, side, generator=g, dtype=torch.float64) * 2 - 1
    m = (torch.rand(B, 1, side, side, generator=g) < 0.6).double()
    return x, lm, mask, IG.masked_mse(target, m)


@pytest.mark.parametrize("guidance", [1, 2.5])
@pytest.mark.parametrize("threshold", ["CLIP", "NONE", "DYNAMIC"])
@pytest.mark.parametrize("prediction,rescale", [("DDPM", None), ("V_PREDICTION", None), ("V_PREDICTION", 2.0),
                                                ("V_PREDICTION", 3.0)])   # 3: (1 / s) s does not round-trip to 1
def test_step_gradient_matches_autograd_through_the_restated_step(prediction, rescale, threshold, guidance):
    pipe = _pipe(prediction, threshold, rescale)
    smp, model = pipe.sampler, pipe.get_model()
    x, lm, mask, fn = _data(guidance != 1)
    ts, last = 600, 450
    kw = dict(time_step_last=last, guidance_scale=guidance, ddim_eta=0, return_details=True)
    with torch.no_grad():
        x0_u, xs_u, _ = smp.get_xt_minus_1(model, ts, x, lm, mask, {}, **kw)
        x0_g, xs_g, _ = smp.get_xt_minus_1(model, ts, x, lm, mask, {}, guide=LossGuide(fn, scale=1.0, normalize=False), **kw)
    assert torch.equal(x0_u, x0_g)                # the step itself is unguided
    grad = xs_u - xs_g                            # zeta = 1

    t = torch.full((B,), ts - 1)

    def model_fn(xt):
        if guidance != 1:
            pu, pc = model(torch.cat([xt, xt]), torch.cat([t, t]), lm, mask, {})[0].chunk(2)
            return pc, pu
        return model(xt, t, lm, mask, {})[0], None

    leaf = x.clone().requires_grad_(True)
    g = smp.gammas[ts].double().expand(B)
    IG.restated_step_loss(leaf, model_fn, g, fn, prediction, threshold, rescale or 1.0, guidance).backward()
    err = float((grad - leaf.grad).norm() / leaf.grad.norm())
    assert leaf.grad.norm() > 0 and err < 1e-10, err
    if threshold != "NONE":
        assert float(((x0_u * (rescale or 1.0)).abs() >= 1).double().mean()) > 0   # the clamp acted somewhere


def test_dps_step_size_and_zero_loss():
    """normalize=True: zeta_b = scale / sqrt(loss_b); a sample whose loss is exactly 0 is left alone"""
    pipe = _pipe("V_PREDICTION", "CLIP")
    smp, model = pipe.sampler, pipe.get_model()
    x, lm, mask, fn = _data(False)
    kw = dict(time_step_last=450, guidance_scale=1, ddim_eta=0, return_details=True)
    gate = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)   # sample 1 has loss 0 (and gradient 0 * v)
    gated = lambda x0: fn(x0) * gate
    with torch.no_grad():
        x0, xs_u, _ = smp.get_xt_minus_1(model, 600, x, lm, mask, {}, **kw)
        _, xs_1, _ = smp.get_xt_minus_1(model, 600, x, lm, mask, {}, guide=LossGuide(gated, 1.0, normalize=False), **kw)
        _, xs_n, _ = smp.get_xt_minus_1(model, 600, x, lm, mask, {}, guide=LossGuide(gated, 0.3, normalize=True), **kw)
    loss = gated(x0)
    want = xs_u - (0.3 / loss.sqrt().clamp(min=1e-8)).reshape(-1, 1, 1, 1) * (xs_u - xs_1)
    assert float((xs_n[[0, 2]] - want[[0, 2]]).norm() / (xs_u - xs_n).norm()) < 1e-10
    assert torch.equal(xs_n[1], xs_u[1]) and not torch.equal(xs_n[0], xs_u[0])
    z = LossGuide(fn, 2.0).zeta(torch.tensor([4.0, 0.0, 1e-30]))
    assert z[0] == 1.0 and z[1] == 0.0 and z[2] == 2.0 / 1e-8   # sqrt(loss) is clamped from below by 1e-8


@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("solver", [None, "dpmpp_2m"])
def test_scale_zero_is_the_unguided_trajectory_and_parameters_are_restored(nested, solver):
    pipe = _pipe("V_PREDICTION", "CLIP", nested=nested)
    side = 32 if nested else SIDE
    x, lm, mask, fn = _data(False, side)
    kw = dict(resample_steps=True, num_inference_steps=4, solver=solver, **({} if solver else {"ddim_eta": 0}))
    run = lambda **k: (torch.manual_seed(3), pipe.sampler.sample(pipe.get_model(), x, lm, mask, {}, **kw, **k))[1]
    with torch.no_grad():
        plain, zero, guided = run(), run(guide=LossGuide(fn, scale=0.0)), run(guide=LossGuide(fn, scale=0.05))
    assert torch.equal(plain, zero) and not torch.equal(plain, guided)
    assert all(p.requires_grad for p in pipe.parameters())   # frozen for the call only
    target_err = lambda img: float(fn(img).sum())
    assert target_err(guided) < target_err(plain)             # and the guide does what it is for


def test_clipped_elements_get_no_gradient_at_a_scale_that_does_not_round_trip():
    """float32, image scale 3: a clipped x0 is +-fl(1 / 3) and fl(1 / 3) * 3 need not be 1 -- it still counts as clipped"""
    pipe = _pipe("V_PREDICTION", "CLIP", 3.0)
    pipe.model.float()
    smp, model = pipe.sampler, pipe.get_model()
    x, lm, mask, fn = _data(False)
    x, lm, mask = x.float() * 2, lm.float(), mask.float()
    kw = dict(time_step_last=999, guidance_scale=1, ddim_eta=0, return_details=True)   # g ~ 0: x_s is all x_t ...
    with torch.no_grad():
        x0, xs_u, _ = smp.get_xt_minus_1(model, 1000, x, lm, mask, {}, **kw)
        _, xs_g, _ = smp.get_xt_minus_1(model, 1000, x, lm, mask, {}, guide=LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)),
                                                                                     1.0, normalize=False), **kw)
    clipped = (x0 * 3).abs() >= 1 - 1e-6
    assert 0.05 < float(clipped.float().mean()) < 0.95
    # the direct term a k v m is the only one local to the pixel; J^T of the stub mixes neighbours, so compare against the
    # same call with the clipped elements' gradient removed by hand: a loss that ignores them moves x_s identically
    with torch.no_grad():
        _, xs_h, _ = smp.get_xt_minus_1(model, 1000, x, lm, mask, {}, guide=LossGuide(
            lambda z: (z * (~clipped).float()).pow(2).sum(dim=(1, 2, 3)), 1.0, normalize=False), **kw)
    assert torch.equal(xs_g, xs_h) and not torch.equal(xs_g, xs_u)


def test_parameters_are_handed_back_between_the_items_of_a_yield_output_generator():
    pipe = _pipe("V_PREDICTION", "CLIP")
    x, lm, mask, fn = _data(False)
    with torch.no_grad():
        gen = pipe.sampler.sample(pipe.get_model(), x, lm, mask, {}, resample_steps=True, num_inference_steps=4, ddim_eta=0,
                                  guide=LossGuide(fn, scale=0.05), yield_output=True)
        first = next(gen)
    assert torch.isfinite(first).all()
    assert all(p.requires_grad for p in pipe.parameters())   # the caller stopped early and still holds the generator
    del gen


def test_guided_sampling_with_known_images_keeps_the_known_region():
    pipe = _pipe("V_PREDICTION", "CLIP")
    x, lm, mask, fn = _data(False)
    g = torch.Generator().manual_seed(11)
    known = torch.rand(B, 3, SIDE, SIDE, generator=g, dtype=torch.float64) * 2 - 1
    km = torch.zeros(B, 1, SIDE, SIDE, dtype=torch.float64)
    km[..., :4] = 1
    with torch.no_grad():
        out = pipe.sampler.sample(pipe.get_model(), x, lm, mask, {}, resample_steps=True, num_inference_steps=4, ddim_eta=0,
                                  guide=LossGuide(fn, scale=0.05), known_images=known, known_mask=km)
    assert torch.equal(out[..., :4], known[..., :4])          # step -> guide -> blend: the blend has the last word


def test_refusals():
    from mdm_hip.graph import GraphedSampler

    pipe = _pipe("V_PREDICTION", "CLIP")
    x, lm, mask, fn = _data(False)
    call = lambda guide: pipe.sampler.sample(pipe.get_model(), x, lm, mask, {}, resample_steps=True, num_inference_steps=2,
                                             ddim_eta=0, guide=guide)
    with pytest.raises(TypeError, match="callable"):
        LossGuide(3.0)
    with pytest.raises(TypeError, match="LossGuide"):
        call(fn)                                               # the bare function, not wrapped
    with pytest.raises(ValueError, match="one loss per sample"):
        call(LossGuide(lambda x0: x0.pow(2).sum()))            # a scalar, not [B]
    with pytest.raises(ValueError, match="does not depend on x0"):
        call(LossGuide(lambda x0: torch.ones(x0.shape[0], dtype=x0.dtype)))
    with pytest.raises(NotImplementedError, match="hipGraph"):
        GraphedSampler(pipe).sample(B, {"lm_outputs": lm, "lm_mask": mask}, SIDE, "cpu", guide=LossGuide(fn))
    assert all(p.requires_grad for p in pipe.parameters())   # a refused call leaves the parameters trainable


def test_new_entries_are_declared_and_exported():
    names = {p[0]: p for p in _lib.header_prototypes()}
    for n in ("mdm_conv3x3_stem_dgrad", "mdm_guide_seed", "mdm_guide_apply"):
        assert n in names
    assert len(names["mdm_conv3x3_stem_dgrad"][2]) == 10 and names["mdm_conv3x3_stem_dgrad"][3][-2:] == ["dtype", "stream"]
    assert _lib.ABI_VERSION == 6                              # additive
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        for n in ("mdm_conv3x3_stem_dgrad", "mdm_guide_seed", "mdm_guide_apply"):
            assert hasattr(lib, n)
        # host-side argument checks need no GPU: more than 8 input channels, a channel count off the chunk
        assert lib.mdm_conv3x3_stem_dgrad(1, 1, 1, 1, 4, 4, 32, 9, 1, None) < 0 and b"Cin" in lib.mdm_last_error()
        assert lib.mdm_conv3x3_stem_dgrad(1, 1, 1, 1, 4, 4, 12, 3, 1, None) < 0
        assert lib.mdm_guide_apply(1, None, None, 1, 1, 4, None) < 0


def test_stem_kernel_file_is_scanned_clean():
    """tools/mfma_hazard_scan.py covers csrc/stem.hip; tools/kernel_resources.py: no kernel of it spills"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mfma_hazard_scan.py"), "stem.hip"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "HEAD", "stem.hip"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rows = [l for l in r.stdout.splitlines() if "stem_dgrad_kernel" in l]
    assert len(rows) == 16, r.stdout                          # 8 channel counts x 2 dtypes
    for l in rows:
        vgpr, agpr, spill, scratch, occ, lds = (int(v) for v in l.split()[-6:])
        assert spill == 0 and scratch == 0 and 0 < vgpr <= 128 and lds == 48960, l
