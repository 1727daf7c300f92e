"""CPU: the DPM-Solver++(2M) sampler (``solver="dpmpp_2m"``) -- the torch-op path of mdm_hip.samplers, which is also what
the GPU kernel is compared with (tests/test_dpm_solver_gpu.py).  The reference has no such solver, so the yardsticks are
tests/dpm_cases.py: the published update restated in fp64, the closed-form probability-flow solution for Gaussian data,
and the identity "first order == DDIM(eta = 0)" that ties the new path to code pinned to the reference's goldens."""
import math

import pytest
import torch

import dpm_cases as DC
import stub_models as SM


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def sc(**kw):
    from mdm_hip import samplers as S

    base = dict(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                loss_target_type="DDPM", threshold_function="CLIP")
    base.update(kw)
    return S.SamplerConfig(**base)


class FixedPrediction:
    """a 'model' for get_xt_minus_1 that returns given tensors: [uncond | cond] when the batch arrives doubled"""

    def __init__(self, pc, pu):
        self.pc, self.pu = pc, pu

    def __call__(self, x_t, times, lm_outputs, lm_mask, micros={}):
        out = torch.cat([self.pu, self.pc]) if x_t.shape[0] == 2 * self.pc.shape[0] else self.pc
        return out, torch.ones_like(out)


# (time, target time, time of the step before): the noisy end, the middle and the clean end of the 1000-step schedule.
# The noisy end is t = 999 as in test_sampler_step_matches_reference_formulas (tests/test_diffusion_ops_gpu.py), whose
# comment explains the amplification of fp32 rounding there; (1, 0) is the last step of every schedule (gamma_s = 1).
SECOND = [(999, 959, 1000), (500, 470, 540), (2, 1, 5)]
FIRST = SECOND + [(1, 0, None)]


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
@pytest.mark.parametrize("thr", ["NONE", "CLIP", "DYNAMIC", "DYNAMIC_IF"])
@pytest.mark.parametrize("cfg,scale", [(1.0, None), (3.0, 2.0)])
@pytest.mark.parametrize("second", [False, True])
def test_update_matches_the_fp64_restatement(pred, thr, cfg, scale, second):
    """get_xt_minus_1(solver="dpmpp_2m") on CPU tensors (fp32 torch ops) == the published update in fp64, 1e-4 of the
    largest value (the project's gate for the step formulas in fp32)."""
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(prediction_type=pred, threshold_function=thr, rescale_signal=scale))
    gen = torch.Generator().manual_seed(3)
    B, H = 3, 20
    x_t = torch.randn(B, 3, H, H, generator=gen) * 1.3
    pc, pu = torch.randn(B, 3, H, H, generator=gen), torch.randn(B, 3, H, H, generator=gen)
    x0_prev = torch.rand(B, 3, H, H, generator=gen) * 2 - 1
    lm = torch.zeros(B if cfg == 1 else 2 * B, 2, 4)
    for t, s, p in (SECOND if second else FIRST):
        state = {"x0": x0_prev, "g": smp.read_gamma(torch.full((B,), p))} if second else {}
        x0, x_s, _ = smp.get_xt_minus_1(FixedPrediction(pc, pu), t, x_t, lm, None, {}, time_step_last=s,
                                        guidance_scale=cfg, return_details=True, solver="dpmpp_2m",
                                        solver_state=state, second_order=second)
        gam = smp.gammas.double()
        r0, rs = DC.dpmpp_2m_update(x_t, pc, gam[t].expand(B), gam[s].expand(B), gam[p].expand(B) if second else None,
                                    x0_prev, second, pred, thr, scale or 1.0, pu if cfg != 1 else None, cfg)
        e0, es = relerr(x0, r0), relerr(x_s, rs)
        print("t=%d -> %d: x0 %.2e x_s %.2e" % (t, s, e0, es))
        assert state["x0"] is x0 and torch.equal(state["g"], smp.read_gamma(torch.full((B,), t)))   # history moved on
        assert e0 < 1e-4 and es < 1e-4, (t, s, e0, es)
        if s == 0:
            assert torch.equal(x_s, x0)   # the last step is a plain denoise


def _pipes(nested):
    from mdm_hip import diffusion as D

    if nested:
        cfg = D.NestedDiffusionConfig(sampler_config=sc(schedule_shifted=True, rescale_signal=1), use_vdm_loss_weights=False,
                                      use_double_loss=True, no_use_residual=True)
        return D.NestedDiffusion(SM.StubNestedUNet(), cfg), 32
    return D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=sc(), use_vdm_loss_weights=False)), 16


def _sample(pipe, side, seed=13, **kw):
    g = torch.Generator().manual_seed(7)
    sample = {"lm_outputs": torch.randn(3, 5, 8, generator=g), "lm_mask": torch.ones(3, 5)}
    torch.manual_seed(seed)
    with torch.no_grad():
        return pipe.sample(3, sample, side, torch.device("cpu"), resample_steps=True, **kw)


@pytest.mark.parametrize("nested", [False, True])
def test_first_order_is_ddim(nested):
    """Diffusion.sample(solver="dpmpp_2m") with 1 and 2 steps has no second-order step (first, last) and must equal
    DDIM(eta = 0), which the host goldens pin to the reference.  With 6 steps four steps are second order and the two
    solvers must differ by more than the same gate -- measured: 1.5e-1 (Sampler), 1.4e-1 (NestedSampler) of the largest
    value (the stub denoiser is far from a posterior mean, so its x0 moves a lot from step to step)."""
    pipe, side = _pipes(nested)
    for n in (1, 2):
        a = _sample(pipe, side, num_inference_steps=n, solver="dpmpp_2m")
        b = _sample(pipe, side, num_inference_steps=n, ddim_eta=0)
        assert relerr(a, b) < 1e-4, n
    a = _sample(pipe, side, num_inference_steps=6, solver="dpmpp_2m")
    b = _sample(pipe, side, num_inference_steps=6, ddim_eta=0)
    print("6 steps, 2M vs DDIM(0): %.3e" % relerr(a, b))
    assert relerr(a, b) > 1e-4
    assert torch.isfinite(a).all()


def _gaussian_setup(schedule):
    """fp64 sampler on the project's schedule + the exact denoiser for N(mu, s^2) data on the same gammas"""
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(schedule_type=schedule, threshold_function="NONE")).double()
    model = D.Model(DC.GaussianDenoiser(smp.gammas))
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return smp, model, x_T


@pytest.mark.parametrize("schedule", ["COSINE", "DDPM", "DEEPFLOYD"])
@pytest.mark.parametrize("n", [10, 20, 40, 80])
def test_solves_the_probability_flow_ode_better_than_ddim(schedule, n):
    """Gaussian data, exact denoiser: the state before the last step (the last step is the same first-order denoise
    for both solvers) is at most HALF as far from the exact flow as DDIM(eta = 0)'s at the same step count."""
    smp, model, x_T = _gaussian_setup(schedule)
    steps = smp.set_timesteps(n)
    exact = DC.gaussian_flow(x_T, smp.gammas[steps[0]], smp.gammas[steps[-2]])
    kw = dict(resample_steps=True, return_sequence=True, num_inference_steps=n)
    with torch.no_grad():
        e2m = float((smp.sample(model, x_T, None, None, {}, solver="dpmpp_2m", **kw)[-2] - exact).abs().max())
        eddim = float((smp.sample(model, x_T, None, None, {}, ddim_eta=0, **kw)[-2] - exact).abs().max())
    print("%s n=%d: DDIM %.3e 2M %.3e ratio %.2f" % (schedule, n, eddim, e2m, eddim / e2m))
    assert e2m <= 0.5 * eddim


def test_convergence_is_second_order():
    """gamma 0.02 -> 0.98 in steps uniform in lambda, fp64, through the public single-update method: halving the step
    32 -> 64 -> 128 divides the error by at least 3 each time (first order: 2, second order: 4)."""
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(threshold_function="NONE")).double()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    lam = lambda g: 0.5 * math.log(g / (1 - g))
    errs = []
    for n in (32, 64, 128):
        lams = torch.linspace(lam(0.02), lam(0.98), n + 1, dtype=torch.float64)
        gam = torch.sigmoid(2 * lams)   # gamma = alpha^2 with lambda = log(alpha / sigma)
        col = lambda i: gam[i].expand(2).reshape(-1, 1, 1, 1)
        x_t, x0_prev = x, None
        for i in range(n):
            x0_prev, x_t = smp.get_prediction_xt_last_2m(
                x_t, DC.gaussian_v(x_t, col(i)), col(i), col(i + 1), g_prev=col(i - 1) if i else None, x0_prev=x0_prev,
                second_order=i > 0, clip_fn=smp.clip_sample)
        errs.append(float((x_t - DC.gaussian_flow(x, gam[0], gam[n])).abs().max()))
    print("errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    assert errs[0] / errs[1] >= 3 and errs[1] / errs[2] >= 3


@pytest.mark.parametrize("start", [-1, 600])
def test_sampling_loop_orders_and_history(start):
    """Sampler.sample(solver=...) == a hand-rolled loop over the fp64 restatement: first order on the first step of
    the trajectory (also one that starts late, t > -1) and on the last, second order with the x0 / gamma of the step
    before in between; return_sequence and yield_output see the same states."""
    smp, model, x_T = _gaussian_setup("DEEPFLOYD")
    n = 8
    steps = [int(s) for s in smp.set_timesteps(n) if start < 0 or s <= start]
    gam = smp.gammas
    x, x0_prev, want = x_T, None, []
    for i, (t, s) in enumerate(zip(steps[:-1], steps[1:])):
        second = 0 < i < len(steps) - 2
        x0_prev, x = DC.dpmpp_2m_update(x, DC.gaussian_v(x, gam[t]), gam[t].expand(2), gam[s].expand(2),
                                        gam[steps[i - 1]].expand(2) if second else None, x0_prev, second)
        want.append(x)
    kw = dict(resample_steps=True, num_inference_steps=n, t=start, solver="dpmpp_2m")
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, return_sequence=True, **kw)
        ys = list(smp.sample(model, x_T, None, None, {}, yield_output=True, **kw))
    assert len(seq) == len(steps) and len(ys) == len(steps)   # x_T + one per step / one per step + the final image
    for a, b in zip(seq[1:-1], want[:-1]):
        assert relerr(a, b) < 1e-9
    assert relerr(seq[-1], want[-1].clamp(-1, 1)) < 1e-9 and relerr(ys[-1], want[-1].clamp(-1, 1)) < 1e-9
    assert relerr(ys[len(steps) // 2], want[len(steps) // 2]) < 1e-9


def test_without_resampling_every_schedule_step_is_taken():
    """resample_steps=False walks all n_steps times; the solver follows (a 12-step schedule keeps this quick)"""
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(num_diffusion_steps=12, threshold_function="NONE")).double()
    model = D.Model(DC.GaussianDenoiser(smp.gammas))
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with torch.no_grad():
        a = smp.sample(model, x_T, None, None, {}, solver="dpmpp_2m", return_sequence=True)
        b = smp.sample(model, x_T, None, None, {}, solver="dpmpp_2m", return_sequence=True, resample_steps=True,
                       num_inference_steps=12)
    assert len(a) == 13 and all(torch.equal(u, v) for u, v in zip(a, b))


def test_ops_refuse_cpu_tensors():
    """GPU tensors always take the kernel and nothing routes from it to torch: the operator itself has no CPU path"""
    from mdm_hip import _lib, ops

    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_step_2m(x, x, torch.tensor([0.5]), torch.tensor([0.6]), "V_PREDICTION")


def test_guards():
    pipe, side = _pipes(False)
    with pytest.raises(ValueError, match="unknown solver"):
        _sample(pipe, side, num_inference_steps=3, solver="heun")
    with pytest.raises(ValueError, match="ddim_eta"):
        _sample(pipe, side, num_inference_steps=3, solver="dpmpp_2m", ddim_eta=0.5)
    with pytest.raises(ValueError):   # raised at the call, not at the generator's first next()
        pipe.sampler.sample(pipe.get_model(), torch.zeros(1, 3, 16, 16), None, None, {}, yield_output=True, solver="heun")
    with pytest.raises(ValueError):
        pipe.sampler.get_xt_minus_1(pipe.get_model(), 5, torch.zeros(1, 3, 16, 16), None, None, solver="dpmpp_2m", ddim_eta=0.0)
    # solver=None is today's behaviour: the same call with and without the keyword
    a = _sample(pipe, side, num_inference_steps=4)
    b = _sample(pipe, side, num_inference_steps=4, solver=None)
    assert torch.equal(a, b)
