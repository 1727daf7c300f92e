"""CPU: the SA-Solver sampler (``solver=SASolver(...)`` / ``"sa"``) -- the torch-op path of mdm_hip.samplers, which is also
what the GPU kernel is held to (tests/test_sa_solver_gpu.py).  The reference has no such solver, so the yardsticks are
tests/sa_cases.py (the update restated in fp64 with coefficients from numerical quadrature), the closed-form Gaussian flow
of tests/dpm_cases.py, and the identities "first order, tau = 0 == DDIM(eta = 0)" and "first order, tau = 1 == DDIM(eta = 1)"
that tie the new path to code pinned to the reference's goldens."""
import math

import pytest
import torch

import dpm_cases as DC
import sa_cases as SC
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


# the three schedule positions of test_dpm_solver_host.py (time, target time) and the last step
POSITIONS = [(999, 959), (500, 470), (2, 1), (1, 0)]

H_GRID = [1e-4, 1e-3, 1e-2, 0.1, 0.5, 0.999, 1.0, 2.0, 8.0]
RATIOS = [1 / 3, 1.0, 3.0]
TAUS = [0.0, 0.5, 1.0]


# ---- 1. coefficients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_coefficients_match_quadrature(tau):
    """the sampler's predictor and corrector coefficients, orders 1-3, against composite-Simpson quadrature of the defining
    integral over h in [1e-4, 8] and uneven node spacing (ratios 1/3, 1, 3): <= 1e-10 relative in fp64, and
    sum_j c_j = -expm1(-kappa h)"""
    from mdm_hip import samplers as S

    T = lambda v: torch.tensor([v], dtype=torch.float64)
    worst = 0.0
    for h in H_GRID:
        for r1 in RATIOS:
            for r2 in RATIOS:
                h1, h2 = r1 * h, r2 * r1 * h
                for order in (1, 2, 3):
                    want = SC.quad_coeffs([0.0, -h1, -h1 - h2][:order], h, tau)
                    got = [float(c) for c in S.sa_predictor_coeffs(T(h), tau, order, T(h1), T(h2))]
                    # the corrector redoes a step of h from node a-1 (offset 0) to node a (offset h); a-2 lies h1 before
                    wantc = SC.quad_coeffs([h, 0.0, -h1][:order], h, tau)
                    gotc = [float(c) for c in S.sa_corrector_coeffs(T(h), tau, order, T(h1))]
                    for w, g in zip(want + wantc, got[:order] + gotc[:order]):
                        worst = max(worst, abs(g - w) / abs(w))
                    assert all(c == 0 for c in got[order:] + gotc[order:])
                    total = -math.expm1(-(1 + tau * tau) * h)
                    assert abs(sum(got) - total) <= 1e-12 * total and abs(sum(gotc) - total) <= 1e-12 * total
    print("tau=%g: worst relative error %.2e" % (tau, worst))
    assert worst <= 1e-10


# ---- 2. first-order identities --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,gate", [(torch.float64, 1e-12), (torch.float32, 1e-4)])
@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
def test_first_order_is_ddim(dtype, gate, pred):
    """order (1, 0): tau = 0 is DDIM(eta = 0), tau = 1 with a given noise is DDIM(eta = 1) with the same noise
    (sigma_b^2 (1 - e^{-2h}) = beta-tilde) -- at both ends and in the middle of the schedule and on the last step"""
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(prediction_type=pred))
    smp = smp.double() if dtype == torch.float64 else smp
    gen = torch.Generator().manual_seed(3)
    B, H = 3, 20
    x_t = (torch.randn(B, 3, H, H, generator=gen) * 1.3).to(dtype)
    p = torch.randn(B, 3, H, H, generator=gen).to(dtype)
    z = torch.randn(B, 3, H, H, generator=gen).to(dtype)
    for t, s in POSITIONS:
        g, gl = smp.read_gamma(torch.full((B,), t)), smp.read_gamma(torch.full((B,), s))
        last = s == 0
        for tau, eta in ((0.0, 0.0), (1.0, 1.0)):
            x0, xl, _ = smp.get_prediction_xt_last_sa(x_t, p, g, gl, gate=(1, 0, 0.0 if last else tau, 0.0), input_noise=z,
                                                      clip_fn=smp.clip_sample)
            r0, rl, _ = smp.get_prediction_xt_last(x_t, p, g, gl, clip_fn=smp.clip_sample, need_noise=not last,
                                                   ddim_eta=eta, input_noise=z)
            e0, el = relerr(x0, r0), relerr(xl, rl)
            print("%s t=%d -> %d tau=%g: x0 %.2e x_s %.2e" % (dtype, t, s, tau, e0, el))
            assert e0 <= gate and el <= gate
            if last:
                assert torch.equal(xl, x0)


# ---- 3. order on grids uniform in lambda ----------------------------------------------------------------------
def _lambda_grid_errors(step, ns=(16, 32, 64)):
    """gamma 0.02 -> 0.98 in n steps uniform in lambda, fp64, the exact Gaussian denoiser; ``step(smp, i, x_t, v, col,
    state) -> (x_t, state)`` is one update through a public single-update method -> max errors against the exact flow"""
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(threshold_function="NONE")).double()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    lam = lambda g: 0.5 * math.log(g / (1 - g))
    errs = []
    for n in ns:
        lams = torch.linspace(lam(0.02), lam(0.98), n + 1, dtype=torch.float64)
        gam = torch.sigmoid(2 * lams)
        col = lambda i: gam[i].expand(2).reshape(-1, 1, 1, 1)
        x_t, state = x, None
        for i in range(n):
            x_t, state = step(smp, i, x_t, DC.gaussian_v(x_t, col(i)), col, state)
        errs.append(float((x_t - DC.gaussian_flow(x, gam[0], gam[n])).abs().max()))
    return errs


def _sa_stepper(P, C):
    def step(smp, i, x_t, v, col, state):
        h0, h1, ps = state or (None, None, None)
        gate = (min(P, i + 1), 0 if i == 0 else min(C, i + 1), 0.0, 0.0)
        _, x_t, state = smp.get_prediction_xt_last_sa(x_t, v, col(i), col(i + 1), gate=gate, h0=h0, h1=h1, psum=ps,
                                                      g_h0=col(i - 1) if i else None, g_h1=col(i - 2) if i > 1 else None,
                                                      clip_fn=smp.clip_sample)
        return x_t, state
    return step


def _2m_step(smp, i, x_t, v, col, state):
    x0, x_t = smp.get_prediction_xt_last_2m(x_t, v, col(i), col(i + 1), g_prev=col(i - 1) if i else None, x0_prev=state,
                                            second_order=i > 0, clip_fn=smp.clip_sample)
    return x_t, x0


def test_convergence_is_third_order():
    """SASolver(3, 3): halving the step 16 -> 32 -> 64 divides the max error by >= 6 each time (third order: 8), and the
    error is <= 1/4 of dpmpp_2m's at each n.  Predictor-only order 3 is printed, not held to the ratio: its first step is
    first order and nothing repairs it."""
    e33 = _lambda_grid_errors(_sa_stepper(3, 3))
    e2m = _lambda_grid_errors(_2m_step)
    e30 = _lambda_grid_errors(_sa_stepper(3, 0))
    print("SA(3,3) errors", e33, "ratios %.2f %.2f" % (e33[0] / e33[1], e33[1] / e33[2]))
    print("2M      errors", e2m, "2M / SA(3,3): %.1f %.1f %.1f" % tuple(a / b for a, b in zip(e2m, e33)))
    print("SA(3,0) errors", e30, "ratios %.2f %.2f" % (e30[0] / e30[1], e30[1] / e30[2]))
    assert e33[0] / e33[1] >= 6 and e33[1] / e33[2] >= 6
    assert all(a <= 0.25 * b for a, b in zip(e33, e2m))


# ---- 4. the project's schedules -------------------------------------------------------------------------------
def _gaussian_setup(schedule):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    smp = S.Sampler(sc(schedule_type=schedule, threshold_function="NONE")).double()
    model = D.Model(DC.GaussianDenoiser(smp.gammas))
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return smp, model, x_T


@pytest.mark.parametrize("schedule", ["COSINE", "DDPM", "DEEPFLOYD"])
@pytest.mark.parametrize("n", [10, 20, 40, 80])
def test_solves_the_probability_flow_ode_better_than_ddim(schedule, n):
    """Gaussian data, exact denoiser, steps uniform in time: the state before the last step is at most HALF as far from the
    exact flow as DDIM(eta = 0)'s -- the condition dpmpp_2m is held to.  No claim against 2M on these grids (printed)."""
    from mdm_hip import samplers as S

    smp, model, x_T = _gaussian_setup(schedule)
    steps = smp.set_timesteps(n)
    exact = DC.gaussian_flow(x_T, smp.gammas[steps[0]], smp.gammas[steps[-2]])
    kw = dict(resample_steps=True, return_sequence=True, num_inference_steps=n)
    with torch.no_grad():
        run = lambda **more: float((smp.sample(model, x_T, None, None, {}, **kw, **more)[-2] - exact).abs().max())
        esa, e2m, eddim = run(solver=S.SASolver(3, 3)), run(solver="dpmpp_2m"), run(ddim_eta=0)
    print("%s n=%d: DDIM %.3e 2M %.3e SA(3,3) %.3e  SA/DDIM %.4f  SA/2M %.3f" % (schedule, n, eddim, e2m, esa, esa / eddim,
                                                                               esa / e2m))
    assert esa <= 0.5 * eddim


# ---- 5. stochastic --------------------------------------------------------------------------------------------
def _noise_source(noises):
    it = iter(noises)
    return lambda x: next(it)


@pytest.mark.parametrize("P,C", [(3, 3), (2, 1)])
def test_stochastic_sample_matches_the_fp64_loop(P, C):
    """tau = 1 with given noises: a whole sample() == the explicit fp64 loop of tests/sa_cases.py (corrector written as the
    step redone from x_{a-1}, coefficients by quadrature) within 1e-9"""
    from mdm_hip import samplers as S

    smp, model, x_T = _gaussian_setup("DEEPFLOYD")
    n = 8
    steps = [int(s) for s in smp.set_timesteps(n)]
    gam = [float(smp.gammas[s]) for s in steps]
    gen = torch.Generator().manual_seed(11)
    noises = [torch.randn(x_T.shape, generator=gen, dtype=torch.float64) for _ in range(n)]
    denoise = lambda x, g: DC.gaussian_x0(x, torch.tensor(g, dtype=torch.float64))
    want = SC.sa_trajectory(denoise, x_T, gam, P, C, [1.0] * n, noises)
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, solver=S.SASolver(P, C, tau=1.0), resample_steps=True,
                         num_inference_steps=n, return_sequence=True, solver_noise_fn=_noise_source(noises))
    errs = [relerr(a, b) for a, b in zip(seq[1:-1], want[:-1])] + [relerr(seq[-1], want[-1].clamp(-1, 1))]
    print("per-step errors", ["%.1e" % e for e in errs])
    assert max(errs) < 1e-9


def _final_variance(smp, model, n, solver):
    """The denoiser is affine, so the final state is a x_T + sum_i b_i z_i + const: propagate the basis inputs (one batch
    row each) -> a^2 var_T + sum_i b_i^2 with var_T = 1"""
    rows = n + 2          # row 0: all zero (the constant); row 1: x_T = 1; row 2 + i: z_i = 1
    x_T = torch.zeros(rows, 1, 2, 2, dtype=torch.float64)
    x_T[1] = 1
    noises = []
    for i in range(n):
        z = torch.zeros_like(x_T)
        z[2 + i] = 1
        noises.append(z)
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, solver=solver, resample_steps=True, num_inference_steps=n,
                         return_sequence=True, solver_noise_fn=_noise_source(noises))
    out = seq[-2][:, 0, 0, 0]     # the state before the last step; seq[-1] is clipped to [-1, 1]
    coef = out[1:] - out[0]
    return float((coef ** 2).sum())


def test_stochastic_variance_converges():
    """SASolver(3, 3, tau=1) on DEEPFLOYD, Gaussian data: the variance of the final state, exact by propagating basis
    inputs (the last step, a plain denoise, is the linear map x -> MU + k (x - sqrt(g) MU) of the state before it), deviates
    from the data's variance S^2 by a relative amount that shrinks monotonically over n = 10, 20, 40, 80.
    Measured: 0.3030, 0.1462, 0.0446, 0.0113."""
    from mdm_hip import samplers as S

    smp, model, _ = _gaussian_setup("DEEPFLOYD")
    devs = []
    for n in (10, 20, 40, 80):
        steps = smp.set_timesteps(n)
        g = float(smp.gammas[steps[-2]])
        k = math.sqrt(g) * DC.S * DC.S / (g * DC.S * DC.S + 1 - g)   # d E[x0 | x] / d x at the last step's gamma
        var = k * k * _final_variance(smp, model, n, S.SASolver(3, 3, tau=1.0))
        devs.append(abs(var - DC.S * DC.S) / (DC.S * DC.S))
    print("relative deviation of the variance:", ["%.4f" % d for d in devs])
    assert all(a > b for a, b in zip(devs, devs[1:]))


# ---- 6. loop bookkeeping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [-1, 600])
def test_sampling_loop_orders_and_history(start, monkeypatch):
    """orders 1, 2, 3, .., 1 and corrector off, 2, 3, .., skipped, also from a late start; sample() == the explicit fp64
    loop; return_sequence and yield_output see the same states"""
    from mdm_hip import samplers as S

    smp, model, x_T = _gaussian_setup("DEEPFLOYD")
    n = 8
    steps = [int(s) for s in smp.set_timesteps(n) if start < 0 or s <= start]
    gam = [float(smp.gammas[s]) for s in steps]
    denoise = lambda x, g: DC.gaussian_x0(x, torch.tensor(g, dtype=torch.float64))
    want = SC.sa_trajectory(denoise, x_T, gam, 3, 3, [0.0] * n)
    seen = []
    inner = S.Sampler.get_prediction_xt_last_sa

    def spy(self, *a, **kw):
        seen.append(tuple(kw["gate"][:2]))
        return inner(self, *a, **kw)

    monkeypatch.setattr(S.Sampler, "get_prediction_xt_last_sa", spy)
    kw = dict(resample_steps=True, num_inference_steps=n, t=start, solver="sa")
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, return_sequence=True, **kw)
        m = len(steps) - 1
        assert seen == [(min(3, i + 1), 0 if i == 0 else min(3, i + 1)) for i in range(m - 1)] + [(1, 0)]
        ys = list(smp.sample(model, x_T, None, None, {}, yield_output=True, **kw))
    assert len(seq) == len(steps) and len(ys) == len(steps)
    for a, b in zip(seq[1:-1], want[:-1]):
        assert relerr(a, b) < 1e-9
    assert relerr(seq[-1], want[-1].clamp(-1, 1)) < 1e-9 and relerr(ys[-1], want[-1].clamp(-1, 1)) < 1e-9
    assert relerr(ys[len(steps) // 2], want[len(steps) // 2]) < 1e-9


def test_tau_interval_gates_per_step():
    """tau_interval = (lo, hi) in fractions of n_steps: tau inside, 0 outside, per step -- and the corrector redoes a step
    with the tau THAT step was taken at"""
    from mdm_hip import samplers as S

    smp, model, x_T = _gaussian_setup("DEEPFLOYD")
    n = 8
    steps = [int(s) for s in smp.set_timesteps(n)]
    gam = [float(smp.gammas[s]) for s in steps]
    sol = S.SASolver(3, 3, tau=0.8, tau_interval=(0.3, 0.7))
    taus = [0.8 if 0.3 <= t / 1000 <= 0.7 else 0.0 for t in steps[:-1]]
    assert 0 < sum(t > 0 for t in taus) < n and [sol.tau_at(t, 1000) for t in steps[:-1]] == taus
    gates = sol.gates(steps[:-1], steps[1:], 1000)
    assert [g[2] for g in gates] == taus[:-1] + [0.0] and [g[3] for g in gates[1:-1]] == taus[:-2]
    gen = torch.Generator().manual_seed(12)
    noises = [torch.randn(x_T.shape, generator=gen, dtype=torch.float64) for _ in range(n)]
    denoise = lambda x, g: DC.gaussian_x0(x, torch.tensor(g, dtype=torch.float64))
    want = SC.sa_trajectory(denoise, x_T, gam, 3, 3, taus, noises)
    used = [z for z, t in zip(noises, taus[:-1] + [0.0]) if t > 0]   # only the steps inside the interval draw
    with torch.no_grad():
        seq = smp.sample(model, x_T, None, None, {}, solver=sol, resample_steps=True, num_inference_steps=n,
                         return_sequence=True, solver_noise_fn=_noise_source(used))
    assert max(relerr(a, b) for a, b in zip(seq[1:-1], want[:-1])) < 1e-9


def test_a_change_after_the_step_survives_the_correction():
    """the corrector is a difference, so what is done to x_a after the step (the known-region blend) stays: get_xt_minus_1
    with a solver_state, the state shifted between the calls, == the fp64 loop with the same shift"""
    from mdm_hip import samplers as S

    smp, model, x_T = _gaussian_setup("DEEPFLOYD")
    steps = [int(s) for s in smp.set_timesteps(5)]
    gam = [float(smp.gammas[s]) for s in steps]
    denoise = lambda x, g: DC.gaussian_x0(x, torch.tensor(g, dtype=torch.float64))
    shift = lambda i, x: x + 0.05 * (i + 1)
    want = SC.sa_trajectory(denoise, x_T, gam, 3, 3, [0.0] * 5, after=shift)
    x, state = x_T, {}
    with torch.no_grad():
        for i, (t, s) in enumerate(zip(steps[:-1], steps[1:])):
            x = smp.get_xt_minus_1(model, t, x, None, None, {}, time_step_last=s, solver=S.SASolver(3, 3),
                                   solver_state=state)
            x = shift(i, x)
            assert state["count"] == i + 1 and relerr(x, want[i]) < 1e-9


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
def test_diffusion_sample_passes_the_solver_through(nested):
    """Diffusion.sample / NestedDiffusion.sample(solver=...): 1 and 2 steps have no higher-order step and no corrector that
    changes anything beyond first order... 1 step equals DDIM(eta = 0); "sa" means SASolver(); 6 steps differ from DDIM;
    tau > 0 draws from torch's generator (another seed, another image)"""
    from mdm_hip import samplers as S

    pipe, side = _pipes(nested)
    a = _sample(pipe, side, num_inference_steps=1, solver="sa")
    b = _sample(pipe, side, num_inference_steps=1, ddim_eta=0)
    assert relerr(a, b) < 1e-4
    a = _sample(pipe, side, num_inference_steps=6, solver="sa")
    b = _sample(pipe, side, num_inference_steps=6, solver=S.SASolver())
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert relerr(a, _sample(pipe, side, num_inference_steps=6, ddim_eta=0)) > 1e-4
    c = _sample(pipe, side, num_inference_steps=6, solver=S.SASolver(2, 2, tau=1.0))
    d = _sample(pipe, side, num_inference_steps=6, solver=S.SASolver(2, 2, tau=1.0))
    assert torch.equal(c, d) and relerr(c, a) > 1e-4 and torch.isfinite(c).all()


def test_other_solvers_do_not_change():
    """solver=None and "dpmpp_2m" are bit-identical whether or not the SA path can be reached: the same calls with
    Sampler.get_prediction_xt_last_sa and ops.sampler_step_sa removed"""
    from mdm_hip import ops
    from mdm_hip import samplers as S

    pipe, side = _pipes(False)
    calls = [dict(num_inference_steps=5), dict(num_inference_steps=5, ddim_eta=0.5),
             dict(num_inference_steps=5, solver="dpmpp_2m"), dict(num_inference_steps=5, solver=None)]
    before = [_sample(pipe, side, **kw) for kw in calls]
    mp = pytest.MonkeyPatch()
    try:
        mp.delattr(S.Sampler, "get_prediction_xt_last_sa")
        mp.delattr(ops, "sampler_step_sa")
        after = [_sample(pipe, side, **kw) for kw in calls]
    finally:
        mp.undo()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(before[0], before[3])


# ---- 7. guards ------------------------------------------------------------------------------------------------
def test_guards():
    from mdm_hip import _lib, ops
    from mdm_hip import samplers as S
    import mdm_hip

    assert mdm_hip.SASolver is S.SASolver and S.SASolver() == S.SASolver(3, 3, 0.0, None)
    pipe, side = _pipes(False)
    with pytest.raises(ValueError, match="unknown solver"):
        _sample(pipe, side, num_inference_steps=3, solver="heun")
    for solver in ("sa", S.SASolver(2, 2)):
        with pytest.raises(ValueError, match="ddim_eta"):
            _sample(pipe, side, num_inference_steps=3, solver=solver, ddim_eta=0.5)
    model, x = pipe.get_model(), torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError):   # raised at the call, not at the generator's first next()
        pipe.sampler.sample(model, x, None, None, {}, yield_output=True, solver="sa", ddim_eta=0.0)
    with pytest.raises(ValueError):
        pipe.sampler.get_xt_minus_1(model, 5, x, None, None, solver="sa", ddim_eta=0.0)
    with pytest.raises(ValueError, match="resample"):
        pipe.sampler.sample(model, x, None, None, {}, solver="sa", known_images=x, resample=2)
    guide = S.LossGuide(lambda x0: (x0 ** 2).mean(dim=(1, 2, 3)))
    with pytest.raises(NotImplementedError, match="guide"):
        pipe.sampler.sample(model, x, None, None, {}, solver="sa", guide=guide)
    with pytest.raises(NotImplementedError, match="guide"):
        pipe.sampler.get_xt_minus_1(model, 5, x, None, None, solver=S.SASolver(), guide=guide)
    for bad in (dict(predictor=4), dict(predictor=0), dict(predictor=-1), dict(corrector=4), dict(corrector=-1),
                dict(predictor=2.5), dict(tau=-0.1), dict(tau=float("nan")), dict(tau_interval=(0.7, 0.3)),
                dict(tau_interval=0.5)):
        with pytest.raises(ValueError):
            S.SASolver(**bad)
    with pytest.raises(ValueError):   # no positive step in log-SNR
        S.SASolver().gate(0, 5, 5, 1000)
    # GPU tensors always take the kernel and nothing routes from it to torch: the operator itself has no CPU path
    with pytest.raises(_lib.MdmHipError):
        ops.sampler_step_sa(x, x, torch.tensor([0.5]), torch.tensor([0.6]), "V_PREDICTION", (1, 0, 0.0, 0.0))
