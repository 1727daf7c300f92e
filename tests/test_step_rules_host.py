"""CPU: the ``StepRule`` interface of mdm_hip.samplers -- what ``solver=`` resolves to, the rows of the three built-in
rules against literal tables, and a rule written HERE against the documented interface alone, which must reproduce the
built-in ancestral rule bit for bit (tests/test_step_rules_gpu.py runs the same rule through the captured graph)."""
import numpy as np
import pytest
import torch

import stub_models as SM
from test_dpm_solver_host import sc


def restated(eta=None):
    """DDPM / DDIM(eta) once more, as a rule of one's own: the base class, ``get_prediction_xt_last`` and nothing private"""
    from mdm_hip import samplers as S

    class Restated(S.StepRule):
        def __init__(self, eta):
            self.eta, self.key = eta, ("restated", eta)

        def rows(self, sampler, times, times_last):   # the noise gate: off on the last step (nested: on the step from t = 1)
            on = np.asarray(times) != 1 if isinstance(sampler, S.NestedSampler) else np.asarray(times_last) != 0
            return on.astype("float32").reshape(-1, 1)

        def step(self, sampler, k, x_t, pred, g_t, g_s, row, g_hist, state, noise_fn=None, **common):
            graph = torch.is_tensor(row)   # a device row: every step draws, the gate decides
            x0, x_s, _ = sampler.get_prediction_xt_last(x_t, pred, g_t, g_s, ddim_eta=self.eta, return_eps=False,
                                                        need_noise=graph or bool(row[0]), noise_gate=row if graph else None,
                                                        **common)
            return x0, x_s

    return Restated(eta)


def _samplers():
    from mdm_hip import samplers as S

    return S.Sampler(sc()), S.NestedSampler(sc(schedule_shifted=True, rescale_signal=1))


def test_resolver_and_keys():
    from mdm_hip import samplers as S

    assert isinstance(S._rule_of(None), S.StepRule) and S._rule_of(None, 0.5).ddim_eta == 0.5
    assert S._rule_of("sa") == S.SASolver() and isinstance(S._rule_of("dpmpp_2m"), S.StepRule)
    mine = S.SASolver(2, 1, tau=0.5)
    assert S._rule_of(mine) is mine and isinstance(mine, S.StepRule)
    own = restated(0.5)
    assert S._rule_of(own) is own
    with pytest.raises(ValueError, match="unknown solver"):
        S._rule_of("heun")
    key = lambda solver, eta=None: S._rule_of(solver, eta).key
    assert key("sa") == key(S.SASolver()) and hash(key("sa")) == hash(key(S.SASolver()))
    assert key(None) == key(None) and key(None, 0.5) == key(None, 0.5) and key("dpmpp_2m") == key("dpmpp_2m")
    different = [key(None), key(None, 0.0), key(None, 0.5), key("dpmpp_2m"), key("sa"), key(S.SASolver(3, 2)),
                 key(S.SASolver(2, 3)), key(S.SASolver(tau=0.5)), key(S.SASolver(tau=0.5, tau_interval=(0.1, 0.9))), own.key]
    assert len(set(different)) == len(different)
    assert (S._rule_of(None).history, S._rule_of("dpmpp_2m").history, S._rule_of("sa").history) == (0, 1, 2)


SIX = np.array([858, 715, 572, 429, 286, 143, 0])   # set_timesteps(6) and (2) of a 1000-step schedule
TWO = np.array([667, 334, 0])
F = lambda rows: np.asarray(rows, dtype="float32")


def test_rows_against_literal_tables():
    from mdm_hip import samplers as S

    plain, nested = _samplers()
    assert (plain.set_timesteps(6) == SIX).all() and (plain.set_timesteps(2) == TWO).all()
    rows = lambda rule, smp, steps: rule.rows(smp, steps[:-1], steps[1:])
    same = lambda got, want: got.dtype == np.float32 and got.shape == F(want).shape and (got == F(want)).all()
    anc = S._rule_of(None)
    assert same(rows(anc, plain, SIX), [[1], [1], [1], [1], [1], [0]]) and same(rows(anc, plain, TWO), [[1], [0]])
    # the nested sampler's gate is t != 1: on a resampled schedule every step adds noise, the last one too ...
    assert same(rows(anc, nested, SIX), [[1]] * 6) and same(rows(anc, nested, TWO), [[1], [1]])
    # ... and on the full schedule the step from t = 1 does not
    assert same(anc.rows(nested, np.array([3, 2, 1]), np.array([2, 1, 0])), [[1], [1], [0]])
    assert same(anc.rows(plain, np.array([3, 2, 1]), np.array([2, 1, 0])), [[1], [1], [0]])
    two_m = S._rule_of("dpmpp_2m")
    for smp in (plain, nested):
        assert same(rows(two_m, smp, SIX), [[0], [1], [1], [1], [1], [0]]) and same(rows(two_m, smp, TWO), [[0], [0]])
        assert same(rows(S._rule_of("sa"), smp, SIX),
                    [[1, 0, 0, 0], [2, 2, 0, 0], [3, 3, 0, 0], [3, 3, 0, 0], [3, 3, 0, 0], [1, 0, 0, 0]])
        assert same(rows(S._rule_of("sa"), smp, TWO), [[1, 0, 0, 0], [1, 0, 0, 0]])
        assert same(rows(S.SASolver(2, 2, tau=1.0), smp, SIX),
                    [[1, 0, 1, 0], [2, 2, 1, 1], [2, 2, 1, 1], [2, 2, 1, 1], [2, 2, 1, 1], [1, 0, 0, 0]])
        assert same(rows(S.SASolver(2, 2, tau=1.0), smp, TWO), [[1, 0, 1, 0], [1, 0, 0, 0]])
        # tau acts on the steps that start at 0.572 and 0.429 of the schedule; the corrector redoes a step at ITS tau
        assert same(rows(S.SASolver(3, 3, tau=0.8, tau_interval=(0.3, 0.7)), smp, SIX),
                    [[1, 0, 0, 0], [2, 2, 0, 0], [3, 3, 0.8, 0], [3, 3, 0.8, 0.8], [3, 3, 0, 0.8], [1, 0, 0, 0]])
        assert same(rows(S.SASolver(3, 0, tau=0.5), smp, SIX),
                    [[1, 0, 0.5, 0], [2, 0, 0.5, 0], [3, 0, 0.5, 0], [3, 0, 0.5, 0], [3, 0, 0.5, 0], [1, 0, 0, 0]])
    assert rows(two_m, plain, SIX[-1:]).shape == (0, 1) and rows(S._rule_of("sa"), plain, SIX[-1:]).shape == (0, 4)


def test_rows_of_a_late_start_are_those_of_a_fresh_trajectory():
    """the rows count from times[0]: over the last four steps of the six they are what four steps of their own give"""
    from mdm_hip import samplers as S

    plain, nested = _samplers()
    tail = SIX[2:]
    for smp in (plain, nested):
        assert (S._rule_of("dpmpp_2m").rows(smp, tail[:-1], tail[1:]) == F([[0], [1], [1], [0]])).all()
        assert (S._rule_of("sa").rows(smp, tail[:-1], tail[1:]) == F([[1, 0, 0, 0], [2, 2, 0, 0], [3, 3, 0, 0], [1, 0, 0, 0]])).all()
        sol = S.SASolver(3, 3, tau=0.8, tau_interval=(0.3, 0.7))   # the first step lies in the interval; nothing before it
        assert (sol.rows(smp, tail[:-1], tail[1:]) == F([[1, 0, 0.8, 0], [2, 2, 0.8, 0.8], [3, 3, 0, 0.8], [1, 0, 0, 0]])).all()
        for solver in (None, "dpmpp_2m", "sa", sol):   # ... and of the full schedule's rows only the head differs
            rule = S._rule_of(solver)
            full, late = rule.rows(smp, SIX[:-1], SIX[1:]), rule.rows(smp, tail[:-1], tail[1:])
            assert late.shape == full[2:].shape and (late[-1] == full[-1]).all()
    assert (S._rule_of(None).rows(plain, tail[:-1], tail[1:]) == F([[1], [1], [1], [0]])).all()


def _pipe(nested):
    from mdm_hip import diffusion as D

    if nested:
        cfg = D.NestedDiffusionConfig(sampler_config=sc(schedule_shifted=True, rescale_signal=1), use_vdm_loss_weights=False,
                                      use_double_loss=True, no_use_residual=True)
        return D.NestedDiffusion(SM.StubNestedUNet(), cfg), 32
    return D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=sc(), use_vdm_loss_weights=False)), 16


@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("eta", [None, 0.5])
@pytest.mark.parametrize("resampled", [True, False])
def test_a_rule_of_ones_own_reproduces_the_ancestral_rule(nested, eta, resampled):
    """Sampler.sample / NestedSampler.sample(solver=<the rule above>) == solver=None with the same ddim_eta, bit for bit,
    from the same torch seed: 6 resampled steps, and the last 12 of the full schedule (where the nested gate is off once)"""
    pipe, side = _pipe(nested)
    g = torch.Generator().manual_seed(7)
    lm, mask = torch.randn(3, 5, 8, generator=g), torch.ones(3, 5)
    x_T = torch.randn(3, 3, side, side, generator=g)
    kw = dict(resample_steps=True, num_inference_steps=6) if resampled else dict(t=12)

    def run(**more):
        torch.manual_seed(13)
        with torch.no_grad():
            return pipe.sampler.sample(pipe.get_model(), x_T.clone(), lm, mask, {}, **kw, **more)

    want, out = run(ddim_eta=eta), run(solver=restated(eta))
    assert out.shape == (3, 3, side, side) and torch.isfinite(out).all() and torch.equal(out, want)
    assert not torch.equal(want, run(ddim_eta=0.0))   # the noise matters: the comparison is not vacuous
    with pytest.raises(ValueError, match="ddim_eta"):   # the base class's refusals hold for it
        run(solver=restated(eta), ddim_eta=0.5)
    with pytest.raises(ValueError, match="resample"):
        run(solver=restated(eta), known_images=x_T, resample=2)
