"""Yardsticks for the SA-Solver sampler (``solver=SASolver(...)``) that do not come from the package under test.

The update of Xue et al. (NeurIPS 2023, "SA-Solver: Stochastic Adams Solver for Fast Sampling of Diffusion Models") on the
data prediction, restated in fp64 from its definition with nothing imported from ``mdm_hip``:

    alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda = log(alpha / sigma); a step from node a to node b,
    h = lambda_b - lambda_a, kappa = 1 + tau^2, m_j the guided, thresholded x0 of node j, l_j the Lagrange basis over the
    nodes' offsets s_j = lambda_j - lambda_a

    x_b = (sigma_b / sigma_a) e^{-tau^2 h} x_a + alpha_b sum_j c_j m_j + sigma_b sqrt(1 - e^{-2 tau^2 h}) z
    c_j = kappa int_0^h e^{-kappa (h - s)} l_j(s) ds

The coefficients come from NUMERICAL QUADRATURE of that integral (composite Simpson, 20 000 panels) -- not from the moment
recurrence or the series the package uses.  The corrector redoes the step a-1 -> a with nodes a, a-1, .. once m_a is known; in
``sa_trajectory``, an explicit loop over steps, it is written as the defining update from x_{a-1} again (same x_{a-1} term, same
noise), NOT as the difference the kernel applies, so the two forms check each other.  ``sa_single`` is one launch on GIVEN state
(arbitrary h0 / h1 / psum), which only the difference form can express: the kernel's contract.

The Gaussian denoiser and flow are those of tests/dpm_cases.py.
"""
import math

import numpy as np
import torch

import dpm_cases as DC

PANELS = 20000


def lam(g):
    return 0.5 * math.log(g / (1.0 - g))


def quad_coeffs(offsets, h, tau, lo=0.0, panels=PANELS):
    """c_j = kappa int_lo^{lo + h} e^{-kappa (lo + h - s)} l_j(s) ds over the nodes at ``offsets`` (composite Simpson)"""
    kappa = 1.0 + tau * tau
    s = np.linspace(lo, lo + h, 2 * panels + 1)
    w = np.ones_like(s)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    w *= h / (6.0 * panels)
    e = kappa * np.exp(-kappa * (lo + h - s))
    out = []
    for j, sj in enumerate(offsets):
        l = np.ones_like(s)
        for k, sk in enumerate(offsets):
            if k != j:
                l *= (s - sk) / (sj - sk)
        out.append(float(np.sum(w * e * l)))
    return out


def x0_of(x_t, pred, g, pred_type="V_PREDICTION", thr="NONE", image_scale=1.0, pred_uncond=None, guidance=1.0):
    """m: guidance combine, x0, threshold -- per-sample gamma ``g`` [B]"""
    x_t, p = x_t.double(), pred.double()
    if pred_uncond is not None:
        p = pred_uncond.double() + guidance * (p - pred_uncond.double())
    g = DC._col(g)
    if pred_type == "V_PREDICTION":
        x0 = g.sqrt() * x_t - (1 - g).sqrt() * p
    else:
        x0 = (x_t - (1 - g).sqrt() * p) / g.sqrt()
    return DC.threshold(x0, thr, image_scale)


def sa_step(x_a, g_a, g_b, ms, gs, order, tau, z=None):
    """The defining update for ONE sample from gamma ``g_a`` to ``g_b`` with the data predictions ``ms`` formed at the gammas
    ``gs`` (any nodes, the first ``order`` of the lists are used) -> (x_b, alpha_b sum_j c_j m_j).  g_b == 1: x_b = ms[0]."""
    if g_b >= 1.0:
        return ms[0].clone(), ms[0].clone()
    la, lb = lam(g_a), lam(g_b)
    h = lb - la
    c = quad_coeffs([lam(gj) - la for gj in gs[:order]], h, tau)
    s = sum(cj * mj for cj, mj in zip(c, ms[:order])) * math.sqrt(g_b)
    x_b = math.sqrt((1 - g_b) / (1 - g_a)) * math.exp(-tau * tau * h) * x_a + s
    if tau > 0:
        x_b = x_b + math.sqrt(1 - g_b) * math.sqrt(1 - math.exp(-2 * tau * tau * h)) * z
    return x_b, s


def sa_single(x_t, m, g, g_last, gate, h0=None, h1=None, g_h0=None, g_h1=None, psum=None, z=None):
    """One launch on a batch with per-sample gammas ([B] each) and GIVEN state, as the kernel's contract states it:
    corrector as the difference x_t - psum + alpha_a sum_j c^c_j m_j, then the predictor.  gate = (p, c, tau, tau of the
    corrected step).  -> (x_last, new psum); samples with g_last == 1 get x_last = m."""
    p, c, tau, tau_c = gate
    xl, ps = [], []
    for b in range(x_t.shape[0]):
        ga, gb = float(g[b]), float(g_last[b])
        mb = m[b].double()
        if gb >= 1.0:
            xl.append(mb.clone())
            ps.append(torch.zeros_like(mb))
            continue
        ms = [mb] + [None if v is None else v[b].double() for v in (h0, h1)]
        gs = [ga] + [None if v is None else float(v[b]) for v in (g_h0, g_h1)]
        x_a = x_t[b].double()
        if c >= 1:
            lp = lam(gs[1])
            cc = quad_coeffs([lam(gj) - lp for gj in gs[:c]], lam(ga) - lp, tau_c)
            x_a = x_a - psum[b].double() + math.sqrt(ga) * sum(cj * mj for cj, mj in zip(cc, ms[:c]))
        x_b, s = sa_step(x_a, ga, gb, ms, gs, p, tau, None if z is None else z[b].double())
        xl.append(x_b)
        ps.append(s)
    return torch.stack(xl), torch.stack(ps)


def sa_trajectory(denoise, x_T, gammas, P, C, taus, noises=None, after=None):
    """An explicit loop over the steps of a trajectory through the nodes ``gammas`` (floats, the last may be 1), the same
    for every sample of ``x_T``.  ``denoise(x, g) -> m`` (fp64).  Orders: predictor min(P, i + 1), corrector off at i = 0 and
    min(C, i + 1) afterwards; the last step to gamma == 1 is first order, tau = 0, no corrector.  ``taus[i]``: tau of step
    i; ``noises[i]``: its z.  ``after(i, x)``: something done to the state after step i (it survives the correction).
    -> the list of states after every step."""
    x = x_T.double()
    n = len(gammas) - 1
    hist = []            # (m, g, predictor order used FROM that node), most recent first
    x_prev = z_prev = None
    out = []
    for i in range(n):
        g, gl = float(gammas[i]), float(gammas[i + 1])
        m = denoise(x, g)
        last = gl >= 1.0
        p = 1 if last else min(P, i + 1)
        c = 0 if (last or i == 0) else min(C, i + 1)
        tau = 0.0 if last else float(taus[i])
        z = None if noises is None else noises[i]
        x_a = x
        if c >= 1:
            ms, gs = [m] + [v[0] for v in hist], [g] + [v[1] for v in hist]
            redo, _ = sa_step(x_prev, hist[0][1], g, ms, gs, c, float(taus[i - 1]), z_prev)
            was, _ = sa_step(x_prev, hist[0][1], g, ms[1:], gs[1:], hist[0][2], float(taus[i - 1]), z_prev)
            x_a = x + (redo - was)
        ms, gs = [m] + [v[0] for v in hist], [g] + [v[1] for v in hist]
        x_new, _ = sa_step(x_a, g, gl, ms, gs, p, tau, z)
        x_prev, z_prev = x_a, z
        hist = [(m, g, p)] + hist[:2]
        x = x_new if after is None else after(i, x_new)
        out.append(x)
    return out
