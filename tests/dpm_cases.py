"""Yardsticks for the DPM-Solver++(2M) sampler that do not come from the package under test.

(a) ``dpmpp_2m_update``: the published update (Lu, Zhou, Bao, Chen, Li, Zhu 2022, "DPM-Solver++: Fast Solver for Guided
    Sampling of Diffusion Probabilistic Models", multistep / data prediction) written out in fp64 straight from its
    definitions -- alpha, sigma, lambda = log(alpha / sigma), h -- with nothing imported from ``mdm_hip``.
(b) ``GaussianDenoiser`` / ``gaussian_flow``: for per-pixel data N(mu, s^2) the posterior mean E[x0 | x_t] and the
    solution of the probability-flow ODE are closed forms, so a solver's error is measurable without a trained network.
"""
import torch
import torch.nn as nn

MU, S = 0.2, 0.5


def _col(v):
    return torch.as_tensor(v, dtype=torch.float64).reshape(-1, 1, 1, 1)


def threshold(x0, kind, scale):
    """the four threshold functions on x0 (image_scale ``scale``): clamp in units of x0 * scale, back to x0's units"""
    if kind == "NONE":
        return x0
    v = x0 * scale
    if kind == "CLIP":
        return v.clamp(-1, 1) / scale
    ratio, vmax = {"DYNAMIC": (0.995, 100.0), "DYNAMIC_IF": (0.95, 1.5)}[kind]
    q = torch.quantile(v.reshape(v.shape[0], -1).abs(), ratio, dim=1).clamp(min=1, max=vmax).reshape(-1, 1, 1, 1)
    return torch.maximum(torch.minimum(v, q), -q) / q / scale


def dpmpp_2m_update(x_t, pred, g, gl, gp=None, x0_prev=None, second_order=False, pred_type="V_PREDICTION",
                    thr="NONE", image_scale=1.0, pred_uncond=None, guidance=1.0):
    """-> (x0, x_s) in fp64.  g / gl / gp: gamma of the current time, of the target, of the step before (per sample)."""
    x_t, p = x_t.double(), pred.double()
    if pred_uncond is not None:
        p = pred_uncond.double() + guidance * (p - pred_uncond.double())
    g, gl = _col(g), _col(gl)
    alpha_t, sigma_t = g.sqrt(), (1 - g).sqrt()
    alpha_s, sigma_s = gl.sqrt(), (1 - gl).sqrt()
    if pred_type == "V_PREDICTION":
        x0 = alpha_t * x_t - sigma_t * p
    else:   # eps prediction
        x0 = (x_t - sigma_t * p) / alpha_t
    x0 = threshold(x0, thr, image_scale)
    D = x0
    if second_order:
        gp = _col(gp)
        lam = lambda a, s: torch.log(a / s)
        h = lam(alpha_s, sigma_s) - lam(alpha_t, sigma_t)
        h_prev = lam(alpha_t, sigma_t) - lam(gp.sqrt(), (1 - gp).sqrt())
        r = h / (2 * h_prev)
        D = (1 + r) * x0 - r * x0_prev.double()
    x_s = (sigma_s / sigma_t) * x_t + (alpha_s - sigma_s * alpha_t / sigma_t) * D
    return x0, x_s


# ---- Gaussian data: everything in closed form ------------------------------------------------------------
def _var(g):
    return g * S * S + 1 - g   # variance of x_t


def gaussian_x0(x_t, g):
    """E[x0 | x_t] for x0 ~ N(MU, S^2), x_t = sqrt(g) x0 + sqrt(1 - g) eps"""
    return MU + g.sqrt() * S * S / _var(g) * (x_t - g.sqrt() * MU)


def gaussian_v(x_t, g):
    """the v-prediction that yields ``gaussian_x0``: x0 = sqrt(g) x_t - sqrt(1 - g) v"""
    return (g.sqrt() * x_t - gaussian_x0(x_t, g)) / (1 - g).sqrt()


def gaussian_flow(x_t, g_t, g_s):
    """exact solution of the probability-flow ODE from gamma g_t to gamma g_s"""
    return g_s.sqrt() * MU + (_var(g_s) / _var(g_t)).sqrt() * (x_t - g_t.sqrt() * MU)


class GaussianDenoiser(nn.Module):
    """vision-model stand-in (same call surface as tests/stub_models.StubUNet) that returns the exact v-prediction.
    The sampler hands the denoiser ``t - 1``; the time whose gamma is meant is ``times + 1``."""

    def __init__(self, gammas):
        super().__init__()
        self.input_channels = 3
        self.conditions = None
        self.register_buffer("gammas", gammas.clone())

    def forward(self, x_t, times, lm_outputs, lm_mask, micros={}):
        g = self.gammas[times + 1].reshape(-1, 1, 1, 1)
        return gaussian_v(x_t, g)
