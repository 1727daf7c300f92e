"""Yardsticks for image inversion that do not come from the package under test: nothing here imports ``mdm_hip``.

(a) ``invert_step_ref``: the preimage of one DDIM(0) step with the prediction held fixed, in fp64 straight from its
    definition -- alpha = sqrt(gamma), sigma = sqrt(1 - gamma), s the cleaner node:
        eps:  x_t = (alpha_t / alpha_s) (x_s - sigma_s p) + sigma_t p
        v:    x_t = (x_s - (sigma_s alpha_t - alpha_s sigma_t) p) / (alpha_s alpha_t + sigma_s sigma_t)
    with the small coefficients as the quotients (gamma_t - gamma_s) / (sigma_s alpha_t + alpha_s sigma_t) and
    (gamma_s - gamma_t) / ((sigma_t alpha_s + alpha_t sigma_s) alpha_s), and ``ddim0_ref``, the step it inverts.
(b) ``posterior_ref`` / ``noise_map_ref``: the mean and the noise factor of the ancestral step (the DDPM posterior, or
    DDIM(eta > 0)) and the noise z = (x_s - mu) / sigma that lands it on a given x_s; z = 0 where sigma == 0.
(c) ``GaussianEpsDenoiser``: the eps-predicting twin of ``dpm_cases.GaussianDenoiser``.
"""
import torch
import torch.nn as nn

from dpm_cases import MU, S, _col, gaussian_x0, threshold   # fp64 closed forms; dpm_cases imports nothing of mdm_hip either


def guided(pred, pred_uncond=None, guidance=1.0):
    p = pred.double()
    return p if pred_uncond is None else pred_uncond.double() + guidance * (p - pred_uncond.double())


def x0_ref(x_t, p, g, pred_type):
    a, s = g.sqrt(), (1 - g).sqrt()
    return a * x_t - s * p if pred_type == "V_PREDICTION" else (x_t - s * p) / a


def invert_step_ref(x_s, pred, g_s, g_t, pred_type="V_PREDICTION", pred_uncond=None, guidance=1.0):
    """-> x_t in fp64.  g_s / g_t: gamma of the cleaner node and of the noisier one (per sample)."""
    x_s, p = x_s.double(), guided(pred, pred_uncond, guidance)
    g_s, g_t = _col(g_s), _col(g_t)
    a_s, s_s, a_t, s_t = g_s.sqrt(), (1 - g_s).sqrt(), g_t.sqrt(), (1 - g_t).sqrt()
    if pred_type == "V_PREDICTION":
        d = (g_t - g_s) / (s_s * a_t + a_s * s_t)          # sigma_s alpha_t - alpha_s sigma_t
        return (x_s - d * p) / (a_s * a_t + s_s * s_t)
    c = (g_s - g_t) / ((s_t * a_s + a_t * s_s) * a_s)      # sigma_t - alpha_t sigma_s / alpha_s
    return (a_t / a_s) * x_s + c * p


def ddim0_ref(x_t, pred, g_t, g_s, pred_type="V_PREDICTION", pred_uncond=None, guidance=1.0):
    """one deterministic DDIM step from gamma g_t to the cleaner g_s, no threshold, fp64"""
    x_t, p = x_t.double(), guided(pred, pred_uncond, guidance)
    g_t, g_s = _col(g_t), _col(g_s)
    x0 = x0_ref(x_t, p, g_t, pred_type)
    eps = (x_t - g_t.sqrt() * x0) / (1 - g_t).sqrt()
    return g_s.sqrt() * x0 + (1 - g_s).sqrt() * eps


def posterior_ref(x_t, pred, g, gl, pred_type="V_PREDICTION", thr="NONE", image_scale=1.0, pred_uncond=None, guidance=1.0,
                  ddim_eta=None):
    """-> (mu, sigma) of the ancestral step from gamma g to gamma gl in fp64: the DDPM posterior q(x_s | x_t, x0) at the
    thresholded x0 (``ddim_eta`` None), or DDIM(eta): sigma = eta sigma_posterior, mu = alpha_s x0 + sqrt(1 - gl - sigma^2) eps"""
    x_t, p = x_t.double(), guided(pred, pred_uncond, guidance)
    g, gl = _col(g), _col(gl)
    x0 = threshold(x0_ref(x_t, p, g, pred_type), thr, image_scale)
    alpha = g / gl
    var = (1 - alpha) * (1 - gl) / (1 - g)
    if ddim_eta is None:
        mu = gl.sqrt() * (1 - alpha) / (1 - g) * x0 + alpha.sqrt() * (1 - gl) / (1 - g) * x_t
    else:
        var = ddim_eta ** 2 * var
        eps = (x_t - g.sqrt() * x0) / (1 - g).sqrt()
        mu = gl.sqrt() * x0 + (1 - gl - var).sqrt() * eps
    return mu, var.sqrt()


def noise_map_ref(x_t, x_s, pred, g, gl, **kw):
    mu, sigma = posterior_ref(x_t, pred, g, gl, **kw)
    on = sigma > 0
    return torch.where(on, (x_s.double() - mu) / torch.where(on, sigma, torch.ones_like(sigma)), torch.zeros_like(mu))


def gaussian_eps(x_t, g):
    """the eps-prediction that yields ``dpm_cases.gaussian_x0``: x0 = (x_t - sqrt(1 - g) eps) / sqrt(g)"""
    return (x_t - g.sqrt() * gaussian_x0(x_t, g)) / (1 - g).sqrt()


class GaussianEpsDenoiser(nn.Module):
    """``dpm_cases.GaussianDenoiser`` for an eps-predicting sampler: the exact eps-prediction of per-pixel N(MU, S^2) data.
    The sampler hands the denoiser ``t - 1``; the time whose gamma is meant is ``times + 1``."""

    def __init__(self, gammas):
        super().__init__()
        self.input_channels = 3
        self.conditions = None
        self.register_buffer("gammas", gammas.clone())

    def forward(self, x_t, times, lm_outputs, lm_mask, micros={}):
        return gaussian_eps(x_t, self.gammas[times + 1].reshape(-1, 1, 1, 1))
