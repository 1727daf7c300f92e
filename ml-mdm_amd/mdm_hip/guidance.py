"""Projected and rescaled classifier-free guidance -- three published, training-free corrections of the one line
``p_u + w (p_c - p_u)``, for a pixel-space model that is sampled at high guidance and oversaturates there:

  APG       adaptive projected guidance (Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance
            Scales in Diffusion Models", ICLR 2025): in x0 space the guidance update is split into the part parallel to the
            conditional prediction -- the one that saturates, scaled by ``eta`` -- and the part orthogonal to it; the
            update's norm is capped (``norm_threshold``) and a (negative) ``momentum`` runs across the steps
  rescale   (Lin, Liu, Li, Yang, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", WACV 2024, section 3.4):
            the guided prediction is pulled back to the per-sample standard deviation of the conditional one, blended by
            ``rescale`` (the paper's phi)
  interval  (Kynkaanniemi et al., "Applying Guidance in a Limited Interval Improves Sample and Distribution Quality in
            Diffusion Models", NeurIPS 2024): guidance acts in a band of the schedule only; outside it the step takes the
            conditional prediction

Per scale and per sample, with x0 = a x_t + be p (``Sampler._x0_coeffs``), w the guidance scale, sc the image scale:

    D   = a x_t + be p_c                       conditional x0, model units
    E   = be (p_c - p_u) + momentum run_prev   (run_prev = 0 on the first guided step of a trajectory)
    run = E                                    stored before the cap, as in the paper's code
    rms = sc sqrt(sum(E^2) / chw)              image units
    s   = min(1, norm_threshold / rms)  if norm_threshold > 0 else 1        (rms == 0: 1)
    c   = sum(E D) / sum(D^2)                                               (sum(D^2) == 0: 0)
    p_g = p_c + (w - 1) s (E - (1 - eta) c D) / be
    p_g = p_g (rescale std(p_c) / std(p_g) + 1 - rescale)   if rescale > 0  (population std over chw; std(p_g) == 0: 1)

``norm_threshold`` caps the RMS of the update in IMAGE units, not the paper's L2 norm: one value then serves every scale of
a nested model.  The paper's radius is ``r = norm_threshold * sqrt(C * H * W)``.  With the defaults this is plain
classifier-free guidance up to rounding.

GPU tensors: ``ops.cfg_combine`` (two launches per scale, csrc/guidance.hip); CPU tensors: ``cfg_combine`` below.  The
samplers take ``cfg=CFG(...)`` and run the combine in front of the unchanged step, which then sees no unconditional
prediction and guidance 1 -- the place of perturbed-attention guidance's combine.
"""
import math

import torch


class CFG:
    """``CFG(eta=1.0, norm_threshold=0.0, momentum=0.0, rescale=0.0, interval=None)``.

    ``eta``: the factor on the part of the guidance update parallel to the conditional x0 (1 keeps it, 0 removes it).
    ``norm_threshold``: cap on the update's RMS in image units ([-1, 1] images); 0 = none.  ``momentum``: in (-1, 1), the
    paper uses negative values (-0.5); 0 = none.  ``rescale``: in [0, 1], the blend of the std rescale; 0 = none.
    ``interval = (lo, hi)`` in fractions of ``num_diffusion_steps``: guidance is on where lo <= t / T <= hi for the time t
    the step starts from; None = everywhere."""

    def __init__(self, eta=1.0, norm_threshold=0.0, momentum=0.0, rescale=0.0, interval=None):
        self.eta, self.norm_threshold = float(eta), float(norm_threshold)
        self.momentum, self.rescale = float(momentum), float(rescale)
        if interval is not None:
            try:
                lo, hi = interval
                interval = (float(lo), float(hi))
            except (TypeError, ValueError):
                raise ValueError("CFG: interval = %r (wanted (lo, hi) in fractions of the schedule, or None)" % (interval,))
        self.interval = interval
        self.validate()

    def validate(self):
        if not math.isfinite(self.eta):
            raise ValueError("CFG: eta = %r (wanted a finite number)" % (self.eta,))
        if not (math.isfinite(self.norm_threshold) and self.norm_threshold >= 0):
            raise ValueError("CFG: norm_threshold = %r (wanted a finite number >= 0; 0 = no cap)" % (self.norm_threshold,))
        if not abs(self.momentum) < 1:
            raise ValueError("CFG: momentum = %r (wanted |momentum| < 1)" % (self.momentum,))
        if not 0 <= self.rescale <= 1:
            raise ValueError("CFG: rescale = %r (wanted 0 <= rescale <= 1)" % (self.rescale,))
        if self.interval is not None:
            lo, hi = self.interval
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError("CFG: interval = %r (wanted finite lo <= hi)" % (self.interval,))

    def on(self, time_step, num_diffusion_steps):
        """is guidance on for the step that starts at schedule time ``time_step``"""
        if self.interval is None:
            return True
        return self.interval[0] <= float(time_step) / float(num_diffusion_steps) <= self.interval[1]

    def key(self):
        """hashable: what a graph key holds"""
        return ("cfg", self.eta, self.norm_threshold, self.momentum, self.rescale, self.interval)

    def options(self):
        """the keyword arguments of ``cfg_combine`` / ``ops.cfg_combine``"""
        return dict(eta=self.eta, norm_threshold=self.norm_threshold, momentum=self.momentum, rescale=self.rescale)

    def __repr__(self):
        return "CFG(eta=%r, norm_threshold=%r, momentum=%r, rescale=%r, interval=%r)" % (
            self.eta, self.norm_threshold, self.momentum, self.rescale, self.interval)


def _is_v(prediction_type):
    return (prediction_type.name if hasattr(prediction_type, "name") else str(prediction_type)).upper() == "V_PREDICTION"


def cfg_combine(x_t, pred, pred_uncond, g, prediction_type, guidance_scale, eta=1.0, norm_threshold=0.0, momentum=0.0,
                rescale=0.0, image_scale=1.0, run_prev=None, on=True):
    """torch ops of ``ops.cfg_combine`` (for CPU tensors; the module's formulas in the tensors' dtype) -> (p_g, run).
    ``g``: per-sample gamma, broadcast as [B, 1, 1, 1].  ``run_prev``: the ``run`` of the step before, None = no history.
    ``run`` is None without momentum.  ``on=False`` (outside the guidance interval): (pred, run_prev) themselves."""
    if not on:
        return pred, run_prev
    g = g.reshape(-1, 1, 1, 1).to(pred.dtype)
    if _is_v(prediction_type):
        a, be = g.sqrt(), -(1 - g).sqrt()
    else:
        a, be = 1 / g.sqrt(), -(1 - g).sqrt() / g.sqrt()
    sc = image_scale if image_scale else 1.0
    dims = (1, 2, 3)
    D = a * x_t + be * pred
    E = be * (pred - pred_uncond)
    if momentum != 0 and run_prev is not None:
        E = E + momentum * run_prev
    run = E if momentum != 0 else None
    chw = pred[0].numel()
    rms = sc * (E.pow(2).sum(dims, keepdim=True) / chw).sqrt()
    s = torch.ones_like(rms)
    if norm_threshold > 0:
        s = torch.where(rms > 0, (norm_threshold / rms.clamp_min(torch.finfo(rms.dtype).tiny)).clamp(max=1), s)
    dd = D.pow(2).sum(dims, keepdim=True)
    c = torch.where(dd > 0, (E * D).sum(dims, keepdim=True) / torch.where(dd > 0, dd, torch.ones_like(dd)), torch.zeros_like(dd))
    p_g = pred + (guidance_scale - 1) * s * (E - (1 - eta) * c * D) / be
    if rescale > 0:
        sd_c, sd_g = (t.var(dims, unbiased=False, keepdim=True).sqrt() for t in (pred, p_g))
        ratio = torch.where(sd_g > 0, sd_c / torch.where(sd_g > 0, sd_g, torch.ones_like(sd_g)), torch.ones_like(sd_g))
        p_g = p_g * torch.where(sd_g > 0, rescale * ratio + 1 - rescale, torch.ones_like(sd_g))
    return p_g, run
