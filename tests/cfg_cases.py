"""Projected and rescaled classifier-free guidance (mdm_hip/guidance.py): the definition restated in fp64 torch, and the
inputs, shapes and option sets that tests/test_cfg_host.py and tests/test_cfg_gpu.py share.

Per sample b, g = gamma[b], x0 = a x_t + be p  (V: a = sqrt(g), be = -sqrt(1 - g); eps: a = 1 / sqrt(g),
be = -sqrt(1 - g) / sqrt(g)), sc the image scale, w the guidance scale:

    D_c  = a x_t + be p_c
    dD   = be (p_c - p_u)  [+ momentum run_prev, where there is a history]
    run  = dD                                        (before the cap)
    rms  = sc sqrt(sum(dD^2) / chw)
    s    = min(1, norm_threshold / rms) if norm_threshold > 0 else 1       (rms == 0: 1)
    c    = sum(dD D_c) / sum(D_c^2)                                         (sum(D_c^2) == 0: 0)
    u    = s (dD - (1 - eta) c D_c)
    p_g  = p_c + (w - 1) u / be
    p_g  = p_g (rescale std(p_c) / std(p_g) + 1 - rescale) if rescale > 0   (std(p_g) == 0: factor 1)
    guidance off (outside the interval): p_g = p_c, run = run_prev
"""
import functools
import math

import torch

W = 7.5
GAMMAS = (0.98, 0.5, 0.02)
PRED_TYPES = ("V_PREDICTION", "DDPM")
# (B, C, H, W): below one wave; ragged against a 256-thread block; the UNet-64 image; several slabs with a ragged tail;
# one sample across many blocks
SHAPES = [(1, 3, 2, 2), (3, 3, 5, 4), (2, 3, 64, 64), (3, 3, 160, 136), (1, 3, 256, 256)]
OPTIONS = {
    "default": dict(),
    "eta0": dict(eta=0.0),
    "all": dict(eta=0.25, norm_threshold=0.1, momentum=-0.5, rescale=0.7),
    "rescale1": dict(rescale=1.0),
    "cap-momentum": dict(norm_threshold=0.05, momentum=0.5),
    # without momentum the update's RMS is 0.3 |be|: 0.04 at gamma = 0.98 (cap idle), 0.21 and 0.30 in the other rows (active)
    "cap-mixed": dict(norm_threshold=0.2),
}


def coeffs(g, pred_type):
    """(a, be), shaped like ``g``"""
    if pred_type == "V_PREDICTION":
        return g.sqrt(), -(1 - g).sqrt()
    return 1 / g.sqrt(), -(1 - g).sqrt() / g.sqrt()


def cfg_ref(x_t, p_c, p_u, gamma, pred_type, w, eta=1.0, norm_threshold=0.0, momentum=0.0, rescale=0.0, image_scale=1.0,
            run_prev=None, on=True):
    """fp64 -> (p_g, run, info); ``run`` is None without momentum; ``info``: per-sample rms (before the cap), s and c.
    The inputs are taken at the values they hold (fp32 inputs are widened, not re-drawn)."""
    d = lambda t: None if t is None else t.detach().double().cpu()   # the restatement runs on the host
    x_t, p_c, p_u, run_prev = d(x_t), d(p_c), d(p_u), d(run_prev)
    if not on:
        return p_c, run_prev, {}
    B = p_c.shape[0]
    g = d(torch.as_tensor(gamma)).reshape(B, 1, 1, 1)
    a, be = coeffs(g, pred_type)
    chw = p_c[0].numel()
    flat = lambda t: t.reshape(B, -1)
    D = a * x_t + be * p_c
    dD = be * (p_c - p_u)
    if momentum != 0 and run_prev is not None:
        dD = dD + momentum * run_prev
    run = dD.clone() if momentum != 0 else None
    rms = image_scale * (flat(dD).pow(2).sum(1) / chw).sqrt()
    s = torch.ones(B, dtype=torch.float64)
    c = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        if norm_threshold > 0 and float(rms[b]) > 0:
            s[b] = min(1.0, norm_threshold / float(rms[b]))
        dd = float(flat(D)[b].pow(2).sum())
        if dd > 0:
            c[b] = float((flat(dD)[b] * flat(D)[b]).sum()) / dd
    col = lambda v: v.reshape(B, 1, 1, 1)
    u = col(s) * (dD - (1 - eta) * col(c) * D)
    p_g = p_c + (w - 1) * u / be
    if rescale > 0:
        for b in range(B):
            sd_c, sd_g = (float(flat(t)[b].var(unbiased=False).sqrt()) for t in (p_c, p_g))
            if sd_g > 0:
                p_g[b] = p_g[b] * (rescale * sd_c / sd_g + 1 - rescale)
    return p_g, run, dict(rms=rms, s=s, c=c)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=0):
    """fp32: p_c, x_t ~ N(0, 1); p_u = p_c + 0.3 N(0, 1); run = 0.2 N(0, 1); gammas (0.98, 0.5, 0.02) per row"""
    B = shape[0]
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    p_c, x_t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    p_u = p_c + 0.3 * torch.randn(shape, generator=g)
    run = 0.2 * torch.randn(shape, generator=g)
    gamma = torch.tensor([GAMMAS[b % len(GAMMAS)] for b in range(B)])
    return dict(x_t=x_t, p_c=p_c, p_u=p_u, run=run, gamma=gamma)


@functools.lru_cache(maxsize=None)
def reference(shape, opt, pred_type, seed=0):
    """the fp64 result for ``inputs(shape, seed)`` under OPTIONS[opt] at w = W, computed once -> (p_g, run, info)"""
    i = inputs(shape, seed)
    kw = OPTIONS[opt]
    return cfg_ref(i["x_t"], i["p_c"], i["p_u"], i["gamma"], pred_type, W, run_prev=i["run"] if kw.get("momentum") else None, **kw)


def maxerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def paper_radius(norm_threshold, chw):
    """the L2 radius of the APG paper that the RMS cap ``norm_threshold`` stands for at ``chw`` elements"""
    return norm_threshold * math.sqrt(chw)
