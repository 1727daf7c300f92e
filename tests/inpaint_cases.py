"""Yardsticks for image-conditioned sampling (known-region replacement with resampling jumps, RePaint -- Lugmayr et al.
2022; late start, SDEdit -- Meng et al. 2022) that do not come from the package under test.  The reference has neither,
so there is no golden: everything here is the published arithmetic written out in fp64 with nothing imported from
``mdm_hip``.

(a) ``blend`` / ``jump``: the two per-pixel formulas.
(b) ``pyramid``: the per-scale known images and masks of a nested model (a low-resolution pixel is known only where every
    pixel of its block is).
(c) ``shifted``: the per-scale gamma of a nested model with a shifted schedule, SNR' = SNR / s^p.
(d) ``reference_loop``: DDIM(eta = 0) on a v-prediction denoiser with the blend after every step and ``resample``
    repetitions of every step but the last, consuming a given list of normals in launch order.
"""
import torch
import torch.nn.functional as F


def _col(v):
    return torch.as_tensor(v, dtype=torch.float64).reshape(-1, 1, 1, 1)


def blend(x, known, mask, gamma, inv_scale, noise):
    """k = sqrt(g) known inv_scale + sqrt(1 - g) n;  x where m == 0, k where m == 1, m k + (1 - m) x in between"""
    x, known, m, n = x.double(), known.double(), mask.double(), noise.double()
    g = _col(gamma)
    k = g.sqrt() * known * inv_scale + (1 - g).sqrt() * n
    out = m * k + (1 - m) * x
    out = torch.where(m == 1, k, out)
    return torch.where(m.expand_as(x) == 0, x, out)


def jump(x_s, g_t, g_s, noise, gate=True):
    """forward transition from level g_s back to the noisier g_t: a = g_t / g_s, x_t = sqrt(a) x_s + sqrt(1 - a) n"""
    if not gate:
        return x_s.double()
    a = _col(g_t) / _col(g_s)
    return a.sqrt() * x_s.double() + (1 - a).clamp(min=0).sqrt() * noise.double()


def pyramid(known, mask, ratios):
    """hi -> lo lists for ``ratios`` (top side / side).  Images: block means.  Masks: the top scale as given; below, 1
    where the MINIMUM over the block of (mask == 1) is 1, else 0."""
    ks, ms = [known.double()], [mask.double()]
    full = (mask == 1).double()
    for r in ratios[1:]:
        ks.append(F.avg_pool2d(known.double(), r))
        ms.append(-F.max_pool2d(-full, r))
    return ks, ms


def shifted(gamma, scale, power=1):
    """SNR' = SNR / scale^power for scale > 1 (gamma = 1 stays 1)"""
    gamma = torch.as_tensor(gamma, dtype=torch.float64)
    if scale <= 1:
        return gamma
    s = float(scale) ** power
    return torch.where(gamma >= 1, torch.ones_like(gamma), gamma / (gamma + s * (1 - gamma)))


def reference_loop(x_T, gammas, steps, v_of, known, mask, noises, resample=1, inv_scale=1.0):
    """-> the state after every step (after its last repetition and blend), fp64.  ``gammas``: the schedule table;
    ``steps``: descending times ending in 0; ``v_of(x, g)``: the denoiser's v-prediction at gamma g; ``noises``: normals
    shaped like x, consumed one per blend and one per jump, in that order within a repetition."""
    noises = iter(noises)
    x, out = x_T.double(), []
    B = x.shape[0]
    for i, (t, s) in enumerate(zip(steps[:-1], steps[1:])):
        g_t, g_s = gammas[t].double().expand(B), gammas[s].double().expand(B)
        reps = resample if i < len(steps) - 2 else 1
        for rep in range(reps):
            a_t, s_t, a_s, s_s = _col(g_t).sqrt(), (1 - _col(g_t)).sqrt(), _col(g_s).sqrt(), (1 - _col(g_s)).sqrt()
            x0 = a_t * x - s_t * v_of(x, _col(g_t))
            eps = (x - a_t * x0) / s_t
            x = a_s * x0 + s_s * eps                      # DDIM(eta = 0)
            x = blend(x, known, mask, g_s, inv_scale, next(noises))
            if rep < reps - 1:
                x = jump(x, g_t, g_s, next(noises))
        out.append(x)
    return out
