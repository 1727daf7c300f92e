"""Noise schedules and the DDPM / DDIM sampling update around the denoiser.

Host-side mirror of ``ml_mdm.samplers`` (reference ml-mdm-matryoshka/ml_mdm/samplers.py):
``SamplerConfig`` (:67-118), the schedule families (:126-165), ``Sampler`` (:177-609) and
``NestedSampler`` (:612-793) with the same public method names, so the reference's
``Diffusion`` / CLIs can drive it.

Per-pixel arithmetic: on GPU tensors one reverse step --
guidance combine, v/eps -> x0, clip / dynamic threshold, DDPM posterior or DDIM(eta)
update, noise -- is ONE kernel per scale (``ops.sampler_step`` -> ``mdm_sampler_step``);
there is no fallback from that path (a missing library raises).  The same formulas written
with torch ops serve CPU tensors: that is what the host-logic tests drive against the
reference's golden outputs (tests/test_diffusion_host.py), and what a custom ``clip_fn``
gets.  One deliberate difference from the reference: gammas are per-sample ``[B, 1, 1, 1]``
tensors, broadcast, instead of being materialised at full image size (:196-199).

Beyond the reference: ``sample(..., solver="dpmpp_2m")`` replaces the first-order update by
DPM-Solver++(2M) (Lu et al. 2022; ``get_prediction_xt_last_2m`` -> ``ops.sampler_step_2m``),
same structure -- one kernel per scale on GPU tensors, torch ops on CPU tensors; ``solver=SASolver(...)`` / ``"sa"`` by
SA-Solver (Xue et al. 2023; ``get_prediction_xt_last_sa`` -> ``ops.sampler_step_sa``), a stochastic Adams
predictor-corrector of up to third order, the same way.  So does image conditioning:
``sample(..., known_images=, known_mask=, resample=, known_seed=)`` holds a region of every trajectory on a given image
(the replacement method of RePaint, Lugmayr et al. 2022, with its resampling jumps; ``KnownRegion`` ->
``ops.sampler_known_blend`` / ``ops.sampler_jump``), and ``Diffusion.partial_diffusion`` starts a trajectory late from a
noised image (SDEdit, Meng et al. 2022).  Six options act on the denoiser call or on the prediction handed to the update
and leave the update alone -- loss guidance (``guide``), perturbed-attention guidance (``pag_scale`` / ``pag_layers``), regional
prompts and token weights (``regions`` / ``region_layers``), FreeU (``freeu``), projected / rescaled classifier-free
guidance (``cfg``) and tiled sampling of a canvas larger than the model's window (``tiles``): ``SampleOptions`` says what each
does, holds their checks and is what travels from ``sample`` to the step.  Image inversion goes the other way, from a GIVEN
image to the noise and the trajectory that reproduce it: ``Sampler.invert`` (DDIM inversion with fixed-point refinement;
``ops.sampler_invert_step`` / ``invert_step``) and ``Sampler.noise_maps`` with ``sample(..., step_noise=maps)`` (edit-friendly
DDPM inversion; ``ops.sampler_noise_map`` / ``noise_map``); the update rules and the reverse-step kernels are untouched by it.
"""
import contextlib
import math
from dataclasses import dataclass, fields
from enum import Enum

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import freeu as _freeu
from . import guidance as _guidance
from . import ops, pag
from . import regions as _regions
from . import attn_maps as _attn_maps
from . import attn_control as _attn_control
from . import tiling as _tiling
from .unet import switched


class ScheduleType(Enum):
    COSINE = 0
    DDPM = 1
    DEEPFLOYD = 2


class PredictionType(Enum):
    DDPM = 0
    DDIM = 1
    V_PREDICTION = 2


class ThresholdType(Enum):
    NONE = 0
    CLIP = 1
    DYNAMIC = 2
    DYNAMIC_IF = 3


def _enum(cls, v):
    return v if isinstance(v, cls) else cls[str(v).upper()]


QUANTILE_ROW_LIMIT = 1 << 24   # torch.quantile refuses a longer row ("input tensor is too large")


def dynamic_threshold_ref(x0s, ratio, vmax):
    """The per-sample threshold [B] of the dynamic threshold functions in torch ops: the ``ratio`` quantile of |x0s| over
    everything behind the first axis, clamped to [1, vmax] -- ``torch.quantile``'s own rule written out, so that it holds
    for rows of any length.  With a = |x0s| sorted ascending along a row of n values:

        rank = ratio (n - 1) in the dtype of the data (fp32 data: an fp32 product) ; lo = floor(rank) ;
        hi = min(ceil(rank), n - 1) ; w = rank - lo ; quantile = lerp(a[lo], a[hi], w)

    A row that holds a NaN gives NaN.  fp32 unless ``x0s`` is fp64.  Up to 2^24 values per row this is ``torch.quantile``
    bit for bit; ``ops.abs_quantile`` computes the same on the GPU without the sort."""
    flat = x0s if x0s.dtype == torch.float64 else x0s.float()
    a = flat.reshape(flat.shape[0], -1).abs().sort(dim=1).values
    n = a.shape[1]
    rank = torch.tensor(ratio, dtype=a.dtype) * (n - 1)
    lo = min(int(rank.floor()), n - 1)
    hi = min(int(rank.ceil()), n - 1)
    w = (rank - rank.floor()).to(a.device)
    quant = torch.lerp(a[:, lo], a[:, hi], w)
    quant = torch.where(a[:, -1].isnan(), torch.full_like(quant, float("nan")), quant)   # NaN sorts last
    return quant.clamp(min=1, max=vmax)


def _abs_quantile_clamped(flat, ratio, vmax):
    """clamp(quantile_ratio |flat[b]|, 1, vmax) of a [B, n] tensor.  fp32 on the GPU: the radix select
    (``ops.abs_quantile``; it has no backward, so a tensor that asks for a gradient keeps the torch ops).  Otherwise
    ``torch.quantile`` up to its row limit and the same rule by a sort beyond it."""
    if flat.is_cuda and flat.dtype == torch.float32 and not (flat.requires_grad and torch.is_grad_enabled()):
        return ops.abs_quantile(flat, ratio, 1, vmax)
    if flat.shape[1] > QUANTILE_ROW_LIMIT:
        return dynamic_threshold_ref(flat, ratio, vmax)
    return torch.quantile(flat.abs(), ratio, dim=1).clamp(min=1, max=vmax)


@dataclass
class SamplerConfig:
    num_diffusion_steps: int = 32
    reproject_signal: bool = False
    schedule_type: ScheduleType = ScheduleType.DDPM
    prediction_type: PredictionType = PredictionType.DDPM
    loss_target_type: PredictionType = None
    beta_start: float = 0.0001
    beta_end: float = 0.02
    threshold_function: ThresholdType = ThresholdType.CLIP
    rescale_schedule: float = 1.0
    rescale_signal: float = None
    schedule_shifted: bool = False
    schedule_shifted_power: float = 1

    def __post_init__(self):
        self.schedule_type = _enum(ScheduleType, self.schedule_type)
        self.prediction_type = _enum(PredictionType, self.prediction_type)
        if self.loss_target_type is not None:
            self.loss_target_type = _enum(PredictionType, self.loss_target_type)
        self.threshold_function = _enum(ThresholdType, self.threshold_function)


def gammas_cosine(n, logsnr_min=-5.0, logsnr_max=5.0):
    """reference :126-136 (progressive-distillation cosine log-SNR schedule); gamma_0 = 1."""
    t = np.linspace(0.0, 1.0, num=n)
    b = np.arctan(np.exp(-0.5 * logsnr_max))
    a = np.arctan(np.exp(-0.5 * logsnr_min)) - b
    logsnr = -2.0 * np.log(np.tan(a * t + b))
    return np.concatenate(([1.0], 1.0 / (1.0 + np.exp(-logsnr))))


def gammas_linear_beta(n, beta_start, beta_end):
    """reference :139-146 (Ho et al. linear betas); gamma_t = prod_{s<=t} (1 - beta_s), beta_0 = 0."""
    betas = np.concatenate(([0.0], np.linspace(beta_start, beta_end, num=n)))
    return np.exp(np.cumsum(np.log(1.0 - betas)))


def gammas_squaredcos_cap_v2(n):
    """reference :149-165 (DeepFloyd / diffusers squaredcos_cap_v2), betas capped at 0.999."""
    bar = lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = np.asarray([0.0] + [min(1 - bar((i + 1) / n) / bar(i / n), 0.999) for i in range(n)])
    return np.exp(np.cumsum(np.log(1.0 - betas)))


def _b(v):
    """[B] -> [B, 1, 1, 1]"""
    return v.reshape(-1, 1, 1, 1)


SOLVERS = ("dpmpp_2m", "sa")


# an entry of a trajectory dict, in the form x_t has (a tensor, or a hi -> lo list) -> the list, or None
_listed = lambda v: v if v is None or isinstance(v, (list, tuple)) else [v]


class StepRule:
    """The update rule of a trajectory: what ``solver=`` resolves to (``_rule_of``), once, at the entry points.  The eager
    loop and ``GraphedSampler`` consume it alike, from the host the one, from device tables the other.  A rule of one's
    own subclasses this and gives ``key``, ``rows`` and ``step``.
    ``key``: hashable, the rule's part of a graph key.  ``history``: how many earlier nodes' gammas ``step`` reads (0 .. 2).
    ``check(ddim_eta, opts, known_images, resample)``: what the rule refuses of a call.  ``rows(sampler, times, times_last)``
    -> host float32 [len(times), width]: all that varies from step to step over the steps ``times`` -> ``times_last`` (host
    arrays), counted from ``times[0]``, the first step of a trajectory wherever on the schedule it starts.  ``buffers(xs)``
    -> the per-scale fp32 state the step kernels update in place, a dict of hi -> lo lists.  ``step(sampler, k, x_t, pred,
    g_t, g_s, row, g_hist, state, **common)`` -> (x0, x_s) of scale ``k``; ``row``: one row of ``rows``, host numbers in the
    eager loop and a device float[1, width] in a captured graph; ``g_hist[j][k]``: the gamma of the node j + 1 steps back;
    ``state``: what ``buffers`` (graph) or ``load`` (eager) made; ``common``: what every rule hands on to
    ``get_prediction_xt_last*`` (prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale, thr_out, rng) and
    ``noise_fn``, the caller's ``solver_noise_fn``.  The eager trajectory dict ``st`` (``solver_state`` of ``get_xt_minus_1``):
    ``row`` makes the row of one such call from it and from what the ``caller`` decides (``second_order``), ``load`` makes
    (g_hist, state) from it, ``store`` leaves the step's results in it."""

    history = 0

    def check(self, ddim_eta, opts, known_images, resample):
        if ddim_eta is not None:
            raise ValueError("solver=%r has no ddim_eta (got %r): dpmpp_2m is deterministic, SASolver takes tau=" % (self.key, ddim_eta))
        if resample > 1:
            raise ValueError("resample=%d with solver=%r: the multistep history is void after a jump" % (resample, self.key))

    def row(self, sampler, st, time_step, last, **caller):
        return self.rows(sampler, np.array([int(time_step)]), np.array([int(last)]))[0]

    buffers = lambda self, xs: {}                               # a rule without history: nothing to keep,
    load = lambda self, sampler, st, xs, g_t: ([], {})          # nothing to load
    store = lambda self, sampler, st, state, x0, g_t, row: None   # and nothing to store


class Ancestral(StepRule):
    """``solver=None``: the reference's two, the ancestral DDPM posterior or DDIM(``ddim_eta``).  Row: the noise gate."""

    def __init__(self, ddim_eta=None):
        self.ddim_eta, self.key = ddim_eta, ("ancestral", ddim_eta)

    check = lambda self, *call: None   # it refuses nothing

    def rows(self, sampler, times, times_last):
        return np.asarray(sampler._noisy_step(times, times_last), dtype="float32").reshape(-1, 1)

    def step(self, sampler, k, x_t, pred, g_t, g_s, row, g_hist, state, noise_fn=None, **common):
        gate = row if torch.is_tensor(row) else None   # a captured graph draws on every row; the device gate decides
        x0, x_s, _ = sampler.get_prediction_xt_last(x_t, pred, g_t, g_s, need_noise=gate is not None or bool(row[0]),
                                                    ddim_eta=self.ddim_eta, return_eps=False, noise_gate=gate, **common)
        return x0, x_s


class DPMpp2M(StepRule):
    """``solver="dpmpp_2m"``.  Row: the order gate -- second order where there is history and a finite step in log-SNR: not on
    the first and not on the last step of a trajectory (0, 1, .., 1, 0).  State: "x0" of the step before, formed at ``g_hist[0]``."""

    key, history = "dpmpp_2m", 1

    def rows(self, sampler, times, times_last):
        order = np.zeros((len(times), 1), dtype="float32")
        order[1:-1, 0] = np.asarray(times[:-2]) > np.asarray(times[1:-1])
        return order

    def buffers(self, xs):
        x0 = [torch.zeros_like(x, dtype=torch.float32) for x in xs]
        return dict(x0=x0, x0_out=x0)

    def row(self, sampler, st, time_step, last, second_order=False):
        return np.float32([bool(second_order)])   # the caller's decision

    def load(self, sampler, st, xs, g_t):
        none = [None] * len(xs)
        return [_listed(st.get("g")) or none], dict(x0=_listed(st.get("x0")) or none, x0_out=none)

    def store(self, sampler, st, state, x0, g_t, row):
        st["x0"], st["g"] = sampler._from_scales(x0), sampler._from_scales(g_t)

    def step(self, sampler, k, x_t, pred, g_t, g_s, row, g_hist, state, rng=None, noise_fn=None, **common):
        return sampler.get_prediction_xt_last_2m(
            x_t, pred, g_t, g_s, g_prev=g_hist[0][k], x0_prev=state["x0"][k], x0_out=state["x0_out"][k],
            second_order=row if torch.is_tensor(row) else bool(row[0]), **common)


@dataclass(frozen=True)
class SASolver(StepRule):
    """``solver=SASolver(predictor=3, corrector=3, tau=0.0, tau_interval=None)``: SA-Solver (Xue et al., NeurIPS 2023,
    "SA-Solver: Stochastic Adams Solver for Fast Sampling of Diffusion Models"); ``solver="sa"`` means the defaults.

    On the data prediction, per scale and per sample, with alpha = sqrt(gamma), sigma = sqrt(1 - gamma), lambda =
    log(alpha / sigma), a step from node a to node b of h = lambda_b - lambda_a, kappa = 1 + tau^2, m_j the guided,
    thresholded x0 formed at node j and l_j the Lagrange basis over the offsets s_j = lambda_j - lambda_a:

        x_b = (sigma_b / sigma_a) e^{-tau^2 h} x_a + alpha_b sum_j c_j m_j + sigma_b sqrt(-expm1(-2 tau^2 h)) z
        c_j = kappa int_0^h e^{-kappa (h - s)} l_j(s) ds

    ``predictor`` = P in 1..3: exponential Adams-Bashforth over nodes a, a-1, .., of order min(P, i + 1) at launch i of a
    trajectory.  ``corrector`` = C in 0..3 (0 = none): Adams-Moulton -- the step a-1 -> a redone over nodes a, a-1, ..
    once m_a is known, which is the denoiser call the next step makes anyway: no extra evaluation.  Off at i = 0, order
    min(C, i + 1) afterwards.  It shares the x_{a-1} term and the noise with the predictor, so it is applied as a
    difference and whatever was done to x_a after the step (the known-region blend) survives it.
    ``tau`` >= 0: 0 is the probability-flow ODE, 1 the reverse SDE (first order: DDIM(eta = 0) and DDIM(eta = 1)).
    ``tau_interval = (lo, hi)`` in fractions of ``num_diffusion_steps``: tau acts where lo <= t / T <= hi for the time t
    the step starts from, 0 outside; None = everywhere.
    The last step (to gamma = 1) is first order with tau = 0 and no corrector: x = x0.  A late start restarts the count."""

    predictor: int = 3
    corrector: int = 3
    tau: float = 0.0
    tau_interval: object = None

    def __post_init__(self):
        if isinstance(self.predictor, bool) or int(self.predictor) != self.predictor or not 1 <= self.predictor <= 3:
            raise ValueError("SASolver: predictor = %r (wanted 1, 2 or 3)" % (self.predictor,))
        if isinstance(self.corrector, bool) or int(self.corrector) != self.corrector or not 0 <= self.corrector <= 3:
            raise ValueError("SASolver: corrector = %r (wanted 0 .. 3; 0 = no corrector)" % (self.corrector,))
        if not (math.isfinite(self.tau) and self.tau >= 0):
            raise ValueError("SASolver: tau = %r (wanted a finite number >= 0)" % (self.tau,))
        object.__setattr__(self, "predictor", int(self.predictor))
        object.__setattr__(self, "corrector", int(self.corrector))
        object.__setattr__(self, "tau", float(self.tau))
        if self.tau_interval is not None:
            try:
                lo, hi = self.tau_interval
                lo, hi = float(lo), float(hi)
            except (TypeError, ValueError):
                raise ValueError("SASolver: tau_interval = %r (wanted (lo, hi) in fractions of the schedule, or None)"
                                 % (self.tau_interval,))
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError("SASolver: tau_interval = %r (wanted finite lo <= hi)" % (self.tau_interval,))
            object.__setattr__(self, "tau_interval", (lo, hi))

    def tau_at(self, time_step, num_diffusion_steps):
        """tau of the step that starts at schedule time ``time_step``"""
        if self.tau_interval is None:
            return self.tau
        inside = self.tau_interval[0] <= float(time_step) / float(num_diffusion_steps) <= self.tau_interval[1]
        return self.tau if inside else 0.0

    def gate(self, count, time_step, time_step_last, num_diffusion_steps, tau_prev=0.0):
        """-> (predictor order, corrector order, tau, tau of the step before) of launch ``count`` (0 = the first of this
        trajectory), a step from ``time_step`` to ``time_step_last`` (0: the last step)"""
        if int(time_step_last) >= int(time_step):
            raise ValueError("SASolver: a step from time %d to time %d has no positive step in log-SNR (more inference "
                             "steps than the schedule has?)" % (int(time_step), int(time_step_last)))
        if int(time_step_last) == 0:
            return (1, 0, 0.0, 0.0)
        c = 0 if count == 0 else min(self.corrector, count + 1)
        return (min(self.predictor, count + 1), c, self.tau_at(time_step, num_diffusion_steps), float(tau_prev) if c else 0.0)

    def gates(self, times, times_last, num_diffusion_steps):
        """the gates of a whole trajectory over the steps ``times`` -> ``times_last`` (host arrays): a list of 4-tuples"""
        out, tau_prev = [], 0.0
        for i, (t, s) in enumerate(zip(times, times_last)):
            out.append(self.gate(i, int(t), int(s), num_diffusion_steps, tau_prev))
            tau_prev = out[-1][2]
        return out

    # ---- the StepRule.  Row: the gate.  State: "h0", "h1" (the x0 of the launches before, formed at ``g_hist``), "psum"
    history, key = 2, property(lambda self: self)

    def check(self, ddim_eta, opts, known_images, resample):
        StepRule.check(self, ddim_eta, opts, known_images, resample)
        if opts.map_guide is not None:
            raise NotImplementedError("map_guide= together with an SA solver: a correction of x_t between the predictor's "
                                      "launch and the corrector's, which redoes that step from the history, is not "
                                      "implemented -- as for guide=")
        if opts.guide is not None:
            raise NotImplementedError("guide= together with an SA solver: the guide's correction of x_s between the "
                                      "predictor and the corrector that redoes the step is not implemented")

    def rows(self, sampler, times, times_last):
        return np.asarray(self.gates(times, times_last, sampler.n_steps), dtype="float32").reshape(-1, 4)

    def buffers(self, xs):
        zeros = lambda on: [torch.zeros_like(x, dtype=torch.float32) if on else None for x in xs]
        h0 = zeros(True)   # x0 goes straight into h0: the kernel reads its elements of h0 before it writes them
        return dict(h0=h0, h1=zeros(max(self.predictor, self.corrector) >= 3), psum=zeros(self.corrector >= 1), x0_out=h0)

    def _host_gate(self, row):
        """a host row -> the gate in host numbers, tau as the solver holds it (a float32 row has rounded it)"""
        tau = lambda v: self.tau if np.float32(v) == np.float32(self.tau) else float(v)
        return int(row[0]), int(row[1]), tau(row[2]), tau(row[3])

    def row(self, sampler, st, time_step, last, **caller):
        return self.gate(st.get("count", 0), time_step, last, sampler.n_steps, st.get("tau", 0.0))

    def load(self, sampler, st, xs, g_t):
        none = [None] * len(xs)
        fresh = self.buffers(xs) if st.get("h0") is None and xs[0].is_cuda else {}
        state = {name: list(_listed(st.get(name)) or fresh.get(name, none)) for name in ("h0", "h1", "psum")}
        g0 = _listed(st.get("g0")) or list(g_t)   # no history yet: this step's own gamma stands in, unread
        return [g0, _listed(st.get("g1")) or g0], dict(state, x0_out=none)   # eager: x0 is the caller's, a tensor of its own

    def store(self, sampler, st, state, x0, g_t, row):
        for name in ("h0", "h1", "psum"):
            st[name] = sampler._from_scales(state[name])
        st["g1"], st["g0"] = st.get("g0"), sampler._from_scales(g_t)
        st["count"], st["tau"] = st.get("count", 0) + 1, self._host_gate(row)[2]

    def step(self, sampler, k, x_t, pred, g_t, g_s, row, g_hist, state, rng=None, noise_fn=None, **common):
        gate = row if torch.is_tensor(row) else self._host_gate(row)
        given = noise_fn is not None and not torch.is_tensor(row) and gate[2] > 0
        x0, x_s, new = sampler.get_prediction_xt_last_sa(
            x_t, pred, g_t, g_s, gate=gate, max_order=(self.predictor, self.corrector), rng=rng, stochastic=self.tau > 0,
            input_noise=noise_fn(x_t) if given else None, x0_out=state["x0_out"][k], g_h0=g_hist[0][k], g_h1=g_hist[1][k],
            **{name: state[name][k] for name in ("h0", "h1", "psum")}, **common)
        state["h0"][k], state["h1"][k], state["psum"][k] = new
        return x0, x_s


def _rule_of(solver, ddim_eta=None):
    """``solver=`` as given -> its ``StepRule``: None (DDPM / DDIM(``ddim_eta``)), a name of ``SOLVERS``, or a rule"""
    if solver is None:
        return Ancestral(ddim_eta)
    if isinstance(solver, StepRule):
        return solver
    if isinstance(solver, str) and solver in SOLVERS:
        return DPMpp2M() if solver == "dpmpp_2m" else SASolver()
    raise ValueError("unknown solver %r (known: %s, or an SASolver; None = DDPM / DDIM)" % (solver, ", ".join(SOLVERS)))


def _checked_rule(solver, ddim_eta, opts, known_images=None, resample=1):
    """what every entry point does with ``solver=``: resolve it, and refuse what the call cannot have -> the rule"""
    rule = _rule_of(solver, ddim_eta)
    _check_known(known_images, resample)
    rule.check(ddim_eta, opts, known_images, resample)
    return rule


def _dlambda(ga, gb):
    """lambda(gb) - lambda(ga) for lambda = log(sqrt(g) / sqrt(1 - g)), without cancellation (as the 2M update takes it)"""
    return 0.5 * torch.log1p((gb - ga) / (ga * (1 - gb)))


def _sa_phi(x):
    """phi_n(x) = x int_0^1 e^{-x (1 - u)} u^n du for n = 0, 1, 2 (x > 0): the moments of the SA-Solver integral in units
    of h^n.  Below x = 1 the series n! sum_k (-1)^k x^(k+1) / (n + k + 1)! in nested form (20 terms, no cancellation),
    from there on phi_0 = -expm1(-x), phi_n = 1 - (n / x) phi_{n-1} -- what the kernel does in fp64."""
    small = x < 1
    xs = torch.where(small, x, torch.ones_like(x))
    series = []
    for n in range(3):
        s = torch.ones_like(xs)
        for k in range(19, 0, -1):
            s = 1 - xs * s / (n + k + 1)
        series.append(xs * s / (n + 1))
    xl = torch.where(small, torch.ones_like(x), x)
    p0 = -torch.expm1(-xl)
    p1 = 1 - p0 / xl
    p2 = 1 - 2 * p1 / xl
    return [torch.where(small, a, b) for a, b in zip(series, (p0, p1, p2))]


def sa_predictor_coeffs(h, tau, order, h1=None, h2=None):
    """c_j of the SA-Solver predictor for a step of ``h`` in lambda from node a: (c_a, c_{a-1}, c_{a-2}) (zeros beyond
    ``order``), ``h1`` = lambda_a - lambda_{a-1}, ``h2`` = lambda_{a-1} - lambda_{a-2}.  Tensors of one shape, fp64 for
    full accuracy; ``tau`` and ``order`` host numbers."""
    phi = _sa_phi((1 + tau * tau) * h)
    zero = torch.zeros_like(h)
    if order == 1:
        return phi[0], zero, zero
    u1 = -h1 / h
    if order == 2:
        c1 = phi[1] / u1
        return phi[0] - c1, c1, zero
    u2 = u1 - h2 / h
    c1 = (phi[2] - u2 * phi[1]) / (u1 * (u1 - u2))
    c2 = (phi[2] - u1 * phi[1]) / (u2 * (u2 - u1))
    return phi[0] - c1 - c2, c1, c2


def sa_corrector_coeffs(h, tau, order, h2=None):
    """c_j of the SA-Solver corrector for the step of ``h`` in lambda from node a-1 to node a, taken at ``tau``:
    (c_a, c_{a-1}, c_{a-2}) (zeros beyond ``order``), ``h2`` = lambda_{a-1} - lambda_{a-2}"""
    phi = _sa_phi((1 + tau * tau) * h)
    zero = torch.zeros_like(h)
    if order == 1:
        return phi[0], zero, zero
    if order == 2:
        return phi[1], phi[0] - phi[1], zero
    u2 = -h2 / h
    ca = (phi[2] - u2 * phi[1]) / (1 - u2)
    c2 = (phi[2] - phi[1]) / (u2 * (u2 - 1))
    return ca, phi[0] - ca - c2, c2


def _check_known(known_images, resample):
    if int(resample) != resample or resample < 1:
        raise ValueError("resample must be an integer >= 1 (got %r)" % (resample,))
    if resample > 1 and known_images is None:
        raise ValueError("resample=%d repeats the steps around a known region: it needs known_images" % resample)


def pag_combine(pred, pred_uncond, pred_pert, guidance_scale=1, pag_scale=0.0):
    """torch ops of ``ops.pag_combine`` (for CPU tensors): classifier-free guidance plus perturbed-attention guidance (Ahn
    et al. 2024),  p_u + w (p_c - p_u) + s (p_c - p_hat);  p_c alone in front where ``pred_uncond`` is None"""
    base = pred if pred_uncond is None else pred_uncond + guidance_scale * (pred - pred_uncond)
    return base + pag_scale * (pred - pred_pert)


def pag_rows(n, lm_outputs, lm_mask, micros):
    """The conditioning of a perturbed-attention-guidance batch: the model's rows [uncond | cond] (or [cond]) followed by
    the ``n`` perturbed rows, which carry the CONDITIONAL rows -- the last ``n`` -- of ``lm_outputs``, ``lm_mask`` and every
    per-row tensor of ``micros`` once more.  -> (lm_outputs, lm_mask, micros)"""
    rows = lm_outputs.shape[0]
    ext = lambda v: torch.cat([v, v[-n:]])
    per_row = lambda v: torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == rows
    return (ext(lm_outputs), None if lm_mask is None else ext(lm_mask),
            {k: ext(v) if per_row(v) else v for k, v in micros.items()})


def repeat_rows(xs, t, reps):
    """every scale of ``xs`` and the times ``t`` once per block of the model batch ([uncond | cond | perturbed]: ``reps``
    of them); one block: as given, no copy"""
    return (xs, t) if reps == 1 else ([torch.cat([x] * reps) for x in xs], torch.cat([t] * reps))


def split_rows(preds, uncond, pert):
    """what the model made of such a batch, per scale -> (conditional predictions, unconditional ones or Nones, perturbed
    ones or None): the blocks present are [uncond |] cond [| perturbed]"""
    if not (uncond or pert):
        return list(preds), [None] * len(preds), None
    parts = [p.chunk(1 + uncond + pert) for p in preds]
    return ([p[int(uncond)] for p in parts], [p[0] if uncond else None for p in parts],
            [p[-1] for p in parts] if pert else None)


def model_rows(opts, guidance_scale, B, T, lm_outputs, lm_mask, micros):
    """The conditioning as the model's rows see it, from what ``sample`` was given ([uncond | cond], or [cond]): the
    perturbed block's rows appended (``pag_rows``), then every row once per window of ``opts.tiles`` (``T`` of them;
    ``tiling.cond_rows``).  The same for every step of a call.  -> (lm_outputs, lm_mask, micros)"""
    uncond, pert = opts.blocks(guidance_scale)
    if uncond or pert:
        assert B * (1 + uncond) == lm_outputs.shape[0]
    if pert:
        lm_outputs, lm_mask, micros = pag_rows(B, lm_outputs, lm_mask, micros)
    if opts.tiles is not None:
        lm_outputs, lm_mask, micros = _tiling.cond_rows(T, lm_outputs, lm_mask, micros)
    return lm_outputs, lm_mask, micros


def gather_windows(xs, tiles, ratios, reps):
    """every scale of ``xs`` (canvases, hi -> lo, ``ratios`` = top side / side) -> the windows of ``tiles`` as rows of the
    model batch, once per block (``reps``): one ``ops.tiles_gather`` per scale on GPU tensors, ``tiling.gather`` otherwise"""
    out = []
    for x, r in zip(xs, ratios):
        tl = tiles.at(r)
        out.append(ops.tiles_gather(x.float(), tl.window, tl.stride, reps) if x.is_cuda else _tiling.gather(x, tl, reps))
    return out


def merge_windows(preds, tiles, ratios, canvases):
    """the model's predictions on such rows -> whole-canvas predictions [reps B, C, H, W] per scale (``canvases``: the
    (H, W) of every scale): one ``ops.tiles_merge`` per scale on GPU tensors, ``tiling.merge`` otherwise"""
    out = []
    for p, r, (H, W) in zip(preds, ratios, canvases):
        tl = tiles.at(r)
        out.append(ops.tiles_merge(p.float(), H, W, tl.window, tl.stride, tl.blend) if p.is_cuda
                   else _tiling.merge(p, tl, H, W))
    return out


def known_blend(x, known, mask, g, inv_scale=1.0, noise=None):
    """torch ops of ``ops.sampler_known_blend`` (for CPU tensors; not in place):  k = sqrt(g) known inv_scale +
    sqrt(1 - g) n;  x where mask == 0, k where mask == 1, m k + (1 - m) x in between.  ``g`` broadcasts as [B, 1, 1, 1]."""
    g = _b(g)
    k = g.sqrt() * (known * inv_scale) + (1 - g).sqrt() * noise
    return torch.where(mask == 0, x, torch.where(mask == 1, k, mask * k + (1 - mask) * x))


def jump(x_s, g_t, g_s, noise):
    """torch ops of ``ops.sampler_jump``: the forward transition from level g_s back to the noisier g_t"""
    a = _b(g_t) / _b(g_s)
    return a.sqrt() * x_s + (1 - a).clamp(min=0).sqrt() * noise


def invert_step(x_s, pred, g_s, g_t, prediction_type, pred_uncond=None, guidance_scale=1):
    """torch ops of ``ops.sampler_invert_step`` (for CPU tensors): the preimage of one DDIM(0) step with the prediction held
    fixed.  With alpha = sqrt(g), sigma = sqrt(1 - g), ``g_s`` the cleaner level (g_s > g_t; g_s == 1 allowed) and p the
    guided prediction:

        eps:  x_t = (alpha_t / alpha_s) (x_s - sigma_s p) + sigma_t p
        v:    x_t = (x_s - (sigma_s alpha_t - alpha_s sigma_t) p) / (alpha_s alpha_t + sigma_s sigma_t)

    so that ``get_prediction_xt_last(x_t, p, g_t, g_s, ddim_eta=0)`` without a threshold returns ``x_s``.  The small
    coefficients come as quotients, (sigma_t alpha_s)^2 - (alpha_t sigma_s)^2 = g_s - g_t, not as differences: between
    neighbouring nodes of a 1000-step schedule the difference would cancel to a few digits."""
    p = pred if pred_uncond is None else pred_uncond + guidance_scale * (pred - pred_uncond)
    g_s, g_t = _b(g_s), _b(g_t)
    a_s, s_s, a_t, s_t = g_s.sqrt(), (1 - g_s).sqrt(), g_t.sqrt(), (1 - g_t).sqrt()
    cross = s_t * a_s + a_t * s_s
    if _enum(PredictionType, prediction_type) == PredictionType.V_PREDICTION:
        inv = 1 / (a_s * a_t + s_s * s_t)
        return inv * x_s + (g_s - g_t) / cross * inv * p
    return a_t / a_s * x_s + (g_s - g_t) / (cross * a_s) * p


def noise_map(x_s, mu, g, g_last, ddim_eta=None):
    """torch ops of the last line of ``ops.sampler_noise_map``: z = (x_s - mu) / sigma for the mean ``mu`` of the step from
    level ``g`` to ``g_last`` and sigma the factor ``get_prediction_xt_last`` puts on its noise -- the square root of the DDPM
    posterior variance, times ``ddim_eta`` under DDIM; z = 0 for a sample with sigma == 0 (g_last == 1)"""
    g, g_last = _b(g), _b(g_last)
    sigma = ((1 - g / g_last) * (1 - g_last) / (1 - g)).sqrt()
    if ddim_eta is not None:
        sigma = ddim_eta * sigma
    on = sigma > 0
    return torch.where(on, (x_s - mu) / torch.where(on, sigma, torch.ones_like(sigma)), torch.zeros_like(x_s))


def _check_step_noise(step_noise, solver, ddim_eta, resample):
    """what a call with ``step_noise=`` cannot have"""
    if step_noise is None:
        return
    if solver is not None:
        raise ValueError("step_noise= with solver=%r: the maps are the noise of the ancestral step (solver=None) they were "
                         "extracted for" % (solver,))
    if ddim_eta is not None and ddim_eta <= 0:
        raise ValueError("step_noise= with ddim_eta=%r: a deterministic step adds no noise, the maps would be ignored" % (ddim_eta,))
    if resample > 1:
        raise ValueError("step_noise= with resample=%d: there is one map per step, and a repeated step would add it twice" % resample)
    if not isinstance(step_noise, (list, tuple)):
        raise ValueError("step_noise must be the list of maps Sampler.noise_maps returned (got %s)" % type(step_noise).__name__)


def known_pyramid(known, mask, ratios):
    """One top-scale image and mask -> hi->lo lists for the scales ``ratios`` (top side / side of the scale; ratios[0] == 1).
    Images are average-pooled.  A lower-scale pixel is known only where EVERY pixel of its block is (mask == 1 there),
    stored as 0 / 1 floats; the top scale keeps the mask it was given, fractions included."""
    hip = known.is_cuda
    pool = (lambda x, r: ops.avgpool(x.float().contiguous(), r)) if hip else F.avg_pool2d
    ks, ms = [known], [mask]
    full = (mask == 1).to(known.dtype)
    for r in ratios[1:]:
        ks.append(pool(known, r))
        # the block mean of a 0 / 1 image is 1 only where all r * r are 1: the next value below is 1 - 1 / r^2
        ms.append((pool(full, r) > 1 - 0.5 / (r * r)).to(known.dtype))
    return ks, ms


class KnownRegion:
    """The known images of one ``sample()`` call: per scale (hi -> lo) an image [B, C, H, W] in output units ([-1, 1]), a mask
    [B, 1, H, W] in [0, 1] and 1 / image_scale of that scale, or None where the scale is free; plus the source of the
    known-region noise.  GPU tensors: one ``ops.DeviceRng(seed)`` of its own, drawn in the kernels on stream 1 and advanced
    by ``numel`` after every launch -- it never touches the ancestral-noise generator or torch's global one.  CPU tensors:
    ``noise_fn(x)`` if given (called once per blend / jump, in launch order), else a private ``torch.Generator`` seeded
    with ``seed``.  Within one iteration: blends hi -> lo, then jumps hi -> lo."""

    def __init__(self, images, masks, inv_scales, seed=0, noise_fn=None):
        self.images, self.masks, self.inv_scales = images, masks, inv_scales
        self.noise_fn = noise_fn
        first = next(k for k in images if k is not None)
        self.hip = first.is_cuda
        if self.hip:
            self.rng = ops.DeviceRng(seed, first.device)
        elif noise_fn is None:
            gen = torch.Generator().manual_seed(int(seed) & (2**63 - 1))
            self.noise_fn = lambda x: torch.randn(x.shape, generator=gen, dtype=x.dtype)

    @staticmethod
    def build(x_shapes, device, dtype, known_images, known_mask, ratios, image_scales, seed=0, noise_fn=None):
        """Normalise what ``sample()`` was given.  ``known_images`` / ``known_mask``: one top-scale tensor each (the lower
        scales come from ``known_pyramid``), or hi -> lo lists with None where a scale is free (a None mask beside a given
        image means all ones)."""
        n = len(x_shapes)
        if isinstance(known_images, (list, tuple)):
            if len(known_images) != n:
                raise ValueError("known_images has %d entries, the model %d scales" % (len(known_images), n))
            if known_mask is not None and (not isinstance(known_mask, (list, tuple)) or len(known_mask) != n):
                raise ValueError("known_mask must be a list of %d entries (or None) beside a list of known_images" % n)
            ks, ms = list(known_images), list(known_mask) if known_mask is not None else [None] * n
            if all(k is None for k in ks):
                raise ValueError("known_images holds no image")
        else:
            if isinstance(known_mask, (list, tuple)):
                raise ValueError("known_mask is a list but known_images one tensor")
            k = known_images.to(device=device, dtype=dtype)
            m = torch.ones(k.shape[0], 1, *k.shape[2:], device=device, dtype=dtype) if known_mask is None else known_mask
            KnownRegion._check(k, m, x_shapes[0])
            ks, ms = known_pyramid(k, m.to(device=device, dtype=dtype), ratios)
        for i, (k, shape) in enumerate(zip(ks, x_shapes)):
            if k is None:
                if ms[i] is not None:
                    raise ValueError("known_mask[%d] without known_images[%d]" % (i, i))
                continue
            k = k.to(device=device, dtype=dtype).contiguous()
            m = ms[i]
            m = torch.ones(k.shape[0], 1, *k.shape[2:], device=device, dtype=dtype) if m is None else m
            KnownRegion._check(k, m, shape)
            ks[i], ms[i] = k, m.to(device=device, dtype=dtype).contiguous()
        inv = [1.0 / s if s else 1.0 for s in image_scales]
        return KnownRegion(ks, ms, inv, seed, noise_fn)

    @staticmethod
    def _check(k, m, shape):
        shape = tuple(shape)
        if tuple(k.shape) != shape:
            raise ValueError("known image %s vs the sampled image %s" % (tuple(k.shape), shape))
        if tuple(m.shape) != (shape[0], 1, shape[2], shape[3]):
            raise ValueError("known mask must be %s (got %s)" % ((shape[0], 1, shape[2], shape[3]), tuple(m.shape)))
        if (shape[2] * shape[3]) % 4:
            raise ValueError("known-region sampling needs H * W to be a multiple of 4 (got %d x %d)" % (shape[2], shape[3]))

    def blend(self, xs, gs):
        """every scale's x_s (at its own gamma ``gs[i]``) with its known image; -> the list (GPU tensors: in place)"""
        out = list(xs)
        for i, (x, g) in enumerate(zip(xs, gs)):
            k, m, inv = self.images[i], self.masks[i], self.inv_scales[i]
            if k is None:
                continue
            if self.hip:
                out[i] = ops.sampler_known_blend(x, k, m, g, inv_scale=inv, rng=self.rng, rng_stream=1)
                self.rng.advance(x.numel())
            else:
                out[i] = known_blend(x, k, m, g, inv, self.noise_fn(x))
        return out

    def jump(self, xs, g_t, g_s):
        """every scale back from its level g_s[i] to g_t[i]"""
        out = []
        for x, gt, gs in zip(xs, g_t, g_s):
            if self.hip:
                out.append(ops.sampler_jump(x, gt, gs, rng=self.rng, rng_stream=1, out=x))
                self.rng.advance(x.numel())
            else:
                out.append(jump(x, gt, gs, self.noise_fn(x)))
        return out


class LossGuide:
    """Loss-guided sampling (diffusion posterior sampling, Chung et al. 2023; "universal" / classifier guidance):
    ``sample(..., guide=LossGuide(fn, scale, normalize))`` pulls every step towards a small ``fn``.

    ``fn(x0) -> loss [B]``: any differentiable torch function of the top-scale clean-image estimate ``x0`` in image units
    (what ``_postprocess`` returns for it: fp32 ``[B, C, H, W]``), one NON-NEGATIVE scalar per sample.  Per step, with
    v = d sum_b loss_b / d x0 and x0 = threshold(scale (a x_t + b pred(x_t))) (``get_x0_eps_from_pred``):

        grad = a (v . m) k + J^T [b (v . m) k]         (J = d pred / d x_t: one autograd pass through the denoiser)
        x_s <- x_s - zeta_b grad,   zeta_b = scale / max(sqrt(loss_b), 1e-8) if normalize (the DPS step) else scale

    The threshold is differentiated as a CLAMP: m = 0 where x0 was clipped, k = image scale (/ the threshold for the
    dynamic thresholds); the per-sample quantile of a dynamic threshold is treated as a constant.  Lower scales of a nested
    model receive their J^T part only.  Under classifier-free guidance the seed goes to both halves of the doubled batch
    with weights s and 1 - s.  A sample whose loss is exactly 0 is left alone.  The step itself (and the history of
    ``solver="dpmpp_2m"``) is unguided: the correction is applied to x_s, before the known-region blend of
    ``known_images=``.  Model parameters are frozen for the duration of the call, so the backward pass launches input
    gradients only.  The MXFP8 layers are inference-only and raise; ``GraphedSampler`` refuses ``guide=``."""

    SQRT_FLOOR = 1e-8

    def __init__(self, fn, scale=1.0, normalize=True):
        if not callable(fn):
            raise TypeError("LossGuide: fn must be callable, x0 [B, C, H, W] -> loss [B] (got %r)" % (type(fn).__name__,))
        self.fn, self.scale, self.normalize = fn, float(scale), bool(normalize)

    def loss_and_grad(self, x0):
        """-> (loss [B] detached, d sum(loss) / d x0)"""
        x = x0.detach().requires_grad_(True)
        with torch.enable_grad():
            loss = self.fn(x)
            if not torch.is_tensor(loss) or tuple(loss.shape) != (x.shape[0],):
                raise ValueError("LossGuide: fn must return one loss per sample, shape (%d,) (got %s)"
                                 % (x.shape[0], tuple(loss.shape) if torch.is_tensor(loss) else type(loss).__name__))
            if not loss.requires_grad:
                raise ValueError("LossGuide: the loss does not depend on x0 (nothing to differentiate)")
            v, = torch.autograd.grad(loss.sum(), x)
        return loss.detach(), v

    def zeta(self, loss):
        """per-sample step size [B], on the loss's device: no host synchronisation"""
        z = self.scale / loss.sqrt().clamp(min=self.SQRT_FLOOR) if self.normalize else torch.full_like(loss, self.scale)
        return torch.where(loss > 0, z, torch.zeros_like(z))


class MapGuide:
    """Attention-map guidance: ``sample(..., map_guide=MapGuide(fn, scale, layers, interval, iterations))`` moves x_t down the
    gradient of a loss on the text cross-attention maps before the reverse step (Attend-and-Excite, Chefer et al. 2023;
    layout guidance and self-guidance are the same mechanism with another ``fn``).

    ``fn(maps) -> loss [B]``: any differentiable torch function, one NON-NEGATIVE scalar per image, of what
    ``attn_maps.GradRows.maps()`` returns for the B images: {(h, w): fp32 [B, S, h, w]}, the text term's probabilities, mean
    over the heads and over the recording layers of that resolution (``AttendExcite`` is a ready-made one).
    ``scale``: the step size, a float or a callable (time_step, num_diffusion_steps) -> float.
    ``layers``: the vocabulary of ``pag.select``; the layers with text keys among them record.
    ``interval = (lo, hi)`` in fractions of ``num_diffusion_steps``, the convention of ``AttnMaps.interval``: a step is
    guided where lo <= t / T <= hi for the time t it starts from; None: every step.
    ``iterations``: gradient sub-steps per guided step -- a fixed count, nothing is read back from the device.

    Per guided step, ``iterations`` times, before the step's own denoiser call: every scale's x_t becomes a leaf; the model
    runs once with grad enabled and frozen parameters on the B CONDITIONAL rows only (the conditional half of
    ``lm_outputs`` / ``lm_mask``), at the time the step uses, with only the recorder switch on (``ops.attn_cross_probs``,
    whose backward is mdm_attn_cross_maps_bwd: no PAG, regions or FreeU switch, their kernels have no backward);
    loss = fn(maps); one ``autograd.grad`` of loss.sum() to the leaves; x_t <- x_t - scale grad for every scale that got a
    gradient (GPU tensors: ``ops.guide_apply``).  A sample whose loss is exactly 0 keeps its bits.  Then the step runs
    unchanged, with all its options, on the moved x_t; what the model returned in the guidance pass is discarded, and the
    pass does not record into ``attn_maps=``.  The MXFP8 layers are inference-only and raise; ``GraphedSampler`` refuses."""

    def __init__(self, fn, scale, layers="all", interval=(0.5, 1.0), iterations=1):
        if not callable(fn):
            raise TypeError("MapGuide: fn must be callable, {(h, w): maps [B, S, h, w]} -> loss [B] (got %r)" % (type(fn).__name__,))
        if not callable(scale):
            try:
                scale = float(scale)
            except (TypeError, ValueError):
                raise TypeError("MapGuide: scale = %r (wanted a float, or a callable (time_step, num_diffusion_steps) -> float)"
                                % (scale,))
            if not math.isfinite(scale):
                raise ValueError("MapGuide: scale = %r (wanted a finite step size)" % (scale,))
        if interval is not None:
            try:
                lo, hi = interval
                interval = (float(lo), float(hi))
            except (TypeError, ValueError):
                raise ValueError("MapGuide: interval = %r (wanted (lo, hi) in fractions of the schedule, or None)" % (interval,))
            if not (math.isfinite(interval[0]) and math.isfinite(interval[1]) and interval[0] <= interval[1]):
                raise ValueError("MapGuide: interval = %r (wanted finite lo <= hi)" % (interval,))
        if not (callable(layers) or isinstance(layers, (str, list, tuple, set, frozenset))):
            raise ValueError("MapGuide: layers = %r (wanted a named set, a list of module names, or a predicate)" % (layers,))
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError("MapGuide: iterations = %r (wanted an int >= 1: a fixed count of gradient sub-steps)" % (iterations,))
        self.fn, self.scale, self.layers, self.interval, self.iterations = fn, scale, layers, interval, iterations

    def on(self, time_step, num_diffusion_steps):
        """is the step that starts from ``time_step`` guided?"""
        if self.interval is None:
            return True
        return self.interval[0] <= float(time_step) / float(num_diffusion_steps) <= self.interval[1]

    def scale_at(self, time_step, num_diffusion_steps):
        """the step size of the step that starts from ``time_step``, a host float"""
        return float(self.scale(int(time_step), int(num_diffusion_steps))) if callable(self.scale) else self.scale

    def loss(self, maps, B):
        """fn(maps), checked -> loss [B], attached to the tape"""
        loss = self.fn(maps)
        if not torch.is_tensor(loss) or tuple(loss.shape) != (B,):
            raise ValueError("MapGuide: fn must return one loss per image, shape (%d,) (got %s)"
                             % (B, tuple(loss.shape) if torch.is_tensor(loss) else type(loss).__name__))
        if not loss.requires_grad:
            raise ValueError("MapGuide: the loss does not depend on the maps (nothing to differentiate)")
        return loss


class AttendExcite:
    """The loss of Attend-and-Excite (Chefer et al., SIGGRAPH 2023) as a ``MapGuide`` function, in plain torch: every
    subject token must attend strongly somewhere,

        loss_b = max over s in tokens_b of (1 - max over (y, x) of M~[b, s, y, x]).

    ``tokens``: one list of token indices for every image, or one list per image.  ``resolution = (h, w)``: which maps,
    M = maps[resolution]; None takes the single recorded resolution (several: ValueError).  ``exclude``: token indices
    (start / end / padding markers) removed from M, the rest renormalised per pixel to sum 1.  ``smooth``: M~ = M under a
    3 x 3 Gaussian of sigma 0.5 with reflect padding, as in the paper; else M~ = M."""

    def __init__(self, tokens, resolution=None, smooth=True, exclude=()):
        tokens = list(tokens)
        if not tokens:
            raise ValueError("AttendExcite: no tokens")
        per_row = all(isinstance(t, (list, tuple)) for t in tokens)
        rows = [list(t) for t in tokens] if per_row else [tokens]
        for r in rows:
            if not r or any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in r):
                raise ValueError("AttendExcite: tokens = %r (wanted a non-empty list of token indices >= 0, or one per image)"
                                 % (tokens,))
        self.tokens, self.per_row = rows, per_row
        self.resolution = None if resolution is None else (int(resolution[0]), int(resolution[1]))
        self.smooth = bool(smooth)
        self.exclude = tuple(int(t) for t in exclude)
        if any(t in self.exclude for r in rows for t in r):
            raise ValueError("AttendExcite: a subject token is among the excluded ones (%r)" % (self.exclude,))

    @staticmethod
    def kernel(dtype, device):
        """the 3 x 3 Gaussian of sigma 0.5, normalised"""
        g = torch.exp(-torch.arange(-1, 2, dtype=torch.float64) ** 2 / (2 * 0.5 ** 2))
        k = torch.outer(g, g)
        return (k / k.sum()).to(dtype=dtype, device=device)

    def __call__(self, maps):
        if self.resolution is None:
            if len(maps) != 1:
                raise ValueError("AttendExcite: maps of the resolutions %s: say which with resolution=" % (sorted(maps),))
            M = next(iter(maps.values()))
        else:
            if self.resolution not in maps:
                raise ValueError("AttendExcite: no maps of resolution %s (recorded: %s)" % (self.resolution, sorted(maps)))
            M = maps[self.resolution]
        B, S, h, w = M.shape
        if self.per_row and len(self.tokens) != B:
            raise ValueError("AttendExcite: token lists for %d images, maps of %d" % (len(self.tokens), B))
        if max(max(r) for r in self.tokens) >= S:
            raise ValueError("AttendExcite: token %d of %d" % (max(max(r) for r in self.tokens), S))
        if self.exclude:
            keep = torch.ones(S, dtype=torch.bool, device=M.device)
            keep[list(self.exclude)] = False
            M = M * keep.to(M.dtype)[None, :, None, None]
            M = M / M.sum(dim=1, keepdim=True).clamp(min=1e-20)
        if self.smooth:
            k = self.kernel(M.dtype, M.device)
            M = F.conv2d(F.pad(M.reshape(B * S, 1, h, w), (1, 1, 1, 1), mode="reflect" if min(h, w) > 1 else "replicate"),
                         k[None, None]).reshape(B, S, h, w)
        peak = M.amax(dim=(2, 3))                                   # [B, S]
        rows = self.tokens if self.per_row else self.tokens * B
        return torch.stack([(1 - peak[b, r]).max() for b, r in enumerate(rows)])


@dataclass(frozen=True)
class SampleOptions:
    """The sampling options beyond the reference, as the keywords of ``Sampler.sample``, ``get_xt_minus_1``,
    ``GraphedSampler.sample``, ``Diffusion.sample`` and ``Diffusion.partial_diffusion``.  Every default leaves every step
    as it is; each option changes the denoiser call or the prediction handed to the update, never the update, so all of
    them compose with ``ddim_eta``, ``solver=``, ``known_images=`` / ``resample``, a late start, LoRA and MXFP8.

    ``guide``: a ``LossGuide`` -- loss-guided sampling; per step: the update, then the guide's correction, then the
    known-region blend.  The model runs on leaf x_t with grad enabled, the step itself unchanged under no_grad; the loss
    sees the top scale.  Eager samplers only.
    ``pag_scale = s > 0``: perturbed-attention guidance (Ahn et al. 2024).  Every denoiser call carries B more rows,
    [uncond | cond | perturbed] (``lm_outputs`` stays [uncond | cond], or [cond] at ``guidance_scale == 1``), in which the
    ``SelfAttention`` layers that ``pag_layers`` selects (``pag.select``: "mid", "deepest", "all", names, a predicate)
    attend to themselves only, and the step gets  p_u + w (p_c - p_u) + s (p_c - p_hat)  from one combine per scale (GPU
    tensors: ``ops.pag_combine``, CPU tensors: ``pag_combine``).
    ``regions = rp`` (a ``mdm_hip.RegionPrompts`` over the conditional rows of ``lm_outputs``): in the ``SelfAttention``
    layers with text keys that ``region_layers`` selects (the vocabulary of ``pag.select``; default every one) the text
    logits get rp's bias -- log(token weight) + log(region coverage of the query position); 0 in the unconditional rows;
    the perturbed block of ``pag_scale`` repeats the conditional rows'.
    ``freeu = FreeU(b=(b1, b2), s=(s1, s2), structure=False, levels="deepest2")``: FreeU (Si et al. 2024) -- in the up
    blocks that ``freeu.select`` names, the skip concat multiplies the first half of the backbone channels by b (v2,
    ``structure=True``: by 1 + (b - 1) x the min-max normalised channel mean) and the 2 x 2 lowest spatial frequencies of
    the skip by s, for every row of the model batch alike.  No extra denoiser call.
    ``cfg = CFG(eta=1, norm_threshold=0, momentum=0, rescale=0, interval=None)`` with ``guidance_scale != 1``: the
    classifier-free guidance combine  p_u + w (p_c - p_u)  is replaced by the projected / rescaled one of
    ``mdm_hip/guidance.py`` -- adaptive projected guidance (Sadat et al. 2025: the part of the update parallel to the
    conditional x0 scaled by ``eta``, its RMS in image units capped at ``norm_threshold`` -- the paper's radius over
    sqrt(C H W), so one value serves every scale --, a ``momentum`` across steps), the std rescale (Lin et al. 2024,
    ``rescale`` = phi) and the guidance interval (Kynkaanniemi et al. 2024: outside ``interval``, in fractions of
    ``num_diffusion_steps``, the step takes the conditional prediction).  One combine per scale in front of the unchanged
    step (GPU tensors: ``ops.cfg_combine``, two launches; CPU tensors: ``guidance.cfg_combine``), which then gets no
    unconditional prediction and guidance 1.  The momentum history, one buffer per scale, starts empty with every
    trajectory, wherever it starts, and every denoiser call updates it, the repeats of ``resample`` included.  Nothing
    changes at ``guidance_scale == 1``.
    ``tiles = Tiles(window, stride=None, blend="uniform")`` (``mdm_hip/tiling.py``): tiled sampling (MultiDiffusion, Bar-Tal
    et al. 2023) of a canvas larger than the window the model was trained at -- x_T is the canvas (``Diffusion.sample(...,
    image_side=(H, W))``).  Every denoiser call runs on the overlapping windows of x_t, T per image, B T rows per block
    [uncond | cond | perturbed] with the conditioning and the times repeated per window (once per ``sample()`` call), and the
    windows' predictions are averaged where they overlap -- uniformly, or under a tent (``blend="ramp"``) -- into
    whole-canvas predictions: one gather and one merge per scale (GPU tensors: ``ops.tiles_gather`` / ``ops.tiles_merge``,
    CPU tensors: ``tiling.gather`` / ``tiling.merge``).  Everything behind the denoiser call -- both guidance combines, the
    step, the dynamic-threshold quantile, ``known_images``, ``solver=`` -- sees whole canvases; FreeU and the perturbed rows
    act per window.  A nested model takes window, stride and canvas as multiples of its largest ratio.  One window equal
    to the canvas changes no bit.  All T windows go through ONE denoiser call: memory grows with the canvas.

    ``attn_maps = maps`` (a ``mdm_hip.AttnMaps`` over the conditional rows and the S tokens of ``lm_outputs``): the
    ``SelfAttention`` layers with text keys that ``maps.layers`` selects add the probabilities of their text cross-attention
    -- the biased ones under ``regions`` --, mean over heads, into ``maps`` (``ops.attn_cross_maps``, one launch per layer
    and recorded step; CPU tensors: ``attn_maps.cross_maps``) for the conditional block of the model batch, in the steps
    of ``maps.interval``.  The layers' outputs are computed as before: the images do not change by a bit.  Reads detached
    values, so it composes with ``guide`` too.
    ``map_guide = MapGuide(fn, scale, layers, interval, iterations)``: attention-map guidance (``MapGuide``; ``AttendExcite``
    is the ready-made ``fn``) -- in the steps of its interval, x_t is first moved down the gradient of a loss on the text
    cross-attention maps of the conditional rows (one more forward + backward over B rows per iteration, with only the
    recorder switch on), then the step runs unchanged with every other option on the moved x_t.  Eager samplers only.
    ``control = ctl`` (a ``mdm_hip.AttnControl`` over the conditional rows and the S tokens of ``lm_outputs``): prompt-to-prompt
    attention control (Hertz et al. 2022; ``mdm_hip/attn_control.py``) -- the conditional block is [sources | edits], and in
    the layers ``ctl.cross_layers`` / ``ctl.self_layers`` select an edited row computes with its source row's text
    cross-attention probabilities (through ``mapper`` / ``keep`` / ``scale``) and, early in the trajectory, its
    self-attention map (``ops.attention_controlled``).  Those layers take the split path for the edited rows in EVERY step;
    the two intervals only set the device gates of the step, so outside them an edited row agrees with the uncontrolled
    sampler to rounding, not bit for bit.  Sources, the unconditional and the perturbed rows take the ordinary launches.
    Composes with ``cfg``, ``pag_scale``, ``freeu``, ``attn_maps`` (the recorder still reads each row's OWN q and k_c: an
    edited row's recorded map is its own, not the one it computed with), every solver, ``known_images``, a late start and
    ``step_noise``.  A control whose rows are all sources launches nothing new.

    The model switches (perturbed rows, region bias, FreeU, the map recorder) are held around each step's denoiser call only
    (``switches``), never across a ``yield``, and a switch that is off is not even resolved.  What excludes what
    (``check``: NotImplementedError): ``guide`` with each of the other four, because their kernels have no backward or, for
    ``cfg``, no Jacobian; ``pag_scale`` with ``cfg``; ``guide`` with ``tiles`` (no backward); ``regions`` with ``tiles``
    (the bias is laid out over the whole canvas); and ``attn_maps`` with ``tiles`` (a window's queries are not the
    canvas's); ``map_guide`` with ``guide`` (two corrections of one step), with ``tiles`` and with an SA solver; ``control``
    with ``guide`` and ``map_guide`` (no backward), with ``regions`` and with ``tiles``.  Everything else composes.

    Not a field here: ``step_noise=maps`` (``Sampler.noise_maps`` -> ``sample``) replaces the noise the ancestral update adds,
    so it is a plain keyword of ``sample`` beside ``solver_noise_fn``; every option above composes with it, because the maps
    are added behind whatever prediction the options make.  ``Sampler.invert`` and ``Sampler.noise_maps`` themselves take the
    options that act on the denoiser call only (``Sampler.INVERSION_REFUSED``)."""

    guide: object = None
    pag_scale: float = 0.0
    pag_layers: object = "mid"
    regions: object = None
    region_layers: object = "all"
    freeu: object = None
    cfg: object = None
    tiles: object = None
    attn_maps: object = None
    map_guide: object = None
    control: object = None

    REFUSED = {
        ("control", "guide"): "control= together with guide=: the controlled rows' cross kernel (mdm_attn_cross_bias) has no "
                              "backward, so the guide's input gradient cannot pass it",
        ("control", "map_guide"): "control= together with map_guide=: the map loss is differentiated through each row's own "
                                  "attention, and an edited row's output depends on its source's maps, which have no backward",
        ("control", "regions"): "control= together with regions=: both act on the text cross-attention of the conditional "
                                "rows, and mixing biased probabilities over the token axis is not implemented",
        ("control", "tiles"): "control= together with tiles=: every image is a block of windows, and pairing the windows of an "
                              "edit with those of its source is not implemented",
        ("guide", "pag"): "guide= together with pag_scale != 0: the perturbed rows' attention kernel (mdm_attn_cross_addv) "
                          "has no backward, so the guide's input gradient cannot pass it",
        ("guide", "regions"): "guide= together with regions=: the biased cross-attention kernel (mdm_attn_cross_bias) has "
                              "no backward, so the guide's input gradient cannot pass it",
        ("guide", "freeu"): "guide= together with freeu=: the fused concat (mdm_freeu_apply) has no backward, so the "
                            "guide's input gradient cannot pass it",
        ("guide", "cfg"): "guide= together with cfg=: the guide seeds the two halves of the doubled batch with the weights "
                          "of the plain combine (w and 1 - w); the projected / rescaled combine depends on per-sample "
                          "statistics of both predictions, and its Jacobian is not implemented",
        ("pag", "cfg"): "pag_scale != 0 together with cfg=: mdm_pag_combine adds the perturbed-attention term to the plain "
                        "combine; projecting, capping and rescaling an update of three predictions is not implemented",
        ("guide", "tiles"): "guide= together with tiles=: the window kernels (mdm_tiles_gather, mdm_tiles_merge) have no "
                            "backward, so the guide's input gradient cannot pass them",
        ("regions", "tiles"): "regions= together with tiles=: the bias is laid out per query position of the whole canvas, "
                              "and cropping it per window is not implemented",
        ("attn_maps", "tiles"): "attn_maps= together with tiles=: a window's queries are not the canvas's, and merging the "
                                "maps of the windows is not implemented",
        ("map_guide", "guide"): "map_guide= together with guide=: two corrections of one step -- the map loss moves x_t before "
                                "the step, the guide's loss moves x_s after it -- have not been tested together",
        ("map_guide", "tiles"): "map_guide= together with tiles=: a window's queries are not the canvas's, and merging the "
                                "maps of the windows is not implemented",
    }

    @classmethod
    def pop(cls, keywords):
        """takes the options' names out of a dict of keywords -> the object (unchecked)"""
        return cls(**{f.name: keywords.pop(f.name) for f in fields(cls) if f.name in keywords})

    def check(self):
        """every type and range check, and the pairs of ``REFUSED``; several things wrong: guide, pag, regions, freeu, cfg,
        tiles"""
        on = dict(guide=self.guide is not None, pag=self.pag_scale != 0, regions=self.regions is not None,
                  freeu=self.freeu is not None, cfg=self.cfg is not None, tiles=self.tiles is not None,
                  attn_maps=self.attn_maps is not None, map_guide=self.map_guide is not None,
                  control=self.control is not None)

        def refuse(a, b):
            if on[a] and on[b]:
                raise NotImplementedError(self.REFUSED[a, b])

        if on["guide"] and not isinstance(self.guide, LossGuide):
            raise TypeError("guide must be an mdm_hip.LossGuide (got %r)" % (type(self.guide).__name__,))
        if self.pag_scale < 0:
            raise ValueError("pag_scale must be >= 0 (got %r); 0 = no perturbed-attention guidance" % (self.pag_scale,))
        refuse("guide", "pag")
        refuse("guide", "regions")
        if on["regions"] and not callable(getattr(self.regions, "rows_for", None)):
            raise ValueError("regions = %r (wanted a mdm_hip.RegionPrompts)" % (self.regions,))
        refuse("guide", "freeu")
        if on["freeu"] and not isinstance(self.freeu, _freeu.FreeU):
            raise ValueError("freeu = %r (wanted a mdm_hip.FreeU)" % (self.freeu,))
        if on["cfg"]:
            if not isinstance(self.cfg, _guidance.CFG):
                raise ValueError("cfg = %r (wanted a mdm_hip.CFG)" % (self.cfg,))
            self.cfg.validate()
        refuse("guide", "cfg")
        refuse("pag", "cfg")
        if on["tiles"] and not isinstance(self.tiles, _tiling.Tiles):
            raise ValueError("tiles = %r (wanted a mdm_hip.Tiles)" % (self.tiles,))
        refuse("guide", "tiles")
        refuse("regions", "tiles")
        if on["attn_maps"] and not isinstance(self.attn_maps, _attn_maps.AttnMaps):
            raise ValueError("attn_maps = %r (wanted a mdm_hip.AttnMaps)" % (self.attn_maps,))
        refuse("attn_maps", "tiles")
        if on["map_guide"] and not isinstance(self.map_guide, MapGuide):
            raise TypeError("map_guide must be an mdm_hip.MapGuide (got %r)" % (type(self.map_guide).__name__,))
        refuse("map_guide", "guide")
        refuse("map_guide", "tiles")
        if on["control"] and not isinstance(self.control, _attn_control.AttnControl):
            raise ValueError("control = %r (wanted a mdm_hip.AttnControl)" % (self.control,))
        refuse("control", "guide")
        refuse("control", "map_guide")
        refuse("control", "regions")
        refuse("control", "tiles")
        return self

    def blocks(self, guidance_scale):
        """-> (unconditional block present, perturbed block present) of the model batch [uncond | cond | perturbed]; the
        conditional block always is, so the rows are 1 + their sum times the images"""
        return guidance_scale != 1, self.pag_scale != 0

    def cfg_at(self, guidance_scale):
        """the ``CFG`` that acts at this guidance scale: None at 1, where there is nothing to combine"""
        return self.cfg if guidance_scale != 1 else None

    def switches(self, model, guidance_scale, B, device=None, names=None, bias=None, rec=None, step=None, ctrl=None):
        """-> the context manager of one denoiser call over ``B`` images: the model switches that are on -- perturbed rows,
        region bias, FreeU, the map recorder -- as ONE ``unet.switched``.  They touch disjoint attributes, so there is no
        order among them to get right.  A captured graph body passes the names it resolved (``layer_names``), its
        ``StaticBias`` and its ``attn_maps.StaticRows`` (``rec``); the eager samplers pass none of them, and ``step`` =
        (the time the step starts from, ``num_diffusion_steps``), by which ``attn_maps.interval`` decides whether this call
        records (None: it does) and ``control``'s intervals set the gates of this call (None: both on).  ``ctrl``: a graph
        body's static ``attn_control.BatchCtrl``, whose gates the body has set."""
        controlled = self.control is not None and self.control.R > 0   # (all rows sources: nothing to control)
        if self.pag_scale == 0 and self.regions is None and self.freeu is None and self.attn_maps is None and not controlled:
            return _UNCHANGED
        vision_model = getattr(model, "vision_model", model)
        pag_layers, region_layers = (self.pag_layers, self.region_layers) if names is None else names[:2]
        on = []
        if self.pag_scale != 0:
            on.append(pag.perturbed(vision_model, pag_layers, rows=B))
        if self.regions is not None:
            if bias is None:
                if self.regions.rows != B:
                    raise ValueError("regions over %d rows for a batch of %d images" % (self.regions.rows, B))
                bias = self.regions.rows_for(*self.blocks(guidance_scale), device)
            on.append(_regions.applied(vision_model, bias, region_layers))
        if self.freeu is not None:
            on.append(_freeu.applied(vision_model, self.freeu))
        if self.attn_maps is not None:
            if rec is None and (step is None or self.attn_maps.on(*step)):
                if self.attn_maps.rows != B:
                    raise ValueError("attn_maps over %d rows for a batch of %d images" % (self.attn_maps.rows, B))
                rec = self.attn_maps.rows_for(*self.blocks(guidance_scale), device)
            if rec is not None:
                on.append(_attn_maps.applied(vision_model, rec, self.attn_maps.layers if names is None else names[2]))
        if controlled:
            if ctrl is None:
                if self.control.rows != B:
                    raise ValueError("control over %d rows for a batch of %d images" % (self.control.rows, B))
                ctrl = self.control.rows_for(*self.blocks(guidance_scale), device)
                ctrl.set_gates(*((1.0, 1.0) if step is None else self.control.gates(*step)))
            on.append(_attn_control.applied(vision_model, ctrl, self.control, None if names is None else names[-1]))
        if not on:   # a recorder outside its interval: this call launches what it always did
            return _UNCHANGED
        return switched(s for one in on for s in one.settings)

    def layer_names(self, vision_model):
        """-> (perturbed layers, biased layers) as tuples of module names: hashable; () where the option is off; with
        ``attn_maps``, and only then, a third: the recording layers; with a ``control`` that has edited rows, and only then,
        a last one: its (cross layers, self layers)"""
        names = (pag.layer_names(vision_model, self.pag_layers) if self.pag_scale != 0 else (),
                 _regions.layer_names(vision_model, self.region_layers) if self.regions is not None else ())
        if self.attn_maps is not None:
            names += (_attn_maps.layer_names(vision_model, self.attn_maps.layers),)
        if self.control is not None and self.control.R > 0:
            names += (self.control.layer_sets(vision_model),)
        return names

    def graph_key(self, vision_model, guidance_scale, names):
        """the options' part of a ``GraphedSampler`` key, ``names`` being ``layer_names`` of the model: one component per
        option that is on -- calls that differ in nothing else share a captured graph"""
        key = ()
        if self.pag_scale != 0:
            key += (("pag", float(self.pag_scale), names[0]),)
        if self.regions is not None:
            key += (("regions", self.regions.S, self.regions.ld, names[1]),)
        if self.freeu is not None:
            key += (_freeu.graph_key(vision_model, self.freeu),)
        if self.cfg_at(guidance_scale) is not None:
            key += (self.cfg.key(),)
        if self.tiles is not None:
            key += (self.tiles.graph_key(),)
        if self.attn_maps is not None:   # (the interval is a table of gates that every call rewrites: no part of the key)
            key += (("attn_maps", self.attn_maps.S, self.attn_maps.ld, names[2]),)
        if self.control is not None and self.control.R > 0:
            # (mapper, keep, scale and the intervals are static buffers and gate tables that every call rewrites)
            key += (("control", self.control.S, self.control.ld, self.control.source, self.control.self_max_queries, names[-1]),)
        return key


_UNCHANGED = contextlib.nullcontext()   # no switch on; the caller's grad mode left alone (stateless: one serves every use)


class _frozen_parameters:
    """requires_grad of every parameter off inside, restored after: a guided step needs input gradients only"""

    def __init__(self, model):
        self.params = [p for p in model.parameters()] if isinstance(model, nn.Module) else []

    def __enter__(self):
        self.saved = [p.requires_grad for p in self.params]
        for p in self.params:
            p.requires_grad_(False)
        return self

    def __exit__(self, *a):
        for p, r in zip(self.params, self.saved):
            p.requires_grad_(r)


class Sampler(nn.Module):
    def __init__(self, sampler_config: SamplerConfig):
        super().__init__()
        self._config = cfg = sampler_config
        self.n_steps = cfg.num_diffusion_steps
        if cfg.schedule_type == ScheduleType.COSINE:
            g = gammas_cosine(self.n_steps)
        elif cfg.schedule_type == ScheduleType.DDPM:
            g = gammas_linear_beta(self.n_steps, cfg.beta_start, cfg.beta_end)
        elif cfg.schedule_type == ScheduleType.DEEPFLOYD:
            g = gammas_squaredcos_cap_v2(self.n_steps)
        else:
            raise ValueError("unknown schedule")
        self.register_buffer("_gammas", torch.tensor(g).float())
        gammas = self.get_schedule_shifted(self._gammas.clone(), cfg.rescale_schedule)
        gt, gl = gammas[2:], gammas[1:-1]
        w = gl * (1 - gt) / (1 - gl) / gt - 1  # VDM weights (:223-228)
        self.register_buffer("gammas", gammas)
        self.register_buffer("vdm_loss_weights", torch.cat([w[:1], w[:1], w]))
        if cfg.loss_target_type is None:
            cfg.loss_target_type = cfg.prediction_type
        self.device_rng = None   # ops.DeviceRng: draw the sampling noise inside the step kernel (see use_device_rng)

    def use_device_rng(self, seed: int, device):
        """Draw the ancestral-sampling noise INSIDE the step kernel from the library's counter-based generator
        (replayable on the host, oracle/philox_ref.py) instead of ``torch.randn_like`` -- one launch less per scale."""
        self.device_rng = ops.DeviceRng(seed, device)
        return self

    # ---- schedule access -------------------------------------------------------------
    def read_gamma(self, time, image=None):
        return _b(self.gammas[time])

    def get_schedule_shifted(self, gammas, scale_factor=None):
        """SNR' = SNR / s^p (:255-264)."""
        if scale_factor is not None and scale_factor > 1:
            s = scale_factor ** self._config.schedule_shifted_power
            snr = gammas / (1 - gammas)
            gammas = 1 / (1 + s / snr)
        return gammas

    def get_image_rescaled(self, images, scale_factor=None):
        s = self._config.rescale_signal if scale_factor is None else scale_factor
        return images / s if s else images

    # ---- training-side helpers (:233-279, 347-390) --------------------------------------
    def get_eps_time(self, images, time=None, noise_fn=torch.randn_like):
        B = images.shape[0]
        if time is None:
            time = torch.randint(0, self.n_steps, (B,), device=images.device)
        else:  # scalar or per-sample tensor
            time = torch.as_tensor(time, device=images.device) * torch.ones(B, dtype=torch.long, device=images.device)
        return noise_fn(images), self.read_gamma(time + 1), self.read_gamma(time), self.vdm_loss_weights[time + 1], time

    def get_xt(self, images, eps, g):
        return g.sqrt() * images + (1 - g).sqrt() * eps

    def get_prediction_targets(self, images, eps, g, g_last, prediction_type=None):
        pt = prediction_type or self._config.loss_target_type
        if pt in (PredictionType.DDPM, PredictionType.DDIM):
            return eps
        if pt == PredictionType.V_PREDICTION:
            return g.sqrt() * eps - (1 - g).sqrt() * images
        raise ValueError("unsupported prediction type")

    def get_x0_eps_from_pred(self, x_t, pred, g, prediction_type=None, clip_fn=None, return_eps=True):
        pt = prediction_type or self._config.prediction_type
        if pt in (PredictionType.DDPM, PredictionType.DDIM):
            x0 = (x_t - pred * (1 - g).sqrt()) / g.sqrt()
        elif pt == PredictionType.V_PREDICTION:
            x0 = x_t * g.sqrt() - pred * (1 - g).sqrt()
        else:
            raise ValueError("unsupported prediction type")
        if clip_fn is not None:
            x0 = clip_fn(x0)
        if not return_eps:
            return x0
        return x0, (x_t - x0 * g.sqrt()) / (1 - g).sqrt()

    def get_pred_from_x0_xt(self, x_t, x0, g, prediction_type=None):
        pt = prediction_type or self._config.prediction_type
        if pt in (PredictionType.DDPM, PredictionType.DDIM):
            return (x_t - x0 * g.sqrt()) / (1 - g).sqrt()
        if pt == PredictionType.V_PREDICTION:
            return (g.sqrt() * x_t - x0) / (1 - g).sqrt()
        raise ValueError("unsupported prediction type")

    # ---- one reverse step (:281-345) -------------------------------------------------------
    def get_prediction_xt_last(self, x_t, pred, g, g_last, prediction_type=None, clip_fn=None, need_noise=False,
                               ddim_eta=None, input_noise=None, image_scale=None, return_eps=True, pred_uncond=None,
                               guidance_scale=1, thr_out=None, rng=None, noise_gate=None):
        """``thr_out``: a list of the caller's; the per-sample dynamic threshold of this step (None for the other threshold
        functions) is appended to it -- what a ``LossGuide`` needs of the step besides x0.  GPU tensors only: ``rng`` (an
        ``ops.DeviceRng`` instead of ``self.device_rng``) and ``noise_gate`` (a device float[1]; 0 = add no noise), which is
        how one captured graph serves every step."""
        if self._on_hip(x_t, clip_fn):   # the same update as ONE kernel (two for dynamic thresholding)
            x_t, pred, kw = self._hip_step_args(x_t, pred, g, g_last, prediction_type, clip_fn, image_scale, pred_uncond,
                                                guidance_scale, thr_out, ddim_eta)
            rng = self.device_rng if rng is None else rng
            noisy = need_noise and not (ddim_eta is not None and ddim_eta <= 0)
            noise = input_noise
            if noisy and noise is None and rng is None:
                noise = torch.randn_like(x_t)   # torch's generator, like the reference (:340)
            x0, x_last = ops.sampler_step(x_t, pred, g, g_last, ddim_eta=ddim_eta, need_noise=noisy, noise=noise, rng=rng,
                                          noise_gate=noise_gate, **kw)
            if noisy and noise is None:
                rng.advance(x_t.numel())
            eps = (x_last - _b(g_last).sqrt() * x0) / (1 - _b(g_last)).sqrt() if return_eps else None
            return x0, x_last, eps
        if rng is not None or noise_gate is not None:
            raise ValueError("rng= and noise_gate= belong to the step kernel: GPU tensors only")
        alpha = g / g_last
        beta = 1 - alpha
        beta_tilde = beta * (1 - g_last) / (1 - g)
        x0 = self._x0_thresholded(x_t, pred, g, prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale, thr_out)
        if ddim_eta is None:  # ancestral DDPM posterior mean
            x_last = x0 * beta * g_last.sqrt() / (1 - g) + x_t * alpha.sqrt() * (1 - g_last) / (1 - g)
        else:
            eps = (x_t - x0 * g.sqrt()) / (1 - g).sqrt()
            if ddim_eta > 0:
                beta_tilde = (ddim_eta ** 2) * beta_tilde
                x_last = x0 * g_last.sqrt() + eps * (1 - g_last - beta_tilde).sqrt()
            else:
                need_noise = False
                x_last = x0 * g_last.sqrt() + eps * (1 - g_last).sqrt()
        if need_noise:
            noise = torch.randn_like(x_last) if input_noise is None else input_noise
            x_last = x_last + beta_tilde.sqrt() * noise
        eps = (x_last - g_last.sqrt() * x0) / (1 - g_last).sqrt() if return_eps else None
        return x0, x_last, eps

    def _on_hip(self, x_t, clip_fn):
        """GPU tensors take the step kernels, unless a custom ``clip_fn`` asks for the torch ops"""
        return x_t.is_cuda and (clip_fn is None or clip_fn == self.clip_sample)

    def _x0_thresholded(self, x_t, pred, g, prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale, thr_out):
        """what both updates start with, in torch ops: guidance combine, x0, threshold -> x0"""
        if pred_uncond is not None:
            pred = pred_uncond + guidance_scale * (pred - pred_uncond)
        x0 = self.get_x0_eps_from_pred(x_t, pred, g, prediction_type=prediction_type, return_eps=False)
        scale = 1 if image_scale is None else image_scale
        if thr_out is not None:
            thr_out.append(self._dynamic_thr(x0 * scale) if clip_fn == self.clip_sample else None)
        return torch.clip(x0, -scale, scale) / scale if clip_fn is None else clip_fn(x0, scale)

    def _hip_step_args(self, x_t, pred, g, g_last, prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale,
                       thr_out, ddim_eta=None):
        """what both step kernels start with -> (fp32 x_t, fp32 pred, their keyword arguments: prediction type, image scale,
        guidance, clip mode and per-sample threshold).  The dynamic thresholds cost one launch for the unclipped x0 and
        the five of the quantile's radix select (``ops.abs_quantile``)."""
        scale = 1 if image_scale is None else image_scale
        x_t, pred = x_t.float(), pred.float()
        kw = dict(prediction_type=prediction_type or self._config.prediction_type, image_scale=scale,
                  guidance_scale=guidance_scale, pred_uncond=None if pred_uncond is None else pred_uncond.float())
        fn = self._config.threshold_function if clip_fn is not None else None
        thr, clip = None, "NONE"
        if fn in (ThresholdType.DYNAMIC, ThresholdType.DYNAMIC_IF):
            x0s, _ = ops.sampler_step(x_t, pred, g, g_last, ddim_eta=ddim_eta, clip="X0_ONLY", **kw)
            thr = self._dynamic_thr(x0s)
            clip = "DYNAMIC"
        elif fn == ThresholdType.CLIP:
            clip = "CLIP"
        elif clip_fn is None:
            # clip_fn=None in the reference: clamp(x0, -s, s) / s == CLIP on x0 / s with unit scale ... only for s == 1
            if scale != 1:
                raise NotImplementedError("clip_fn=None with image_scale != 1 on the HIP path")
            clip = "CLIP"
        if thr_out is not None:
            thr_out.append(thr)
        return x_t, pred, dict(kw, clip=clip, thr=thr)

    def _dynamic_thr(self, x0s):
        """the per-sample threshold [B] of the dynamic threshold functions for the unclipped x0 in image units (the clamped
        quantile of its magnitude, as ``_threshold_sample`` takes it), None for the others"""
        fn = self._config.threshold_function
        if fn not in (ThresholdType.DYNAMIC, ThresholdType.DYNAMIC_IF):
            return None
        ratio, vmax = (0.995, 100) if fn == ThresholdType.DYNAMIC else (0.95, 1.5)
        flat = x0s if x0s.dtype == torch.float64 else x0s.float()
        return _abs_quantile_clamped(flat.reshape(flat.shape[0], -1), ratio, vmax)

    # ---- the two steps of image inversion (not in the reference) ----------------------------------------
    def get_inverted_xt(self, x_s, pred, g_s, g_t, prediction_type=None, pred_uncond=None, guidance_scale=1, out=None):
        """The preimage of one DDIM(0) step with the prediction held fixed (``invert_step`` has the formulas) -> x_t at the
        noisier level ``g_t``.  GPU tensors take ``ops.sampler_invert_step`` (``out``: the buffer it writes), CPU tensors
        the torch ops."""
        pt = prediction_type or self._config.prediction_type
        if self._on_hip(x_s, None):
            return ops.sampler_invert_step(x_s.float(), pred.float(), g_s, g_t, pt, guidance_scale=guidance_scale, out=out,
                                           pred_uncond=None if pred_uncond is None else pred_uncond.float())
        if out is not None:
            raise ValueError("out= belongs to the invert kernel: GPU tensors only")
        return invert_step(x_s, pred, g_s, g_t, pt, pred_uncond, guidance_scale)

    def get_noise_map(self, x_t, x_s, pred, g, g_last, prediction_type=None, clip_fn=None, ddim_eta=None, image_scale=None,
                      pred_uncond=None, guidance_scale=1):
        """The noise z for which the step of ``get_prediction_xt_last`` -- same arguments, ``need_noise=True,
        input_noise=z`` -- takes ``x_t`` to ``x_s``: z = (x_s - mu) / sigma, mu and sigma that step's mean and noise factor;
        0 for a sample with ``g_last == 1``.  ``ddim_eta``: None or > 0.  GPU tensors take ``ops.sampler_noise_map`` (the
        dynamic thresholds: the x0 kernel and ``ops.abs_quantile`` in front of it, as the step does), CPU tensors the torch
        ops: the step itself without noise, then ``noise_map``."""
        if ddim_eta is not None and ddim_eta <= 0:
            raise ValueError("get_noise_map: ddim_eta = %r adds no noise, there is no map to solve for" % (ddim_eta,))
        if self._on_hip(x_t, clip_fn):
            x_t, pred, kw = self._hip_step_args(x_t, pred, g, g_last, prediction_type, clip_fn, image_scale, pred_uncond,
                                                guidance_scale, None, ddim_eta)
            return ops.sampler_noise_map(x_t, x_s.float(), pred, g, g_last, ddim_eta=ddim_eta, **kw)
        _, mu, _ = self.get_prediction_xt_last(x_t, pred, g, g_last, prediction_type, clip_fn, need_noise=False,
                                               ddim_eta=ddim_eta, image_scale=image_scale, return_eps=False,
                                               pred_uncond=pred_uncond, guidance_scale=guidance_scale)
        return noise_map(x_s, mu, g, g_last, ddim_eta)

    # ---- one step of DPM-Solver++(2M) (not in the reference) ------------------------------------------
    def get_prediction_xt_last_2m(self, x_t, pred, g, g_last, g_prev=None, x0_prev=None, second_order=False,
                                  prediction_type=None, clip_fn=None, image_scale=None, pred_uncond=None,
                                  guidance_scale=1, thr_out=None, x0_out=None):
        """One update of DPM-Solver++(2M) (Lu et al. 2022, multistep, data prediction) -> (x0, x_last).

        Guidance combine, x0 and threshold as ``get_prediction_xt_last``; then, with alpha = sqrt(gamma), sigma =
        sqrt(1 - gamma), lambda = log(alpha / sigma), h = lambda(g_last) - lambda(g), h_prev = lambda(g) - lambda(g_prev),

            D      = (1 + h / (2 h_prev)) x0 - (h / (2 h_prev)) x0_prev     if second_order else x0
            x_last = (sigma_last / sigma) x_t + (alpha_last - sigma_last alpha / sigma) D

        ``second_order`` must be off when there is no history (first step) and when ``g_last == 1`` (last step: h is
        infinite; first order gives x_last = x0 there, as DDIM does).  First order is DDIM(eta = 0).  Gammas are
        per-sample tensors and need not lie on the schedule.  GPU tensors take ``ops.sampler_step_2m`` (where
        ``second_order`` may also be a device float[1] gate, and ``x0_out`` the buffer x0 is written to: ``x0_prev`` itself
        keeps the history in place), CPU tensors the torch ops below."""
        if self._on_hip(x_t, clip_fn):
            x_t, pred, kw = self._hip_step_args(x_t, pred, g, g_last, prediction_type, clip_fn, image_scale, pred_uncond,
                                                guidance_scale, thr_out)
            return ops.sampler_step_2m(x_t, pred, g, g_last, g_prev=g_prev, x0_prev=x0_prev, second_order=second_order,
                                       x0_out=x0_out, **kw)
        if x0_out is not None:
            raise ValueError("x0_out= belongs to the step kernel: GPU tensors only")
        x0 = self._x0_thresholded(x_t, pred, g, prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale, thr_out)
        D = x0
        if second_order:
            # 2 (lambda_a - lambda_b) = log(a (1 - b) / (b (1 - a))) = log1p((a - b) / (b (1 - a))): no cancellation
            h2 = torch.log1p((g_last - g) / (g * (1 - g_last)))
            h2_prev = torch.log1p((g - g_prev) / (g_prev * (1 - g)))
            r = 0.5 * h2 / h2_prev
            D = x0 + r * (x0 - x0_prev)
        ratio = ((1 - g_last) / (1 - g)).sqrt()
        x_last = ratio * x_t + (g_last.sqrt() - ratio * g.sqrt()) * D
        return x0, x_last

    # ---- one step of SA-Solver (not in the reference) -------------------------------------------------
    def get_prediction_xt_last_sa(self, x_t, pred, g, g_last, gate=(1, 0, 0.0, 0.0), h0=None, h1=None, psum=None, g_h0=None,
                                  g_h1=None, max_order=(3, 3), input_noise=None, rng=None, stochastic=None,
                                  prediction_type=None, clip_fn=None, image_scale=None, pred_uncond=None, guidance_scale=1,
                                  thr_out=None, x0_out=None):
        """One launch of SA-Solver (``SASolver`` has the definition) at the node of ``g`` -> (x0, x_last, (h0, h1, psum)).

        Guidance combine, x0 and threshold as ``get_prediction_xt_last``; then the corrector on ``x_t`` (the step from
        ``h0``'s node redone: x_t - psum + alpha sum c^c_j m_j), the predictor to ``g_last``, the predictor's sum for the
        next launch's corrector, and the history moved on: the returned state is (x0, the h0 given, the new sum).
        ``gate`` = (predictor order, corrector order, tau, tau of the corrected step) -- ``SASolver.gate`` makes it; on the
        last step (``g_last == 1``) it must be (1, 0, 0, .): x_last = x0.  ``h0`` / ``h1``: the x0 of the two launches before,
        formed at ``g_h0`` / ``g_h1``; ``psum``: the sum the launch before returned.  Gammas are per-sample tensors and
        need not lie on the schedule.  tau > 0 takes ``input_noise``, else ``torch.randn_like``.
        GPU tensors take ``ops.sampler_step_sa``: ``h0`` / ``h1`` / ``psum`` are then updated IN PLACE (and returned),
        ``gate`` may be a device float[4] and ``max_order`` = (P, C) its ceilings, ``x0_out`` the buffer x0 is written to
        (``h0`` itself is allowed), ``rng`` an ``ops.DeviceRng`` to draw from in the kernel (default ``self.device_rng``),
        which is advanced by ``x_t.numel()`` where ``stochastic`` is on (default: tau > 0 in a host gate) -- on every
        launch, whatever its tau, so that a captured graph and the eager loop draw the same numbers.
        CPU tensors take the torch ops below, in the dtype of ``x_t`` with the coefficients formed in fp64."""
        if self._on_hip(x_t, clip_fn):
            x_t, pred, kw = self._hip_step_args(x_t, pred, g, g_last, prediction_type, clip_fn, image_scale, pred_uncond,
                                                guidance_scale, thr_out)
            if stochastic is None:
                stochastic = (not torch.is_tensor(gate)) and gate[2] > 0
            rng = self.device_rng if rng is None else rng
            noise = input_noise
            if stochastic and noise is None and rng is None:
                noise = torch.randn_like(x_t)
            x0, x_last = ops.sampler_step_sa(x_t, pred, g, g_last, gate=gate, h0=h0, h1=h1, psum=psum, g_h0=g_h0, g_h1=g_h1,
                                             max_predictor=max_order[0], max_corrector=max_order[1], noise=noise,
                                             rng=rng if (stochastic and noise is None) else None, x0_out=x0_out, **kw)
            if stochastic and noise is None:
                rng.advance(x_t.numel())
            return x0, x_last, (h0, h1, psum)
        if x0_out is not None or rng is not None or torch.is_tensor(gate):
            raise ValueError("x0_out=, rng= and a device gate belong to the step kernel: GPU tensors only")
        p, c, tau, tau_c = gate
        x0 = self._x0_thresholded(x_t, pred, g, prediction_type, clip_fn, image_scale, pred_uncond, guidance_scale, thr_out)
        last = g_last >= 1
        if bool(last.all()):
            return x0, x0, (x0, h0, psum)
        gd = g.double()
        gl = torch.where(last, 0.5 * (1 + gd), g_last.double())   # a finite stand-in where the sample is on its last step
        to = lambda v: v.to(x_t.dtype)
        x_a = x_t
        if c >= 1:
            g0 = g_h0.double()
            cc = sa_corrector_coeffs(_dlambda(g0, gd), tau_c, c, _dlambda(g_h1.double(), g0) if c >= 3 else None)
            s = to(gd.sqrt() * cc[0]) * x0
            if c >= 2:
                s = s + to(gd.sqrt() * cc[1]) * h0
            if c >= 3:
                s = s + to(gd.sqrt() * cc[2]) * h1
            x_a = x_t - psum + s
        h = _dlambda(gd, gl)
        cp = sa_predictor_coeffs(h, tau, p, _dlambda(g_h0.double(), gd) if p >= 2 else None,
                                 _dlambda(g_h1.double(), g_h0.double()) if p >= 3 else None)
        s = to(gl.sqrt() * cp[0]) * x0
        if p >= 2:
            s = s + to(gl.sqrt() * cp[1]) * h0
        if p >= 3:
            s = s + to(gl.sqrt() * cp[2]) * h1
        x_last = to(((1 - gl) / (1 - gd)).sqrt() * torch.exp(-tau * tau * h)) * x_a + s
        if tau > 0:
            noise = torch.randn_like(x_t) if input_noise is None else input_noise
            x_last = x_last + to((1 - gl).sqrt() * (-torch.expm1(-2 * tau * tau * h)).sqrt()) * noise
        if bool(last.any()):
            x_last = torch.where(last, x0, x_last)
        return x0, x_last, (x0, h0, s)

    def _threshold_sample(self, sample, ratio=0.995, max_value=100):
        """Imagen dynamic thresholding (:461-498)."""
        shape, dtype = sample.shape, sample.dtype
        flat = (sample if sample.dtype == torch.float64 else sample.float()).reshape(shape[0], -1)   # fp64 stays fp64
        s = _abs_quantile_clamped(flat, ratio, max_value).unsqueeze(1)
        return (torch.clamp(flat, -s, s) / s).reshape(shape).to(dtype)

    def clip_sample(self, pred_x0, image_scale=1):
        s, fn = image_scale, self._config.threshold_function
        if fn == ThresholdType.CLIP:
            return (pred_x0 * s).clip(-1, 1) / s
        if fn == ThresholdType.DYNAMIC:
            return self._threshold_sample(pred_x0 * s, 0.995, 100) / s
        if fn == ThresholdType.DYNAMIC_IF:
            return self._threshold_sample(pred_x0 * s, 0.95, 1.5) / s
        return pred_x0

    # ---- loss-guided sampling (LossGuide; not in the reference) ---------------------------------------
    def _x0_coeffs(self, g, prediction_type=None):
        """(a, b) of x0 = a x_t + b pred (``get_x0_eps_from_pred``), shaped like ``g``"""
        pt = prediction_type or self._config.prediction_type
        if pt in (PredictionType.DDPM, PredictionType.DDIM):
            return 1 / g.sqrt(), -(1 - g).sqrt() / g.sqrt()
        if pt == PredictionType.V_PREDICTION:
            return g.sqrt(), -(1 - g).sqrt()
        raise ValueError("unsupported prediction type")

    def _guide_update(self, guide, x_in, preds, x0, x_s, g, image_scale, guidance_scale, thr=None):
        """The guide's correction of one step.  Lists hi -> lo: ``x_in`` the leaves the model was run on, ``preds`` the
        (conditional, unconditional or None) predictions still attached to the tape, ``x_s`` the step's results; ``x0`` /
        ``g`` / ``image_scale`` / ``thr``: the top scale's clean-image estimate as the step returned it, its gamma, image scale
        and dynamic threshold (``thr_out`` of the step; None for the other threshold functions).
        -> the corrected ``x_s`` list (GPU tensors: in place)"""
        scale = image_scale if image_scale else 1
        loss, v = guide.loss_and_grad(x0 * scale if scale != 1 else x0)
        a, b = self._x0_coeffs(g)
        fn = self._config.threshold_function
        dynamic = fn in (ThresholdType.DYNAMIC, ThresholdType.DYNAMIC_IF)
        pc, pu = preds[0]
        if x0.is_cuda:
            clip = "DYNAMIC" if dynamic else ("CLIP" if fn == ThresholdType.CLIP else "NONE")
            direct, seed = ops.guide_seed(v.float(), x0, a, b, clip=clip, thr=thr if dynamic else None, image_scale=scale)
        else:
            w = v * scale
            if fn != ThresholdType.NONE:
                # clipped: x0 = +-fl(1 / scale), and fl(fl(1 / scale) scale) is 1 or a rounding below it when scale is no
                # power of two -- four ulps of slack, as the kernel takes (mdm_guide_seed)
                w = w * ((x0 * scale).abs() < 1 - 4 * torch.finfo(x0.dtype).eps).to(v.dtype)
            if dynamic:   # the quantile the step's clip_sample took, as a constant
                w = w / _b(thr).to(v.dtype)
            direct, seed = a * w, b * w
        seed = seed.to(pc.dtype)
        outs, seeds = ([pc], [seed]) if pu is None else ([pc, pu], [guidance_scale * seed, (1 - guidance_scale) * seed])
        jts = torch.autograd.grad(outs, x_in, grad_outputs=seeds, allow_unused=True)
        zeta = guide.zeta(loss)
        out = list(x_s)
        for i, (x, jt) in enumerate(zip(x_s, jts)):
            d = direct if i == 0 else None
            if d is None and jt is None:
                continue
            if x.is_cuda:
                out[i] = ops.guide_apply(x, zeta, direct=d, jt=None if jt is None else jt.float())
            else:
                grad = d if jt is None else (jt if d is None else d + jt)
                out[i] = x - _b(zeta).to(x.dtype) * grad
        return out

    # ---- attention-map guidance (MapGuide; not in the reference) ----------------------------------------
    def _map_guide_pass(self, mg, model, time_step, x_t, t, lm_outputs, lm_mask, micros, guidance_scale):
        """The correction of x_t in front of one guided step (``MapGuide``): ``mg.iterations`` times, the model on leaf x_t
        (the list of scales, hi -> lo) with grad enabled and frozen parameters -- the B conditional rows with their text, at
        the time the step uses, under the recorder switch alone --, the loss of the recorded maps, one ``autograd.grad`` to
        the leaves, x_t <- x_t - scale grad per scale that got one.  -> the moved list (new tensors: the caller's stay)"""
        B = x_t[0].shape[0]
        if guidance_scale != 1:   # [uncond | cond] -> cond
            rows = lm_outputs.shape[0]
            assert rows == 2 * B
            half = lambda v: v[-B:] if (torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == rows) else v
            lm_outputs, lm_mask, micros = half(lm_outputs), half(lm_mask), {k: half(v) for k, v in micros.items()}
        vision_model = getattr(model, "vision_model", model)
        names = _attn_maps.layer_names(vision_model, mg.layers)
        scale = mg.scale_at(time_step, self.n_steps)
        xs = list(x_t)
        for _ in range(mg.iterations):
            x_in = [x.detach().clone().requires_grad_(True) for x in xs]
            handle = _attn_maps.GradRows(lm_outputs.shape[1], 0, B, B)
            with torch.enable_grad(), _frozen_parameters(model), _attn_maps.applied(vision_model, handle, names):
                self._call_model(model, x_in, t - 1, lm_outputs, lm_mask, micros)   # model sees t-1 (:415); outputs discarded
                if not handle.counts():
                    raise ValueError("MapGuide: no layer recorded (the model was run without text keys)")
                loss = mg.loss(handle.maps(), B)
                grads = torch.autograd.grad(loss.sum(), x_in, allow_unused=True)
            zeta = torch.where(loss.detach() > 0, torch.full_like(loss.detach(), scale), torch.zeros_like(loss.detach())).float()
            for i, g in enumerate(grads):
                if g is None:
                    continue
                x = x_in[i].detach()
                if x.is_cuda:
                    xs[i] = ops.guide_apply(x, zeta, direct=g.float())
                else:
                    z = _b(zeta).to(x.dtype)
                    xs[i] = torch.where(z != 0, x - z * g, x)
        return xs

    def forward_model(self, model, x_t, t, lm_outputs, lm_mask, micros={}, guidance_scale=1):
        """classifier-free guidance doubles the batch: [uncond | cond] (:435-459)."""
        (pc,), (pu,), extras, _ = self._forward_model_raw(model, [x_t], t, lm_outputs, lm_mask, micros, guidance_scale)
        return (pc if pu is None else pu + guidance_scale * (pc - pu)), extras

    def _forward_model_raw(self, model, x_t, t, lm_outputs, lm_mask, micros, guidance_scale, opts=SampleOptions(),
                           rows=None, step=None):
        """The one denoiser call of a step.  ``x_t``: the list of scales -> (conditional predictions, unconditional
        predictions or Nones, extras, perturbed predictions or None), one entry per scale: the guidance combine itself is
        folded into the step kernel.  The model runs once, on [uncond | cond | perturbed] -- the blocks ``opts.blocks``
        names, the perturbed one with the conditional rows' conditioning (``pag_rows``) -- under ``opts.switches``.
        ``opts.tiles``: every block holds the windows of every image, B T rows (``gather_windows``), the conditioning and
        the times are repeated per window, and the predictions are merged back to whole canvases (``merge_windows``) before
        they are split; the extras are those of each image's window 0.  ``rows``: (T, (lm_outputs, lm_mask, micros)) -- the
        window count of the checked geometry and what ``model_rows`` made for this call; ``_sample`` makes both once, not
        once per step.  ``step``: (the time the step starts from, ``num_diffusion_steps``) for ``opts.attn_maps``'s interval."""
        uncond, pert = opts.blocks(guidance_scale)
        B = x_t[0].shape[0]
        tiles, T = opts.tiles, 1
        if tiles is not None:
            ratios = self._scale_info(model)[0]
            canvases = [tuple(x.shape[2:]) for x in x_t]
            T = rows[0] if rows is not None else tiles.check(*canvases[0], ratios).count(*canvases[0])
        lm_outputs, lm_mask, micros = (rows[1] if rows is not None
                                       else model_rows(opts, guidance_scale, B, T, lm_outputs, lm_mask, micros))
        reps = 1 + uncond + pert
        if tiles is None:
            xin, tin = repeat_rows(x_t, t, reps)
        else:
            xin, tin = gather_windows(x_t, tiles, ratios, reps), _tiling.time_rows(t, T, reps)
        with opts.switches(model, guidance_scale, B * T, x_t[0].device, step=step):
            preds, extras = self._call_model(model, xin, tin, lm_outputs, lm_mask, micros)
        if tiles is not None:
            preds = merge_windows(preds, tiles, ratios, canvases)
            if extras is not None:
                extras = extras[::T]
        if extras is not None and reps > 1:
            extras = extras.chunk(reps)[int(uncond)]
        pcs, pus, pps = split_rows(preds, uncond, pert)
        return pcs, pus, extras, pps

    # ---- what differs between one scale and several: NestedSampler overrides these ----------------------------
    def _call_model(self, model, xs, t, lm_outputs, lm_mask, micros):
        """the model on the list of scales ``xs`` -> (list of predictions, extras)"""
        pred, extras = model(xs[0], t, lm_outputs, lm_mask, micros)
        return [pred], extras

    def _to_scales(self, model, x_t):
        """what ``get_xt_minus_1`` is given -> the list of scales, hi -> lo"""
        return [x_t]

    def _from_scales(self, xs):
        """a list of scales -> the form ``get_xt_minus_1`` takes and returns"""
        return xs[0]

    def _scale_info(self, model):
        """-> (top side / side, image_scale) of every scale, hi -> lo: what the step kernel of that scale gets"""
        return [1], [self._config.rescale_signal or 1]

    def _gammas_of_scales(self, model, gamma):
        """the schedule's gamma -> that of every scale, hi -> lo"""
        return [gamma]

    def _noisy_step(self, time_step, last):
        """the last step adds no noise (:421); elementwise on arrays of times"""
        return last != 0

    def _scale_gammas(self, model, time, B):
        """gamma of every scale (hi -> lo) at schedule time ``time``, [B, 1, 1, 1] each"""
        return self._gammas_of_scales(model, self.read_gamma(torch.ones(B, dtype=torch.long, device=self.gammas.device) * time))

    # ---- one iteration: denoiser, then the update of every scale -----------------------------------------------
    def get_xt_minus_1(self, model, time_step, x_t, lm_outputs, lm_mask, micros={}, time_step_last=None,
                       guidance_scale=1, ddim_eta=None, return_details=False, solver=None, solver_state=None,
                       second_order=False, **options):
        """``x_t`` and what is returned: tensors here, hi -> lo lists in ``NestedSampler`` (whose first step may be given the
        top scale alone).  ``solver="dpmpp_2m"``: the DPM-Solver++(2M) update instead of DDPM / DDIM.  ``solver_state`` is
        the caller's dict of history, updated in place: {"x0": x0 of the step before, "g": the gamma it was formed at};
        ``second_order`` (decided by the caller: off on the first and on the last step) uses it.  ``solver=SASolver(...)`` /
        ``"sa"``: SA-Solver; ``solver_state`` then carries "h0", "h1", "psum" (the x0 of the two launches before and the
        predictor's sum), "g0", "g1" (their gammas), "count" (launches so far: the orders follow it, an empty dict restarts
        them) and "tau" (of the step before), and ``second_order`` is not used.  ``options``: the keywords
        of ``SampleOptions`` (``guide``, ``pag_scale``, ``pag_layers``, ``regions``, ``region_layers``, ``freeu``, ``cfg``,
        ``tiles``), checked here.  The momentum history of ``cfg`` lives in ``solver_state["cfg_run"]`` (one tensor per
        scale, absent until the first guided step), so without a ``solver_state`` every call starts without history."""
        opts = SampleOptions(**options).check()
        rule = _checked_rule(solver, ddim_eta, opts)
        last = time_step - 1 if time_step_last is None else time_step_last
        row = rule.row(self, {} if solver_state is None else solver_state, time_step, last, second_order=second_order)
        return self._step(model, time_step, x_t, lm_outputs, lm_mask, micros, opts, rule, row, last, guidance_scale,
                          return_details, solver_state)

    def _step(self, model, time_step, x_t, lm_outputs, lm_mask, micros, opts, rule, row, last, guidance_scale=1,
              return_details=False, solver_state=None, rows=None, noise_fn=None, step_noise=None):
        """``get_xt_minus_1`` behind its checks: what the loop of ``_sample`` calls, with the options it checked and the
        ``StepRule`` it resolved once, that rule's ``row`` of this step and the time ``last`` the step goes to (and, under
        ``opts.tiles``, with the window count and the conditioning it repeated per window once: ``rows``).  Denoiser, update
        of every scale, then the guide's correction if there is one: with a guide the model runs on leaf x_t with grad
        enabled and the update under no_grad on detached tensors; without, in the caller's grad mode."""
        x_t = self._to_scales(model, x_t)
        ones = torch.ones(x_t[0].shape[0], dtype=torch.long, device=self.gammas.device)
        t = ones * time_step
        g_t = self._gammas_of_scales(model, self.read_gamma(t))
        g_s = self._gammas_of_scales(model, self.read_gamma(ones * last))
        image_scales = self._scale_info(model)[1]
        st = {} if solver_state is None else solver_state
        g_hist, state = rule.load(self, st, x_t, g_t)
        if opts.map_guide is not None and opts.map_guide.on(time_step, self.n_steps):   # moves x_t; the step below is unchanged
            x_t = self._map_guide_pass(opts.map_guide, model, time_step, x_t, t, lm_outputs, lm_mask, micros, guidance_scale)
        cfg_kw = {} if opts.cfg_at(guidance_scale) is None else dict(cfg_state=st, cfg_on=opts.cfg.on(time_step, self.n_steps))
        guide = opts.guide
        x_in, grad, no_grad, thr = x_t, _UNCHANGED, _UNCHANGED, None
        if guide is not None:
            x_in = [x.detach().requires_grad_(True) for x in x_t]
            grad, no_grad = torch.enable_grad(), torch.no_grad()
            thr = []   # one entry per scale, hi -> lo
        with grad:
            pcs, pus, _, pps = self._forward_model_raw(model, x_in, t - 1, lm_outputs, lm_mask, micros, guidance_scale,
                                                       opts, rows, (time_step, self.n_steps))   # model sees t-1 (:415)
        outs = (x_in, pcs, pus)
        if guide is not None:   # the update itself: unchanged, on detached tensors
            outs = ([None if v is None else v.detach() for v in vs] for vs in outs)
        with no_grad:
            x0, x_s = self._step_scales(*outs, g_t, g_s, image_scales, opts, rule, row, state, g_hist, guidance_scale,
                                        thr_out=thr, pps=pps, noise_fn=noise_fn, step_noise=step_noise, **cfg_kw)
        if guide is not None:
            x_s = self._guide_update(guide, x_in, list(zip(pcs, pus)), x0[0], x_s, g_t[0], image_scales[0], guidance_scale,
                                     thr[0])
        rule.store(self, st, state, x0, g_t, row)
        if not return_details:
            return self._from_scales(x_s)
        return self._from_scales(x0), self._from_scales(x_s), (g_t[-1], g_s[-1])

    def _step_scales(self, x_t, pcs, pus, g_t, g_s, image_scales, opts, rule, row, state, g_hist=(), guidance_scale=1,
                     thr_out=None, pps=None, rng=None, cfg_state=None, cfg_on=True, cfg_gates=None, noise_fn=None,
                     step_noise=None):
        """The update of every scale behind the denoiser call -> (x0 list, x_s list), all lists hi -> lo: ``rule.step`` per
        scale with the rule's ``row``, ``state`` and ``g_hist`` (``StepRule``).  The one reverse step of the eager samplers
        and of ``GraphedSampler``, whose graph passes a device row, the rule's buffers, its generator ``rng`` and the cfg
        state and gates through to the kernels.  What the step is handed is ``_guided_preds``'s.  ``step_noise``: this
        step's noise maps, one per scale (``_sample``'s ``step_noise[i]``), the ``input_noise`` of the ancestral step."""
        n = len(x_t)
        pcs, pus, guidance_scale = self._guided_preds(x_t, pcs, pus, g_t, image_scales, opts, guidance_scale, pps, cfg_state,
                                                      cfg_on, cfg_gates)
        kw = dict(prediction_type=self._config.prediction_type, clip_fn=self.clip_sample, guidance_scale=guidance_scale,
                  thr_out=thr_out, rng=rng, noise_fn=noise_fn)
        given = (lambda k: {}) if step_noise is None else (lambda k: dict(input_noise=step_noise[k]))
        x0, x_s = zip(*(rule.step(self, k, x_t[k], pcs[k], g_t[k], g_s[k], row, g_hist, state, image_scale=image_scales[k],
                                  pred_uncond=pus[k], **given(k), **kw) for k in range(n)))
        return list(x0), list(x_s)

    def _guided_preds(self, x_t, pcs, pus, g_t, image_scales, opts, guidance_scale=1, pps=None, cfg_state=None, cfg_on=True,
                      cfg_gates=None):
        """What the update of a step is handed, from what the denoiser call returned -> (predictions, unconditional
        predictions or Nones, guidance scale), lists hi -> lo.  ``pps`` with ``opts.pag_scale != 0``: the perturbed
        predictions -- one combine per scale (GPU tensors: ``ops.pag_combine``, CPU tensors: ``pag_combine``) makes the guided
        prediction, with no unconditional one and guidance 1; ``opts.cfg`` with ``guidance_scale != 1``: the same with
        ``_cfg_scales``.  Neither: as given -- the plain combine is the step kernel's."""
        n = len(x_t)
        cfg, pag_scale = opts.cfg_at(guidance_scale), opts.pag_scale
        if cfg is not None:
            pcs = self._cfg_scales(cfg, x_t, pcs, pus, g_t, image_scales, guidance_scale, cfg_state, cfg_on, cfg_gates)
            pus, guidance_scale = [None] * n, 1
        if pps is not None and pag_scale != 0:
            pcs = [ops.pag_combine(pc.float(), None if pu is None else pu.float(), pp.float(), guidance_scale, pag_scale)
                   if pc.is_cuda else pag_combine(pc, pu, pp, guidance_scale, pag_scale) for pc, pu, pp in zip(pcs, pus, pps)]
            pus, guidance_scale = [None] * n, 1
        return pcs, pus, guidance_scale

    def _cfg_scales(self, cfg, x_t, pcs, pus, g_t, image_scales, guidance_scale, state=None, on=True, gates=None):
        """The projected / rescaled guidance combine of every scale (``mdm_hip/guidance.py``) -> the guided predictions.
        ``state``: the trajectory's dict; ``state["cfg_run"]`` holds the momentum history, one tensor per scale, updated here
        (GPU tensors: in place) and absent until the first guided step.  Eager: ``on`` says whether the step lies in the
        guidance interval -- outside it nothing is launched, the conditional predictions pass through and the history
        stays.  ``GraphedSampler``: ``gates`` = (run_gate, w_gate), device float[1] each, and static history buffers in
        ``state["cfg_run"]``; the same kernels run gated on every row, to the same bits."""
        if gates is None and not on:
            return pcs
        state = {} if state is None else state
        run = state.get("cfg_run")
        run_gate, w_gate = gates if gates is not None else (None, None)
        kw = dict(cfg.options(), prediction_type=self._config.prediction_type)
        out, runs = [], []
        for i, (x, pc, pu) in enumerate(zip(x_t, pcs, pus)):
            prev = None if run is None else run[i]
            if pc.is_cuda:
                p, r = ops.cfg_combine(x.float(), pc.float(), pu.float(), g_t[i], guidance_scale=guidance_scale,
                                       image_scale=image_scales[i], run_prev=prev, run_out=prev, run_gate=run_gate,
                                       w_gate=w_gate, **kw)
            else:
                p, r = _guidance.cfg_combine(x, pc, pu, g_t[i], guidance_scale=guidance_scale, image_scale=image_scales[i],
                                             run_prev=prev, **kw)
            out.append(p)
            runs.append(r)
        if cfg.momentum != 0:
            state["cfg_run"] = runs
        return out

    # ---- the sampling loop (:510-609) ----------------------------------------------------------
    def set_timesteps(self, num_inference_steps=250):
        ratio = (self._config.num_diffusion_steps + 1) / (num_inference_steps + 1)
        return (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1].copy().astype(np.int64)

    def sample(self, *args, **kwargs):
        """``solver=None``: ancestral DDPM, or DDIM with ``ddim_eta`` (the reference's two).  ``solver="dpmpp_2m"``:
        DPM-Solver++(2M), deterministic, second order, one denoiser call per step -- made for few steps
        (``resample_steps=True, num_inference_steps=20..50``).  ``solver=SASolver(predictor, corrector, tau,
        tau_interval)`` (``"sa"``: the defaults): SA-Solver, a predictor-corrector of up to third order with a noise level
        between the probability-flow ODE and the reverse SDE, one denoiser call per step too; its noise comes from
        ``use_device_rng`` if set, else from ``torch.randn_like``.  It takes no ``guide=`` and no ``resample > 1``.
        ``step_noise=maps`` (what ``noise_maps`` returned for an image, with the same schedule arguments and ``t=``): the
        ancestral step adds ``maps[i][k]`` at step i, scale k, in place of drawn noise -- the trajectory of that image, or,
        with another prompt, its edit (``_sample`` has the details)."""
        opts = SampleOptions.pop(dict(kwargs)).check()   # the checks of the call, here and not at the generator's first next()
        _checked_rule(kwargs.get("solver"), kwargs.get("ddim_eta"), opts, kwargs.get("known_images"), kwargs.get("resample", 1))
        _check_step_noise(kwargs.get("step_noise"), kwargs.get("solver"), kwargs.get("ddim_eta"), kwargs.get("resample", 1))
        guide = opts.guide
        gen = self._sample(*args, **kwargs)
        if guide is None:
            return gen if kwargs.get("yield_output", False) else next(gen)
        # a guided call freezes the parameters while it computes (the backward passes launch input gradients only) and
        # hands them back before it returns -- around every item of a yield_output generator, not across the caller's code
        model = args[0] if args else kwargs["model"]
        if not kwargs.get("yield_output", False):
            with _frozen_parameters(model):
                return next(gen)
        return self._frozen_items(gen, model)

    @staticmethod
    def _frozen_items(gen, model):
        while True:
            with _frozen_parameters(model):
                try:
                    item = next(gen)
                except StopIteration:
                    return
            yield item

    def _known_region(self, model, x_t, known_images, known_mask, known_seed, known_noise_fn):
        ratios, image_scales = self._scale_info(model)
        top = x_t[0] if isinstance(x_t, (list, tuple)) else x_t
        B, C, H, W = top.shape
        if H % ratios[-1] or W % ratios[-1]:
            raise ValueError("image side %d x %d is not a multiple of the nesting ratio %d" % (H, W, ratios[-1]))
        shapes = [(B, C, H // r, W // r) for r in ratios]
        return KnownRegion.build(shapes, top.device, top.dtype if top.is_floating_point() else torch.float32, known_images,
                                 known_mask, ratios, image_scales, known_seed, known_noise_fn)

    # ---- image inversion (not in the reference): from a GIVEN image to the noise and the trajectory that reproduce it -------
    INVERSION_REFUSED = {
        "guide": "guide=: the guide corrects x_s after a reverse step, and inversion takes no reverse step",
        "map_guide": "map_guide=: it moves x_t in front of a reverse step, and inversion takes no reverse step",
        "tiles": "tiles=: inversion of a canvas larger than the model's window is not implemented",
        "known_images": "known_images=: the whole image is given -- there is no free region to hold beside a known one",
        "cfg": "cfg=: the projected / rescaled combine carries a momentum along the sampling direction and reads x_t; the "
               "implicit step that mdm_sampler_invert_step solves takes the plain combine p_u + w (p_c - p_u) only",
        "pag": "pag_scale != 0: mdm_sampler_invert_step takes the plain combine p_u + w (p_c - p_u) only, a combine of three "
               "predictions in front of it is not implemented",
        "control": "control=: inversion finds the trajectory of a GIVEN image under its own prompt -- there is no source row to "
                   "take attention maps from; control belongs to the replay (sample_from)",
    }

    def _inversion_options(self, what, options, refused):
        """the ``SampleOptions`` of an inversion call out of its keywords, checked; ``refused``: the names of
        ``INVERSION_REFUSED`` this call cannot have"""
        on = {name: options.pop(name, None) is not None for name in ("known_images", "known_mask")}
        opts = SampleOptions(**options).check()
        on = dict(guide=opts.guide is not None, map_guide=opts.map_guide is not None, tiles=opts.tiles is not None,
                  known_images=on["known_images"] or on["known_mask"], cfg=opts.cfg is not None, pag=opts.pag_scale != 0,
                  control=opts.control is not None)
        for name in tuple(refused) + ("control",):   # (no inversion call takes a control)
            if on[name]:
                raise NotImplementedError("%s does not take %s" % (what, self.INVERSION_REFUSED[name]))
        return opts

    def _inversion_nodes(self, what, num_inference_steps, resample_steps, t):
        """the schedule nodes of an inversion call, descending to 0: those of ``_sample`` with the same arguments; ``t``
        keeps the nodes <= t, the first of which is where ``partial_diffusion`` would start"""
        steps = self.set_timesteps(num_inference_steps if resample_steps else self.n_steps)
        if t is not None:
            if not (steps <= t).any():
                raise ValueError("%s: t = %r is below every step of the schedule" % (what, t))
            steps = steps[steps <= t]
        return steps

    def _image_scales(self, model, images):
        """a top-scale image in output units -> (the average-pooled pyramid hi -> lo, the image scale of every level): the
        clean image of level k in the units of x_t is pyramid[k] / scale[k], as ``partial_diffusion`` takes it"""
        ratios, image_scales = self._scale_info(model)
        hip = images.is_cuda
        top = images.float() if hip else images
        if top.shape[-2] % ratios[-1] or top.shape[-1] % ratios[-1]:
            raise ValueError("image side %d x %d is not a multiple of the nesting ratio %d" % (*top.shape[-2:], ratios[-1]))
        return [top] + [ops.avgpool(top, r) if hip else F.avg_pool2d(top, r) for r in ratios[1:]], image_scales

    @torch.no_grad()
    def invert(self, model, images, lm_outputs, lm_mask, micros={}, iterations=1, num_inference_steps=2000,
               resample_steps=False, t=None, guidance_scale=1, **options):
        """DDIM inversion with fixed-point refinement (Song et al. 2021; Pan et al. 2023, "AIDI"; Garibi et al. 2024,
        "ReNoise"): the deterministic DDIM(0) map walked BACKWARDS from ``images`` (top scale, output units) -> (x_t at the
        noisiest node reached -- a hi -> lo list in ``NestedSampler`` --, that node's time), so that ``sample(model, x_t, ...,
        t=time, ddim_eta=0)`` with the same schedule arguments, conditioning and guidance returns the images.

        The nodes are those of ``set_timesteps`` as ``_sample`` takes them (``num_inference_steps`` / ``resample_steps``),
        walked in ascending order from node 0, where every scale holds its clean image / image scale (a nested model: the
        average-pooled pyramid); ``t`` stops at the first node <= t.  A step from node s to the noisier node t is implicit
        -- the prediction belongs to the x_t looked for -- and is solved by ``iterations`` = K denoiser calls:

            y^0 = x_s ;   y^{j+1} = invert_step(x_s, p(y^j, t))   (``get_inverted_xt``; the model is handed t - 1) ;   x_t = y^K

        K = 1 is plain DDIM inversion with the prediction evaluated at the target time; more converge to the exact
        preimage of the DDIM(0) step (for the v-prediction of Gaussian data on the cosine schedule the round-trip error
        falls 16x per iteration).  K n denoiser calls over n steps: ``GraphedSampler.invert`` replays them.  No threshold is
        applied -- a clamp has no inverse --, so the round trip is exact where sampling does not clamp either.
        ``options``: of ``SampleOptions`` those that only change the denoiser call -- ``regions`` / ``region_layers``,
        ``freeu``, and ``attn_maps``, which records the maps of the GIVEN image, at the last iteration of every step in its
        interval; LoRA and MXFP8 act inside the model.  ``INVERSION_REFUSED`` says why the others are not taken."""
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError("invert: iterations = %r (wanted an int >= 1)" % (iterations,))
        opts = self._inversion_options("invert", dict(options), ("guide", "map_guide", "tiles", "known_images", "cfg", "pag"))
        quiet = opts if opts.attn_maps is None else SampleOptions(**dict(vars(opts), attn_maps=None))
        nodes = self._inversion_nodes("invert", num_inference_steps, resample_steps, t)[::-1]
        pyr, image_scales = self._image_scales(model, images)
        xs = [x if sc == 1 else x / sc for x, sc in zip(pyr, image_scales)]
        B = xs[0].shape[0]
        ones = torch.ones(B, dtype=torch.long, device=self.gammas.device)
        for s, tt in zip(nodes[:-1], nodes[1:]):
            g_s, g_t = self._scale_gammas(model, int(s), B), self._scale_gammas(model, int(tt), B)
            ys = xs
            for j in range(iterations):
                pcs, pus, _, _ = self._forward_model_raw(model, ys, ones * int(tt) - 1, lm_outputs, lm_mask, micros,
                                                         guidance_scale, opts if j == iterations - 1 else quiet, None,
                                                         (int(tt), self.n_steps))
                ys = [self.get_inverted_xt(xs[k], pcs[k], g_s[k], g_t[k], pred_uncond=pus[k], guidance_scale=guidance_scale)
                      for k in range(len(xs))]
            xs = ys
        return self._from_scales(xs), int(nodes[-1])

    @torch.no_grad()
    def noise_maps(self, model, images, lm_outputs, lm_mask, micros={}, num_inference_steps=2000, resample_steps=False,
                   t=None, guidance_scale=1, ddim_eta=None, seed=0, noise_fn=None, return_nodes=False, **options):
        """Edit-friendly DDPM inversion (Huberman-Spiegelglas et al. 2024) of ``images`` (top scale, output units) ->
        (x_start, maps) for ``sample(model, x_start, ..., t=<the same>, step_noise=maps)`` with the same schedule arguments
        and ``ddim_eta`` (None: the DDPM posterior; or > 0).

        Every node above 0 of the trajectory (``_sample``'s steps; ``t`` keeps those <= t) gets a noisy copy of the image
        of its own, with INDEPENDENT noise, x_i = alpha_i image / scale + sigma_i eps_i per scale (a nested model: the
        average-pooled pyramid and every scale's own gamma); ``x_start`` is the first.  ``maps[i]``, one tensor per scale
        hi -> lo, is the noise z for which step i lands on the next copy exactly: z = (x_{i+1} - mu_i) / sigma_i with mu_i,
        sigma_i the mean and noise factor of the ancestral step at x_i under the model's prediction there, this call's
        conditioning and guidance, and the sampler's own threshold function (``get_noise_map``).  None where the step adds
        no noise (``_noisy_step``: the last).  The n - 1 denoiser calls are independent of each other.
        Replaying the maps reproduces the copies, hence the image, under ANY guidance scale and threshold function, because
        the maps absorb what the step does; another prompt at replay edits the image with its layout kept.
        The draws: GPU tensors -- ``ops.noise_images`` from ONE ``ops.DeviceRng(seed)`` on stream 0, the nodes in sampling
        order (noisiest first), within a node the scales hi -> lo, the generator advanced by ``numel`` after each; CPU
        tensors -- ``noise_fn(image)`` (default ``torch.randn_like``) called in the same order.
        ``options``: as ``invert``, plus ``cfg=`` and ``pag_scale`` / ``pag_layers`` -- the prediction handed on is then the
        combined one (``_guided_preds``, what the step itself would be handed).  ``return_nodes``: also return the copies, a
        list over the nodes of hi -> lo lists."""
        if ddim_eta is not None and ddim_eta <= 0:
            raise ValueError("noise_maps: ddim_eta = %r is deterministic, it adds no noise to extract" % (ddim_eta,))
        opts = self._inversion_options("noise_maps", dict(options), ("guide", "map_guide", "tiles", "known_images"))
        steps = self._inversion_nodes("noise_maps", num_inference_steps, resample_steps, t)
        if len(steps) < 2:
            raise ValueError("noise_maps: t = %r leaves no step to invert" % (t,))
        times = steps[:-1]
        noisy = Ancestral(ddim_eta).rows(self, times, steps[1:])[:, 0]
        pyr, image_scales = self._image_scales(model, images)
        hip = images.is_cuda
        B = pyr[0].shape[0]
        rng = ops.DeviceRng(seed, images.device) if hip else None
        noise_fn = noise_fn or torch.randn_like

        def copy_at(time):
            if time == 0:   # gamma = 1: the image itself, nothing drawn
                return [x if sc == 1 else x / sc for x, sc in zip(pyr, image_scales)]
            out = []
            for img, g, sc in zip(pyr, self._scale_gammas(model, time, B), image_scales):
                if hip:
                    out.append(ops.noise_images(img, g, rng=rng, inv_scale=1.0 / sc)[0])
                    rng.advance(img.numel())
                else:
                    out.append(Sampler.get_xt(self, img if sc == 1 else img / sc, noise_fn(img), g))
            return out

        ones = torch.ones(B, dtype=torch.long, device=self.gammas.device)
        history = {}   # cfg: the momentum buffers, along the sampling direction
        x_start = cur = copy_at(int(times[0]))
        nodes, maps = [cur], []
        for i, ts in enumerate(times):
            ts, last = int(ts), int(steps[i + 1])
            if not noisy[i]:
                maps.append(None)
                continue
            nxt = copy_at(last)
            g_t, g_s = self._scale_gammas(model, ts, B), self._scale_gammas(model, last, B)
            pcs, pus, _, pps = self._forward_model_raw(model, cur, ones * ts - 1, lm_outputs, lm_mask, micros, guidance_scale,
                                                       opts, None, (ts, self.n_steps))
            cfg_kw = {} if opts.cfg_at(guidance_scale) is None else dict(cfg_state=history, cfg_on=opts.cfg.on(ts, self.n_steps))
            pcs, pus, w = self._guided_preds(cur, pcs, pus, g_t, image_scales, opts, guidance_scale, pps, **cfg_kw)
            maps.append([self.get_noise_map(cur[k], nxt[k], pcs[k], g_t[k], g_s[k], clip_fn=self.clip_sample, ddim_eta=ddim_eta,
                                            image_scale=image_scales[k], pred_uncond=pus[k], guidance_scale=w)
                         for k in range(len(cur))])
            cur = nxt
            if last != 0:
                nodes.append(cur)
        x_start = self._from_scales(x_start)
        return (x_start, maps, nodes) if return_nodes else (x_start, maps)

    def _checked_step_noise(self, model, x_t, step_noise, rule_rows):
        """``step_noise`` against the trajectory it is replayed on -> one entry per step: the hi -> lo list of maps, or None
        where the step adds no noise"""
        top = x_t[0] if isinstance(x_t, (list, tuple)) else x_t
        B, C, H, W = top.shape
        shapes = [(B, C, H // r, W // r) for r in self._scale_info(model)[0]]
        if len(step_noise) != len(rule_rows):
            raise ValueError("step_noise holds the maps of %d steps, this trajectory has %d (the schedule arguments and t= "
                             "of the noise_maps call?)" % (len(step_noise), len(rule_rows)))
        out = []
        for i, (maps, row) in enumerate(zip(step_noise, rule_rows)):
            if not row[0]:
                out.append(None)
                continue
            maps = _listed(maps)
            if maps is None:
                raise ValueError("step_noise[%d] is None, but step %d of this trajectory adds noise" % (i, i))
            if len(maps) != len(shapes) or any(not torch.is_tensor(m) or tuple(m.shape) != s for m, s in zip(maps, shapes)):
                raise ValueError("step_noise[%d]: wanted %d maps of the shapes %s (got %s)"
                                 % (i, len(shapes), shapes, [tuple(m.shape) if torch.is_tensor(m) else type(m).__name__ for m in maps]))
            out.append(list(maps))
        return out

    def _sample(self, model, x_t, lm_outputs, lm_mask, micros, return_sequence=False, use_beta_tilde=False, t=-1,
                num_inference_steps=2000, ddim_eta=None, guidance_scale=1, resample_steps=False, disable_bar=True,
                yield_output=False, solver=None, known_images=None, known_mask=None, resample=1, known_seed=0,
                known_noise_fn=None, solver_noise_fn=None, step_noise=None, **post_args):
        """``guide``, ``pag_scale`` / ``pag_layers``, ``regions`` / ``region_layers``, ``freeu``, ``cfg``, ``tiles``: see
        ``SampleOptions``; they are taken out of the keywords here (``sample`` has checked them), the rest goes to ``_postprocess``.
        ``known_images`` / ``known_mask``: hold a region of the trajectory on a given image.  After every reverse step,
        whichever update made it, every scale's x_s is replaced where the mask is 1 by the known image diffused to that
        scale's target gamma (``known_blend``; the last step goes to gamma = 1: the known region of the result IS the known
        image).  ``resample = r > 1`` (RePaint's jumps of length 1): every step but the last is taken r times, with the
        forward transition s -> t (``jump``) in between, so that the free region can follow the known one --
        (n - 1) r + 1 denoiser calls.  The noise of both comes from ``known_seed`` (see ``KnownRegion``).  One top-scale
        tensor each, or hi -> lo lists for a nested model (``[None, low]``: super-resolution of a given image).
        ``solver_noise_fn(x)``: with an ``SASolver`` of tau > 0, the noise of every launch that adds some (called per scale,
        hi -> lo) instead of the device generator / ``torch.randn_like``.
        ``step_noise``: the noise maps of ``noise_maps`` -- one entry per step of THIS trajectory (same schedule arguments
        and ``t=``), each a hi -> lo list of tensors shaped like that scale's x_t, or None where the step adds no noise (the
        last).  The ancestral step (``solver=None``; DDPM, or DDIM with ``ddim_eta > 0``) gets ``step_noise[i][k]`` as its
        ``input_noise``: no generator is read or advanced.  With ``x_t`` = the ``x_start`` of ``noise_maps`` and its
        conditioning the trajectory passes through that call's noisy copies of the image, whatever the guidance scale and
        the threshold function; another conditioning edits the image.  None: no bit changes."""
        assert not (yield_output and return_sequence)
        opts = SampleOptions.pop(post_args)
        rule = _checked_rule(solver, ddim_eta, opts, known_images, resample)
        _check_step_noise(step_noise, solver, ddim_eta, resample)
        if known_mask is not None and known_images is None:
            raise ValueError("known_mask without known_images")
        if not resample_steps:
            num_inference_steps = self.n_steps
        steps_host = self.set_timesteps(num_inference_steps)
        if t > -1:
            steps_host = steps_host[steps_host <= t]
        steps = torch.from_numpy(steps_host).to(self.gammas.device)
        # the rule's row of every step, counted from the first step of THIS trajectory, wherever it starts
        rule_rows = rule.rows(self, steps_host[:-1], steps_host[1:] if resample_steps else steps_host[:-1] - 1)
        if step_noise is not None:
            step_noise = self._checked_step_noise(model, x_t, step_noise, rule_rows)
        known = None
        if known_images is not None:
            known = self._known_region(model, x_t, known_images, known_mask, known_seed, known_noise_fn)
        seq = [x_t] if return_sequence else []
        x0 = extra = None
        history = {}   # the rule's entries (``StepRule.store``); cfg: the momentum buffers ("cfg_run")
        rows = None    # tiles: the window count and the conditioning repeated per window, the same for every step
        if opts.tiles is not None:
            top = x_t[0] if isinstance(x_t, (list, tuple)) else x_t
            T = opts.tiles.check(*top.shape[2:], self._scale_info(model)[0]).count(*top.shape[2:])
            rows = T, model_rows(opts, guidance_scale, top.shape[0], T, lm_outputs, lm_mask, micros)
        for i, ts in enumerate(steps[:-1]):
            reps = resample if i < len(steps) - 2 else 1
            for rep in range(reps):
                x0, x_t, extra = self._step(
                    model, ts, x_t, lm_outputs, lm_mask, micros, opts, rule, rule_rows[i], steps[i + 1] if resample_steps else ts - 1,
                    guidance_scale, return_details=True, solver_state=history, rows=rows, noise_fn=solver_noise_fn,
                    step_noise=None if step_noise is None else step_noise[i])
                if known is not None:
                    xs = self._to_scales(model, x_t)
                    B = xs[0].shape[0]
                    g_s = self._scale_gammas(model, steps[i + 1], B)
                    xs = known.blend(xs, g_s)
                    if rep < reps - 1:
                        xs = known.jump(xs, self._scale_gammas(model, ts, B), g_s)
                    x_t = self._from_scales(xs)
            if yield_output:
                yield self._postprocess(x_t, x0, extra, **post_args)
            if return_sequence:
                seq.append(self._postprocess(x_t))
        if return_sequence:
            seq[-1] = torch.clip(seq[-1], -1, 1)
            yield seq
        else:
            yield self._postprocess(x_t, x0, extra, clip=True, **post_args)

    def _postprocess(self, x_t, x0=None, extra=None, yield_full=False, clip=False, image_scale=None, **unused):
        scale = self._config.rescale_signal if image_scale is None else image_scale
        if scale:
            x0 = x0 * scale if x0 is not None else x0
            x_t = x_t * scale
        if clip:
            x_t = torch.clip(x_t, -1, 1)
        return (x0, x_t, extra) if yield_full else x_t


class NestedSampler(Sampler):
    """Multi-resolution variant: lists of images, highest resolution first (reference :612-793)."""

    def get_gammas(self, gamma, scales, images=None):
        if not self._config.schedule_shifted:
            return [gamma for _ in scales]
        return [self.get_schedule_shifted(gamma, s) for s in scales]

    def _signal(self, x, s):
        return x if self._config.schedule_shifted else self.get_image_rescaled(x, s)

    def _scale_info(self, model):
        scales = model.vision_model.nest_ratio + [1]
        return [scales[0] // s for s in scales], [1 if self._config.schedule_shifted else s for s in scales]

    def _gammas_of_scales(self, model, gamma):
        return self.get_gammas(gamma, model.vision_model.nest_ratio + [1])

    def _noisy_step(self, time_step, last):
        return time_step != 1   # (:700)

    def _to_scales(self, model, x_t):
        if not isinstance(x_t, torch.Tensor):
            return x_t
        # first step: draw independent noise at every lower resolution (:669-676)
        return [x_t] + [torch.randn_like(F.avg_pool2d(x_t, r)) for r in self._scale_info(model)[0][1:]]

    def _from_scales(self, xs):
        return xs

    def get_xt(self, x0, eps, g, scales):
        return [Sampler.get_xt(self, self._signal(x, s), e, gi) for x, s, e, gi in zip(x0, scales, eps, g)]

    def get_prediction_targets(self, x0, eps, g, g_last, scales, prediction_type=None):
        return [Sampler.get_prediction_targets(self, self._signal(x, s), e, gi, gl, prediction_type)
                for x, s, e, gi, gl in zip(x0, scales, eps, g, g_last)]

    def forward_model(self, model, x_t, t, lm_outputs, lm_mask, micros={}, guidance_scale=1):
        pcs, pus, _, _ = self._forward_model_raw(model, x_t, t, lm_outputs, lm_mask, micros, guidance_scale)
        return [pc if pu is None else pu + guidance_scale * (pc - pu) for pc, pu in zip(pcs, pus)]

    def _call_model(self, model, xs, t, lm_outputs, lm_mask, micros):
        """(:777-790); the nested model takes and returns lists, and no extras"""
        return list(model(xs, t, lm_outputs, lm_mask, micros)), None

    def _postprocess(self, x_t, x0=None, extra=None, yield_full=False, clip=False, output_inner=False, **unused):
        scales = [1 if self._config.schedule_shifted else x.size(-1) / x_t[-1].size(-1) for x in x_t]
        one = lambda i: Sampler._postprocess(self, x_t[i], x0[i] if x0 is not None else None, extra,
                                             yield_full=yield_full, clip=clip, image_scale=scales[i], **unused)
        out = one(0)
        if not output_inner:
            return out
        outs = [out] + [one(i) for i in range(1, len(x_t))]
        up = lambda x, size: F.interpolate(x, tuple(size), mode="bilinear")   # (H, W): a canvas need not be square
        if not yield_full:
            return torch.cat([up(o, outs[0].shape[-2:]) for o in outs[::-1]], -1)
        a, b, e = zip(*outs)
        return (torch.cat([up(v, a[0].shape[-2:]) for v in a[::-1]], -1),
                torch.cat([up(v, b[0].shape[-2:]) for v in b[::-1]], -1), e[-1])
