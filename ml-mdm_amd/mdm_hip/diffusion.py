"""Train-step and sampling call surface around the denoiser.

Host-side mirror of ``ml_mdm.diffusion`` (reference ml-mdm-matryoshka/ml_mdm/diffusion.py):
``DiffusionConfig`` (:29-50), ``Model`` (:53-87), ``Diffusion`` (:90-206),
``NestedDiffusionConfig`` (:214-248), ``NestedModel`` (:251-292), ``NestedDiffusion``
(:295-387) -- same names, same ``get_loss(sample)`` / ``sample(num_examples, sample,
image_side, device, **kw)`` signatures and return tuples, so ``trainer.train_batch``
(trainer.py:13-96) and the CLIs run against it unchanged.

``get_loss`` accepts optional ``time`` / ``noise_fn`` overrides so a parity test can feed
the same timesteps and noise to both implementations (the reference draws them from the
device RNG, samplers.py:236-241).

Loss-side arithmetic: on GPU tensors the noising ``x_t = sqrt(g) x + sqrt(1-g) eps``
is one kernel per scale, the image pyramid one ``mdm_avgpool`` per level, and prediction-space conversion + target
+ MSE + per-sample mean one differentiable kernel per scale (``ops.diffusion_loss``) -- 4 launches for the 64x64
pipeline where the torch formulation needs ~25.  CPU tensors (host-logic tests against the reference goldens) take
the torch formulation of the same formulas; nothing falls back from the GPU path.
"""
from dataclasses import dataclass, field, replace
from typing import List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, samplers


@dataclass
class DiffusionConfig:
    sampler_config: samplers.SamplerConfig = field(default_factory=samplers.SamplerConfig)
    model_output_scale: float = 0
    use_vdm_loss_weights: bool = True


@dataclass
class NestedDiffusionConfig(DiffusionConfig):
    use_double_loss: bool = False
    multi_res_weights: str = None
    no_use_residual: bool = False
    use_random_interp: bool = False
    mixed_ratio: str = None
    random_downsample: bool = False
    average_downsample: bool = False
    mid_downsample: bool = False


class Model(nn.Module):
    """thin wrapper that owns the vision model (what DDP wraps, clis/train_parallel.py:148)."""

    def __init__(self, vision_model, diffusion_config: DiffusionConfig = None):
        super().__init__()
        self.diffusion_config = diffusion_config or DiffusionConfig()
        self._output_scale = self.diffusion_config.model_output_scale
        self.vision_model = vision_model
        self.sampler = None

    def set_sampler(self, sampler):
        self.sampler = sampler

    def load(self, vision_file):
        return self.vision_model.load(vision_file)

    def save(self, vision_file, other_items=None):
        self.vision_model.save(vision_file, other_items=other_items)

    @property
    def input_channels(self):
        return self.vision_model.input_channels

    def forward(self, x_t, times, lm_outputs, lm_mask, micros):
        out = self.vision_model(x_t, times, lm_outputs, lm_mask, micros)
        if self._output_scale != 0:
            out = torch.tanh(out / self._output_scale) * self._output_scale
        return out, torch.ones_like(out)


class Diffusion(nn.Module):
    def __init__(self, denoising_model, diffusion_config: DiffusionConfig):
        super().__init__()
        self.model = Model(denoising_model, diffusion_config)
        self.sampler = samplers.Sampler(diffusion_config.sampler_config)
        self.model.set_sampler(self.sampler)
        self._config = diffusion_config
        self.loss_fn = nn.MSELoss(reduction="none")
        # get_loss returns (loss, time, x_t, means, TARGETS, weights) like the reference; the fused GPU loss never
        # forms the target tensor, so it is built only on request (the trainer of this package does not ask)
        self.materialize_targets = True

    def get_model(self):
        return self.model.module if hasattr(self.model, "module") else self.model

    def to(self, device):
        self.model = self.model.to(device)
        self.sampler = self.sampler.to(device)
        return self

    def train(self, mode=True):
        self.model.train(mode)

    def eval(self):
        self.model.eval()
        self.sampler.eval()

    def get_micro_conditioning(self, sample):
        conditions = self.get_model().vision_model.conditions
        return {k: sample[k] for k in conditions if k in sample} if conditions is not None else {}

    def get_pred_for_training(self, x_t, pred, g):
        sc = self._config.sampler_config
        if sc.loss_target_type == sc.prediction_type:
            return pred
        x0, _ = self.sampler.get_x0_eps_from_pred(x_t, pred, g, sc.prediction_type)
        return self.sampler.get_pred_from_x0_xt(x_t, x0, g, sc.loss_target_type)

    def get_loss(self, sample, time=None, noise_fn=torch.randn_like):
        images, lm_outputs, lm_mask = sample["images"], sample["lm_outputs"], sample["lm_mask"]
        eps, g, g_last, weights, time = self.sampler.get_eps_time(images, time, noise_fn)
        if not self._config.use_vdm_loss_weights:
            weights = None
        if images.is_cuda:
            sc = self._config.sampler_config
            inv = 1.0 / sc.rescale_signal if sc.rescale_signal else 1.0
            x_t, eps = ops.noise_images(images.float(), g, eps.float(), inv_scale=inv)
            means, _ = self.model(x_t, time, lm_outputs, lm_mask, self.get_micro_conditioning(sample))
            # the reference builds x_t from the RESCALED images but the target from the raw ones (diffusion.py:153, 163):
            # the target term of the loss kernel gets scale 1 (they differ only for a V-prediction target with rescale_signal)
            loss = ops.diffusion_loss(means, x_t, images.float(), eps, g, sc.prediction_type, sc.loss_target_type, inv_scale=1.0)
            tgt = None
            if self.materialize_targets:
                tgt = self.sampler.get_prediction_targets(images, eps, g, g_last, sc.loss_target_type)
            return loss, time, x_t, means, tgt, weights
        x_t = self.sampler.get_xt(self.sampler.get_image_rescaled(images), eps, g)
        means, _ = self.model(x_t, time, lm_outputs, lm_mask, self.get_micro_conditioning(sample))
        tgt = self.sampler.get_prediction_targets(images, eps, g, g_last, self._config.sampler_config.loss_target_type)
        pred = self.get_pred_for_training(x_t, means, g)
        loss = self.loss_fn(pred, tgt).mean(axis=(1, 2, 3))
        return loss, time, x_t, means, tgt, weights

    def get_noise(self, num_examples, input_channels, image_side, device):
        """``image_side``: an int (a square, as the reference), or (H, W) -- the canvas of tiled sampling"""
        H, W = image_side if isinstance(image_side, (tuple, list)) else (image_side, image_side)
        return torch.randn(num_examples, input_channels, H, W).to(device)  # CPU RNG, as the reference (:177)

    def sample(self, num_examples, sample, image_side, device, **kwargs):
        """keywords go to the sampler's ``sample`` (``guidance_scale``, ``solver``, ``known_images`` ..., and the options of
        ``samplers.SampleOptions``).  ``image_side``: an int, or (H, W) with ``tiles=`` (a nested model's lower-scale start
        noise follows the canvas)"""
        self.eval()
        noise = self.get_noise(num_examples, self.get_model().input_channels, image_side, device)
        return self.sampler.sample(self.get_model(), noise, sample["lm_outputs"], sample["lm_mask"],
                                   self.get_micro_conditioning(sample), **kwargs)

    def partial_diffusion(self, images, t, lm_outputs, lm_mask, device, return_sequence=False, micros={}, seed=0,
                          noise_fn=None, graphed=None, **kwargs):
        """Start a trajectory late, from ``images`` noised to schedule time ``t`` (SDEdit, Meng et al. 2022) -- the mirror
        of the reference's ``Diffusion.partial_diffusion`` (diffusion.py:199-206, dead code there), made to work.  The
        trajectory starts at the first step of the sampling schedule (``resample_steps`` / ``num_inference_steps`` as
        ``sample``) that is <= t, and the images are noised to THAT step's gamma; t = 0 returns clip(images).  A nested
        model gets the average-pooled pyramid with independent noise and its own (shifted) gamma per scale, as
        ``get_loss`` builds it.  GPU tensors: ``ops.noise_images`` per scale, drawn from ``ops.DeviceRng(seed)`` on
        stream 0 and advanced by ``numel`` per scale, hi -> lo; CPU tensors: the torch formula with ``noise_fn``
        (default ``torch.randn_like``).  ``graphed``: a ``GraphedSampler`` of this pipeline -- the remaining steps are
        replayed by it (``start_step``) instead of the eager sampler.  Other keywords go to ``sample`` (``ddim_eta``,
        ``solver``, ``guidance_scale``, ``known_images`` ..., and the options of ``samplers.SampleOptions``)."""
        self.eval()
        smp, model = self.sampler, self.get_model()
        n = kwargs.get("num_inference_steps", 2000) if kwargs.get("resample_steps", False) else smp.n_steps
        steps = smp.set_timesteps(n)
        if not (steps <= t).any():
            raise ValueError("partial_diffusion: t = %r is below every step of the schedule" % (t,))
        t0 = int(steps[steps <= t][0])
        images = images.to(device)
        hip = images.is_cuda
        ratios, image_scales = smp._scale_info(model)
        gammas = smp._scale_gammas(model, t0, images.shape[0])
        pyr = [images.float() if hip else images]
        for r in ratios[1:]:
            pyr.append(ops.avgpool(pyr[0], r) if hip else F.avg_pool2d(pyr[0], r))
        x_t = []
        if hip:
            rng = ops.DeviceRng(seed, images.device)
            for img, g, sc in zip(pyr, gammas, image_scales):
                x_t.append(ops.noise_images(img, g, rng=rng, inv_scale=1.0 / sc if sc else 1.0)[0])
                rng.advance(img.numel())
        else:
            noise_fn = noise_fn or torch.randn_like
            for img, g, sc in zip(pyr, gammas, image_scales):
                x_t.append(samplers.Sampler.get_xt(smp, img / sc if sc else img, noise_fn(img), g))
        nested = isinstance(smp, samplers.NestedSampler)
        if graphed is not None:
            if return_sequence or kwargs.get("yield_output", False):
                raise ValueError("partial_diffusion(graphed=...) returns the final images only")
            kw = {k: v for k, v in kwargs.items() if k not in ("resample_steps", "num_inference_steps")}
            sample = dict(micros, lm_outputs=lm_outputs, lm_mask=lm_mask)
            return graphed.sample(images.shape[0], sample, images.shape[-1], device, num_inference_steps=n, start_noise=x_t,
                                  start_step=t0, **kw)
        return smp.sample(model, x_t if nested else x_t[0], lm_outputs, lm_mask, micros, return_sequence=return_sequence,
                          t=t0, **kwargs)


    def invert(self, images, lm_outputs, lm_mask, device, method="ddim", graphed=None, micros={}, **kwargs):
        """A GIVEN image back to the noise and the trajectory that reproduce it -> an ``Inverted`` for ``sample_from``.
        ``method="ddim"``: DDIM inversion with fixed-point refinement (``Sampler.invert``; ``iterations=`` K); ``graphed``: a
        ``GraphedSampler`` of this pipeline replays the K n denoiser calls.  ``method="ddpm"``: edit-friendly DDPM inversion
        (``Sampler.noise_maps``; ``ddim_eta=``, ``seed=`` / ``noise_fn=``) -- its n - 1 calls are independent and run once,
        eagerly, whatever ``graphed`` says.  Schedule keywords (``num_inference_steps`` / ``resample_steps`` / ``t``) as
        ``sample`` and ``partial_diffusion``; they are kept in the record.  Other keywords go to the sampler's method
        (``guidance_scale`` and the options it takes)."""
        if method not in ("ddim", "ddpm"):
            raise ValueError("invert: method = %r (wanted \"ddim\" or \"ddpm\")" % (method,))
        self.eval()
        smp, model = self.sampler, self.get_model()
        images = images.to(device)
        resample_steps = bool(kwargs.pop("resample_steps", False))
        n = int(kwargs.pop("num_inference_steps", 2000)) if resample_steps else smp.n_steps
        schedule = dict(num_inference_steps=n, resample_steps=True)   # (all of the schedule's steps: the same nodes)
        if method == "ddpm":
            eta = kwargs.pop("ddim_eta", None)
            x_t, maps = smp.noise_maps(model, images, lm_outputs, lm_mask, micros, ddim_eta=eta, **schedule, **kwargs)
            t0 = int(smp._inversion_nodes("invert", n, True, kwargs.get("t"))[0])
            return Inverted("ddpm", x_t, t0, maps, ddim_eta=eta, **schedule)
        if graphed is not None:
            sample = dict(micros, lm_outputs=lm_outputs, lm_mask=lm_mask)
            x_t, t0 = graphed.invert(images, sample, device, num_inference_steps=n, **kwargs)
        else:
            x_t, t0 = smp.invert(model, images, lm_outputs, lm_mask, micros, **schedule, **kwargs)
        return Inverted("ddim", x_t, t0, None, **schedule)

    def sample_from(self, inv, sample, device, graphed=None, **kwargs):
        """Resume from an ``Inverted``: the trajectory from ``inv.x_t`` at time ``inv.t`` on the schedule it was made with --
        DDIM(0) for a DDIM record, the replay of ``inv.step_noise`` (``step_noise=``) under ``inv.ddim_eta`` for a DDPM one.
        With the conditioning and guidance of the inversion: the image again; with another prompt in ``sample``
        (``lm_outputs`` / ``lm_mask`` and the micro-conditioning): its edit.  The late start is ``partial_diffusion``'s:
        ``t=`` of the eager sampler, ``start_step`` / ``start_noise`` of ``graphed``.  Other keywords go to ``sample``."""
        self.eval()
        smp, model = self.sampler, self.get_model()
        kw = dict(kwargs, ddim_eta=0 if inv.method == "ddim" else inv.ddim_eta)
        if inv.step_noise is not None:
            kw["step_noise"] = inv.step_noise
        xs = inv.x_t if isinstance(inv.x_t, (list, tuple)) else [inv.x_t]
        if graphed is not None:
            return graphed.sample(xs[0].shape[0], sample, xs[0].shape[-1], device, num_inference_steps=inv.num_inference_steps,
                                  start_noise=[x.to(device) for x in xs], start_step=inv.t, **kw)
        x_t = [x.to(device) for x in xs] if isinstance(inv.x_t, (list, tuple)) else inv.x_t.to(device)
        return smp.sample(model, x_t, sample["lm_outputs"], sample["lm_mask"], self.get_micro_conditioning(sample), t=inv.t,
                          num_inference_steps=inv.num_inference_steps, resample_steps=inv.resample_steps, **kw)


@dataclass
class Inverted:
    """What ``Diffusion.invert`` found for an image, and what ``Diffusion.sample_from`` needs to resume from it.
    ``method``: "ddim" or "ddpm".  ``x_t``: the start of the trajectory, at schedule time ``t`` (a hi -> lo list for a nested
    model).  ``step_noise``: the noise maps of the DDPM method (``Sampler.noise_maps``), None for DDIM.  The schedule
    arguments it was made with -- the replay must walk the same nodes -- and, for the maps, the ``ddim_eta`` they solve."""
    method: str
    x_t: object
    t: int
    step_noise: object = None
    num_inference_steps: int = None
    resample_steps: bool = True
    ddim_eta: float = None

    def repeat(self, n):
        """-> the record with the rows of ``x_t`` and of every noise map repeated ``n`` times in BLOCK order ([rows | rows |
        ...]): the start of a batch whose first block replays the inverted images -- the sources of
        ``sample_from(..., control=AttnControl(...))`` -- and whose other blocks are their edits under other prompts."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError("Inverted.repeat: n = %r (wanted an int >= 1)" % (n,))
        rep = lambda t: torch.cat([t] * n)
        both = lambda v: None if v is None else ([rep(t) for t in v] if isinstance(v, (list, tuple)) else rep(v))
        noise = None if self.step_noise is None else [both(z) for z in self.step_noise]
        return replace(self, x_t=both(self.x_t), step_noise=noise)


class NestedModel(Model):
    def forward(self, x_t: List[torch.Tensor], times, lm_outputs, lm_mask, micros={}, mixed_ratio=None):
        if not self.diffusion_config.no_use_residual:
            # the reference's residual branch reads an undefined variable (diffusion.py:277-291) and both shipped
            # nested configs disable it (cc12m_256x256.yaml:24, cc12m_1024x1024.yaml:25)
            raise NotImplementedError("NestedModel requires no_use_residual=True")
        batch = x_t[0].size(0)
        if mixed_ratio is not None:  # run the higher resolutions on a prefix of the batch only
            x_t = [x[: int(m * x.size(0))] for x, m in zip(x_t, mixed_ratio)]
        p_t = self.vision_model(x_t, times, lm_outputs, lm_mask, micros)
        if mixed_ratio is not None:
            p_t = [torch.cat([p, p.new_zeros(batch - p.size(0), *p.shape[1:])], 0) for p in p_t]
        return p_t


class NestedDiffusion(Diffusion):
    def __init__(self, denoising_model, diffusion_config: NestedDiffusionConfig):
        nn.Module.__init__(self)
        self.model = NestedModel(denoising_model, diffusion_config)
        self.sampler = samplers.NestedSampler(diffusion_config.sampler_config)
        self.model.set_sampler(self.sampler)
        self._config = diffusion_config
        self.loss_fn = nn.MSELoss(reduction="none")
        self.materialize_targets = True
        self.mixed_ratio = None
        if diffusion_config.mixed_ratio:
            r = np.cumsum(np.asarray([float(x) for x in diffusion_config.mixed_ratio.split(":")]))
            self.mixed_ratio = r / r[-1]

    def get_loss(self, sample, time=None, noise_fn=torch.randn_like):
        images, lm_outputs, lm_mask = sample["images"], sample["lm_outputs"], sample["lm_mask"]
        micros = self.get_micro_conditioning(sample)
        vm = self.get_model().vision_model
        if any(vm.is_temporal):
            raise NotImplementedError("temporal nesting is not implemented")
        scales = vm.nest_ratio + [1]
        ratios = [scales[0] // s for s in scales]

        eps, g, g_last, weights, time = self.sampler.get_eps_time(images, time, noise_fn)
        if not self._config.use_vdm_loss_weights:
            weights = None
        # image pyramid by average pooling; the low-resolution noise is drawn independently (:333-356)
        hip = images.is_cuda
        pyr, noises = [images.float() if hip else images], [eps]
        for i in range(1, len(ratios)):
            rr = ratios[i] // ratios[i - 1]
            pyr.append(ops.avgpool(pyr[-1], rr) if hip else F.avg_pool2d(pyr[-1], rr))
            noises.append(noise_fn(pyr[-1]))
        g = self.sampler.get_gammas(g, scales, pyr)
        g_last = self.sampler.get_gammas(g_last, scales, pyr)
        if hip:
            return self._get_loss_hip(pyr, noises, g, g_last, scales, time, lm_outputs, lm_mask, micros, weights)

        x_t = self.sampler.get_xt(pyr, noises, g, scales)
        p_t = self.model(x_t, time, lm_outputs, lm_mask, micros, self.mixed_ratio)
        tgt = self.sampler.get_prediction_targets(pyr, noises, g, g_last, scales, self._config.sampler_config.loss_target_type)
        pred = [self.get_pred_for_training(x, p, gi) for x, p, gi in zip(x_t, p_t, g)]

        if self._config.multi_res_weights is not None:
            assert self._config.use_double_loss
            w = [float(v) for v in self._config.multi_res_weights.split(":")]
        else:
            w = [1.0] * len(x_t)
        loss = 0
        for i in range(len(x_t)):
            if i == 0 or self._config.use_double_loss:
                li = self.loss_fn(pred[i], tgt[i]).mean(axis=(1, 2, 3))
                if self.mixed_ratio is not None:
                    li = li / self.mixed_ratio[i]
                    li[int(self.mixed_ratio[i] * li.size(0)):] = 0
            else:
                li = pred[i].mean() * 0.0
            loss = loss + li * w[i]
        return loss, time, x_t[0], pred[0], tgt[0], weights

    def _get_loss_hip(self, pyr, noises, g, g_last, scales, time, lm_outputs, lm_mask, micros, weights):
        """GPU tensors: noising and loss are one kernel each per scale (see the module docstring)"""
        sc = self._config.sampler_config
        inv = [1.0 if sc.schedule_shifted else (1.0 / s if s else 1.0) for s in scales]   # NestedSampler._signal
        x_t = [ops.noise_images(x, gi, e.float(), inv_scale=iv)[0] for x, gi, e, iv in zip(pyr, g, noises, inv)]
        p_t = self.model(x_t, time, lm_outputs, lm_mask, micros, self.mixed_ratio)
        if self._config.multi_res_weights is not None:
            assert self._config.use_double_loss
            w = [float(v) for v in self._config.multi_res_weights.split(":")]
        else:
            w = [1.0] * len(x_t)
        loss = 0
        for i in range(len(x_t)):
            if i == 0 or self._config.use_double_loss:
                li = ops.diffusion_loss(p_t[i], x_t[i], pyr[i], noises[i].float(), g[i], sc.prediction_type,
                                        sc.loss_target_type, inv_scale=inv[i])
                if self.mixed_ratio is not None:
                    li = li / self.mixed_ratio[i]
                    li = torch.cat([li[: int(self.mixed_ratio[i] * li.size(0))], li.new_zeros(li.size(0) - int(self.mixed_ratio[i] * li.size(0)))])
            else:
                li = p_t[i].mean() * 0.0
            loss = loss + li * w[i]
        pred0 = tgt0 = None
        if self.materialize_targets:
            tgt0 = samplers.Sampler.get_prediction_targets(self.sampler, self.sampler._signal(pyr[0], scales[0]), noises[0],
                                                           g[0], g_last[0], sc.loss_target_type)
            pred0 = self.get_pred_for_training(x_t[0], p_t[0], g[0])
        return loss, time, x_t[0], pred0, tgt0, weights
