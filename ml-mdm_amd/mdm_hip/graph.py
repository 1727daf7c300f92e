"""hipGraph replay for sampling.

Sampling is hundreds of strictly sequential denoiser calls on fixed shapes (reference samplers.py:516-578).  At small
batch the ~1500 kernel launches of one call are host-bound (Python + launch, whatever the GPU needs), so:

``GraphedDenoiser``   the model forward alone as a graph (drop-in wrapper around the vision model: the eager sampler
                      keeps driving it).
``GraphedSampler``    ONE WHOLE DENOISE ITERATION as a graph -- per-step schedule lookup, denoiser forward (with the
                      text conditioning hoisted out of the loop: it does not depend on t), the fused reverse-step
                      kernel of every scale (guidance combine, x0, clip, DDPM / DDIM update, in-kernel noise), the
                      step-counter and RNG advance -- replayed ``num_inference_steps`` times with no host work in
                      between.  All per-step values live in device tables indexed by a device-side counter.

Inference only (no autograd through a replay); parameters must not change between replays -- call ``reset()`` after
loading a checkpoint (the packed kernel-layout weights baked into the graph would be stale otherwise).  Attaching, detaching,
merging or unmerging LoRA adapters (``mdm_hip.lora``) changes what a forward launches: both classes
drop their graphs when ``ops.adapter_epoch()`` has moved, so the next call captures anew instead of replaying a stale one.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops, regions as _regions
from . import tiling as _tiling
from .samplers import (SASolver, SampleOptions, _check_known, _check_solver, _solver_of, gather_windows, merge_windows,
                       model_rows, repeat_rows, split_rows)
from .unet import switch_state, switchable


class GraphedDenoiser(nn.Module):
    """The model forward as one hipGraph per input signature (and per perturbed-row pattern of perturbed-attention
    guidance).  While any attention layer carries a cross-attention bias handle (``regions.applied``: regional prompts,
    token weights) the model is called EAGERLY: the bias tensors belong to the caller, who may rewrite or replace them
    between calls, so no graph is captured with them -- and a graph captured without the bias is never replayed."""

    def __init__(self, model: nn.Module, warmup: int = 2):
        super().__init__()
        self.model = model
        self._warmup = warmup
        self._graphs = {}
        self._adapter_epoch = ops.adapter_epoch()
        self._switchable = switchable(model)

    # attributes the diffusion / sampler code reads from the vision model
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__("model"), name)

    def reset(self):
        self._graphs.clear()

    @staticmethod
    def _sig(x_t, times, cond, mask):
        xs = x_t if isinstance(x_t, (list, tuple)) else [x_t]
        return (tuple(tuple(x.shape) for x in xs), isinstance(x_t, (list, tuple)), tuple(times.shape), times.dtype,
                None if cond is None else tuple(cond.shape), None if mask is None else tuple(mask.shape),
                torch.is_autocast_enabled(), xs[0].device.index)

    def forward(self, x_t, times, conditioning=None, cond_mask=None, micros={}):
        if torch.is_grad_enabled() or self.model.training or micros:
            return self.model(x_t, times, conditioning, cond_mask, micros)
        switches = switch_state(self._switchable)
        if any(h is not None for h in switches["_cross_bias"]):
            return self.model(x_t, times, conditioning, cond_mask, micros)
        if ops.adapter_epoch() != self._adapter_epoch:   # LoRA adapters attached / detached / merged / unmerged since
            self._graphs.clear()
            self._adapter_epoch = ops.adapter_epoch()
        # (+ the perturbed rows of perturbed-attention guidance, layer by layer, and the FreeU switch of every block: they
        # change what a forward launches)
        key = self._sig(x_t, times, conditioning, cond_mask) + (switches["_pag_rows"], switches["_freeu"])
        ent = self._graphs.get(key)
        is_list = isinstance(x_t, (list, tuple))
        xs = list(x_t) if is_list else [x_t]
        if ent is None:
            static_x = [x.clone() for x in xs]
            static_t = times.clone()
            static_c = conditioning.clone() if conditioning is not None else None
            static_m = cond_mask.clone() if cond_mask is not None else None
            arg_x = static_x if is_list else static_x[0]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):   # warm-up: packs weights, sets kernel attributes, sizes the allocator
                for _ in range(self._warmup):
                    self.model(arg_x, static_t, static_c, static_m, {})
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self.model(arg_x, static_t, static_c, static_m, {})
            ent = (graph, static_x, static_t, static_c, static_m, static_out)
            self._graphs[key] = ent
        graph, static_x, static_t, static_c, static_m, static_out = ent
        for s, x in zip(static_x, xs):
            s.copy_(x)
        static_t.copy_(times)
        if static_c is not None:
            static_c.copy_(conditioning)
        if static_m is not None:
            static_m.copy_(cond_mask)
        graph.replay()
        if isinstance(static_out, (list, tuple)):
            return [o.clone() for o in static_out]
        return static_out.clone()


class GraphedSampler:
    """``Diffusion.sample`` / ``NestedDiffusion.sample`` with one hipGraph replay per denoise step.

    Semantics are those of ``Sampler._sample`` with ``resample_steps=True`` (reference samplers.py:516-609, 655-713):
    DDPM (``ddim_eta=None``) or DDIM(eta), classifier-free guidance, CLIP / NONE / DYNAMIC / DYNAMIC_IF thresholding (the
    dynamic ones: x0 kernel -> ``ops.abs_quantile``, a radix select of five launches whose workspace -- 35 KB per sample --
    lives in the graph's pool, -> update kernel, all inside the graph; no sort), or ``solver="dpmpp_2m"``
    (DPM-Solver++(2M): deterministic, the x0 history of every scale lives in a static buffer that the step kernel updates
    in place, the order flag of each step comes from a device table), or ``solver=SASolver(...)`` / ``"sa"`` (SA-Solver: the
    gate {predictor order, corrector order, tau, tau of the step before} of every step and the times of the two steps before
    come from device tables, h0 / h1 / psum of every scale live in static buffers the step kernel updates in place; with
    tau == 0 nothing is drawn and the generator is never touched, with tau > 0 every row draws from it and advances it, the
    gate deciding whether the noise is added -- as the DDPM path does with its noise gate).  The ancestral noise comes
    from the library's counter-based generator (``ops.DeviceRng``, replayable on the host); the START noise is drawn
    like the eager path (CPU generator for the top scale, reference diffusion.py:177), or passed in.

    Image conditioning as in ``Sampler._sample``: ``known_images`` / ``known_mask`` live in static buffers and the body
    ends with the blend kernel of every scale that has one, drawing from a second static generator; ``resample = r > 1``
    repeats every row of the iteration tables but the last r times and ends the body with the jump kernel of every scale,
    gated by a device table (1 on all but the last row of a group).  ``start_step`` starts the replay at the first row
    whose time is <= it (the SDEdit start; ``start_noise`` then carries the noised image).  Without known images and
    with resample == 1 the captured graph has no launch more than before.

    ``cfg=CFG(...)`` (projected / rescaled guidance, ``mdm_hip/guidance.py``): the body runs the combine kernels of every
    scale on every row, gated by two device tables -- the interval gate (off: the conditional prediction passes through bit
    for bit) and the history gate of the momentum (off up to and on the first guided row of the call: the static momentum
    buffers are then not read, so what a warm-up pass or an earlier call left in them is never seen)."""

    def __init__(self, pipeline, warmup: int = 2, seed: int = 0):
        self.pipe = pipeline
        self.sampler = pipeline.sampler
        self._warmup = warmup
        self._seed = seed
        self._graphs = {}
        self._adapter_epoch = ops.adapter_epoch()

    def reset(self):
        self._graphs.clear()

    # ---- host-side schedule ------------------------------------------------------------------------------
    def _tables(self, n_steps, device, resample=1):
        steps = self.sampler.set_timesteps(n_steps)                 # n+1 entries, descending, last = 0
        t, s = steps[:-1], steps[1:]
        gate = self.sampler._noisy_step(t, s)   # the last step adds no noise
        mk = lambda a, dt: torch.as_tensor(a.copy()).to(device=device, dtype=dt)
        # dpmpp_2m: the time of the step before (step 0 has none: its own, never used) and the order gate -- second order
        # wherever there is history and a finite step in log-SNR, i.e. not on the first and not on the last step
        # (0, 1, ..., 1, 0; all zeros for n <= 2)
        p = np.concatenate((t[:1], t[:-1]))
        order = np.zeros(len(t), dtype="float32")
        order[1:-1] = (p[1:-1] > t[1:-1])
        # resample = r: every row but the last r times; the jump gate is on wherever the same row follows
        reps = np.full(len(t), int(resample))
        reps[-1] = 1
        jump = np.ones(int(reps.sum()), dtype="float32")
        jump[np.cumsum(reps) - 1] = 0
        t, s, gate, p, order = (np.repeat(a, reps) for a in (t, s, gate, p, order))
        return (mk(t, torch.long), mk(s, torch.long), mk(gate.astype("float32"), torch.float32), mk(p, torch.long),
                mk(order, torch.float32), mk(jump, torch.float32)), t

    def _build(self, key, xs, cond, mask, n_steps, ddim_eta, guidance, micros, solver, known, resample, opts, names,
               bias_source):
        """``opts``: the call's ``SampleOptions``, with what ``sample`` resolved of them for this model: ``names``, its
        ``layer_names``, and the caller's bias handle (None without ``regions``)"""
        smp = self.sampler
        cfg = opts.cfg_at(guidance)
        model = self.pipe.get_model()
        vm = model.vision_model
        dev = xs[0].device
        B = xs[0].shape[0]
        ratios, image_scales = smp._scale_info(model)
        # tiles: every block of the model batch holds the T windows of every image (cond, mask and micros came repeated)
        tiles = opts.tiles
        canvases = [tuple(x.shape[2:]) for x in xs]
        T = 1 if tiles is None else tiles.count(*canvases[0])
        (tab_t, tab_s, tab_gate, tab_p, tab_order, tab_jump), t_host = self._tables(n_steps, dev, resample)
        idx = torch.zeros(1, dtype=torch.long, device=dev)
        rng = ops.DeviceRng(self._seed, dev)
        # known-region sampling: static image / mask per scale that has one, and a generator of its own
        kn_img = kn_mask = kn_inv = kn_rng = None
        if known is not None:
            kn_img = [None if k is None else k.clone() for k in known.images]
            kn_mask = [None if m is None else m.clone() for m in known.masks]
            kn_inv, kn_rng = known.inv_scales, ops.DeviceRng(0, dev)
        x_static = [x.clone() for x in xs]
        # dpmpp_2m: the x0 of the step before, per scale.  Read only where the order gate is on, so what a warm-up pass or
        # an earlier sample() call left in it is never seen: step 0 (gate off) rewrites it
        x0_prev = [torch.zeros_like(x) for x in xs] if solver == "dpmpp_2m" else None
        # an SASolver: h0 / h1 / psum per scale, updated in place by the step kernel and read only where the gate's orders
        # are on; the gate {predictor order, corrector order, tau, tau of the step before} of every row (sample() fills the
        # rows it replays; until then first order without corrector, what the warm-up passes run with) and the time two
        # steps back.  Noise is drawn from the generator, and the generator advanced, only if the solver's tau > 0
        sa = solver if isinstance(solver, SASolver) else None
        sa_bufs = tab_sa = tab_p1 = None
        if sa is not None:
            top = max(sa.predictor, sa.corrector)
            sa_bufs = dict(h0=[torch.zeros_like(x) for x in xs],
                           h1=[torch.zeros_like(x) if top >= 3 else None for x in xs],
                           psum=[torch.zeros_like(x) if sa.corrector >= 1 else None for x in xs])
            tab_sa = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * len(t_host), dtype=torch.float32, device=dev)
            tab_p1 = torch.as_tensor(np.concatenate((t_host[:1], t_host[:1], t_host[:-2]))[:len(t_host)].copy()).to(dev)
        # cfg: the momentum history per scale and the two gate tables, one row per replay; sample() fills the tables for
        # the rows it replays.  Until then: guidance on, no history -- what the warm-up passes (row 0) run with
        cfg_state = cfg_run_gate = cfg_w_gate = None
        if cfg is not None:
            cfg_state = {"cfg_run": [torch.zeros_like(x) for x in xs]} if cfg.momentum != 0 else {}
            cfg_run_gate = torch.zeros(len(t_host), dtype=torch.float32, device=dev)
            cfg_w_gate = torch.ones(len(t_host), dtype=torch.float32, device=dev)
        micros_s = {k: v.clone() for k, v in micros.items()}   # micro-conditioning ([B] per key, diffusion.py:136-141): static inputs
        # the text path (lm_proj, masked mean, cond_emb) does not depend on t: computed once per sample() call into
        # static buffers, outside the per-step graph
        ce, cs, cm = vm.forward_conditioning(cond, mask)
        ce_s, cs_s, cm_s = ce.clone(), cs.clone(), (cm.clone() if cm is not None else None)
        out_scale = model._output_scale
        # regional prompts: static bias buffers, one per attention resolution -- the warm-up passes discover the resolutions
        # (each buffer starts as a copy of the caller's bias); every sample() call fills them anew
        bias_s = _regions.StaticBias(bias_source) if bias_source is not None else None

        def body():
            t = tab_t.index_select(0, idx)
            s = tab_s.index_select(0, idx)
            gate = tab_gate.index_select(0, idx)
            gammas = lambda time: smp._gammas_of_scales(model, smp.gammas.index_select(0, time).expand(B))
            g_t, g_s = gammas(t), gammas(s)
            history = {}
            if sa is not None:   # x0 goes straight into h0 (the kernel reads its elements of h0 before it writes them)
                history = dict(sa_gate=tab_sa.index_select(0, idx), x0_out=sa_bufs["h0"],
                               sa_state=dict(sa_bufs, g0=gammas(tab_p.index_select(0, idx)),
                                             g1=gammas(tab_p1.index_select(0, idx))))
            elif solver is not None:   # the history lives in x0_prev: the step kernel updates it in place
                history = dict(second_order=tab_order.index_select(0, idx), g_prev=gammas(tab_p.index_select(0, idx)),
                               x0_prev=x0_prev, x0_out=x0_prev)
            times = (t - 1).expand(B)
            # the model's batch: [uncond | cond] under classifier-free guidance, + [perturbed] under perturbed-attention
            # guidance (the static conditioning and micros buffers hold that many rows)
            uncond, pert = opts.blocks(guidance)
            reps = 1 + uncond + pert
            if tiles is None:
                xin, tin = repeat_rows(x_static, times, reps)
            else:   # one gather per scale in place of the repeat; the merge below hands the step whole canvases
                xin, tin = gather_windows(x_static, tiles, ratios, reps), _tiling.time_rows(times, T, reps)
            with opts.switches(vm, guidance, B * T, names=names, bias=bias_s):
                preds = vm.forward_denoising(smp._from_scales(xin), tin, ce_s, cs_s, cm_s, micros_s)
            preds = list(preds) if isinstance(preds, (list, tuple)) else [preds]
            if out_scale != 0:
                preds = [torch.tanh(p / out_scale) * out_scale for p in preds]
            if tiles is not None:
                preds = merge_windows(preds, tiles, ratios, canvases)
            preds, pus, pps = split_rows(preds, uncond, pert)
            # the step of every scale as the eager sampler takes it (dynamic thresholds: x0 kernel -> ops.abs_quantile, the
            # library's radix select, -> update kernel, all captured).  Every row draws and advances the generator in
            # the eager sampler's order (use_device_rng()); the device gate decides whether the noise is added
            if cfg is not None:
                history.update(cfg_state=cfg_state,
                               cfg_gates=(cfg_run_gate.index_select(0, idx), cfg_w_gate.index_select(0, idx)))
            _, x_last = smp._step_scales(x_static, preds, pus, g_t, g_s, image_scales, opts, need_noise=True,
                                         guidance_scale=guidance, ddim_eta=ddim_eta, solver=solver, rng=rng, noise_gate=gate,
                                         pps=pps, **history)
            for x, xl in zip(x_static, x_last):
                x.copy_(xl)
            if known is not None:   # blends hi -> lo, then jumps hi -> lo: the draw order of KnownRegion
                for i, x in enumerate(x_static):
                    if kn_img[i] is not None:
                        ops.sampler_known_blend(x, kn_img[i], kn_mask[i], g_s[i], inv_scale=kn_inv[i], rng=kn_rng, rng_stream=1)
                        kn_rng.advance(x.numel())
                if resample > 1:
                    jump = tab_jump.index_select(0, idx)
                    for i, x in enumerate(x_static):
                        ops.sampler_jump(x, g_t[i], g_s[i], rng=kn_rng, rng_stream=1, gate=jump, out=x)
                        # the eager sampler advances only where it jumps
                        kn_rng.state[1:2].add_((jump != 0).long() * ((x.numel() + 3) // 4))
            idx.add_(1)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up: packs weights, sets kernel attributes, sizes the allocator
            for _ in range(self._warmup):
                idx.zero_()           # every warm-up pass runs step 0 (a 1-step schedule has no step 1 to index)
                body()
            # ... and leaves no trace: the first replay starts at step 0 with the generator at (seed, 0), like the
            # eager sampler after use_device_rng(seed)
            idx.zero_()
            rng.state.copy_(torch.tensor([self._seed & (2**63 - 1), 0], dtype=torch.int64))
            if kn_rng is not None:
                kn_rng.state.zero_()
        torch.cuda.current_stream().wait_stream(side)
        if bias_s is not None:
            bias_s.freeze()   # a resolution first met during the capture would be an allocation inside the graph: an error
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        # everything the graph reads by raw pointer must outlive it: the schedule tables too (they are locals of this
        # function; once freed, a later allocation reuses their memory and the replayed index_select reads garbage
        # indices -> out-of-bounds gather)
        ent = dict(graph=graph, x=x_static, ce=ce_s, cs=cs_s, cm=cm_s, idx=idx, rng=rng, n=len(t_host), micros=micros_s,
                   t_host=t_host, order=tab_order, bias=bias_s, kn_img=kn_img, kn_mask=kn_mask, kn_rng=kn_rng,
                   cfg_run_gate=cfg_run_gate, cfg_w_gate=cfg_w_gate, sa_gate=tab_sa,
                   keep=(tab_t, tab_s, tab_gate, tab_p, tab_order, tab_jump, x0_prev, cfg_state, sa_bufs, tab_p1))
        self._graphs[key] = ent
        return ent

    @torch.no_grad()
    def sample(self, num_examples, sample, image_side, device, num_inference_steps=50, ddim_eta=None, guidance_scale=1,
               start_noise=None, seed=None, solver=None, known_images=None, known_mask=None, resample=1, known_seed=0,
               start_step=None, **options):
        """``options``: the keywords of ``SampleOptions`` (what each does is said there), with these graph-specific facts;
        the key parts are ``SampleOptions.graph_key``, and the body runs the model under ``SampleOptions.switches``.
        ``guide``: refused -- neither the user's function nor the autograd pass of every step can be captured.
        ``cfg``: the graph key holds ("cfg", eta, norm_threshold, momentum, rescale, interval): other values capture anew.
        Each entry owns the momentum buffers and the two gate tables; every call rewrites the tables for the rows it
        replays, so a late start and a second call begin without history, as the eager sampler does.
        ``freeu``: the graph key holds ("freeu", the resolved block names, their b's, their s's, structure): other values
        capture anew.
        ``regions`` / ``region_layers``: each graph entry owns static bias buffers, one per attention resolution, filled by
        ``copy_`` from ``regions`` on every call (the pattern of the known images), and its body hands the switch a handle
        over those buffers.  The graph key holds ("regions", S, ld, the resolved layer names): other masks or weights
        replay the same graph, another S or layer set captures anew.
        ``pag_scale`` / ``pag_layers``: the static conditioning and micros buffers carry the perturbed block's rows and one
        combine kernel per scale precedes the step; the scale and the resolved layer names are part of the graph key.
        ``tiles``: ``image_side`` may be (H, W).  The static conditioning and micros buffers carry every row once per
        window, the body gathers the windows in place of the row repeat and merges the predictions in front of the
        combines and the step (one launch per scale each), and the graph key holds ("tiles", window, stride, blend).
        -> images like ``Diffusion.sample(..., resample_steps=True, num_inference_steps=n, ddim_eta=eta,
        guidance_scale=w, solver=solver)``.  ``start_noise`` (tensor, or hi->lo list for a nested model) replaces the
        drawn x_T.  ``solver="dpmpp_2m"`` draws no noise after x_T (``seed`` has nothing to act on).
        ``known_images`` / ``known_mask`` / ``resample`` / ``known_seed``: as ``Sampler._sample``; whether a scale has a
        known image, and ``resample``, are part of the graph key.  ``start_step=t``: replay only the rows whose time is
        <= t, from ``start_noise`` = the image noised to the first of them (``Diffusion.partial_diffusion(...,
        graphed=self)`` does the noising); the first replayed row of ``dpmpp_2m`` is first order, as in the eager sampler.
        ``solver=SASolver(...)`` (``"sa"``: the defaults): its fields are part of the graph key; every call writes the gate
        table for the rows it replays, counted from its first row, so a late start restarts the orders; with ``tau > 0``
        ``seed`` seeds the noise."""
        opts = SampleOptions(**options)
        if opts.guide is not None:
            raise NotImplementedError("GraphedSampler does not take guide=: loss-guided sampling calls an arbitrary user "
                                      "function and an autograd pass through the denoiser every step, and neither can be "
                                      "captured in a hipGraph; use the eager Sampler.sample(..., guide=...)")
        _check_solver(solver, ddim_eta)
        _check_known(known_images, resample, solver)
        opts.check()
        solver = _solver_of(solver)
        sa = solver if isinstance(solver, SASolver) else None
        if sa is not None:   # a schedule with a repeated time has a step of h = 0: refused before anything is captured
            st = self.sampler.set_timesteps(int(num_inference_steps))
            sa.gates(st[:-1], st[1:], self.sampler.n_steps)
        cfg = opts.cfg_at(guidance_scale)
        if known_mask is not None and known_images is None:
            raise ValueError("known_mask without known_images")
        if start_step is not None and start_noise is None:
            raise ValueError("start_step needs start_noise: the image noised to that step")
        if ops.adapter_epoch() != self._adapter_epoch:
            # LoRA adapters were attached / detached / merged / unmerged since the graphs were captured: what a forward
            # launches, or the weights it reads, changed -- stale like after a checkpoint load, so capture anew
            self._graphs.clear()
            self._adapter_epoch = ops.adapter_epoch()
        self.pipe.eval()
        smp = self.sampler
        model = self.pipe.get_model()
        if start_noise is None:
            x = self.pipe.get_noise(num_examples, model.input_channels, image_side, device)   # an int, or (H, W)
            # independent noise at every lower resolution (:669-676)
            xs = [x] + [torch.randn(num_examples, x.shape[1], x.shape[2] // r, x.shape[3] // r, device=x.device)
                        for r in smp._scale_info(model)[0][1:]]
        else:
            xs = [t.to(device).float() for t in (start_noise if isinstance(start_noise, (list, tuple)) else [start_noise])]
        cond, mask = sample["lm_outputs"], sample["lm_mask"]
        if guidance_scale != 1:
            assert xs[0].shape[0] * 2 == cond.shape[0], "classifier-free guidance: lm_outputs = [uncond | cond]"
        # micro-conditioning the sample carries (scale, watermark_score, ...), as Diffusion.sample passes it on
        # (reference diffusion.py:194-196); one value per row of the model's batch (2B under guidance)
        micros = {k: torch.as_tensor(v, device=xs[0].device).reshape(-1).float()
                  for k, v in self.pipe.get_micro_conditioning(sample).items()}
        regions = opts.regions
        if regions is not None and (regions.rows != xs[0].shape[0] or regions.S != cond.shape[1]):
            raise ValueError("regions over %d rows of %d tokens for a batch of %d images with %d tokens"
                             % (regions.rows, regions.S, xs[0].shape[0], cond.shape[1]))
        names = opts.layer_names(model.vision_model)
        # the perturbed block repeats the conditional rows of everything per-row; tiles repeat every row once per window
        T = 1
        if opts.tiles is not None:
            T = opts.tiles.check(*xs[0].shape[2:], smp._scale_info(model)[0]).count(*xs[0].shape[2:])
        if opts.pag_scale != 0 or opts.tiles is not None:
            cond, mask, micros = model_rows(opts, guidance_scale, xs[0].shape[0], T, cond, mask, micros)
        key = (tuple(tuple(x.shape) for x in xs), tuple(cond.shape), int(num_inference_steps), ddim_eta, float(guidance_scale),
               torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None,
               ops.fp32_split_enabled(),   # a captured graph keeps the arithmetic it was captured with
               tuple(sorted((k, tuple(v.shape)) for k, v in micros.items())), solver)
        known = None
        if known_images is not None:
            known = smp._known_region(model, xs, known_images, known_mask, known_seed, None)
            key = key + (tuple(k is not None for k in known.images), int(resample))
        key = key + opts.graph_key(model.vision_model, guidance_scale, names)
        bias_source = None if regions is None else regions.rows_for(*opts.blocks(guidance_scale), xs[0].device)
        ent = self._graphs.get(key) or self._build(key, xs, cond, mask, int(num_inference_steps), ddim_eta, float(guidance_scale), micros,
                                                   solver, known, int(resample), opts, names, bias_source)
        if bias_source is not None:
            ent["bias"].fill(bias_source)
        for sx, x in zip(ent["x"], xs):
            sx.copy_(x)
        if known is not None:
            for dst, src in zip(ent["kn_img"] + ent["kn_mask"], known.images + known.masks):
                if dst is not None:
                    dst.copy_(src)
            ent["kn_rng"].state.copy_(torch.tensor([known_seed & (2**63 - 1), 0], dtype=torch.int64))
        for k, v in micros.items():
            ent["micros"][k].copy_(v)
        ce, cs, cm = model.vision_model.forward_conditioning(cond, mask)
        ent["ce"].copy_(ce)
        ent["cs"].copy_(cs)
        if ent["cm"] is not None:
            ent["cm"].copy_(cm)
        first = 0
        if start_step is not None:
            rows = np.nonzero(ent["t_host"] <= start_step)[0]
            if start_step < 0:
                raise ValueError("start_step = %r is below every step of the schedule" % (start_step,))
            first = int(rows[0]) if len(rows) else ent["n"]   # t = 0: nothing left to replay
        ent["idx"].fill_(first)
        if cfg is not None:
            # the interval gate of every row, and the history gate: on from the row after the first guided one of this call
            w_on = np.asarray([cfg.on(t, smp.n_steps) for t in ent["t_host"]], dtype="float32")
            seen = np.concatenate(([0.0], np.cumsum(w_on[first:])[:-1])) if first < ent["n"] else np.zeros(0)
            run_on = np.zeros(ent["n"], dtype="float32")
            run_on[first:] = seen > 0
            ent["cfg_w_gate"].copy_(torch.from_numpy(w_on))
            ent["cfg_run_gate"].copy_(torch.from_numpy(run_on))
        if sa is not None and first < ent["n"]:
            # the gate of every row this call replays, counted from its first row: a late start restarts the orders
            th = ent["t_host"]
            gates = np.zeros((ent["n"], 4), dtype="float32")
            gates[:, 0] = 1
            gates[first:] = sa.gates(th[first:], np.concatenate((th[1:], [0]))[first:], smp.n_steps)
            ent["sa_gate"].copy_(torch.from_numpy(gates))
        if seed is not None:
            ent["rng"].state.copy_(torch.tensor([seed & (2**63 - 1), 0], dtype=torch.int64))
        # dpmpp_2m from a late start: there is no history at the first replayed row -- its order gate is off for this call
        order_row = ent["order"][first:first + 1] if (solver == "dpmpp_2m" and first > 0) else None
        if order_row is not None:
            saved = order_row.clone()
            order_row.zero_()
        for _ in range(ent["n"] - first):
            ent["graph"].replay()
        if order_row is not None:
            order_row.copy_(saved)
        out = [x.clone() for x in ent["x"]]
        return smp._postprocess(smp._from_scales(out), clip=True)
