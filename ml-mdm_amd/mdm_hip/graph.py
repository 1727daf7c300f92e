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

from . import attn_maps as _attn_maps, ops, regions as _regions
from . import tiling as _tiling
from .samplers import (SampleOptions, _check_step_noise, _checked_rule, gather_windows, merge_windows, model_rows, repeat_rows,
                       split_rows)
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
        # (a recorder: the caller's too; an attention control: its tables and gates are the caller's as well)
        if any(h is not None for h in switches["_cross_bias"] + switches["_attn_rec"] + switches["_attn_ctrl"]):
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


def _predict(smp, vm, opts, guidance, names, xs, times, cond_s, micros_s, out_scale, bias_s=None, rec_s=None, tiled=None,
             ctrl_s=None):
    """The denoiser call of a graph body: the vision model ``vm`` on the static images ``xs`` (hi -> lo) at ``times`` [B], with
    the static conditioning ``cond_s`` = (cond_emb, cond_states, cond_mask) and micros -> (conditional predictions,
    unconditional ones or Nones, perturbed ones or None), one entry per scale.  The model's batch: [uncond | cond] under
    classifier-free guidance, + [perturbed] under perturbed-attention guidance (the static conditioning and micros buffers
    hold that many rows), under ``opts.switches`` with the body's static bias / recorder / attention-control handles.  ``tiled`` = (tiles,
    ratios, canvases, T): one gather per scale in place of the row repeat, one merge behind the model -- whole canvases out."""
    uncond, pert = opts.blocks(guidance)
    reps = 1 + uncond + pert
    T = 1
    if tiled is None:
        xin, tin = repeat_rows(xs, times, reps)
    else:
        tiles, ratios, canvases, T = tiled
        xin, tin = gather_windows(xs, tiles, ratios, reps), _tiling.time_rows(times, T, reps)
    with opts.switches(vm, guidance, xs[0].shape[0] * T, names=names, bias=bias_s, rec=rec_s, ctrl=ctrl_s):
        preds = vm.forward_denoising(smp._from_scales(xin), tin, *cond_s, micros_s)
    preds = list(preds) if isinstance(preds, (list, tuple)) else [preds]
    if out_scale != 0:
        preds = [torch.tanh(p / out_scale) * out_scale for p in preds]
    if tiled is not None:
        preds = merge_windows(preds, tiles, ratios, canvases)
    return split_rows(preds, uncond, pert)


class GraphedSampler:
    """``Diffusion.sample`` / ``NestedDiffusion.sample`` with one hipGraph replay per denoise step.

    Semantics are those of ``Sampler._sample`` with ``resample_steps=True`` (reference samplers.py:516-609, 655-713):
    DDPM (``ddim_eta=None``) or DDIM(eta), classifier-free guidance, CLIP / NONE / DYNAMIC / DYNAMIC_IF thresholding (the
    dynamic ones: x0 kernel -> ``ops.abs_quantile``, a radix select of five launches whose workspace -- 35 KB per sample --
    lives in the graph's pool, -> update kernel, all inside the graph; no sort), or any other ``solver=``: the update rule
    is a ``samplers.StepRule``, whose rows (noise gate, order gate, SA gate) and the times of the nodes it reads gammas of
    are device tables and whose history lives in static buffers that the step kernel updates in place.  Noise after x_T
    comes from the library's counter-based generator (``ops.DeviceRng``, replayable on the host): a rule that draws
    advances it on every row and its row decides whether the noise is added; one that never draws never touches it.
    The START noise is drawn like the eager path (CPU generator for the top scale, reference diffusion.py:177), or passed in.

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
    def _tables(self, n_steps, device, resample, rule):
        """-> device tables (time, target time, jump gate, the ``rule.history`` earlier nodes' times, the rule's rows), host times"""
        steps = self.sampler.set_timesteps(n_steps)                 # n+1 entries, descending, last = 0
        mk = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        # resample = r: every row but the last r times; the jump gate is on wherever the same row follows
        reps = np.full(n_steps, int(resample))
        reps[-1] = 1
        jump = np.ones(int(reps.sum()), dtype="float32")
        jump[np.cumsum(reps) - 1] = 0
        t, s = np.repeat(steps[:-1], reps), np.repeat(steps[1:], reps)
        # the node j steps back (a rule with history takes no resample); before the first: its own time, never read
        prev = [mk(np.concatenate((np.repeat(t[:1], j), t))[:len(t)], torch.long) for j in range(1, rule.history + 1)]
        return (mk(t, torch.long), mk(s, torch.long), mk(jump, torch.float32), prev,
                mk(rule.rows(self.sampler, t, s), torch.float32)), (t, s)

    def _build(self, key, xs, cond, mask, n_steps, guidance, micros, rule, known, resample, opts, names, bias_source,
               step_noise=False):
        """``rule``: the call's ``StepRule``; ``opts``: its ``SampleOptions``, with what ``sample`` resolved of them for this
        model: ``names``, its ``layer_names``, and the caller's bias handle (None without ``regions``); ``step_noise``: the
        body hands the step the call's noise maps"""
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
        (tab_t, tab_s, tab_jump, tab_prev, tab_rule), (t_host, s_host) = self._tables(n_steps, dev, resample, rule)
        idx = torch.zeros(1, dtype=torch.long, device=dev)
        rng = ops.DeviceRng(self._seed, dev)
        # known-region sampling: static image / mask per scale that has one, and a generator of its own
        kn_img = kn_mask = kn_inv = kn_rng = None
        if known is not None:
            kn_img = [None if k is None else k.clone() for k in known.images]
            kn_mask = [None if m is None else m.clone() for m in known.masks]
            kn_inv, kn_rng = known.inv_scales, ops.DeviceRng(0, dev)
        x_static = [x.clone() for x in xs]
        # step_noise: the maps of every row, [rows, B, C, H, W] per scale; the body hands the step row ``idx`` of each as its
        # noise.  sample() fills the rows it replays (zeros where a step has no map: its gate is 0 anyway)
        noise_tab = [torch.zeros(len(t_host), *x.shape, dtype=torch.float32, device=dev) for x in xs] if step_noise else None
        # the rule's history, updated in place by the step kernel and read only where its row says there is some: what a
        # warm-up pass or an earlier call left is never seen.  ``tab_rule`` holds the full schedule's rows until a call
        # writes those it replays; the warm-up passes run row 0
        state = rule.buffers(x_static)
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
        # cross-attention maps: static accumulators, one per attention resolution, found by the warm-up passes too, and the
        # table of gates, one row per replay; sample() zeroes the former and fills the latter.  Until then: every row records
        rec_s = rec_gate = None
        if opts.attn_maps is not None:
            rec_s = _attn_maps.StaticRows(opts.attn_maps.rows_for(*opts.blocks(guidance), dev))
            rec_gate = torch.ones(len(t_host), dtype=torch.float32, device=dev)
        # attention control: static copies of M, D and the row tables (a handle of this entry's own, not the one the eager
        # samplers share), and the two gate tables, one row per replay; sample() fills M, D and the tables.  Until then:
        # both gates on -- what the warm-up passes run with
        ctrl_s = ctrl_gc = ctrl_gs = None
        if opts.control is not None and opts.control.R > 0:
            ctrl_s = opts.control.rows_for(*opts.blocks(guidance), dev, cached=False)
            ctrl_gc = torch.ones(len(t_host), dtype=torch.float32, device=dev)
            ctrl_gs = torch.ones(len(t_host), dtype=torch.float32, device=dev)

        def body():
            t = tab_t.index_select(0, idx)
            s = tab_s.index_select(0, idx)
            row = tab_rule.index_select(0, idx)
            gammas = lambda time: smp._gammas_of_scales(model, smp.gammas.index_select(0, time).expand(B))
            g_t, g_s = gammas(t), gammas(s)
            g_hist = [gammas(p.index_select(0, idx)) for p in tab_prev]
            times = (t - 1).expand(B)
            if rec_s is not None:
                rec_s.gate = rec_gate.index_select(0, idx)
            if ctrl_s is not None:
                ctrl_s.gate_c, ctrl_s.gate_s = ctrl_gc.index_select(0, idx), ctrl_gs.index_select(0, idx)
            preds, pus, pps = _predict(smp, vm, opts, guidance, names, x_static, times, (ce_s, cs_s, cm_s), micros_s, out_scale,
                                       bias_s, rec_s, None if tiles is None else (tiles, ratios, canvases, T), ctrl_s)
            # the step of every scale as the eager sampler takes it (dynamic thresholds: x0 kernel -> ops.abs_quantile, the
            # library's radix select, -> update kernel, all captured), drawing in its order (use_device_rng())
            cfg_kw = {} if cfg is None else dict(cfg_state=cfg_state, cfg_gates=(cfg_run_gate.index_select(0, idx),
                                                                                  cfg_w_gate.index_select(0, idx)))
            given = None if noise_tab is None else [tab.index_select(0, idx)[0] for tab in noise_tab]
            _, x_last = smp._step_scales(x_static, preds, pus, g_t, g_s, image_scales, opts, rule, row, state, g_hist,
                                         guidance_scale=guidance, rng=rng, pps=pps, step_noise=given, **cfg_kw)
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
        if rec_s is not None:
            rec_s.freeze()    # the same; and the capture counts the launches of one step per resolution
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        # everything the graph reads by raw pointer must outlive it: the schedule tables too (they are locals of this
        # function; once freed, a later allocation reuses their memory and the replayed index_select reads garbage
        # indices -> out-of-bounds gather)
        ent = dict(graph=graph, x=x_static, ce=ce_s, cs=cs_s, cm=cm_s, idx=idx, rng=rng, n=len(t_host), micros=micros_s,
                   t_host=t_host, s_host=s_host, rows=tab_rule, bias=bias_s, kn_img=kn_img, kn_mask=kn_mask, kn_rng=kn_rng,
                   cfg_run_gate=cfg_run_gate, cfg_w_gate=cfg_w_gate, rec=rec_s, rec_gate=rec_gate, noise=noise_tab,
                   ctrl=ctrl_s, ctrl_gc=ctrl_gc, ctrl_gs=ctrl_gs, keep=(tab_t, tab_s, tab_jump, tab_prev, state, cfg_state))
        self._graphs[key] = ent
        return ent

    def _build_invert(self, key, xs, cond, mask, n_steps, iterations, guidance, micros, opts, names, bias_source):
        """The graph of ``invert``: ONE denoiser call at a static iterate plus the invert kernel of every scale, replayed
        K n times.  Device tables, one row per replay: the time of the cleaner node s the step starts from, the time of
        the node t it goes to (the time the model is handed, plus one), and a gate that is 1 on a step's last iteration,
        where the iterate becomes the next step's x_s."""
        smp = self.sampler
        model = self.pipe.get_model()
        vm = model.vision_model
        dev = xs[0].device
        B = xs[0].shape[0]
        nodes = smp.set_timesteps(n_steps)[::-1]                     # ascending from 0
        mk = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        s_host, t_host = np.repeat(nodes[:-1], iterations), np.repeat(nodes[1:], iterations)
        last_host = np.zeros(len(t_host), dtype="float32")
        last_host[iterations - 1::iterations] = 1
        tab_s, tab_t, tab_last = mk(s_host, torch.long), mk(t_host, torch.long), mk(last_host, torch.float32)
        idx = torch.zeros(1, dtype=torch.long, device=dev)
        x_static = [x.clone() for x in xs]   # x_s, the node the step starts from
        y_static = [x.clone() for x in xs]   # the iterate y^j: what the model sees, and what the invert kernel writes
        micros_s = {k: v.clone() for k, v in micros.items()}
        ce, cs, cm = vm.forward_conditioning(cond, mask)
        cond_s = (ce.clone(), cs.clone(), cm.clone() if cm is not None else None)
        out_scale = model._output_scale
        bias_s = _regions.StaticBias(bias_source) if bias_source is not None else None
        rec_s = rec_gate = None
        if opts.attn_maps is not None:   # records on a step's last iteration, inside the recorder's interval: invert() fills the gates
            rec_s = _attn_maps.StaticRows(opts.attn_maps.rows_for(*opts.blocks(guidance), dev))
            rec_gate = torch.ones(len(t_host), dtype=torch.float32, device=dev)

        def body():
            s, t, last = tab_s.index_select(0, idx), tab_t.index_select(0, idx), tab_last.index_select(0, idx)
            gammas = lambda time: smp._gammas_of_scales(model, smp.gammas.index_select(0, time).expand(B))
            g_s, g_t = gammas(s), gammas(t)
            if rec_s is not None:
                rec_s.gate = rec_gate.index_select(0, idx)
            preds, pus, _ = _predict(smp, vm, opts, guidance, names, y_static, (t - 1).expand(B), cond_s, micros_s, out_scale,
                                     bias_s, rec_s)
            for k, (x, y) in enumerate(zip(x_static, y_static)):
                # the kernel reads x_s and the predictions and writes the iterate, which the model is done with
                smp.get_inverted_xt(x, preds[k], g_s[k], g_t[k], pred_uncond=pus[k], guidance_scale=guidance, out=y)
                x.copy_(torch.where(last != 0, y, x))   # the gate SELECTS: off, x_s keeps its bits
            idx.add_(1)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up: packs weights, sets kernel attributes, sizes the allocator
            for _ in range(self._warmup):
                idx.zero_()
                body()
            idx.zero_()
        torch.cuda.current_stream().wait_stream(side)
        if bias_s is not None:
            bias_s.freeze()
        if rec_s is not None:
            rec_s.freeze()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        ent = dict(graph=graph, x=x_static, y=y_static, ce=cond_s[0], cs=cond_s[1], cm=cond_s[2], idx=idx, micros=micros_s,
                   t_host=t_host, last_host=last_host, nodes=nodes, bias=bias_s, rec=rec_s, rec_gate=rec_gate,
                   keep=(tab_s, tab_t, tab_last))
        self._graphs[key] = ent
        return ent

    @torch.no_grad()
    def invert(self, images, sample, device, iterations=1, num_inference_steps=50, t=None, guidance_scale=1, **options):
        """``Sampler.invert(..., resample_steps=True)`` -- DDIM inversion with fixed-point refinement -- with one hipGraph
        replay per denoiser call: K n of them (``_build_invert``), to the eager result bit for bit.  -> (x_t at the noisiest
        node reached, a hi -> lo list for a nested model; that node's time).  ``t``: stop at the first node <= t -- the
        same graph, fewer replays.  ``options``: those ``Sampler.invert`` takes (``regions`` / ``region_layers``, ``freeu``,
        ``attn_maps``), with the static buffers and the graph-key parts they have in ``sample``; the key also holds
        "invert" and K."""
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError("invert: iterations = %r (wanted an int >= 1)" % (iterations,))
        smp = self.sampler
        opts = smp._inversion_options("GraphedSampler.invert", dict(options),
                                      ("guide", "map_guide", "tiles", "known_images", "cfg", "pag"))
        if ops.adapter_epoch() != self._adapter_epoch:   # as sample(): LoRA adapters moved since the graphs were captured
            self._graphs.clear()
            self._adapter_epoch = ops.adapter_epoch()
        self.pipe.eval()
        model = self.pipe.get_model()
        n = int(num_inference_steps)
        nodes = smp._inversion_nodes("invert", n, True, t)[::-1]
        pyr, image_scales = smp._image_scales(model, images.to(device))
        xs = [x if sc == 1 else x / sc for x, sc in zip(pyr, image_scales)]
        cond, mask = sample["lm_outputs"], sample["lm_mask"]
        if guidance_scale != 1:
            assert xs[0].shape[0] * 2 == cond.shape[0], "classifier-free guidance: lm_outputs = [uncond | cond]"
        micros = {k: torch.as_tensor(v, device=xs[0].device).reshape(-1).float()
                  for k, v in self.pipe.get_micro_conditioning(sample).items()}
        regions, maps = opts.regions, opts.attn_maps
        for what, o in (("regions", regions), ("attn_maps", maps)):
            if o is not None and (o.rows != xs[0].shape[0] or o.S != cond.shape[1]):
                raise ValueError("%s over %d rows of %d tokens for a batch of %d images with %d tokens"
                                 % (what, o.rows, o.S, xs[0].shape[0], cond.shape[1]))
        names = opts.layer_names(model.vision_model)
        key = (("invert", int(iterations)), tuple(tuple(x.shape) for x in xs), tuple(cond.shape), n, float(guidance_scale),
               torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None,
               ops.fp32_split_enabled(), tuple(sorted((k, tuple(v.shape)) for k, v in micros.items())))
        key = key + opts.graph_key(model.vision_model, guidance_scale, names)
        bias_source = None if regions is None else regions.rows_for(*opts.blocks(guidance_scale), xs[0].device)
        ent = self._graphs.get(key) or self._build_invert(key, xs, cond, mask, n, int(iterations), float(guidance_scale), micros,
                                                          opts, names, bias_source)
        if bias_source is not None:
            ent["bias"].fill(bias_source)
        for sx, sy, x in zip(ent["x"], ent["y"], xs):
            sx.copy_(x)
            sy.copy_(x)
        for k, v in micros.items():
            ent["micros"][k].copy_(v)
        ce, cs, cm = model.vision_model.forward_conditioning(cond, mask)
        ent["ce"].copy_(ce)
        ent["cs"].copy_(cs)
        if ent["cm"] is not None:
            ent["cm"].copy_(cm)
        replays = (len(nodes) - 1) * int(iterations)
        if maps is not None:
            rec_on = ent["last_host"] * np.asarray([maps.on(tt, smp.n_steps) for tt in ent["t_host"]], dtype="float32")
            ent["rec_gate"].copy_(torch.from_numpy(rec_on))
            ent["rec"].zero()
        ent["idx"].zero_()
        for _ in range(replays):
            ent["graph"].replay()
        if maps is not None:
            ent["rec"].flush(maps, int(rec_on[:replays].sum()))
        out = [x.clone() for x in ent["x"]]
        return smp._from_scales(out), int(nodes[-1])

    @torch.no_grad()
    def sample(self, num_examples, sample, image_side, device, num_inference_steps=50, ddim_eta=None, guidance_scale=1,
               start_noise=None, seed=None, solver=None, known_images=None, known_mask=None, resample=1, known_seed=0,
               start_step=None, step_noise=None, **options):
        """``options``: the keywords of ``SampleOptions`` (what each does is said there), with these graph-specific facts;
        the key parts are ``SampleOptions.graph_key``, and the body runs the model under ``SampleOptions.switches``.
        ``guide``, ``map_guide``: refused -- neither the user's function nor the autograd pass of a guided step can be captured.
        ``cfg``: the graph key holds ("cfg", eta, norm_threshold, momentum, rescale, interval): other values capture anew.
        Each entry owns the momentum buffers and the two gate tables; every call rewrites the tables for the rows it
        replays, so a late start and a second call begin without history, as the eager sampler does.
        ``freeu``: the graph key holds ("freeu", the resolved block names, their b's, their s's, structure): other values
        capture anew.
        ``regions`` / ``region_layers``: each graph entry owns static bias buffers, one per attention resolution, filled by
        ``copy_`` from ``regions`` on every call (the pattern of the known images), and its body hands the switch a handle
        over those buffers.  The graph key holds ("regions", S, ld, the resolved layer names): other masks or weights
        replay the same graph, another S or layer set captures anew.
        ``attn_maps``: each graph entry owns static accumulators, one per attention resolution, zeroed at the start of every
        call outside the graph, and a table of gates, one per row, that the call fills from ``attn_maps.interval``: a row
        outside it launches the same kernel, which returns before it loads anything.  After the last replay the accumulators
        are copied into ``attn_maps``.  The graph key holds ("attn_maps", S, ld, the resolved layer names).
        ``control``: each graph entry owns static copies of M, D and the row tables (``attn_control.BatchCtrl``) and two gate
        tables, one row per replay, that every call fills from the control's intervals (M and D by ``copy_``).  The graph key
        holds ("control", S, ld, source, self_max_queries, the resolved layer names): other ``mapper`` / ``keep`` / ``scale`` /
        interval values replay the same graph.  A control whose rows are all sources adds nothing to the key or the graph.
        ``pag_scale`` / ``pag_layers``: the static conditioning and micros buffers carry the perturbed block's rows and one
        combine kernel per scale precedes the step; the scale and the resolved layer names are part of the graph key.
        ``tiles``: ``image_side`` may be (H, W).  The static conditioning and micros buffers carry every row once per
        window, the body gathers the windows in place of the row repeat and merges the predictions in front of the
        combines and the step (one launch per scale each), and the graph key holds ("tiles", window, stride, blend).
        -> images like ``Diffusion.sample(..., resample_steps=True, num_inference_steps=n, ddim_eta=eta,
        guidance_scale=w, solver=solver)``.  ``start_noise`` (tensor, or hi->lo list for a nested model) replaces the
        drawn x_T.
        ``known_images`` / ``known_mask`` / ``resample`` / ``known_seed``: as ``Sampler._sample``; whether a scale has a
        known image, and ``resample``, are part of the graph key.  ``start_step=t``: replay only the rows whose time is
        <= t, from ``start_noise`` = the image noised to the first of them (``Diffusion.partial_diffusion(...,
        graphed=self)`` does the noising).  ``solver=``: ``rule.key`` is part of the graph key (an ``SASolver``: its fields); every
        call writes the rule's rows from its first replayed row on, counted from it: a late start restarts the orders.
        ``step_noise=maps`` (``Sampler.noise_maps``; as ``Sampler._sample``, which says what is refused): the maps live in a
        static [rows, B, C, H, W] table per scale, filled by ``copy_`` on every call, and the body hands the step row ``idx``
        of each table as its noise, so the generator is neither read nor advanced.  The graph key gains a "step_noise" flag:
        other map values replay the same graph.  The tables hold rows x the size of x_t in fp32 -- about 0.67 GB for 50
        steps of one nested-1024 image (3 x (1024^2 + 256^2 + 64^2) floats per row), per image of the batch."""
        opts = SampleOptions(**options)
        if opts.guide is not None:
            raise NotImplementedError("GraphedSampler does not take guide=: loss-guided sampling calls an arbitrary user "
                                      "function and an autograd pass through the denoiser every step, and neither can be "
                                      "captured in a hipGraph; use the eager Sampler.sample(..., guide=...)")
        if opts.map_guide is not None:
            raise NotImplementedError("GraphedSampler does not take map_guide=: attention-map guidance calls an arbitrary "
                                      "user function and an autograd pass through the denoiser in every guided step, and "
                                      "neither can be captured in a hipGraph; use the eager Sampler.sample(..., map_guide=...)")
        rule = _checked_rule(solver, ddim_eta, opts.check(), known_images, resample)
        _check_step_noise(step_noise, solver, ddim_eta, resample)
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
        maps = opts.attn_maps
        if maps is not None and (maps.rows != xs[0].shape[0] or maps.S != cond.shape[1]):
            raise ValueError("attn_maps over %d rows of %d tokens for a batch of %d images with %d tokens"
                             % (maps.rows, maps.S, xs[0].shape[0], cond.shape[1]))
        control = opts.control if (opts.control is not None and opts.control.R > 0) else None
        if opts.control is not None and (opts.control.rows != xs[0].shape[0] or opts.control.S != cond.shape[1]):
            raise ValueError("control over %d rows of %d tokens for a batch of %d images with %d tokens"
                             % (opts.control.rows, opts.control.S, xs[0].shape[0], cond.shape[1]))
        names = opts.layer_names(model.vision_model)
        # the perturbed block repeats the conditional rows of everything per-row; tiles repeat every row once per window
        T = 1
        if opts.tiles is not None:
            T = opts.tiles.check(*xs[0].shape[2:], smp._scale_info(model)[0]).count(*xs[0].shape[2:])
        if opts.pag_scale != 0 or opts.tiles is not None:
            cond, mask, micros = model_rows(opts, guidance_scale, xs[0].shape[0], T, cond, mask, micros)
        key = (tuple(tuple(x.shape) for x in xs), tuple(cond.shape), int(num_inference_steps), rule.key, float(guidance_scale),
               torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None,
               ops.fp32_split_enabled(),   # a captured graph keeps the arithmetic it was captured with
               tuple(sorted((k, tuple(v.shape)) for k, v in micros.items())))
        known = None
        if known_images is not None:
            known = smp._known_region(model, xs, known_images, known_mask, known_seed, None)
            key = key + (tuple(k is not None for k in known.images), int(resample))
        key = key + opts.graph_key(model.vision_model, guidance_scale, names)
        if step_noise is not None:   # checked against the rows this call replays, before anything is captured
            steps = smp.set_timesteps(int(num_inference_steps))
            kept = steps[:-1] <= (steps[0] if start_step is None else start_step)
            step_noise = smp._checked_step_noise(model, xs, step_noise, rule.rows(smp, steps[:-1][kept], steps[1:][kept]))
            key = key + (("step_noise",),)
        bias_source = None if regions is None else regions.rows_for(*opts.blocks(guidance_scale), xs[0].device)
        ent = self._graphs.get(key) or self._build(key, xs, cond, mask, int(num_inference_steps), float(guidance_scale), micros,
                                                   rule, known, int(resample), opts, names, bias_source, step_noise is not None)
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
        if maps is not None:
            rec_on = np.asarray([maps.on(t, smp.n_steps) for t in ent["t_host"]], dtype="float32")
            ent["rec_gate"].copy_(torch.from_numpy(rec_on))
            ent["rec"].zero()
        if control is not None:
            ent["ctrl"].fill(control)
            g = np.asarray([control.gates(t, smp.n_steps) for t in ent["t_host"]], dtype="float32").reshape(-1, 2)
            ent["ctrl_gc"].copy_(torch.from_numpy(np.ascontiguousarray(g[:, 0])))
            ent["ctrl_gs"].copy_(torch.from_numpy(np.ascontiguousarray(g[:, 1])))
        # the rule's rows of this call, counted from its first row: a late start is a trajectory of its own
        ent["rows"][first:].copy_(torch.from_numpy(rule.rows(smp, ent["t_host"][first:], ent["s_host"][first:])))
        if step_noise is not None:
            for i, z in enumerate(step_noise):
                for k, tab in enumerate(ent["noise"]):
                    tab[first + i].zero_() if z is None else tab[first + i].copy_(z[k])
        if seed is not None:
            ent["rng"].state.copy_(torch.tensor([seed & (2**63 - 1), 0], dtype=torch.int64))
        for _ in range(ent["n"] - first):
            ent["graph"].replay()
        if maps is not None:
            ent["rec"].flush(maps, int(rec_on[first:].sum()))
        out = [x.clone() for x in ent["x"]]
        return smp._postprocess(smp._from_scales(out), clip=True)
