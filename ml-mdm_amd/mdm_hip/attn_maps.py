"""Cross-attention maps: where every text token attends, recorded while the model runs.

The text term of a ``SelfAttention`` layer is a softmax of its own over the S text keys,

    out = softmax(q k^T) v + softmax(q k_c^T [+ bias]; live keys) v_c,

so its probabilities are an L x S quantity (L = h * w query positions) that the fused kernels never write.  A selected
layer launches ``ops.attn_cross_maps`` (``mdm_attn_cross_maps``, include/mdm_hip_ext.h) after its usual attention call:
the probabilities, mean over heads, accumulated into one fp32 buffer per attention resolution.  The layer's output is
computed exactly as before, so the images do not change by a bit; with ``regions=`` the maps show the BIASED attention.

``AttnMaps``   the accumulators of ``rows`` conditional batch rows over ``S`` tokens, the layer selection, the interval
               of the schedule that records, and what reads them: ``maps()`` per resolution, ``heatmap(size)`` over all.
``record``     the switch for one forward outside the samplers (``with record(vision_model, maps): model(...)``).
``applied``    the switch a sampler holds around its denoiser call, in the style of ``regions.applied``.
``cross_maps`` the kernel restated in torch ops, for CPU tensors.
``cross_probs`` the same probabilities as a DIFFERENTIABLE function of qkv (``ops.attn_cross_probs`` in torch ops).
``GradRows``   the recorder of attention-map guidance (``samplers.MapGuide``): it keeps the maps on the autograd tape.
The samplers do the rest: ``Sampler.sample(..., attn_maps=maps)``, ``GraphedSampler.sample`` alike -- the conditional
block of [uncond | cond | perturbed] is what is recorded.
"""
import math

import torch
import torch.nn.functional as F

from . import ops, pag
from .regions import _ld
from .unet import switched


def cross_maps(qkv, kvc, mask, heads, acc, bias=None, weight=1.0, gate=None, row0=0, rows=None):
    """``ops.attn_cross_maps`` in torch ops (CPU tensors, any float dtype; arithmetic in fp32):
    acc[r - row0, l, s] += weight * gate / heads * sum_h softmax_s(q_h[r, l] . k_c,h[r, s] / sqrt(d) + bias[r, l, s]) over
    the live keys -- mask != 0 and bias > -1e30 --, 0 for a query with none; the columns [S, ld) of ``acc`` untouched."""
    N, S = qkv.shape[0], kvc.shape[1]
    C = qkv.shape[-1] // 3
    L = qkv.numel() // max(N * 3 * C, 1)
    d = C // heads
    rows = N - row0 if rows is None else int(rows)
    w = float(weight) * (1.0 if gate is None else float(gate))
    if w == 0:
        return acc
    sl = slice(row0, row0 + rows)
    with torch.no_grad():
        q = qkv.detach().reshape(N, L, 3 * C)[sl, :, :C].float().reshape(rows, L, heads, d)
        k = kvc.detach()[sl, :, :C].float().reshape(rows, S, heads, d)
        logits = torch.einsum("blhd,bshd->bhls", q, k) / math.sqrt(d)
        live = torch.ones(rows, 1, L, S, dtype=torch.bool, device=q.device)
        if bias is not None:
            b = bias.detach()[sl, :, :S].float()[:, None]
            ok = b > -1e30                      # false for NaN too
            live = live & ok
            logits = logits + torch.where(ok, b, torch.zeros_like(b))
        if mask is not None:
            live = live & (mask.detach()[sl].float() != 0)[:, None, None, :]
        logits = logits.masked_fill(~live, float("-inf"))
        m = logits.amax(dim=-1, keepdim=True).clamp(min=-1e30)
        e = torch.exp(logits - m)
        l = e.sum(dim=-1, keepdim=True)
        p = torch.where(l > 0, e / l.clamp(min=1e-38), torch.zeros_like(e))
        acc[:, :, :S] += (w / heads) * p.sum(dim=1)
    return acc


def cross_probs(qkv, kvc, mask, heads, row0=0, rows=None):
    """``ops.attn_cross_probs`` in torch ops (CPU tensors, any float dtype; arithmetic in fp32) -> fp32 [rows, L, ld], ld = S
    rounded up to 4 with zero pad columns: ``cross_maps`` without ``no_grad`` and without an accumulator, differentiable in
    ``qkv`` by torch autograd; ``kvc`` and ``mask`` are constants."""
    N, S = qkv.shape[0], kvc.shape[1]
    C = qkv.shape[-1] // 3
    L = qkv.numel() // max(N * 3 * C, 1)
    d = C // heads
    rows = N - row0 if rows is None else int(rows)
    sl = slice(row0, row0 + rows)
    q = qkv.reshape(N, L, 3 * C)[sl, :, :C].float().reshape(rows, L, heads, d)
    k = kvc.detach()[sl, :, :C].float().reshape(rows, S, heads, d)
    logits = torch.einsum("blhd,bshd->bhls", q, k) / math.sqrt(d)
    live = torch.ones(rows, 1, L, S, dtype=torch.bool, device=q.device)
    if mask is not None:
        live = live & (mask.detach()[sl].float() != 0)[:, None, None, :]
    logits = logits.masked_fill(~live, float("-inf"))
    m = logits.detach().amax(dim=-1, keepdim=True).clamp(min=-1e30)
    e = torch.exp(logits - m)
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(l > 0, e / l.clamp(min=1e-38), torch.zeros_like(e))
    return F.pad(p.mean(dim=1), (0, _ld(S) - S))


def layer_names(vision_model, layers="all"):
    """the layers ``layers`` selects (the vocabulary of ``pag.select``) that HAVE text keys, as a tuple of names"""
    names = tuple(n for n, m in pag.select(vision_model, layers) if m.cond_dim is not None and m.cond_dim > 0)
    if not names:
        raise ValueError("AttnMaps: layers = %r selects no attention layer with text keys" % (layers,))
    return names


class AttnMaps:
    """``AttnMaps(S, rows, layers="all", interval=None)``: the recorder of ``rows`` conditional batch rows over ``S``
    tokens.  ``layers``: the selectors of ``pag.select`` (a named set, a list of module names, a predicate), of which the
    layers with text keys record.  ``interval = (lo, hi)`` in fractions of ``num_diffusion_steps``: a step records where
    lo <= t / T <= hi for the time t it starts from (as ``CFG.interval``); None: every step.

    One fp32 accumulator [rows, h * w, ld] (ld = S rounded up to 4) per attention resolution (h, w), created on first
    use, and beside it the number of (step, layer) pairs added into it -- counted on the host: the schedule and the layer
    list say it, nothing is read back from the device."""

    def __init__(self, S, rows, layers="all", interval=None):
        self.S, self.rows = int(S), int(rows)
        if self.S < 1 or self.rows < 1:
            raise ValueError("AttnMaps: S = %d tokens, rows = %d" % (self.S, self.rows))
        if interval is not None:
            try:
                lo, hi = interval
                interval = (float(lo), float(hi))
            except (TypeError, ValueError):
                raise ValueError("AttnMaps: interval = %r (wanted (lo, hi) in fractions of the schedule, or None)" % (interval,))
            if not (math.isfinite(interval[0]) and math.isfinite(interval[1]) and interval[0] <= interval[1]):
                raise ValueError("AttnMaps: interval = %r (wanted finite lo <= hi)" % (interval,))
        if not (callable(layers) or isinstance(layers, (str, list, tuple, set, frozenset))):
            raise ValueError("AttnMaps: layers = %r (wanted a named set, a list of module names, or a predicate)" % (layers,))
        self.layers, self.interval = layers, interval
        self.ld = _ld(self.S)
        self._acc = {}     # (h, w) -> fp32 [rows, h * w, ld]
        self._count = {}   # (h, w) -> (step, layer) pairs recorded

    def on(self, time_step, num_diffusion_steps):
        """does the step that starts from ``time_step`` record?"""
        if self.interval is None:
            return True
        return self.interval[0] <= float(time_step) / float(num_diffusion_steps) <= self.interval[1]

    def acc(self, h, w, device):
        """the accumulator of resolution (h, w): zeros on first use; the same tensor every time"""
        key = (int(h), int(w))
        t = self._acc.get(key)
        if t is None:
            t = self._acc[key] = torch.zeros(self.rows, key[0] * key[1], self.ld, dtype=torch.float32, device=device)
            self._count[key] = 0
        elif t.device != torch.device(device):
            raise ValueError("AttnMaps: the accumulator of resolution %s lives on %s, the model runs on %s (reset() first)"
                             % (key, t.device, device))
        return t

    def counted(self, h, w, n=1):
        self._count[(int(h), int(w))] += int(n)

    def counts(self):
        """{(h, w): (step, layer) pairs recorded}"""
        return dict(self._count)

    def reset(self):
        self._acc.clear()
        self._count.clear()
        return self

    def maps(self):
        """-> {(h, w): fp32 [rows, S, h, w]}: the mean over the recorded steps, layers and heads (zeros: nothing recorded)"""
        out = {}
        for (h, w), t in self._acc.items():
            m = t[:, :, :self.S] / max(self._count[(h, w)], 1)
            out[(h, w)] = m.transpose(1, 2).reshape(self.rows, self.S, h, w).contiguous()
        return out

    def heatmap(self, size):
        """-> fp32 [rows, S, H, W]: every resolution upsampled bilinearly to ``size`` (H or (H, W)), averaged weighted by
        its count of recorded (step, layer) pairs"""
        hw = (size, size) if isinstance(size, int) else tuple(int(v) for v in size)
        if len(hw) != 2 or min(hw) < 1:
            raise ValueError("AttnMaps: size = %r (wanted H or (H, W))" % (size,))
        total = sum(self._count.values())
        if total == 0:
            raise ValueError("AttnMaps: nothing recorded")
        out = None
        for key, m in self.maps().items():
            if self._count[key] == 0:
                continue
            up = F.interpolate(m, size=hw, mode="bilinear", align_corners=False) * (self._count[key] / total)
            out = up if out is None else out + up
        return out

    def rows_for(self, guidance=False, pag_rows=False, device=None):
        """the handle a sampler hands to ``applied``: the conditional block of a model batch [uncond |] cond [| perturbed]"""
        return BatchRows(self, self.rows if guidance else 0, (1 + bool(guidance) + bool(pag_rows)) * self.rows)


def _mixed(what, N, rows, total):
    return ValueError("%s: a batch of %d rows for maps over %d rows of a model batch of %d; mixed-resolution nested batches "
                      "are not supported" % (what, N, rows, total))


def _check_tokens(what, S, kvc):
    if kvc.shape[1] != S:
        raise ValueError("%s: maps over %d tokens for text keys of %d" % (what, S, kvc.shape[1]))


class BatchRows:
    """``AttnMaps`` with the recorded block of the model's batch fixed -- rows [row0, row0 + maps.rows) of ``total``: what
    a layer's ``_attn_rec`` holds during an eager denoiser call.  Adds into the ``AttnMaps`` directly and counts there."""

    def __init__(self, maps, row0, total):
        self.maps, self.row0, self.total = maps, int(row0), int(total)
        self.S, self.ld, self.rows = maps.S, maps.ld, maps.rows

    def record(self, qkv, kvc, mask, heads, bias, N, h, w):
        if N != self.total:
            raise _mixed("AttnMaps", N, self.rows, self.total)
        _check_tokens("AttnMaps", self.S, kvc)
        acc = self.maps.acc(h, w, qkv.device)
        fn = ops.attn_cross_maps if qkv.is_cuda else cross_maps
        fn(qkv, kvc, mask, heads, acc, bias=bias, row0=self.row0, rows=self.rows)
        self.maps.counted(h, w)


class StaticRows:
    """A handle over fixed buffers, one per attention resolution (``GraphedSampler``; the pattern of
    ``regions.StaticBias``): allocated in the warm-up passes, zeroed by ``zero()`` at the start of every ``sample()``
    outside the graph, added into by the captured launches -- each gated by ``gate``, a device float[1] the graph body
    reads from its table of steps --, and copied into the ``AttnMaps`` by ``flush`` at the end.  The launches of ONE step
    per resolution are counted during the capture (``freeze()`` starts the count), so the total needs no read-back."""

    def __init__(self, source):
        self.S, self.ld, self.rows = source.S, source.ld, source.rows
        self.row0, self.total = source.row0, source.total
        self.buffers, self.per_step = {}, {}
        self.gate = None
        self._frozen = False

    def record(self, qkv, kvc, mask, heads, bias, N, h, w):
        if N != self.total:
            raise _mixed("StaticRows", N, self.rows, self.total)
        _check_tokens("StaticRows", self.S, kvc)
        buf = self.buffers.get((h, w))
        if buf is None:
            if self._frozen:
                raise ValueError("StaticRows: no buffer for the attention resolution (%d, %d): the model reached it after "
                                 "the warm-up passes" % (h, w))
            buf = self.buffers[(h, w)] = torch.zeros(self.rows, h * w, self.ld, dtype=torch.float32, device=qkv.device)
        ops.attn_cross_maps(qkv, kvc, mask, heads, buf, bias=bias, gate=self.gate, row0=self.row0, rows=self.rows)
        self.per_step[(h, w)] = self.per_step.get((h, w), 0) + 1

    def freeze(self):
        self._frozen = True
        self.per_step = {}   # what follows is the capture: one step
        return self

    def zero(self):
        for buf in self.buffers.values():
            buf.zero_()

    def flush(self, maps, steps):
        """the buffers into ``maps`` (copied where it holds nothing yet, so the bits are the eager sampler's), counted as
        ``steps`` recorded steps"""
        for (h, w), buf in self.buffers.items():
            dst = maps.acc(h, w, buf.device)
            if maps.counts()[(h, w)] == 0:
                dst.copy_(buf)
            else:
                dst.add_(buf)
            maps.counted(h, w, steps * self.per_step.get((h, w), 0))


class GradRows:
    """``GradRows(S, row0, rows, total)``: the recorder of attention-map guidance -- rows [row0, row0 + rows) of a model
    batch of ``total``, over ``S`` tokens.  ``record`` calls the DIFFERENTIABLE op (``ops.attn_cross_probs``; CPU tensors:
    ``cross_probs``) and keeps, per attention resolution, the running sum of what it returned and the layer count, so
    ``maps()`` is attached to the autograd graph of the forward that recorded: a loss on it reaches the model's input.
    One handle serves one forward.  A bias (``regions=``) is refused: the biased map has no backward."""

    def __init__(self, S, row0, rows, total):
        self.S, self.row0, self.rows, self.total = int(S), int(row0), int(rows), int(total)
        if self.S < 1 or self.rows < 1 or self.row0 < 0 or self.row0 + self.rows > self.total:
            raise ValueError("GradRows: S = %d tokens, rows [%d, %d) of a batch of %d"
                             % (self.S, self.row0, self.row0 + self.rows, self.total))
        self.ld = _ld(self.S)
        self._sum = {}     # (h, w) -> fp32 [rows, h * w, ld], on the tape
        self._count = {}   # (h, w) -> layers recorded

    def record(self, qkv, kvc, mask, heads, bias, N, h, w):
        if bias is not None:
            raise NotImplementedError("GradRows: a bias on the text logits (regions=): the biased cross-attention map has no "
                                      "backward (mdm_attn_cross_maps_bwd takes none)")
        if N != self.total:
            raise _mixed("GradRows", N, self.rows, self.total)
        _check_tokens("GradRows", self.S, kvc)
        fn = ops.attn_cross_probs if qkv.is_cuda else cross_probs
        # the text keys are constants of the guidance: trainable adapters of kv_cond (LoRA) get no gradient from the maps
        p = fn(qkv, kvc.detach(), mask, heads, row0=self.row0, rows=self.rows)
        key = (int(h), int(w))
        self._sum[key] = p if key not in self._sum else self._sum[key] + p
        self._count[key] = self._count.get(key, 0) + 1

    def counts(self):
        """{(h, w): layers recorded}"""
        return dict(self._count)

    def maps(self):
        """-> {(h, w): fp32 [rows, S, h, w]}: the mean over the recording layers and the heads, on the autograd tape"""
        out = {}
        for (h, w), t in self._sum.items():
            m = t[:, :, :self.S] / self._count[(h, w)]
            out[(h, w)] = m.transpose(1, 2).reshape(self.rows, self.S, h, w)
        return out


class applied(switched):
    """``with applied(vision_model, handle, layers="all"):`` -- inside, the selected ``SelfAttention`` layers that have text
    keys call ``handle.record(...)`` after their attention (``handle``: a ``BatchRows`` / ``StaticRows`` / ``GradRows``, or
    anything with that method); on exit (also by an exception) every layer has what it had before."""

    def __init__(self, vision_model, handle, layers="all"):
        if not callable(getattr(handle, "record", None)):
            raise ValueError("applied: %r has no record(qkv, kvc, mask, heads, bias, N, h, w)" % (handle,))
        super().__init__((vision_model.get_submodule(n), {"_attn_rec": handle}) for n in layer_names(vision_model, layers))


def record(vision_model, maps, layers=None):
    """``with record(vision_model, maps):`` -- the same switch for a single forward outside the samplers (a training or
    evaluation step): every row of the batch is recorded (``maps.rows`` of them), in ``layers`` (default: ``maps.layers``)."""
    if not isinstance(maps, AttnMaps):
        raise ValueError("record: %r (wanted a mdm_hip.AttnMaps)" % (maps,))
    return applied(vision_model, BatchRows(maps, 0, maps.rows), maps.layers if layers is None else layers)


__all__ = ["AttnMaps", "BatchRows", "StaticRows", "GradRows", "applied", "record", "cross_maps", "cross_probs", "layer_names"]
