"""Regional prompts and token weights: an additive bias on the logits of the text cross-attention.

"A red car" on the left and "a blue house" on the right, or "(snow:1.4)", are one operation on this model: the text term
of a ``SelfAttention`` layer is a softmax of its own over the S text keys, and a bias b[row, query position, token] added
to its logits before the softmax multiplies the token's unnormalised attention weight by e^b.  With

    b = log(weight of the token) + log(area-mean of the token's region over the pixels of the query position)

a weight w scales a token's share by w, a region of 0 / 1 switches it off / leaves it alone per position, and a feathered
region fades it out smoothly (log 0 = -inf excludes the key exactly as ``lm_mask == 0`` does).  The bias touches the small
L x S pass only: a selected layer with text keys and no attention control calls ``ops.attention(..., bias=b)`` --
``mdm_attn_fwd`` without text keys, then ``mdm_attn_cross_bias`` in place (include/mdm_hip_ext.h; ``ops.attention_biased``
is that call on its own).  Training-free and sampling only: the kernel has no backward.

``RegionPrompts``  the spans of ONE token sequence the caller already has (``lm_outputs`` [rows, S, D], ``lm_mask``) and
                   their regions / weights -> the bias of every attention resolution, cached.
``concat``         per-prompt encoder outputs -> one sequence, its mask and the spans.
``applied``        the switch (``with applied(vision_model, rp, layers): ...``), in the style of ``pag.perturbed``.
The samplers do the rest: ``Sampler.sample(..., regions=rp, region_layers="all")``, ``GraphedSampler.sample`` alike.
"""
import math

import torch
import torch.nn.functional as F

from . import ops, pag
from .unet import switched

NEG_INF = float("-inf")


def _ld(S):
    """row length of a bias over S keys: a lane's four consecutive keys are one 16-byte load"""
    return (int(S) + 3) // 4 * 4


class RegionPrompts:
    """``RegionPrompts(S, image_size, spans, rows)``: a bias over the ``S`` tokens of ``rows`` conditional batch rows.

    ``image_size``: H or (H, W), the resolution the regions are drawn at.  ``spans``: a list of ``(start, stop, region,
    weight)`` over tokens [start, stop) -- ``region``: None (everywhere) or a [rows, 1, H, W] tensor in [0, 1];
    ``weight``: a float > 0, or a [rows, stop - start] tensor >= 0.  Spans must not overlap (ValueError); a token in no
    span has bias 0.  ``device``: where the bias tensors live (default: that of the first tensor among the spans, else
    CPU); a sampler asks for its own device."""

    def __init__(self, S, image_size, spans, rows, device=None):
        self.S, self.rows = int(S), int(rows)
        if self.S < 1 or self.rows < 1:
            raise ValueError("RegionPrompts: S = %d tokens, rows = %d" % (self.S, self.rows))
        hw = (image_size, image_size) if isinstance(image_size, int) else tuple(int(v) for v in image_size)
        if len(hw) != 2 or min(hw) < 1:
            raise ValueError("RegionPrompts: image_size = %r (wanted H or (H, W))" % (image_size,))
        self.image_size = hw
        self.ld = _ld(self.S)
        self._cache = {}   # (layout, h, w, device) -> [len(layout) * rows, h * w, ld]
        self.spans = self._checked(spans)
        self.device = torch.device(device) if device is not None else next(
            (t.device for sp in self.spans for t in sp[2:] if torch.is_tensor(t)), torch.device("cpu"))

    # ---- spans --------------------------------------------------------------------------------------------
    def _checked(self, spans):
        out = []
        for sp in spans:
            if len(sp) != 4:
                raise ValueError("RegionPrompts: a span is (start, stop, region, weight), got %r" % (sp,))
            start, stop, region, weight = sp
            start, stop = int(start), int(stop)
            if not 0 <= start < stop <= self.S:
                raise ValueError("RegionPrompts: span [%d, %d) of %d tokens" % (start, stop, self.S))
            if region is not None:
                if not torch.is_tensor(region) or tuple(region.shape) != (self.rows, 1) + self.image_size:
                    raise ValueError("RegionPrompts: the region of span [%d, %d) is %s (wanted None or a tensor %s)" % (
                        start, stop, tuple(region.shape) if torch.is_tensor(region) else type(region).__name__,
                        (self.rows, 1) + self.image_size))
                if float(region.min()) < 0 or float(region.max()) > 1:
                    raise ValueError("RegionPrompts: the region of span [%d, %d) leaves [0, 1]" % (start, stop))
            if torch.is_tensor(weight):
                if tuple(weight.shape) != (self.rows, stop - start) or float(weight.min()) < 0:
                    raise ValueError("RegionPrompts: the weight of span [%d, %d) is %s (wanted a float > 0 or a tensor %s "
                                     ">= 0)" % (start, stop, tuple(weight.shape), (self.rows, stop - start)))
            elif not (isinstance(weight, (int, float)) and weight > 0 and math.isfinite(weight)):
                raise ValueError("RegionPrompts: the weight of span [%d, %d) is %r (wanted a float > 0 or a tensor >= 0)"
                                 % (start, stop, weight))
            out.append((start, stop, region, weight))
        order = sorted(out, key=lambda s: s[0])
        for a, b in zip(order, order[1:]):
            if b[0] < a[1]:
                raise ValueError("RegionPrompts: spans [%d, %d) and [%d, %d) overlap" % (a[0], a[1], b[0], b[1]))
        return out

    def set_spans(self, spans):
        """Other regions / weights over the same S tokens and rows: every cached bias tensor is rewritten IN PLACE (same
        storage, so whatever holds one -- a handle, a captured graph's source -- sees the new values)."""
        self.spans = self._checked(spans)
        for (layout, h, w, dev), t in self._cache.items():
            t.copy_(self._compute(layout, h, w, dev))
        return self

    # ---- the bias -----------------------------------------------------------------------------------------
    def _pool_ratio(self, h, w):
        H, W = self.image_size
        if h < 1 or w < 1 or H % h or W % w or H // h != W // w:
            raise ValueError("RegionPrompts: image_size %s is not divisible into square pixel blocks by the attention "
                             "resolution (%d, %d)" % (self.image_size, h, w))
        return H // h

    def _cond(self, h, w, device):
        """the conditional rows' bias [rows, h * w, ld]; the columns [S, ld) hold -inf (the kernel never uses them)"""
        r = self._pool_ratio(h, w)
        b = torch.zeros(self.rows, h * w, self.ld, dtype=torch.float32, device=device)
        b[:, :, self.S:] = NEG_INF
        for start, stop, region, weight in self.spans:
            if torch.is_tensor(weight):
                lw = torch.log(weight.to(device=device, dtype=torch.float32))[:, None, :]          # [rows, 1, n]
            else:
                lw = math.log(weight)
            if region is not None:
                reg = region.to(device=device, dtype=torch.float32)
                if r > 1:   # area-mean over the pixel block of a query position
                    reg = ops.avgpool(reg, r) if reg.is_cuda else F.avg_pool2d(reg, r)
                lw = torch.log(reg).reshape(self.rows, h * w, 1) + lw
            b[:, :, start:stop] = lw
        return b

    def _compute(self, layout, h, w, device):
        cond = self._cond(h, w, device)
        if layout == ("cond",):
            return cond
        zero = None
        if "uncond" in layout:   # no regions, no weights: bias 0 (the pad columns as everywhere)
            zero = torch.zeros_like(cond)
            zero[:, :, self.S:] = NEG_INF
        return torch.cat([zero if k == "uncond" else cond for k in layout])

    def layout_of(self, N):
        """the blocks of a batch of N rows: [cond], [uncond | cond] or [uncond | cond | perturbed] (the perturbed block of
        perturbed-attention guidance repeats the conditional rows).  Anything else -- a mixed-resolution nested batch, whose
        low-resolution calls carry other rows -- is a ValueError."""
        lay = {self.rows: ("cond",), 2 * self.rows: ("uncond", "cond"), 3 * self.rows: ("uncond", "cond", "cond")}.get(N)
        if lay is None:
            raise ValueError("RegionPrompts: a batch of %d rows for regions over %d rows (wanted %d, %d = [uncond | cond], or "
                             "%d = [uncond | cond | perturbed]); mixed-resolution nested batches are not supported"
                             % (N, self.rows, self.rows, 2 * self.rows, 3 * self.rows))
        return lay

    def bias(self, N, h, w, layout=None, device=None):
        """-> fp32 [N, h * w, ld], ld = S rounded up to 4: for a token of span i, log(weight) + log(area-mean of region_i
        over the pixel block of position (y, x) of an h x w grid); -inf where either factor is 0; 0 outside every span and
        in unconditional rows.  Cached per (h, w): the same tensor every time, rewritten in place by ``set_spans``."""
        layout = self.layout_of(N) if layout is None else tuple(layout)
        if len(layout) * self.rows != N:
            raise ValueError("RegionPrompts: a batch of %d rows for %d blocks of %d rows; mixed-resolution nested batches "
                             "are not supported" % (N, len(layout), self.rows))
        device = self.device if device is None else torch.device(device)
        key = (layout, int(h), int(w), device)
        t = self._cache.get(key)
        if t is None:
            t = self._cache[key] = self._compute(layout, int(h), int(w), device)
        return t

    def rows_for(self, guidance=False, pag_rows=False, device=None):
        """the handle a sampler hands to ``applied``: this bias for a model batch of [uncond |] cond [| perturbed]"""
        return BatchBias(self, (("uncond",) if guidance else ()) + ("cond",) + (("cond",) if pag_rows else ()), device)


class BatchBias:
    """``RegionPrompts`` with the block layout of the model's batch and the device fixed: what a layer's ``_cross_bias``
    holds during a sampler's denoiser call"""

    def __init__(self, rp, layout, device=None):
        self.rp, self.layout, self.device = rp, tuple(layout), device
        self.S, self.ld, self.rows = rp.S, rp.ld, len(self.layout) * rp.rows

    def bias(self, N, h, w):
        return self.rp.bias(N, h, w, self.layout, self.device)


class StaticBias:
    """A handle over fixed buffers, one per attention resolution (``GraphedSampler``): ``source`` is asked once per
    resolution -- in the warm-up passes -- and its answer CLONED; ``fill(source)`` copies new values into the same buffers,
    which a captured graph reads by address."""

    def __init__(self, source):
        self.S, self.ld, self.rows = source.S, source.ld, source.rows
        self.buffers = {}
        self._source = source

    def bias(self, N, h, w):
        buf = self.buffers.get((h, w))
        if buf is None:
            if self._source is None:
                raise ValueError("StaticBias: no buffer for the attention resolution (%d, %d): the model reached it after the "
                                 "warm-up passes" % (h, w))
            buf = self.buffers[(h, w)] = self._source.bias(N, h, w).clone()
        if buf.shape[0] != N:
            raise ValueError("StaticBias: a batch of %d rows for buffers of %d; mixed-resolution nested batches are not "
                             "supported" % (N, buf.shape[0]))
        return buf

    def freeze(self):
        self._source = None
        return self

    def fill(self, source):
        for (h, w), buf in self.buffers.items():
            buf.copy_(source.bias(buf.shape[0], h, w))


def concat(prompts, uncond=None):
    """Per-prompt encoder outputs -> one token sequence and its spans.

    ``prompts``: a list of ``(lm_outputs [rows, S_i, D], lm_mask [rows, S_i], region, weight)`` (``region`` / ``weight`` as
    in ``RegionPrompts``; a 2-tuple means everywhere, weight 1), concatenated along S in the order given.  ``uncond``:
    ``(lm_outputs [rows, S_u, D], lm_mask [rows, S_u])`` of the unconditional text, or None; the result is then
    [uncond | cond] along the batch, the SHORTER of the two sequences padded to the longer with zero states and
    ``lm_mask`` 0 -- and, where it is the conditional one that is padded, a span of weight 0 (a -inf bias column), which
    excludes the padding also in a model that does not mask its cross attention.
    -> ({"lm_outputs": ..., "lm_mask": ...}, spans): the sample-dict entries, and the spans for ``RegionPrompts(S, ...)``
    with S = ``lm_outputs.shape[1]``.

    What is regional is the spatial cross-attention alone: the pooled text embedding and the LM head
    (``forward_conditioning``) see the WHOLE concatenated sequence, every prompt in every place."""
    if not prompts:
        raise ValueError("concat: no prompts")
    spans, lms, masks, at = [], [], [], 0
    for p in prompts:
        lm, mask = p[0], p[1]
        region, weight = (p[2], p[3]) if len(p) == 4 else (None, 1.0)
        if lm.dim() != 3 or tuple(mask.shape) != tuple(lm.shape[:2]) or lm.shape[0] != prompts[0][0].shape[0] \
                or lm.shape[2] != prompts[0][0].shape[2]:
            raise ValueError("concat: lm_outputs %s with lm_mask %s" % (tuple(lm.shape), tuple(mask.shape)))
        lms.append(lm)
        masks.append(mask.to(lm.dtype) if mask.dtype != lm.dtype else mask)
        spans.append((at, at + lm.shape[1], region, weight))
        at += lm.shape[1]
    lm, mask = torch.cat(lms, dim=1), torch.cat(masks, dim=1)
    if uncond is not None:
        ulm, umask = uncond
        if ulm.shape[0] != lm.shape[0] or ulm.shape[2] != lm.shape[2] or tuple(umask.shape) != tuple(ulm.shape[:2]):
            raise ValueError("concat: unconditional lm_outputs %s with lm_mask %s for prompts %s"
                             % (tuple(ulm.shape), tuple(umask.shape), tuple(lm.shape)))
        S = max(lm.shape[1], ulm.shape[1])
        pad = lambda t, n: t if n == 0 else torch.cat([t, t.new_zeros((t.shape[0], n) + tuple(t.shape[2:]))], dim=1)
        if S > lm.shape[1]:
            spans.append((lm.shape[1], S, None, lm.new_zeros((lm.shape[0], S - lm.shape[1]), dtype=torch.float32)))
        lm = torch.cat([pad(ulm.to(lm.dtype), S - ulm.shape[1]), pad(lm, S - lm.shape[1])])
        mask = torch.cat([pad(umask.to(mask.dtype), S - umask.shape[1]), pad(mask, S - mask.shape[1])])
    return {"lm_outputs": lm, "lm_mask": mask}, spans


def layer_names(vision_model, layers="all"):
    """the layers ``layers`` selects (the vocabulary of ``pag.select``) that HAVE text keys, as a tuple of names"""
    names = tuple(n for n, m in pag.select(vision_model, layers) if m.cond_dim is not None and m.cond_dim > 0)
    if not names:
        raise ValueError("region_layers = %r selects no attention layer with text keys" % (layers,))
    return names


class applied(switched):
    """``with applied(vision_model, rp, layers="all"):`` -- inside, the selected ``SelfAttention`` layers that have text keys
    add ``rp.bias(N, H, W)`` to their text logits (``rp``: a ``RegionPrompts``, or any handle with that method); on exit
    (also by an exception) every layer has what it had before."""

    def __init__(self, vision_model, rp, layers="all"):
        if not callable(getattr(rp, "bias", None)):
            raise ValueError("applied: %r has no bias(N, h, w)" % (rp,))
        super().__init__((vision_model.get_submodule(n), {"_cross_bias": rp}) for n in layer_names(vision_model, layers))


__all__ = ["RegionPrompts", "BatchBias", "StaticBias", "concat", "applied", "layer_names"]
