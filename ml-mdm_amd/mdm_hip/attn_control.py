"""Prompt-to-prompt attention control (Hertz et al., "Prompt-to-Prompt Image Editing with Cross Attention Control", 2022):
an EDITED row of the batch computes with the attention maps of its SOURCE row, so the edit keeps the source's layout.

The model batch is [uncond | cond | perturbed]; control acts on the conditional block, whose rows are [sources | edits].
For an edited row r with source s, at a controlled layer, per head h:

    out_h[r] = A_h(g_s ? s : r) v_h[r]  +  P_h(s) V'_h[r]  +  P_h(r) V''_h[r]
    V'[r][i, :]  = g_c sum_{j live in r} M_r[i, j] v_c[r][j, :]          M_r[i, j] = scale[r][j] mapper[r][i, j]
    V''[r][j, :] = (g_c D_r[j] + 1 - g_c) v_c[r][j, :]                   D_r[j]    = scale[r][j] keep[r][j]

A = the self-attention map, P = the text cross-attention probabilities (a softmax of its own over the S text keys, so mixing
it over the token axis is linear in v_c: (P M) v_c = P (M v_c)); g_c, g_s: the gates of the step (``cross_interval``,
``self_interval``; g_s also needs L <= ``self_max_queries``).  A selected layer takes this split path for its edited rows in
EVERY step -- only the gates change, and they are device values -- so one captured graph serves a trajectory and the eager and
the graphed sampler issue the same launches.  Outside the intervals an edited row therefore agrees with the uncontrolled
sampler to rounding, not bit for bit.  Sources, unselected layers and the other two blocks take the ordinary launch: a
selected layer calls ``ops.attention(..., ctrl_rows=rows)``, whose block table is ``ops._attn_blocks``
(``ops.attention_controlled`` is that call on its own).

``AttnControl``  sources, alignment (``mapper``), ``keep``, ``scale``, intervals and layers; ``AttnControl.aligned`` builds the
                 matrices from token pairs.  The project ships no tokenizer: alignments are token indices.
``BatchCtrl``    the control with the block layout of the model batch and the device fixed: the tables the kernels read.
``applied``      the switch (``with applied(vision_model, handle, control): ...``), in the style of ``regions.applied``.
``mix_kv`` / ``gather_qkv``  the two kernels restated in torch ops, for CPU tensors.
The samplers do the rest: ``Sampler.sample(..., control=ctl)``, ``GraphedSampler.sample`` alike.  Sampling only: no backward.
"""
import math

import torch

from . import pag
from .regions import _ld
from .unet import switched


def _interval(what, value):
    try:
        lo, hi = value
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("AttnControl: %s = %r (wanted (lo, hi) in fractions of the schedule)" % (what, value))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("AttnControl: %s = %r (wanted finite lo <= hi)" % (what, value))
    return lo, hi


def _layers(what, value):
    if not (callable(value) or isinstance(value, (str, list, tuple, set, frozenset))):
        raise ValueError("AttnControl: %s = %r (wanted a named set, a list of module names, or a predicate)" % (what, value))
    return value


class AttnControl:
    """``AttnControl(S, source, mapper=None, keep=None, scale=None, ...)``: control over the ``len(source)`` conditional
    batch rows and their ``S`` text tokens.

    ``source[r] == r``: row r is a source; otherwise r is an edit of the source row ``source[r]``.  All sources come before
    all edits (ValueError otherwise): rows [0, G) are sources, [G, B) edits.  Per edited row r -- given as a dict {r: tensor}
    or a list of B entries with None where the default is meant --
    ``mapper[r]`` fp32 [S, S], row = source token, column = edit token (default: identity); ``keep[r]`` fp32 [S] (default 0):
    how much of the edit's OWN attention to token j stays; ``scale[r]`` fp32 [S] (default 1).  Word swap / replace: identity
    mapper, keep 0; refine: a partial permutation, keep 1 on the new tokens; reweight: scale.
    ``cross_interval`` / ``self_interval``: (lo, hi) in fractions of ``num_diffusion_steps`` by the time a step starts from
    (as ``CFG.interval``, ``AttnMaps.interval``): lo <= t / T <= hi.  ``cross_layers`` / ``self_layers``: the vocabulary of
    ``pag.select``; of the former the layers with text keys count.  ``self_max_queries``: self-attention maps are shared
    only in layers of at most this many queries."""

    def __init__(self, S, source, mapper=None, keep=None, scale=None, cross_interval=(0.2, 1.0), self_interval=(0.6, 1.0),
                 cross_layers="all", self_layers="all", self_max_queries=1024):
        self.S = int(S)
        if self.S < 1:
            raise ValueError("AttnControl: S = %d tokens" % self.S)
        try:
            source = [s for s in source]
        except TypeError:
            raise ValueError("AttnControl: source = %r (wanted a list of row indices)" % (source,))
        if not source or any(isinstance(s, bool) or not isinstance(s, int) for s in source):
            raise ValueError("AttnControl: source = %r (wanted a non-empty list of row indices)" % (source,))
        B = len(source)
        if any(not 0 <= s < B for s in source):
            raise ValueError("AttnControl: source = %r names a row outside [0, %d)" % (source, B))
        if any(source[s] != s for s in source):
            raise ValueError("AttnControl: source = %r: the source of an edited row must itself be a source (source[s] == s)"
                             % (source,))
        G = sum(1 for r, s in enumerate(source) if s == r)
        if any(source[r] != r for r in range(G)):
            raise ValueError("AttnControl: source = %r: order the rows so that all sources come before all edits -- rows "
                             "[0, G) with source[r] == r, then the edited rows" % (source,))
        self.source, self.rows, self.G, self.R = tuple(source), B, G, B - G
        self.ld = _ld(self.S)
        self.cross_interval = _interval("cross_interval", cross_interval)
        self.self_interval = _interval("self_interval", self_interval)
        self.cross_layers = _layers("cross_layers", cross_layers)
        self.self_layers = _layers("self_layers", self_layers)
        if isinstance(self_max_queries, bool) or not isinstance(self_max_queries, int) or self_max_queries < 0:
            raise ValueError("AttnControl: self_max_queries = %r (wanted an int >= 0)" % (self_max_queries,))
        self.self_max_queries = self_max_queries
        S = self.S
        mapper = self._per_row("mapper", mapper, (S, S))
        keep = self._per_row("keep", keep, (S,))
        scale = self._per_row("scale", scale, (S,))
        # M [R, S, ld] (pad columns 0; the kernel never reads them) and D [R, S], fp32 on the CPU; handles copy them
        self.M = torch.zeros(self.R, S, self.ld, dtype=torch.float32)
        self.D = torch.zeros(self.R, S, dtype=torch.float32)
        for k, r in enumerate(range(G, B)):
            sc = torch.ones(S) if scale[r] is None else scale[r]
            self.M[k, :, :S] = (torch.eye(S) if mapper[r] is None else mapper[r]) * sc[None, :]
            self.D[k] = (torch.zeros(S) if keep[r] is None else keep[r]) * sc
        self._handles = {}

    def _per_row(self, what, value, shape):
        """{row: fp32 CPU tensor or None} of every row, checked"""
        B = self.rows
        if value is None:
            value = {}
        if isinstance(value, dict):
            given = dict(value)
        else:
            value = list(value)
            if len(value) != B:
                raise ValueError("AttnControl: %s has %d entries for %d rows (wanted a dict {row: tensor}, or one entry per "
                                 "row with None for the default)" % (what, len(value), B))
            given = {r: v for r, v in enumerate(value) if v is not None}
        out = {r: None for r in range(B)}
        for r, v in given.items():
            if isinstance(r, bool) or not isinstance(r, int) or not self.G <= r < B:
                raise ValueError("AttnControl: %s[%r]: not an edited row (the edited rows are [%d, %d))" % (what, r, self.G, B))
            if not torch.is_tensor(v) or tuple(v.shape) != shape:
                raise ValueError("AttnControl: %s[%d] is %s (wanted a tensor %s)" % (
                    what, r, tuple(v.shape) if torch.is_tensor(v) else type(v).__name__, shape))
            v = v.detach().to(device="cpu", dtype=torch.float32)
            if not bool(torch.isfinite(v).all()):
                raise ValueError("AttnControl: %s[%d] holds a value that is not finite" % (what, r))
            out[r] = v
        return out

    @classmethod
    def aligned(cls, S, source, pairs, scale=None, **kw):
        """``pairs[r]``: a list of (edit token, source token) for the edited row r (a dict {r: list}, or one entry per row
        with None for sources) -> the control with ``mapper[r][source token, edit token] = 1`` and ``keep[r][j] = 1`` for
        every token j of the edit that is in no pair: paired tokens take the source's attention, new ones keep their own."""
        S = int(S)
        source = list(source)
        items = pairs.items() if isinstance(pairs, dict) else [(r, p) for r, p in enumerate(pairs) if p is not None]
        mapper, keep = {}, {}
        for r, ps in items:
            m, k = torch.zeros(S, S), torch.ones(S)
            for p in ps:
                try:
                    e, s = p
                except (TypeError, ValueError):
                    raise ValueError("AttnControl.aligned: pairs[%r] holds %r (wanted (edit token, source token))" % (r, p))
                if not (isinstance(e, int) and isinstance(s, int) and 0 <= e < S and 0 <= s < S):
                    raise ValueError("AttnControl.aligned: pair (%r, %r) of row %r for %d tokens" % (e, s, r, S))
                m[s, e] = 1
                k[e] = 0
            mapper[r], keep[r] = m, k
        return cls(S, source, mapper=mapper, keep=keep, scale=scale, **kw)

    # ---- the gates ------------------------------------------------------------------------------------------
    def gates(self, time_step, num_diffusion_steps):
        """-> (g_c, g_s) of the step that starts from ``time_step``, floats 0 / 1 (g_s before the layer's query count)"""
        f = float(time_step) / float(num_diffusion_steps)
        return (float(self.cross_interval[0] <= f <= self.cross_interval[1]),
                float(self.self_interval[0] <= f <= self.self_interval[1]))

    # ---- the model's side -------------------------------------------------------------------------------------
    def layer_sets(self, vision_model):
        """-> (cross layer names, self layer names): of ``cross_layers`` the layers WITH text keys, of ``self_layers`` all"""
        cross = tuple(n for n, m in pag.select(vision_model, self.cross_layers) if m.cond_dim is not None and m.cond_dim > 0)
        return cross, pag.layer_names(vision_model, self.self_layers)

    def static_key(self, vision_model):
        """what a captured graph depends on: other mapper / keep / scale / interval values replay the same graph"""
        return ("control", self.S, self.ld, self.source, self.self_max_queries) + self.layer_sets(vision_model)

    def rows_for(self, guidance=False, pag_rows=False, device=None, cached=True):
        """the handle a sampler hands to ``applied``: the control for a model batch of [uncond |] cond [| perturbed]; the
        eager samplers share one per layout and device (its gates are rewritten every step)"""
        device = torch.device("cpu" if device is None else device)
        key = (bool(guidance), bool(pag_rows), device)
        if not cached:
            return BatchCtrl(self, *key)
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = BatchCtrl(self, *key)
        return h


class BatchCtrl:
    """``AttnControl`` with the block layout of the model's batch and the device fixed: the row tables, M, D and the two
    gates as device tensors.  ``GraphedSampler`` owns one per graph entry (static copies: ``fill`` rewrites M and D in place,
    the graph body points ``gate_c`` / ``gate_s`` at the row of its gate tables); the eager samplers ``set_gates`` per step."""

    def __init__(self, control, guidance, pag_rows, device):
        self.S, self.ld, self.rows, self.G, self.R = control.S, control.ld, control.rows, control.G, control.R
        self.self_max_queries = control.self_max_queries
        B = control.rows
        self.total = (1 + bool(guidance) + bool(pag_rows)) * B
        base = B if guidance else 0
        self.row0 = base + control.G
        self.src_host = tuple(base + control.source[r] for r in range(control.G, B))
        self.own = torch.arange(self.row0, self.row0 + self.R, dtype=torch.int32, device=device)
        self.src = torch.tensor(self.src_host, dtype=torch.int32, device=device)
        self.M = control.M.to(device).contiguous()
        self.D = control.D.to(device).contiguous()
        self.gate_c = torch.ones(1, dtype=torch.float32, device=device)
        self.gate_s = torch.ones(1, dtype=torch.float32, device=device)
        self.zero = torch.zeros(1, dtype=torch.float32, device=device)   # the gate of a layer outside a layer set

    def fill(self, control):
        """other mapper / keep / scale values of a control with the same rows and tokens, IN PLACE (same storage: a captured
        graph reads it by address).  The source rows are part of the graph key, so the tables stay."""
        if (control.S, control.rows, control.G) != (self.S, self.rows, self.G):
            raise ValueError("BatchCtrl: a control over other rows or tokens")
        self.M.copy_(control.M)
        self.D.copy_(control.D)

    def set_gates(self, g_c, g_s):
        self.gate_c.fill_(float(g_c))
        self.gate_s.fill_(float(g_s))


class LayerCtrl:
    """what a layer's ``_attn_ctrl`` holds: the batch handle and which of the two controls this layer is selected for"""

    def __init__(self, handle, cross, self_):
        self.handle, self.cross, self.self_ = handle, bool(cross), bool(self_)

    def rows(self, N, L, kvc):
        """-> the ``ctrl_rows`` of ``ops.attention`` for this layer at a batch of N rows of L queries"""
        h = self.handle
        if N != h.total:
            raise ValueError("AttnControl: a batch of %d rows for control over %d rows of a model batch of %d; "
                             "mixed-resolution nested batches are not supported" % (N, h.rows, h.total))
        if kvc is not None and kvc.shape[1] != h.S:
            raise ValueError("AttnControl: control over %d tokens for text keys of %d" % (h.S, kvc.shape[1]))
        return _Rows(h, h.gate_c if (self.cross and kvc is not None) else h.zero,
                     h.gate_s if (self.self_ and L <= h.self_max_queries) else h.zero)


class _Rows:
    __slots__ = ("row0", "R", "own", "src", "src_host", "M", "D", "gate_c", "gate_s")

    def __init__(self, h, gate_c, gate_s):
        self.row0, self.R, self.own, self.src, self.src_host, self.M, self.D = h.row0, h.R, h.own, h.src, h.src_host, h.M, h.D
        self.gate_c, self.gate_s = gate_c, gate_s


class applied(switched):
    """``with applied(vision_model, handle, control=None, names=None):`` -- inside, the ``SelfAttention`` layers that
    ``control.cross_layers`` (those with text keys) or ``control.self_layers`` select run ``ops.attention(..., ctrl_rows=)`` with
    ``handle`` (a ``BatchCtrl``); on exit (also by an exception) every layer has what it had before.  ``names``: the two
    layer sets already resolved (``AttnControl.layer_sets``)."""

    def __init__(self, vision_model, handle, control=None, names=None):
        if not isinstance(handle, BatchCtrl):
            raise ValueError("applied: %r (wanted a BatchCtrl: AttnControl.rows_for(...))" % (handle,))
        if names is None:
            if control is None:
                raise ValueError("applied: neither a control nor its layer names")
            names = control.layer_sets(vision_model)
        cross, self_ = set(names[0]), set(names[1])
        if not cross and not self_:
            raise ValueError("AttnControl: cross_layers and self_layers select no attention layer")
        order = [n for n, _ in pag.select(vision_model, "all") if n in cross or n in self_]
        super().__init__((vision_model.get_submodule(n), {"_attn_ctrl": LayerCtrl(handle, n in cross, n in self_)})
                         for n in order)


# ---- the kernels in torch ops, for CPU tensors ------------------------------------------------------------------
def mix_kv(kvc, own, src, M, D, mask, gate):
    """``ops.ctrl_mix_kv`` in torch ops: fp32 accumulation over j ascending, one rounding to kvc's dtype"""
    N, S, C2 = kvc.shape
    C = C2 // 2
    on = float(gate) != 0
    own, src = [int(v) for v in own], [int(v) for v in src]
    kv_a = kvc.new_zeros(len(own), S, C2)
    kv_b = kvc.new_zeros(len(own), S, C2)
    for k, (r, s) in enumerate(zip(own, src)):
        kv_a[k, :, :C] = kvc[s, :, :C]
        kv_b[k] = kvc[r]
        if not on:
            continue
        v = kvc[r, :, C:].float()
        live = torch.ones(S, dtype=torch.bool) if mask is None else mask.reshape(N, S)[r] != 0
        acc = torch.zeros(S, C, dtype=torch.float32)
        for j in range(S):
            if live[j]:
                acc = torch.addcmul(acc, M[k, :, j:j + 1].float(), v[j:j + 1])
        kv_a[k, :, C:] = acc.to(kvc.dtype)
        kv_b[k, :, C:] = (v * D[k].float()[:, None]).to(kvc.dtype)
    return kv_a, kv_b


def gather_qkv(qkv, own, src, gate):
    """``ops.ctrl_gather_qkv`` in torch ops; the k and v columns of q_src, which the kernel leaves undefined, are zeros"""
    C = qkv.shape[-1] // 3
    own = torch.as_tensor([int(v) for v in own], dtype=torch.long)
    src = torch.as_tensor([int(v) for v in src], dtype=torch.long)
    q3 = qkv.reshape(qkv.shape[0], -1, 3 * C)
    qs = q3[own].clone()
    if float(gate) != 0:
        qs[..., :2 * C] = q3[src][..., :2 * C]
    qx = torch.zeros_like(qs)
    qx[..., :C] = q3[src][..., :C]
    return qs, qx


__all__ = ["AttnControl", "BatchCtrl", "LayerCtrl", "applied", "mix_kv", "gather_qkv"]
