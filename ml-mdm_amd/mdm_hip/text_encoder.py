"""Frozen T5 v1.1 / flan text encoder on the HIP path (mirror of ml_mdm.language_models.factory: T5Encoder,
LanguageModel; factory.py:14-38, 84-101).

The reference runs ``google/flan-t5-xl`` on every training batch and in every ``sample()`` call.  Padded tokens can
never influence valid ones (keys are masked, and factory.py:101 zeroes the padded outputs), so the whole encoder runs
on the PACKED valid tokens of a batch -- each token keeps its original position for the relative bias, which makes
the packing exact, masks with holes included.  Per layer: 4 GEMMs (the library's existing kernel; Wq|Wk|Wv and
Wi0|Wi1 concatenated), one attention launch, two residual-add + RMSNorm launches, one gated-GELU launch
(csrc/text_encoder.hip).  Parameters frozen, forward-only weight packs and ``no_grad`` -- except with a textual
inversion attached (textual_inversion.py): then the forward is one autograd node, and its backward is the chain of INPUT
gradients down to the learned embedding rows (csrc/text_encoder_bwd.hip; input-gradient packs built on first use).

The tokenizer and ``from_pretrained`` stay the user's: build a ``T5EncoderConfig.from_hf(hf_model.config)``, then
``load_state_dict(hf_model.state_dict(), strict=False)``.  Nothing here imports ``transformers``.
"""
import dataclasses
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .unet import compute_dtype


@dataclasses.dataclass
class T5EncoderConfig:
    vocab_size: int
    d_model: int
    d_kv: int
    d_ff: int
    num_layers: int
    num_heads: int
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"

    def __post_init__(self):
        if self.feed_forward_proj != "gated-gelu":
            raise NotImplementedError("feed_forward_proj=%r: only the gated-gelu feed-forward of T5 v1.1 / flan is built"
                                      % (self.feed_forward_proj,))

    @classmethod
    def from_hf(cls, cfg):
        """from any object with the attributes of a ``transformers.T5Config``"""
        kw = {}
        for f in dataclasses.fields(cls):
            if hasattr(cfg, f.name):
                kw[f.name] = getattr(cfg, f.name)
            elif f.default is dataclasses.MISSING:
                raise AttributeError("config object has no attribute %r" % f.name)
        return cls(**kw)


def relative_bucket(rel, num_buckets=32, max_distance=128):
    """The bidirectional T5 bucket of ``rel`` = key position - query position (an integer CPU tensor), computed in fp32
    with the same operations as the reference's model so that the boundaries fall where its own do."""
    rel = torch.as_tensor(rel, dtype=torch.long, device="cpu")
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    r = rel.abs()
    half = nb // 2
    large = half + (torch.log(r.float() / half) / math.log(max_distance / half) * (nb - half)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return out + torch.where(r < half, r, large)


def bias_index(S, num_buckets=32, max_distance=128):
    """bucket of every relative position r in [-(S-1), S-1]: a [2S-1] long tensor, entry r + S - 1"""
    return relative_bucket(torch.arange(-(S - 1), S), num_buckets, max_distance)


def pack_index(mask):
    """Host-side packing plan of a 0/1 mask [B, S] (numpy array or CPU tensor; holes are legal):
    ``idx`` [T] flat indices b * S + s of the valid tokens in row order, ``seq_start`` [B + 1], ``pos`` [T] original
    index of each packed token in its row, ``src`` [B * S] packed index of each position or -1, ``max_len``."""
    m = np.asarray(mask.numpy() if isinstance(mask, torch.Tensor) else mask) != 0
    if m.ndim != 2:
        raise ValueError("attention mask must be [B, S], got shape %s" % (m.shape,))
    B, S = m.shape
    idx = np.flatnonzero(m.reshape(-1))
    lens = m.sum(axis=1)
    seq_start = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(lens, out=seq_start[1:])
    src = np.full(B * S, -1, dtype=np.int32)
    src[idx] = np.arange(idx.size, dtype=np.int32)
    return {"idx": idx.astype(np.int64), "seq_start": seq_start, "pos": (idx % S).astype(np.int32), "src": src,
            "max_len": int(lens.max()) if B else 0, "T": int(idx.size), "B": B, "S": S}


class _Params(nn.Module):
    """pure parameter container (the forward pass lives in T5Encoder.forward)"""


def _frozen(t):
    return nn.Parameter(t, requires_grad=False)


def _linear(cout, cin):
    m = _Params()
    m.weight = _frozen(torch.randn(cout, cin) * cin ** -0.5)
    return m


def _norm(d):
    m = _Params()
    m.weight = _frozen(torch.ones(d))
    return m


_LINEARS = ("layer.0.SelfAttention.q", "layer.0.SelfAttention.k", "layer.0.SelfAttention.v", "layer.0.SelfAttention.o",
            "layer.1.DenseReluDense.wi_0", "layer.1.DenseReluDense.wi_1", "layer.1.DenseReluDense.wo")


class T5Encoder(nn.Module):
    """``T5Encoder(config)``: the encoder of a T5 v1.1 / flan model; ``state_dict`` keys are those of
    ``transformers.T5EncoderModel``.  ``forward`` has the signature of the reference's ``T5Encoder.forward``
    (factory.py:22-38) and returns the last hidden state, fp32 ``[B, S, d_model]``, zero at masked positions."""

    def __init__(self, config: T5EncoderConfig):
        super().__init__()
        c = self.config = config
        inner = c.num_heads * c.d_kv
        if c.d_model % 8 or c.d_ff % 8 or inner % 8:
            raise ValueError("d_model, d_ff and num_heads * d_kv must be multiples of 8 (16-byte chunks of bf16)")
        self.shared = _Params()
        self.shared.weight = _frozen(torch.randn(c.vocab_size, c.d_model))
        enc = self.encoder = _Params()
        enc.embed_tokens = _Params()
        enc.embed_tokens.weight = self.shared.weight          # tied, as in the reference's model
        enc.block = nn.ModuleList()
        for l in range(c.num_layers):
            blk = _Params()
            l0, l1 = _Params(), _Params()
            att = l0.SelfAttention = _Params()
            att.q, att.k, att.v = _linear(inner, c.d_model), _linear(inner, c.d_model), _linear(inner, c.d_model)
            att.o = _linear(c.d_model, inner)
            if l == 0:
                att.relative_attention_bias = _Params()
                att.relative_attention_bias.weight = _frozen(
                    torch.randn(c.relative_attention_num_buckets, c.num_heads) * c.d_model ** -0.5)
            l0.layer_norm = _norm(c.d_model)
            ff = l1.DenseReluDense = _Params()
            ff.wi_0, ff.wi_1, ff.wo = _linear(c.d_ff, c.d_model), _linear(c.d_ff, c.d_model), _linear(c.d_model, c.d_ff)
            l1.layer_norm = _norm(c.d_model)
            blk.layer = nn.ModuleList([l0, l1])
            enc.block.append(blk)
        enc.final_layer_norm = _norm(c.d_model)
        self._packs = {}        # dtype -> (signature of the masters, [(Wqkv, Wo, Wi, Wo_ff) per layer])
        self._tables = {}       # S -> (signature of the bias weight, [H, 2S-1] fp32 table)
        self._released = None   # the dtype the masters were released for
        self._dpacks = {}       # dtype -> (signature, [input-gradient packs per layer]): only after a differentiable forward
        self.__dict__["_adapter"] = None   # the attached TextualInversion (not a submodule: it owns its parameter)

    # ---- reference call surface ---------------------------------------------------------------------------------
    @property
    def embed_dim(self):
        return self.config.d_model

    def load(self):
        pass

    def state_dict(self, *args, **kwargs):
        if self._released is not None:
            raise _lib.MdmHipError("release_masters() dropped the fp32 projection weights of this T5Encoder: it has no "
                                   "state_dict any more (save it before releasing, or reload the checkpoint)")
        return super().state_dict(*args, **kwargs)

    # ---- weights ------------------------------------------------------------------------------------------------
    def _masters(self, l):
        blk = self.encoder.block[l]
        return [blk.get_submodule(n).weight for n in _LINEARS]

    def _layer_packs(self, dtype):
        if self._released is not None:
            if dtype != self._released:
                raise _lib.MdmHipError("masters were released after packing for %s; %s is no longer available"
                                       % (self._released, dtype))
            return self._packs[dtype][1]
        L = self.config.num_layers
        sig = tuple((w._version, w.data_ptr()) for l in range(L) for w in self._masters(l))
        ent = self._packs.get(dtype)
        if ent is not None and ent[0] == sig:
            return ent[1]

        def pack(*ws):   # forward-only: this model never runs backward
            w = ws[0] if len(ws) == 1 else torch.cat(ws, 0)
            return ops.packed_weight(w.detach(), None, dtype, forward_only=True)[0]

        packs = []
        for l in range(L):
            q, k, v, o, wi0, wi1, wo = self._masters(l)
            packs.append((pack(q, k, v), pack(o), pack(wi0, wi1), pack(wo)))
        self._packs[dtype] = (sig, packs)
        return packs

    def _layer_dpacks(self, dtype):
        """[(Wqkv, Wo, Wi, Wo_ff) per layer] in the input-gradient layout of the GEMM, for the concatenations the forward
        packs: a second copy of the projection weights (2.4 GB for flan-t5-xl in bf16), built on the first differentiable
        forward and never otherwise."""
        if self._released is not None:
            raise _lib.MdmHipError("release_masters() dropped the fp32 projection weights of this T5Encoder: a differentiable "
                                   "forward (textual inversion) needs them for its input-gradient packs -- reload the checkpoint")
        L = self.config.num_layers
        sig = tuple((w._version, w.data_ptr()) for l in range(L) for w in self._masters(l))
        ent = self._dpacks.get(dtype)
        if ent is not None and ent[0] == sig:
            return ent[1]

        def pack(*ws):   # a temporary tensor each time: the forward copy packed_weight builds beside it dies with it
            w = ws[0].detach() if len(ws) == 1 else torch.cat(ws, 0)
            wd = ops.packed_weight(w, None, dtype, forward_only=False)[1]
            if wd is None:
                raise _lib.MdmHipError("no input-gradient pack for a projection of shape %s" % (tuple(w.shape),))
            return wd

        packs = []
        for l in range(L):
            q, k, v, o, wi0, wi1, wo = self._masters(l)
            packs.append((pack(q, k, v), pack(o), pack(wi0, wi1), pack(wo)))
        self._dpacks[dtype] = (sig, packs)
        return packs

    def release_masters(self, dtype=None):
        """Drop the fp32 copies of the projection weights once they are packed for ``dtype`` (default: the current
        compute dtype): flan-t5-xl keeps 2.4 GB of packed bf16 weights instead of 4.9 GB more of masters.  The
        embedding, the norms and the bias table stay.  Afterwards only that dtype runs and ``state_dict()`` raises."""
        if self._dpacks:
            raise _lib.MdmHipError("this T5Encoder has run a differentiable forward (textual inversion): its input-gradient "
                                   "packs are rebuilt from the fp32 projection weights, which release_masters() would drop")
        dtype = dtype or compute_dtype()
        ops._require_gpu(self.shared.weight)
        packs = self._layer_packs(dtype)
        self._packs = {dtype: (None, packs)}
        for l in range(self.config.num_layers):
            for w in self._masters(l):
                w.data = torch.empty(0, device=w.device)
        self._released = dtype
        return self

    def _bias_table(self, S):
        w = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        sig = (w._version, w.data_ptr())
        ent = self._tables.get(S)
        if ent is None or ent[0] != sig:
            c = self.config
            bi = bias_index(S, c.relative_attention_num_buckets, c.relative_attention_max_distance).to(w.device)
            if len(self._tables) > 16:
                self._tables.clear()
            ent = self._tables[S] = (sig, w.detach().float().index_select(0, bi).t().contiguous())
        return ent[1]

    # ---- forward ------------------------------------------------------------------------------------------------
    def forward(self, input_ids, attention_mask=None, return_dict=None, return_penultimate=None, *args, **kwargs):
        """Inference (``no_grad``, nothing saved) unless a textual-inversion adapter is attached, its parameter requires
        grad and grad mode is on: then one autograd node runs the same launches, saves what the backward needs and
        returns the input gradient of the learned rows (textual_inversion.py)."""
        ti = self._adapter
        if ti is None or not (torch.is_grad_enabled() and ti.embeddings.requires_grad):
            with torch.no_grad():
                plan = self._plan(input_ids, attention_mask)
                return self._launch(plan, None if ti is None else ti.embeddings.detach(), None)
        return _T5EncoderGradFn.apply(ti.embeddings, self, input_ids, attention_mask)

    def _plan(self, input_ids, attention_mask, flat=False):
        """host side of a forward: checks, the packing plan and its one copy to the device.  ``flat``: also upload the
        packed -> flat index b * S + s of every token (what the backward of the final norm gathers through)"""
        c = self.config
        ti = self._adapter
        table = self.shared.weight
        ops._require_gpu(table)
        dev = table.device
        for t in (input_ids, attention_mask):
            if isinstance(t, torch.Tensor) and t.is_cuda and t.device != dev:
                raise _lib.MdmHipError("T5Encoder is on %s, got a tensor on %s" % (dev, t.device))
        if input_ids.ndim != 2:
            raise ValueError("input_ids must be [B, S]")
        B, S = int(input_ids.shape[0]), int(input_ids.shape[1])
        if S > 512:
            raise _lib.MdmHipError("sequence length %d > 512: the attention kernel holds one head's bias table in LDS" % S)
        if attention_mask is None:
            mask_h = np.ones((B, S), dtype=bool)
        elif isinstance(attention_mask, torch.Tensor):
            mask_h = attention_mask.detach().cpu().numpy()      # a GPU mask costs this one copy; host masks cost nothing
        else:
            mask_h = np.asarray(attention_mask)
        if tuple(mask_h.shape) != (B, S):
            raise ValueError("attention_mask %s does not match input_ids %s" % (mask_h.shape, (B, S)))
        pk = pack_index(mask_h)
        T = pk["T"]
        plan = {"pk": pk, "B": B, "S": S, "T": T, "dev": dev, "ids_h": None}
        if T == 0:
            return plan

        # one pinned host buffer, one asynchronous copy: [ids | seq_start | pos | src | flat]
        ids_on_host = not (isinstance(input_ids, torch.Tensor) and input_ids.is_cuda)
        parts = [pk["seq_start"], pk["pos"], pk["src"]]
        if flat:
            parts.append(pk["idx"].astype(np.int32))
        if ids_on_host:
            ids_h = np.asarray(input_ids.numpy() if isinstance(input_ids, torch.Tensor) else input_ids).reshape(-1)[pk["idx"]]
            bad = (ids_h < 0) | (ids_h >= c.vocab_size)
            if ti is not None:
                bad &= ~np.isin(ids_h, ti.token_ids)
            if bad.any():
                raise ValueError("token id %d outside [0, %d)%s" % (int(ids_h[bad][0]), c.vocab_size,
                                 "" if ti is None else " and not a placeholder of the attached textual inversion"))
            plan["ids_h"] = ids_h
            parts.insert(0, ids_h.astype(np.int32))
        host = torch.from_numpy(np.concatenate(parts)).pin_memory()
        devbuf = host.to(dev, non_blocking=True)
        o = 0
        if ids_on_host:
            ids = devbuf[:T]
            o = T
        else:
            gather = torch.from_numpy(pk["idx"]).pin_memory().to(dev, non_blocking=True)
            ids = input_ids.reshape(-1).index_select(0, gather).to(torch.int32)
        plan["ids"] = ids
        o1, o2, o3 = o + B + 1, o + B + 1 + T, o + B + 1 + T + B * S
        plan["seq_start"], plan["pos"], plan["src"], plan["flat"] = devbuf[o:o1], devbuf[o1:o2], devbuf[o2:o3], devbuf[o3:]
        return plan

    def _launch(self, plan, learned, save):
        """The launch sequence on a plan.  ``learned`` (fp32 [P, D] or None): the rows of the attached adapter, which
        override the table.  ``save`` (a dict or None): keep what the backward needs -- per layer the two fp32 stream
        rows, qkv, the attention output, its log-sum-exp and u -- instead of reusing one set of buffers."""
        c = self.config
        table = self.shared.weight
        pk, B, S, T, dev = plan["pk"], plan["B"], plan["S"], plan["T"], plan["dev"]
        D = c.d_model
        out = torch.empty(B, S, D, dtype=torch.float32, device=dev)
        if T == 0:
            return out.zero_()
        ids, seq_start, pos, src = plan["ids"], plan["seq_start"], plan["pos"], plan["src"]
        dtype = compute_dtype()
        dt = ops.F32 if dtype == torch.float32 else ops.BF16
        packs = self._layer_packs(dtype)
        bias = self._bias_table(S)
        H, dk, F, eps = c.num_heads, c.d_kv, c.d_ff, float(c.layer_norm_epsilon)
        inner = H * dk
        L, p, st = _lib.lib(), ops._p, ops._stream
        new = lambda n, t=dtype: torch.empty(T, n, dtype=t, device=dev)
        x, h, delta, y = new(D, torch.float32), new(D), new(D), new(F)
        if save is None:       # one set for every layer; a saving forward allocates these per layer below
            qkv, att, u = new(3 * inner), new(inner), new(2 * F)

        def gemm(a, w, yout, cin, cout):
            ops._conv_launch(a, w, None, None, None, yout, None, T, 1, 1, cin, 1, 1, cout, 1, 1, 0, 0)

        blocks = self.encoder.block
        if learned is None:
            _lib.check(L.mdm_t5_embed_rms(p(ids), p(table), p(blocks[0].layer[0].layer_norm.weight), p(x), p(h), T, D,
                                          c.vocab_size, eps, dt, st()), "mdm_t5_embed_rms")
        else:
            if learned.device != dev or learned.dtype != torch.float32 or not learned.is_contiguous():
                raise _lib.MdmHipError("the textual-inversion embeddings must be contiguous fp32 on the encoder's device (%s), "
                                       "got %s on %s" % (dev, learned.dtype, learned.device))
            slot_of_id = self._adapter._slot_table(dev)
            _lib.check(L.mdm_t5_embed_rms_slots(p(ids), p(table), p(slot_of_id), p(learned), p(blocks[0].layer[0].layer_norm.weight),
                                                p(x), p(h), T, D, c.vocab_size, int(slot_of_id.numel()), int(learned.shape[0]),
                                                eps, dt, st()), "mdm_t5_embed_rms_slots")
        layers = []
        for l in range(c.num_layers):
            wqkv, wo, wi, wo_ff = packs[l]
            if save is not None:
                xa, qkv, att, u, lse = x.clone(), new(3 * inner), new(inner), new(2 * F), torch.empty(H, T, device=dev)
            gemm(h, wqkv, qkv, D, 3 * inner)
            if save is None:
                _lib.check(L.mdm_t5_attn_fwd(p(qkv), p(seq_start), p(pos), p(bias), p(att), B, T, S, pk["max_len"], H, dk, dt,
                                             st()), "mdm_t5_attn_fwd")
            else:
                _lib.check(L.mdm_t5_attn_fwd_lse(p(qkv), p(seq_start), p(pos), p(bias), p(att), p(lse), B, T, S, pk["max_len"],
                                                 H, dk, dt, st()), "mdm_t5_attn_fwd_lse")
            gemm(att, wo, delta, inner, D)
            _lib.check(L.mdm_t5_add_rms(p(x), p(delta), p(blocks[l].layer[1].layer_norm.weight), p(h), T, D, eps, dt, st()),
                       "mdm_t5_add_rms")
            if save is not None:
                layers.append((xa, x.clone(), qkv, att, lse, u))
            gemm(h, wi, u, D, 2 * F)
            _lib.check(L.mdm_t5_gated_gelu(p(u), p(y), T, F, dt, st()), "mdm_t5_gated_gelu")
            gemm(y, wo_ff, delta, F, D)
            if l + 1 < c.num_layers:
                _lib.check(L.mdm_t5_add_rms(p(x), p(delta), p(blocks[l + 1].layer[0].layer_norm.weight), p(h), T, D, eps, dt,
                                            st()), "mdm_t5_add_rms")
        _lib.check(L.mdm_t5_final_rms(p(x), p(delta), p(self.encoder.final_layer_norm.weight), p(src), p(out), B * S, D, eps,
                                      dt, st()), "mdm_t5_final_rms")
        if save is not None:
            save.update(dtype=dtype, layers=layers, delta=delta, bias=bias)
        return out

    def _backward(self, plan, saved, dout):
        """d loss / d learned [P, D] from d loss / d out [B, S, D]: the reverse chain of ``_launch``, input gradients only
        (per layer four GEMMs on the input-gradient packs -- one for each of the forward's, which packs Wq|Wk|Wv and
        Wi0|Wi1 as one weight each -- and the attention, gated GELU and RMS backward of csrc/text_encoder_bwd.hip)"""
        c = self.config
        ti = self._adapter
        pk, B, S, T, dev = plan["pk"], plan["B"], plan["S"], plan["T"], plan["dev"]
        D, H, dk, F, eps = c.d_model, c.num_heads, c.d_kv, c.d_ff, float(c.layer_norm_epsilon)
        inner = H * dk
        dtype = saved["dtype"]
        dt = ops.F32 if dtype == torch.float32 else ops.BF16
        dpacks = self._layer_dpacks(dtype)
        L, p, st = _lib.lib(), ops._p, ops._stream
        dout = ops._c(dout.float())
        new = lambda n, t=dtype: torch.empty(T, n, dtype=t, device=dev)
        dx = new(D, torch.float32)
        # the stream gradient as a GEMM operand: dx itself in fp32, a storage-type copy written by the norm kernels in bf16
        g = dx if dtype == torch.float32 else new(D)
        glo = None if dtype == torch.float32 else g
        dh, dy, du, datt, dqkv = new(D), new(F), new(2 * F), new(inner), new(3 * inner)
        flat = plan["flat"]

        def dgemm(a, w, yout, k, n):     # yout [T, n] = a [T, k] @ W [k, n], W the forward's weight as the dgrad pack holds it
            ops._conv_launch(a, w, None, None, None, yout, None, T, 1, 1, k, 1, 1, n, 1, 1, 0, 0)

        blocks = self.encoder.block
        layers = saved["layers"]
        _lib.check(L.mdm_t5_final_rms_bwd(p(layers[-1][1]), p(saved["delta"]), p(self.encoder.final_layer_norm.weight), p(dout),
                                          p(flat), p(dx), p(glo), T, D, eps, dt, st()), "mdm_t5_final_rms_bwd")
        for l in reversed(range(c.num_layers)):
            xa, xb, qkv, att, lse, u = layers[l]
            dwqkv, dwo, dwi, dwo_ff = dpacks[l]
            dgemm(g, dwo_ff, dy, D, F)
            _lib.check(L.mdm_t5_gated_gelu_bwd(p(u), p(dy), p(du), T, F, dt, st()), "mdm_t5_gated_gelu_bwd")
            dgemm(du, dwi, dh, 2 * F, D)
            _lib.check(L.mdm_t5_rms_bwd(p(xb), p(blocks[l].layer[1].layer_norm.weight), p(dh), p(dx), p(glo), T, D, eps, dt,
                                        st()), "mdm_t5_rms_bwd")
            dgemm(g, dwo, datt, D, inner)
            _lib.check(L.mdm_t5_attn_bwd(p(qkv), p(att), p(lse), p(datt), p(plan["seq_start"]), p(plan["pos"]), p(saved["bias"]),
                                         p(dqkv), B, T, S, pk["max_len"], H, dk, dt, st()), "mdm_t5_attn_bwd")
            dgemm(dqkv, dwqkv, dh, 3 * inner, D)
            _lib.check(L.mdm_t5_rms_bwd(p(xa), p(blocks[l].layer[0].layer_norm.weight), p(dh), p(dx), p(glo), T, D, eps, dt,
                                        st()), "mdm_t5_rms_bwd")
        slot_start, tokens = ti._slot_index(plan, dev)
        P = len(ti.token_ids)
        dlearned = torch.empty(P, D, dtype=torch.float32, device=dev)
        _lib.check(L.mdm_t5_embed_bwd(p(dx), p(slot_start), p(tokens), p(dlearned), P, D, int(tokens.numel()), T, st()),
                   "mdm_t5_embed_bwd")
        return dlearned


class _T5EncoderGradFn(torch.autograd.Function):
    """The encoder as ONE autograd node whose only differentiable input is the [P, D] parameter of the attached textual
    inversion: the forward is the inference launch sequence (same bits), the backward ``T5Encoder._backward``."""

    @staticmethod
    def forward(ctx, embeddings, enc, input_ids, attention_mask):
        plan = enc._plan(input_ids, attention_mask, flat=True)
        saved = {}
        if plan["T"]:
            enc._layer_dpacks(compute_dtype())     # the input-gradient packs: built on the first differentiable forward
        out = enc._launch(plan, ops._c(embeddings.detach()), saved)
        ti = enc._adapter
        # the plan and the slot index of the backward are built from the adapter as it is now: remember which it was
        ctx.enc, ctx.plan, ctx.saved, ctx.adapter, ctx.token_ids = enc, plan, saved, ti, tuple(ti.token_ids)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        enc, plan, saved = ctx.enc, ctx.plan, ctx.saved
        ti = enc._adapter
        if ti is not ctx.adapter:
            raise _lib.MdmHipError("the textual inversion was detached (or another attached) between this forward and its "
                                   "backward")
        if tuple(ti.token_ids) != ctx.token_ids:
            raise _lib.MdmHipError("the token_ids of the textual inversion changed between this forward and its backward "
                                   "(load_state_dict?): %s then, %s now -- run the forward again"
                                   % (list(ctx.token_ids), list(ti.token_ids)))
        if saved is None:
            raise _lib.MdmHipError("this forward of the T5Encoder was already backpropagated through: its saved activations "
                                   "are freed after the first backward, retain_graph=True or not -- run the forward again")
        ctx.saved = None
        if plan["T"] == 0:
            return torch.zeros_like(ti.embeddings), None, None, None
        return enc._backward(plan, saved, dout), None, None, None



class LanguageModel(nn.Module):
    """Mirror of the reference's ``LanguageModel`` (factory.py:44-102): tokens -> (text states, mask).  ``model`` is a
    ``T5Encoder`` (or None / dropped with ``args.use_precomputed_text_embeddings``).  Tokens that arrive as a host
    array, as they do from the reference's reader, are packed on the host: the pad-token mask never visits the GPU
    before the encoder has been launched."""

    def __init__(self, args, model):
        super().__init__()
        self.model = model
        self.embed_dim = model.embed_dim
        self.device = "cpu"
        self.args = args
        if args.use_precomputed_text_embeddings:
            self.model = None

    def to(self, device):
        if self.model is not None:
            self.model = self.model.to(device)
        self.device = device
        return self

    def forward(self, sample, tokenizer):
        args = self.args
        if getattr(args, "categorical_conditioning", False):
            raise NotImplementedError("categorical conditioning has no text encoder (the reference's create_lm refuses it too)")
        tokens = sample["tokens"]
        pad = tokenizer.token_id(args.reader_config.padding_token)
        if isinstance(tokens, torch.Tensor):
            mask_h = None
            lm_mask = (tokens != pad).float()
        else:
            tokens = np.asarray(tokens)
            mask_h = tokens != pad
            lm_mask = torch.from_numpy(mask_h.astype(np.float32)).to(self.device, non_blocking=True)
        if args.use_precomputed_text_embeddings:
            emb = sample["text_embedding"].float()
            return emb * lm_mask.to(emb.device).unsqueeze(-1), lm_mask
        mask_arg = lm_mask if mask_h is None else mask_h
        if getattr(args, "fp16", False):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = self.model(tokens, mask_arg, return_penultimate=True).float()
        else:
            out = self.model(tokens, mask_arg, return_penultimate=True).float()
        if not isinstance(self.model, T5Encoder):     # T5Encoder already wrote exact zeros at the padded positions
            out = out * lm_mask.unsqueeze(-1)
        return out, lm_mask
