"""Cases shared by the cross-attention-map tests (CPU and GPU): the fp64 restatement of what ``mdm_attn_cross_maps`` adds
(``w / H * sum_h softmax(logits + bias; live keys)``), the oracle's attention layer with a recording hook swapped in by layer
(the way ``region_cases.biased_oracle`` swaps its bias in), a stub denoiser that records the handle it sees, and the case
tables.  Kernel inputs are ``pag_cases.attn_inputs`` / ``masks`` and ``region_cases.kernel_bias``."""
import contextlib
import functools
import math

import torch

import pag_cases as PG
import parity_cases as PC
import region_cases as RC
import unet_oracle as O

NEG_INF = float("-inf")

# (d, H, L, S) of the bit-exact checks: one key tile and several, a ragged query tile, H = 1 and 3
EXACT_CASES = [(32, 3, 80, 5), (96, 1, 64, 77), (128, 3, 16, 130), (64, 3, 80, 32)]
# the sampler calls: DDIM(0), DPM-Solver++(2M), CFG + PAG + regions, an interval ("half": the first half of the schedule)
SAMPLER_CASES = [
    ("mini_unet", dict(ddim_eta=0), None),
    ("mini_nested", dict(solver="dpmpp_2m"), None),
    ("mini_unet", dict(ddim_eta=0, pag_scale=1.5, regions=True), None),
    ("mini_nested", dict(ddim_eta=0), (0.5, 1.0)),
]
SAMPLER_IDS = ["unet-ddim0", "nested-dpmpp_2m", "unet-cfg-pag-regions", "nested-ddim0-interval"]


# ---- the kernel ----------------------------------------------------------------------------------------------------
def probs_ref(q, kc, heads, mask, bias):
    """fp64 probabilities of the text term, mean over heads.  q [B, C, L], kc [B, C, S], mask [B, S] or None, bias
    [B, L, >= S] or None -> ([B, L, S], live [B, L]): logits q.k/sqrt(d) + bias, then exclusion (mask == 0, or bias <=
    -1e30) as ``region_cases.cross_term_ref``; a query with no live key gets zeros."""
    B, C, L = q.shape
    S = kc.shape[-1]
    d = C // heads
    s = 1.0 / math.sqrt(math.sqrt(d))
    qh = (q.double() * s).reshape(B, heads, d, L)
    kh = (kc.double() * s).reshape(B, heads, d, S)
    logits = torch.einsum("bhdl,bhds->bhls", qh, kh)
    live = torch.ones(B, L, S, dtype=torch.bool)
    if bias is not None:
        b = bias[:, :, :S].double()
        live = live & (b > -1e30)
        logits = logits + torch.where(live, b, torch.zeros_like(b))[:, None]
    if mask is not None:
        live = live & (mask != 0)[:, None, :]
    logits = logits.masked_fill(~live[:, None], NEG_INF)
    any_live = live.any(dim=-1)
    probs = torch.softmax(torch.where(any_live[:, None, :, None], logits, torch.zeros_like(logits)), dim=-1)
    probs = torch.where(any_live[:, None, :, None], probs, torch.zeros_like(probs))
    return probs.mean(dim=1), any_live


def cross_maps_ref(qkv, kvc, mask, bias, heads, acc, w=1.0):
    """fp64: acc [B, L, ld] with w x the head-mean probabilities added to its columns [0, S); the others as they are.
    qkv [B, L, 3C], kvc [B, S, 2C], mask [B, S] or None, bias [B, L, >= S] or None."""
    C = qkv.shape[-1] // 3
    S = kvc.shape[1]
    p, _ = probs_ref(qkv.double()[..., :C].transpose(1, 2), kvc.double()[..., :C].transpose(1, 2), heads, mask, bias)
    out = acc.double().clone()
    out[..., :S] += w * p
    return out


@functools.lru_cache(maxsize=None)
def kernel_acc(L, S, seed=0):
    """[3, L, ld] fp32, made once and never written: N(0, 1) in the columns [0, S), NaN in the pad columns; ld as
    ``region_cases.kernel_bias``'s (always some pad columns)"""
    ld = RC.kernel_bias(L, S).shape[-1]
    a = torch.randn(3, L, ld, generator=torch.Generator().manual_seed(31 * L + S + seed))
    a[..., S:] = float("nan")
    return a


# ---- the oracle with recording layers ----------------------------------------------------------------------------------
def recorded_attention_layer(orig, sd, pfx, x, cond, cond_mask, heads, store, rp=None):
    """``unet_oracle.attention_layer`` (or, with ``rp``, ``region_cases.biased_attention_layer``), which first adds the
    text term's head-mean probabilities of every batch row, fp64 from the oracle's own q and k_c, to
    ``store[(H, W)] = [sum [B, H W, S], layers]``"""
    import torch.nn.functional as F

    B, C, H, W = x.shape
    qkv = O._conv(sd, pfx + "qkv", O._gn(sd, pfx + "norm", x, 32)).reshape(B, 3 * C, H * W)
    D = cond.shape[-1]
    cn = F.layer_norm(cond, (D,), sd[pfx + "norm_cond.weight"], sd[pfx + "norm_cond.bias"], 1e-5)
    kv = O._linear(sd, pfx + "kv_cond", cn).transpose(1, 2)
    p, _ = probs_ref(qkv[:, :C], kv[:, :C], heads, cond_mask, None if rp is None else rp.bias(B, H, W))
    ent = store.setdefault((H, W), [torch.zeros_like(p), 0])
    ent[0] += p
    ent[1] += 1
    if rp is not None:
        return RC.biased_attention_layer(sd, pfx, x, cond, cond_mask, heads, rp)
    return orig(sd, pfx, x, cond, cond_mask, heads)


@contextlib.contextmanager
def recording_oracle(sd, names, store, rp=None):
    """Inside, ``unet_oracle.attention_layer`` records the layers ``names`` of the state dict ``sd`` into ``store``
    (recognised by the identity of their qkv weight, as ``pag_cases.perturbed_oracle``)"""
    ids = {id(sd[n + ".qkv.weight"]) for n in names}
    orig = O.attention_layer

    def layer(sd_, pfx, x, cond, cond_mask, heads=8):
        if id(sd_[pfx + "qkv.weight"]) in ids:
            return recorded_attention_layer(orig, sd_, pfx, x, cond, cond_mask, heads, store, rp)
        return orig(sd_, pfx, x, cond, cond_mask, heads)

    O.attention_layer = layer
    try:
        yield
    finally:
        O.attention_layer = orig


@functools.lru_cache(maxsize=None)
def oracle_maps(name, names):
    """fp32 oracle forward of ``pag_cases.model_inputs(name)`` (batch 4) recording the layers ``names`` -> ({(h, w): fp64
    [4, S, h, w], the mean over the layers}, list of outputs)"""
    _, cfg, sd = PC.build_module(name)
    inp = PG.model_inputs(name)
    store = {}
    with torch.no_grad(), recording_oracle(sd, names, store):
        outs = O.model_forward(sd, cfg, inp["x"], inp["times"], inp["cond"], inp["mask"], {})
    maps = {(h, w): (t / n).transpose(1, 2).reshape(t.shape[0], t.shape[2], h, w) for (h, w), (t, n) in store.items()}
    return maps, [o.detach() for o in PC.as_list(outs)]


# ---- a stub denoiser that records the handle it sees -------------------------------------------------------------------
class RecordingStub(RC.RecordingStub):
    """``region_cases.RecordingStub`` (three attention layers, two with text keys); every call also records which layers
    carry an ``_attn_rec`` handle, and the rows it stands for: (row0, rows, total)"""

    def __init__(self, nested=False):
        super().__init__(nested)
        self.rec_seen = []

    def forward(self, x, t, lm, mask, micros={}):
        self.rec_seen.append({n: (None if m._attn_rec is None else (m._attn_rec.row0, m._attn_rec.rows, m._attn_rec.total))
                              for n, m in self.attention().items()})
        return super().forward(x, t, lm, mask, micros)
