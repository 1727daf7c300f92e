"""Cases shared by the regional-prompt tests (CPU and GPU): the fp64 restatement of the biased text cross-attention
(``out = base + softmax(logits + bias; live keys) v_c``), the oracle's attention layer with that bias, a context that swaps it
into the imported oracle module by layer, seeded kernel inputs and the model inputs with two regional spans."""
import contextlib
import functools
import math

import torch

import pag_cases as PG
import parity_cases as PC
import unet_oracle as O

NEG_INF = float("-inf")


# ---- the kernel ----------------------------------------------------------------------------------------------------
def cross_term_ref(q, kc, vc, heads, mask, bias):
    """fp64 cross term.  q [B, C, L], kc / vc [B, C, S], mask [B, S] or None, bias [B, L, >= S] or None -> ([B, C, L], live
    [B, L]): logits q.k/sqrt(d) + bias, then exclusion (mask == 0, or bias <= -1e30); a query with no live key gets 0."""
    B, C, L = q.shape
    S = kc.shape[-1]
    d = C // heads
    s = 1.0 / math.sqrt(math.sqrt(d))   # both sides scaled by d^-1/4, as unet_oracle.attention_core
    qh = (q.double() * s).reshape(B, heads, d, L)
    kh = (kc.double() * s).reshape(B, heads, d, S)
    vh = vc.double().reshape(B, heads, d, S)
    logits = torch.einsum("bhdl,bhds->bhls", qh, kh)
    live = torch.ones(B, L, S, dtype=torch.bool)
    if bias is not None:
        b = bias[:, :, :S].double()
        live = live & (b > -1e30)
        logits = logits + torch.where(live, b, torch.zeros_like(b))[:, None]
    if mask is not None:
        live = live & (mask != 0)[:, None, :]
    logits = logits.masked_fill(~live[:, None], NEG_INF)
    any_live = live.any(dim=-1)                                    # [B, L]
    probs = torch.softmax(torch.where(any_live[:, None, :, None], logits, torch.zeros_like(logits)), dim=-1)
    probs = torch.where(any_live[:, None, :, None], probs, torch.zeros_like(probs))
    out = torch.einsum("bhds,bhls->bhdl", vh, probs)
    return out.reshape(B, C, L), any_live


def cross_bias_ref(qkv, kvc, mask, bias, heads, base=None):
    """fp64: out = base + softmax_S(q k_c^T / sqrt(d) + bias; live keys) v_c.  qkv [B, L, 3C], kvc [B, S, 2C], mask [B, S]
    or None, bias [B, L, ld >= S] (columns past S ignored), base [B, L, C] or None = v -> [B, L, C]."""
    qkv = qkv.double()
    C = qkv.shape[-1] // 3
    q = qkv[..., :C].transpose(1, 2)
    base = qkv[..., 2 * C:] if base is None else base.double()
    kv = kvc.double().transpose(1, 2)
    cross, _ = cross_term_ref(q, kv[:, :C], kv[:, C:], heads, mask, bias)
    return (base + cross.transpose(1, 2)).contiguous()


@functools.lru_cache(maxsize=None)
def kernel_bias(L, S, seed=0):
    """[3, L, ld] fp32, made once and never written: N(0, 2) with about a quarter of the entries -inf; batch row 1 is all
    zero; in batch row 2 the queries [L // 4, L // 4 + max(L // 8, 1)) have every key excluded; the pad columns [S, ld)
    hold NaN.  ld = S rounded up to 4, + 4 where S is a multiple of 4 already (so that there always are pad columns)."""
    g = torch.Generator().manual_seed(77 * L + S + seed)
    ld = (S + 3) // 4 * 4
    ld = ld + 4 if ld == S else ld
    b = torch.randn(3, L, ld, generator=g) * 2.0
    b[torch.rand(3, L, ld, generator=g) < 0.25] = NEG_INF
    b[1] = 0.0
    lo = L // 4
    b[2, lo: lo + max(L // 8, 1)] = NEG_INF
    b[:, :, S:] = float("nan")
    return b


def dead_band(L):
    lo = L // 4
    return lo, lo + max(L // 8, 1)


# ---- the oracle with biased layers -----------------------------------------------------------------------------------
def biased_attention_layer(sd, pfx, x, cond, cond_mask, heads, rp, pag_rows=0):
    """``unet_oracle.attention_layer`` with ``rp.bias(B, H, W)`` added to the text logits (and, as
    ``pag_cases.perturbed_attention_layer``, the self term of the trailing ``pag_rows`` rows replaced by v)"""
    import torch.nn.functional as F

    B, C, H, W = x.shape
    qkv = O._conv(sd, pfx + "qkv", O._gn(sd, pfx + "norm", x, 32)).reshape(B, 3 * C, H * W)
    q, k, v = qkv[:, :C], qkv[:, C: 2 * C], qkv[:, 2 * C:]
    n = B - pag_rows
    h = torch.cat([O.attention_core(q[:n], k[:n], v[:n], heads), v[n:]])
    if (pfx + "kv_cond.weight") in sd:
        D = cond.shape[-1]
        cn = F.layer_norm(cond, (D,), sd[pfx + "norm_cond.weight"], sd[pfx + "norm_cond.bias"], 1e-5)
        kv = O._linear(sd, pfx + "kv_cond", cn).transpose(1, 2)
        cross, _ = cross_term_ref(q, kv[:, :C], kv[:, C:], heads, cond_mask, rp.bias(B, H, W))
        h = h + cross.to(h.dtype)
    x = x + O._conv(sd, pfx + "proj_out", h.reshape(B, C, H, W))
    if (pfx + "ffn.1.weight") in sd:
        f = O._conv(sd, pfx + "ffn.1", O._gn(sd, pfx + "ffn.0", x, 32))
        x = x + O._conv(sd, pfx + "ffn.3", F.gelu(f))
    return x


@contextlib.contextmanager
def biased_oracle(sd, names, rp):
    """Inside, ``unet_oracle.attention_layer`` biases the layers ``names`` of the state dict ``sd`` (recognised by the
    identity of their qkv weight, as ``pag_cases.perturbed_oracle``)"""
    ids = {id(sd[n + ".qkv.weight"]) for n in names}
    orig = O.attention_layer

    def layer(sd_, pfx, x, cond, cond_mask, heads=8):
        if id(sd_[pfx + "qkv.weight"]) in ids:
            return biased_attention_layer(sd_, pfx, x, cond, cond_mask, heads, rp)
        return orig(sd_, pfx, x, cond, cond_mask, heads)

    O.attention_layer = layer
    try:
        yield
    finally:
        O.attention_layer = orig


def side_of(name):
    return 32 if name == "mini_nested" else 16


def seam_regions(side, rows=2, feather=4):
    """(left, right): [rows, 1, side, side] in [0, 1], left + right = 1, a linear ramp ``feather`` pixels wide at the seam"""
    x = torch.arange(side, dtype=torch.float32) + 0.5
    left = ((side / 2 + feather / 2 - x) / feather).clamp(0, 1)
    left = left.reshape(1, 1, 1, side).expand(rows, 1, side, side).contiguous()
    return left, 1 - left


def model_spans(name, S=8, seed=None):
    """two spans that split the case's S tokens in half: left region weight 1, right region weight 1.5, a feathered seam"""
    left, right = seam_regions(side_of(name))
    return [(0, S // 2, left, 1.0), (S // 2, S, right, 1.5)]


def model_regions(name, device=None):
    import mdm_hip

    return mdm_hip.RegionPrompts(8, side_of(name), model_spans(name), rows=2, device=device)


def model_inputs(name):
    """batch 4 from the parity case (rows 2, 3 repeat rows 0, 1): under ``model_regions`` -- [uncond | cond] -- rows 0-1
    get zero bias, rows 2-3 the two spans"""
    return PG.model_inputs(name)


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, names):
    """fp32 oracle forward of ``model_inputs(name)`` with the layers ``names`` (a tuple; empty = none) biased by
    ``model_regions(name)`` -> list of outputs"""
    _, cfg, sd = PC.build_module(name)
    inp = model_inputs(name)
    rp = model_regions(name)
    with torch.no_grad(), biased_oracle(sd, names, rp):
        outs = O.model_forward(sd, cfg, inp["x"], inp["times"], inp["cond"], inp["mask"], {})
    return [o.detach() for o in PC.as_list(outs)]


# ---- a stub denoiser that records the handle it sees ---------------------------------------------------------------------
class RecordingStub(PG.RecordingStub):
    """``pag_cases.RecordingStub`` with a second attention layer that has text keys and one that has none; every call
    records which of them carry a ``_cross_bias`` handle, and the handle's rows"""

    def __init__(self, nested=False):
        super().__init__(nested)
        import mdm_hip

        blk = torch.nn.Module()
        blk.attn = torch.nn.ModuleList([mdm_hip.unet.SelfAttention(32, cond_dim=8), mdm_hip.unet.SelfAttention(32)])
        self.down_blocks = torch.nn.ModuleList([blk])
        self.seen = []

    def attention(self):
        return {n: m for n, m in self.named_modules() if isinstance(m, type(self.mid_blocks[0].attn[0]))}

    def forward(self, x, t, lm, mask, micros={}):
        self.seen.append({n: (None if m._cross_bias is None else (m._cross_bias.rows, m._cross_bias.layout))
                          for n, m in self.attention().items()})
        return super().forward(x, t, lm, mask, micros)
