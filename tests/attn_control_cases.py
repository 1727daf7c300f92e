"""Cases shared by the attention-control tests (CPU and GPU): the fp64 restatement of the controlled layer

    out_h[r] = A_h(g_s ? s : r) v_h[r] + P_h(s) V'_h[r] + P_h(r) V''_h[r]

written with per-head einsums and independently of ``mdm_hip/attn_control.py``; the oracle's attention layer with it, a context
that swaps it into the imported oracle module by layer; seeded kernel inputs (NaN in the pad columns of M, a masked edit token
whose M column is large, a source row with a holed mask); model inputs for a batch of 4 with source = [0, 1, 0, 1] whose rows 2
and 3 carry the OTHER row's text states; and a stub denoiser that notes the handle and the gates it sees."""
import contextlib
import functools
import math

import torch

import pag_cases as PG
import parity_cases as PC
import unet_oracle as O


# ---- the formula ------------------------------------------------------------------------------------------------------
def self_probs(q, k, heads):
    """fp64 A_h = softmax(q_h k_h^T / sqrt(d)).  q, k [L, C] -> [H, L, L]"""
    L, C = q.shape
    d = C // heads
    qh, kh = q.double().reshape(L, heads, d), k.double().reshape(L, heads, d)
    return torch.softmax(torch.einsum("lhd,mhd->hlm", qh, kh) / math.sqrt(d), dim=-1)


def text_probs(q, kc, heads, mask):
    """fp64 P_h = softmax over the live keys (mask != 0) of q_h k_c,h^T / sqrt(d); no live key: a zero row.
    q [L, C], kc [S, C], mask [S] or None -> [H, L, S]"""
    L, C = q.shape
    S, d = kc.shape[0], C // heads
    logits = torch.einsum("lhd,shd->hls", q.double().reshape(L, heads, d), kc.double().reshape(S, heads, d)) / math.sqrt(d)
    if mask is None:
        return torch.softmax(logits, dim=-1)
    live = mask != 0
    if not bool(live.any()):
        return torch.zeros_like(logits)
    return torch.softmax(logits.masked_fill(~live[None, None, :], float("-inf")), dim=-1)


def apply_probs(p, v, heads):
    """p [H, L, K], v [K, C] -> [L, C]"""
    K, C = v.shape
    return torch.einsum("hlk,khd->lhd", p, v.double().reshape(K, heads, C // heads)).reshape(p.shape[1], C)


def mixed_values(vc, M, D, mask, g_c):
    """fp64 (V', V'') of one edited row.  vc [S, C]; M [S, >= S] (row = source token, column = edit token; entries of masked
    columns and of the columns past S are SELECTED away, never multiplied); D [S]; mask [S] of the edited row or None"""
    S = vc.shape[0]
    vc = vc.double()
    live = torch.ones(S, dtype=torch.bool) if mask is None else mask != 0
    Mr = torch.where(live[None, :], M[:, :S].double(), torch.zeros(S, S, dtype=torch.float64))
    v_live = torch.where(live[:, None], vc, torch.zeros_like(vc))
    va = g_c * (Mr @ v_live)
    vb = (g_c * D.double() + 1 - g_c)[:, None] * vc
    return va, vb


def mix_kv_ref(kvc, own, src, M, D, mask, gate):
    """fp64 (kv_a, kv_b) [R, S, 2C] of ``mdm_ctrl_mix_kv``"""
    C = kvc.shape[-1] // 2
    a, b = [], []
    for k, (r, s) in enumerate(zip(own, src)):
        va, vb = mixed_values(kvc[r, :, C:], M[k], D[k], None if mask is None else mask[r], float(gate))
        a.append(torch.cat([kvc[s, :, :C].double(), va], dim=-1))
        b.append(torch.cat([kvc[r, :, :C].double(), vb], dim=-1))
    return torch.stack(a), torch.stack(b)


def controlled_rows_ref(qkv, kvc, mask, heads, own, src, M, D, g_c, g_s):
    """fp64 [R, L, C]: the outputs of the edited rows ``own`` (absolute batch rows) with sources ``src``.
    qkv [N, L, 3C], kvc [N, S, 2C] or None, mask [N, S] or None, M [R, S, >= S], D [R, S]"""
    C = qkv.shape[-1] // 3
    out = []
    for k, (r, s) in enumerate(zip(own, src)):
        a = r if not g_s else s
        o = apply_probs(self_probs(qkv[a, :, :C], qkv[a, :, C:2 * C], heads), qkv[r, :, 2 * C:], heads)
        if kvc is not None:
            mr, ms = (None, None) if mask is None else (mask[r], mask[s])
            va, vb = mixed_values(kvc[r, :, C:], M[k], D[k], mr, float(g_c))
            o = o + apply_probs(text_probs(qkv[s, :, :C], kvc[s, :, :C], heads, ms), va, heads)
            o = o + apply_probs(text_probs(qkv[r, :, :C], kvc[r, :, :C], heads, mr), vb, heads)
        out.append(o)
    return torch.stack(out)


def ordinary_rows_ref(qkv, kvc, mask, heads, rows, perturbed=False):
    """fp64 [len(rows), L, C]: A v + P v_c, or v + P v_c for the perturbed rows of perturbed-attention guidance"""
    C = qkv.shape[-1] // 3
    out = []
    for r in rows:
        v = qkv[r, :, 2 * C:]
        o = v.double() if perturbed else apply_probs(self_probs(qkv[r, :, :C], qkv[r, :, C:2 * C], heads), v, heads)
        if kvc is not None:
            p = text_probs(qkv[r, :, :C], kvc[r, :, :C], heads, None if mask is None else mask[r])
            o = o + apply_probs(p, kvc[r, :, C:], heads)
        out.append(o)
    return torch.stack(out)


# ---- kernel inputs ------------------------------------------------------------------------------------------------------
def ld_of(S):
    """S rounded up to 4, + 4 where S is a multiple of 4 already: there always are pad columns"""
    ld = (S + 3) // 4 * 4
    return ld + 4 if ld == S else ld


@functools.lru_cache(maxsize=None)
def mix_case(S, C, R, seed=0):
    """-> dict, made once and never written: kvc [R + 1, S, 2C] (row 0 the source), own = [1 .. R], src = [0] * R, mask
    [R + 1, S] (the source and the odd edited rows holed + tail-masked, ``pag_cases.masks`` row 1; the even ones full), M
    [R, S, ld] N(0, 1/4) with NaN in the pad columns and 1e30 in the columns of an edited row's masked tokens, D [R, S]"""
    g = torch.Generator().manual_seed(131 * S + C + 7 * R + seed)
    holed = PG.masks(S)[1]
    mask = torch.stack([holed] + [holed if k % 2 == 0 else torch.ones(S) for k in range(R)])
    ld = ld_of(S)
    M = torch.randn(R, S, ld, generator=g) * 0.5
    M[:, :, S:] = float("nan")
    for k in range(R):
        M[k][:, :S][:, mask[k + 1] == 0] = 1e30
    return dict(kvc=torch.randn(R + 1, S, 2 * C, generator=g), own=list(range(1, R + 1)), src=[0] * R, mask=mask, M=M,
                D=torch.rand(R, S, generator=g) * 2, ld=ld)


@functools.lru_cache(maxsize=None)
def layer_case(d, H, L, S, seed=0):
    """N = 7 = 2 uncond + 2 sources + 2 edits + 1 perturbed: qkv [7, L, 3C], kvc [7, S, 2C], mask [7, S] (source row 2 holed,
    edited row 5 holed, the others full), own = [4, 5], src = [2, 3], M [2, S, ld] (NaN pads, 1e30 in the columns of row 5's
    masked tokens), D [2, S].  Made once, never written."""
    g = torch.Generator().manual_seed(17 * d + 3 * H + L + 1000 * S + seed)
    C = H * d
    holed = PG.masks(S)[1]
    mask = torch.ones(7, S)
    mask[2], mask[5] = holed, holed
    ld = ld_of(S)
    M = torch.randn(2, S, ld, generator=g) * (1.0 / math.sqrt(S))
    M[:, :, S:] = float("nan")
    M[1][:, :S][:, holed == 0] = 1e30
    return dict(qkv=torch.randn(7, L, 3 * C, generator=g), kvc=torch.randn(7, S, 2 * C, generator=g), mask=mask, own=[4, 5],
                src=[2, 3], M=M, D=torch.rand(2, S, generator=g), ld=ld, row0=4, pag_rows=1)


def layer_ref(case, H, g_c, g_s, masked=True):
    """fp64 [7, L, C] of ``layer_case``"""
    m = case["mask"] if masked else None
    lead = ordinary_rows_ref(case["qkv"], case["kvc"], m, H, range(4))
    mid = controlled_rows_ref(case["qkv"], case["kvc"], m, H, case["own"], case["src"], case["M"], case["D"], g_c, g_s)
    tail = ordinary_rows_ref(case["qkv"], case["kvc"], m, H, [6], perturbed=True)
    return torch.cat([lead, mid, tail])


class Rows:
    """the ``ctrl_rows`` of ``ops.attention_controlled``, built by hand"""

    def __init__(self, case, g_c, g_s, device):
        f = lambda t, dt: torch.as_tensor(t, dtype=dt).to(device).contiguous()
        self.row0, self.R, self.src_host = case["row0"], len(case["own"]), tuple(case["src"])
        self.own, self.src = f(case["own"], torch.int32), f(case["src"], torch.int32)
        self.M, self.D = f(case["M"], torch.float32), f(case["D"], torch.float32)
        self.gate_c, self.gate_s = f([float(g_c)], torch.float32), f([float(g_s)], torch.float32)


# ---- the oracle with controlled layers ------------------------------------------------------------------------------------
SOURCE = [0, 1, 0, 1]
S_TOK = 8
SELF_MAX_QUERIES = 64   # the mini models attend at 8 x 8 = 64 queries: exactly the threshold, which is inclusive


def model_control_tables():
    """(mapper, keep, scale) of rows 2 and 3: row 2 a cyclic shift of the tokens with two new tokens kept and one weight
    raised; row 3 the identity with token 1 kept at half weight"""
    m2 = torch.zeros(S_TOK, S_TOK)
    for j in range(S_TOK):
        m2[(j + 1) % S_TOK, j] = 1.0
    m2[:, 6:] = 0
    k2 = torch.zeros(S_TOK)
    k2[6:] = 1
    s2 = torch.ones(S_TOK)
    s2[2] = 1.5
    k3 = torch.zeros(S_TOK)
    k3[1] = 1
    s3 = torch.ones(S_TOK)
    s3[1] = 0.5
    return {2: m2}, {2: k2, 3: k3}, {2: s2, 3: s3}


def model_control(**kw):
    import mdm_hip

    mapper, keep, scale = model_control_tables()
    kw.setdefault("self_max_queries", SELF_MAX_QUERIES)
    return mdm_hip.AttnControl(S_TOK, SOURCE, mapper=mapper, keep=keep, scale=scale, **kw)


def model_tables():
    """the same as M [2, S, S] and D [2, S] in fp64, from the definition"""
    mapper, keep, scale = model_control_tables()
    M, D = [], []
    for r in (2, 3):
        sc = scale.get(r, torch.ones(S_TOK)).double()
        M.append(mapper.get(r, torch.eye(S_TOK)).double() * sc[None, :])
        D.append(keep.get(r, torch.zeros(S_TOK)).double() * sc)
    return torch.stack(M), torch.stack(D)


def controlled_attention_layer(sd, pfx, x, cond, cond_mask, heads, gates, cross, self_):
    """``unet_oracle.attention_layer`` whose rows 2, 3 are edits of rows 0, 1 (``SOURCE``): their attention is formed in
    fp64 from the formula; ``gates`` = (g_c, g_s) of the step, ``cross`` / ``self_``: is the layer in the two sets"""
    import torch.nn.functional as F

    B, C, H, W = x.shape
    qkv = O._conv(sd, pfx + "qkv", O._gn(sd, pfx + "norm", x, 32)).reshape(B, 3 * C, H * W)
    q, k, v = qkv[:, :C], qkv[:, C: 2 * C], qkv[:, 2 * C:]
    kv = None
    h = O.attention_core(q[:2], k[:2], v[:2], heads)
    if (pfx + "kv_cond.weight") in sd:
        Dm = cond.shape[-1]
        cn = F.layer_norm(cond, (Dm,), sd[pfx + "norm_cond.weight"], sd[pfx + "norm_cond.bias"], 1e-5)
        kv = O._linear(sd, pfx + "kv_cond", cn).transpose(1, 2)
        h = h + O.attention_core(q[:2], kv[:2, :C], kv[:2, C:], heads, None if cond_mask is None else cond_mask[:2])
    g_c = gates[0] if (cross and kv is not None) else 0.0
    g_s = gates[1] if (self_ and H * W <= SELF_MAX_QUERIES) else 0.0
    M, D = model_tables()
    edits = controlled_rows_ref(qkv.transpose(1, 2), None if kv is None else kv.transpose(1, 2), cond_mask, heads, [2, 3],
                                [0, 1], M, D, g_c, g_s)
    h = torch.cat([h, edits.transpose(1, 2).to(h.dtype)])
    x = x + O._conv(sd, pfx + "proj_out", h.reshape(B, C, H, W))
    if (pfx + "ffn.1.weight") in sd:
        f = O._conv(sd, pfx + "ffn.1", O._gn(sd, pfx + "ffn.0", x, 32))
        x = x + O._conv(sd, pfx + "ffn.3", F.gelu(f))
    return x


@contextlib.contextmanager
def controlled_oracle(sd, names_cross, names_self, gates):
    """Inside, ``unet_oracle.attention_layer`` controls the layers of either set (module names of the whole model; recognised
    by the identity of their qkv weight, as ``pag_cases.perturbed_oracle``)"""
    ids_c = {id(sd[n + ".qkv.weight"]) for n in names_cross}
    ids_s = {id(sd[n + ".qkv.weight"]) for n in names_self}
    orig = O.attention_layer

    def layer(sd_, pfx, x, cond, cond_mask, heads=8):
        w = id(sd_[pfx + "qkv.weight"])
        if w in ids_c or w in ids_s:
            return controlled_attention_layer(sd_, pfx, x, cond, cond_mask, heads, gates, w in ids_c, w in ids_s)
        return orig(sd_, pfx, x, cond, cond_mask, heads)

    O.attention_layer = layer
    try:
        yield
    finally:
        O.attention_layer = orig


def model_inputs(name):
    """batch 4 from the parity case: rows 2, 3 repeat the images and times of rows 0, 1 and carry the text states and the mask
    of the OTHER row (row 2: row 1's, row 3: row 0's) -- an edit under another prompt"""
    inp = PC.inputs(name)
    two = lambda t: torch.cat([t, t])
    swap = lambda t: torch.cat([t, t.flip(0)])
    x = [two(t) for t in inp["x"]] if isinstance(inp["x"], list) else two(inp["x"])
    return dict(x=x, times=two(inp["times"]), cond=swap(inp["cond"]), mask=swap(inp["mask"]))


def all_names(name):
    model = PC.build_module(name)[0]
    return model_control().layer_sets(model)


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, gates):
    """fp32 oracle forward of ``model_inputs(name)``; ``gates``: None = the uncontrolled oracle, else (g_c, g_s) with every
    layer in both sets -> list of outputs"""
    _, cfg, sd = PC.build_module(name)
    inp = model_inputs(name)
    cross, self_ = all_names(name) if gates is not None else ((), ())
    with torch.no_grad(), controlled_oracle(sd, cross, self_, gates):
        outs = O.model_forward(sd, cfg, inp["x"], inp["times"], inp["cond"], inp["mask"], {})
    return [o.detach() for o in PC.as_list(outs)]


# ---- a stub denoiser that records the handle and the gates it sees --------------------------------------------------------
class RecordingStub(PG.RecordingStub):
    """``pag_cases.RecordingStub`` with a second attention layer that has text keys and one that has none; every call records,
    per layer, None or (cross, self, row0, R, source rows, total, g_c, g_s) of its ``_attn_ctrl``"""

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
        def note(c):
            if c is None:
                return None
            h = c.handle
            return (c.cross, c.self_, h.row0, h.R, h.src_host, h.total, float(h.gate_c), float(h.gate_s))

        self.seen.append({n: note(m._attn_ctrl) for n, m in self.attention().items()})
        return super().forward(x, t, lm, mask, micros)
