"""Cases shared by the perturbed-attention-guidance tests (CPU and GPU): fp64 restatements of the perturbed attention
(``out = v + cross``) and of the combine, the oracle's ``attention_layer`` with the self term replaced by ``v`` for a range
of batch rows, a context that swaps it into the imported oracle module by layer, and seeded inputs."""
import contextlib
import functools

import torch

import parity_cases as PC
import unet_oracle as O


# ---- the kernel ----------------------------------------------------------------------------------------------------
def cross_addv_ref(qkv, kvc, mask, heads):
    """fp64: out = v + softmax_S(q k_c^T / sqrt(d), masked) v_c.  qkv [B, L, 3C], kvc [B, S, 2C] or None, mask [B, S] or
    None -> [B, L, C].  The cross term is ``unet_oracle.attention_core``; a batch row whose keys are ALL masked has no cross
    term (the oracle's softmax of an empty set is NaN there; the kernels define it as zero, mdm_attn_fwd alike)."""
    qkv = qkv.double()
    C = qkv.shape[-1] // 3
    q, v = qkv[..., :C].transpose(1, 2), qkv[..., 2 * C:].transpose(1, 2)   # [B, C, L]
    out = v
    if kvc is not None:
        kv = kvc.double().transpose(1, 2)                                   # [B, 2C, S]
        cross = O.attention_core(q, kv[:, :C], kv[:, C:], heads, None if mask is None else mask.double())
        if mask is not None:
            live = (mask != 0).any(dim=1)
            cross = torch.where(live[:, None, None], cross, torch.zeros_like(cross))
        out = v + cross
    return out.transpose(1, 2).contiguous()


def masks(S, kind="mixed"):
    """[3, S]: one full row, one with holes in the middle and a masked tail, one fully masked"""
    m = torch.ones(3, S)
    m[1, S // 3:: 3] = 0
    m[1, (3 * S) // 4 + 1:] = 0
    m[2] = 0
    return m


@functools.lru_cache(maxsize=None)
def attn_inputs(L, S, H, d, seed=0):
    """qkv [3, L, 3C], kvc [3, S, 2C] fp32, made once and never written"""
    g = torch.Generator().manual_seed(1000 * L + 10 * S + H + d + seed)
    C = H * d
    return torch.randn(3, L, 3 * C, generator=g), torch.randn(3, S, 2 * C, generator=g)


# ---- the combine ---------------------------------------------------------------------------------------------------
def combine_ref(pc, pu, pp, w, s):
    """fp64: p_u + w (p_c - p_u) + s (p_c - p_hat); p_c in front where there is no p_u"""
    pc, pp = pc.double(), pp.double()
    base = pc if pu is None else pu.double() + w * (pc - pu.double())
    return base + s * (pc - pp)


def combine_scale(pc, pu, pp, w, s):
    """what the combine's rounding errors are relative to: |p_u| + |w| |p_c - p_u| + |s| |p_c - p_hat|"""
    pc, pp = pc.double(), pp.double()
    base = pc.abs() if pu is None else pu.double().abs() + abs(w) * (pc - pu.double()).abs()
    return base + abs(s) * (pc - pp).abs()


# ---- the oracle with perturbed layers --------------------------------------------------------------------------------
def perturbed_attention_layer(sd, pfx, x, cond, cond_mask, heads=8, rows=0):
    """``unet_oracle.attention_layer`` with the self-attention map of the trailing ``rows`` batch rows replaced by the
    identity: their self term is v"""
    import torch.nn.functional as F

    B, C, H, W = x.shape
    qkv = O._conv(sd, pfx + "qkv", O._gn(sd, pfx + "norm", x, 32)).reshape(B, 3 * C, H * W)
    q, k, v = qkv[:, :C], qkv[:, C: 2 * C], qkv[:, 2 * C:]
    h = torch.cat([O.attention_core(q[: B - rows], k[: B - rows], v[: B - rows], heads), v[B - rows:]])
    if (pfx + "kv_cond.weight") in sd:
        D = cond.shape[-1]
        cn = F.layer_norm(cond, (D,), sd[pfx + "norm_cond.weight"], sd[pfx + "norm_cond.bias"], 1e-5)
        kv = O._linear(sd, pfx + "kv_cond", cn).transpose(1, 2)
        h = h + O.attention_core(q, kv[:, :C], kv[:, C:], heads, cond_mask)
    x = x + O._conv(sd, pfx + "proj_out", h.reshape(B, C, H, W))
    if (pfx + "ffn.1.weight") in sd:
        f = O._conv(sd, pfx + "ffn.1", O._gn(sd, pfx + "ffn.0", x, 32))
        x = x + O._conv(sd, pfx + "ffn.3", F.gelu(f))
    return x


@contextlib.contextmanager
def perturbed_oracle(sd, names, rows):
    """Inside, ``unet_oracle.attention_layer`` perturbs the layers ``names`` (module names of the whole model, e.g.
    ``inner_unet.mid_blocks.0.attn.0``) of the state dict ``sd``.  The oracle hands a nested net a sub-dict of the SAME
    tensors under shortened keys, so a layer is recognised by the identity of its qkv weight, not by its prefix alone."""
    ids = {id(sd[n + ".qkv.weight"]) for n in names}
    orig = O.attention_layer

    def layer(sd_, pfx, x, cond, cond_mask, heads=8):
        if id(sd_[pfx + "qkv.weight"]) in ids:
            return perturbed_attention_layer(sd_, pfx, x, cond, cond_mask, heads, rows)
        return orig(sd_, pfx, x, cond, cond_mask, heads)

    O.attention_layer = layer
    try:
        yield
    finally:
        O.attention_layer = orig


def model_inputs(name):
    """the parity case's inputs twice: a batch of 4 whose rows 2, 3 repeat rows 0, 1"""
    inp = PC.inputs(name)
    two = lambda t: torch.cat([t, t])
    x = [two(t) for t in inp["x"]] if isinstance(inp["x"], list) else two(inp["x"])
    return dict(x=x, times=two(inp["times"]), cond=two(inp["cond"]), mask=two(inp["mask"]))


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, names, rows=2):
    """fp32 oracle forward of ``model_inputs(name)`` with the layers ``names`` (a tuple; empty = none) perturbed on the
    trailing ``rows`` rows -> list of outputs"""
    _, cfg, sd = PC.build_module(name)
    inp = model_inputs(name)
    with torch.no_grad(), perturbed_oracle(sd, names, rows):
        outs = O.model_forward(sd, cfg, inp["x"], inp["times"], inp["cond"], inp["mask"], {})
    return [o.detach() for o in PC.as_list(outs)]


# ---- a stub denoiser that records its calls, with one real (never run) attention layer to select -------------------------
class RecordingStub(torch.nn.Module):
    """``model(x, t, lm_outputs, lm_mask, micros)`` as the samplers call it: a row-wise function of (x, t, text, micros),
    plus a term that depends on whether the row is perturbed (``_pag_rows`` of the stub's mid-block attention layer at the
    time of the call), so that the three blocks of a batch come out distinct.  Every call is recorded."""

    def __init__(self, nested=False):
        super().__init__()
        import mdm_hip

        self.nested = nested
        blk = torch.nn.Module()
        blk.attn = torch.nn.ModuleList([mdm_hip.unet.SelfAttention(32, cond_dim=8)])
        self.mid_blocks = torch.nn.ModuleList([blk])
        self.nest_ratio = [1]   # two scales of one size: unit image scales, one schedule
        self.calls = []

    @property
    def vision_model(self):
        return self

    def one(self, x, t, lm, micros, k):
        n = x.shape[0]
        rows = self.mid_blocks[0].attn[0]._pag_rows
        pert = torch.zeros(n, 1, 1, 1)
        if rows:
            pert[n - rows:] = 1
        c = lm.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        m = micros["scale"].reshape(-1, 1, 1, 1) / 64.0 if "scale" in micros else 0.0
        tt = (t.float() / 1000.0).reshape(-1, 1, 1, 1)
        return (0.3 + 0.1 * k) * x + 0.1 * torch.tanh(3 * tt) + 0.4 * c + 0.05 * m + pert * (0.2 * torch.roll(x, 1, dims=-1) - 0.1)

    def forward(self, x, t, lm, mask, micros={}):
        self.calls.append(dict(x=[v.clone() for v in x] if self.nested else x.clone(), t=t.clone(), lm=lm.clone(),
                               mask=None if mask is None else mask.clone(),
                               micros={k: v.clone() if torch.is_tensor(v) else v for k, v in micros.items()},
                               pag_rows=self.mid_blocks[0].attn[0]._pag_rows))
        if self.nested:
            return [self.one(v, t, lm, micros, k) for k, v in enumerate(x)]
        out = self.one(x, t, lm, micros, 0)
        return out, torch.ones_like(out)
