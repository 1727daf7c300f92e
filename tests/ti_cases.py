"""Textual-inversion cases shared by the CPU tests, the GPU tests and tools/make_t5_grad_golden.py.

Two things live here.

* fp64 torch restatements of the four backward formulas the HIP kernels implement (attention from the saved log-sum-exp,
  gated GELU, RMS norm, embedding reduce).  The host tests pin each one to autograd of the forward formula in
  ``t5_cases``; the GPU kernel tests compare the kernels with these restatements.
* The gradient cases of the whole encoder: loss = sum(out * G) with a seeded cotangent G per input draw, differentiated
  by torch autograd through ``t5_cases.oracle_forward`` in fp64 -- with respect to the embedding table (a leaf), or to
  one embedding row per position (dx0).
"""
import os

import numpy as np
import torch

import t5_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_grad.pt")
# fp32: every case whose reference (transformers, fp32, CPU) is a factor ten under the 1e-3 gradient gate; deep24 is not a
# gradient case (fp32 torch alone is at 1e-4 on it).  bf16: on the mini cases the reference itself is at 0.18.
GRAD_CASES = ["mini", "mini_holes", "xl2", "deep24_t5init"]
BF16_GRAD_CASES = ["xl2", "deep24_t5init"]
GRAD_GATE = 1e-3
K_TANH = 0.7978845608028654     # the forward kernel's sqrt(2 / pi)


# ---------------------------------------------------------------------------------------------------------------------
# restatements of the backward formulas, fp64
# ---------------------------------------------------------------------------------------------------------------------
def _rows(pk):
    for b in range(pk["B"]):
        t0, t1 = int(pk["seq_start"][b]), int(pk["seq_start"][b + 1])
        if t1 > t0:
            yield b, t0, t1


def attn_forward(qkv, pk, table, H, S):
    """packed qkv [T, 3 H 64] -> (out [T, H 64], lse [H, T]) in fp64; table [H, 2S-1]"""
    d = 64
    qkv, table = qkv.double(), table.double()
    T = pk["T"]
    out, lse = torch.zeros(T, H * d, dtype=torch.float64), torch.zeros(H, T, dtype=torch.float64)
    pos = torch.from_numpy(np.asarray(pk["pos"])).long()
    for _, t0, t1 in _rows(pk):
        rel = pos[t0:t1][None, :] - pos[t0:t1][:, None] + (S - 1)            # [q, k]
        for h in range(H):
            q, k, v = (qkv[t0:t1, i * H * d + h * d:i * H * d + (h + 1) * d] for i in range(3))
            s = q @ k.t() + table[h][rel]
            lse[h, t0:t1] = torch.logsumexp(s, dim=-1)
            out[t0:t1, h * d:(h + 1) * d] = torch.softmax(s, dim=-1) @ v
    return out, lse


def attn_backward(qkv, out, lse, dout, pk, table, H, S):
    """dqkv [T, 3 H 64] from the SAVED out and lse, as mdm_t5_attn_bwd forms it:
    P = exp(q k^T + bias - lse), delta = rowsum(dO o O), dV = P^T dO, dS = P o (dO V^T - delta), dQ = dS K, dK = dS^T Q"""
    d = 64
    qkv, out, lse, dout, table = qkv.double(), out.double(), lse.double(), dout.double(), table.double()
    dqkv = torch.zeros_like(qkv)
    pos = torch.from_numpy(np.asarray(pk["pos"])).long()
    for _, t0, t1 in _rows(pk):
        rel = pos[t0:t1][None, :] - pos[t0:t1][:, None] + (S - 1)
        for h in range(H):
            cq, ck, cv = (slice(i * H * d + h * d, i * H * d + (h + 1) * d) for i in range(3))
            co = slice(h * d, (h + 1) * d)
            q, k, v = qkv[t0:t1, cq], qkv[t0:t1, ck], qkv[t0:t1, cv]
            do, o = dout[t0:t1, co], out[t0:t1, co]
            p = torch.exp(q @ k.t() + table[h][rel] - lse[h, t0:t1, None])
            delta = (do * o).sum(-1, keepdim=True)
            ds = p * (do @ v.t() - delta)
            dqkv[t0:t1, cq] = ds @ k
            dqkv[t0:t1, ck] = ds.t() @ q
            dqkv[t0:t1, cv] = p.t() @ do
    return dqkv


def gelu_new_grad(a):
    """d gelu_new / da, tanh form"""
    t = torch.tanh(K_TANH * (a + 0.044715 * a ** 3))
    return 0.5 * (1.0 + t) + 0.5 * a * (1.0 - t * t) * K_TANH * (1.0 + 3 * 0.044715 * a * a)


def gated_gelu_backward(u, dy):
    """u [T, 2F], dy [T, F] -> du [T, 2F] of y = gelu_new(u[:, :F]) * u[:, F:]"""
    u, dy = u.double(), dy.double()
    F = dy.shape[1]
    a, b = u[:, :F], u[:, F:]
    return torch.cat([dy * b * gelu_new_grad(a), dy * TC.gelu_new(a)], dim=1)


def rms_backward(x, w, dh, eps):
    """input gradient of h = w * x * rsqrt(mean(x^2) + eps): rs (w dh) - x rs^3 / D sum(w dh x)"""
    x, w, dh = x.double(), w.double(), dh.double()
    D = x.shape[-1]
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    wg = w * dh
    return rs * wg - x * rs ** 3 / D * (wg * x).sum(-1, keepdim=True)


def slot_index(ids, token_ids):
    """inverted index of the packed ids [n_tokens] over the placeholder ids: (slot_start [P + 1], tokens [n]) int32, a
    slot's tokens ascending -- what the host builds for mdm_t5_embed_bwd"""
    ids = np.asarray(ids).reshape(-1)
    lists = [np.flatnonzero(ids == t) for t in token_ids]
    start = np.zeros(len(token_ids) + 1, dtype=np.int32)
    np.cumsum([len(l) for l in lists], out=start[1:])
    tokens = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return start, tokens


def embed_backward(dx0, slot_start, tokens, dtype=torch.float64):
    """dlearned [P, D]: per slot the sum of dx0 over its tokens, sequentially in list order, in ``dtype``"""
    P = len(slot_start) - 1
    out = torch.zeros(P, dx0.shape[1], dtype=dtype)
    dx0 = dx0.to(dtype)
    for j in range(P):
        for k in range(int(slot_start[j]), int(slot_start[j + 1])):
            out[j] = out[j] + dx0[int(tokens[k])]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# gradient cases of the whole encoder
# ---------------------------------------------------------------------------------------------------------------------
def cotangents(name):
    """G [DRAWS, B, S, D] fp32, seeded and fixed per draw; zero at masked positions so that it is a cotangent of what
    the encoder returns"""
    c = TC.CASES[name]
    m = TC.mask_of(name)
    G = torch.randn((TC.DRAWS,) + tuple(m.shape) + (c["cfg"]["d_model"],), generator=TC._gen(name, "cotangent"))
    return G * m[None, :, :, None]


def oracle_table_grad(sd, cfg, ids, mask, G, table=None, dtype=torch.float64):
    """d sum(out * G) / d table through the oracle; ``table`` (default: the case's) may have rows beyond the vocabulary"""
    table = (sd["shared.weight"] if table is None else table).to(dtype).clone().requires_grad_(True)
    sd = dict(sd)
    sd["shared.weight"] = table
    out = TC.oracle_forward(sd, cfg, ids, mask, dtype)
    (out * G.to(dtype)).sum().backward()
    return table.grad


def oracle_dx0(sd, cfg, ids, mask, G, dtype=torch.float64):
    """d sum(out * G) / d x0 [B, S, D]: the oracle run on a table with one row per position"""
    B, S = ids.shape
    rows = sd["shared.weight"].to(dtype)[ids.reshape(-1)].clone().requires_grad_(True)
    sd = dict(sd)
    sd["shared.weight"] = rows
    out = TC.oracle_forward(sd, cfg, torch.arange(B * S).view(B, S), mask, dtype)
    (out * G.to(dtype)).sum().backward()
    return rows.grad.view(B, S, -1)


_grad_cache = {}


def oracle_table_grads(name):
    """[DRAWS, vocab, D] fp64 table gradients of the case (computed once per process, never modified)"""
    if name not in _grad_cache:
        cfg, sd = TC.config(name), TC.weights(name)
        ids, m = TC.inputs(name)
        G = cotangents(name)
        _grad_cache[name] = torch.stack([oracle_table_grad(sd, cfg, ids[i], m, G[i]) for i in range(TC.DRAWS)])
    return _grad_cache[name]


def subsample_dx0(dx0, name):
    """what the fixture keeps of dx0 [B, S, D]: every ``sub``-th channel of the valid rows"""
    return TC.valid_rows(dx0, TC.mask_of(name))[..., :: TC.CASES[name]["sub"]].double().contiguous()
