"""GPU: the T5 text-encoder kernels (csrc/text_encoder.hip) one by one against torch on the CPU, and
mdm_hip.T5Encoder / LanguageModel against the fp64 oracle of t5_cases.py and the transformers fixture.

Gates
  fp32   rel-L2 <= 1e-4 (the project's forward gate).
  bf16, one kernel   the kernels compute in fp32 from the bf16 inputs and round once on the way out, so against an fp64
         result formed from the SAME bf16 inputs every element is within half a bf16 ulp, 2^-9 relative: rel-L2 <= 2^-9
         (+ the fp32 gate for the arithmetic before the rounding).  The attention also rounds the probabilities to bf16
         ahead of the PV product: to first order that adds at most 2^-9 sum_k p_k |v_k| per output element, which the test
         evaluates on the reference itself.
  bf16, model   rel-L2 over ALL valid tokens of the concatenated input draws against the fp64 oracle <= the error of
         transformers under bf16 autocast on the same case, as stored in the fixture -- no margin (the rule of
         test_model_gpu.py): the kernels keep the residual stream, the norm statistics and the softmax in fp32, autocast
         rounds scores and probabilities to bf16.
Padded positions must be exactly 0.0.  Run with -s to see the measured values.

The 24-layer cases (t5_cases.CASES, with the reference-only measurements behind them): deep24_t5init, caption-length
rows and T5's own query scale, is gated in both modes; deep24, un-scaled queries and rows of 3 tokens, in fp32 only.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import t5_cases as TC
from mdm_hip import _lib, ops, text_encoder as TE

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF16_HALF_ULP = 2.0 ** -9
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


def _dt(dtype):
    return ops.F32 if dtype == torch.float32 else ops.BF16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gate(dtype, extra=0.0):
    return TOL if dtype == torch.float32 else TOL + BF16_HALF_ULP * (1.0 + extra)


def _rms_ref(x, w, eps):
    x = x.double()
    return w.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [2048, 200, 72, 8])
@pytest.mark.parametrize("with_delta", [True, False])
def test_add_rms(dtype, D, with_delta):
    T, eps = 37, 1e-6
    g = _gen(D)
    x = torch.randn(T, D, generator=g) * 30.0
    delta = torch.randn(T, D, generator=g).to(dtype) if with_delta else None
    w = torch.rand(D, generator=g) + 0.5
    xs = x + delta.float() if with_delta else x
    xg, dg, wg = x.to(DEV), None if delta is None else delta.to(DEV), w.to(DEV)
    h = torch.empty(T, D, dtype=dtype, device=DEV)
    _lib.check(_lib.lib().mdm_t5_add_rms(_p(xg), _p(dg), _p(wg), _p(h), T, D, eps, _dt(dtype), ops._stream()), "mdm_t5_add_rms")
    assert torch.equal(xg.cpu(), xs)                           # the fp32 stream: one fp32 add, bit for bit
    err = TC.rel_l2(h.float(), _rms_ref(xs, w, eps))
    print("add_rms %s D=%d delta=%s: %.3e" % (dtype, D, with_delta, err))
    assert err <= _gate(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [2048, 200])
def test_embed_rms(dtype, D):
    T, V, eps = 53, 97, 1e-6
    g = _gen(7 + D)
    table = torch.randn(V, D, generator=g)
    ids = torch.randint(0, V, (T,), generator=g)
    w = torch.rand(D, generator=g) + 0.5
    x = torch.full((T, D), float("nan"), device=DEV)
    h = torch.empty(T, D, dtype=dtype, device=DEV)
    ig, tg, wg = ids.to(DEV, torch.int32), table.to(DEV), w.to(DEV)     # (named: a temporary's memory is reused at once)
    _lib.check(_lib.lib().mdm_t5_embed_rms(_p(ig), _p(tg), _p(wg), _p(x), _p(h), T, D, V, eps, _dt(dtype), ops._stream()),
               "mdm_t5_embed_rms")
    assert torch.equal(x.cpu(), table[ids])
    err = TC.rel_l2(h.float(), _rms_ref(table[ids], w, eps))
    print("embed_rms %s D=%d: %.3e" % (dtype, D, err))
    assert err <= _gate(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [2048, 200])
def test_final_rms_scatters_and_zeroes(dtype, D):
    eps = 1e-6
    m = np.array([[1, 1, 1, 0, 0, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1]])
    pk = TE.pack_index(m)
    T, R = pk["T"], m.size
    g = _gen(11 + D)
    x = torch.randn(T, D, generator=g) * 10.0
    delta = torch.randn(T, D, generator=g).to(dtype)
    w = torch.rand(D, generator=g) + 0.5
    out = torch.full((R, D), float("nan"), device=DEV)
    xg, dg, wg, sg = x.to(DEV), delta.to(DEV), w.to(DEV), torch.from_numpy(pk["src"]).to(DEV)
    _lib.check(_lib.lib().mdm_t5_final_rms(_p(xg), _p(dg), _p(wg), _p(sg), _p(out), R, D, eps, _dt(dtype), ops._stream()),
               "mdm_t5_final_rms")
    out = out.cpu()
    assert torch.equal(xg.cpu(), x)                           # the stream is not modified
    pad = torch.from_numpy(m.reshape(-1) == 0)
    assert bool((out[pad] == 0).all()) and not bool(torch.signbit(out[pad]).any())
    err = TC.rel_l2(out[~pad], _rms_ref(x + delta.float(), w, eps))
    print("final_rms %s D=%d: %.3e" % (dtype, D, err))
    assert err <= TOL                                          # the output is fp32 in both modes


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [5120, 640, 24])
def test_gated_gelu(dtype, F):
    T = 41
    u = (torch.randn(T, 2 * F, generator=_gen(F)) * 2.0).to(dtype)
    y = torch.empty(T, F, dtype=dtype, device=DEV)
    ug = u.to(DEV)
    _lib.check(_lib.lib().mdm_t5_gated_gelu(_p(ug), _p(y), T, F, _dt(dtype), ops._stream()), "mdm_t5_gated_gelu")
    ud = u.double()
    ref = TC.gelu_new(ud[:, :F]) * ud[:, F:]
    assert torch.equal(TC.gelu_new(torch.tensor([1.0], dtype=torch.float64)), 0.5 * (1 + torch.tanh(torch.tensor(
        [0.7978845608028654 * 1.044715], dtype=torch.float64))))
    err = TC.rel_l2(y.float(), ref)
    print("gated_gelu %s F=%d: %.3e" % (dtype, F, err))
    assert err <= _gate(dtype)


ATTN_LENGTHS = [1, 5, 16, 17, 33, 77, 128, 129, 300, 512]


def _attn_case(H, holes, seed):
    """mask [B, S]: the named lengths mixed in one batch; with ``holes`` the same COUNTS spread over the row"""
    S = 512
    g = _gen(seed)
    m = np.zeros((len(ATTN_LENGTHS), S), dtype=np.int64)
    for b, n in enumerate(ATTN_LENGTHS):
        if holes and n < S:
            m[b, np.sort(torch.randperm(S, generator=g)[:n].numpy())] = 1
        else:
            m[b, :n] = 1
    return m, S


def _attn_ref(qkv, pk, table, H, S):
    """fp64, per row and head; also sum_k p_k |v_k| for the bound on the rounding of P"""
    d = 64
    qkv = qkv.double()
    out, absout = torch.zeros(pk["T"], H * d, dtype=torch.float64), torch.zeros(pk["T"], H * d, dtype=torch.float64)
    pos = torch.from_numpy(pk["pos"]).long()
    for b in range(pk["B"]):
        t0, t1 = int(pk["seq_start"][b]), int(pk["seq_start"][b + 1])
        if t1 == t0:
            continue
        rel = pos[t0:t1][None, :] - pos[t0:t1][:, None] + (S - 1)            # [q, k]
        for h in range(H):
            q, k, v = (qkv[t0:t1, i * H * d + h * d:i * H * d + (h + 1) * d] for i in range(3))
            p = torch.softmax(q @ k.t() + table[h].double()[rel], dim=-1)
            out[t0:t1, h * d:(h + 1) * d] = p @ v
            absout[t0:t1, h * d:(h + 1) * d] = p @ v.abs()
    return out, absout


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,q_scale", [(2, 1.0), (2, 0.125), (32, 1.0)])
@pytest.mark.parametrize("holes", [False, True], ids=["suffix", "holes"])
def test_attention(dtype, H, q_scale, holes):
    d = 64
    m, S = _attn_case(H, holes, 100 + H)
    pk = TE.pack_index(m)
    T, B = pk["T"], pk["B"]
    g = _gen(1000 + H + int(holes))
    qkv = torch.randn(T, 3 * H * d, generator=g)
    qkv[:, :H * d] *= q_scale                  # 1: scores of std ~8, near arg-max rows; 1/8: O(1) scores, broad rows
    qkv = qkv.to(dtype)
    table = torch.randn(H, 2 * S - 1, generator=g)
    out = torch.full((T, H * d), float("nan"), dtype=dtype, device=DEV)
    qg, sg, pg, tg = qkv.to(DEV), torch.from_numpy(pk["seq_start"]).to(DEV), torch.from_numpy(pk["pos"]).to(DEV), table.to(DEV)
    _lib.check(_lib.lib().mdm_t5_attn_fwd(_p(qg), _p(sg), _p(pg), _p(tg), _p(out), B, T, S, pk["max_len"], H, d, _dt(dtype),
                                          ops._stream()), "mdm_t5_attn_fwd")
    ref, absref = _attn_ref(qkv, pk, table, H, S)
    out = out.float().cpu()
    assert bool(torch.isfinite(out).all())
    err = TC.rel_l2(out, ref)
    extra = float(absref.norm() / ref.norm())
    print("attention %s H=%d q_scale=%g holes=%s: %.3e (gate %.3e)" % (dtype, H, q_scale, holes, err, _gate(dtype, extra)))
    assert err <= _gate(dtype, extra)
    for b in range(B):                         # and per row, so that a short row cannot hide behind the long ones
        t0, t1 = int(pk["seq_start"][b]), int(pk["seq_start"][b + 1])
        e = TC.rel_l2(out[t0:t1], ref[t0:t1])
        ex = float(absref[t0:t1].norm() / ref[t0:t1].norm())
        assert e <= _gate(dtype, ex), (b, t1 - t0, e)


def test_attention_short_grid():
    """max_len below S: the grid is sized by the longest row, results unchanged"""
    H, d, S = 2, 64, 128
    m = np.zeros((5, S), dtype=np.int64)
    for b, n in enumerate([7, 40, 1, 0, 23]):
        m[b, :n] = 1
    pk = TE.pack_index(m)
    T = pk["T"]
    g = _gen(5)
    qkv, table = torch.randn(T, 3 * H * d, generator=g), torch.randn(H, 2 * S - 1, generator=g)
    qg, sg, pg, tg = qkv.to(DEV), torch.from_numpy(pk["seq_start"]).to(DEV), torch.from_numpy(pk["pos"]).to(DEV), table.to(DEV)
    outs = []
    for ml in (pk["max_len"], S):
        out = torch.full((T, H * d), float("nan"), device=DEV)
        _lib.check(_lib.lib().mdm_t5_attn_fwd(_p(qg), _p(sg), _p(pg), _p(tg), _p(out), 5, T, S, ml, H, d, ops.F32, ops._stream()),
                   "mdm_t5_attn_fwd")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    assert TC.rel_l2(outs[0], _attn_ref(qkv, pk, table, H, S)[0]) <= TOL


def test_invalid_arguments_are_errors():
    L = _lib.lib()
    t = torch.zeros(64, 3 * 64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.MdmHipError):       # head dim 32: no kernel, said loudly
        _lib.check(L.mdm_t5_attn_fwd(_p(t), _p(i), _p(i), _p(t), _p(t), 1, 4, 8, 8, 2, 32, ops.F32, ops._stream()), "attn d=32")
    assert b"d == 64" in L.mdm_last_error()
    with pytest.raises(_lib.MdmHipError):       # S beyond the LDS table
        _lib.check(L.mdm_t5_attn_fwd(_p(t), _p(i), _p(i), _p(t), _p(t), 1, 4, 513, 8, 1, 64, ops.F32, ops._stream()), "attn S")
    with pytest.raises(_lib.MdmHipError):
        _lib.check(L.mdm_t5_add_rms(_p(t), None, _p(t), _p(t), 4, 12, 1e-6, ops.F32, ops._stream()), "rms D % 8")
    with pytest.raises(_lib.MdmHipError):
        _lib.check(L.mdm_t5_gated_gelu(_p(t), _p(t), 4, 16, 7, ops._stream()), "gelu dtype")
    with pytest.raises(_lib.MdmHipError):
        _lib.check(L.mdm_t5_embed_rms(None, _p(t), _p(t), _p(t), _p(t), 4, 16, 8, 1e-6, ops.F32, ops._stream()), "null ids")


# ---------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(name):
    if name not in _models:
        _models.clear()                          # one case's weights on the card at a time
        _models[name] = TC.build_module(name, DEV)
    return _models[name]


def _run(name, dtype):
    m = _model(name)
    ids, mask = TC.inputs(name)
    outs = []
    for i in range(TC.DRAWS):
        if dtype == torch.bfloat16:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                outs.append(m(ids[i].to(DEV), mask.to(DEV)))
        else:
            outs.append(m(ids[i].to(DEV), mask.to(DEV)))
        assert outs[-1].dtype == torch.float32 and outs[-1].shape == ids[i].shape + (m.config.d_model,)
    return torch.stack(outs).cpu(), mask


@pytest.fixture(scope="module")
def gold():
    return torch.load(TC.GOLDEN, weights_only=False)


@pytest.mark.parametrize("name", TC.MODEL_CASES + TC.FP32_ONLY_CASES + ["mini_holes"])
def test_model_fp32(name, gold):
    """fp32 mode against the fixture (transformers fp32, channel subsample) and, on the full tensors, against the fp64
    oracle the CPU tests pin to transformers; both <= 1e-4."""
    out, mask = _run(name, torch.float32)
    g = gold["cases"][name]
    assert bool((out[:, mask == 0] == 0).all())
    e_fix = TC.rel_l2(TC.subsample(out, name), g["out_sub"])
    e_orc = TC.rel_l2(TC.valid_rows(out, mask), TC.valid_rows(TC.oracle_outputs(name), mask))
    print("model fp32 %s: vs fixture %.3e, vs fp64 oracle %.3e (transformers fp32 vs fp64 oracle %.3e)"
          % (name, e_fix, e_orc, g["ref_fp32_error"]))
    assert e_fix <= TOL and e_orc <= TOL


@pytest.mark.parametrize("name", TC.MODEL_CASES + ["mini_holes"])
def test_model_bf16(name, gold):
    out, mask = _run(name, torch.bfloat16)
    g = gold["cases"][name]
    assert bool((out[:, mask == 0] == 0).all())
    err = TC.rel_l2(TC.valid_rows(out, mask), TC.valid_rows(TC.oracle_outputs(name), mask))
    print("model bf16 %s: %.3e vs fp64 oracle; transformers under bf16 autocast %.3e" % (name, err, g["ref_bf16_error"]))
    assert err <= g["ref_bf16_error"]


def test_model_cases_are_as_required():
    for name in TC.MODEL_CASES + TC.FP32_ONLY_CASES:
        mask = TC.mask_of(name)
        assert float(mask.sum(1).max()) == mask.shape[1] and float(mask.mean()) >= 0.25
        assert TC.DRAWS >= 4


def _captions(S):
    """the same captions (ids + lengths, one with a hole) padded to S"""
    g = _gen(3)
    ids = torch.zeros(3, S, dtype=torch.long)
    mask = torch.zeros(3, S)
    for b, n in enumerate([32, 9, 21]):
        ids[b, :n] = torch.randint(1, 512, (n,), generator=g)
        mask[b, :n] = 1
    mask[2, 4] = 0
    return ids, mask


def test_padding_invariance_and_determinism():
    m = _model("mini")
    (i32, m32), (i128, m128) = _captions(32), _captions(128)
    a = m(i32.to(DEV), m32.to(DEV)).cpu()
    b = m(i128.to(DEV), m128.to(DEV)).cpu()
    assert torch.equal(a[m32.bool()], b[m128.bool()])          # valid rows: bit-identical whatever the padding
    assert bool((b[m128 == 0] == 0).all())
    assert torch.equal(m(i128.to(DEV), m128.to(DEV)).cpu(), b)    # two calls
    with torch.autocast("cuda", dtype=torch.bfloat16):
        c, d = m(i128.to(DEV), m128.to(DEV)).cpu(), m(i128.to(DEV), m128.to(DEV)).cpu()
    assert torch.equal(c, d) and not torch.equal(c, b)


def test_host_and_gpu_inputs_agree():
    m = _model("mini")
    ids, mask = TC.inputs("mini_holes")           # a hole mask and an all-pad row; same vocabulary as mini
    ref = m(ids[0].to(DEV), mask.to(DEV)).cpu()
    assert torch.equal(m(ids[0].numpy(), mask.numpy()).cpu(), ref)                 # host arrays (the reader's)
    assert torch.equal(m(ids[0], mask).cpu(), ref)                                 # CPU tensors
    assert torch.equal(m(ids[0].to(DEV), mask.numpy() != 0).cpu(), ref)            # GPU ids, host mask
    assert bool((ref[2] == 0).all())                                               # the row with no valid token
    full = m(ids[0].to(DEV)).cpu()                                                 # no mask = every token valid
    assert torch.equal(full, m(ids[0].to(DEV), torch.ones_like(mask)).cpu())
    assert bool((m(ids[0], torch.zeros_like(mask)) == 0).all())                    # nothing valid at all


def test_release_masters():
    m = TC.build_module("mini", DEV)
    ids, mask = TC.inputs("mini")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        before = m(ids[0].to(DEV), mask.to(DEV)).cpu()
        m.release_masters()
        after = m(ids[0].to(DEV), mask.to(DEV)).cpu()
    assert torch.equal(before, after)
    assert m.encoder.block[0].layer[0].SelfAttention.q.weight.numel() == 0
    with pytest.raises(_lib.MdmHipError, match="release_masters"):
        m.state_dict()
    with pytest.raises(_lib.MdmHipError):
        m(ids[0].to(DEV), mask.to(DEV))          # fp32 mode: its weights were never packed


def test_forward_only_pack_has_no_dgrad_copy():
    w = torch.randn(128, 64, device=DEV)
    wf, wd = ops.packed_weight(w, None, torch.bfloat16, forward_only=True)[:2]
    assert wd is None and wf.numel() == 128 * 64
    wf2, wd2 = ops.packed_weight(w, None, torch.bfloat16)[:2]
    assert wd2 is not None and torch.equal(wf, wf2)


def test_language_model_forward():
    args = NS(use_precomputed_text_embeddings=False, categorical_conditioning=False, fp16=False,
              reader_config=NS(padding_token="<pad>"))
    tok = NS(token_id=lambda t: 0)
    name = "mini"
    cfg, sd = TC.config(name), TC.weights(name)
    lm = TE.LanguageModel(args, TC.build_module(name)).to(DEV)
    ids, _ = _captions(48)
    tokens = ids.numpy()                                    # the reader hands over a host array
    mask = (ids != 0).float()
    ref = TC.oracle_forward(sd, cfg, ids, mask, torch.float64)
    out, lm_mask = lm({"tokens": tokens}, tok)
    assert torch.equal(lm_mask.cpu(), mask) and out.dtype == torch.float32
    assert TC.rel_l2(out[mask.bool()], ref[mask.bool()]) <= TOL and bool((out.cpu()[mask == 0] == 0).all())
    out_t, _ = lm({"tokens": ids.to(DEV)}, tok)           # tokens already on the device
    assert torch.equal(out_t, out)
    args.fp16 = True
    out_b, _ = lm({"tokens": tokens}, tok)
    e = TC.rel_l2(out_b[mask.bool()], ref[mask.bool()])
    assert TOL < e < 0.2, e                                # bf16 path taken under args.fp16
    # pre-computed embeddings: no model at all
    args.use_precomputed_text_embeddings = True
    lm2 = TE.LanguageModel(args, TC.build_module(name)).to(DEV)
    emb = torch.randn(3, 48, 256, generator=_gen(0)).to(DEV)
    out2, mask2 = lm2({"tokens": tokens, "text_embedding": emb}, tok)
    assert lm2.model is None and torch.equal(out2.cpu(), emb.cpu() * mask.unsqueeze(-1)) and torch.equal(mask2.cpu(), mask)


def test_encoder_output_drives_the_unet():
    """a T5 of d_model 64 (2 heads x 64) feeding mini_unet, whose conditioning width is 64: finite loss, finite grads"""
    import parity_cases as PC

    cfg = TE.T5EncoderConfig(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_layers=2, num_heads=2)
    torch.manual_seed(0)
    enc = TE.T5Encoder(cfg).to(DEV)
    unet, _, _ = PC.build_module("mini_unet")
    unet = unet.to(DEV)
    inp = PC.inputs("mini_unet")
    mask = inp["mask"]
    ids = torch.randint(1, 128, mask.shape, generator=_gen(9))
    cond = enc(ids.numpy(), mask.numpy())
    assert cond.shape == inp["cond"].shape and bool((cond.cpu()[mask == 0] == 0).all()) and not cond.requires_grad
    out = unet(inp["x"].to(DEV), inp["times"].to(DEV), cond, mask.to(DEV))
    loss = PC.loss_of(out, inp["gys"])
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) != 0.0
    assert all(bool(torch.isfinite(p.grad).all()) for p in unet.parameters() if p.grad is not None)
