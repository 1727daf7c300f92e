"""GPU: the input-gradient kernels of the frozen T5 encoder (csrc/text_encoder_bwd.hip) against the fp64 restatements of
ti_cases.py, and mdm_hip.textual_inversion end to end against torch autograd through the fp64 oracle of t5_cases.py.

Gates
  kernels   rel-L2 per output tensor against the fp64 restatement formed from the SAME storage-rounded inputs: 2e-5 in
            fp32, 3e-2 in bf16 (the project's kernel gates).  lse of the forward: absolute 1e-6 from fp64, in fp32.
  encoder   fp32: rel-L2 of the embedding gradient over the four input draws pooled <= 1e-3 (the project's gradient gate).
            bf16: <= the error of transformers under bf16 autocast on the same case times the largest per-draw / pooled
            ratio of that error, both as stored in tests/golden/t5_grad.pt -- the spread the reference shows against
            itself, and nothing more.
Run with -s to see the measured values.
"""
import numpy as np
import pytest
import torch

import t5_cases as TC
import ti_cases as TI
from mdm_hip import _lib, ops, text_encoder as TE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
KGATE = {torch.float32: 2e-5, torch.bfloat16: 3e-2}
HOLES = [1, 1, 0, 1, 0, 0, 1, 1, 1, 0]            # the mini_holes pattern


def _dt(dtype):
    return ops.F32 if dtype == torch.float32 else ops.BF16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return ops._stream()


def _L():
    return _lib.lib()


def _mask(rows, S):
    m = np.zeros((len(rows), S), dtype=np.int64)
    for b, r in enumerate(rows):
        if isinstance(r, int):
            m[b, :r] = 1
        else:
            m[b, :len(r)] = r
    return m


def _dev_plan(pk):
    return torch.from_numpy(pk["seq_start"]).to(DEV), torch.from_numpy(pk["pos"]).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# attention: forward with log-sum-exp, backward
# ---------------------------------------------------------------------------------------------------------------------
MIXED = ([1, 15, 16, 17, 31, 32, 33, 64, 77, 0, HOLES * 8], 80, 2)      # rows, S, H
LONG = ([512], 512, 1)


def _attn_inputs(case, dtype, q_scale, seed, integer=False):
    rows, S, H = case
    pk = TE.pack_index(_mask(rows, S))
    T, d = pk["T"], 64
    g = _gen(seed)
    if integer:
        qkv = torch.randint(-3, 4, (T, 3 * H * d), generator=g).float()
        dout = torch.randint(-3, 4, (T, H * d), generator=g).float()
        table = torch.zeros(H, 2 * S - 1)
    else:
        qkv = torch.randn(T, 3 * H * d, generator=g)
        qkv[:, :H * d] *= q_scale
        dout = torch.randn(T, H * d, generator=g)
        table = torch.randn(H, 2 * S - 1, generator=g)
    return pk, qkv.to(dtype), dout.to(dtype), table, S, H


def _fwd_lse(qkv, pk, table, S, H, dtype, lse=True):
    T = pk["T"]
    sg, pg = _dev_plan(pk)
    qg, tg = qkv.to(DEV), table.to(DEV)
    out = torch.full((T, H * 64), float("nan"), dtype=dtype, device=DEV)
    if lse:
        ls = torch.full((H, T), float("nan"), device=DEV)
        _lib.check(_L().mdm_t5_attn_fwd_lse(_p(qg), _p(sg), _p(pg), _p(tg), _p(out), _p(ls), pk["B"], T, S, pk["max_len"], H,
                                            64, _dt(dtype), _st()), "mdm_t5_attn_fwd_lse")
        return out.cpu(), ls.cpu()
    _lib.check(_L().mdm_t5_attn_fwd(_p(qg), _p(sg), _p(pg), _p(tg), _p(out), pk["B"], T, S, pk["max_len"], H, 64, _dt(dtype),
                                    _st()), "mdm_t5_attn_fwd")
    return out.cpu(), None


def _bwd(qkv, out, lse, dout, pk, table, S, H, dtype):
    T = pk["T"]
    sg, pg = _dev_plan(pk)
    qg, og, lg, dg, tg = qkv.to(DEV), out.to(DEV), lse.to(DEV), dout.to(DEV), table.to(DEV)
    dqkv = torch.full((T, 3 * H * 64), float("nan"), dtype=dtype, device=DEV)
    _lib.check(_L().mdm_t5_attn_bwd(_p(qg), _p(og), _p(lg), _p(dg), _p(sg), _p(pg), _p(tg), _p(dqkv), pk["B"], T, S,
                                    pk["max_len"], H, 64, _dt(dtype), _st()), "mdm_t5_attn_bwd")
    return dqkv.cpu()


def _saved(qkv, pk, table, H, S, dtype):
    """out and lse as a forward would have saved them: the fp64 values rounded to the storage types"""
    out, lse = TI.attn_forward(qkv, pk, table, H, S)
    return out.to(dtype), lse.float()


def _check_dqkv(tag, got, ref, H, gate):
    assert bool(torch.isfinite(got.float()).all()), "%s: non-finite (or unwritten) elements" % tag
    n = H * 64
    for i, name in enumerate(("dq", "dk", "dv")):
        err = TC.rel_l2(got[:, i * n:(i + 1) * n].float(), ref[:, i * n:(i + 1) * n])
        print("%s %s: %.3e (gate %.1e)" % (tag, name, err, gate))
        assert err <= gate, (tag, name, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [MIXED, LONG], ids=["mixed", "long512"])
def test_attn_fwd_lse(dtype, case):
    pk, qkv, _, table, S, H = _attn_inputs(case, dtype, 64 ** -0.5, 11)
    out0, _ = _fwd_lse(qkv, pk, table, S, H, dtype, lse=False)
    out1, lse = _fwd_lse(qkv, pk, table, S, H, dtype)
    assert torch.equal(out0, out1)
    assert bool(torch.isfinite(lse).all())
    _, ref = TI.attn_forward(qkv, pk, table, H, S)
    err = float((lse.double() - ref).abs().max())          # absolute: lse is near 5 (S = 80) and 7 (S = 512) here
    print("lse %s: max absolute error %.3e, rel-L2 %.3e" % (dtype, err, TC.rel_l2(lse, ref)))
    if dtype == torch.float32:
        assert err <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [MIXED, LONG], ids=["mixed", "long512"])
def test_attn_bwd(dtype, case):
    pk, qkv, dout, table, S, H = _attn_inputs(case, dtype, 64 ** -0.5, 21)
    out, lse = _saved(qkv, pk, table, H, S, dtype)
    got = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    ref = TI.attn_backward(qkv, out, lse, dout, pk, table, H, S)
    _check_dqkv("attn_bwd %s S=%d" % (dtype, S), got, ref, H, KGATE[dtype])
    # per row, so that a short row cannot hide behind the long ones
    for b in range(pk["B"]):
        t0, t1 = int(pk["seq_start"][b]), int(pk["seq_start"][b + 1])
        if t1 > t0:
            assert TC.rel_l2(got[t0:t1].float(), ref[t0:t1]) <= KGATE[dtype], "row %d (%d tokens)" % (b, t1 - t0)


def test_attn_bwd_unscaled_queries_fp32():
    """scores of std ~8: every softmax is near an arg-max"""
    dtype = torch.float32
    pk, qkv, dout, table, S, H = _attn_inputs(MIXED, dtype, 1.0, 31)
    out, lse = _saved(qkv, pk, table, H, S, dtype)
    got = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    _check_dqkv("attn_bwd unscaled", got, TI.attn_backward(qkv, out, lse, dout, pk, table, H, S), H, KGATE[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_bwd_single_key_exact(dtype):
    """integer data, zero bias, one key per row: P = 1, so dv == dout and dq == dk == 0 exactly"""
    case = ([1] * 9 + [0, 1], 80, 2)
    pk, qkv, dout, table, S, H = _attn_inputs(case, dtype, 1.0, 41, integer=True)
    out, lse = _fwd_lse(qkv, pk, table, S, H, dtype)
    n = H * 64
    assert torch.equal(out, qkv[:, 2 * n:])
    got = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    assert torch.equal(got[:, 2 * n:], dout)
    assert bool((got[:, :2 * n] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_bwd_dq_dk_not_swapped(dtype):
    """asymmetric data: q and k of different scale and sign pattern, so dq and dk differ by far more than the gate"""
    pk, qkv, dout, table, S, H = _attn_inputs(([33, 17], 40, 2), dtype, 1.0, 51)
    n = H * 64
    qkv = qkv.float()
    qkv[:, :n] = qkv[:, :n].abs() * 0.05
    qkv[:, n:2 * n] = qkv[:, n:2 * n] * 1.5 + 0.5
    qkv = qkv.to(dtype)
    out, lse = _saved(qkv, pk, table, H, S, dtype)
    got = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    ref = TI.attn_backward(qkv, out, lse, dout, pk, table, H, S)
    _check_dqkv("attn_bwd asymmetric %s" % dtype, got, ref, H, KGATE[dtype])
    assert TC.rel_l2(got[:, :n].float(), ref[:, n:2 * n]) > 0.5 and TC.rel_l2(got[:, n:2 * n].float(), ref[:, :n]) > 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_bwd_deterministic_and_independent(dtype):
    rows, S, H = MIXED
    pk, qkv, dout, table, S, H = _attn_inputs(MIXED, dtype, 64 ** -0.5, 61)
    out, lse = _saved(qkv, pk, table, H, S, dtype)
    a = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    b = _bwd(qkv, out, lse, dout, pk, table, S, H, dtype)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for r in (1, 8, 10):                                   # 15 tokens, 77 tokens, the row with holes
        t0, t1 = int(pk["seq_start"][r]), int(pk["seq_start"][r + 1])
        pk1 = TE.pack_index(_mask([rows[r]], S))
        alone = _bwd(qkv[t0:t1], out[t0:t1], lse[:, t0:t1].contiguous(), dout[t0:t1], pk1, table, S, H, dtype)
        assert torch.equal(alone.view(torch.uint8), a[t0:t1].view(torch.uint8)), "row %d depends on the batch" % r


def test_attn_bwd_argument_checks():
    dtype = torch.float32
    pk, qkv, dout, table, S, H = _attn_inputs(([5, 3], 8, 1), dtype, 1.0, 71)
    out, lse = _saved(qkv, pk, table, H, S, dtype)
    T = pk["T"]
    sg, pg = _dev_plan(pk)
    qg, og, lg, dg, tg = qkv.to(DEV), out.to(DEV), lse.to(DEV), dout.to(DEV), table.to(DEV)
    dqkv = torch.full((T, 3 * H * 64), 7.0, device=DEV)
    L = _L()

    def call(qp=None, S_=S, d=64, dt=ops.F32):
        return L.mdm_t5_attn_bwd(_p(qg) if qp is None else qp[0], _p(og), _p(lg), _p(dg), _p(sg), _p(pg), _p(tg), _p(dqkv),
                                 pk["B"], T, S_, min(pk["max_len"], S_), H, d, dt, _st())

    assert call(d=32) != 0
    assert call(S_=513) != 0
    assert call(qp=(None,)) != 0
    assert call(dt=99) != 0
    ls2 = torch.full((H, T), 7.0, device=DEV)
    assert L.mdm_t5_attn_fwd_lse(_p(qg), _p(sg), _p(pg), _p(tg), _p(og), _p(ls2), pk["B"], T, 513, pk["max_len"], H, 64, ops.F32,
                                 _st()) != 0
    assert L.mdm_t5_attn_fwd_lse(_p(qg), _p(sg), _p(pg), _p(tg), _p(og), None, pk["B"], T, S, pk["max_len"], H, 64, ops.F32,
                                 _st()) != 0
    assert L.mdm_t5_gated_gelu_bwd(_p(qg), _p(dg), None, T, 64, ops.F32, _st()) != 0
    assert L.mdm_t5_rms_bwd(_p(qg), _p(tg), _p(dg), None, None, T, 64, 1e-6, ops.F32, _st()) != 0
    assert L.mdm_t5_rms_bwd(_p(qg), _p(tg), _p(dg), _p(dqkv), None, T, 64, 1e-6, 99, _st()) != 0
    torch.cuda.synchronize()
    assert bool((dqkv == 7.0).all()) and bool((ls2 == 7.0).all())          # nothing was launched
    assert call() == 0                                                     # and the valid call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv).all()) and not bool((dqkv == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# RMS norm, gated GELU, embedding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,D", [(5, 8), (7, 264), (4, 2048)])
def test_rms_bwd(dtype, T, D):
    eps = 1e-6
    g = _gen(D)
    x = torch.randn(T, D, generator=g) * 3.0
    w = torch.rand(D, generator=g) + 0.5
    dh = torch.randn(T, D, generator=g).to(dtype)
    dx0 = torch.randn(T, D, generator=g)
    xg, wg, dg, dx = x.to(DEV), w.to(DEV), dh.to(DEV), dx0.to(DEV)
    lo = torch.full((T, D), float("nan"), dtype=dtype, device=DEV)
    _lib.check(_L().mdm_t5_rms_bwd(_p(xg), _p(wg), _p(dg), _p(dx), _p(lo), T, D, eps, _dt(dtype), _st()), "mdm_t5_rms_bwd")
    ref = TI.rms_backward(x, w, dh, eps)
    err = TC.rel_l2(dx.cpu() - dx0, ref)                   # the ADDED part: an overwrite would leave -dx0 in it
    print("rms_bwd %s T=%d D=%d: %.3e" % (dtype, T, D, err))
    # fp32 either way: dx is the fp32 stream gradient (the subtraction of dx0 costs 1 ulp of |dx0 + ref|)
    assert err <= KGATE[torch.float32]
    assert TC.rel_l2(lo.float(), dx0.double() + ref) <= KGATE[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [8, 264, 2048])
def test_final_rms_bwd(dtype, D):
    eps = 1e-6
    m = np.array([[1, 1, 1, 0, 0, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1]])
    pk = TE.pack_index(m)
    T, R = pk["T"], m.size
    g = _gen(100 + D)
    x = torch.randn(T, D, generator=g) * 3.0
    delta = torch.randn(T, D, generator=g).to(dtype)
    w = torch.rand(D, generator=g) + 0.5
    dout = torch.randn(R, D, generator=g)
    xg, eg, wg, og = x.to(DEV), delta.to(DEV), w.to(DEV), dout.to(DEV)
    flat = torch.from_numpy(pk["idx"].astype(np.int32)).to(DEV)
    dx = torch.full((T, D), float("nan"), device=DEV)
    _lib.check(_L().mdm_t5_final_rms_bwd(_p(xg), _p(eg), _p(wg), _p(og), _p(flat), _p(dx), None, T, D, eps, _dt(dtype), _st()),
               "mdm_t5_final_rms_bwd")
    ref = TI.rms_backward(x + delta.float(), w, dout[torch.from_numpy(pk["idx"])], eps)
    err = TC.rel_l2(dx.cpu(), ref)
    print("final_rms_bwd %s D=%d: %.3e" % (dtype, D, err))
    assert err <= KGATE[torch.float32]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("F", [8, 640])
def test_gated_gelu_bwd(dtype, F):
    T = 41
    g = _gen(F)
    u = (torch.randn(T, 2 * F, generator=g) * 3.0).clamp(-9.0, 9.0)
    u[0, :4] = torch.tensor([9.0, -9.0, 0.0, -0.75])
    u[1, F:F + 2] = torch.tensor([9.0, -9.0])
    u = u.to(dtype)
    dy = torch.randn(T, F, generator=g).to(dtype)
    ug, dg = u.to(DEV), dy.to(DEV)
    du = torch.full((T, 2 * F), float("nan"), dtype=dtype, device=DEV)
    _lib.check(_L().mdm_t5_gated_gelu_bwd(_p(ug), _p(dg), _p(du), T, F, _dt(dtype), _st()), "mdm_t5_gated_gelu_bwd")
    ref = TI.gated_gelu_backward(u, dy)
    du = du.float().cpu()
    assert bool(torch.isfinite(du).all())
    for name, sl in (("da", slice(0, F)), ("db", slice(F, 2 * F))):
        err = TC.rel_l2(du[:, sl], ref[:, sl])
        print("gated_gelu_bwd %s F=%d %s: %.3e" % (dtype, F, name, err))
        assert err <= KGATE[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_embed_rms_slots(dtype):
    T, V, D, P, eps = 53, 97, 264, 3, 1e-6
    g = _gen(5)
    table = torch.randn(V, D, generator=g)
    learned = torch.randn(P, D, generator=g)
    w = torch.rand(D, generator=g) + 0.5
    ids = torch.randint(0, V, (T,), generator=g)
    tg, lg, wg = table.to(DEV), learned.to(DEV), w.to(DEV)

    def run(ids, slot_of_id, plain=False):
        ig = ids.to(DEV, torch.int32)
        x = torch.full((T, D), float("nan"), device=DEV)
        h = torch.full((T, D), float("nan"), dtype=dtype, device=DEV)
        if plain:
            _lib.check(_L().mdm_t5_embed_rms(_p(ig), _p(tg), _p(wg), _p(x), _p(h), T, D, V, eps, _dt(dtype), _st()),
                       "mdm_t5_embed_rms")
        else:
            sg = slot_of_id.to(DEV, torch.int32)
            _lib.check(_L().mdm_t5_embed_rms_slots(_p(ig), _p(tg), _p(sg), _p(lg), _p(wg), _p(x), _p(h), T, D, V,
                                                   int(sg.numel()), P, eps, _dt(dtype), _st()), "mdm_t5_embed_rms_slots")
        return x.cpu(), h.cpu()

    x0, h0 = run(ids, None, plain=True)
    x1, h1 = run(ids, torch.full((V,), -1))
    assert torch.equal(x0, x1) and torch.equal(h0.view(torch.uint8), h1.view(torch.uint8))
    # slots: id 3 (inside the vocabulary) -> row 1, ids V and V + 1 (beyond it) -> rows 2 and 0
    slot_of_id = torch.full((V + 2,), -1)
    slot_of_id[3], slot_of_id[V], slot_of_id[V + 1] = 1, 2, 0
    ids2 = ids.clone()
    ids2[::5], ids2[1::7], ids2[2::11] = 3, V, V + 1
    x2, h2 = run(ids2, slot_of_id)
    ext = torch.cat([table, learned[2:3], learned[0:1]])
    ext[3] = learned[1]
    assert int((x2 != ext[ids2]).sum()) == 0
    # the normed rows: the plain kernel run on the extended table must give the same bits
    tg = ext.to(DEV)
    V = V + 2
    x3, h3 = run(ids2, None, plain=True)
    assert torch.equal(h2.view(torch.uint8), h3.view(torch.uint8))


def test_embed_bwd():
    P, D, T = 5, 264, 420
    g = _gen(9)
    dx0 = torch.randn(T, D, generator=g)
    ids = torch.randint(10, 20, (T,), generator=g)
    ids[torch.randperm(T, generator=g)[:300]] = 3                       # slot 1: 300 tokens
    token_ids = [12, 3, 15, 999, 17]                                    # slot 3: no token
    start, tokens = TI.slot_index(ids.numpy(), token_ids)
    assert start[2] - start[1] == 300 and start[4] == start[3]
    out = torch.full((P, D), float("nan"), device=DEV)
    dg, sg, kg = dx0.to(DEV), torch.from_numpy(start).to(DEV), torch.from_numpy(tokens).to(DEV)
    _lib.check(_L().mdm_t5_embed_bwd(_p(dg), _p(sg), _p(kg), _p(out), P, D, int(tokens.size), T, _st()), "mdm_t5_embed_bwd")
    out = out.cpu()
    assert torch.equal(out, TI.embed_backward(dx0, start, tokens, torch.float32))      # sequential fp32 sum, every bit
    assert bool((out[3] == 0).all())
    err = TC.rel_l2(out, TI.embed_backward(dx0, start, tokens))
    print("embed_bwd: %.3e" % err)
    assert err <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------
# the encoder with an attached textual inversion
# ---------------------------------------------------------------------------------------------------------------------
from mdm_hip import textual_inversion as TXI  # noqa: E402

_models = {}


def _model(name):
    if name not in _models:
        _models.clear()                          # one case's weights on the card at a time
        _models[name] = TC.build_module(name, DEV)
    return _models[name]


@pytest.fixture(scope="module")
def gold():
    return torch.load(TI.GOLDEN, weights_only=False)


def _table_grads(name, dtype):
    """[DRAWS, vocab, D]: every id a placeholder, the rows initialised with the table, so that the gradient of the
    embeddings is the table gradient"""
    m = _model(name)
    ids, mask = TC.inputs(name)
    G = TI.cotangents(name)
    ti = TXI.attach(m, range(m.config.vocab_size), init=m.shared.weight.detach())
    try:
        grads = []
        for i in range(TC.DRAWS):
            ti.embeddings.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                out = m(ids[i].numpy() if i % 2 else ids[i].to(DEV), mask.to(DEV))     # host and device ids alternate
            assert out.requires_grad and out.dtype == torch.float32
            (out * G[i].to(DEV)).sum().backward()
            grads.append(ti.embeddings.grad.detach().cpu().clone())
    finally:
        ti.detach()
    return torch.stack(grads)


@pytest.mark.parametrize("name", TI.GRAD_CASES)
def test_encoder_table_gradient_fp32(name, gold):
    got, ref = _table_grads(name, torch.float32), TI.oracle_table_grads(name)
    err = TC.rel_l2(got, ref)
    per = [TC.rel_l2(got[i], ref[i]) for i in range(TC.DRAWS)]
    print("table gradient fp32 %s: %.3e pooled, per draw %s (transformers fp32 vs fp64 oracle %.3e)"
          % (name, err, ["%.2e" % e for e in per], gold["cases"][name]["ref_fp32_error"]))
    assert bool(torch.isfinite(got).all())
    assert err <= TI.GRAD_GATE


@pytest.mark.parametrize("name", TI.BF16_GRAD_CASES)
def test_encoder_table_gradient_bf16(name, gold):
    got, ref = _table_grads(name, torch.bfloat16), TI.oracle_table_grads(name)
    err = TC.rel_l2(got, ref)
    g = gold["cases"][name]
    gate = g["ref_bf16_error"] * g["ref_bf16_spread"]
    print("table gradient bf16 %s: %.3e pooled; gate %.3e = transformers under bf16 autocast %.3e x spread %.3f"
          % (name, err, gate, g["ref_bf16_error"], g["ref_bf16_spread"]))
    assert bool(torch.isfinite(got).all())
    assert err <= gate


def test_attached_encoder_computes_the_same_bits():
    m = TC.build_module("mini", DEV)
    ids, mask = TC.inputs("mini_holes")                      # a hole mask and an all-pad row; same vocabulary as mini
    i0, mk = ids[0].to(DEV), mask.to(DEV)
    ref = m(i0, mk)
    assert ref.grad_fn is None and not ref.requires_grad
    toks = [5, 17, 300]
    ti = TXI.attach(m, toks)                                 # rows default to the table's own
    assert not m._dpacks
    with torch.no_grad():
        assert torch.equal(m(i0, mk), ref)
    assert not m._dpacks                                     # no input-gradient packs for inference
    out = m(i0, mk)
    assert out.grad_fn is not None and torch.equal(out.detach(), ref)      # grad mode: the same bits
    assert torch.float32 in m._dpacks                        # ... and the packs exist now
    assert torch.equal(m(ids[0].numpy(), mask.numpy()).detach(), ref)
    with pytest.raises(_lib.MdmHipError, match="differentiable"):
        m.release_masters()
    ti.embeddings.requires_grad_(False)
    assert m(i0, mk).grad_fn is None
    ti.embeddings.requires_grad_(True)
    ti.detach()
    after = m(i0, mk)
    assert after.grad_fn is None and torch.equal(after, ref)
    # the other way round: released masters refuse a differentiable forward
    m2 = TC.build_module("mini", DEV)
    m2(i0, mk)
    m2.release_masters(torch.float32)
    TXI.attach(m2, toks)
    with torch.no_grad():
        assert torch.equal(m2(i0, mk), ref)
    with pytest.raises(_lib.MdmHipError, match="release_masters"):
        m2(i0, mk)


def test_language_model_keeps_the_graph_and_backward_guards():
    """LanguageModel.forward with an adapter attached returns a tensor with history, in fp32 and under args.fp16, whose
    backward reaches the embeddings and equals the encoder's called directly; a backward that cannot be right -- a second
    one, or one after the adapter's token ids changed -- is refused with a clear error"""
    from types import SimpleNamespace as NS

    args = NS(use_precomputed_text_embeddings=False, categorical_conditioning=False, fp16=False,
              reader_config=NS(padding_token="<pad>"))
    tok = NS(token_id=lambda t: 0)
    m = TC.build_module("mini", DEV)
    lm = TE.LanguageModel(args, m).to(DEV)
    g = _gen(5)
    mask = torch.from_numpy(_mask([12, 5, 0, 9], 12)).bool()
    ids = torch.randint(1, m.config.vocab_size, mask.shape, generator=g) * mask      # pad id 0 where masked
    assert lm({"tokens": ids.numpy()}, tok)[0].grad_fn is None                       # nothing attached: no history
    toks = [7, m.config.vocab_size + 3]
    ids[0, 2], ids[1, 4], ids[3, 0], ids[3, 8] = toks[0], toks[1], toks[1], toks[0]
    G = torch.randn(mask.shape + (m.config.d_model,), generator=g).to(DEV)
    ti = TXI.attach(m, toks, init_ids=[7, 9])
    grads = {}
    for fp16 in (False, True):
        args.fp16 = fp16
        for tokens in (ids.numpy(), ids.to(DEV)):
            ti.embeddings.grad = None
            out, lm_mask = lm({"tokens": tokens}, tok)
            assert out.grad_fn is not None and out.dtype == torch.float32 and torch.equal(lm_mask.cpu().bool(), mask)
            (out * G).sum().backward()
            gr = ti.embeddings.grad
            assert gr is not None and bool(torch.isfinite(gr).all()) and bool((gr.abs().sum(dim=1) > 0).all())
            grads.setdefault(fp16, []).append(ti.embeddings.grad.clone())
        assert torch.equal(grads[fp16][0], grads[fp16][1])                           # host ids and device ids: same bits
    args.fp16 = False
    ti.embeddings.grad = None
    (m(ids.numpy(), mask.numpy()) * G).sum().backward()
    assert torch.equal(ti.embeddings.grad, grads[False][0])                          # the encoder called directly
    assert TC.rel_l2(grads[True][0], grads[False][0]) > 1e-5                         # args.fp16 took the bf16 path

    out = lm({"tokens": ids.numpy()}, tok)[0]
    loss = (out * G).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(_lib.MdmHipError, match="already backpropagated"):
        loss.backward()
    out = lm({"tokens": ids.numpy()}, tok)[0]
    sd = ti.state_dict()
    sd["_extra_state"] = {"token_ids": [toks[1], toks[0]]}
    ti.load_state_dict(sd)
    with pytest.raises(_lib.MdmHipError, match="token_ids"):
        (out * G).sum().backward()
    out = lm({"tokens": ids.numpy()}, tok)[0]
    ti.detach()
    with pytest.raises(_lib.MdmHipError, match="detached"):
        (out * G).sum().backward()


def test_real_placeholders_fp32():
    """two ids beyond the vocabulary and one inside it, several occurrences each across rows of different lengths, against
    the fp64 oracle run on a table extended by those rows"""
    name = "mini"
    m = TC.build_module(name, DEV)
    cfg, sd = TC.config(name), TC.weights(name)
    V, D = cfg.vocab_size, cfg.d_model
    toks = [V + 1, 40, V]
    g = _gen(77)
    rows = torch.randn(3, D, generator=g)
    mask = torch.from_numpy(_mask([48, 19, 7, 0, 30], 48)).float()
    ids = torch.randint(0, V, mask.shape, generator=g)
    for b, where in ((0, [0, 5, 47]), (1, [3, 18]), (2, [6]), (4, [1, 2, 29])):
        for k, s in enumerate(where):
            ids[b, s] = toks[(b + k) % 3]
    ids[2, 0], ids[0, 20] = toks[0], toks[1]
    assert all(int(((ids == t) & mask.bool()).sum()) >= 3 for t in toks)
    G = torch.randn(mask.shape + (D,), generator=g) * mask[..., None]
    ext = torch.cat([sd["shared.weight"], rows[2:3], rows[0:1]])              # rows V and V + 1
    ext[40] = rows[1]
    ref = TI.oracle_table_grad(sd, cfg, ids, mask, G, table=ext)[toks]
    with pytest.raises(ValueError, match="outside"):
        m(ids.numpy(), mask.numpy())                                           # not attached: ids beyond the vocabulary
    ti = TXI.attach(m, toks, init=rows)
    for dev_ids in (False, True):
        ti.embeddings.grad = None
        out = m(ids.to(DEV) if dev_ids else ids.numpy(), mask.numpy())
        fwd = TC.rel_l2(out.detach().cpu()[mask.bool()], TC.oracle_forward({**sd, "shared.weight": ext}, cfg, ids, mask)[mask.bool()])
        (out * G.to(DEV)).sum().backward()
        err = TC.rel_l2(ti.embeddings.grad, ref)
        print("placeholders fp32 (ids on %s): forward %.3e, gradient %.3e" % ("device" if dev_ids else "host", fwd, err))
        assert fwd <= 1e-4 and err <= TI.GRAD_GATE
    bad = ids.clone()
    bad[0, 1] = V + 2
    with pytest.raises(ValueError, match="placeholder"):
        m(bad.numpy(), mask.numpy())
    with pytest.raises(_lib.MdmHipError, match="beyond the vocabulary"):
        ti.merge()


def _chain():
    import parity_cases as PC
    from mdm_hip import diffusion as Df
    from mdm_hip import samplers as Sm

    unet = PC.build_module("mini_unet")[0]
    scfg = Sm.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                            loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=False, rescale_signal=None)
    pipe = Df.Diffusion(unet, Df.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False)).to(torch.device(DEV))
    inp = PC.inputs("mini_unet")
    width = inp["cond"].shape[-1]
    cfg = TE.T5EncoderConfig(vocab_size=128, d_model=width, d_kv=64, d_ff=128, num_layers=3, num_heads=2)
    torch.manual_seed(0)
    enc = TE.T5Encoder(cfg).to(DEV)
    return pipe, enc, cfg, inp


def test_chain_unet_loss_to_embeddings_and_train_batch():
    import types

    from mdm_hip import trainer

    ops.set_grad_sink(None)
    pipe, enc, cfg, inp = _chain()
    vm = pipe.model.vision_model
    for p in vm.parameters():
        p.requires_grad_(False)
    mask = inp["mask"]
    g = _gen(9)
    toks = [cfg.vocab_size, 11]
    ids = torch.randint(1, cfg.vocab_size, mask.shape, generator=g)
    ids[0, 0], ids[1, 0], ids[0, 1], ids[1, 1] = toks[0], toks[0], toks[1], toks[1]
    assert bool(mask[:2, :2].all())
    ti = TXI.attach(enc, toks, init_ids=[3, 11])
    images = (torch.rand(mask.shape[0], 3, 16, 16, generator=g) * 2 - 1).to(DEV)

    def sample():
        return {"lm_outputs": enc(ids.numpy(), mask.numpy()), "lm_mask": mask.to(DEV), "images": images}

    # one get_loss + backward: the gradient of the embeddings is the oracle's VJP with the cotangent of this very run
    torch.manual_seed(100)
    pipe.train()
    smp = sample()
    smp["lm_outputs"].retain_grad()
    losses, _, _, _, _, weights = pipe.get_loss(smp)
    trainer._loss_of(losses, weights).backward()
    cot = smp["lm_outputs"].grad.detach().cpu()
    assert float(cot.abs().max()) > 0
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    ext = torch.cat([sd["shared.weight"], sd["shared.weight"][3:4]])
    ref = TI.oracle_table_grad(sd, cfg, ids, mask.float(), cot, table=ext)[toks]
    err = TC.rel_l2(ti.embeddings.grad, ref)
    print("chain: d loss / d embeddings vs oracle VJP %.3e" % err)
    assert err <= TI.GRAD_GATE
    assert all(p.grad is None for p in list(vm.parameters()) + list(enc.parameters()))

    # three optimizer steps over the embeddings alone
    ti.embeddings.grad = None
    base0 = {k: p.detach().clone() for k, p in list(vm.named_parameters()) + [("t5." + k, p) for k, p in enc.named_parameters()]}
    emb0 = ti.embeddings.detach().clone()
    opt = torch.optim.AdamW(ti.parameters(), lr=1e-2, weight_decay=0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
    args = types.SimpleNamespace(fp16=False, gradient_clip_norm=1.0)
    vals = []
    for i in range(3):
        torch.manual_seed(100 + i)
        vals.append(trainer.train_batch(pipe, sample(), opt, sched, None, args)[0])
    torch.cuda.synchronize()
    print("chain: train_batch losses %s, path: %s" % (vals, opt._mdm_fused_reason))
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in vals)
    assert not torch.equal(ti.embeddings.detach(), emb0)
    now = dict(list(vm.named_parameters()) + [("t5." + k, p) for k, p in enc.named_parameters()])
    assert all(torch.equal(now[k].detach(), v) for k, v in base0.items())
