"""CPU: the fp64 restatements of the text encoder's backward formulas (ti_cases.py) against torch autograd of the forward
formulas of t5_cases.py, the gradient fixture tests/golden/t5_grad.pt, and the host-side half of
mdm_hip.textual_inversion: attach / detach / merge, the refusals, the state dict, the range check of forward.
"""
import numpy as np
import pytest
import torch

import t5_cases as TC
import ti_cases as TI
from mdm_hip import _lib, text_encoder as TE, textual_inversion as TXI

EXACT = 1e-10
NEW_SYMBOLS = ["mdm_t5_attn_fwd_lse", "mdm_t5_attn_bwd", "mdm_t5_gated_gelu_bwd", "mdm_t5_rms_bwd", "mdm_t5_final_rms_bwd",
               "mdm_t5_embed_rms_slots", "mdm_t5_embed_bwd"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------
def test_attention_backward_restatement_is_autograd_of_the_forward():
    H, S, d = 2, 40, 64
    m = np.zeros((4, S), dtype=np.int64)
    m[0, :S] = 1
    m[1] = [1, 1, 0, 1, 0, 0, 1, 1, 1, 0] * 4
    m[3, :1] = 1                                             # row 2 is empty
    pk = TE.pack_index(m)
    T = pk["T"]
    g = _gen(1)
    qkv = torch.randn(T, 3 * H * d, generator=g, dtype=torch.float64)
    qkv[:, :H * d] *= d ** -0.5
    dout = torch.randn(T, H * d, generator=g, dtype=torch.float64)
    table = torch.randn(H, 2 * S - 1, generator=g, dtype=torch.float64)
    # the forward formula of t5_cases on the dense [B, S] layout
    dense = torch.zeros(4 * S, 3 * H * d, dtype=torch.float64)
    idx = torch.from_numpy(pk["idx"])
    dense[idx] = qkv
    dense.requires_grad_(True)
    q, k, v = (dense[:, i * H * d:(i + 1) * H * d].view(4, S, H, d).transpose(1, 2) for i in range(3))
    pos = torch.arange(S)
    bias = table[:, (pos[None, :] - pos[:, None]) + S - 1]                            # [H, q, k]
    mask = torch.from_numpy(m).double()
    kmask = mask.clone()
    kmask[2] = 1
    out_dense = TC.attention(q, k, v, bias, kmask).transpose(1, 2).reshape(4 * S, H * d)
    out, lse = TI.attn_forward(qkv, pk, table, H, S)
    assert TC.rel_l2(out, out_dense[idx]) <= EXACT
    (out_dense[idx] * dout).sum().backward()
    got = TI.attn_backward(qkv, out, lse, dout, pk, table, H, S)
    n = H * d
    for i, name in enumerate(("dq", "dk", "dv")):
        err = TC.rel_l2(got[:, i * n:(i + 1) * n], dense.grad[idx][:, i * n:(i + 1) * n])
        print("attention backward restatement %s: %.3e" % (name, err))
        assert err <= EXACT


def test_gated_gelu_backward_restatement():
    g = _gen(2)
    F = 24
    u = (torch.randn(7, 2 * F, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dy = torch.randn(7, F, generator=g, dtype=torch.float64)
    (TC.gelu_new(u[:, :F]) * u[:, F:] * dy).sum().backward()
    assert TC.rel_l2(TI.gated_gelu_backward(u.detach(), dy), u.grad) <= EXACT
    assert abs(TI.K_TANH - (2.0 / np.pi) ** 0.5) < 1e-15


def test_rms_backward_restatement():
    g = _gen(3)
    x = (torch.randn(5, 72, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    w = torch.rand(72, generator=g, dtype=torch.float64) + 0.5
    dh = torch.randn(5, 72, generator=g, dtype=torch.float64)
    (TC.rms(x, w, 1e-6) * dh).sum().backward()
    assert TC.rel_l2(TI.rms_backward(x.detach(), w, dh, 1e-6), x.grad) <= EXACT


def test_embedding_backward_restatement():
    g = _gen(4)
    token_ids = [7, 40, 3, 99]
    ids = torch.randint(0, 50, (60,), generator=g)
    ids[::4] = 7
    learned = torch.randn(4, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    table = torch.randn(50, 16, generator=g, dtype=torch.float64)
    slot = torch.full((100,), -1, dtype=torch.long)
    slot[token_ids] = torch.arange(4)
    x0 = torch.where((slot[ids] >= 0)[:, None], learned[slot[ids].clamp_min(0)], table[ids])
    dx0 = torch.randn(60, 16, generator=g, dtype=torch.float64)
    (x0 * dx0).sum().backward()
    start, tokens = TI.slot_index(ids.numpy(), token_ids)
    assert start[-1] == tokens.size and all(np.all(np.diff(tokens[start[j]:start[j + 1]]) > 0) for j in range(4))
    got = TI.embed_backward(dx0, start, tokens)
    assert TC.rel_l2(got, learned.grad) <= EXACT and bool((got[3] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return torch.load(TI.GOLDEN, weights_only=False)


def test_fixture_cases_and_reference_errors(gold):
    assert set(gold["cases"]) == set(TI.GRAD_CASES) and set(TI.BF16_GRAD_CASES) <= set(TI.GRAD_CASES)
    for name in TI.GRAD_CASES:
        g = gold["cases"][name]
        sums = TC.checksums(TC.weights(name))
        for k, s in g["param_sum"].items():
            assert abs(sums[k] - s) <= 1e-9 * max(1.0, abs(s)), k
        assert len(g["ref_fp32_error_per_draw"]) == len(g["ref_bf16_error_per_draw"]) == TC.DRAWS
        # the reference's own fp32 gradient leaves a factor ten under the gate it is a yardstick for
        assert 10 * g["ref_fp32_error"] < TI.GRAD_GATE, (name, g["ref_fp32_error"])
        for key in ("fp32", "bf16"):
            assert abs(g["ref_%s_spread" % key] - max(g["ref_%s_error_per_draw" % key]) / g["ref_%s_error" % key]) < 1e-12
            assert 1.0 <= g["ref_%s_spread" % key] < 1.5


@pytest.mark.parametrize("name", TI.GRAD_CASES)
def test_oracle_still_produces_the_fixture_dx0(name, gold):
    cfg, sd = TC.config(name), TC.weights(name)
    ids, mask = TC.inputs(name)
    G = TI.cotangents(name)
    dx0 = TI.oracle_dx0(sd, cfg, ids[0], mask, G[0])
    assert float(dx0[mask == 0].abs().max() if (mask == 0).any() else 0.0) == 0.0
    err = TC.rel_l2(TI.subsample_dx0(dx0, name), gold["cases"][name]["dx0_sub"])
    print("%s: oracle dx0 vs fixture %.3e" % (name, err))
    assert err <= 1e-9


def test_dx0_sums_to_the_table_gradient():
    """the two ways of asking the oracle agree: the table gradient is dx0 summed over the positions of each id"""
    name = "mini_holes"
    cfg, sd = TC.config(name), TC.weights(name)
    ids, mask = TC.inputs(name)
    G = TI.cotangents(name)
    dx0 = TI.oracle_dx0(sd, cfg, ids[0], mask, G[0])
    tg = torch.zeros(cfg.vocab_size, cfg.d_model, dtype=torch.float64).index_add_(0, ids[0].reshape(-1), dx0.reshape(-1, cfg.d_model))
    assert TC.rel_l2(tg, TI.oracle_table_grads(name)[0]) <= EXACT


# ---------------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------------
def _enc():
    return TC.build_module("mini")


def test_new_symbols_are_declared():
    names = {n for n, _, _, _ in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert set(NEW_SYMBOLS) <= names
    assert "text_encoder_bwd.hip" in _lib.SOURCES and _lib.ABI_VERSION == 6


def test_attach_initial_rows():
    enc = _enc()
    V, D = enc.config.vocab_size, enc.config.d_model
    table = enc.shared.weight.detach()
    ti = TXI.attach(enc, [5, 9])
    assert isinstance(ti, torch.nn.Module) and ti.embeddings.dtype == torch.float32 and ti.embeddings.requires_grad
    assert torch.equal(ti.embeddings.detach(), table[[5, 9]]) and [p is ti.embeddings for p in ti.parameters()] == [True]
    assert len(list(enc.parameters())) == len(list(_enc().parameters()))       # the encoder did not gain a parameter
    assert all(not p.requires_grad for p in enc.parameters())
    ti.detach()
    ti = TXI.attach(enc, torch.tensor([V, V + 3]), init_ids=[1, 2])
    assert torch.equal(ti.embeddings.detach(), table[[1, 2]])
    ti.detach()
    rows = torch.randn(2, D, generator=_gen(0))
    ti = TXI.attach(enc, [V + 1, 4], init=rows)
    assert torch.equal(ti.embeddings.detach(), rows) and ti.embeddings.data_ptr() != rows.data_ptr()
    assert ti.token_ids == [V + 1, 4] and ti.encoder is enc


def test_attach_refusals():
    enc = _enc()
    V, D = enc.config.vocab_size, enc.config.d_model
    with pytest.raises(ValueError, match="duplicate"):
        TXI.attach(enc, [3, 7, 3])
    with pytest.raises(ValueError, match=r"init must be \[2, %d\]" % D):
        TXI.attach(enc, [3, 7], init=torch.zeros(2, D + 1))
    with pytest.raises(ValueError, match="init must be"):
        TXI.attach(enc, [3, 7], init=torch.zeros(3, D))
    with pytest.raises(ValueError, match="beyond the vocabulary"):
        TXI.attach(enc, [V])                                  # an added token has no row to start from
    with pytest.raises(ValueError, match="init_ids"):
        TXI.attach(enc, [3, 7], init_ids=[1])
    with pytest.raises(ValueError, match="init_ids"):
        TXI.attach(enc, [3], init_ids=[V])
    with pytest.raises(ValueError, match="empty"):
        TXI.attach(enc, [])
    with pytest.raises(TypeError):
        TXI.attach(torch.nn.Linear(2, 2), [1])
    assert enc._adapter is None                               # a refused attach leaves nothing behind
    TXI.attach(enc, [3])
    with pytest.raises(_lib.MdmHipError, match="already attached"):
        TXI.attach(enc, [4])


def test_state_dict_round_trip():
    enc = _enc()
    V = enc.config.vocab_size
    ti = TXI.attach(enc, [V + 2, 17], init=torch.randn(2, enc.config.d_model, generator=_gen(1)))
    sd = ti.state_dict()
    assert set(sd) == {"embeddings", "_extra_state"} and sd["_extra_state"]["token_ids"] == [V + 2, 17]
    assert not any("shared" in k or "block" in k for k in sd)                  # the encoder is not in it
    ti.detach()
    enc2 = _enc()
    ti2 = TXI.attach(enc2, [1, 2])
    ti2._slot_table("cpu")
    ti2.load_state_dict(sd)
    assert ti2.token_ids == [V + 2, 17] and torch.equal(ti2.embeddings.detach(), sd["embeddings"])
    assert int(ti2._slot_table("cpu")[V + 2]) == 0 and int(ti2._slot_table("cpu")[17]) == 1 and int(ti2._slot_table("cpu")[1]) == -1
    with pytest.raises(ValueError, match="placeholder tokens"):
        TXI.attach(_enc(), [1, 2, 3]).load_state_dict(sd)
    assert set(enc2.state_dict()) == set(_enc().state_dict())                  # and the adapter is not in the encoder's


def test_merge_and_detach():
    enc = _enc()
    V, D = enc.config.vocab_size, enc.config.d_model
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    rows = torch.randn(2, D, generator=_gen(2))
    ti = TXI.attach(enc, [6, 200], init=rows)
    assert ti.detach() is ti and enc._adapter is None
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())      # exactly as before
    ti = TXI.attach(enc, [6, 200], init=rows)
    ti.merge()
    assert enc._adapter is None
    w = enc.shared.weight.detach()
    assert torch.equal(w[[6, 200]], rows) and enc.encoder.embed_tokens.weight is enc.shared.weight
    keep = torch.ones(V, dtype=torch.bool)
    keep[[6, 200]] = False
    assert torch.equal(w[keep], before["shared.weight"][keep])
    ti = TXI.attach(enc, [V + 1, 6], init=rows)
    with pytest.raises(_lib.MdmHipError, match="beyond the vocabulary"):
        ti.merge()
    assert enc._adapter is ti and torch.equal(enc.shared.weight.detach()[6], rows[0])   # a refused merge wrote nothing


def test_range_check_of_forward_knows_the_placeholders():
    """ids beyond the vocabulary pass the host-side check of forward only while attached.  The check is part of the host
    plan, which runs here on a CPU module with the device test and the pinned copy stubbed out."""
    enc = _enc()
    V = enc.config.vocab_size
    ids = np.array([[1, 2, V + 4, 0], [V + 4, 5, 0, 0]])
    mask = (ids != 0)

    import unittest.mock as mock

    from mdm_hip import ops

    with mock.patch.object(ops, "_require_gpu", lambda t: None), \
            mock.patch.object(torch.Tensor, "pin_memory", lambda self: self):
        with pytest.raises(ValueError, match=r"token id %d outside \[0, %d\)" % (V + 4, V)):
            enc._plan(ids, mask)
        ti = TXI.attach(enc, [V + 4], init_ids=[9])
        plan = enc._plan(ids, mask)
        assert plan["T"] == 5 and list(plan["ids_h"]) == [1, 2, V + 4, V + 4, 5]
        start, tokens = ti._slot_index(plan, "cpu")
        assert start.tolist() == [0, 2] and tokens.tolist() == [2, 3]
        bad = ids.copy()
        bad[0, 0] = V + 5
        with pytest.raises(ValueError, match="not a placeholder"):
            enc._plan(bad, mask)
        bad[0, 0] = -1
        with pytest.raises(ValueError, match="outside"):
            enc._plan(bad, mask)
        ti.detach()
        with pytest.raises(ValueError, match="outside"):
            enc._plan(ids, mask)


def test_language_model_keeps_the_graph():
    """LanguageModel.forward passes the encoder's output through .float() and nothing else: an fp32 tensor with a grad_fn
    comes out as it went in"""
    import inspect

    src = inspect.getsource(TE.LanguageModel.forward)
    assert "no_grad" not in src and ".detach()" not in src
    t = torch.zeros(2, 3, requires_grad=True) * 2
    assert t.float() is t
