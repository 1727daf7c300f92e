"""CPU: the T5 text encoder's oracle pinned to ``transformers`` (live and through tests/golden/t5_encoder.pt), and the
host-side half of mdm_hip.text_encoder: bucket function, packing plan, state-dict keys, ABI symbols, no CPU fallback.

fp32 comparisons are gated at 1e-4, the project's forward gate (smoke(), check_summary).
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import t5_cases as TC
from mdm_hip import _lib, text_encoder as TE

TOL = 1e-4
NEW_SYMBOLS = ["mdm_t5_embed_rms", "mdm_t5_add_rms", "mdm_t5_final_rms", "mdm_t5_gated_gelu", "mdm_t5_attn_fwd"]


@pytest.fixture(scope="module")
def gold():
    return torch.load(TC.GOLDEN, weights_only=False)


@contextlib.contextmanager
def _transformers():
    """``transformers`` probes optional packages with importlib.util.find_spec, which raises ValueError on the spec-less
    stub modules (mlx, torchvision ...) that oracle/ref_import.py leaves in sys.modules once a reference-marked test has
    run in the same process: hide those while it imports and builds a model (it imports its model files lazily)"""
    roots = ("torchinfo", "simple_parsing", "dataclass_wizard", "mlx", "torchvision", "boto3")
    hidden = {k: m for k, m in list(sys.modules.items())
              if m is not None and getattr(m, "__spec__", None) is None and k.split(".")[0] in roots}
    for k in hidden:
        del sys.modules[k]
    try:
        yield pytest.importorskip("transformers")
    finally:
        sys.modules.update(hidden)


def _hf_model(name):
    with _transformers():
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
        import make_t5_golden

        return make_t5_golden.hf_model(name)


@pytest.mark.parametrize("name", ["mini", "mini_holes"])
def test_oracle_matches_transformers_live(name):
    hf = _hf_model(name)
    ids, mask = TC.inputs(name)
    ref = TC.oracle_outputs(name)
    with torch.no_grad():
        out = torch.stack([hf(input_ids=ids[i], attention_mask=mask).last_hidden_state * mask[..., None]
                           for i in range(TC.DRAWS)])
    err = TC.rel_l2(TC.valid_rows(out, mask), TC.valid_rows(ref, mask))
    print("%s: fp64 oracle vs transformers fp32 %.3e" % (name, err))
    assert err < TOL
    assert float(ref[:, mask == 0].abs().max()) == 0.0 if (mask == 0).any() else True


@pytest.mark.parametrize("name", TC.FIXTURE_CASES)
def test_fixture_is_of_these_weights_and_inputs(name, gold):
    g = gold["cases"][name]
    sums = TC.checksums(TC.weights(name))
    assert set(sums) == set(g["param_sum"])
    for k, s in g["param_sum"].items():
        assert abs(sums[k] - s) <= 1e-9 * max(1.0, abs(s)), k
    ids, mask = TC.inputs(name)
    assert torch.equal(ids, g["ids"].long()) and torch.equal(mask, g["mask"].float())


@pytest.mark.parametrize("name", TC.FIXTURE_CASES)
def test_oracle_matches_fixture(name, gold):
    g = gold["cases"][name]
    err = TC.rel_l2(TC.subsample(TC.oracle_outputs(name), name), g["out_sub"])
    print("%s: fp64 oracle vs fixture (transformers fp32) %.3e; stored: fp32 %.3e, bf16 autocast %.3e"
          % (name, err, g["ref_fp32_error"], g["ref_bf16_error"]))
    assert err < TOL
    assert 10 * g["ref_fp32_error"] < TOL < g["ref_bf16_error"]      # a case can carry the gate: the reference is well under it


def test_bucket_function_matches_fixture_table(gold):
    rel, table = gold["bucket_rel"], gold["bucket"]
    assert torch.equal(TE.relative_bucket(rel), table)
    assert torch.equal(TC.bucket(rel), table)
    for S in range(1, 513):
        assert torch.equal(TE.bias_index(S), table[511 - (S - 1):511 + S]), S
    # the named points of the definition: sign half, exact range, log range, cap
    b = lambda r: int(TE.relative_bucket(torch.tensor([r]))[0])
    assert [b(0), b(-1), b(1), b(-7), b(7), b(-8), b(8), b(-127), b(127), b(-500), b(500)] == \
        [0, 1, 17, 7, 23, 8, 24, 15, 31, 15, 31]


def _plan_by_hand(m):
    B, S = m.shape
    idx, pos, start = [], [], [0]
    for b in range(B):
        for s in range(S):
            if m[b, s]:
                idx.append(b * S + s)
                pos.append(s)
        start.append(len(idx))
    src = [-1] * (B * S)
    for t, i in enumerate(idx):
        src[i] = t
    return idx, start, pos, src


@pytest.mark.parametrize("kind", ["suffix", "holes", "all_pad_row", "S1", "empty"])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_pack_index(kind, as_tensor):
    m = {
        "suffix": np.array([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]]),
        "holes": np.array([[1, 0, 1, 1, 0, 1], [0, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 1]]),
        "all_pad_row": np.array([[1, 1, 0], [0, 0, 0], [0, 1, 1]]),
        "S1": np.array([[1], [0], [1]]),
        "empty": np.zeros((2, 4), dtype=np.int64),
    }[kind]
    pk = TE.pack_index(torch.from_numpy(m).float() if as_tensor else m)
    idx, start, pos, src = _plan_by_hand(m)
    assert pk["idx"].tolist() == idx and pk["seq_start"].tolist() == start
    assert pk["pos"].tolist() == pos and pk["src"].tolist() == src
    assert pk["T"] == len(idx) and pk["max_len"] == int(m.sum(1).max())
    assert pk["seq_start"].dtype == np.int32 and pk["pos"].dtype == np.int32 and pk["src"].dtype == np.int32


def test_state_dict_keys():
    cfg = TC.config("mini")
    ours = TE.T5Encoder(cfg)
    sd = ours.state_dict()
    want = TC.state_dict_keys(cfg)
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert sd["shared.weight"].data_ptr() == sd["encoder.embed_tokens.weight"].data_ptr()      # tied
    assert not any(p.requires_grad for p in ours.parameters())
    assert ours.embed_dim == cfg.d_model and ours.load() is None


def test_state_dict_keys_equal_transformers_both_ways():
    hf = _hf_model("mini")
    ours = TE.T5Encoder(TE.T5EncoderConfig.from_hf(hf.config))
    assert set(ours.state_dict()) == set(hf.state_dict())
    assert ours.load_state_dict(hf.state_dict()) is not None                 # strict: ours <- theirs
    missing, unexpected = hf.load_state_dict(ours.state_dict(), strict=False)      # theirs <- ours
    assert not missing and not unexpected
    for k, v in hf.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k


def test_loads_a_conditional_generation_checkpoint():
    c = TC.config("mini")
    with _transformers() as tr:
        full = tr.T5ForConditionalGeneration(tr.T5Config(
            vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, num_layers=2, num_decoder_layers=1,
            num_heads=c.num_heads, feed_forward_proj="gated-gelu"))
    ours = TE.T5Encoder(TE.T5EncoderConfig.from_hf(full.config))
    assert ours.config.num_layers == 2 and ours.config.feed_forward_proj == "gated-gelu"
    missing, unexpected = ours.load_state_dict(full.state_dict(), strict=False)
    assert not missing
    assert unexpected and all(k.startswith(("decoder.", "lm_head.")) for k in unexpected)
    assert torch.equal(ours.state_dict()["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"],
                       full.state_dict()["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"])


def test_config():
    class Cfg:      # any object with the attributes
        vocab_size, d_model, d_kv, d_ff, num_layers, num_heads = 100, 64, 64, 128, 2, 1
        relative_attention_num_buckets, layer_norm_epsilon, feed_forward_proj = 16, 1e-5, "gated-gelu"

    c = TE.T5EncoderConfig.from_hf(Cfg)
    assert (c.vocab_size, c.d_model, c.relative_attention_num_buckets, c.relative_attention_max_distance,
            c.layer_norm_epsilon) == (100, 64, 16, 128, 1e-5)
    Cfg.feed_forward_proj = "relu"
    with pytest.raises(NotImplementedError):
        TE.T5EncoderConfig.from_hf(Cfg)
    with pytest.raises(NotImplementedError):
        TE.T5EncoderConfig(100, 64, 64, 128, 2, 1, feed_forward_proj="gated-silu")


def test_product_code_does_not_import_transformers():
    src = open(TE.__file__).read()
    assert "import transformers" not in src and "from transformers" not in src


def test_new_symbols_declared_and_exported():
    declared = {name for name, _, _, _ in _lib.header_prototypes()}
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert getattr(L, s) is not None
    assert _lib.ABI_VERSION == 6 and "text_encoder.hip" in _lib.SOURCES


def test_cpu_tensor_raises():
    m = TE.T5Encoder(TC.config("mini"))
    ids, mask = TC.inputs("mini")
    with pytest.raises(_lib.MdmHipError):
        m(ids[0], mask)
    with pytest.raises(_lib.MdmHipError):
        m(ids[0].numpy(), mask.numpy())


def test_packed_weight_forward_only_is_opt_in():
    import inspect

    from mdm_hip import ops

    sig = inspect.signature(ops.packed_weight)
    assert sig.parameters["forward_only"].default is False


def test_language_model_precomputed_branch_on_host():
    """the use_precomputed_text_embeddings branch needs no encoder and no GPU: embeddings x pad mask"""
    from types import SimpleNamespace as NS

    args = NS(use_precomputed_text_embeddings=True, categorical_conditioning=False, fp16=False,
              reader_config=NS(padding_token="<pad>"))
    tok = NS(token_id=lambda t: 0)
    lm = TE.LanguageModel(args, TE.T5Encoder(TC.config("mini")))
    assert lm.model is None and lm.embed_dim == 256
    tokens = np.array([[5, 9, 0, 0], [7, 0, 3, 1]])
    emb = torch.randn(2, 4, 8, generator=torch.Generator().manual_seed(0))
    for tk in (tokens, torch.from_numpy(tokens)):
        out, mask = lm({"tokens": tk, "text_embedding": emb}, tok)
        assert mask.tolist() == [[1, 1, 0, 0], [1, 0, 1, 1]]
        assert torch.equal(out, emb * mask.unsqueeze(-1))
