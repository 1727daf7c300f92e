"""Seeded T5-encoder cases shared by the CPU tests, the GPU tests and tools/make_t5_golden.py.

The oracle here is a plain-torch T5 v1.1 / flan encoder written from the formulas (RMS norm without mean or bias,
un-scaled scores + shared bucketed relative bias, gated tanh-GELU); it takes a dtype, so it runs in fp64.  The CPU tests
pin it to ``transformers.T5EncoderModel`` (live, and through tests/golden/t5_encoder.pt); the GPU tests compare the HIP
encoder with it on the full tensors.

Weights are drawn per tensor from ``torch.Generator().manual_seed(...)`` at O(1) activation scale: linear weights with
std 1 / sqrt(fan_in), norm weights uniform in [0.5, 1.5], the embedding and the bias table with std 1 (a freshly
constructed Hugging Face model is too close to zero to test anything).
"""
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_encoder.pt")
DRAWS = 4       # seeded input draws per case: an error is taken over their concatenation

# name: config fields, S, the rows' masks (an int = that many leading valid tokens, a list = explicit 0/1 row), and the
# channel stride of the subsample the fixture keeps of the valid rows
CASES = {
    # the probe geometry: 3 layers, 4 heads x 64; 115 of 231 tokens valid
    "mini": dict(cfg=dict(vocab_size=512, d_model=256, d_kv=64, d_ff=640, num_layers=3, num_heads=4), S=77,
                 rows=[77, 33, 5], sub=4),
    # a mask with holes next to a full row and suffix padding; 64 of 120 valid
    "mini_holes": dict(cfg=dict(vocab_size=512, d_model=256, d_kv=64, d_ff=640, num_layers=3, num_heads=4), S=40,
                       rows=[40, [1, 1, 0, 1, 0, 0, 1, 1, 1, 0] * 4, 0], sub=4),
    # flan-t5-xl geometry, 2 layers, small vocabulary; 216 of 512 valid
    "xl2": dict(cfg=dict(vocab_size=256, d_model=2048, d_kv=64, d_ff=5120, num_layers=2, num_heads=32), S=128,
                rows=[128, 61, 20, 7], sub=64),
    # depth: 24 layers at d_model 512 at a caption's length (S = 64; 84 of 128 valid).  The weights follow the rule of the
    # module docstring with ONE addition: the query weights carry the factor d_kv^-0.5 that T5's own initialisation gives
    # them (q std = (d_model d_kv)^-0.5 -- it absorbs the 1 / sqrt(d) the attention omits).  Without it the rule does not
    # give what it is for, O(1) activations: the scores have a standard deviation near 9, every softmax is close to an
    # arg-max, and over 24 layers a rounding error that flips one decides the output.  Measured on the REFERENCE alone
    # (transformers on the CPU against the fp64 oracle, rel-L2 as everywhere), un-scaled queries, S = 64: fp32 1.5e-3 --
    # above the 1e-4 gate itself -- and 0.855 under bf16 autocast, where rounding only the WEIGHTS to bf16 already moves
    # the fp64 output by 0.84.  With the factor: fp32 1.6e-6, bf16 autocast 1.64e-2 with a spread of +-2 % between input
    # draws, and an error that grows with depth shows as such.
    "deep24_t5init": dict(cfg=dict(vocab_size=256, d_model=512, d_kv=64, d_ff=1024, num_layers=24, num_heads=8), S=64,
                          rows=[64, 20], sub=8, q_scale=64 ** -0.5),
    # 24 layers with the un-scaled rule, as far as it can carry a gate.  How often a flip happens grows with the number
    # of keys that compete; the reference's own fp32 error is 1.5e-3 at S = 64, 2e-4 at S = 16, 8e-5 at S = 8, 1.6e-5 at
    # S = 4, 7.8e-6 at S = 3.  The case takes the longest S that leaves a factor ten under the fp32 gate, S = 3, and makes
    # up the token count with rows (32 rows, 66 of 96 tokens valid).  It is an fp32 case only: under bf16 autocast the
    # reference's own error is 6.5e-2 with a spread of 5.8e-2 ... 7.2e-2 between the four input draws (weights-only
    # rounding: 7.7e-2), so "no worse than the reference, no margin" is decided by which inputs were drawn -- an MI355X
    # run of this package read 6.555e-2 against 6.471e-2.
    "deep24": dict(cfg=dict(vocab_size=256, d_model=512, d_kv=64, d_ff=1024, num_layers=24, num_heads=8), S=3,
                   rows=[3] * 12 + [2] * 10 + [1] * 10, sub=8),
}
# gated in fp32 AND bf16; at least one full-length row and >= 25 % valid tokens each
MODEL_CASES = ["mini", "xl2", "deep24_t5init"]
FP32_ONLY_CASES = ["deep24"]
FIXTURE_CASES = list(CASES)


def _hash(s):
    h = 1469598103934665603
    for ch in s.encode():
        h = ((h ^ ch) * 1099511628211) % (2 ** 64)
    return h


def _gen(name, key):
    return torch.Generator().manual_seed(_hash(name + "/" + key) % (2 ** 31))


def config(name):
    from mdm_hip.text_encoder import T5EncoderConfig

    return T5EncoderConfig(**CASES[name]["cfg"])


def state_dict_keys(cfg):
    """{key: shape} of a ``transformers.T5EncoderModel`` state_dict for this geometry"""
    inner = cfg.num_heads * cfg.d_kv
    keys = {"shared.weight": (cfg.vocab_size, cfg.d_model), "encoder.embed_tokens.weight": (cfg.vocab_size, cfg.d_model)}
    for l in range(cfg.num_layers):
        p = "encoder.block.%d.layer." % l
        for n in "qkv":
            keys[p + "0.SelfAttention.%s.weight" % n] = (inner, cfg.d_model)
        keys[p + "0.SelfAttention.o.weight"] = (cfg.d_model, inner)
        if l == 0:
            keys[p + "0.SelfAttention.relative_attention_bias.weight"] = (cfg.relative_attention_num_buckets, cfg.num_heads)
        keys[p + "0.layer_norm.weight"] = (cfg.d_model,)
        keys[p + "1.DenseReluDense.wi_0.weight"] = (cfg.d_ff, cfg.d_model)
        keys[p + "1.DenseReluDense.wi_1.weight"] = (cfg.d_ff, cfg.d_model)
        keys[p + "1.DenseReluDense.wo.weight"] = (cfg.d_model, cfg.d_ff)
        keys[p + "1.layer_norm.weight"] = (cfg.d_model,)
    keys["encoder.final_layer_norm.weight"] = (cfg.d_model,)
    return keys


def weights(name, cfg=None):
    """the case's fp32 state_dict (keys of T5EncoderModel; the two embedding keys hold one tensor)"""
    cfg = cfg or config(name)
    sd = {}
    for k, shape in state_dict_keys(cfg).items():
        if k == "encoder.embed_tokens.weight":
            sd[k] = sd["shared.weight"]
        elif k.endswith("layer_norm.weight"):
            sd[k] = torch.rand(shape, generator=_gen(name, k)) + 0.5
        elif k == "shared.weight" or "relative_attention_bias" in k:
            sd[k] = torch.randn(shape, generator=_gen(name, k))
        else:
            sd[k] = torch.randn(shape, generator=_gen(name, k)) * shape[1] ** -0.5
            if k.endswith("SelfAttention.q.weight"):
                sd[k] = sd[k] * CASES[name].get("q_scale", 1.0)
    return sd


def checksums(sd):
    return {k: float(v.double().sum()) for k, v in sd.items()}


def mask_of(name):
    S, rows = CASES[name]["S"], CASES[name]["rows"]
    m = torch.zeros(len(rows), S)
    for b, r in enumerate(rows):
        if isinstance(r, int):
            m[b, :r] = 1
        else:
            m[b] = torch.tensor(r, dtype=torch.float32)
    return m


def inputs(name):
    """(ids [DRAWS, B, S] long, mask [B, S] float)"""
    m = mask_of(name)
    g = _gen(name, "ids")
    ids = torch.randint(0, CASES[name]["cfg"]["vocab_size"], (DRAWS,) + tuple(m.shape), generator=g)
    return ids, m


def bucket(rel, num_buckets=32, max_distance=128):
    """bidirectional T5 bucket of rel = key position - query position (fp32 arithmetic, as the reference's model)"""
    nb = num_buckets // 2
    n = rel.abs()
    half = nb // 2
    big = half + (torch.log(n.to(torch.float32) / half) / math.log(max_distance / half) * (nb - half)).to(torch.long)
    big = big.clamp(max=nb - 1)
    return torch.where(rel > 0, nb, 0) + torch.where(n < half, n, big)


def rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def gelu_new(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def attention(q, k, v, bias, mask):
    """q, k, v [B, H, S, d]; bias [H, S, S]; mask [B, S] -> [B, H, S, d]; no 1 / sqrt(d)"""
    s = q @ k.transpose(-1, -2) + bias[None]
    s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def oracle_forward(sd, cfg, ids, mask, dtype=torch.float64):
    """[B, S, d_model] of ``dtype``, zero at masked positions.  Rows with no valid token yield zeros."""
    W = lambda k: sd[k].to(dtype)
    B, S = ids.shape
    H, dk, eps = cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
    pos = torch.arange(S)
    bk = bucket(pos[None, :] - pos[:, None], cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
    bias = W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")[bk].permute(2, 0, 1)   # [H, q, k]
    mask = mask.to(dtype)
    live = mask.sum(1) > 0
    kmask = mask.clone()
    kmask[~live] = 1           # an all-pad row would be softmax over nothing; its output is zeroed below
    x = W("shared.weight")[ids]
    heads = lambda t: t.view(B, S, H, dk).transpose(1, 2)
    for l in range(cfg.num_layers):
        p = "encoder.block.%d.layer." % l
        h = rms(x, W(p + "0.layer_norm.weight"), eps)
        q, k, v = (heads(h @ W(p + "0.SelfAttention.%s.weight" % n).t()) for n in "qkv")
        a = attention(q, k, v, bias, kmask).transpose(1, 2).reshape(B, S, H * dk)
        x = x + a @ W(p + "0.SelfAttention.o.weight").t()
        h = rms(x, W(p + "1.layer_norm.weight"), eps)
        u = gelu_new(h @ W(p + "1.DenseReluDense.wi_0.weight").t()) * (h @ W(p + "1.DenseReluDense.wi_1.weight").t())
        x = x + u @ W(p + "1.DenseReluDense.wo.weight").t()
    return rms(x, W("encoder.final_layer_norm.weight"), eps) * mask[..., None]


_oracle_cache = {}


def oracle_outputs(name):
    """fp64 oracle outputs of the case's DRAWS input draws, [DRAWS, B, S, D] (computed once per process)"""
    if name not in _oracle_cache:
        cfg, sd = config(name), weights(name)
        ids, m = inputs(name)
        with torch.no_grad():
            _oracle_cache[name] = torch.stack([oracle_forward(sd, cfg, ids[i], m, torch.float64) for i in range(DRAWS)])
    return _oracle_cache[name]


def valid_rows(t, mask):
    """[..., B, S, D] -> [..., T, D]: the valid tokens, in row order"""
    return t[..., mask.bool(), :]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def subsample(t, name):
    """what the fixture keeps of an output [DRAWS, B, S, D]: every ``sub``-th channel of the valid rows"""
    return valid_rows(t, mask_of(name))[..., :: CASES[name]["sub"]].float().contiguous()


def build_module(name, device=None):
    """our module with the case's weights"""
    from mdm_hip.text_encoder import T5Encoder

    m = T5Encoder(config(name))
    m.load_state_dict(weights(name))
    return m.to(device) if device is not None else m
