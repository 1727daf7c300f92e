#!/usr/bin/env python
"""Time mdm_hip.T5Encoder against plain torch on the flan-t5-xl geometry (24 layers, d_model 2048, 32 x 64 heads,
gated-GELU d_ff 5120, random weights), bf16.

Legs, alternated call by call inside ONE process (device events around every call, warm-up first):
  ours      mdm_hip.T5Encoder under bf16 autocast, ids and mask as host arrays (the reader's form): packing included
  baseline  the plain-torch oracle of tests/t5_cases.py on the GPU under bf16 autocast (vendor GEMMs + torch softmax) on
            the PADDED batch; its linear weights are stored in bf16 and its bias [H, S, S] is built once per S, so
            neither a per-call weight cast nor the bucket arithmetic is charged to it
  hf        transformers.T5EncoderModel under bf16 autocast, where transformers imports
Workloads
  full    B = 64, S = 128, every token valid
  ragged  B = 64, seeded lengths uniform in 8 ... 64, padded to the longest (a stand-in for captions, not a measured
          distribution)
  small   B = 8, S = 32, every token valid (sampling with guidance)
Next to each time: the algorithmic GEMM FLOPs of the VALID tokens and of the padded batch, and the weight bytes.

    python tools/text_encoder_bench.py [--calls 20] [--warmup 3] [--layers 24] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/text_encoder_bench.py --only ours --workload ragged --calls 5
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ml-mdm_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
sys.dont_write_bytecode = True

import t5_cases as TC  # noqa: E402
from mdm_hip import text_encoder as TE  # noqa: E402

DEV = "cuda:0"


def workloads():
    rng = np.random.RandomState(0)
    lens = rng.randint(8, 65, size=64)
    w = {}
    for name, B, S, ln in (("full", 64, 128, None), ("ragged", 64, int(lens.max()), lens), ("small", 8, 32, None)):
        mask = np.ones((B, S), dtype=np.float32)
        if ln is not None:
            mask = (np.arange(S)[None, :] < ln[:, None]).astype(np.float32)
        ids = rng.randint(1, 32128, size=(B, S)).astype(np.int64) * (mask != 0)
        w[name] = (ids, mask)
    return w


def gemm_flops(cfg, tokens):
    inner = cfg.num_heads * cfg.d_kv
    per_token = 2 * (cfg.d_model * 3 * inner + inner * cfg.d_model + cfg.d_model * 2 * cfg.d_ff + cfg.d_ff * cfg.d_model)
    return float(per_token) * cfg.num_layers * tokens


def attn_flops(cfg, lens):
    return float(sum(4 * int(n) * int(n) * cfg.d_kv * cfg.num_heads for n in lens)) * cfg.num_layers


def weight_bytes(cfg):
    inner = cfg.num_heads * cfg.d_kv
    return 2.0 * cfg.num_layers * (4 * cfg.d_model * inner + 3 * cfg.d_model * cfg.d_ff)


class Baseline:
    """tests/t5_cases.oracle_forward with the per-call constant work hoisted; fp32 norms / embedding, bf16 linear weights"""

    def __init__(self, ours, cfg):
        self.cfg = cfg
        sd = ours.state_dict()
        self.sd = {k: (v.to(torch.bfloat16) if v.dim() == 2 and "shared" not in k and "embed" not in k and "bias" not in k
                       else v) for k, v in sd.items()}
        self.bias = {}

    def __call__(self, ids, mask):
        cfg, sd = self.cfg, self.sd
        B, S = ids.shape
        H, dk, eps = cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
        if S not in self.bias:
            pos = torch.arange(S)
            bk = TC.bucket(pos[None, :] - pos[:, None], cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
            self.bias[S] = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bk.to(DEV)].permute(2, 0, 1)
        bias = self.bias[S]
        x = sd["shared.weight"][ids]
        heads = lambda t: t.view(B, S, H, dk).transpose(1, 2)
        for l in range(cfg.num_layers):
            p = "encoder.block.%d.layer." % l
            h = TC.rms(x, sd[p + "0.layer_norm.weight"], eps)
            q, k, v = (heads(torch.nn.functional.linear(h, sd[p + "0.SelfAttention.%s.weight" % n])) for n in "qkv")
            a = TC.attention(q, k, v, bias, mask).transpose(1, 2).reshape(B, S, H * dk)
            x = x + torch.nn.functional.linear(a, sd[p + "0.SelfAttention.o.weight"])
            h = TC.rms(x, sd[p + "1.layer_norm.weight"], eps)
            u = TC.gelu_new(torch.nn.functional.linear(h, sd[p + "1.DenseReluDense.wi_0.weight"])) * \
                torch.nn.functional.linear(h, sd[p + "1.DenseReluDense.wi_1.weight"])
            x = x + torch.nn.functional.linear(u, sd[p + "1.DenseReluDense.wo.weight"])
        return TC.rms(x, sd["encoder.final_layer_norm.weight"], eps) * mask[..., None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--only", default=None, help="one leg (ours | baseline | hf): no alternation, for a profiler run")
    ap.add_argument("--workload", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    assert a.calls >= 1

    cfg = TE.T5EncoderConfig(vocab_size=32128, d_model=2048, d_kv=64, d_ff=5120, num_layers=a.layers, num_heads=32)
    torch.manual_seed(0)
    with torch.device(DEV):
        ours = TE.T5Encoder(cfg)
    with torch.no_grad():      # T5-like scales: O(1) scores, as a trained checkpoint has
        for blk in ours.encoder.block:
            blk.layer[0].SelfAttention.q.weight.mul_(cfg.d_kv ** -0.5)
    legs = {}
    if a.only in (None, "baseline"):
        base = Baseline(ours, cfg)
        legs["baseline"] = lambda ids, mask, g: base(g[0], g[1])
    if a.only in (None, "hf"):
        try:
            from transformers import T5Config, T5EncoderModel
            with torch.device(DEV):
                hf = T5EncoderModel(T5Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff,
                                             num_layers=cfg.num_layers, num_heads=cfg.num_heads, feed_forward_proj="gated-gelu",
                                             dropout_rate=0.0, use_cache=False)).eval()
            hf.load_state_dict(ours.state_dict())
            legs["hf"] = lambda ids, mask, g: hf(input_ids=g[0], attention_mask=g[1]).last_hidden_state * g[1][..., None]
        except ImportError:
            print("transformers does not import here: no hf leg", flush=True)
    if a.only in (None, "ours"):
        legs["ours"] = lambda ids, mask, g: ours(ids, mask)

    result = {"geometry": dataclass_dict(cfg), "calls": a.calls, "warmup": a.warmup, "weight_bytes_bf16": weight_bytes(cfg),
              "workloads": {}}
    for wname, (ids, mask) in workloads().items():
        if a.workload and wname != a.workload:
            continue
        g = (torch.from_numpy(ids).to(DEV), torch.from_numpy(mask).to(DEV))
        lens = mask.sum(1)
        times = {k: [] for k in legs}
        outs = {}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for it in range(a.warmup + a.calls):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    o = fn(ids, mask, g)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[k].append(e0.elapsed_time(e1))
                    outs[k] = o
        valid, padded = float(lens.sum()), float(mask.size)
        row = {"B": int(mask.shape[0]), "S": int(mask.shape[1]), "valid_tokens": int(valid),
               "gemm_tflop_valid": gemm_flops(cfg, valid) / 1e12, "gemm_tflop_padded": gemm_flops(cfg, padded) / 1e12,
               "attn_tflop_valid": attn_flops(cfg, lens) / 1e12, "legs": {}}
        for k, ts in times.items():
            med = statistics.median(ts)
            row["legs"][k] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
                              "ms_p10_p90": [float(np.percentile(ts, 10)), float(np.percentile(ts, 90))],
                              "useful_gemm_tflops": row["gemm_tflop_valid"] / (med / 1e3)}
        if "ours" in outs and "baseline" in outs:
            m = g[1].bool()
            row["rel_l2_ours_vs_baseline"] = TC.rel_l2(outs["ours"][m], outs["baseline"].float()[m])
        result["workloads"][wname] = row
        print(wname, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


def dataclass_dict(c):
    import dataclasses

    return dataclasses.asdict(c)


if __name__ == "__main__":
    main()
