#!/usr/bin/env python
"""Regional prompts (``sample(..., regions=rp)``) against classifier-free guidance alone, graphed, and the biased
cross-attention kernel against the two it is made from.  Development / reporting tool, in the method of tools/pag_bench.py:
the two legs of a comparison are alternated call by call in ONE process, device events around every call, ``--warmup`` calls
first, ``--calls`` timed; ms per iteration as median, min, max and p10-p90.
   python tools/region_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/region_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens: CFG alone against
CFG + three regional prompts (left third, middle third, right third of the image with feathered seams, weights 1, 1.4 and
0.8, over tokens [0, 10), [10, 20), [20, 30); two tokens in no span) on ``--region-layers`` (default "all").  The cases to
record: unet64 at batch 4 and 64, nested1024 at batch 4.  No ratio is required: the expected cost is the text pass run as a
second launch per layer.
``kernel``: mdm_attn_cross_bias (base = v) against mdm_attn_cross_addv, and ``ops.attention_biased`` (mdm_attn_fwd without
text keys + mdm_attn_cross_bias in place) against ``ops.attention`` (mdm_attn_fwd) on the same tensors at the shipped
shapes (L 64, d 96) and (L 256, d 64), S = 32, B x H = 64 (8 x 8: [uncond | cond] of a batch-4 sampling call), bf16,
``--launches`` launches per pair of events.
Result lines go to ``--out`` (profiles/region_sampling.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import configs, diffusion, ops, regions, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"L64_d96": (8, 64, 32, 8, 96), "L256_d64": (8, 256, 32, 8, 64)}   # B, L, S, H, d
S_TEXT = 32


def _stats(ts):
    pct = lambda q: sorted(ts)[min(len(ts) - 1, int(round(q * (len(ts) - 1))))]
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "p10_p90": [round(pct(0.1), 4), round(pct(0.9), 4)]}


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def three_regions(batch, side, dev, feather=0.06):
    """left / middle / right thirds of the image, linear ramps ``feather`` of the side wide, summing to 1 -> spans"""
    x = (torch.arange(side, dtype=torch.float32, device=dev) + 0.5) / side
    ramp = lambda edge: ((x - edge) / feather + 0.5).clamp(0, 1)
    a, b = ramp(1 / 3), ramp(2 / 3)
    bands = [1 - a, a - b, b]
    full = lambda v: v.clamp(0, 1).reshape(1, 1, 1, side).expand(batch, 1, side, side).contiguous()
    return [(0, 10, full(bands[0]), 1.0), (10, 20, full(bands[1]), 1.4), (20, 30, full(bands[2]), 0.8)]


def sampling(a):
    which, batch, n_it = a.which, a.batch, a.steps
    dev = torch.device("cuda:0")
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                loss_target_type="DDPM", schedule_shifted=which != "unet64", rescale_signal=1 if which != "unet64" else None,
                                schedule_shifted_power=2 if which == "nested1024" else 1)
    torch.manual_seed(0)
    if which == "unet64":
        net, side = mdm_hip.UNet(3, 3, configs.unet64_config(2048)), 64
        pipe = diffusion.Diffusion(net, diffusion.DiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False))
    else:
        net, side = mdm_hip.NestedUNet(3, 3, configs.nested1024_config(2048)), 1024
        pipe = diffusion.NestedDiffusion(net, diffusion.NestedDiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False,
                                                                              use_double_loss=True, no_use_residual=True))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
    pipe = pipe.to(dev)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(batch, S_TEXT, 2048, generator=g)
    smp = {"lm_outputs": torch.cat([torch.zeros_like(cond), cond]).to(dev), "lm_mask": torch.ones(2 * batch, S_TEXT).to(dev)}
    rp = mdm_hip.RegionPrompts(S_TEXT, side, three_regions(batch, side, dev), rows=batch, device=dev)
    gs = GraphedSampler(pipe, seed=0)
    legs = {"cfg": {}, "cfg_regions": {"regions": rp, "region_layers": a.region_layers}}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    names = regions.layer_names(net, a.region_layers)
    bias = {"%dx%d" % hw: list(t.shape) for hw, t in next(e["bias"] for e in gs._graphs.values() if e["bias"] is not None).buffers.items()}
    res = {"tool": "region_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "regions": "three feathered thirds, weights 1 / 1.4 / 0.8", "region_layers": len(names), "bias_buffers": bias,
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    res["regions_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_regions"]["median"] / res["ms_per_iteration"]["cfg"]["median"], 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    res = {"tool": "region_bench kernel", "kernels": "mdm_attn_cross_bias / mdm_attn_cross_addv / mdm_attn_fwd, bf16, S = 32, B x H = 64",
           "calls": a.calls, "warmup": a.warmup, "launches_per_event_pair": a.launches, "shapes": {}}
    for tag, (B, L, S, H, d) in KERNEL_SHAPES.items():
        g = torch.Generator().manual_seed(2)
        qkv = torch.randn(B, L, 3 * H * d, generator=g).to(dev, torch.bfloat16)
        kvc = torch.randn(B, S, 2 * H * d, generator=g).to(dev, torch.bfloat16)
        bias = (torch.randn(B, L, S, generator=g) * 2).to(dev)
        legs = {"attn_fwd": lambda: ops.attention(qkv, kvc, None, H),
                "attention_biased": lambda: ops.attention_biased(qkv, kvc, None, bias, H),
                "attn_cross_addv": lambda: ops.attn_cross_addv(qkv, kvc, None, H),
                "attn_cross_bias": lambda: ops.attn_cross_bias(qkv, kvc, None, bias, H)}
        times = {k: [] for k in legs}
        with torch.no_grad():
            for it in range(a.warmup + a.calls):
                for k, fn in legs.items():
                    def many():
                        for _ in range(a.launches):
                            out = fn()
                        return out

                    ms, out = _timed(many)
                    if it >= a.warmup:
                        times[k].append(1e3 * ms / a.launches)
        st = {k: _stats(ts) for k, ts in times.items()}
        res["shapes"][tag] = {"B_L_S_H_d": [B, L, S, H, d], "us_per_call": st, "finite": bool(torch.isfinite(out).all()),
                              "cross_bias_over_cross_addv_median": round(st["attn_cross_bias"]["median"] / st["attn_cross_addv"]["median"], 3),
                              "attention_biased_over_attn_fwd_median": round(st["attention_biased"]["median"] / st["attn_fwd"]["median"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--region-layers", default="all")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the result line to this file")
    a = ap.parse_args()
    res = sampling(a) if a.what == "sampling" else kernel(a)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
