#!/usr/bin/env python
"""Cross-attention map recording (``sample(..., attn_maps=maps)``) against classifier-free guidance alone, graphed, and the
map kernel against the kernel it mirrors.  Development / reporting tool, in the method of tools/region_bench.py: the two legs
of a comparison are alternated call by call in ONE process, device events around every call, ``--warmup`` calls first,
``--calls`` timed; ms per iteration as median, min, max and p10-p90.
   python tools/attn_maps_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/attn_maps_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens: CFG alone against
CFG + recording on ``--layers`` (default "all"), every step.  The cases to record: unet64 at batch 4 and 64, nested1024 at
batch 4.  No ratio is required (the feature is opt-in): the expected cost is one launch per layer that re-reads q (B L C) and
k_c (B S C) of the conditional rows and reads and writes B L ld floats.
``kernel``: mdm_attn_cross_maps against mdm_attn_cross_addv on the same tensors at the shipped shapes (L 64, d 96) and
(L 256, d 64), S = 32, B = 4 and H = 8 (the conditional block of a batch-4 sampling call; the mirrored kernel gets the same B),
bf16, ``--launches`` launches per pair of events; and with S = 77 (two key tiles: the two-pass path).
Result lines go to ``--out`` (profiles/attn_maps_sampling.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import attn_maps, configs, diffusion, ops, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"L64_d96": (4, 64, 32, 8, 96), "L256_d64": (4, 256, 32, 8, 64),
                 "L64_d96_S77": (4, 64, 77, 8, 96), "L256_d64_S77": (4, 256, 77, 8, 64)}   # B, L, S, H, d
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
    maps = mdm_hip.AttnMaps(S_TEXT, batch, layers=a.layers)
    gs = GraphedSampler(pipe, seed=0)
    legs = {"cfg": {}, "cfg_maps": {"attn_maps": maps}}
    times, finite, same = {k: [] for k in legs}, True, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            outs = {}
            for k, kw in legs.items():
                torch.manual_seed(5)
                maps.reset()
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                outs[k] = out
                finite = finite and bool(torch.isfinite(out if torch.is_tensor(out) else out[0]).all())
            pair = [v if torch.is_tensor(v) else v[0] for v in outs.values()]
            same = same and torch.equal(*pair)
    names = attn_maps.layer_names(net, a.layers)
    res = {"tool": "attn_maps_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "recording_layers": len(names), "accumulators": {"%dx%d" % hw: n for hw, n in maps.counts().items()},
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite, "images_bit_identical": same}
    res["maps_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_maps"]["median"] / res["ms_per_iteration"]["cfg"]["median"], 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    res = {"tool": "attn_maps_bench kernel", "kernels": "mdm_attn_cross_maps / mdm_attn_cross_addv, bf16, B = 4, H = 8",
           "calls": a.calls, "warmup": a.warmup, "launches_per_event_pair": a.launches, "shapes": {}}
    for tag, (B, L, S, H, d) in KERNEL_SHAPES.items():
        g = torch.Generator().manual_seed(2)
        qkv = torch.randn(B, L, 3 * H * d, generator=g).to(dev, torch.bfloat16)
        kvc = torch.randn(B, S, 2 * H * d, generator=g).to(dev, torch.bfloat16)
        ld = (S + 3) // 4 * 4
        bias = (torch.randn(B, L, ld, generator=g) * 2).to(dev)
        acc = torch.zeros(B, L, ld, device=dev)
        legs = {"attn_cross_addv": lambda: ops.attn_cross_addv(qkv, kvc, None, H),
                "attn_cross_maps": lambda: ops.attn_cross_maps(qkv, kvc, None, H, acc),
                "attn_cross_maps_bias": lambda: ops.attn_cross_maps(qkv, kvc, None, H, acc, bias=bias)}
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
        moved = 2 * B * (L + S) * H * d + 8 * B * L * ld   # bytes by counting: q and k_c once, acc read and written
        res["shapes"][tag] = {"B_L_S_H_d": [B, L, S, H, d], "us_per_call": st, "finite": bool(torch.isfinite(acc).all()),
                              "bytes_by_counting": moved,
                              "cross_maps_over_cross_addv_median": round(st["attn_cross_maps"]["median"] / st["attn_cross_addv"]["median"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--layers", default="all")
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
