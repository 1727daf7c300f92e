#!/usr/bin/env python
"""Prompt-to-prompt attention control (``sample(..., control=ctl)``) against classifier-free guidance alone, graphed, and the
rates of the two preparation kernels.  Development / reporting tool, in the method of tools/region_bench.py: the two legs of a
comparison are alternated call by call in ONE process, device events around every call, ``--warmup`` calls first, ``--calls``
timed; ms per iteration as median, min, max and p10-p90.
   python tools/attn_control_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/attn_control_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens, one source and
``batch - 1`` edits of it (28 tokens aligned one to one, tokens 28-31 new and kept, token 5 at weight 1.5): CFG alone against
CFG + control on all layers with the default intervals.  The cases to record: unet64 and nested1024 at batch 4.  No ratio is
required: the feature is opt-in, and its expected cost is the edited rows' attention as four launches per layer instead of
one plus the two preparation kernels.
``kernel``: mdm_ctrl_mix_kv and mdm_ctrl_gather_qkv at the shipped attention shapes (L 64, d 96) and (L 256, d 64), H = 8,
S = 32, R = 3 edited rows of a batch of 8, bf16, gate on, ``--launches`` launches per pair of events; GB/s over the bytes
each kernel must move (mix: two [S, 2C] rows read and two written per edited row, + M; gather: 4C read and 4C written per
query of an edited row).
Result lines go to ``--out`` (profiles/attn_control_sampling.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import configs, diffusion, ops, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"L64_d96": (8, 64, 32, 8, 96), "L256_d64": (8, 256, 32, 8, 64)}   # N, L, S, H, d
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


def one_source(batch):
    """row 0 the source, rows 1 .. batch - 1 its edits: 28 aligned tokens, four new ones kept, one reweighted"""
    scale = torch.ones(S_TEXT)
    scale[5] = 1.5
    edits = range(1, batch)
    return mdm_hip.AttnControl.aligned(S_TEXT, [0] * batch, {r: [(j, j) for j in range(28)] for r in edits},
                                       scale={r: scale for r in edits})


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
    ctl = one_source(batch)
    gs = GraphedSampler(pipe, seed=0)
    legs = {"cfg": {}, "cfg_control": {"control": ctl}}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    cross, self_ = ctl.layer_sets(net)
    res = {"tool": "attn_control_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls,
           "warmup": a.warmup, "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "control": "1 source + %d edits, 28 aligned tokens, 4 kept, 1 reweighted; intervals %s / %s; self_max_queries %d"
                      % (batch - 1, ctl.cross_interval, ctl.self_interval, ctl.self_max_queries),
           "cross_layers": len(cross), "self_layers": len(self_), "graphs": len(gs._graphs),
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    res["control_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_control"]["median"] / res["ms_per_iteration"]["cfg"]["median"], 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    res = {"tool": "attn_control_bench kernel", "kernels": "mdm_ctrl_mix_kv / mdm_ctrl_gather_qkv, bf16, S = 32, H = 8, R = 3 of N = 8",
           "calls": a.calls, "warmup": a.warmup, "launches_per_event_pair": a.launches, "shapes": {}}
    for tag, (N, L, S, H, d) in KERNEL_SHAPES.items():
        g = torch.Generator().manual_seed(2)
        C, R = H * d, 3
        qkv = torch.randn(N, L, 3 * C, generator=g).to(dev, torch.bfloat16)
        kvc = torch.randn(N, S, 2 * C, generator=g).to(dev, torch.bfloat16)
        ctl = one_source(R + 1)
        h = ctl.rows_for(guidance=True, device=dev)
        legs = {"ctrl_mix_kv": lambda: ops.ctrl_mix_kv(kvc, h.own, h.src, h.M, h.D, None, h.gate_c),
                "ctrl_gather_qkv": lambda: ops.ctrl_gather_qkv(qkv, h.own, h.src, h.gate_s)}
        nbytes = {"ctrl_mix_kv": R * (4 * S * 2 * C * 2 + S * h.ld * 4), "ctrl_gather_qkv": R * L * 8 * C * 2}
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
        res["shapes"][tag] = {"N_L_S_H_d": [N, L, S, H, d], "R": R, "us_per_call": st, "bytes": nbytes,
                              "gb_per_s_median": {k: round(nbytes[k] / (st[k]["median"] * 1e-6) / 1e9, 1) for k in legs},
                              "mix_kv_gflops_median": round(2.0 * R * S * S * C / (st["ctrl_mix_kv"]["median"] * 1e-6) / 1e9, 1),
                              "note": "per call: the launch and the op's two torch.empty included, so a latency at these sizes"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=10)
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
