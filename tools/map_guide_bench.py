#!/usr/bin/env python
"""Attention-map guidance (``sample(..., map_guide=MapGuide(AttendExcite(...), ...))``) against classifier-free guidance alone,
eager, and the backward kernel against the forward kernel it differentiates.  Development / reporting tool, in the method of
tools/attn_maps_bench.py: the two legs of a comparison are alternated call by call in ONE process, device events around every
call, ``--warmup`` calls first, ``--calls`` timed; ms per iteration as median, min, max and p10-p90.
   python tools/map_guide_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 6] [--warmup 2] [--out FILE]
   python tools/map_guide_bench.py kernel [--calls 6] [--warmup 2] [--launches 20] [--out FILE]

``sampling``: the EAGER sampler (the graphed one refuses ``map_guide=``), DDIM(eta = 0), guidance 7.5, bf16 autocast, random
weights, S = 32 text tokens: CFG alone against CFG + ``map_guide`` on ``--layers`` (default "all") in EVERY step
(``interval=None``), one iteration per step, AttendExcite on two tokens at the finest attention resolution.  No ratio is
required (the feature is opt-in): by counting, a guided step adds one forward + one input-gradient backward over the B
conditional rows to the step's forward over 2 B rows.
``kernel``: mdm_attn_cross_maps_bwd against mdm_attn_cross_maps on the same tensors at the shipped shapes (L 256, d 64) and
(L 64, d 96), S = 32, B = 4 and H = 8 (the conditional block of a batch-4 sampling call), bf16, ``--launches`` launches per
pair of events; and with S = 77 (two key tiles: the two-sweep path).
Result lines go to ``--out`` (profiles/map_guide_sampling.jsonl)."""
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
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"L256_d64": (4, 256, 32, 8, 64), "L64_d96": (4, 64, 32, 8, 96),
                 "L256_d64_S77": (4, 256, 77, 8, 64), "L64_d96_S77": (4, 64, 77, 8, 96)}   # B, L, S, H, d
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


class _Resolutions:
    """a recorder that only notes the attention resolutions it is called at"""

    def __init__(self):
        self.seen = set()

    def record(self, qkv, kvc, mask, heads, bias, N, h, w):
        self.seen.add((h, w))


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
    # the finest attention resolution with text keys: one recording forward
    probe = _Resolutions()
    vm = getattr(pipe.get_model(), "vision_model", pipe.get_model())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), attn_maps.applied(vm, probe, a.layers):
        pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=1, ddim_eta=0, guidance_scale=7.5)
    res_hw = max(probe.seen)
    guide = mdm_hip.MapGuide(mdm_hip.AttendExcite([1, 2], resolution=res_hw), a.scale, layers=a.layers, interval=None)
    legs = {"cfg": {}, "cfg_map_guide": {"map_guide": guide}}
    times, finite = {k: [] for k in legs}, True
    outs = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=n_it, ddim_eta=0,
                                                     guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                outs[k] = out if torch.is_tensor(out) else out[0]
                finite = finite and bool(torch.isfinite(outs[k]).all())
    names = attn_maps.layer_names(vm, a.layers)
    moved = float((outs["cfg_map_guide"].float() - outs["cfg"].float()).norm() / outs["cfg"].float().norm())
    res = {"tool": "map_guide_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "eager, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "map_guide": "AttendExcite([1, 2]) at %dx%d, scale %g, every step, 1 iteration" % (res_hw + (a.scale,)),
           "recording_layers": len(names), "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite,
           "guide_moved_the_image_rel_l2": round(moved, 4)}
    res["map_guide_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_map_guide"]["median"] / res["ms_per_iteration"]["cfg"]["median"], 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    res = {"tool": "map_guide_bench kernel", "kernels": "mdm_attn_cross_maps_bwd / mdm_attn_cross_maps, bf16, B = 4, H = 8",
           "calls": a.calls, "warmup": a.warmup, "launches_per_event_pair": a.launches, "shapes": {}}
    for tag, (B, L, S, H, d) in KERNEL_SHAPES.items():
        g = torch.Generator().manual_seed(2)
        qkv = torch.randn(B, L, 3 * H * d, generator=g).to(dev, torch.bfloat16)
        kvc = torch.randn(B, S, 2 * H * d, generator=g).to(dev, torch.bfloat16)
        ld = (S + 3) // 4 * 4
        dacc = torch.randn(B, L, ld, generator=g).to(dev)
        acc = torch.zeros(B, L, ld, device=dev)
        dqkv = torch.zeros_like(qkv)
        legs = {"attn_cross_maps": lambda: ops.attn_cross_maps(qkv, kvc, None, H, acc),
                "attn_cross_maps_bwd": lambda: ops.attn_cross_maps_bwd(qkv, kvc, None, H, dacc, dqkv)}
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
        moved = 2 * B * (L + S) * H * d + 4 * B * L * ld + 2 * B * L * H * d   # q and k_c once, dacc read, dq written (bf16)
        flops = (2 * (1 if S <= 64 else 2) + 2) * B * H * L * S * d
        res["shapes"][tag] = {"B_L_S_H_d": [B, L, S, H, d], "us_per_call": st, "finite": bool(torch.isfinite(dqkv.float()).all()),
                              "bytes_by_counting": moved, "flops_by_counting": flops,
                              "bwd_over_fwd_median": round(st["attn_cross_maps_bwd"]["median"] / st["attn_cross_maps"]["median"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--layers", default="all")
    ap.add_argument("--scale", type=float, default=20.0)
    ap.add_argument("--calls", type=int, default=6)
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
