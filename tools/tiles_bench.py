#!/usr/bin/env python
"""Tiled (MultiDiffusion) sampling (``sample(..., tiles=Tiles(...))``) against untiled sampling on the same number of model
rows, graphed, and its two kernels' rates.  Development / reporting tool, in the method of tools/cfg_bench.py: the legs of a
comparison are alternated call by call in ONE process, device events around every call, ``--warmup`` calls first,
``--calls`` timed; ms per iteration as median, min, max and p10-p90.
   python tools/tiles_bench.py sampling [unet64|nested1024] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/tiles_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens.
  unet64      untiled at B = 4 images of 64 x 64 against ONE 64 x 160 canvas under Tiles(64, 32): T = 4 windows, so both legs
              put 2 x 4 rows of 64 x 64 through the denoiser and the difference is the two kernels (and the step on 64 x 160
              instead of 4 x 64 x 64 elements).
  nested1024  untiled at B = 2 images of 1024 x 1024 against ONE 1024 x 1536 canvas under Tiles(1024, 512): T = 2.
No ratio is required: the result carries the measured difference per iteration beside the byte count of the definition --
per scale, gather reads B T C h w and writes reps times that, merge reads reps B T C h w and writes reps B C H W, 4 bytes each.
``kernel``: mdm_tiles_gather (reps = 1) and mdm_tiles_merge (both blends) at a canvas [4, 3, 1024, 1536] under windows of
1024 x 1024 at stride 512 (T = 2), each leg as one captured graph of ``--launches`` back-to-back calls per pair of events;
GB/s counts the bytes of the definition.  Each kernel twice: on ONE buffer set (176 MB: it stays in the 256 MB last-level
cache across the calls, a cache-assisted rate) and, the ``_rotated`` legs, cycling through ``--sets`` buffer sets (4: 705
MB, so no call finds its data cached: the HBM rate).  Result lines go to ``--out`` (profiles/tiles_sampling.jsonl)."""
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

S_TEXT = 32
CASES = {"unet64": dict(side=64, canvas=(64, 160), window=64, stride=32), "nested1024": dict(side=1024, canvas=(1024, 1536),
                                                                                                window=1024, stride=512)}
KERNEL_CANVAS, KERNEL_WINDOW, KERNEL_STRIDE = (4, 3, 1024, 1536), (1024, 1024), (512, 512)


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
    which, n_it = a.which, a.steps
    case = CASES[which]
    dev = torch.device("cuda:0")
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                loss_target_type="DDPM", schedule_shifted=which != "unet64", rescale_signal=1 if which != "unet64" else None,
                                schedule_shifted_power=2 if which == "nested1024" else 1)
    torch.manual_seed(0)
    if which == "unet64":
        net = mdm_hip.UNet(3, 3, configs.unet64_config(2048))
        pipe = diffusion.Diffusion(net, diffusion.DiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False))
    else:
        net = mdm_hip.NestedUNet(3, 3, configs.nested1024_config(2048))
        pipe = diffusion.NestedDiffusion(net, diffusion.NestedDiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False,
                                                                              use_double_loss=True, no_use_residual=True))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
    pipe = pipe.to(dev)
    tiles = mdm_hip.Tiles(case["window"], case["stride"])
    T = tiles.count(*case["canvas"])

    def text(batch):
        g = torch.Generator().manual_seed(1)
        cond = torch.randn(batch, S_TEXT, 2048, generator=g)
        return {"lm_outputs": torch.cat([torch.zeros_like(cond), cond]).to(dev), "lm_mask": torch.ones(2 * batch, S_TEXT).to(dev)}

    gs = GraphedSampler(pipe, seed=0)
    legs = {"untiled": (T, text(T), case["side"], {}), "tiled": (1, text(1), case["canvas"], {"tiles": tiles})}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, (batch, smp, side, kw) in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    ratios = pipe.sampler._scale_info(pipe.get_model())[0]
    H, W = case["canvas"]
    reps = 2
    window_elements = sum(T * 3 * (case["window"] // r) ** 2 for r in ratios)
    canvas_elements = sum(3 * (H // r) * (W // r) for r in ratios)
    res = {"tool": "tiles_bench sampling", "model": which, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "untiled": "B = %d of %d x %d" % (T, case["side"], case["side"]), "tiled": "B = 1 of %d x %d, %r, T = %d" % (H, W, tiles, T),
           "model_rows_both_legs": reps * T, "output_shape": list(out.shape),
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    base, tiled = (res["ms_per_iteration"][k]["median"] for k in ("untiled", "tiled"))
    res["tiled_minus_untiled_ms_median"] = round(tiled - base, 4)
    res["tiled_over_untiled_median"] = round(tiled / base, 4)
    res["gather_bytes_mb"] = round(4 * window_elements * (1 + reps) / 1e6, 3)
    res["merge_bytes_mb"] = round(4 * reps * (window_elements + canvas_elements) / 1e6, 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    B, C, H, W = KERNEL_CANVAS
    g = torch.Generator().manual_seed(2)
    # one buffer set (176 MB) fits in the 256 MB last-level cache and stays there across back-to-back launches: those
    # legs measure a cache-assisted rate.  The "_rotated" legs cycle through ``--sets`` buffer sets (4: 705 MB), so that a
    # launch finds none of its data cached: the HBM rate.
    xs = [torch.randn(B, C, H, W, generator=g).to(dev) for _ in range(a.sets)]
    rowss = [ops.tiles_gather(x, KERNEL_WINDOW, KERNEL_STRIDE) for x in xs]
    outs = [torch.empty_like(x) for x in xs]
    x, rows, out = xs[0], rowss[0], outs[0]
    turn = {"n": 0}

    def rotated(fn):
        def call():
            i = turn["n"] % a.sets
            turn["n"] += 1
            fn(xs[i], rowss[i], outs[i])
        return call

    gather = lambda x, rows, out: ops.tiles_gather(x, KERNEL_WINDOW, KERNEL_STRIDE, out=rows)
    merge = lambda blend: (lambda x, rows, out: ops.tiles_merge(rows, H, W, KERNEL_WINDOW, KERNEL_STRIDE, blend, out=out))
    n_gather, n_merge = 8 * rows.numel(), 4 * (rows.numel() + out.numel())
    legs = {"tiles_gather": (lambda: gather(x, rows, out), n_gather),
            "tiles_merge_uniform": (lambda: merge("uniform")(x, rows, out), n_merge),
            "tiles_merge_ramp": (lambda: merge("ramp")(x, rows, out), n_merge),
            "tiles_gather_rotated": (rotated(gather), n_gather),
            "tiles_merge_uniform_rotated": (rotated(merge("uniform")), n_merge),
            "tiles_merge_ramp_rotated": (rotated(merge("ramp")), n_merge)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn, _ in legs.values():
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graphs = {}
    for k, (fn, _) in legs.items():
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(a.launches):
                fn()
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.calls):
        for k in legs:
            ms, _ = _timed(graphs[k].replay)
            if it >= a.warmup:
                times[k].append(1e3 * ms / a.launches)
    us = {k: _stats(ts) for k, ts in times.items()}
    return {"tool": "tiles_bench kernel", "dtype": "fp32", "canvas": list(KERNEL_CANVAS), "window": list(KERNEL_WINDOW),
            "stride": list(KERNEL_STRIDE), "windows": rows.shape[0] // B, "calls": a.calls, "warmup": a.warmup,
            "buffer_sets_rotated": a.sets, "bytes_per_buffer_set": 4 * (x.numel() + rows.numel()),
            "launches_per_graph": a.launches, "us_per_call": us, "bytes": {k: legs[k][1] for k in legs},
            "gb_per_s_median": {k: round(legs[k][1] / us[k]["median"] * 1e-3, 1) for k in legs},
            "finite": bool(torch.isfinite(out).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4, help="kernel: buffer sets the _rotated legs cycle through")
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
