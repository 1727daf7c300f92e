#!/usr/bin/env python
"""Graphed DDIM inversion (``GraphedSampler.invert``) against graphed DDIM(0) sampling, and the two inversion kernels' rates.
Development / reporting tool, in the method of tools/cfg_bench.py: the legs of a comparison are alternated call by call in
ONE process, device events around every call, ``--warmup`` calls first, ``--calls`` timed; median, min, max and p10-p90.
   python tools/invert_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/invert_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: guidance 7.5, bf16 autocast, random weights, S = 32 text tokens.  Legs: ``sample`` -- DDIM(eta = 0), ms per
iteration --, and ``invert`` with K = 1 and K = 3 iterations, ms per MODEL CALL (a call of n steps makes K n of them).  The
cases to record: unet64 at batch 4 and 64, nested1024 at batch 4.  No ratio is required: a replay of either graph is one
denoiser call plus one streaming kernel per scale (invert: and one gated copy of x_s, 12 bytes per element).
``kernel``: mdm_sampler_invert_step (16 bytes per element with an unconditional prediction) and mdm_sampler_noise_map (20)
beside mdm_sampler_step (DDPM posterior, noise given: 24) at [4, 3 * 1024^2] fp32, each leg one captured graph of
``--launches`` back-to-back calls per pair of events; GB/s counts the bytes of the definition.
Result lines go to ``--out`` (profiles/invert_sampling.jsonl)."""
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

KERNEL_SHAPE = (4, 3, 1024, 1024)
S_TEXT = 32
ITERATIONS = (1, 3)


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
    images = torch.tanh(torch.randn(batch, 3, side, side, generator=g)).to(dev)
    gs = GraphedSampler(pipe, seed=0)
    legs = {"sample": (lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5), n_it)}
    for K in ITERATIONS:
        legs["invert_K%d" % K] = (lambda K=K: gs.invert(images, smp, dev, iterations=K, num_inference_steps=n_it, guidance_scale=7.5)[0],
                                  K * n_it)
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, (fn, calls) in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(fn)
                if it >= a.warmup:
                    times[k].append(ms / calls)
                out = out if isinstance(out, (list, tuple)) else [out]
                finite = finite and all(bool(torch.isfinite(o).all()) for o in out)
    elements = sum(batch * 3 * (side // r) ** 2 for r in pipe.sampler._scale_info(pipe.get_model())[0])
    res = {"tool": "invert_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "setup": "graphed, guidance 7.5, bf16, random weights, S = %d; sample: DDIM(eta = 0)" % S_TEXT,
           "image_elements_all_scales": elements, "ms_per_model_call": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    base = res["ms_per_model_call"]["sample"]["median"]
    res["invert_minus_sample_ms_median"] = {k: round(v["median"] - base, 4) for k, v in res["ms_per_model_call"].items() if k != "sample"}
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    x, y, pc, pu, nz = (torch.randn(KERNEL_SHAPE, generator=g).to(dev) for _ in range(5))
    B = KERNEL_SHAPE[0]
    g_t, g_s = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.6, device=dev)
    pt = samplers.PredictionType.V_PREDICTION
    out = torch.empty_like(x)
    n = x.numel() * 4
    legs = {
        "sampler_invert_step": (lambda: ops.sampler_invert_step(x, pc, g_s, g_t, pt, pred_uncond=pu, guidance_scale=7.5, out=out), 4 * n),
        "sampler_noise_map": (lambda: ops.sampler_noise_map(x, y, pc, g_t, g_s, pt, clip="CLIP", pred_uncond=pu, guidance_scale=7.5), 5 * n),
        "sampler_step": (lambda: ops.sampler_step(x, pc, g_t, g_s, pt, need_noise=True, noise=nz, clip="CLIP", pred_uncond=pu,
                                                  guidance_scale=7.5), 6 * n),
    }
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
    return {"tool": "invert_bench kernel", "dtype": "fp32", "shape": list(KERNEL_SHAPE), "calls": a.calls, "warmup": a.warmup,
            "launches_per_graph": a.launches, "bytes_per_element": {k: legs[k][1] // x.numel() for k in legs}, "us_per_call": us,
            "gb_per_s_median": {k: round(legs[k][1] / us[k]["median"] * 1e-3, 1) for k in legs},
            "note": "the 50 MB tensors (200-300 MB per leg) stay in the 256 MB last-level cache in part: not a pure HBM rate"}


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
