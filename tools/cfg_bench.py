#!/usr/bin/env python
"""Projected and rescaled classifier-free guidance (``sample(..., cfg=CFG(...))``) against plain classifier-free guidance,
graphed, and its two kernels' rates.  Development / reporting tool, in the method of tools/freeu_bench.py: the legs of a
comparison are alternated call by call in ONE process, device events around every call, ``--warmup`` calls first,
``--calls`` timed; ms per iteration as median, min, max and p10-p90.
   python tools/cfg_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/cfg_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens: plain guidance
against ``CFG(eta=0, norm_threshold=0.1, momentum=-0.5, rescale=0.7)`` (the values do not change what is launched).  The
cases to record: unet64 at batch 4 and 64, nested1024 at batch 4.  No ratio is required: the result carries the measured
difference per iteration beside the byte-count estimate -- 36 bytes per image element with momentum (statistics: x_t, p_c,
p_u, run read, run written; combine: x_t, p_c, run read, out written), 28 without, plus the fp32 copies of the bf16
predictions that the plain path's step kernel also reads, over every scale.
``kernel``: mdm_cfg_stats and mdm_cfg_combine with momentum and rescale on, at the fp32 image shapes of those cases
([B, 3, 64, 64] for B = 4 and 64, [4, 3, 1024, 1024]) and at [1, 3, 1024, 1024], each leg as one captured graph of
``--launches`` back-to-back calls per pair of events; GB/s counts the bytes of the definition (statistics 20, combine 16 per
element).  The B = 4 UNet-64 tensors (0.2 MB each) stay in the caches across the repeated calls: a cache rate, not an HBM rate.
Result lines go to ``--out`` (profiles/cfg_sampling.jsonl)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import _lib, configs, diffusion, ops, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"unet64_batch4": (4, 3 * 64 * 64), "unet64_batch64": (64, 3 * 64 * 64), "nested1024_batch4": (4, 3 * 1024 * 1024),
                 "one_1024_image": (1, 3 * 1024 * 1024)}   # B, chw
S_TEXT = 32
OPTS = dict(eta=0.0, norm_threshold=0.1, momentum=-0.5, rescale=0.7)


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
    gs = GraphedSampler(pipe, seed=0)
    legs = {"plain": {}, "cfg": {"cfg": mdm_hip.CFG(**OPTS)}}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    elements = sum(batch * 3 * (side // r) ** 2 for r in pipe.sampler._scale_info(pipe.get_model())[0])
    res = {"tool": "cfg_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "cfg": repr(legs["cfg"]["cfg"]), "image_elements_all_scales": elements,
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    base, with_cfg = (res["ms_per_iteration"][k]["median"] for k in ("plain", "cfg"))
    res["cfg_minus_plain_ms_median"] = round(with_cfg - base, 4)
    res["cfg_over_plain_median"] = round(with_cfg / base, 4)
    res["estimate_36_bytes_per_element_mb"] = round(36 * elements / 1e6, 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel_shape(a, shape):
    dev = torch.device("cuda:0")
    B, chw = shape
    g = torch.Generator().manual_seed(2)
    x, pc, run = (torch.randn(B, chw, generator=g).to(dev) for _ in range(3))
    pu = pc + 0.3 * torch.randn(B, chw, generator=g).to(dev)
    gamma = torch.full((B,), 0.5, device=dev)
    out = torch.empty_like(pc)
    L, st = _lib.lib(), ops._stream
    wsb = ctypes.c_size_t(0)
    _lib.check(L.mdm_cfg_plan(B, chw, 1, ctypes.byref(wsb)), "mdm_cfg_plan")
    ws = torch.zeros(wsb.value // 4 + 4, device=dev)
    p = lambda t: t.data_ptr()
    stats = lambda: _lib.check(L.mdm_cfg_stats(p(x), p(pc), p(pu), p(gamma), p(run), p(run), None, None, OPTS["momentum"], 1, p(ws),
                                               wsb.value, B, chw, 2, st()), "mdm_cfg_stats")
    comb = lambda: _lib.check(L.mdm_cfg_combine(p(x), p(pc), p(pu), p(gamma), p(run), None, p(ws), wsb.value, p(out), 7.5, OPTS["eta"],
                                                OPTS["norm_threshold"], OPTS["rescale"], 1.0, B, chw, 2, st()), "mdm_cfg_combine")
    n = B * chw * 4
    legs = {"cfg_stats": (stats, 5 * n), "cfg_combine": (comb, 4 * n)}
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
    return {"B_chw": list(shape), "us_per_call": us,
            "gb_per_s_median": {k: round(legs[k][1] / us[k]["median"] * 1e-3, 1) for k in legs},
            "finite": bool(torch.isfinite(out).all())}


def kernel(a):
    return {"tool": "cfg_bench kernel", "dtype": "fp32", "options": OPTS, "calls": a.calls, "warmup": a.warmup,
            "launches_per_graph": a.launches, "shapes": {tag: kernel_shape(a, shape) for tag, shape in KERNEL_SHAPES.items()}}


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
