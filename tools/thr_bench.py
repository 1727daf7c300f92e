#!/usr/bin/env python
"""The dynamic-threshold quantile as a radix select (``ops.abs_quantile`` -> mdm_abs_quantile) against ``torch.quantile``.
Development / reporting tool, in the method of tools/cfg_bench.py: the legs of a comparison are alternated call by call in
ONE process, device events around every call, ``--warmup`` calls first, ``--calls`` timed; median, min, max and p10-p90.
   python tools/thr_bench.py threshold [--calls 20] [--warmup 3] [--launches 10] [--out FILE]
   python tools/thr_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]

``threshold``: from x0 s (fp32 [B, n], normal, standard deviation 0.6) to thr, DeepFloyd's function (ratio 0.95, clamp to
[1, 1.5]): ``torch.quantile(|x|, 0.95, dim=1).clamp(1, 1.5)`` against ``ops.abs_quantile(x, 0.95, 1, 1.5)``, each leg as
``--launches`` back-to-back eager calls per pair of events, at [64, 3 64^2], [4, 3 256^2], [4, 3 1024^2] and [1, 3 2048 3072];
at the last one torch's leg records its error instead of a time.  Then the library's launches alone, as captured graphs of
``--launches`` calls (no host time): the whole call, and the three passes of the select one by one
(mdm_dev_abs_quantile_stage) as GB/s counted on x read once per pass.  torch's leg is NOT captured: a graph of ten
``torch.quantile`` calls at [4, 3 1024^2] faulted when it was replayed (a memory aperture violation in the sort's
onesweep kernel), so its sort runs only eagerly here.  The small shapes stay in the caches across the repeated calls: a cache
rate, not an HBM rate.
``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens, threshold function
DYNAMIC_IF: the sampler as it is against the same sampler with ``ops.abs_quantile`` swapped for the ``torch.quantile``
restatement below while its graph is captured; ms per iteration, and what each captured graph holds in device memory.  The cases
to record: unet64 at batch 4 and 64, nested1024 at batch 4.  Where a scale has rows above 2^20 values (nested1024) the torch leg
is left out and the result says so: that is the captured sort that faulted.
Result lines go to ``--out`` (profiles/thr_sampling.jsonl)."""
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

SHAPES = {"unet64_batch64": (64, 3 * 64 * 64), "nested256_top_batch4": (4, 3 * 256 * 256),
          "nested1024_top_batch4": (4, 3 * 1024 * 1024), "canvas_2048x3072": (1, 3 * 2048 * 3072)}   # B, n
Q, CMIN, CMAX = 0.95, 1.0, 1.5
S_TEXT = 32
TORCH_GRAPH_ROW_LIMIT = 1 << 20   # rows above this: torch's leg is not captured (see the docstring)


def torch_threshold(x, q, cmin=None, cmax=None, return_stats=False):
    """what the samplers did before: abs, segmented sort, gather, lerp, clamp"""
    return torch.quantile(x.reshape(x.shape[0], -1).abs(), q, dim=1).clamp(min=cmin, max=cmax)


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


def _graph_of(fn, launches):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            out = fn()
    return g, out


def threshold_shape(a, shape):
    dev = torch.device("cuda:0")
    B, n = shape
    x = (torch.randn(B, n, generator=torch.Generator().manual_seed(2)) * 0.6).to(dev)
    res = {"B_n": list(shape)}
    outs = {}

    def eager(fn, tag):   # --launches back-to-back calls on the current stream
        def run():
            for _ in range(a.launches):
                outs[tag] = fn()
        return run

    legs = {}
    try:
        torch_threshold(x, Q, CMIN, CMAX)
        legs["torch_quantile"] = eager(lambda: torch_threshold(x, Q, CMIN, CMAX), "torch_quantile")
    except RuntimeError as e:
        res["torch_quantile_error"] = str(e).splitlines()[0]
    legs["abs_quantile"] = eager(lambda: ops.abs_quantile(x, Q, CMIN, CMAX), "abs_quantile")
    torch.cuda.synchronize()
    # the library's launches alone, captured: the five of a call, and the passes one by one, each on the workspace the
    # launches before it left
    graphs = {"abs_quantile_graphed": _graph_of(lambda: ops.abs_quantile(x, Q, CMIN, CMAX), a.launches)[0]}
    L, wsb = _lib.lib(), ctypes.c_size_t(0)
    _lib.check(L.mdm_abs_quantile_plan(B, n, ctypes.byref(wsb)), "mdm_abs_quantile_plan")
    stage = lambda ws, k: _lib.check(L.mdm_dev_abs_quantile_stage(x.data_ptr(), ws.data_ptr(), wsb.value, B, n, Q, k, ops._stream()),
                                     "mdm_dev_abs_quantile_stage")
    keep = []
    for lvl in (1, 2, 3):
        ws = torch.empty(wsb.value // 4, dtype=torch.int32, device=dev)
        keep.append(ws)
        for k in range(lvl):
            stage(ws, k)
        graphs["level%d" % lvl] = _graph_of(lambda ws=ws, lvl=lvl: stage(ws, lvl), a.launches)[0]
    legs.update({k: g.replay for k, g in graphs.items()})
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.calls):
        for k in legs:
            ms, _ = _timed(legs[k])
            if it >= a.warmup:
                times[k].append(1e3 * ms / a.launches)
    res["us_per_call"] = {k: _stats(ts) for k, ts in times.items()}
    res["gb_per_s_median_x_read_once"] = {k: round(B * n * 4 / res["us_per_call"][k]["median"] * 1e-3, 1)
                                          for k in ("level1", "level2", "level3")}
    if "torch_quantile" in outs:
        res["torch_over_abs_quantile_median"] = round(res["us_per_call"]["torch_quantile"]["median"]
                                                      / res["us_per_call"]["abs_quantile"]["median"], 2)
        res["thr_bits_differ"] = int((outs["torch_quantile"].view(torch.int32) != outs["abs_quantile"].view(torch.int32)).sum())
    res["thr"] = [round(float(v), 6) for v in outs["abs_quantile"][:4]]
    return res


def threshold(a):
    return {"tool": "thr_bench threshold", "dtype": "fp32", "q": Q, "clamp": [CMIN, CMAX], "calls": a.calls, "warmup": a.warmup,
            "launches_per_graph": a.launches, "shapes": {tag: threshold_shape(a, shape) for tag, shape in SHAPES.items()}}


class _swapped:
    """``ops.abs_quantile`` replaced by the torch restatement while a leg runs (the capture of its graph included)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.keep = ops.abs_quantile
        if self.on:
            ops.abs_quantile = torch_threshold

    def __exit__(self, *exc):
        ops.abs_quantile = self.keep


def sampling(a):
    which, batch, n_it = a.which, a.batch, a.steps
    dev = torch.device("cuda:0")
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                loss_target_type="DDPM", threshold_function="DYNAMIC_IF", schedule_shifted=which != "unet64",
                                rescale_signal=1 if which != "unet64" else None,
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
    legs = {"abs_quantile": False, "torch_quantile": True}
    if 3 * side * side > TORCH_GRAPH_ROW_LIMIT:
        del legs["torch_quantile"]
    gss = {k: GraphedSampler(pipe, seed=0) for k in legs}
    times, finite, mem, outs = {k: [] for k in legs}, True, {}, {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        # one eager step first: the packed weights are made here, not inside the first leg's memory figures
        pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=1, ddim_eta=0, guidance_scale=7.5)
        for it in range(a.warmup + a.calls):
            for k, swap in legs.items():
                torch.manual_seed(5)
                if it == 0:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                with _swapped(swap):
                    ms, out = _timed(lambda: gss[k].sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0,
                                                           guidance_scale=7.5))
                if it == 0:   # the call that captured: what the graph keeps, and the peak on the way
                    mem[k] = {"graph_holds_mb": round((torch.cuda.memory_allocated() - before) / 2**20, 1),
                              "peak_over_start_mb": round((torch.cuda.max_memory_allocated() - before) / 2**20, 1)}
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
                outs[k] = out
    res = {"tool": "thr_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), DYNAMIC_IF, guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite, "capture_memory": mem}
    if "torch_quantile" not in legs:
        res["torch_quantile"] = "not run: rows of %d values; the captured torch.quantile faulted on replay at this size" % (3 * side * side)
        return res
    new, old = (res["ms_per_iteration"][k]["median"] for k in ("abs_quantile", "torch_quantile"))
    res["torch_minus_abs_quantile_ms_median"] = round(old - new, 4)
    res["graph_memory_torch_minus_abs_quantile_mb"] = round(mem["torch_quantile"]["graph_holds_mb"] - mem["abs_quantile"]["graph_holds_mb"], 1)
    res["images_max_abs_difference"] = float((outs["abs_quantile"].float() - outs["torch_quantile"].float()).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["threshold", "sampling"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the result line to this file")
    a = ap.parse_args()
    if a.calls is None:
        a.calls = 20 if a.what == "threshold" else 10
    if a.warmup is None:
        a.warmup = 3 if a.what == "threshold" else 2
    res = threshold(a) if a.what == "threshold" else sampling(a)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
