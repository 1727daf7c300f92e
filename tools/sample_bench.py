#!/usr/bin/env python
"""Sampling latency of the three shipped architectures, eager sampler vs GraphedSampler (one hipGraph replay per whole
denoise iteration).  Development / reporting tool:
   python tools/sample_bench.py [unet64|nested256|nested1024] [batch] [steps]

With ``--solver dpmpp_2m``: the few-step solver against the first-order path it sits beside.  Two graphed legs, DDIM(eta = 0)
and DPM-Solver++(2M), alternated call by call in ONE process (device events around every ``GraphedSampler.sample`` call of
``steps`` iterations, ``--warmup`` calls first, ``--calls`` timed): ms per iteration as median, min, max and p10-p90.  Then
the wall time of one ``--few``-step (25) 2M ``sample()`` next to one ``--many``-step (250) ancestral DDPM ``sample()``.
   python tools/sample_bench.py nested1024 4 8 --solver dpmpp_2m [--calls 20] [--warmup 3] [--out FILE]
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/sample_bench.py unet64 4 8 --solver dpmpp_2m --calls 3 --many 0
With ``--solver sa [--tau 1]``: the same two-leg measurement with graphed DPM-Solver++(2M) and graphed SA-Solver
(``SASolver(3, 3, tau)``: one launch per scale that reads three fp32 images more than 2M's) as the legs; the result line is
appended to profiles/sa_sampling.jsonl unless ``--out`` names another file.
   python tools/sample_bench.py nested256 4 8 --solver sa [--tau 1] [--calls 20] [--warmup 3] [--many 0]

With ``--known``: known-region sampling against the path it sits beside.  Two graphed legs of ancestral DDPM, without known
images (the captured graph of before: no launch more) and with a half-image mask (one ``mdm_sampler_known_blend`` launch per
scale and iteration more), alternated call by call in ONE process, timed like the solver legs.  ``--free-only`` times the
first leg alone through keywords that older revisions of the package know too: the same figure from another checkout.
   python tools/sample_bench.py nested1024 4 8 --known [--calls 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import configs, diffusion, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402


def solver_legs(pipe, smp, batch, side, dev, n_it, a):
    """graphed DDIM(0) and graphed ``a.solver`` -- for ``sa``: graphed 2M and graphed SA-Solver --, alternated; then
    few-step solver vs many-step DDPM wall time"""
    gs = GraphedSampler(pipe, seed=7)
    if a.solver == "sa":
        base, legs = "dpmpp_2m", {"dpmpp_2m": dict(solver="dpmpp_2m"), "sa": dict(solver=samplers.SASolver(3, 3, tau=a.tau))}
    else:
        base, legs = "ddim_eta0", {"ddim_eta0": dict(ddim_eta=0), a.solver: dict(solver=a.solver)}

    def timed(**kw):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = gs.sample(batch, smp, side, dev, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    times, finite = {k: [] for k in legs}, True
    for it in range(a.warmup + a.calls):
        for k, kw in legs.items():
            ms, out = timed(num_inference_steps=n_it, **kw)
            if it >= a.warmup:
                times[k].append(ms / n_it)
            finite = finite and bool(torch.isfinite(out).all())
    pct = lambda ts, q: sorted(ts)[min(len(ts) - 1, int(round(q * (len(ts) - 1))))]
    res = {"ms_per_iteration": {k: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
                                    "p10_p90": [round(pct(ts, 0.1), 4), round(pct(ts, 0.9), 4)]} for k, ts in times.items()}}
    lo, hi = res["ms_per_iteration"][base]["p10_p90"]
    if a.solver == "sa":
        res["tau"] = a.tau
        res["sa_minus_2m_median_ms"] = round(res["ms_per_iteration"]["sa"]["median"] - res["ms_per_iteration"][base]["median"], 4)
        res["sa_median_inside_2m_p10_p90"] = bool(lo <= res["ms_per_iteration"]["sa"]["median"] <= hi)
    else:
        res["solver_median_inside_ddim_p10_p90"] = bool(lo <= res["ms_per_iteration"][a.solver]["median"] <= hi)
    if a.many > 0:
        wall = {}
        for tag, kw in (("%s_%d_steps" % (a.solver, a.few), dict(legs[a.solver], num_inference_steps=a.few)),
                        ("ddpm_%d_steps" % a.many, dict(num_inference_steps=a.many))):
            timed(**kw)   # builds and warms the graph of this step count
            ms, out = timed(**kw)
            wall[tag] = round(ms, 2)
            finite = finite and bool(torch.isfinite(out).all())
        res["sample_wall_ms"] = wall
    res["finite"] = finite
    return res


def _stats(ts):
    pct = lambda q: sorted(ts)[min(len(ts) - 1, int(round(q * (len(ts) - 1))))]
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "p10_p90": [round(pct(0.1), 4), round(pct(0.9), 4)]}


def known_legs(pipe, smp, batch, side, dev, n_it, a):
    """graphed DDPM without known images and with the left half of the image known, alternated"""
    gs = GraphedSampler(pipe, seed=7)
    g = torch.Generator().manual_seed(3)
    known = (torch.rand(batch, 3, side, side, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(batch, 1, side, side, device=dev)
    mask[..., : side // 2] = 1
    legs = {"free": {}}
    if not a.free_only:
        legs["known_half"] = dict(known_images=known, known_mask=mask)
    times, finite = {k: [] for k in legs}, True
    for it in range(a.warmup + a.calls):
        for k, kw in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = gs.sample(batch, smp, side, dev, num_inference_steps=n_it, **kw)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1) / n_it)
            finite = finite and bool(torch.isfinite(out).all())
    res = {"ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    if not a.free_only:
        res["known_minus_free_median_ms"] = round(res["ms_per_iteration"]["known_half"]["median"] - res["ms_per_iteration"]["free"]["median"], 4)
        res["known_half_is_kept"] = bool((out[..., : side // 2] - known[..., : side // 2]).abs().max() < 1e-5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="?", default="nested1024", choices=["unet64", "nested256", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=8)
    ap.add_argument("--solver", default=None, choices=list(samplers.SOLVERS))
    ap.add_argument("--tau", type=float, default=0.0, help="with --solver sa: the noise level of SASolver(3, 3, tau)")
    ap.add_argument("--known", action="store_true", help="graphed DDPM with and without a half-image mask, alternated")
    ap.add_argument("--free-only", action="store_true", help="with --known: the leg without known images alone")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--few", type=int, default=25)
    ap.add_argument("--many", type=int, default=250, help="0: skip the wall-time comparison")
    ap.add_argument("--out", default=None, help="append the result line to this file")
    a = ap.parse_args()
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
        cfg = configs.nested256_config(2048) if which == "nested256" else configs.nested1024_config(2048)
        net, side = mdm_hip.NestedUNet(3, 3, cfg), 256 if which == "nested256" else 1024
        pipe = diffusion.NestedDiffusion(net, diffusion.NestedDiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False,
                                                                              use_double_loss=True, no_use_residual=True))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
    pipe = pipe.to(dev)
    g = torch.Generator().manual_seed(1)
    smp = {"lm_outputs": torch.randn(batch, 32, 2048, generator=g).to(dev), "lm_mask": torch.ones(batch, 32).to(dev)}
    if a.known:
        res = {"model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
               "sampler": "GraphedSampler, ancestral DDPM, CFG off, bf16, random weights"}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            res.update(known_legs(pipe, smp, batch, side, dev, n_it, a))
        res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
        emit(res, a.out)
        return
    if a.solver is not None:
        res = {"model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
               "sampler": "GraphedSampler, CFG off, bf16, random weights"}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            res.update(solver_legs(pipe, smp, batch, side, dev, n_it, a))
        res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
        emit(res, a.out or (os.path.join(ROOT, "profiles", "sa_sampling.jsonl") if a.solver == "sa" else None))
        return
    res = {"model": which, "batch": batch, "timed_steps": n_it, "sampler": "DDPM (ddim_eta=None), CFG off, bf16"}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pipe.sampler.use_device_rng(7, dev)
        pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=n_it)
        torch.cuda.synchronize()
        res["eager_ms_per_step"] = round((time.perf_counter() - t0) / n_it * 1e3, 3)
        gs = GraphedSampler(pipe, seed=7)
        gs.sample(batch, smp, side, dev, num_inference_steps=n_it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out2 = gs.sample(batch, smp, side, dev, num_inference_steps=n_it)
        torch.cuda.synchronize()
        res["graphed_ms_per_step"] = round((time.perf_counter() - t0) / n_it * 1e3, 3)
    res["finite"] = bool(torch.isfinite(out).all() and torch.isfinite(out2).all())
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    emit(res, a.out)


def emit(res, out):
    print(json.dumps(res), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
