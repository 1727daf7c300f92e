#!/usr/bin/env python
"""What activation recomputation for the ResNet blocks (``mdm_hip.enable_activation_recompute``) costs in step time and
saves in memory, bf16, random weights.  Development / reporting tool, in the method of tools/lora_bench.py: the two legs
(switch off / on) are alternated call by call in ONE process on the same pipeline and optimizer, ``--warmup`` calls first,
``--calls`` timed, device events around every call, median [p10-p90].
   python tools/recompute_bench.py [--models unet64,nested256,nested1024] [--calls 10] [--warmup 2]
                                   [--out FILE]   (profiles/recompute_train.jsonl is a recorded run of it)

  per model (UNet-64 at batch 64, nested-256 at batch 16, nested-1024 at ``--batch-1024``, default 2):
      train step ms (``trainer.train_batch``, fused path), switch off against on, and ``torch.cuda.max_memory_allocated()``
      of one step of each (peak statistics reset before it)
  kernels  ``mdm_gn_reapply`` alone at three shipped shapes: achieved GB/s over the bytes it must move (one read of x, one
      write of y, the coefficients), launches on rotating operands larger together than the last-level cache, replayed as
      one hipGraph"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import configs, diffusion, ops, samplers, trainer  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

DEV = torch.device("cuda:0")
MODELS = {   # name: (config constructor, nested, image side)
    "unet64": ("unet64_config", False, 64),
    "nested256": ("nested256_config", True, 256),
    "nested1024": ("nested1024_config", True, 1024),
}
# (N, H, W, C): the small and the large end of the shipped shapes, and UNet-64's first level
KERNEL_SHAPES = [(64, 16, 16, 768), (64, 64, 64, 256), (4, 1024, 1024, 32)]


def _stats(ts):
    pct = lambda q: sorted(ts)[min(len(ts) - 1, int(round(q * (len(ts) - 1))))]
    return {"median": round(statistics.median(ts), 4), "p10_p90": [round(pct(0.1), 4), round(pct(0.9), 4)]}


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _pipe(name):
    ctor, nested, side = MODELS[name]
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                                loss_target_type="DDPM", threshold_function="CLIP")
    torch.manual_seed(0)
    if nested:
        sc.schedule_shifted, sc.rescale_signal = True, 1
        net = mdm_hip.NestedUNet(3, 3, getattr(configs, ctor)(2048))
        dcfg = diffusion.NestedDiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False, use_double_loss=True, no_use_residual=True)
        pipe = diffusion.NestedDiffusion(net, dcfg)
    else:
        net = mdm_hip.UNet(3, 3, getattr(configs, ctor)(2048))
        pipe = diffusion.Diffusion(net, diffusion.DiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=4321))
    return pipe.to(DEV), side


def step_legs(name, batch, a, base):
    ops.set_grad_sink(None)
    pipe, side = _pipe(name)
    vm = pipe.model.vision_model
    opt = torch.optim.AdamW(vm.parameters(), lr=5e-5, weight_decay=0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0)
    ema = trainer.ModelEma(vm)
    args = types.SimpleNamespace(fp16=True, gradient_clip_norm=2.0)
    g = torch.Generator().manual_seed(3)
    sample = {"images": (torch.rand(batch, 3, side, side, generator=g) * 2 - 1).to(DEV),
              "lm_outputs": torch.randn(batch, 32, 2048, generator=g).to(DEV), "lm_mask": torch.ones(batch, 32).to(DEV)}
    losses = {False: [], True: []}

    def leg(on):
        def go():
            ops.enable_activation_recompute(on)
            losses[on].append(float(trainer.train_batch(pipe, sample, opt, sched, None, args, ema_model=ema)[0]))
        return go

    legs = {"recompute_off": leg(False), "recompute_on": leg(True)}
    times = {k: [] for k in legs}
    peak = {}
    try:
        for it in range(a.warmup + a.calls):
            for k, fn in legs.items():
                if it == a.warmup:   # the first timed call of each leg also gives its peak (statistics reset before it)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                ms = _timed(fn)
                if it == a.warmup:
                    peak[k] = torch.cuda.max_memory_allocated()
                if it >= a.warmup:
                    times[k].append(ms)
    finally:
        ops.enable_activation_recompute(False)
        ops.set_grad_sink(None)
    res = dict(base, model=name, batch=batch, leg="train step: trainer.train_batch", unit="ms per step",
               path="fused" if getattr(opt, "_mdm_fused", None) not in (None, False) else "plain")
    res["ms"] = {k: _stats(ts) for k, ts in times.items()}
    res["max_memory_allocated_bytes"] = peak
    res["on_minus_off_median_ms"] = round(res["ms"]["recompute_on"]["median"] - res["ms"]["recompute_off"]["median"], 4)
    res["peak_saved_gb"] = round((peak["recompute_off"] - peak["recompute_on"]) / 2**30, 3)
    res["finite"] = all(l == l and abs(l) != float("inf") for ls in losses.values() for l in ls)
    return res


def kernel_legs(a, base):
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(4)
    res = dict(base, leg="kernel rates: mdm_gn_reapply (bf16, SiLU, no dropout)", unit="GB/s over the bytes the kernel must move",
               streaming_yardstick="concat_kernel 6.1 TB/s (profiles/)", kernels={})
    for (N, H, W, C) in KERNEL_SHAPES:
        nbytes = 2 * N * H * W * C * 2 + N * C * 2 * 4
        nbuf = max(4, min(24, int(600e6 // nbytes) + 1))   # together past the 256 MB last-level cache
        one = torch.randn(N, H, W, C, generator=g).to(bf)
        xs = [(one + 0.01 * k).to(DEV) for k in range(nbuf)]
        ys = [torch.empty_like(x) for x in xs]
        coef = (torch.randn(N, C, 2, generator=g)).to(DEV)
        L = mdm_hip._lib.lib()

        def launch(k):
            mdm_hip._lib.check(L.mdm_gn_reapply(xs[k].data_ptr(), coef.data_ptr(), ys[k].data_ptr(), N, H * W, C, 1, 0.0, 0, 0,
                                                ops.BF16, ops._stream()), "mdm_gn_reapply")

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch(0)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for k in range(nbuf):
                launch(k)
        t = []
        for it in range(a.warmup + a.calls):
            ms = _timed(graph.replay) / nbuf
            if it >= a.warmup:
                t.append(ms)
        st = _stats(t)
        res["kernels"]["N=%d %dx%dx%d" % (N, H, W, C)] = {
            "us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]], "bytes": nbytes,
            "rotating_buffers": nbuf, "GBps": round(nbytes / (st["median"] * 1e-3) / 1e9, 1)}
        del xs, ys, graph
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="unet64,nested256,nested1024")
    ap.add_argument("--batch-64", type=int, default=64)
    ap.add_argument("--batch-256", type=int, default=16)
    ap.add_argument("--batch-1024", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None, help="append the result lines to this file (default: stdout only)")
    a = ap.parse_args()
    base = {"calls": a.calls, "warmup": a.warmup,
            "setup": "bf16 autocast, random weights, switch off / on alternated call by call in one process, device events"}
    batches = {"unet64": a.batch_64, "nested256": a.batch_256, "nested1024": a.batch_1024}
    results = []
    for name in [m for m in a.models.split(",") if m]:
        results.append(step_legs(name, batches[name], a, base))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    if not a.no_kernels:
        results.append(kernel_legs(a, base))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for res in results:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
