#!/usr/bin/env python
"""FreeU (``sample(..., freeu=cfg)``) against classifier-free guidance alone, graphed, and its two kernels against the plain
concat.  Development / reporting tool, in the method of tools/region_bench.py: the legs of a comparison are alternated call
by call in ONE process, device events around every call, ``--warmup`` calls first, ``--calls`` timed; ms per iteration as
median, min, max and p10-p90.
   python tools/freeu_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/freeu_bench.py kernel [--calls 20] [--warmup 3] [--launches 20] [--out FILE]

``sampling``: GraphedSampler DDIM(eta = 0), guidance 7.5, bf16 autocast, random weights, S = 32 text tokens: CFG alone against
CFG + FreeU v1 and CFG + FreeU v2 at the two deepest up blocks (``levels="deepest2"``, b = (1.2, 1.4), s = (0.9, 0.2): the
values do not change what is launched).  The cases to record: unet64 at batch 4 and 64, nested1024 at batch 4.  No ratio is
required: by byte counting the extra cost is one more read of the backbone (v2) and of the skip at two levels.
``kernel``: mdm_freeu_stats (v1: reads r; v2: reads r and h) and mdm_freeu_apply against mdm_concat at the shipped 16 x 16
concat shape of the UNet-64 (N = 8: [uncond | cond] of a batch-4 sampling call, C1 = C2 = 768, bf16) and at N = 128 (batch
64), each leg as one captured graph of ``--launches`` back-to-back calls per pair of events (a call from Python costs more
than these kernels run); GB/s counts the bytes of the definition (stats: the tensors read; apply and concat: the output
written and as many bytes read).  The tensors of the N = 8 shape (6 MB) stay in the caches across the repeated calls: its
figures are cache rates, not HBM rates.
Result lines go to ``--out`` (profiles/freeu_sampling.jsonl)."""
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
from mdm_hip import _lib, configs, diffusion, freeu, ops, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

KERNEL_SHAPES = {"batch4": (8, 16, 16, 768, 768), "batch64": (128, 16, 16, 768, 768)}   # N, H, W, C1, C2
S_TEXT = 32
B_S = dict(b=(1.2, 1.4), s=(0.9, 0.2))


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
    legs = {"cfg": {}, "cfg_freeu_v1": {"freeu": mdm_hip.FreeU(**B_S)}, "cfg_freeu_v2": {"freeu": mdm_hip.FreeU(structure=True, **B_S)}}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: gs.sample(batch, smp, side, dev, num_inference_steps=n_it, ddim_eta=0, guidance_scale=7.5, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    sel = freeu.select(net, legs["cfg_freeu_v1"]["freeu"])
    res = {"tool": "freeu_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "graphed, DDIM(eta = 0), guidance 7.5, bf16, random weights, S = %d" % S_TEXT,
           "freeu": "deepest2, b = %s, s = %s" % (B_S["b"], B_S["s"]),
           "blocks": {n: m.num_residual_blocks for n, m, _, _ in sel},
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    base = res["ms_per_iteration"]["cfg"]["median"]
    res["v1_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_freeu_v1"]["median"] / base, 4)
    res["v2_over_cfg_median"] = round(res["ms_per_iteration"]["cfg_freeu_v2"]["median"] / base, 4)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel_shape(a, shape):
    dev = torch.device("cuda:0")
    N, H, W, C1, C2 = shape
    g = torch.Generator().manual_seed(2)
    h = torch.randn(N, H, W, C1, generator=g).to(dev, torch.bfloat16)
    r = torch.randn(N, H, W, C2, generator=g).to(dev, torch.bfloat16)
    out = torch.empty(N, H, W, C1 + C2, device=dev, dtype=torch.bfloat16)
    L, st = _lib.lib(), ops._stream
    wsb = ctypes.c_size_t(0)
    _lib.check(L.mdm_freeu_plan(N, H, W, C1, C2, ops.BF16, 1, ctypes.byref(wsb)), "mdm_freeu_plan")
    ws = torch.zeros(wsb.value // 4 + 4, device=dev)
    p = lambda t: t.data_ptr()
    stats = lambda v2: _lib.check(L.mdm_freeu_stats(p(h), p(r), p(ws), wsb.value, N, H, W, C1, C2, v2, ops.BF16, st()), "mdm_freeu_stats")
    apply = lambda v2: _lib.check(L.mdm_freeu_apply(p(h), p(r), p(ws), wsb.value, p(out), N, H, W, C1, C2, 1.2, 0.2, v2, ops.BF16, st()),
                                  "mdm_freeu_apply")
    legs = {"concat": (lambda: _lib.check(L.mdm_concat(p(h), p(r), p(out), N * H * W, C1, C2, 0, ops.BF16, st()), "mdm_concat"),
                       2 * out.numel() * 2),
            "freeu_stats_v1": (lambda: stats(0), r.numel() * 2),
            "freeu_stats_v2": (lambda: stats(1), (r.numel() + h.numel()) * 2),
            "freeu_apply_v1": (lambda: apply(0), 2 * out.numel() * 2),
            "freeu_apply_v2": (lambda: apply(1), 2 * out.numel() * 2)}
    stats(1)   # the workspace the apply legs read
    # each leg as ONE captured graph of --launches back-to-back calls: a call from Python costs more than these kernels run
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
    return {"N_H_W_C1_C2": list(shape), "us_per_call": us,
            "gb_per_s_median": {k: round(legs[k][1] / us[k]["median"] * 1e-3, 1) for k in legs},
            "finite": bool(torch.isfinite(out.float()).all())}


def kernel(a):
    return {"tool": "freeu_bench kernel", "dtype": "bf16", "calls": a.calls, "warmup": a.warmup,
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
