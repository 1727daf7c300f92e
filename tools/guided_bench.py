#!/usr/bin/env python
"""Loss-guided sampling (``LossGuide``) against the eager path it sits beside, and the stem input-gradient kernel against
its read-once byte count.  Development / reporting tool, in the method of tools/sample_bench.py: the two legs of a comparison
are alternated call by call in ONE process, device events around every call, ``--warmup`` calls first, ``--calls`` timed;
ms per iteration as median, min, max and p10-p90.
   python tools/guided_bench.py sampling [unet64|nested1024] [batch] [steps] [--calls 10] [--warmup 2] [--out FILE]
   python tools/guided_bench.py kernel unet64 20 [--calls 20] [--warmup 3] [--out FILE]

``sampling``: eager unguided DDIM(eta = 0) vs the same with a masked-MSE guide (forward + the dgrad-only backward through the
denoiser + the guide's two elementwise kernels), bf16 autocast, random weights.  By counting alone the guided iteration
is about 2 x the unguided one.
``kernel``: mdm_conv3x3_stem_dgrad at the three shipped stem shapes (UNet-64 batch 64: 64 x 64 x 256; nested-256 batch 16:
256 x 256 x 64; nested-1024 batch 4: 1024 x 1024 x 32), bf16, achieved GB/s against the bytes of dy read once + dx written;
``batch`` launches per pair of events (positional, default 4: give 20) over dy buffers in rotation.  By counting the kernel is
VALU-limited (csrc/stem.hip): about half the streaming rate is what to expect.
Result lines go to ``--out`` (profiles/guided_sampling.jsonl)."""
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
from mdm_hip.testing import randomize_zero_params  # noqa: E402

STEM_SHAPES = {"unet64_b64": (64, 64, 64, 256, 3), "nested256_b16": (16, 256, 256, 64, 3), "nested1024_b4": (4, 1024, 1024, 32, 3)}


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
    smp = {"lm_outputs": torch.randn(batch, 32, 2048, generator=g).to(dev), "lm_mask": torch.ones(batch, 32).to(dev)}
    target = (torch.rand(batch, 3, side, side, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(batch, 1, side, side, device=dev)
    mask[..., : side // 2] = 1
    guide = mdm_hip.LossGuide(lambda x0: ((x0 - target) * mask).pow(2).sum(dim=(1, 2, 3)), scale=1.0)
    legs = {"unguided": {}, "guided_masked_mse": {"guide": guide}}
    times, finite = {k: [] for k in legs}, True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for it in range(a.warmup + a.calls):
            for k, kw in legs.items():
                torch.manual_seed(5)
                ms, out = _timed(lambda: pipe.sample(batch, smp, side, dev, resample_steps=True, num_inference_steps=n_it, ddim_eta=0, **kw))
                if it >= a.warmup:
                    times[k].append(ms / n_it)
                finite = finite and bool(torch.isfinite(out).all())
    res = {"tool": "guided_bench sampling", "model": which, "batch": batch, "steps_per_call": n_it, "calls": a.calls, "warmup": a.warmup,
           "sampler": "eager, DDIM(eta = 0), CFG off, bf16, random weights; guide: masked MSE on the left half",
           "ms_per_iteration": {k: _stats(ts) for k, ts in times.items()}, "finite": finite}
    res["guided_over_unguided_median"] = round(res["ms_per_iteration"]["guided_masked_mse"]["median"] / res["ms_per_iteration"]["unguided"]["median"], 3)
    res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def kernel(a):
    dev = torch.device("cuda:0")
    res = {"tool": "guided_bench kernel", "kernel": "mdm_conv3x3_stem_dgrad, bf16", "calls": a.calls, "warmup": a.warmup, "shapes": {}}
    for tag, (N, H, W, Cout, Cin) in STEM_SHAPES.items():
        g = torch.Generator().manual_seed(2)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dev)
        # dy buffers in rotation, at least four and at least 1 GB together: a launch finds none of its lines in the 256 MB
        # last-level cache.  One pair of events spans a.batch launches: launching from Python costs about as much as the
        # kernel runs, and inside a batch the launches queue up behind one another
        nbuf = max(4, -(-(1 << 30) // (N * H * W * Cout * 2)))
        dys = [torch.randn(N, H, W, Cout, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
        ts = []

        def batch(it):
            for k in range(a.batch):
                dx = ops.conv3x3_stem_dgrad(dys[(it * a.batch + k) % nbuf], w)
            return dx

        for it in range(a.warmup + a.calls):
            ms, dx = _timed(lambda: batch(it))
            if it >= a.warmup:
                ts.append(ms / a.batch)
        nbytes = dys[0].numel() * 2 + dx.numel() * 4
        st = _stats(ts)
        res["shapes"][tag] = {"N_H_W_Cout_Cin": [N, H, W, Cout, Cin], "read_once_mb": round(nbytes / 1e6, 1), "ms": st,
                              "launches_per_event_pair": a.batch, "rotating_buffers": nbuf,
                              "gb_per_s_median": round(nbytes / (st["median"] * 1e-3) / 1e9, 1), "finite": bool(torch.isfinite(dx).all())}
        del dys
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sampling", "kernel"])
    ap.add_argument("which", nargs="?", default="unet64", choices=["unet64", "nested1024"])
    ap.add_argument("batch", nargs="?", type=int, default=4)
    ap.add_argument("steps", nargs="?", type=int, default=4)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
