#!/usr/bin/env python
"""What LoRA adapters on the attention projections cost and save on UNet-64 (configs[1] architecture) at batch 64, bf16,
random weights.  Development / reporting tool, in the method of tools/sample_bench.py: the two legs of a comparison are
alternated call by call in ONE process, ``--warmup`` calls first, ``--calls`` timed, device events around every call,
median [p10-p90].
   python tools/lora_bench.py [--batch 64] [--rank 16] [--calls 20] [--warmup 3] [--out profiles/r10_lora.jsonl]

  leg 1  adapter overhead: forward + backward with the base frozen (but for conv_in's bias, so that backward is the whole
         input-gradient chain) without adapters, against the same with rank-r adapters on the default targets
  leg 2  step time: ``trainer.train_batch`` on its plain path with every weight trainable (AdamW over the model), against
         the LoRA step (frozen base, AdamW over the adapters only)
  leg 3  the three kernels alone at M = 16 384, C = 768, N in {768, 1536, 2304}: achieved GB/s over the bytes each must
         move (24 launches on rotating operands, larger together than the last-level cache, replayed as one hipGraph)
  --conv the same for adapters on the ResNet convolutions (``conv_targets``, rank ``--conv-rank``) INSTEAD of legs 1-3:
         forward + backward with the base frozen, without against with conv adapters, on UNet-64 at ``--batch`` and on
         nested-256 at ``--nested-batch`` with adapters on the OUTER net's ResNets only; then the three 3x3 kernels alone
         at the outer net's first level (256 x 256 x 64) and at UNet-64's (64 x 64 x 256)"""
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
from mdm_hip import configs, diffusion, lora, ops, samplers, trainer  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402

DEV = torch.device("cuda:0")


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


def _alternate(legs, a):
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.calls):
        for k, fn in legs.items():
            ms = _timed(fn)
            if it >= a.warmup:
                times[k].append(ms)
    return {k: _stats(ts) for k, ts in times.items()}


def _pipe(seed):
    torch.manual_seed(seed)
    net = mdm_hip.UNet(3, 3, configs.unet64_config(2048))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM")
    return diffusion.Diffusion(net, diffusion.DiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False)).to(DEV)


def _seeded_b(ad):
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in sorted(ad.named_parameters()):
            if name.endswith("lora_B"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))


def overhead_legs(a, base):
    pipe_f, pipe_l = _pipe(0), _pipe(0)
    for p in pipe_f.model.vision_model.parameters():
        p.requires_grad = False
    ad = lora.attach(pipe_l.model.vision_model, rank=a.rank)
    _seeded_b(ad)
    for pipe in (pipe_f, pipe_l):    # one cheap trainable tensor at the very start: backward walks the whole net in both legs
        pipe.model.vision_model.conv_in.bias.requires_grad = True
    g = torch.Generator().manual_seed(2)
    x = torch.randn(a.batch, 3, 64, 64, generator=g).to(DEV)
    t = torch.randint(0, 1000, (a.batch,), generator=g).to(DEV)
    cond, mask = torch.randn(a.batch, 32, 2048, generator=g).to(DEV), torch.ones(a.batch, 32).to(DEV)

    def run(vm):
        def go():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = vm(x, t, cond, mask)
            out.float().square().mean().backward()
        return go

    res = dict(base, leg="adapter overhead: forward + backward, frozen base", unit="ms per call",
               adapters=len(list(ad.parameters())) // 2, adapter_parameters=sum(p.numel() for p in ad.parameters()))
    res["ms"] = _alternate({"frozen_no_adapters": run(pipe_f.model.vision_model), "frozen_with_adapters": run(pipe_l.model.vision_model)}, a)
    res["adapters_minus_none_median_ms"] = round(res["ms"]["frozen_with_adapters"]["median"] - res["ms"]["frozen_no_adapters"]["median"], 4)
    return res


def step_legs(a, base):
    ops.set_grad_sink(None)
    pipe_t, pipe_l = _pipe(0), _pipe(0)
    opt_t = torch.optim.AdamW(pipe_t.model.vision_model.parameters(), lr=1e-5, weight_decay=0)
    opt_t._mdm_fused, opt_t._mdm_fused_reason = False, "forced: the plain path is the yardstick"
    ad = lora.attach(pipe_l.model.vision_model, rank=a.rank)
    _seeded_b(ad)
    opt_l = torch.optim.AdamW(ad.parameters(), lr=1e-5, weight_decay=0)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lambda it: 1.0) for o in (opt_t, opt_l)]
    args = types.SimpleNamespace(fp16=True, gradient_clip_norm=2.0)
    g = torch.Generator().manual_seed(3)
    sample = {"images": (torch.rand(a.batch, 3, 64, 64, generator=g) * 2 - 1).to(DEV),
              "lm_outputs": torch.randn(a.batch, 32, 2048, generator=g).to(DEV), "lm_mask": torch.ones(a.batch, 32).to(DEV)}
    losses = {"full": [], "lora": []}
    legs = {"plain_path_all_weights": lambda: losses["full"].append(trainer.train_batch(pipe_t, sample, opt_t, scheds[0], None, args)[0]),
            "plain_path_lora_adapters": lambda: losses["lora"].append(trainer.train_batch(pipe_l, sample, opt_l, scheds[1], None, args)[0])}
    res = dict(base, leg="step time: trainer.train_batch, plain path", unit="ms per step")
    res["ms"] = _alternate(legs, a)
    res["lora_path_reason"] = getattr(opt_l, "_mdm_fused_reason", None)
    res["finite"] = all(l == l and abs(l) != float("inf") for ls in losses.values() for l in ls)
    res["lora_over_full_median"] = round(res["ms"]["plain_path_lora_adapters"]["median"] / res["ms"]["plain_path_all_weights"]["median"], 4)
    return res


def kernel_legs(a, base):
    M, C, r, nbuf = 16384, 768, a.rank, 24
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(4)
    res = dict(base, leg="kernel rates", unit="GB/s over the bytes the kernel must move", M=M, C=C, r=r,
               rotating_buffers=nbuf, streaming_yardstick="concat_kernel 6.1 TB/s (profiles/)", kernels={})
    xs = [torch.randn(M, C, generator=g).to(bf).to(DEV) for _ in range(nbuf)]
    am = (torch.randn(r, C, generator=g) / C ** 0.5).to(bf).to(DEV)
    ts = [ops.lora_down(x, am) for x in xs]

    def rate(launch, nbytes):
        """``launch(k)`` on buffer set k: the nbuf launches are captured into ONE hipGraph (a kernel of a few microseconds is
        shorter than a host launch) and the replay is timed; per-kernel time = replay / nbuf"""
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
        return {"us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]], "bytes": nbytes,
                "GBps": round(nbytes / (st["median"] * 1e-3) / 1e9, 1)}

    res["kernels"]["lora_down C=%d" % C] = rate(lambda k: ops.lora_down(xs[k], am), M * C * 2 + M * r * 2 + r * C * 2)
    res["kernels"]["lora_wgrad C=%d (slabs + reduce)" % C] = rate(lambda k: ops.lora_wgrad(ts[k], xs[k], 1.0),
                                                                  M * C * 2 + M * r * 2 + r * C * 4)
    for N in (768, 1536, 2304):
        ys = xs if N == C else [torch.randn(M, N, generator=g).to(bf).to(DEV) for _ in range(nbuf)]
        bm = (torch.randn(N, r, generator=g) * 0.02).to(bf).to(DEV)
        res["kernels"]["lora_up_add N=%d" % N] = rate(lambda k, ys=ys, bm=bm: ops.lora_up_add(ys[k], ts[k], bm, 1e-3),
                                                      2 * M * N * 2 + M * r * 2 + N * r * 2)
        del ys
    return res


def conv_overhead_legs(a, base):
    out = []
    for model, batch, sides in (("unet64", a.batch, [64]), ("nested256 (adapters on the outer net only)", a.nested_batch, [256, 64])):
        nested = len(sides) > 1

        def build():
            torch.manual_seed(0)
            net = mdm_hip.NestedUNet(3, 3, configs.nested256_config(2048)) if nested else mdm_hip.UNet(3, 3, configs.unet64_config(2048))
            net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
            return net.to(DEV)

        net_f, net_l = build(), build()
        for p in net_f.parameters():
            p.requires_grad = False
        ad = lora.attach(net_l, targets=(), conv_targets=lora.CONV_TARGETS, conv_rank=a.conv_rank)
        _seeded_b(ad)
        active = 0
        for name, m in net_l.named_modules():
            if getattr(m, "_lora", None) is not None:
                if nested and name.startswith("inner_unet."):
                    m._lora = None            # the outer net's cost alone: the inner net runs as in the other leg
                else:
                    active += len(m._lora.pairs)
        for net in (net_f, net_l):           # one cheap trainable tensor at the very start: backward walks the whole net
            net.conv_in.bias.requires_grad = True
        g = torch.Generator().manual_seed(2)
        xs = [torch.randn(batch, 3, sd, sd, generator=g).to(DEV) for sd in sides]
        t = torch.randint(0, 1000, (batch,), generator=g).to(DEV)
        cond, mask = torch.randn(batch, 32, 2048, generator=g).to(DEV), torch.ones(batch, 32).to(DEV)

        def run(vm):
            def go():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    outs = vm(xs if nested else xs[0], t, cond, mask, {})
                sum(o.float().square().mean() for o in (outs if isinstance(outs, (list, tuple)) else [outs])).backward()
            return go

        res = dict(base, model=model, batch=batch, rank=a.conv_rank, leg="conv adapter overhead: forward + backward, frozen base",
                   unit="ms per call", adapters=active)
        res["ms"] = _alternate({"frozen_no_adapters": run(net_f), "frozen_with_conv_adapters": run(net_l)}, a)
        res["adapters_minus_none_median_ms"] = round(res["ms"]["frozen_with_conv_adapters"]["median"] - res["ms"]["frozen_no_adapters"]["median"], 4)
        out.append(res)
        del net_f, net_l, ad
        torch.cuda.empty_cache()
    return out


def conv_kernel_legs(a, base):
    bf, r, out = torch.bfloat16, a.conv_rank, []
    g = torch.Generator().manual_seed(4)
    for (N, H, W, C, nbuf) in ((4, 256, 256, 64, 16), (64, 64, 64, 256, 16)):
        M = N * H * W
        res = dict(base, leg="3x3 kernel rates", unit="GB/s over the bytes the kernel must move from / to HBM", N=N, H=H, W=W, C=C, r=r,
                   rank=r, rotating_buffers=nbuf, streaming_yardstick="concat_kernel 6.1 TB/s (profiles/)", kernels={})
        xs = [torch.randn(N, H, W, C, generator=g).to(bf).to(DEV) for _ in range(nbuf)]
        am = (torch.randn(r, 9, C, generator=g) / (9 * C) ** 0.5).to(bf).to(DEV)
        bm = (torch.randn(C, 9, r, generator=g) * 0.02).to(bf).to(DEV)
        ts = [ops.lora_down_conv3x3(x, am) for x in xs]

        def rate(launch, nbytes):
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
            return {"us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]], "bytes": nbytes,
                    "GBps": round(nbytes / (st["median"] * 1e-3) / 1e9, 1)}

        res["kernels"]["lora_down_conv3x3"] = rate(lambda k: ops.lora_down_conv3x3(xs[k], am), M * C * 2 + M * r * 2 + r * 9 * C * 2)
        res["kernels"]["lora_up_add_conv3x3 (overwrite: the backward's dX)"] = rate(
            lambda k: ops.lora_up_add_conv3x3(xs[k], ts[k], bm, 1e-3, accumulate=False), M * C * 2 + M * r * 2 + C * 9 * r * 2)
        res["kernels"]["lora_wgrad_conv3x3 (slabs + reduce)"] = rate(lambda k: ops.lora_wgrad_conv3x3(ts[k], xs[k], 1.0),
                                                                     M * C * 2 + M * r * 2 + r * 9 * C * 4)
        out.append(res)
        del xs, ts
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--conv", action="store_true", help="the conv-adapter legs instead of legs 1-3")
    ap.add_argument("--conv-rank", type=int, default=8)
    ap.add_argument("--nested-batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    base = {"model": "unet64", "batch": a.batch, "rank": a.rank, "calls": a.calls, "warmup": a.warmup,
            "setup": "bf16 autocast, random weights, legs alternated call by call in one process, device events"}

    def one(fn):
        return lambda a, base: [fn(a, base)]

    legs = [("conv", conv_overhead_legs), ("conv", conv_kernel_legs)] if a.conv else \
        [(leg, one(fn)) for leg, fn in (("1", overhead_legs), ("2", step_legs), ("3", kernel_legs)) if leg in a.legs.split(",")]
    for _, fn in legs:
        for res in fn(a, base):
            res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
            print(json.dumps(res), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(res) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
