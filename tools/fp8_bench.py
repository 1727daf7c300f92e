#!/usr/bin/env python
"""What the opt-in MXFP8 path of the attention-layer 1x1 GEMMs and (``--conv``) of the ResNet convolutions (mdm_hip/fp8.py,
csrc/fp8.hip) costs and saves, bf16 autocast, random weights.  Development / reporting tool in the method of tools/sample_bench.py: the two legs of a comparison are
alternated call by call in ONE process, ``--warmup`` calls first, ``--calls`` timed, device events around every call,
median [p10-p90].
   python tools/fp8_bench.py [--models unet64:64,unet64:4,nested1024:4] [--steps 8] [--calls 10] [--warmup 2]
                             [--legs sampling,kernels,error] [--conv] [--out profiles/fp8_sampling.jsonl]

  sampling  graphed DDIM (eta = 0) ms per iteration: the plain bf16 model against a second copy of it with the fp8 handle
            attached (two GraphedSamplers, the same start noise and conditioning)
  kernels   at the shipped attention shapes (M = 16 384 pixels; K -> N in 768 -> 2304 / 768 / 3072 and 3072 -> 768): mx8_gemm
            against the bf16 1x1 convolution (conv_gemm_bl_kernel) on the same shapes, TFLOP/s over 2 M N K; mx8_quant in GB/s
            over the bytes it must move; the whole FFN (quantise + two GEMMs against ops.ffn).  8 launches on rotating
            operands replayed as one hipGraph
  error     rel-L2 between the bf16 and the fp8 model's outputs on the same inputs at a few timesteps
  --conv    adds to ``sampling`` and ``error`` a third copy of the model with the attention layers AND conv1 / conv2 / conv3
            of every ResNet in fp8 ("fp8+conv"; on a nested model a fourth, "fp8+conv>=128": the same with min_channels=128,
            the width study), and to ``kernels`` mx8_conv3x3 (+ its mx8_quant_zrow) against the bf16 3x3 convolution
            (conv_gemm_bl_kernel) at the shipped ResNet shapes, TFLOP/s over 2 M 9 Cin Cout
With random weights image quality is not judged."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-mdm_amd"))
import torch  # noqa: E402

import mdm_hip  # noqa: E402
from mdm_hip import configs, diffusion, fp8, ops, samplers  # noqa: E402
from mdm_hip.graph import GraphedSampler  # noqa: E402
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


def _sclk():
    """the shader clock right after a timed loop (one read-only rocm-smi sample), or None"""
    try:
        d = json.loads(subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout)
        card = d[sorted(d)[0]]
        return next((str(v) for k, v in card.items() if "sclk" in k.lower()), None)
    except Exception:   # noqa: BLE001
        return None


def _pipe(which):
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
    return pipe.to(DEV).eval(), side


def model_legs(which, batch, a, base, legs):
    out = []
    pipe_b, side = _pipe(which)
    pipe_f, _ = _pipe(which)
    handle = fp8.attach(pipe_f.model.vision_model)
    extra = {}   # --conv: leg name -> (pipe, handle)
    if a.conv:
        widths = (0, 128) if which != "unet64" else (0,)
        for mc in widths:
            p, _ = _pipe(which)
            extra["fp8+conv" if mc == 0 else "fp8+conv>=%d" % mc] = (
                p, fp8.attach(p.model.vision_model, conv_targets=fp8.CONV_TARGETS, min_channels=mc))
    g = torch.Generator().manual_seed(1)
    smp = {"lm_outputs": torch.randn(batch, 32, 2048, generator=g).to(DEV), "lm_mask": torch.ones(batch, 32).to(DEV)}
    vm_b, vm_f = pipe_b.model.vision_model, pipe_f.model.vision_model
    nested = hasattr(vm_b, "nest_ratio")
    sides = [side * s // vm_b.nest_ratio[0] for s in vm_b.nest_ratio + [1]] if nested else [side]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        if "error" in legs:
            res = dict(base, model=which, batch=batch, leg="rel-L2 between the bf16 and the fp8 model's outputs, same inputs",
                       fp8_layers=len(handle.layers), rel_l2={}, **{"rel_l2 " + k: {} for k in extra})
            for t in (50, 500, 950):
                xs = [torch.randn(batch, 3, sd, sd, generator=g).to(DEV) for sd in sides]
                tt = torch.full((batch,), t, dtype=torch.int64, device=DEV)
                args = (xs if nested else xs[0], tt, smp["lm_outputs"], smp["lm_mask"], {})
                ob, of = vm_b(*args), vm_f(*args)
                ob, of = (list(ob), list(of)) if isinstance(ob, (list, tuple)) else ([ob], [of])
                res["rel_l2"]["t=%d" % t] = [round(float((f.float() - b.float()).norm() / b.float().norm()), 5) for b, f in zip(ob, of)]
                for k, (p, _) in extra.items():
                    oc = p.model.vision_model(*args)
                    oc = list(oc) if isinstance(oc, (list, tuple)) else [oc]
                    res["rel_l2 " + k]["t=%d" % t] = [round(float((f.float() - b.float()).norm() / b.float().norm()), 5) for b, f in zip(ob, oc)]
            out.append(res)
        if "sampling" in legs:
            noise = [torch.randn(batch, 3, sd, sd, generator=g).to(DEV) for sd in sides]
            gb, gf = GraphedSampler(pipe_b, seed=7), GraphedSampler(pipe_f, seed=7)
            gx = {k: GraphedSampler(p, seed=7) for k, (p, _) in extra.items()}
            run = lambda gs: lambda: gs.sample(batch, smp, side, DEV, num_inference_steps=a.steps, start_noise=noise, ddim_eta=0)
            res = dict(base, model=which, batch=batch, steps_per_call=a.steps, leg="graphed DDIM, bf16 against fp8", unit="ms per call",
                       fp8_layers=len(handle.layers))
            for k, (_, hx) in extra.items():
                res["fp8_convs " + k] = len(hx.convs)
            res["ms"] = _alternate(dict({"bf16": run(gb), "fp8": run(gf)}, **{k: run(gs) for k, gs in gx.items()}), a)
            res["sclk_after"] = _sclk()
            res["ms_per_iteration"] = {k: round(v["median"] / a.steps, 4) for k, v in res["ms"].items()}
            res["fp8_over_bf16_median"] = round(res["ms"]["fp8"]["median"] / res["ms"]["bf16"]["median"], 4)
            for k in gx:
                res[k + "_over_bf16_median"] = round(res["ms"][k]["median"] / res["ms"]["bf16"]["median"], 4)
            ib, i_f = run(gb)(), run(gf)()
            res["finite"] = bool(torch.isfinite(ib).all() and torch.isfinite(i_f).all())
            ib = ib.clone()      # a GraphedSampler returns its static output buffer
            res["images_rel_l2_fp8_vs_bf16"] = round(float((i_f.float() - ib.float()).norm() / ib.float().norm()), 5)
            for k, gs in gx.items():
                res["images_rel_l2_%s_vs_bf16" % k] = round(float((run(gs)().float() - ib.float()).norm() / ib.float().norm()), 5)
            out.append(res)
    return out


def kernel_legs(a, base):
    M, nbuf, bf = 16384, 8, torch.bfloat16
    g = torch.Generator().manual_seed(4)
    res = dict(base, leg="kernel rates", M=M, rotating_buffers=nbuf, unit="TFLOP/s over 2 M N K (GEMMs), GB/s over the bytes moved (quantiser)",
               kernels={})

    def rate(launch):
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
        return _stats(t)

    def gemm_entry(st, N, K):
        return {"us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]],
                "TFLOPs": round(2.0 * M * N * K / (st["median"] * 1e-3) / 1e12, 1)}

    with torch.no_grad():
        for K, N, what in ((768, 2304, "qkv"), (768, 768, "proj_out + residual"), (768, 3072, "FFN up, GELU"), (3072, 768, "FFN down + residual")):
            xs = [torch.randn(M, 1, 1, K, generator=g).to(bf).to(DEV) for _ in range(nbuf)]
            w = torch.nn.Parameter((torch.randn(N, K, 1, 1, generator=g) / K ** 0.5).to(DEV))
            b = torch.nn.Parameter(torch.randn(N, generator=g).to(DEV) * 0.1)
            r = torch.randn(M, 1, 1, N, generator=g).to(bf).to(DEV) if "residual" in what else None
            gelu = "GELU" in what
            wq, bq = ops.packed_weight_mx8(w, b)
            aq = [ops.mx8_quant(x) for x in xs]
            tag = "%d -> %d (%s)" % (K, N, what)
            if gelu:   # the bf16 FFN-up launch is the first half of ops.ffn: timed below as part of the whole FFN
                res["kernels"]["mx8_gemm " + tag + ", MXFP8 out"] = gemm_entry(rate(lambda k: ops.mx8_gemm(aq[k], wq, bq, gelu=True, emit=True)), N, K)
                res["kernels"]["mx8_gemm " + tag + ", bf16 out"] = gemm_entry(rate(lambda k: ops.mx8_gemm(aq[k], wq, bq, gelu=True)), N, K)
            else:
                res["kernels"]["mx8_gemm " + tag] = gemm_entry(rate(lambda k: ops.mx8_gemm(aq[k], wq, bq, residual=r)), N, K)
            if not gelu:
                res["kernels"]["conv_gemm_bl bf16 " + tag] = gemm_entry(rate(lambda k: ops.conv(xs[k], w, b, residual=r)), N, K)
            st = rate(lambda k: ops.mx8_quant(xs[k], out=aq[k]))
            nbytes = M * K * 2 + M * K + M * K // 32
            res["kernels"]["mx8_quant bf16 [M, %d] (%s input)" % (K, what)] = {
                "us": round(st["median"] * 1e3, 2), "bytes": nbytes, "GBps": round(nbytes / (st["median"] * 1e-3) / 1e9, 1)}
            del xs, aq
        # the whole FFN, 768 -> 3072 -> 768: quantise + emit GEMM + GEMM against ops.ffn (two bf16 GEMMs)
        C, Hd = 768, 3072
        xs = [torch.randn(M, 1, 1, C, generator=g).to(bf).to(DEV) for _ in range(nbuf)]
        rs = torch.randn(M, 1, 1, C, generator=g).to(bf).to(DEV)
        w1 = torch.nn.Parameter((torch.randn(Hd, C, 1, 1, generator=g) / C ** 0.5).to(DEV))
        b1 = torch.nn.Parameter(torch.zeros(Hd, device=DEV))
        w2 = torch.nn.Parameter((torch.randn(C, Hd, 1, 1, generator=g) / Hd ** 0.5).to(DEV))
        b2 = torch.nn.Parameter(torch.zeros(C, device=DEV))
        q1, q2 = ops.packed_weight_mx8(w1, b1), ops.packed_weight_mx8(w2, b2)

        def ffn8(k):
            h = ops.mx8_gemm(ops.mx8_quant(xs[k].reshape(M, C)), q1[0], q1[1], gelu=True, emit=True)
            return ops.mx8_gemm(h, q2[0], q2[1], residual=rs)

        flops = 4.0 * M * C * Hd
        for name, fn in (("FFN 768 -> 3072 -> 768, fp8 (quantise + 2 GEMMs)", ffn8),
                         ("FFN 768 -> 3072 -> 768, bf16 (ops.ffn)", lambda k: ops.ffn(xs[k], w1, b1, w2, b2, rs))):
            st = rate(fn)
            res["kernels"][name] = {"us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]],
                                    "TFLOPs": round(flops / (st["median"] * 1e-3) / 1e12, 1)}
    res["sclk_after"] = _sclk()
    return [res]


# the shipped ResNet 3x3 shapes (N, H, W, Cin, Cout): UNet-64 B=64 at its three levels and a skip-concat input, then the
# nets of nested-1024 B=4 from the 1024 x 1024 outer net inwards
CONV_SHAPES = [(64, 64, 64, 256, 256), (64, 32, 32, 512, 512), (64, 16, 16, 768, 768), (64, 16, 16, 1536, 768),
               (4, 1024, 1024, 32, 32), (4, 512, 512, 64, 64), (4, 256, 256, 128, 128), (4, 128, 128, 256, 256)]


def conv_kernel_legs(a, base):
    nbuf, bf = 4, torch.bfloat16
    g = torch.Generator().manual_seed(5)
    res = dict(base, leg="3x3 kernel rates", rotating_buffers=nbuf, unit="TFLOP/s over 2 M 9 Cin Cout; the quantiser in us", kernels={})

    def rate(launch):
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
        return _stats(t)

    with torch.no_grad():
        for N, H, W, cin, cout in CONV_SHAPES:
            flops = 2.0 * N * H * W * 9 * cin * cout
            one = torch.randn(N, H, W, cin, generator=g).to(bf).to(DEV)
            xs = [one] + [one.roll(k, 0).contiguous() for k in range(1, nbuf)]
            w = torch.nn.Parameter((torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV))
            b = torch.nn.Parameter(torch.randn(cout, generator=g).to(DEV) * 0.1)
            wq, bq = ops.packed_weight_mx8_3x3(w, b)
            aq = [ops.mx8_quant_zrow(x) for x in xs]
            entry = {}
            for name, fn in (("mx8_conv3x3", lambda k: ops.mx8_conv3x3(aq[k], wq, (N, H, W), bq)),
                             ("mx8_quant_zrow + mx8_conv3x3", lambda k: ops.mx8_conv3x3(ops.mx8_quant_zrow(xs[k]), wq, (N, H, W), bq)),
                             ("conv_gemm_bl bf16", lambda k: ops.conv(xs[k], w, b))):
                st = rate(fn)
                entry[name] = {"us": round(st["median"] * 1e3, 2), "us_p10_p90": [round(v * 1e3, 2) for v in st["p10_p90"]],
                               "TFLOPs": round(flops / (st["median"] * 1e-3) / 1e12, 1)}
            res["kernels"]["%d x %d x %d, %d -> %d" % (N, H, W, cin, cout)] = entry
            del xs, aq, one
            torch.cuda.empty_cache()
    res["sclk_after"] = _sclk()
    return [res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="unet64:64,unet64:4,nested1024:4")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="sampling,kernels,error")
    ap.add_argument("--conv", action="store_true", help="also the ResNet convolutions in fp8 (see above)")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    legs = a.legs.split(",")
    base = {"calls": a.calls, "warmup": a.warmup,
            "setup": "bf16 autocast, random weights, legs alternated call by call in one process, device events"}
    results = []

    def emit(rs):
        for res in rs:
            res["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
            print(json.dumps(res), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(res) + "\n")
            results.append(res)
        torch.cuda.empty_cache()

    if "kernels" in legs:
        emit(kernel_legs(a, base))
        if a.conv:
            emit(conv_kernel_legs(a, base))
    if "sampling" in legs or "error" in legs:
        for spec in a.models.split(","):
            which, batch = spec.split(":")
            emit(model_legs(which, int(batch), a, base, legs))


if __name__ == "__main__":
    main()
