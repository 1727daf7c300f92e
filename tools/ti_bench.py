#!/usr/bin/env python
"""What textual inversion costs on the text encoder and in the train step.  Development / reporting tool, in the method of
tools/lora_bench.py: the legs of a comparison are alternated call by call in ONE process, ``--warmup`` calls first,
``--calls`` timed, device events around every call, median [p10-p90].  Random weights, bf16.
   python tools/ti_bench.py [--rows 64] [--layers 24] [--calls 10] [--warmup 3] [--out profiles/ti_train.jsonl]

  leg 1  the encoder at flan-t5-xl geometry (``--layers`` of its 24 layers) on a caption batch of ``--rows`` rows x 10-40
         tokens: the ordinary forward (no_grad) against the differentiable forward + backward down to the learned rows
  leg 2  ``trainer.train_batch`` on its plain path, UNet-64 frozen, batch ``--batch``: the textual-inversion step (encoder
         forward + backward inside the step, AdamW over the learned rows) against the LoRA step (AdamW over rank-16
         adapters, lm_outputs given)"""
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
from mdm_hip import configs, diffusion, lora, ops, samplers, textual_inversion, trainer  # noqa: E402
from mdm_hip.testing import randomize_zero_params  # noqa: E402
from mdm_hip.text_encoder import T5Encoder, T5EncoderConfig  # noqa: E402

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


def _encoder(a, vocab=32128):
    torch.manual_seed(0)
    cfg = T5EncoderConfig(vocab_size=vocab, d_model=2048, d_kv=64, d_ff=5120, num_layers=a.layers, num_heads=32)
    return T5Encoder(cfg).to(DEV), cfg


def _captions(rows, S, vocab, tok, seed):
    """ids / mask as the reader hands them over (host arrays): 10-40 tokens per row, the placeholder once per row"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(10, 41, (rows,), generator=g)
    ids = torch.randint(1, vocab, (rows, S), generator=g)
    mask = torch.arange(S)[None, :] < lens[:, None]
    ids[torch.arange(rows), torch.randint(0, 10, (rows,), generator=g)] = tok
    return (ids * mask).numpy(), mask.numpy(), int(lens.sum())


def encoder_legs(a, base):
    enc, cfg = _encoder(a)
    tok = cfg.vocab_size
    ids, mask, T = _captions(a.rows, 40, cfg.vocab_size, tok, 1)
    ti = textual_inversion.attach(enc, [tok], init_ids=[1782])
    G = torch.randn(a.rows, 40, cfg.d_model, generator=torch.Generator().manual_seed(2)).to(DEV)

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            enc(ids, mask)

    def fwd_bwd():
        ti.embeddings.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = enc(ids, mask)
        (out * G).sum().backward()

    res = dict(base, leg="encoder: forward against forward + backward", unit="ms per call", rows=a.rows, tokens=T,
               layers=a.layers, geometry="flan-t5-xl (d_model 2048, 32 heads x 64, d_ff 5120)")
    res["ms"] = _alternate({"forward_no_grad": fwd, "forward_backward": fwd_bwd}, a)
    res["fwd_bwd_over_fwd_median"] = round(res["ms"]["forward_backward"]["median"] / res["ms"]["forward_no_grad"]["median"], 4)
    res["peak_memory_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    ti.detach()
    return res


def _pipe(seed):
    torch.manual_seed(seed)
    net = mdm_hip.UNet(3, 3, configs.unet64_config(2048))
    net.load_state_dict(randomize_zero_params(net.state_dict(), seed=1))
    sc = samplers.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM")
    return diffusion.Diffusion(net, diffusion.DiffusionConfig(sampler_config=sc, use_vdm_loss_weights=False)).to(DEV)


def step_legs(a, base):
    ops.set_grad_sink(None)
    enc, cfg = _encoder(a)
    tok = cfg.vocab_size
    ids, mask, T = _captions(a.batch, 32, cfg.vocab_size, tok, 3)
    ti = textual_inversion.attach(enc, [tok], init_ids=[1782])
    pipe_t, pipe_l = _pipe(0), _pipe(0)
    for p in pipe_t.model.vision_model.parameters():
        p.requires_grad = False
    ad = lora.attach(pipe_l.model.vision_model, rank=16)
    opt_t = torch.optim.AdamW(ti.parameters(), lr=1e-4, weight_decay=0)
    opt_l = torch.optim.AdamW(ad.parameters(), lr=1e-5, weight_decay=0)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lambda it: 1.0) for o in (opt_t, opt_l)]
    args = types.SimpleNamespace(fp16=True, gradient_clip_norm=2.0)
    g = torch.Generator().manual_seed(4)
    images = (torch.rand(a.batch, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    lm_mask = torch.from_numpy(mask).float().to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fixed = enc(ids, mask)
    losses = {"ti": [], "lora": []}

    def ti_step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cond = enc(ids, mask)
        sample = {"images": images, "lm_outputs": cond, "lm_mask": lm_mask}
        losses["ti"].append(trainer.train_batch(pipe_t, sample, opt_t, scheds[0], None, args)[0])

    def lora_step():
        sample = {"images": images, "lm_outputs": fixed, "lm_mask": lm_mask}
        losses["lora"].append(trainer.train_batch(pipe_l, sample, opt_l, scheds[1], None, args)[0])

    res = dict(base, leg="step time: trainer.train_batch, plain path, frozen UNet-64", unit="ms per step", batch=a.batch,
               tokens=T, layers=a.layers)
    res["ms"] = _alternate({"textual_inversion_step": ti_step, "lora_step": lora_step}, a)
    res["finite"] = all(l == l and abs(l) != float("inf") for ls in losses.values() for l in ls)
    res["ti_over_lora_median"] = round(res["ms"]["textual_inversion_step"]["median"] / res["ms"]["lora_step"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ti_train.jsonl"))
    a = ap.parse_args()
    from mdm_hip import _lib
    base = {"tool": "ti_bench", "device": torch.cuda.get_device_name(0), "lib": _lib.provenance()["sha256"], "dtype": "bf16"}
    lines = [encoder_legs(a, base)]
    torch.cuda.empty_cache()
    if not a.skip_step:
        lines.append(step_legs(a, base))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for l in lines:
            print(json.dumps(l), flush=True)
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
