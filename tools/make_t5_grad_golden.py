"""Write tests/golden/t5_grad.pt: how well the REAL ``transformers.T5EncoderModel`` differentiates the seeded cases of
tests/t5_cases.py, against torch autograd through the fp64 oracle.  Needs ``transformers``; runs on the build machine only
(CPU).

Loss = sum(out * G) with the seeded cotangent G of ti_cases.cotangents per input draw; the gradient is taken with respect
to the embedding table.  Per gradient case the fixture holds the reference's own error (rel-L2 against the fp64 oracle) in
fp32 and under CPU bf16 autocast, pooled over the input draws and per draw, the largest per-draw / pooled ratio of each (the
spread between draws: the margin the reference needs against itself), and a channel-subsampled fp64 dx0 of draw 0, so that
the host test can check that the oracle still produces it.

    python tools/make_t5_grad_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ml-mdm_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
sys.dont_write_bytecode = True

import t5_cases as TC  # noqa: E402
import ti_cases as TI  # noqa: E402
from make_t5_golden import hf_model  # noqa: E402


def hf_table_grad(hf, ids, mask, G, autocast):
    hf.shared.weight.requires_grad_(True)
    hf.shared.weight.grad = None
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    (out.float() * mask[..., None] * G).sum().backward()
    return hf.shared.weight.grad.detach().clone()


def main():
    gold = {"cases": {}}
    for name in TI.GRAD_CASES:
        hf = hf_model(name)
        for p in hf.parameters():
            p.requires_grad_(False)
        ids, mask = TC.inputs(name)
        G = TI.cotangents(name)
        ref = TI.oracle_table_grads(name)
        f32 = torch.stack([hf_table_grad(hf, ids[i], mask, G[i], False) for i in range(TC.DRAWS)])
        b16 = torch.stack([hf_table_grad(hf, ids[i], mask, G[i], True) for i in range(TC.DRAWS)])
        ent = {"grad_norm": float(ref.norm()), "param_sum": TC.checksums(TC.weights(name))}
        for key, t in (("fp32", f32), ("bf16", b16)):
            per = [TC.rel_l2(t[i], ref[i]) for i in range(TC.DRAWS)]
            ent["ref_%s_error" % key] = TC.rel_l2(t, ref)
            ent["ref_%s_error_per_draw" % key] = per
            ent["ref_%s_spread" % key] = max(per) / ent["ref_%s_error" % key]
        cfg, sd = TC.config(name), TC.weights(name)
        ent["dx0_sub"] = TI.subsample_dx0(TI.oracle_dx0(sd, cfg, ids[0], mask, G[0]), name)
        gold["cases"][name] = ent
        print("%-14s fp32 %.3e (spread %.3f)   bf16 autocast %.3e (spread %.3f)   dx0 sub %s"
              % (name, ent["ref_fp32_error"], ent["ref_fp32_spread"], ent["ref_bf16_error"], ent["ref_bf16_spread"],
                 tuple(ent["dx0_sub"].shape)), flush=True)
    os.makedirs(os.path.dirname(TI.GOLDEN), exist_ok=True)
    torch.save(gold, TI.GOLDEN)
    print("wrote %s (%d bytes)" % (TI.GOLDEN, os.path.getsize(TI.GOLDEN)))


if __name__ == "__main__":
    main()
