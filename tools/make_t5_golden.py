"""Write tests/golden/t5_encoder.pt: what the REAL ``transformers.T5EncoderModel`` computes for the seeded cases of
tests/t5_cases.py.  Needs ``transformers``; runs on the build machine only (CPU).

Per case the fixture holds the ids and the mask, a strided channel subsample of the model's fp32 output on the valid
rows, the model's own error against the fp64 oracle in fp32 and under bf16 autocast (rel-L2 over ALL valid tokens of
the concatenated input draws -- the bf16 figure is the gate of the HIP encoder's bf16 mode), and a per-tensor checksum of
the weights, so that a generator mismatch fails as such.  Plus the model's bucket of every relative position in
[-511, 511].

    python tools/make_t5_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ml-mdm_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
sys.dont_write_bytecode = True

import t5_cases as TC  # noqa: E402


def hf_model(name):
    from transformers import T5Config, T5EncoderModel

    c = TC.config(name)
    hf = T5EncoderModel(T5Config(
        vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, num_layers=c.num_layers,
        num_heads=c.num_heads, relative_attention_num_buckets=c.relative_attention_num_buckets,
        relative_attention_max_distance=c.relative_attention_max_distance, layer_norm_epsilon=c.layer_norm_epsilon,
        feed_forward_proj=c.feed_forward_proj, dropout_rate=0.0, use_cache=False)).eval()
    missing, unexpected = hf.load_state_dict(TC.weights(name), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return hf


def main():
    from transformers.models.t5.modeling_t5 import T5Attention

    gold = {"cases": {}}
    rel = torch.arange(-511, 512)
    gold["bucket_rel"] = rel
    gold["bucket"] = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128)
    assert torch.equal(gold["bucket"], TC.bucket(rel))
    for name in TC.FIXTURE_CASES:
        hf = hf_model(name)
        ids, mask = TC.inputs(name)
        ref = TC.oracle_outputs(name)
        f32, b16 = [], []
        with torch.no_grad():
            for i in range(TC.DRAWS):
                f32.append(hf(input_ids=ids[i], attention_mask=mask).last_hidden_state * mask[..., None])
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    o = hf(input_ids=ids[i], attention_mask=mask).last_hidden_state
                b16.append(o.float() * mask[..., None])
        f32, b16 = torch.stack(f32), torch.stack(b16)
        v = lambda t: TC.valid_rows(t, mask)
        ent = {
            "ids": ids.to(torch.int16), "mask": mask.to(torch.uint8),
            "out_sub": TC.subsample(f32, name),
            "ref_fp32_error": TC.rel_l2(v(f32), v(ref)),
            "ref_bf16_error": TC.rel_l2(v(b16), v(ref)),
            "out_norm": float(v(ref).norm()),
            "param_sum": TC.checksums(TC.weights(name)),
        }
        gold["cases"][name] = ent
        print("%-10s fp32 vs fp64 oracle %.3e   bf16 autocast vs fp64 oracle %.3e   sub %s"
              % (name, ent["ref_fp32_error"], ent["ref_bf16_error"], tuple(ent["out_sub"].shape)), flush=True)
    os.makedirs(os.path.dirname(TC.GOLDEN), exist_ok=True)
    torch.save(gold, TC.GOLDEN)
    print("wrote %s (%d bytes)" % (TC.GOLDEN, os.path.getsize(TC.GOLDEN)))


if __name__ == "__main__":
    main()
