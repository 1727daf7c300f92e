"""Shared by tests/test_lora_host.py (CPU) and tests/test_lora_gpu.py (GPU): fp64 restatements of the three adapter
formulas, the shape lists, and the oracle reference for a model with adapters.

The oracle knows nothing about adapters.  ``merged_state_dict`` replaces every adapted weight W by W + s (B @ A), reshaped to
W's shape; with A and B as CPU leaves that is a differentiable function of them, so ``unet_oracle.model_forward`` on the
merged state dict gives reference outputs AND reference dA / dB through torch autograd -- from code that shares nothing
with the product (no low-rank kernels, no in-place add, no separate adapter path at all)."""
import torch

import parity_cases as PC
import unet_oracle as O

TARGETS = ("qkv", "kv_cond", "proj_out")
# (M, C, r): T[M, r] = X[M, C] A^T
DOWN_SHAPES = [(16, 64, 4), (128, 256, 16), (200, 320, 8), (1030, 768, 64), (300, 3072, 16)]
# (M, N, r): Y[M, N] += s T[M, r] B^T
UP_SHAPES = [(16, 512, 4), (128, 768, 16), (200, 320, 8), (1030, 2304, 64)]
# (M, C, r): D[r, C] = s P[M, r]^T Q[M, C]; the last one spans several M-slabs
WGRAD_SHAPES = DOWN_SHAPES + UP_SHAPES + [(5000, 768, 16)]
# (Cout, Cin, r): W += s B A on fp32 masters
MERGE_SHAPES = [(512, 64, 4), (768, 256, 16), (2304, 768, 64)]
# (M, Cin, Cout, r)
AUTOGRAD_SHAPES = [(200, 320, 264, 8), (128, 256, 768, 16)]
TOL = {torch.float32: 2e-5, torch.bfloat16: 3e-2}   # the op gates of tests/test_ops_gpu.py


def relerr(a, b):
    """max-abs error relative to the largest reference magnitude (tests/test_ops_gpu.py)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def q(t, dtype):
    """round a CPU fp32 tensor through the compute dtype so both sides see the same inputs"""
    return t.to(dtype).float()


def down_ref(x, a):
    return x.double() @ a.double().t()


def up_add_ref(y, t, b, s):
    return y.double() + s * (t.double() @ b.double().t())


def wgrad_ref(p, q_, s):
    return s * (p.double().t() @ q_.double())


def expected_adapters(state_dict, targets, rank):
    """{adapter parameter name: shape} from the vision model's own state-dict keys: every ``<...attn.N>.<target>.weight``"""
    out = {}
    for k, v in state_dict.items():
        parts = k.split(".")
        if len(parts) >= 4 and parts[-1] == "weight" and parts[-2] in targets and parts[-4] == "attn":
            base = k[: -len(".weight")]
            out[base + ".lora_A"] = (rank, v.shape[1])
            out[base + ".lora_B"] = (v.shape[0], rank)
    return out


def seeded_b(ad, seed=77, sigma=0.05):
    """non-zero B values (B is zero after attach), drawn on the CPU in name order"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(ad.named_parameters()):
            if name.endswith("lora_B"):
                p.copy_((torch.randn(p.shape, generator=g) * sigma).to(p.device))


def adapter_values(ad):
    return {k: v.detach().float().cpu().clone() for k, v in ad.named_parameters()}


def merged_state_dict(sd, leaves, scale):
    """sd with every adapted ``<layer>.<target>.weight`` replaced by W + scale * (B @ A) (of the leaves' dtype)"""
    out = dict(sd)
    for k, a in leaves.items():
        if not k.endswith(".lora_A"):
            continue
        base = k[: -len(".lora_A")]
        b = leaves[base + ".lora_B"]
        w = sd[base + ".weight"]
        out[base + ".weight"] = w + scale * (b @ a).reshape(w.shape)
    return out


def oracle_lora_run(name, values, scale, dtype=torch.float32):
    """-> (outputs, {adapter name: gradient}) of the oracle on the merged state dict, loss = parity_cases.loss_of"""
    _, cfg, sd = PC.build_module(name)
    inp = PC.inputs(name)
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in values.items()}
    base = {k: v.to(dtype) for k, v in sd.items()}
    cast = lambda t: [u.to(dtype) for u in t] if isinstance(t, list) else t.to(dtype)
    outs = O.model_forward(merged_state_dict(base, leaves, scale), cfg, cast(inp["x"]), inp["times"], inp["cond"].to(dtype),
                           inp["mask"].to(dtype), inp["micros"])
    PC.loss_of(outs, inp["gys"]).backward()
    return [o.detach().float() for o in PC.as_list(outs)], {k: v.grad.detach().float() for k, v in leaves.items()}


def agg_err(grads, g_ref):
    num = sum(float((grads[k].detach().double().cpu() - g_ref[k].double()).pow(2).sum()) for k in g_ref)
    den = sum(float(g_ref[k].double().pow(2).sum()) for k in g_ref)
    return (num / den) ** 0.5
