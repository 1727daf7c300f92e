"""Shared by tests/test_lora_conv_host.py (CPU) and tests/test_lora_conv_gpu.py (GPU): the shape list of the 3x3 adapter
kernels, their references through ``torch.nn.functional.conv2d`` / ``conv_transpose2d`` / autograd in fp64 on the CPU, the
adapter names a model must get, and the oracle reference for a model with attention AND conv adapters.

As in tests/lora_cases.py the oracle knows nothing about adapters: every adapted weight W is replaced by
W + s (B @ A.view(r, -1)).view_as(W) with A, B as CPU leaves -- a 4-D ``A`` [r, Cin, 3, 3] is flattened for the product, and
the conv adapters use their own scale -- and ``unet_oracle.model_forward`` on that state dict gives outputs and dA / dB."""
import torch
import torch.nn.functional as F

import lora_cases as LC
import parity_cases as PC
import unet_oracle as O

CONV_TARGETS = ("conv1", "conv2", "conv3")
# (N, H, W, C, r) for all three kernels (C is Cout for the up-add):
#   (1, 1, 1, 64, 4)      only the centre tap is inside
#   (1, 4, 4, 8, 4)       every pixel touches a border; one 16-byte chunk of C; smallest rank
#   (2, 5, 7, 40, 8)      H != W, odd sides, 70 rows (row-tile tail), C no multiple of 32 (k-step tail), two images: a shift
#                         across the image boundary must read zeros
#   (1, 3, 40, 32, 8)     one 32-row tile spans several image rows
#   (3, 16, 16, 256, 16)  the mini models' level
#   (2, 8, 8, 320, 64)    largest rank, K = 2880
SHAPES = [(1, 1, 1, 64, 4), (1, 4, 4, 8, 4), (2, 5, 7, 40, 8), (1, 3, 40, 32, 8), (3, 16, 16, 256, 16), (2, 8, 8, 320, 64)]
# the weight gradient only: M = 5120 rows span several slabs
WGRAD_SHAPES = SHAPES + [(5, 32, 32, 64, 16)]
# (N, H, W, Cin, Cout, r) of the autograd op
AUTOGRAD_SHAPES = [(2, 5, 7, 40, 24, 8), (2, 16, 16, 32, 256, 16)]
# (Cout, Cin, r): W [Cout, Cin, 3, 3] += s B A on fp32 masters
MERGE_SHAPES = [(64, 32, 4), (256, 256, 16), (320, 64, 64)]


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def pack_a(a4):
    """A [r, C, 3, 3] -> the kernels' [r, 9, C] (tap = 3 ky + kx)"""
    return a4.permute(0, 2, 3, 1).reshape(a4.shape[0], 9, a4.shape[1]).contiguous()


def unpack(p):
    """packed [O, 9, I] -> a conv2d weight [O, I, 3, 3]"""
    return p.reshape(p.shape[0], 3, 3, p.shape[2]).permute(0, 3, 1, 2)


def pack_a_flipped(a4):
    """A [r, C, 3, 3] -> [C, 9, r] with [c][tap][j] = A[j][8 - tap][c]: what the up-add kernel takes to compute the transposed
    convolution (the backward's dX)"""
    return a4.flip(2, 3).permute(1, 2, 3, 0).reshape(a4.shape[1], 9, a4.shape[0]).contiguous()


def down_ref(x, a):
    """x [N, H, W, C], a [r, 9, C] -> t [N, H, W, r] in fp64"""
    return nhwc(F.conv2d(nchw(x.double()), unpack(a.double()), padding=1))


def up_add_ref(y, t, b, s):
    """y [N, H, W, Cout] + s conv3x3(t [N, H, W, r], b [Cout, 9, r]) in fp64"""
    return y.double() + s * nhwc(F.conv2d(nchw(t.double()), unpack(b.double()), padding=1))


def dx_ref(g, a4, s):
    """the low-rank part of dX as torch states it: s conv_transpose2d(g, A)"""
    return s * nhwc(F.conv_transpose2d(nchw(g.double()), a4.double(), padding=1))


def wgrad_ref(p, q_, s):
    """d [r, 9, C] = s * (the weight gradient of conv2d(q, .) under the output gradient p), through autograd in fp64"""
    r, C = p.shape[3], q_.shape[3]
    w = torch.zeros(r, C, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(nchw(q_.double()), w, padding=1) * nchw(p.double())).sum().backward()
    return s * pack_a(w.grad)


def expected_conv_adapters(model, conv_targets, rank):
    """{adapter parameter name: shape} from the model's own modules: every 3x3 / 1x1 ``conv1|2|3`` below a ``resnets`` list"""
    out = {}
    for k, v in model.state_dict().items():
        parts = k.split(".")
        if len(parts) >= 4 and parts[-1] == "weight" and parts[-2] in conv_targets and parts[-4] == "resnets":
            base = k[: -len(".weight")]
            out[base + ".lora_A"] = (rank, v.shape[1], 3, 3) if v.shape[2] == 3 else (rank, v.shape[1])
            out[base + ".lora_B"] = (v.shape[0], rank)
    return out


def is_conv_adapter(key):
    return key.split(".")[-2] in CONV_TARGETS


def merged_state_dict(sd, leaves, scale, conv_scale):
    """sd with every adapted ``<layer>.<target>.weight`` replaced by W + s (B @ A.view(r, -1)).view_as(W)"""
    out = dict(sd)
    for k, a in leaves.items():
        if not k.endswith(".lora_A"):
            continue
        base = k[: -len(".lora_A")]
        b = leaves[base + ".lora_B"]
        w = sd[base + ".weight"]
        s = conv_scale if is_conv_adapter(k) else scale
        out[base + ".weight"] = w + s * (b @ a.reshape(a.shape[0], -1)).reshape(w.shape)
    return out


def oracle_lora_run(name, values, scale, conv_scale, dtype=torch.float32):
    """-> (outputs, {adapter name: gradient}) of the oracle on the merged state dict, loss = parity_cases.loss_of"""
    _, cfg, sd = PC.build_module(name)
    inp = PC.inputs(name)
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in values.items()}
    base = {k: v.to(dtype) for k, v in sd.items()}
    cast = lambda t: [u.to(dtype) for u in t] if isinstance(t, list) else t.to(dtype)
    outs = O.model_forward(merged_state_dict(base, leaves, scale, conv_scale), cfg, cast(inp["x"]), inp["times"],
                           inp["cond"].to(dtype), inp["mask"].to(dtype), inp["micros"])
    PC.loss_of(outs, inp["gys"]).backward()
    return [o.detach().float() for o in PC.as_list(outs)], {k: v.grad.detach().float() for k, v in leaves.items()}


seeded_b, adapter_values, agg_err, relerr, q, TOL = LC.seeded_b, LC.adapter_values, LC.agg_err, LC.relerr, LC.q, LC.TOL
