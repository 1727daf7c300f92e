"""Yardsticks for input gradients and loss-guided sampling that do not come from the package under test.

(a) ``stem_dgrad_reference``: the input gradient of the 3x3 stem convolution by fp64 autograd of ``F.conv2d`` on the
    dtype-rounded operands; ``impulse_expected``: the same for a one-hot ``dy``, written out by hand.
(b) ``restated_step_loss``: ``loss(fn(threshold(x0(x_t, model(x_t)))))`` as one differentiable torch expression (the
    per-sample quantile of a dynamic threshold is a constant), for autograd in float64.
(c) ``OracleNet``: the CPU oracle (oracle/unet_oracle.py, plain torch, differentiable in its input) behind the vision
    model's call surface; ``masked_mse``: the measurement loss of the sampler tests.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_oracle as O

# (N, H, W, Cout, Cin)
STEM_SHAPES = [
    (2, 16, 16, 32, 3),     # the existing stem test's shape
    (1, 5, 7, 40, 3),       # nothing a multiple of any tile; channel tail
    (3, 1, 9, 8, 1),        # one row (every vertical tap out of image), smallest Cout, one input channel
    (1, 33, 65, 256, 6),    # tile seams in both directions at UNet-64's stem width
]
MODEL_CASES = ["mini_unet", "mini_unet_masked", "mini_nested", "mini_nested2", "mini_nested_mixed"]


def stem_operands(shape, dtype, kind, seed=0):
    """-> (dy [N, H, W, Cout] of dtype, w [Cout, Cin, 3, 3] fp32), CPU.  kind "int": both from {-2 .. 2}; "rand": normal dy
    already rounded to dtype (the weight is rounded by the pack, and by the reference below)"""
    N, H, W, Cout, Cin = shape
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "int":
        dy = torch.randint(-2, 3, (N, H, W, Cout), generator=g).to(dtype)
        w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float()
    else:
        dy = torch.randn(N, H, W, Cout, generator=g).to(dtype)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    return dy, w


def stem_dgrad_reference(dy, w, dtype):
    """dx [N, Cin, H, W] fp64: autograd of F.conv2d(x, w rounded to dtype, padding=1) with output gradient dy"""
    N, H, W, Cout = dy.shape
    x = torch.zeros(N, w.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.to(dtype).double(), padding=1)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return x.grad


def impulse_positions(H, W):
    """the four corners, an edge midpoint and the centre"""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 2)]


def impulse_expected(w, dtype, shape, n, py, px, co):
    """dx for dy = one-hot at (n, py, px, co): dx[n, ci, qy, qx] = w[co, ci, qy - py + 1, qx - px + 1] (the flipped filter
    around the impulse), clipped by the image, zero elsewhere"""
    N, H, W, _, Cin = shape
    wr = w.to(dtype).float()
    dx = torch.zeros(N, Cin, H, W)
    for ky in range(3):
        for kx in range(3):
            qy, qx = py + ky - 1, px + kx - 1
            if 0 <= qy < H and 0 <= qx < W:
                dx[n, :, qy, qx] = wr[co, :, ky, kx]
    return dx


# ---- (b) ---------------------------------------------------------------------------------------------------------
def _col(v):
    return v.reshape(-1, 1, 1, 1)


def restated_step_loss(x_t, model_fn, g, fn, prediction, threshold, image_scale=1.0, guidance=1.0):
    """sum_b loss_b as a differentiable function of x_t (float64).  ``model_fn(x) -> (cond prediction, uncond prediction
    or None)``; ``prediction`` "DDPM" | "V_PREDICTION"; ``threshold`` "NONE" | "CLIP" | "DYNAMIC"."""
    pc, pu = model_fn(x_t)
    p = pc if pu is None else pu + guidance * (pc - pu)
    g = _col(g)
    if prediction == "V_PREDICTION":
        x0 = g.sqrt() * x_t - (1 - g).sqrt() * p
    else:
        x0 = (x_t - (1 - g).sqrt() * p) / g.sqrt()
    x0 = x0 * image_scale
    if threshold == "CLIP":
        x0 = x0.clamp(-1, 1)
    elif threshold == "DYNAMIC":
        s = torch.quantile(x0.detach().reshape(x0.shape[0], -1).abs(), 0.995, dim=1).clamp(min=1, max=100)
        s = _col(s)
        x0 = torch.maximum(torch.minimum(x0, s), -s) / s
    return fn(x0).sum()   # x0 is in image units here: the scale divided out by the step and multiplied back by _postprocess


def masked_mse(target, mask):
    """loss_b = sum over the measured pixels of (x0 - target)^2: the measurement of the sampler tests"""
    def fn(x0):
        return ((x0 - target.to(x0)) * mask.to(x0)).pow(2).sum(dim=(1, 2, 3))
    return fn


# ---- (c) ---------------------------------------------------------------------------------------------------------
class OracleNet(nn.Module):
    """oracle/unet_oracle.py behind the vision model's call surface, CPU fp32: the same parameters as the HIP module"""

    def __init__(self, sd, cfg, nested):
        super().__init__()
        self.sd = {k: v.clone().float() for k, v in sd.items()}
        self.cfg = cfg
        self.input_channels = 3
        if nested:
            self.nest_ratio = [2]   # mini_nested: 32 + 16
            self.is_temporal = [False]

    def forward(self, x_t, times, lm_outputs, lm_mask, micros={}):
        return O.model_forward(self.sd, self.cfg, x_t, times, lm_outputs, lm_mask, micros or None)
