"""Cases shared by the FreeU tests (CPU and GPU).  Yardsticks that import nothing from the code under test (the stub at the
end excepted: it holds one real, never run ``ResNetBlock`` for the selection to find):

  fourier_filter_ref   FreeU's Fourier filter as the paper's code states it, ``torch.fft`` in fp64
  freeu_ref            the whole definition in fp64: scaled backbone (v1 / v2), filtered skip, concat
  closed_form          the seven-mode closed form of the filter, in fp64 and in fp32 (the accumulation yardstick)
  level_freeu          a copy of ``unet_oracle.level`` with its one ``torch.cat`` line replaced by ``freeu_ref``, and
  freeu_oracle         the context that swaps it into the imported oracle module, level by level

Tensors here are NCHW like the oracle's; ``nhwc`` / ``nchw`` convert for the kernels."""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

import parity_cases as PC
import unet_oracle as O


# ---- the definition ----------------------------------------------------------------------------------------------------
def fourier_filter_ref(r, s, threshold=1):
    """fp64: Re ifft2(ifftshift(mask * fftshift(fft2(r)))), mask = s on rows H//2 - t .. H//2 + t - 1 and columns
    W//2 - t .. W//2 + t - 1 of the shifted spectrum, 1 elsewhere.  r [..., H, W]."""
    r = r.double()
    H, W = r.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fft2(r), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=torch.float64)
    mask[H // 2 - threshold: H // 2 + threshold, W // 2 - threshold: W // 2 + threshold] = s
    return torch.fft.ifft2(torch.fft.ifftshift(f * mask, dim=(-2, -1))).real


def backbone_scale_ref(h, b, structure):
    """fp64 m [N, 1, H, W] (v2) or the number b (v1): v2 is 1 + (b - 1) hm, hm the per-sample min-max normalised mean over
    ALL channels; where max == min, hm = 1"""
    if not structure:
        return b
    mu = h.double().mean(dim=1, keepdim=True)
    mn = mu.amin(dim=(2, 3), keepdim=True)
    mx = mu.amax(dim=(2, 3), keepdim=True)
    span = mx - mn
    hm = torch.where(span > 0, (mu - mn) / torch.where(span > 0, span, torch.ones_like(span)), torch.ones_like(mu))
    return 1 + (b - 1) * hm


def freeu_ref(h, r, b, s, structure=False):
    """fp64 [N, C1 + C2, H, W]: cat(h', r') with h'[:, :C1 // 2] = h m, the other backbone channels untouched, and r' the
    Fourier-filtered skip"""
    h, r = h.double(), r.double()
    half = h.shape[1] // 2
    hp = torch.cat([h[:, :half] * backbone_scale_ref(h, b, structure), h[:, half:]], dim=1)
    return torch.cat([hp, fourier_filter_ref(r, s)], dim=1)


def closed_form(r, s, dtype=torch.float64):
    """r + (s - 1) / (H W) sum_k coef_k phi_k, coef_k = sum_{y, x} r phi_k, over the seven real modes
    {1, cos t1, sin t1, cos t2, sin t2, cos t3, sin t3}, t1 = 2 pi y / H, t2 = 2 pi x / W, t3 = t1 + t2 -- every step in
    ``dtype``"""
    r = r.to(dtype)
    H, W = r.shape[-2:]
    t1 = (2 * math.pi * torch.arange(H, dtype=dtype) / H).reshape(H, 1).expand(H, W)
    t2 = (2 * math.pi * torch.arange(W, dtype=dtype) / W).reshape(1, W).expand(H, W)
    t3 = t1 + t2
    acc = torch.zeros_like(r)
    for phi in (torch.ones(H, W, dtype=dtype), t1.cos(), t1.sin(), t2.cos(), t2.sin(), t3.cos(), t3.sin()):
        acc = acc + (r * phi).sum(dim=(-2, -1), keepdim=True) * phi
    return r + ((s - 1) / (H * W)) * acc


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---- kernel cases ------------------------------------------------------------------------------------------------------
# (N, H, W, C1, C2): the smallest legal shape; odd, non-square, ragged pixel count; the mini model's low-resolution level;
# many pixel slabs with few channels; more channels than one block's chunk
KERNEL_SHAPES = [(1, 2, 2, 16, 8), (2, 5, 3, 32, 24), (3, 8, 8, 256, 256), (2, 64, 64, 16, 8), (1, 4, 4, 1536, 768)]
KERNEL_PARAMS = [(1.4, 0.2), (0.7, 1.7)]   # (b, s): amplify + damp, and the reverse


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, seed=0):
    """(h [N, C1, H, W], r [N, C2, H, W]) fp32, made once and never written.  h carries a per-pixel offset so that its
    channel mean spreads: max mu - min mu >= 0.1 max |mu| with room to spare (the v2 scale map divides by it)."""
    N, H, W, C1, C2 = shape
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C1 + seed)
    h = torch.randn(N, C1, H, W, generator=g) + torch.randn(N, 1, H, W, generator=g)
    r = torch.randn(N, C2, H, W, generator=g)
    mu = h.double().mean(dim=1)
    span = mu.amax(dim=(1, 2)) - mu.amin(dim=(1, 2))
    assert bool((span >= 0.1 * mu.abs().amax(dim=(1, 2))).all())
    return h, r


def closed_form_fp32_error():
    """the largest |fp32 closed form - fp64 definition| / max |input| over KERNEL_SHAPES x the s of KERNEL_PARAMS, on
    ``kernel_inputs``: what fp32 accumulation of the seven sums costs"""
    worst = 0.0
    for shape in KERNEL_SHAPES:
        _, r = kernel_inputs(shape)
        for _, s in KERNEL_PARAMS:
            err = (closed_form(r, s, torch.float32).double() - fourier_filter_ref(r, s)).abs().max() / r.abs().max()
            worst = max(worst, float(err))
    return worst


# Measured on the CPU (tests/test_freeu_host.py::test_fp32_closed_form_error_is_the_recorded_figure prints and checks it):
# closed_form_fp32_error() = 7.29e-8 (the worst case is (2, 5, 3, 32, 24) at s = 0.2; every case lies in 3.1e-8 ..
# 7.3e-8: about one rounding of the result at the size of the largest input).  The gate of the elementwise GPU checks is
# c = 8 x that = 5.84e-7, the margin for another summation order and the device's sine and cosine.
FP32_CLOSED_FORM_ERROR = 7.3e-8
C_GATE = 8 * FP32_CLOSED_FORM_ERROR

# Model-level settings: b1 = b2 and s1 = s2.  tests/test_freeu_host.py checks that they move the oracle's outputs by a
# rel-L2 above 1e-2 on mini_unet and mini_nested, so that the model-level tests are not vacuous.
MODEL_B, MODEL_S = (1.4, 1.4), (0.2, 0.2)


# ---- the oracle with FreeU levels ------------------------------------------------------------------------------------
def level_freeu(sd, pfx, x, temb, groups, n_res, n_attn, mode, cond, cond_mask, skips=None, b=1.0, s=1.0, structure=False):
    """``unet_oracle.level`` with the skip concat replaced by ``freeu_ref`` (computed in fp64, returned in x's dtype)"""
    acts = []
    for i in range(n_res):
        if skips is not None:
            x = freeu_ref(x, skips.pop(0), b, s, structure).to(x.dtype)
        x = O.resnet(sd, "%sresnets.%d." % (pfx, i), x, temb, groups)
        for j in range(n_attn):
            x = O.attention_layer(sd, "%sattn.%d." % (pfx, i * n_attn + j), x, cond, cond_mask)
        acts.append(x)
    if mode == "down":
        x = O._conv(sd, pfx + "resample", x, stride=2)
        acts.append(x)
    elif mode == "up":
        x = O._conv(sd, pfx + "resample", F.interpolate(x, scale_factor=2, mode="nearest"))
        acts.append(x)
    return x, acts


@contextlib.contextmanager
def freeu_oracle(sd, levels, structure=False):
    """Inside, ``unet_oracle.level`` applies FreeU at the up blocks ``levels`` = {module name of the whole model, e.g.
    ``inner_unet.up_blocks.0``: (b, s)} of the state dict ``sd``.  The oracle hands a nested net a sub-dict of the SAME
    tensors under shortened keys, so a level is recognised by the identity of its ``resnets.0.conv1.weight`` tensor."""
    ids = {id(sd[n + ".resnets.0.conv1.weight"]): bs for n, bs in levels.items()}
    orig = O.level

    def level(sd_, pfx, x, temb, groups, n_res, n_attn, mode, cond, cond_mask, skips=None):
        bs = ids.get(id(sd_[pfx + "resnets.0.conv1.weight"]))
        if bs is not None and skips is not None:
            return level_freeu(sd_, pfx, x, temb, groups, n_res, n_attn, mode, cond, cond_mask, skips, bs[0], bs[1], structure)
        return orig(sd_, pfx, x, temb, groups, n_res, n_attn, mode, cond, cond_mask, skips)

    O.level = level
    try:
        yield
    finally:
        O.level = orig


INNER = {"mini_unet": "", "mini_nested": "inner_unet.", "mini_nested2": "inner_unet.inner_unet."}


def deepest2(name, b=MODEL_B, s=MODEL_S):
    """the levels dict of "deepest2" for a mini model, written out by hand"""
    return {INNER[name] + "up_blocks.0": (b[0], s[0]), INNER[name] + "up_blocks.1": (b[1], s[1])}


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, b=None, s=None, structure=False, dtype=torch.float32):
    """oracle forward of ``PC.inputs(name)`` in ``dtype`` on the CPU with FreeU at the two deepest up blocks
    (``b=None``: the plain oracle) -> list of outputs"""
    _, cfg, sd = PC.build_module(name)
    inp = PC.inputs(name)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    cast = lambda t: [u.to(dtype) for u in t] if isinstance(t, list) else t.to(dtype)
    ctx = contextlib.nullcontext() if b is None else freeu_oracle(sd, deepest2(name, b, s), structure)
    with torch.no_grad(), ctx:
        outs = O.model_forward(sd, cfg, cast(inp["x"]), inp["times"], inp["cond"].to(dtype), inp["mask"].to(dtype), {})
    return [o.detach() for o in PC.as_list(outs)]


# ---- a stub denoiser that records its calls, with one real (never run) up block to select -------------------------------
class RecordingStub(torch.nn.Module):
    """``model(x, t, lm_outputs, lm_mask, micros)`` as the samplers call it: a row-wise function of (x, t, text) plus a term
    that depends on the ``_freeu`` switch of the stub's one up block at the time of the call.  Every call is recorded."""

    def __init__(self, nested=False):
        super().__init__()
        from mdm_hip.unet import ResNetBlock, ResNetConfig

        self.nested = nested
        self.up_blocks = torch.nn.ModuleList(
            [ResNetBlock(8, 1, 0, False, False, resnet_configs=[ResNetConfig(num_channels=16, output_channels=8, num_groups_norm=4)])])
        self.nest_ratio = [1]   # two scales of one size: unit image scales, one schedule
        self.calls = []

    @property
    def vision_model(self):
        return self

    def one(self, x, t, lm, k):
        sw = self.up_blocks[0]._freeu
        c = lm.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        tt = (t.float() / 1000.0).reshape(-1, 1, 1, 1)
        out = (0.3 + 0.1 * k) * x + 0.1 * torch.tanh(3 * tt) + 0.4 * c
        if sw is not None:
            b, s, structure = sw
            out = out + 0.05 * (b - 1) * torch.roll(x, 1, dims=-1) + 0.07 * (s - 1) + (0.03 if structure else 0.0)
        return out

    def forward(self, x, t, lm, mask, micros={}):
        self.calls.append(dict(t=t.clone(), freeu=self.up_blocks[0]._freeu, name=self.up_blocks[0]._freeu_name))
        if self.nested:
            return [self.one(v, t, lm, k) for k, v in enumerate(x)]
        out = self.one(x, t, lm, 0)
        return out, torch.ones_like(out)
