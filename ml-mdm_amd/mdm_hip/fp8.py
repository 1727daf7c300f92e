"""Opt-in MXFP8 (OCP MX, E4M3 codes + one power-of-two scale byte per 32 channels) weights AND activations for the
plain-GEMM layers of every ``SelfAttention`` and, on request, the convolutions of every ``ResNet`` of a UNet / NestedUNet
on the HIP path -- sampling only.

    h = fp8.attach(vision_model)                 # targets=("qkv", "proj_out", "ffn"), inner nets included
    h = fp8.attach(vision_model, conv_targets=fp8.CONV_TARGETS)          # ... and conv1 / conv2 / conv3 of every ResNet
    h = fp8.attach(vision_model, targets=(), conv_targets=("conv1", "conv2"), min_channels=128)   # the ResNets alone
    ... sample (bf16 activations: torch.autocast or MDM_HIP_DTYPE=bf16, under torch.no_grad()) ...
    h.detach()

With the handle attached a layer runs (``csrc/fp8.hip``)

    hn -> mx8_quant -> qkv GEMM       (bf16 out; the attention itself is unchanged)
    a  -> mx8_quant -> proj_out GEMM  (+ residual)
    fn -> mx8_quant -> FFN-up GEMM    (bias + GELU, emits MXFP8 from its epilogue) -> FFN-down GEMM (bias + residual, bf16 out)

and a targeted ResNet (reference models/unet.py:223-238)

    GN+SiLU       -> mx8_quant_zrow -> conv1: 3x3 implicit GEMM, nine taps over the one quantised tensor (bias)
    GN+FiLM+SiLU  -> mx8_quant_zrow -> conv2: the same (bias + the shortcut as the epilogue's residual)
    x             -> mx8_quant      -> conv3: the 1x1 shortcut, where the block changes its channel count (bias)

on ``v_mfma_scale_f32_16x16x128_f8f6f4``.  The weights are quantised from the fp32 masters once per parameter version
(``ops.packed_weight_mx8`` / ``ops.packed_weight_mx8_3x3``: ``load_state_dict``, an EMA swap or a LoRA ``merge()``
re-quantise by themselves).  ``min_channels`` leaves a ResNet with ``min(Cin, Cout)`` below it on bf16: the k-tile is 128
channels, so a narrower convolution multiplies mostly padding.  The stride-2 / sub-pixel resampling convolutions,
``conv_in`` / ``conv_out``, the nested adapters, ``kv_cond`` (computed once per ``sample()``), the time MLPs and all of
training stay as they are.

The handle is NOT part of the model's module tree (``SelfAttention._fp8`` / ``ResNet._fp8``, a plain attribute like ``_lora``):
``state_dict()`` keys and values are untouched.  There is no backward: an input that requires grad (in grad mode) and fp32
activations raise ``MdmHipError``.  Cost in accuracy: e4m3 has a 3-bit mantissa -- about 4 % relative L2 per GEMM with both
operands quantised; with random weights image quality is not judged.
"""
import torch

from . import ops
from ._lib import MdmHipError
from .unet import ResNet, SelfAttention

TARGETS = ("qkv", "proj_out", "ffn")
CONV_TARGETS = ("conv1", "conv2", "conv3")


class _LayerFp8:
    """what one SelfAttention / ResNet layer sees: which of its projections run in MXFP8 (a plain object, nothing registers)"""

    __slots__ = ("owner", "targets")

    def __init__(self, owner, targets):
        self.owner, self.targets = owner, targets

    def on(self, target):
        return target in self.targets

    @staticmethod
    def _bf16(x):
        if x.dtype != torch.bfloat16:
            raise MdmHipError("the MXFP8 layers take bf16 activations (got %s): sample under torch.autocast / "
                              "MDM_HIP_DTYPE=bf16, or detach() the fp8 handle" % x.dtype)

    def conv(self, x, module, residual=None):
        """the 1x1 convolution ``module`` on the NHWC activation x, both operands in MXFP8 (+ residual)"""
        self._bf16(x)
        w, b = ops.packed_weight_mx8(module.weight, module.bias)
        y = ops.mx8_gemm(ops.mx8_quant(x), w, b, residual=residual)
        return y.reshape(*x.shape[:-1], w.rows)

    def conv3x3(self, x, module, residual=None):
        """the 3x3 convolution ``module`` (stride 1, padding 1) on the NHWC activation x, both operands in MXFP8 (+ residual)"""
        self._bf16(x)
        w, b = ops.packed_weight_mx8_3x3(module.weight, module.bias)
        return ops.mx8_conv3x3(ops.mx8_quant_zrow(x), w, x.shape[:3], b, residual=residual)

    def ffn(self, x, up, down, residual):
        """down(gelu(up(x))) + residual; the hidden tensor leaves the first GEMM's epilogue as MXFP8"""
        self._bf16(x)
        w1, b1 = ops.packed_weight_mx8(up.weight, up.bias)
        w2, b2 = ops.packed_weight_mx8(down.weight, down.bias)
        h = ops.mx8_gemm(ops.mx8_quant(x), w1, b1, gelu=True, emit=True)
        y = ops.mx8_gemm(h, w2, b2, residual=residual)
        return y.reshape(*x.shape[:-1], w2.rows)


class Fp8Layers:
    """The MXFP8 handle of one vision model: ``layers`` [(name, SelfAttention, targets of that layer)] and ``convs``
    [(name, ResNet, conv targets of that block)]"""

    def __init__(self, layers, convs=()):
        self.layers = layers
        self.convs = list(convs)
        self.attached = True
        for _, layer, targets in self.layers + self.convs:
            layer._fp8 = _LayerFp8(self, targets)
        ops.bump_adapter_epoch()

    def detach(self):
        """restore the layers: their forward launches exactly what it did before attach()"""
        if not self.attached:
            raise RuntimeError("this fp8 handle is detached already")
        for _, layer, _ in self.layers + self.convs:
            layer._fp8 = None
        self.attached = False
        ops.bump_adapter_epoch()


def _convs_of(layer, target):
    if target == "ffn":
        return [] if layer.ffn is None else [("ffn.1", layer.ffn[1]), ("ffn.3", layer.ffn[3])]
    return [(target, getattr(layer, target))]


def attach(vision_model, targets=TARGETS, conv_targets=(), min_channels=0) -> Fp8Layers:
    """-> Fp8Layers: every ``SelfAttention`` of ``vision_model`` (UNet / NestedUNet, inner nets included) runs the targeted
    projections in MXFP8 from now on, and every ``ResNet`` the convolutions named in ``conv_targets`` (a subset of
    CONV_TARGETS; empty by default; ``conv3`` where the block has one) unless ``min(Cin, Cout) < min_channels``.
    ``targets=()`` is legal with conv targets.  Refused (the model is left alone): unknown targets, attention targets on a
    model without attention layers, conv targets on a model without ResNets, a targeted layer whose channel counts are not
    multiples of 32 (named), a layer with unmerged LoRA adapters, a model that has a handle already.  While the handle is
    attached ``lora.attach`` (attention targets on fp8 attention layers, conv targets on fp8 ResNets) and ``unmerge()``
    refuse the model in turn: detach() first."""
    targets = (targets,) if isinstance(targets, str) else tuple(targets)
    conv_targets = (conv_targets,) if isinstance(conv_targets, str) else tuple(conv_targets)
    bad = [t for t in targets if t not in TARGETS]
    if bad or not (targets or conv_targets):
        raise ValueError("fp8 targets must be a non-empty subset of %s, got %r%s" % (
            set(TARGETS), targets, " (ResNet convolutions go in conv_targets)" if any(t in CONV_TARGETS for t in bad) else ""))
    bad = [t for t in conv_targets if t not in CONV_TARGETS]
    if bad:
        raise ValueError("fp8 conv targets must be a subset of %s, got %r" % (set(CONV_TARGETS), conv_targets))
    layers = sorted(((n, m) for n, m in vision_model.named_modules() if isinstance(m, SelfAttention)), key=lambda e: e[0])
    resnets = sorted(((n, m) for n, m in vision_model.named_modules() if isinstance(m, ResNet)), key=lambda e: e[0])
    if targets and not layers:
        raise ValueError("the model has no attention layer to run in fp8")
    if conv_targets and not resnets:
        raise ValueError("the model has no ResNet block to run in fp8")
    if any(m._fp8 is not None for _, m in layers + resnets):
        raise RuntimeError("the model already has an fp8 handle attached: detach() it first")
    found = []
    for name, layer in layers if targets else []:
        lo = layer._lora
        if lo is not None and not lo.owner.merged:
            raise RuntimeError("%s has unmerged LoRA adapters: merge() first (the fp8 weights are quantised from the merged "
                               "masters)" % name)
        mine = []
        for t in TARGETS:
            if t not in targets:
                continue
            convs = _convs_of(layer, t)
            for sub, conv in convs:
                cout, cin = conv.weight.shape[0], conv.weight.shape[1]
                if cin % 32 or cout % 32:
                    raise ValueError("%s.%s: %d -> %d channels; the MXFP8 GEMM needs multiples of 32" % (name, sub, cin, cout))
            if convs:
                mine.append(t)
        if mine:
            found.append((name, layer, tuple(mine)))
    if targets and not found:
        raise ValueError("none of the targets %r exists in this model's attention layers" % (targets,))
    found_convs = []
    for name, block in resnets if conv_targets else []:
        lo = block._lora
        if lo is not None and not lo.owner.merged:
            raise RuntimeError("%s has unmerged LoRA adapters: merge() first (the fp8 weights are quantised from the merged "
                               "masters)" % name)
        cout, cin = block.conv1.weight.shape[0], block.conv1.weight.shape[1]
        if min(cin, cout) < min_channels:
            continue
        mine = tuple(t for t in CONV_TARGETS if t in conv_targets and getattr(block, t, None) is not None)
        for t in mine:
            w = getattr(block, t).weight
            if w.shape[0] % 32 or w.shape[1] % 32:
                raise ValueError("%s.%s: %d -> %d channels; the MXFP8 convolution needs multiples of 32" % (name, t, w.shape[1], w.shape[0]))
        if mine:
            found_convs.append((name, block, mine))
    if conv_targets and not found_convs:
        raise ValueError("none of the conv targets %r exists in this model's ResNet blocks at min_channels=%d" % (conv_targets, min_channels))
    return Fp8Layers(found, found_convs)
