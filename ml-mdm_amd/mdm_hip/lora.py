"""Low-rank adapters (LoRA, Hu et al. 2021) for the attention projections and the ResNet convolutions of a UNet /
NestedUNet on the HIP path.

    y = W x + b + (alpha / r) B (A x)        A [r, Cin], B [Cout, r] trainable; W, b frozen
    y = conv3x3(x, W) + b + (alpha / r) B conv3x3(x, A)      A [r, Cin, 3, 3] (a Conv2d(Cin, r, 3, padding=1) weight), B [Cout, r]

``attach(vision_model, rank=16)`` adapts the ``qkv``, ``kv_cond`` and ``proj_out`` projections of every ``SelfAttention``
layer (inner nets of a nested model included) and returns a ``LoraAdapters`` module that owns the new parameters.  The
adapters are NOT part of the vision model's module tree: ``vision_model.state_dict()`` / ``save()`` / ``load()`` keep the
reference's keys and shapes; a layer finds its adapters through the plain attribute ``SelfAttention._lora``.  The adapter
term runs in kernels of its own (``csrc/lora.hip``: ``ops.lora``) right behind the base projection's launch.
``merge()`` folds ``s B A`` into the fp32 master weights -- sampling then costs nothing extra and the checkpoint is a plain
reference checkpoint -- and ``unmerge()`` takes it out again.  Training keeps the term separate: a bf16 copy of
``W + s B A`` would round small updates away.

``conv_targets=("conv1", "conv2", "conv3")`` (any subset; empty by default) also adapts those convolutions of every
``ResNet`` block -- the only layers the outer nets of a nested model have.  The 3x3 ones get a rank-r 3x3 down-projection
(``ops.lora_conv``; merged: ``W + s (B @ A.view(r, 9 Cin)).view_as(W)``), the 1x1 shortcut ``conv3`` the 2-D form above.
They carry a rank and scale of their own (``conv_rank``, ``conv_alpha``: 32- and 64-channel nets want a smaller rank than
768-wide attention) and are drawn from the same generator AFTER all attention adapters, so the attention adapters'
values do not depend on whether conv adapters were asked for.  ``targets=()`` with conv targets adapts a net without
attention.

The reference has no counterpart.  Not covered: the stride-2 / sub-pixel ``resample`` convolutions, ``conv_in`` /
``conv_out``, the nested ``in_adapter`` / ``out_adapter``, the FFN (its GELU sits in the first GEMM's epilogue), dropout on
the adapter path, per-layer ranks beyond the attention / conv split, ``ModelEma`` tracking, the fused train step and
``mdm_hip.distributed.DataParallel`` (``trainer.train_batch`` takes its plain path for an optimizer over adapters).
"""
import math

import torch
import torch.nn as nn

from . import ops
from .unet import ResNet, SelfAttention

TARGETS = ("qkv", "kv_cond", "proj_out")
CONV_TARGETS = ("conv1", "conv2", "conv3")
RANKS = (4, 8, 16, 32, 64)


class _LayerAdapters:
    """what one SelfAttention / ResNet layer sees of its adapters (a plain object: nothing registers in the layer's module
    tree); ``conv``: a ResNet's handle -- the conv adapters' own scale, and the 3x3 op for a 4-D ``A``"""

    __slots__ = ("owner", "pairs", "conv")

    def __init__(self, owner, conv=False):
        self.owner, self.pairs, self.conv = owner, {}, conv

    def active(self, target):
        return target in self.pairs and not self.owner.merged

    def apply(self, target, y, x):
        """y (the base projection's fresh output) with the adapter term of ``target`` added in place; x: the projection's input"""
        if not self.active(target):
            return y
        a, b = self.pairs[target]
        if not self.conv:
            return ops.lora(y, x, a, b, self.owner.scale)
        return (ops.lora_conv if a.dim() == 4 else ops.lora)(y, x, a, b, self.owner.conv_scale)


class _Node(nn.Module):
    pass


class LoraAdapters(nn.Module):
    """The adapter parameters of one vision model: ``<layer name>.<target>.lora_A`` / ``.lora_B`` (fp32, on the device of
    the base weight), plus ``rank`` and ``alpha`` in the state dict -- and ``conv_rank`` / ``conv_alpha`` when there are
    adapters on ResNet convolutions (``<resnet name>.conv1.lora_A`` [r, Cin, 3, 3], ``conv3``: [r, Cin])."""

    def __init__(self, vision_model, rank, alpha, targets, seed, freeze_base, conv_targets=(), conv_rank=None, conv_alpha=None):
        super().__init__()
        self._rank, self._alpha = int(rank), float(alpha)
        self._conv_rank = self._rank if conv_rank is None else int(conv_rank)
        self._conv_alpha = float(self._conv_rank if conv_alpha is None else conv_alpha)
        self.register_buffer("rank", torch.tensor(self._rank, dtype=torch.int64))
        self.register_buffer("alpha", torch.tensor(self._alpha, dtype=torch.float64))
        self.targets = tuple(t for t in TARGETS if t in targets)
        self.conv_targets = tuple(t for t in CONV_TARGETS if t in conv_targets)
        self.merged = False
        self._entries = []   # (layer name, layer, target, base module, A, B)
        layers = sorted(((n, m) for n, m in vision_model.named_modules() if isinstance(m, SelfAttention)), key=lambda e: e[0])
        gen = torch.Generator().manual_seed(int(seed))
        for name, layer in layers:
            handle = _LayerAdapters(self)
            for target in self.targets:
                base = getattr(layer, target, None)
                if base is None:     # an attention layer without text conditioning has no kv_cond
                    continue
                w = base.weight
                cout, cin = w.shape[0], w.shape[1]
                if cin % 8 or cout % 8:
                    raise ValueError("%s.%s: %d -> %d channels; the adapter kernels need multiples of 8" % (name, target, cin, cout))
                a = nn.Parameter((torch.randn(self._rank, cin, generator=gen) / math.sqrt(cin)).to(w.device))
                b = nn.Parameter(torch.zeros(cout, self._rank, device=w.device))
                self._register(name + "." + target, a, b)
                handle.pairs[target] = (a, b)
                self._entries.append((name, layer, target, base, a, b))
            if handle.pairs:
                layer._lora = handle
        if self.targets and not self._entries:
            for _, layer in layers:
                layer._lora = None
            raise ValueError("none of the targets %r exists in this model's attention layers" % (self.targets,))
        # ResNet convolutions: drawn AFTER every attention adapter, in sorted ResNet-name order, conv1, conv2, conv3
        resnets = sorted(((n, m) for n, m in vision_model.named_modules() if isinstance(m, ResNet)), key=lambda e: e[0]) \
            if self.conv_targets else []
        n_attn = len(self._entries)
        try:
            for name, layer in resnets:
                handle = _LayerAdapters(self, conv=True)
                for target in self.conv_targets:
                    base = getattr(layer, target, None)
                    if base is None:     # a ResNet that keeps its channel count has no conv3
                        continue
                    w = base.weight
                    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
                    if cin % 8 or cout % 8:
                        raise ValueError("%s.%s: %d -> %d channels; the adapter kernels need multiples of 8" % (name, target, cin, cout))
                    shape = (self._conv_rank, cin, 3, 3) if k == 3 else (self._conv_rank, cin)
                    a = nn.Parameter((torch.randn(shape, generator=gen) / math.sqrt(cin * k * k)).to(w.device))
                    b = nn.Parameter(torch.zeros(cout, self._conv_rank, device=w.device))
                    self._register(name + "." + target, a, b)
                    handle.pairs[target] = (a, b)
                    self._entries.append((name, layer, target, base, a, b))
                if handle.pairs:
                    layer._lora = handle
        except ValueError:
            for _, layer in layers + resnets:
                layer._lora = None
            raise
        if len(self._entries) == n_attn and self.conv_targets:
            for _, layer in layers + resnets:
                layer._lora = None
            raise ValueError("none of the conv targets %r exists in this model's ResNet blocks" % (self.conv_targets,))
        if len(self._entries) > n_attn:     # an attention-only state dict keeps exactly the keys it had
            self.register_buffer("conv_rank", torch.tensor(self._conv_rank, dtype=torch.int64))
            self.register_buffer("conv_alpha", torch.tensor(self._conv_alpha, dtype=torch.float64))
        self._found = [(p, p.requires_grad) for p in vision_model.parameters()]
        if freeze_base:
            for p, _ in self._found:
                p.requires_grad = False
        ops.bump_adapter_epoch()

    def _register(self, path, a, b):
        node = self
        for part in path.split("."):
            if part not in node._modules:
                node.add_module(part, _Node())
            node = node._modules[part]
        node.lora_A, node.lora_B = a, b

    @property
    def scale(self):
        return self._alpha / self._rank

    @property
    def conv_scale(self):
        return self._conv_alpha / self._conv_rank

    def _fold(self, sign):
        with torch.no_grad():
            for _, layer, _, base, a, b in self._entries:
                w = base.weight.detach()
                s = self.conv_scale if isinstance(layer, ResNet) else self.scale
                # W [Cout, Cin (x 9)] += (+-s) B A on the fp32 master: t = B [Cout, r], b = A^T [Cin (x 9), r]
                a2 = a.detach().reshape(a.shape[0], -1)
                ops.lora_up_add(w.view(w.shape[0], a2.shape[1]), b.detach().contiguous(), a2.t().contiguous(), sign * s)
        ops.invalidate_packed_weights()
        ops.bump_adapter_epoch()

    def merge(self):
        """fold s B A into the fp32 master weights (on the GPU); forward then launches nothing for the adapters"""
        if self.merged:
            raise RuntimeError("the adapters are merged already")
        self._attached()
        self._fold(1.0)
        self.merged = True

    def unmerge(self):
        if not self.merged:
            raise RuntimeError("the adapters are not merged")
        self._attached()
        if any(getattr(layer, "_fp8", None) is not None for _, layer, _, _, _, _ in self._entries):
            raise RuntimeError("the model's adapted layers run in MXFP8 (mdm_hip.fp8): detach() the fp8 handle before unmerge()")
        self._fold(-1.0)
        self.merged = False

    def _attached(self):
        if not self._entries or self._entries[0][1]._lora is None or self._entries[0][1]._lora.owner is not self:
            raise RuntimeError("these adapters are detached from their model")

    def detach(self):
        """remove the adapters from the model and restore ``requires_grad`` as attach() found it (merged weights stay merged)"""
        self._attached()
        for _, layer, _, _, _, _ in self._entries:
            layer._lora = None
        for p, flag in self._found:
            p.requires_grad = flag
        ops.bump_adapter_epoch()

    def load_state_dict(self, state_dict, strict=True, **kw):
        if "rank" in state_dict and int(state_dict["rank"]) != self._rank:
            raise ValueError("these adapters have rank %d, the state dict holds rank %d" % (self._rank, int(state_dict["rank"])))
        if "conv_rank" in state_dict and int(state_dict["conv_rank"]) != self._conv_rank:
            raise ValueError("these adapters have conv rank %d, the state dict holds conv rank %d" % (self._conv_rank, int(state_dict["conv_rank"])))
        if self.merged:
            raise RuntimeError("unmerge() before loading other adapter values: the current ones are folded into the weights")
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._alpha = float(self.alpha)
        if "conv_alpha" in self._buffers:
            self._conv_alpha = float(self.conv_alpha)
        ops.invalidate_packed_weights()
        ops.bump_adapter_epoch()
        return out


def attach(vision_model, rank=16, alpha=None, targets=TARGETS, freeze_base=True, seed=0, conv_targets=(), conv_rank=None,
           conv_alpha=None):
    """-> LoraAdapters for ``vision_model`` (UNet / NestedUNet).  ``alpha=None``: alpha = rank (scale 1).  ``A`` is drawn
    N(0, 1 / Cin) from a CPU generator seeded with ``seed`` in sorted layer-name order, ``B`` is zero: the model's outputs
    are unchanged until the first optimizer step.  ``conv_targets``: a subset of CONV_TARGETS, adapted in every ResNet
    block with rank ``conv_rank`` (default: ``rank``) and scale ``conv_alpha / conv_rank`` (default 1); their ``A`` is
    drawn N(0, 1 / fan_in) behind the attention adapters'.  ``targets=()`` is legal with conv targets."""
    targets = (targets,) if isinstance(targets, str) else tuple(targets)
    conv_targets = (conv_targets,) if isinstance(conv_targets, str) else tuple(conv_targets)
    bad = [t for t in targets if t not in TARGETS]
    if bad or not (targets or conv_targets):
        raise ValueError("LoRA targets must be a non-empty subset of %s, got %r%s" % (
            set(TARGETS), targets, " (the FFN's GELU sits in its first GEMM's epilogue: no adapter there)" if "ffn" in bad else
            " (ResNet convolutions go in conv_targets)" if any(t in CONV_TARGETS for t in bad) else ""))
    bad = [t for t in conv_targets if t not in CONV_TARGETS]
    if bad:
        raise ValueError("LoRA conv targets must be a subset of %s, got %r" % (set(CONV_TARGETS), conv_targets))
    if isinstance(rank, bool) or rank not in RANKS:
        raise ValueError("LoRA rank must be one of %s, got %r" % (RANKS, rank))
    if conv_rank is not None and (isinstance(conv_rank, bool) or conv_rank not in RANKS):
        raise ValueError("LoRA conv rank must be one of %s, got %r" % (RANKS, conv_rank))
    layers = [m for m in vision_model.modules() if isinstance(m, SelfAttention)]
    if targets and not layers:
        raise ValueError("the model has no attention layer to adapt")
    resnets = [m for m in vision_model.modules() if isinstance(m, ResNet)] if conv_targets else []
    if conv_targets and not resnets:
        raise ValueError("the model has no ResNet block to adapt")
    if any(m._lora is not None for m in layers + resnets):
        raise RuntimeError("the model already has adapters attached: detach() them first")
    if targets and any(m._fp8 is not None for m in layers):
        raise RuntimeError("the model's attention layers run in MXFP8 (mdm_hip.fp8): detach() the fp8 handle first, then attach "
                           "and merge() the adapters, then attach fp8 again")
    if any(m._fp8 is not None for m in resnets):
        raise RuntimeError("the model's ResNet convolutions run in MXFP8 (mdm_hip.fp8): detach() the fp8 handle first, then attach "
                           "and merge() the adapters, then attach fp8 again")
    return LoraAdapters(vision_model, rank, rank if alpha is None else alpha, targets, seed, freeze_base, conv_targets, conv_rank,
                        conv_alpha)
