"""Low-rank adapters (LoRA, Hu et al. 2021) for the attention projections of a UNet / NestedUNet on the HIP path.

    y = W x + b + (alpha / r) B (A x)        A [r, Cin], B [Cout, r] trainable; W, b frozen

``attach(vision_model, rank=16)`` adapts the ``qkv``, ``kv_cond`` and ``proj_out`` projections of every ``SelfAttention``
layer (inner nets of a nested model included) and returns a ``LoraAdapters`` module that owns the new parameters.  The
adapters are NOT part of the vision model's module tree: ``vision_model.state_dict()`` / ``save()`` / ``load()`` keep the
reference's keys and shapes; a layer finds its adapters through the plain attribute ``SelfAttention._lora``.  The adapter
term runs in kernels of its own (``csrc/lora.hip``: ``ops.lora``) right behind the base projection's launch.
``merge()`` folds ``s B A`` into the fp32 master weights -- sampling then costs nothing extra and the checkpoint is a plain
reference checkpoint -- and ``unmerge()`` takes it out again.  Training keeps the term separate: a bf16 copy of
``W + s B A`` would round small updates away.

The reference has no counterpart.  Not covered: 3x3 convolutions, the FFN (its GELU sits in the first GEMM's epilogue),
dropout on the adapter path, per-layer ranks, ``ModelEma`` tracking, the fused train step and
``mdm_hip.distributed.DataParallel`` (``trainer.train_batch`` takes its plain path for an optimizer over adapters).
"""
import math

import torch
import torch.nn as nn

from . import ops
from .unet import SelfAttention

TARGETS = ("qkv", "kv_cond", "proj_out")
RANKS = (4, 8, 16, 32, 64)


class _LayerAdapters:
    """what one SelfAttention layer sees of its adapters (a plain object: nothing registers in the layer's module tree)"""

    __slots__ = ("owner", "pairs")

    def __init__(self, owner):
        self.owner, self.pairs = owner, {}

    def active(self, target):
        return target in self.pairs and not self.owner.merged

    def apply(self, target, y, x):
        """y (the base projection's fresh output) with the adapter term of ``target`` added in place; x: the projection's input"""
        if not self.active(target):
            return y
        a, b = self.pairs[target]
        return ops.lora(y, x, a, b, self.owner.scale)


class _Node(nn.Module):
    pass


class LoraAdapters(nn.Module):
    """The adapter parameters of one vision model: ``<layer name>.<target>.lora_A`` / ``.lora_B`` (fp32, on the device of
    the base weight), plus ``rank`` and ``alpha`` in the state dict."""

    def __init__(self, vision_model, rank, alpha, targets, seed, freeze_base):
        super().__init__()
        self._rank, self._alpha = int(rank), float(alpha)
        self.register_buffer("rank", torch.tensor(self._rank, dtype=torch.int64))
        self.register_buffer("alpha", torch.tensor(self._alpha, dtype=torch.float64))
        self.targets = tuple(t for t in TARGETS if t in targets)
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
                node = self
                for part in (name + "." + target).split("."):
                    if part not in node._modules:
                        node.add_module(part, _Node())
                    node = node._modules[part]
                node.lora_A, node.lora_B = a, b
                handle.pairs[target] = (a, b)
                self._entries.append((name, layer, target, base, a, b))
            layer._lora = handle
        if not self._entries:
            for _, layer in layers:
                layer._lora = None
            raise ValueError("none of the targets %r exists in this model's attention layers" % (self.targets,))
        self._found = [(p, p.requires_grad) for p in vision_model.parameters()]
        if freeze_base:
            for p, _ in self._found:
                p.requires_grad = False
        ops.bump_adapter_epoch()

    @property
    def scale(self):
        return self._alpha / self._rank

    def _fold(self, sign):
        with torch.no_grad():
            for _, _, _, base, a, b in self._entries:
                w = base.weight.detach()
                # W [Cout, Cin] += (+-s) B A on the fp32 master: t = B [Cout, r], b = A^T [Cin, r]
                ops.lora_up_add(w.view(w.shape[0], w.shape[1]), b.detach().contiguous(), a.detach().t().contiguous(), sign * self.scale)
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
        if self.merged:
            raise RuntimeError("unmerge() before loading other adapter values: the current ones are folded into the weights")
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._alpha = float(self.alpha)
        ops.invalidate_packed_weights()
        ops.bump_adapter_epoch()
        return out


def attach(vision_model, rank=16, alpha=None, targets=TARGETS, freeze_base=True, seed=0):
    """-> LoraAdapters for ``vision_model`` (UNet / NestedUNet).  ``alpha=None``: alpha = rank (scale 1).  ``A`` is drawn
    N(0, 1 / Cin) from a CPU generator seeded with ``seed`` in sorted layer-name order, ``B`` is zero: the model's outputs
    are unchanged until the first optimizer step."""
    targets = (targets,) if isinstance(targets, str) else tuple(targets)
    bad = [t for t in targets if t not in TARGETS]
    if bad or not targets:
        raise ValueError("LoRA targets must be a non-empty subset of %s, got %r%s" % (
            set(TARGETS), targets, " (the FFN's GELU sits in its first GEMM's epilogue: no adapter there)" if "ffn" in bad else ""))
    if isinstance(rank, bool) or rank not in RANKS:
        raise ValueError("LoRA rank must be one of %s, got %r" % (RANKS, rank))
    layers = [m for m in vision_model.modules() if isinstance(m, SelfAttention)]
    if not layers:
        raise ValueError("the model has no attention layer to adapt")
    if any(m._lora is not None for m in layers):
        raise RuntimeError("the model already has adapters attached: detach() them first")
    return LoraAdapters(vision_model, rank, rank if alpha is None else alpha, targets, seed, freeze_base)
