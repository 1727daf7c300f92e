"""Perturbed-attention guidance (PAG: Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance",
ECCV 2024) -- which layers are perturbed, and the switch that perturbs them.

PAG evaluates the denoiser once more with the self-attention map of a few ``SelfAttention`` layers replaced by the
identity (every query attends to itself only: softmax(q k^T) v becomes v; the text-cross term stays) and pushes the
prediction away from that degraded one:  p = p_u + w (p_c - p_u) + s (p_c - p_hat).  Here the perturbed evaluation is
a block of extra ROWS of the one model batch -- [uncond | cond | perturbed] -- and a selected layer calls
``ops.attention(..., pag_rows=rows)``: ``mdm_attn_fwd`` on the leading rows, ``mdm_attn_cross_addv`` on the trailing
``rows`` (``ops.attention_pag`` is that call on its own; with a bias or control on the layer, ``ops._attn_blocks``).  The
samplers do the rest (``Sampler.sample(..., pag_scale=s, pag_layers="mid")``, ``GraphedSampler.sample`` alike).
"""
import re

from .unet import SelfAttention, switched

LAYER_SETS = ("mid", "deepest", "all")
_MID = re.compile(r"(^|\.)mid_blocks\.\d+\.attn\.\d+$")
_LEVEL = re.compile(r"^((?:inner_unet\.)*)(down|up)_blocks\.(\d+)\.attn\.\d+$")


def _level_of(vision_model, name):
    """(nesting depth, resolution level) of a down / up attention layer -- larger = lower resolution -- or None"""
    m = _LEVEL.match(name)
    if m is None:
        return None
    depth = m.group(1).count("inner_unet.")
    net = vision_model
    for _ in range(depth):
        net = net.inner_unet
    i = int(m.group(3))
    return depth, i if m.group(2) == "down" else len(net.up_blocks) - 1 - i


def select(vision_model, layers="mid"):
    """-> [(name, module)] of the ``SelfAttention`` layers that ``layers`` names, in ``named_modules()`` order:
    "mid" -- the layers under any ``mid_blocks`` (a nested model: those of its inner U-Net); "deepest" -- the down and up
    layers of the lowest resolution level that has any; "all" -- every one; a list / tuple / set of module names; or a
    predicate on the name.  An empty selection raises ValueError."""
    attn = [(n, m) for n, m in vision_model.named_modules() if isinstance(m, SelfAttention)]
    if callable(layers):
        out = [(n, m) for n, m in attn if layers(n)]
    elif isinstance(layers, str):
        if layers == "mid":
            out = [(n, m) for n, m in attn if _MID.search(n)]
        elif layers == "deepest":
            lv = {n: _level_of(vision_model, n) for n, _ in attn}
            have = [v for v in lv.values() if v is not None]
            out = [(n, m) for n, m in attn if have and lv[n] == max(have)]
        elif layers == "all":
            out = attn
        else:
            raise ValueError("pag_layers = %r (known sets: %s; or a list of module names, or a predicate on the name)"
                             % (layers, ", ".join(LAYER_SETS)))
    else:
        names = list(layers)
        known = dict(attn)
        missing = [n for n in names if n not in known]
        if missing:
            raise ValueError("pag_layers: no SelfAttention layer named %s" % ", ".join(repr(n) for n in missing))
        want = set(names)
        out = [(n, m) for n, m in attn if n in want]
    if not out:
        raise ValueError("pag_layers = %r selects no attention layer of this model (%d SelfAttention layers in all%s)"
                         % (layers, len(attn), "; it has no mid blocks" if layers == "mid" else ""))
    return out


def layer_names(vision_model, layers="mid"):
    """the selection as a tuple of names: hashable, what a graph key holds"""
    return tuple(n for n, _ in select(vision_model, layers))


class perturbed(switched):
    """``with perturbed(vision_model, layers, rows):`` -- inside, the trailing ``rows`` batch rows of every selected layer
    get the identity self-attention map; on exit (also by an exception) every layer has what it had before."""

    def __init__(self, vision_model, layers="mid", rows=0):
        rows = int(rows)
        if rows < 0:
            raise ValueError("perturbed: rows = %d" % rows)
        super().__init__((m, {"_pag_rows": rows}) for _, m in select(vision_model, layers))
