"""FreeU (Si, Liu, Huang, Liu, "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024) -- which up blocks it acts on, and the
switch that turns it on.

At the decoder's low-resolution stages FreeU amplifies half of the backbone channels (factor ``b``; with
``structure=True``, FreeU v2, by 1 + (b - 1) hm with hm the min-max normalised channel mean of the backbone) and damps the
lowest spatial frequencies of the skip features (factor ``s`` on the 2 x 2 centre of the shifted spectrum), just before the
two are concatenated.  Here that concat is ``ops.concat`` in ``ResNetBlock.forward``; a selected block calls
``ops.concat_freeu`` instead (two launches: statistics, then the concat with both transforms fused).  No extra model
evaluation.  The samplers do the rest (``Sampler.sample(..., freeu=FreeU(b=(b1, b2), s=(s1, s2)))``,
``GraphedSampler.sample`` alike).

No default values for ``b`` and ``s``: the published ones belong to Stable Diffusion's U-Nets and do not transfer.
"""
import math

from .unet import ResNetBlock, switched

LEVEL_SETS = ("deepest2",)


def _pair(v, what):
    try:
        a, b = v
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError("FreeU: %s = %r (wanted a pair of numbers)" % (what, v))


def _check_b(b, where):
    if not (math.isfinite(b) and b > 0):
        raise ValueError("FreeU: b = %r%s (wanted a finite number > 0)" % (b, where))


def _check_s(s, where):
    if not (math.isfinite(s) and s >= 0):
        raise ValueError("FreeU: s = %r%s (wanted a finite number >= 0)" % (s, where))


class FreeU:
    """``FreeU(b=(b1, b2), s=(s1, s2), structure=False, levels="deepest2")``.

    ``levels="deepest2"``: index 0 of ``b`` / ``s`` goes to the lowest-resolution up block that concatenates skips, index 1
    to the next one (a nested model: blocks of its innermost U-Net).  ``levels={up-block module name: (b, s)}`` names the
    blocks instead; ``b`` and ``s`` are then not given.  ``structure=True``: FreeU v2's structure-aware backbone scale.
    The cut-off of the Fourier filter is the paper's ``threshold = 1``; no other is implemented."""

    def __init__(self, b=None, s=None, structure=False, levels="deepest2", threshold=1):
        if threshold != 1:
            raise ValueError("FreeU: threshold = %r (only the paper's cut-off 1 is implemented)" % (threshold,))
        self.structure = bool(structure)
        if isinstance(levels, dict):
            if b is not None or s is not None:
                raise ValueError("FreeU: levels as a dict carries (b, s) per block; b= and s= are not given beside it")
            self.levels = {str(k): _pair(v, "levels[%r]" % (k,)) for k, v in levels.items()}
            self.b = self.s = None
        elif levels in LEVEL_SETS:
            if b is None or s is None:
                raise ValueError("FreeU: b= and s= are required (no defaults: Stable Diffusion's values do not transfer)")
            self.levels, self.b, self.s = levels, _pair(b, "b"), _pair(s, "s")
        else:
            raise ValueError("FreeU: levels = %r (known sets: %s; or a dict {up-block module name: (b, s)})"
                             % (levels, ", ".join(LEVEL_SETS)))
        self.validate()

    def validate(self):
        pairs = self.levels.items() if isinstance(self.levels, dict) else enumerate(zip(self.b, self.s))
        for k, (b, s) in pairs:
            _check_b(b, " at %r" % (k,))
            _check_s(s, " at %r" % (k,))

    def __repr__(self):
        if isinstance(self.levels, dict):
            return "FreeU(levels=%r, structure=%r)" % (self.levels, self.structure)
        return "FreeU(b=%r, s=%r, structure=%r, levels=%r)" % (self.b, self.s, self.structure, self.levels)


def up_blocks(vision_model):
    """[(name, module)] of every up-path ``ResNetBlock`` (the blocks that concatenate skips), in ``named_modules()`` order"""
    return [(n, m) for n, m in vision_model.named_modules()
            if isinstance(m, ResNetBlock) and n.rsplit(".", 2)[-2:-1] == ["up_blocks"]]


def select(vision_model, cfg):
    """-> [(name, module, b, s)] of the up blocks ``cfg`` acts on, lowest resolution first for "deepest2", in
    ``named_modules()`` order for a dict.  An unknown name, an empty selection and a parameter out of range raise
    ValueError."""
    if not isinstance(cfg, FreeU):
        raise ValueError("freeu = %r (wanted a mdm_hip.FreeU)" % (cfg,))
    cfg.validate()
    if isinstance(cfg.levels, dict):
        known = dict(up_blocks(vision_model))
        missing = [n for n in cfg.levels if n not in known]
        if missing:
            raise ValueError("FreeU: no up block named %s (up blocks: %s)"
                             % (", ".join(repr(n) for n in missing), ", ".join(known) or "none"))
        out = [(n, m) + cfg.levels[n] for n, m in known.items() if n in cfg.levels]
    else:
        net, prefix = vision_model, ""
        while getattr(net, "inner_unet", None) is not None:
            net, prefix = net.inner_unet, prefix + "inner_unet."
        blocks = [m for m in getattr(net, "up_blocks", []) if isinstance(m, ResNetBlock) and m.num_residual_blocks > 0]
        names = {id(m): n for n, m in net.named_modules()}
        out = [(prefix + names[id(m)], m, cfg.b[i], cfg.s[i]) for i, m in enumerate(blocks[:2])]
    if not out:
        raise ValueError("FreeU: %r selects no up block of this model" % (cfg,))
    return out


def graph_key(vision_model, cfg):
    """("freeu", names, b's, s's, structure): hashable, what a graph key holds"""
    sel = select(vision_model, cfg)
    return ("freeu", tuple(n for n, _, _, _ in sel), tuple(b for _, _, b, _ in sel), tuple(s for _, _, _, s in sel),
            cfg.structure)


class applied(switched):
    """``with applied(vision_model, cfg):`` -- inside, the selected up blocks concatenate through ``ops.concat_freeu``; on
    exit (also by an exception) every block has what it had before."""

    def __init__(self, vision_model, cfg):
        super().__init__((m, {"_freeu": (b, s, cfg.structure), "_freeu_name": n}) for n, m, b, s in select(vision_model, cfg))


__all__ = ["FreeU", "select", "applied", "graph_key", "up_blocks"]
