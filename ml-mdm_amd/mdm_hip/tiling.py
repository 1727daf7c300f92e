"""Tiled sampling (MultiDiffusion, Bar-Tal et al., ICML 2023): images larger than the window the denoiser was trained at.

The U-Net has no positional embedding, so a denoiser trained on one window runs on every window of a larger canvas.  Every
reverse step the denoiser runs on overlapping windows of x_t (``gather``), the windows' predictions are averaged where
they overlap (``merge``), and the update runs unchanged on the whole canvas: ``sample(..., tiles=Tiles(window, stride,
blend))``, see ``samplers.SampleOptions``.

Geometry.  Per axis -- canvas L, window win, stride s -- there are n = ceil((L - win) / s) + 1 windows at offsets
o_i = min(i s, L - win): the last one is clamped to the border, so any canvas size works.  The windows form a separable
grid, ny x nx of them; window k = i nx + j, T = ny nx.  1 <= win <= L and 1 <= s <= win, so every pixel lies under a window.
Blend weights are separable and exact in fp32: ``uniform`` is 1; ``ramp`` is min(a + 1, h - a) min(b + 1, w - b) at position
(a, b) of the window, a tent -- and as the sum is normalised by the weights' own sum, canvas borders are not darkened.
Scale i of a nested model (ratio r_i = top side / its side) uses window, stride and canvas divided by r_i; all of them must
be multiples of the largest ratio, so the clamped offsets divide too and the window grid is the same at every scale.

GPU tensors take ``ops.tiles_gather`` / ``ops.tiles_merge`` (one launch per scale each); the functions here are the same
operations in torch ops, for CPU tensors -- the role ``samplers.pag_combine`` plays for perturbed-attention guidance.
"""
import torch

BLENDS = ("uniform", "ramp")


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("Tiles: %s must be an int or a pair (got %r)" % (what, v))
        a, b = v
    else:
        a = b = v
    if int(a) != a or int(b) != b:
        raise ValueError("Tiles: %s must be whole numbers (got %r)" % (what, v))
    return int(a), int(b)


def axis_count(L, win, s):
    """the number of windows along one axis, ceil((L - win) / s) + 1: THE host statement of the count that
    csrc/tiles.hip (tl_axis) computes for itself"""
    return -((win - L) // s) + 1


def axis_offsets(L, win, s):
    """offsets of the windows along one axis: min(i s, L - win) for i < axis_count"""
    return [min(i * s, L - win) for i in range(axis_count(L, win, s))]


class Tiles:
    """``Tiles(window, stride=None, blend="uniform")``: ``window`` an int or (h, w); ``stride`` an int or (sy, sx), default
    half the window per axis (rounded down, at least 1); ``blend`` "uniform" or "ramp".  In pixels of the top scale."""

    def __init__(self, window, stride=None, blend="uniform"):
        h, w = _pair(window, "window")
        if h < 1 or w < 1:
            raise ValueError("Tiles: window must be >= 1 (got %r)" % (window,))
        sy, sx = (max(h // 2, 1), max(w // 2, 1)) if stride is None else _pair(stride, "stride")
        if not (1 <= sy <= h and 1 <= sx <= w):
            raise ValueError("Tiles: stride %r must lie in 1 .. window %r per axis, or pixels between two windows would be "
                             "under none" % ((sy, sx), (h, w)))
        if blend not in BLENDS:
            raise ValueError("Tiles: unknown blend %r (known: %s)" % (blend, ", ".join(BLENDS)))
        self.window, self.stride, self.blend = (h, w), (sy, sx), blend

    def __repr__(self):
        return "Tiles(window=%r, stride=%r, blend=%r)" % (self.window, self.stride, self.blend)

    def graph_key(self):
        """the option's component of a ``GraphedSampler`` key"""
        return ("tiles", self.window, self.stride, self.blend)

    def check(self, H, W, ratios=(1,)):
        """ValueError unless the canvas ``H x W`` can be tiled, at every scale of ``ratios`` (top side / side) -> self"""
        (h, w), (sy, sx) = self.window, self.stride
        if not (h <= H and w <= W):
            raise ValueError("Tiles: window %d x %d is larger than the canvas %d x %d" % (h, w, H, W))
        r = max(ratios)
        if any(v % r for v in (h, w, sy, sx, H, W)):
            raise ValueError("Tiles: window %r, stride %r and canvas %r must all be multiples of the largest nesting ratio %d"
                             % (self.window, self.stride, (H, W), r))
        return self

    def at(self, ratio):
        """the same window grid at a scale ``ratio`` times smaller"""
        if ratio == 1:
            return self
        (h, w), (sy, sx) = self.window, self.stride
        if any(v % ratio for v in (h, w, sy, sx)):
            raise ValueError("Tiles: window %r and stride %r must be multiples of the nesting ratio %d"
                             % (self.window, self.stride, ratio))
        return Tiles((h // ratio, w // ratio), (sy // ratio, sx // ratio), self.blend)

    def offsets(self, H, W):
        """-> (row offsets oy, column offsets ox) of the window grid on a canvas ``H x W``"""
        self.check(H, W)
        return axis_offsets(H, self.window[0], self.stride[0]), axis_offsets(W, self.window[1], self.stride[1])

    def count(self, H, W):
        """T, the number of windows on a canvas ``H x W``"""
        oy, ox = self.offsets(H, W)
        return len(oy) * len(ox)

    def weight(self, dtype=torch.float32, device=None):
        """the blend weights of one window [h, w]: exact integers"""
        h, w = self.window
        if self.blend == "uniform":
            return torch.ones(h, w, dtype=dtype, device=device)
        a, b = torch.arange(h, device=device), torch.arange(w, device=device)
        return (torch.minimum(a + 1, h - a)[:, None] * torch.minimum(b + 1, w - b)[None, :]).to(dtype)


def gather(x, tiles, reps=1):
    """torch ops of ``ops.tiles_gather`` (for CPU tensors): x [B, C, H, W] -> [reps B T, C, h, w]; row (rep B + b) T + k is
    window k of image b"""
    B, C, H, W = x.shape
    oy, ox = tiles.offsets(H, W)
    h, w = tiles.window
    wins = torch.stack([x[:, :, y:y + h, u:u + w] for y in oy for u in ox], dim=1)   # [B, T, C, h, w]
    wins = wins.reshape(B * len(oy) * len(ox), C, h, w)
    return wins if reps == 1 else torch.cat([wins] * reps)


def merge(p, tiles, H, W):
    """torch ops of ``ops.tiles_merge`` (for CPU tensors): p [R T, C, h, w] -> [R, C, H, W], the weighted mean of the windows
    over every pixel, added up in window order; a pixel under one window gets that window's value bit for bit"""
    oy, ox = tiles.offsets(H, W)
    h, w = tiles.window
    T = len(oy) * len(ox)
    if p.dim() != 4 or p.shape[0] % T or tuple(p.shape[2:]) != (h, w):
        raise ValueError("merge: predictions %s are not rows of %d windows of %d x %d" % (tuple(p.shape), T, h, w))
    R, C = p.shape[0] // T, p.shape[1]
    p = p.reshape(R, T, C, h, w)
    wt = tiles.weight(p.dtype, p.device)
    num = p.new_zeros(R, C, H, W)
    one = p.new_zeros(R, C, H, W)    # the plain sum: the value itself where a single window lies over the pixel
    den = p.new_zeros(H, W)
    cnt = p.new_zeros(H, W)
    k = 0
    for y in oy:
        for u in ox:
            num[:, :, y:y + h, u:u + w] += wt * p[:, k]
            one[:, :, y:y + h, u:u + w] += p[:, k]
            den[y:y + h, u:u + w] += wt
            cnt[y:y + h, u:u + w] += 1
            k += 1
    return torch.where(cnt == 1, one, num / den)


def _each(v, T):
    """``v.repeat_interleave(T, dim=0)`` as an expand and a copy: sizes known on the host, capturable"""
    return v.unsqueeze(1).expand(v.shape[0], T, *v.shape[1:]).reshape(v.shape[0] * T, *v.shape[1:])


def cond_rows(T, lm_outputs, lm_mask, micros):
    """the conditioning of a tiled model batch: every row of ``lm_outputs``, ``lm_mask`` and of each per-row tensor of
    ``micros`` once per window, ``T`` times in a row.  -> (lm_outputs, lm_mask, micros)"""
    rows = None if lm_outputs is None else lm_outputs.shape[0]
    per_row = lambda v: torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == rows
    return (None if lm_outputs is None else _each(lm_outputs, T), None if lm_mask is None else _each(lm_mask, T),
            {k: _each(v, T) if per_row(v) else v for k, v in micros.items()})


def time_rows(t, T, reps):
    """the times [B] of a step -> those of the rows [reps B T]"""
    t = _each(t, T)
    return t if reps == 1 else torch.cat([t] * reps)
