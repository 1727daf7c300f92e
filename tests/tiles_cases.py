"""Cases shared by the tiled-sampling tests (CPU and GPU): the fp64 definition of the window gather and of the weighted merge,
written as slice accumulation into numerator and denominator canvases over window offsets found by stepping along the axis
(nothing of the kernels' covering arithmetic), the case table, seeded inputs, and two stub denoisers -- a pointwise one, for
which tiled and untiled sampling must agree, and a recording one."""
import functools

import torch

import pag_cases as PG

# (B, H, W, h, w, sy, sx)
CASES = [
    (1, 2, 2, 2, 2, 1, 1),         # one window
    (2, 5, 7, 3, 4, 2, 3),         # odd sizes, scalar path, clamped on both axes
    (3, 16, 36, 16, 16, 8, 8),     # vector path, last offset clamped to 20
    (2, 16, 40, 16, 16, 6, 6),     # w % 4 == 0 but offsets not multiples of 4
    (1, 8, 8, 4, 4, 1, 1),         # 25 windows, up to 16 covering one pixel
    (1, 64, 160, 64, 64, 32, 32),  # the bench shape
    (2, 32, 56, 32, 32, 16, 16),   # the nested top scale, clamped to 24
    (1, 32, 32, 16, 16, 8, 8),     # vector path with windows overlapping along both axes (3 x 3, up to 4 over a pixel)
]
# the window offsets (rows, columns) of every case, written out
OFFSETS = {
    CASES[0]: ([0], [0]),
    CASES[1]: ([0, 2], [0, 3]),
    CASES[2]: ([0], [0, 8, 16, 20]),
    CASES[3]: ([0], [0, 6, 12, 18, 24]),
    CASES[4]: ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),
    CASES[5]: ([0], [0, 32, 64, 96]),
    CASES[6]: ([0], [0, 16, 24]),
    CASES[7]: ([0, 8, 16], [0, 8, 16]),
}
TABLE = CASES[:7]   # the table the feature was specified with; the cases after it were added for paths it leaves out
REPS = (1, 3)
BLENDS = ("uniform", "ramp")
C = 3


def case_id(case):
    return "B%d-%dx%d-win%dx%d-stride%dx%d" % case


def axis_offsets(L, win, s):
    """step along the axis by ``s`` until a window reaches the border; that one is pushed back inside"""
    out, o = [], 0
    while o + win < L:
        out.append(o)
        o += s
    out.append(L - win)
    return out


def window_offsets(case):
    """-> [(oy, ox)] of window k, in order"""
    _, H, W, h, w, sy, sx = case
    return [(y, x) for y in axis_offsets(H, h, sy) for x in axis_offsets(W, w, sx)]


def weight(h, w, blend):
    """fp64 [h, w]"""
    if blend == "uniform":
        return torch.ones(h, w, dtype=torch.float64)
    wy = torch.tensor([min(a + 1, h - a) for a in range(h)], dtype=torch.float64)
    wx = torch.tensor([min(b + 1, w - b) for b in range(w)], dtype=torch.float64)
    return wy[:, None] * wx[None, :]


def gather_ref(x, case, reps):
    """x [B, C, H, W] -> [reps B T, C, h, w] (the dtype of x: copies)"""
    _, H, W, h, w, _, _ = case
    wins = torch.stack([x[:, :, y:y + h, u:u + w] for y, u in window_offsets(case)], dim=1)
    return torch.cat([wins.reshape(-1, x.shape[1], h, w)] * reps)


def merge_ref(p, case, blend):
    """p [R T, C, h, w] -> (fp64 [R, C, H, W], the number of windows over every pixel [H, W])"""
    _, H, W, h, w, _, _ = case
    offs = window_offsets(case)
    T = len(offs)
    p = p.double().reshape(-1, T, p.shape[1], h, w)
    num = torch.zeros(p.shape[0], p.shape[2], H, W, dtype=torch.float64)
    den = torch.zeros(H, W, dtype=torch.float64)
    count = torch.zeros(H, W, dtype=torch.long)
    wt = weight(h, w, blend)
    for k, (y, u) in enumerate(offs):
        num[:, :, y:y + h, u:u + w] += wt * p[:, k]
        den[y:y + h, u:u + w] += wt
        count[y:y + h, u:u + w] += 1
    return num / den, count


def merge_gate(n_cover):
    """max-abs error over max |p|: each product, each sum, each of the two accumulators and the division round once at
    2^-24; the gate doubles that"""
    return (n_cover + 3) * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def inputs(case, reps):
    """-> (canvas x [B, C, H, W], predictions p [reps B T, C, h, w]) fp32, made once and never written"""
    B, H, W, h, w, _, _ = case
    g = torch.Generator().manual_seed(sum(v * 7 ** i for i, v in enumerate(case)) + reps)
    T = len(window_offsets(case))
    return torch.randn(B, C, H, W, generator=g), torch.randn(reps * B * T, C, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def merged(case, reps, blend):
    """the fp64 merge of ``inputs(case, reps)[1]`` -> (out, count)"""
    return merge_ref(inputs(case, reps)[1], case, blend)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ---- stub denoisers ----------------------------------------------------------------------------------------------------
class PointwiseStub(torch.nn.Module):
    """``model(x, t, lm_outputs, lm_mask, micros)`` as the samplers call it, with pred = f(x_t, t) elementwise plus a shift
    per row from its conditioning: no pixel sees another, so the prediction of a pixel is the same in every window that
    holds it and tiled sampling must reproduce untiled sampling.  ``nested``: two scales at ratio 2."""

    def __init__(self, nested=False):
        super().__init__()
        self.nested = nested
        self.nest_ratio = [2]
        self.calls = 0

    @property
    def vision_model(self):
        return self

    @staticmethod
    def one(x, t, lm, k):
        c = lm.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        tt = (t.float() / 1000.0).reshape(-1, 1, 1, 1)
        return (0.3 + 0.1 * k) * x + 0.2 * torch.sin(2 * x) * tt + 0.1 * torch.tanh(3 * tt) + 0.4 * c

    def forward(self, x, t, lm, mask, micros={}):
        self.calls += 1
        if self.nested:
            return [self.one(v, t, lm, k) for k, v in enumerate(x)]
        out = self.one(x, t, lm, 0)
        return out, torch.ones_like(out)


RecordingStub = PG.RecordingStub   # records x, t, lm, mask, micros and the perturbed rows of every call
