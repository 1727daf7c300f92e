"""Cases shared by the dynamic-threshold quantile tests (CPU and GPU): the definition by a sort, the interpolation ranks from
(n, q) in numpy fp32, the case table and its seeded rows.  Nothing here comes from the package under test.

The definition (``torch.quantile``'s rule): a = |x| sorted ascending, rank = fl32(q) * fl32(n - 1) in fp32, lo = floor(rank),
hi = min(ceil(rank), n - 1), w = rank - lo, quant = w < 0.5 ? a[lo] + w (a[hi] - a[lo]) : a[hi] - (a[hi] - a[lo]) (1 - w),
thr = clamp(quant, cmin, cmax); a row that holds a NaN gives NaN."""
import functools

import numpy as np
import torch

NS = (1, 2, 3, 5, 7, 768, 4099, 12288, 65537)   # scalar and 16-byte paths, one block and several, lo == hi
QS = (0.995, 0.95)
CLAMP = {0.995: (1.0, 100.0), 0.95: (1.0, 1.5)}   # the two dynamic threshold functions
KINDS = (
    "normal",       # random normals x 1.3
    "equal",        # one value everywhere
    "eighths",      # multiples of 1/8: thousands of ties at the selected value
    "two_bins",     # a[lo] = 0.999, a[hi] = 64.0: the two statistics in different level-one bins
    "low8",         # keys that differ only in their lowest 8 bits (level 3 decides)
    "bits8_18",     # keys that differ only in bits 8 .. 18 (level 2 decides)
    "split_mixed",  # a third normals, a third of each of the two above: a row across every level boundary
    "zeros",        # 0.0, -0.0 and denormals
    "small",        # everything below 1: thr = cmin
    "big",          # everything above cmax
    "inf1", "inf2", "nan1",
    "misaligned",   # normals, handed over as x[1:] of an aligned buffer
)
FINITE = tuple(k for k in KINDS if k not in ("inf1", "inf2", "nan1"))


def ranks(n, q):
    """-> (lo, hi, w): the two order statistics and the fp32 weight of the interpolation"""
    rank = np.float32(q) * np.float32(n - 1)
    assert rank.dtype == np.float32
    lo = min(int(np.floor(rank)), n - 1)
    hi = min(int(np.ceil(rank)), n - 1)
    return lo, hi, np.float32(rank - np.floor(rank))


def _bits(t):
    return t.to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def row(kind, n, q):
    """fp32 [n], made once and never written"""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * n + int(q * 1000))
    normal = lambda m=n: torch.randn(m, generator=g) * 1.3
    sign = lambda m=n: torch.randint(0, 2, (m,), generator=g).float() * 2 - 1
    lo, hi, _ = ranks(n, q)
    if kind in ("normal", "misaligned"):
        x = normal()
    elif kind == "equal":
        x = torch.full((n,), 0.7311) * sign()
    elif kind == "eighths":
        x = torch.round(normal() * 8) / 8
    elif kind == "two_bins":
        below = torch.rand(lo + 1, generator=g) * 0.9
        below[0] = 0.999
        above = 64.0 + torch.rand(n - lo - 1, generator=g) * 10
        if above.numel():
            above[0] = 64.0
        x = torch.cat([below, above])[torch.randperm(n, generator=g)] * sign()
    elif kind == "low8":
        x = _bits(0x3F9A3C00 + torch.randint(0, 256, (n,), generator=g)) * sign()
    elif kind == "bits8_18":
        x = _bits(0x3F980000 + torch.randint(0, 2048, (n,), generator=g) * 256 + 0x5A) * sign()
    elif kind == "split_mixed":
        parts = [normal(), _bits(0x3F9A3C00 + torch.randint(0, 256, (n,), generator=g)),
                 _bits(0x3F980000 + torch.randint(0, 2048, (n,), generator=g) * 256 + 0x5A)]
        pick = torch.randint(0, 3, (n,), generator=g)
        x = torch.stack(parts)[pick, torch.arange(n)] * sign()
    elif kind == "zeros":
        den = _bits(torch.randint(1, 0x7FFFFF, (n,), generator=g))
        x = torch.where(torch.rand(n, generator=g) < 0.6, torch.zeros(n), den) * sign()   # the sign makes -0.0 too
    elif kind == "small":
        x = torch.rand(n, generator=g) * 0.9 * sign()
    elif kind == "big":
        x = (200 + torch.rand(n, generator=g) * 50) * sign()
    elif kind in ("inf1", "inf2", "nan1"):
        x = normal()
        pos = torch.randperm(n, generator=g)
        if kind == "nan1":
            x[pos[0]] = float("nan")
        else:
            x[pos[0]] = float("inf")
            if kind == "inf2" and n > 1:
                x[pos[1]] = float("-inf")
    else:
        raise KeyError(kind)
    assert x.dtype == torch.float32 and x.shape == (n,)
    return x


def definition(x, q, cmin, cmax):
    """x fp32 [B, n] on any device -> (stats [B, 2] = (a[lo], a[hi]) bit for bit, thr fp64 [B]: the interpolation evaluated
    in fp64 from those two and the fp32 weight, clamped; NaN for a row that holds one)"""
    a = x.abs().sort(dim=1).values
    lo, hi, w = ranks(a.shape[1], q)
    stats = torch.stack([a[:, lo], a[:, hi]], dim=1)
    alo, ahi, w = stats[:, 0].double(), stats[:, 1].double(), float(w)
    d = ahi - alo
    quant = alo + w * d if w < 0.5 else ahi - d * (1 - w)
    thr = quant.clamp(min=cmin, max=cmax)
    thr = torch.where(a[:, -1].isnan(), torch.full_like(thr, float("nan")), thr)   # NaN sorts last
    return stats, thr


@functools.lru_cache(maxsize=None)
def expected(kind, n, q):
    """``definition`` of ``row(kind, n, q)`` with the clamp of q's threshold function, on the CPU, made once"""
    return definition(row(kind, n, q)[None], q, *CLAMP[q])


def bits_differ(a, b):
    """number of elements whose bit patterns differ"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())


def ulps_off(got, want64):
    """|got - want| in units of fp32's spacing at want, elementwise; 0 where both are NaN or both the same infinity"""
    got, want64 = got.detach().cpu().double(), want64.detach().cpu().double()
    same = (got == want64) | (got.isnan() & want64.isnan())
    spacing = torch.from_numpy(np.spacing(np.abs(want64.numpy()).astype(np.float32)).astype(np.float64))
    off = (got - want64).abs() / spacing
    off = torch.where(off.isnan(), torch.full_like(off, float("inf")), off)
    return torch.where(same, torch.zeros_like(off), off)
