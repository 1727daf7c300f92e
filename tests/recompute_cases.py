"""Cases and helpers shared by tests/test_recompute_host.py and tests/test_recompute_gpu.py (activation recomputation:
``mdm_gn_reapply`` + ``ops.gn_conv`` + ``ops.enable_activation_recompute``).

Which forward kernel family ``mdm_gn_fwd`` takes is decided by ``gn_fused_cfg`` in csrc/norm.hip: the single-kernel ("fused")
family when a group is whole 16-byte chunks (cpg % EPV == 0, EPV = 8 bf16 / 4 fp32), no wider than 64 channels, and the image
fits the register passes (HW <= 1024 in bf16, <= 512 in fp32); the partial -> apply ("split") family otherwise.  The table
names the family per dtype; `family()` recomputes the rule so that a case cannot drift from its label unnoticed.
"""
import torch

# (N, H, W, C, G, family in bf16, family in fp32)
KERNEL_CASES = [
    (2, 4, 4, 32, 8, "split", "fused"),       # cpg = 4: half a bf16 chunk, one fp32 chunk
    (2, 5, 7, 96, 32, "split", "split"),      # odd pixel count, 3 channels per group
    (1, 64, 64, 64, 32, "split", "split"),    # cpg = 2; 4096 pixels: several pixel splits and trips of the store loop
    (2, 6, 6, 64, 8, "fused", "fused"),       # cpg = 8: the single-kernel family in both dtypes, 36 pixels (a partial trip)
    (2, 16, 16, 768, 32, "fused", "fused"),   # a shipped shape (cpg = 24): 3 channel slices of 32 chunk columns in bf16
    (1, 40, 40, 64, 4, "split", "split"),     # cpg = 16 but 1600 pixels: past the register passes of either dtype
    (3, 3, 5, 40, 5, "fused", "fused"),       # cpg = 8, 5 bf16 / 10 fp32 chunk columns (no power of two), 15 pixels, N = 3
]
DROPOUT_P = 0.1
# with dropout the element count must be a multiple of 8 (mdm_dropout's rule): every case above but none by accident
DROPOUT_CASES = [c for c in KERNEL_CASES if (c[0] * c[1] * c[2] * c[3]) % 8 == 0]

# the fused function against the composed stored path: (H, W, Cin, Cout, G); N = 2 throughout (a two-term atomic sum of
# dgamma / dbeta is order-independent)
FUNCTION_CASES = [(8, 8, 32, 32, 8), (6, 10, 32, 64, 8), (8, 8, 64, 32, 32), (6, 10, 64, 64, 8)]


def family(HW, C, G, dtype):
    """the dispatch rule of gn_fused_cfg (csrc/norm.hip), forward direction"""
    epv, lpr = (4, 16) if dtype == torch.float32 else (8, 8)
    cpg = C // G
    if cpg % epv != 0 or cpg > lpr * epv:
        return "split"
    return "fused" if HW <= 8 * (1024 // lpr) else "split"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def kernel_inputs(N, H, W, C, G, dtype, film, seed=0):
    g = gen(1000 * seed + N + 7 * H + 13 * W + C + G)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).to(dtype)
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g) * 0.5
    fl = (torch.randn(N, 2 * C, generator=g) * 0.5).to(dtype) if film else None
    return x, gamma, beta, fl


def gn_fwd_raw(x, gamma, beta, film, G, act, eps=1e-5):
    """mdm_gn_fwd through the C ABI -> (y, coef)"""
    from mdm_hip import _lib, ops

    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    y = torch.empty_like(x)
    stats = torch.empty((N, G, 2), dtype=torch.float32, device=x.device)
    coef = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
    ws = ops._gn_ws(N, HW, C, G, x.device)
    _lib.check(_lib.lib().mdm_gn_fwd(ops._p(x), ops._p(gamma), ops._p(beta), ops._p(film), ops._p(y), ops._p(stats), ops._p(coef),
                                     ops._p(ws), N, HW, C, G, eps, act, ops._dt(x), ops._stream()), "mdm_gn_fwd")
    return y, coef


def dropout_raw(x, p, seed, off):
    from mdm_hip import _lib, ops

    y = torch.empty_like(x)
    _lib.check(_lib.lib().mdm_dropout(ops._p(x), ops._p(y), x.numel(), p, seed, off, ops._dt(x), ops._stream()), "mdm_dropout")
    return y


def ndiff(a, b):
    """elements that differ in any bit"""
    assert a.shape == b.shape and a.dtype == b.dtype
    ia = a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16)
    ib = b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16)
    return int((ia != ib).sum())


class count_gn_conv:
    """context: counts the calls of ops.gn_conv and the bytes of the convolution inputs they do not keep"""

    def __enter__(self):
        from mdm_hip import ops

        self.calls, self.bytes, self._orig = 0, 0, ops.gn_conv

        def wrapped(x, *a, **kw):
            self.calls += 1
            self.bytes += x.numel() * x.element_size()
            return self._orig(x, *a, **kw)

        ops.gn_conv = wrapped
        return self

    def __exit__(self, *exc):
        from mdm_hip import ops

        ops.gn_conv = self._orig
        return False


class recompute:
    """context: the switch set to ``flag``, restored afterwards"""

    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        from mdm_hip import ops

        self.prev = ops.activation_recompute_enabled()
        ops.enable_activation_recompute(self.flag)

    def __exit__(self, *exc):
        from mdm_hip import ops

        ops.enable_activation_recompute(self.prev)
        return False
