"""CPU: the dynamic-threshold quantile -- the rule restated (``samplers.dynamic_threshold_ref`` and the definition of
tests/thr_cases.py) against ``torch.quantile`` bit for bit, the C entries' argument checks (nothing is launched), and the CPU
path of the samplers on a row longer than ``torch.quantile`` takes."""
import ctypes

import pytest
import torch

import thr_cases as TH


@pytest.mark.parametrize("kind", TH.FINITE)
def test_restatement_is_torch_quantile_bit_for_bit(kind):
    from mdm_hip import samplers as S

    for n in TH.NS:
        for q in TH.QS:
            x = TH.row(kind, n, q)[None]
            cmin, cmax = TH.CLAMP[q]
            want = torch.quantile(x.abs(), q, dim=1)
            stats, thr64 = TH.expected(kind, n, q)
            lo, hi, w = TH.ranks(n, q)
            # the definition's two order statistics and weight through torch.lerp (whose product may be fused): every bit;
            # its fp64 evaluation: the three roundings of the fp32 form
            mine = torch.lerp(stats[:, 0], stats[:, 1], torch.tensor(w))
            assert TH.bits_differ(mine, want) == 0, (kind, n, q)
            assert TH.bits_differ(S.dynamic_threshold_ref(x, q, cmax), want.clamp(min=cmin, max=cmax)) == 0, (kind, n, q)
            assert float(TH.ulps_off(want.clamp(min=cmin, max=cmax), thr64).max()) <= 2


@pytest.mark.parametrize("kind", ["inf1", "inf2", "nan1"])
def test_restatement_on_inf_and_nan_rows(kind):
    """NaN rows give NaN; infinities are ordinary largest values and the interpolation is applied as written"""
    from mdm_hip import samplers as S

    for n in TH.NS:
        for q in TH.QS:
            x = TH.row(kind, n, q)[None]
            got = S.dynamic_threshold_ref(x, q, TH.CLAMP[q][1])
            want = torch.quantile(x.abs(), q, dim=1).clamp(min=1, max=TH.CLAMP[q][1])
            assert torch.equal(got.isnan(), want.isnan()) and TH.bits_differ(got.nan_to_num(0.0), want.nan_to_num(0.0)) == 0
            _, thr64 = TH.expected(kind, n, q)
            assert torch.equal(thr64.isnan(), want.isnan()), (kind, n, q)
            if kind == "nan1":
                assert bool(got.isnan().all())


def test_ranks_are_fp32():
    """the fp32 rank is part of the rule: at n = 3 * 1024^2 it gives the weight 0.5 where fp64 gives 0.365; above 2^24 it
    is an integer"""
    lo, hi, w = TH.ranks(3 * 1024 * 1024, 0.995)
    assert hi == lo + 1 and float(w) == 0.5
    assert abs(0.995 * (3 * 1024 * 1024 - 1) % 1 - 0.365) < 1e-3
    for n in (2 ** 24 + 4, 3 * 2048 * 3072):
        for q in TH.QS:
            lo, hi, w = TH.ranks(n, q)
            assert lo == hi and float(w) == 0.0


def test_entries_are_declared_and_refuse_bad_arguments():
    from mdm_hip import _lib

    assert _lib.ABI_VERSION == 6 and "quantile.hip" in _lib.SOURCES
    ext = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert ext["mdm_abs_quantile_plan"][1] == ["B", "n", "ws_bytes"]
    assert ext["mdm_abs_quantile"][1] == ["x", "ws", "ws_bytes", "B", "n", "q", "cmin", "cmax", "thr", "stats", "stream"]
    assert ext["mdm_abs_quantile"][0][4] is ctypes.c_size_t and ext["mdm_abs_quantile"][0][5] is ctypes.c_float
    L = _lib.lib()
    err = lambda: (L.mdm_last_error() or b"").decode()
    # the plan: host-only, positive, a function of B alone, and it refuses what the entry refuses
    ws = ctypes.c_size_t(0)
    plan = lambda B, n: L.mdm_abs_quantile_plan(B, n, ctypes.byref(ws))
    assert plan(1, 1) == 0 and ws.value > 0
    one = ws.value
    assert plan(4, 3 * 1024 * 1024) == 0 and ws.value == 4 * one
    assert plan(1, 2 ** 31 - 1) == 0 and ws.value == one
    assert plan(1, 0) < 0 and "n >= 1" in err()
    assert plan(1, 2 ** 31) < 0 and "n >= 1" in err()
    assert plan(0, 8) < 0 and "B >= 1" in err()
    assert plan(65536, 8) < 0 and "B >= 1" in err()
    assert L.mdm_abs_quantile_plan(1, 8, None) < 0 and "ws_bytes" in err()
    # the entry: made-up pointers that are never followed -- every call is refused before a launch
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    x, wsp, thr, stats = (ctypes.c_void_p(base + 256 * k) for k in range(4))
    good = dict(x=x, ws=wsp, ws_bytes=one, B=1, n=64, q=0.95, cmin=1.0, cmax=1.5, thr=thr, stats=stats, stream=None)
    call = lambda **kw: L.mdm_abs_quantile(*[dict(good, **kw)[k] for k in ext["mdm_abs_quantile"][1]])
    for kw, needle in ((dict(n=0), "n >= 1"), (dict(n=2 ** 31), "n >= 1"), (dict(thr=None), "thr"), (dict(x=None), "x != "),
                       (dict(ws=None), "ws != "), (dict(ws_bytes=one - 1), "ws_bytes"), (dict(B=2), "ws_bytes"),
                       (dict(q=-0.01), "q >= 0"), (dict(q=1.01), "q >= 0"), (dict(q=float("nan")), "q >= 0"),
                       (dict(B=0), "B >= 1"), (dict(cmin=2.0), "cmin <= cmax"), (dict(cmin=float("nan")), "cmin <= cmax"),
                       (dict(ws=ctypes.c_void_p(base + 8)), "ws"), (dict(x=ctypes.c_void_p(base + 2)), "x")):
        assert call(**kw) < 0, kw
        assert needle in err() and "quantile.hip" in err(), (kw, err())


def test_ops_abs_quantile_has_no_cpu_fallback():
    from mdm_hip import _lib, ops

    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.abs_quantile(torch.randn(2, 12), 0.95)


# ---- rows longer than torch.quantile takes ----------------------------------------------------------------------------------
N_LONG = 2 ** 24 + 4


def test_cpu_path_has_no_row_limit():
    """``torch.quantile`` raises on this row; the samplers' CPU path returns the rule's value (lo == hi above 2^24: one order
    statistic, found here by ``torch.kthvalue``).  Two sorts of 16.8 M floats: seconds."""
    from mdm_hip import samplers as S

    q, vmax = 0.95, 1.5
    x = torch.randn(1, N_LONG, generator=torch.Generator().manual_seed(5)) * 0.7
    with pytest.raises(RuntimeError, match="too large"):
        torch.quantile(x.abs(), q, dim=1)
    lo, hi, w = TH.ranks(N_LONG, q)
    assert lo == hi and w == 0
    want = x.abs().kthvalue(lo + 1, dim=1).values
    assert 1 < float(want) < vmax   # the clamp is not what is compared
    smp = S.Sampler(S.SamplerConfig(num_diffusion_steps=8, threshold_function="DYNAMIC_IF"))
    thr = smp._dynamic_thr(x.reshape(1, 1, 2, N_LONG // 2))
    assert thr.shape == (1,) and TH.bits_differ(thr, want) == 0
    got = smp.clip_sample(x, 1)
    assert TH.bits_differ(got, torch.clamp(x, -want[:, None], want[:, None]) / want[:, None]) == 0
