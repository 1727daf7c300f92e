"""The variant ledger (tests/conv_variant_cases.py) and its gates, checked without a GPU: the integer operands keep every
partial sum below 2^24, a CPU emulation of the kernels' arithmetic stays inside the derived random-data bound on every
row, the gates catch planted defects (and the old max-error gate of tests/test_ops_gpu.py does not catch all of them),
every declared edge holds arithmetically, and every kernel-name format of gemm_conv.hip has a row."""
import ctypes
import os
import re

import pytest
import torch

import conv_variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256   # what device_cus() assumes without a GPU
# rows whose fp64 reference takes seconds: the host emulation covers them at a smaller batch / image of the same geometry
LARGE = {"bl128p_1x1_fwd", "bl128p_3x3_fwd", "bl256p_1x1_fwd", "bl256p_3x3_fwd", "direct_32_32", "direct_32_64", "direct_64_32",
         "direct_64_64", "direct_64_32_dgrad", "wgrad_direct"}


def _host_row(row):
    """the row itself, or (LARGE) a copy with the same channels and kernel size on a 2 x 16 x 24 image: the arithmetic of
    the gate does not depend on which kernel runs"""
    if row.id not in LARGE:
        return row
    N, H, W, Cin, Cout, ks, stride = row.dims(CUS)
    small = V.Row(row.id, row.entry, (2, 16, 24, Cin, Cout, ks, stride), row.name, row.edges, row.knobs, res=row.res, bias=row.bias,
                  groups=row.groups, round_once=row.round_once, wgrid=row.wgrid, a_factor=row.a_factor)
    return small


@pytest.mark.parametrize("row", V.ROWS, ids=repr)
def test_integer_operands_stay_below_2_24(row):
    """... at the row's FULL shape for the magnitudes (cheap bound: largest |x| * largest |w| * reduction length + bias)
    and exactly, from the fp64 sums of absolute products, at the host shape"""
    N, H, W, Cin, Cout, ks, stride = row.dims(CUS)
    L = V.reduction_length(row, CUS)
    assert L * 3 * 3 + 11 + 9 < V.INT_LIMIT, (row, L)
    hr = _host_row(row)
    for kind in ("int", "impulse"):
        for g in range(row.groups):
            o = V.operands(hr, kind, CUS, g)
            for t in (o["x"], o["w"], o["dy"], o["b"], o["res"]):
                assert t is None or bool((t == t.round()).all())
            assert float(o["x"].abs().max()) <= 3 and float(o["w"].abs().max()) <= 3 and float(o["dy"].abs().max()) <= 3
            exp = V.reference(hr, o, CUS)
            assert V.int_condition(exp) < V.INT_LIMIT
    o = V.operands(hr, "int", CUS)
    assert 0.35 < float((o["x"] == 0).double().mean()) < 0.75      # roughly half the activations are zero


@pytest.mark.parametrize("row", V.ROWS, ids=repr)
def test_cpu_emulation_is_exact_on_integers_and_within_the_bound(row):
    hr = _host_row(row)
    for g in range(row.groups):
        for kind in ("int", "impulse"):
            o = V.operands(hr, kind, CUS, g)
            exp = V.reference(hr, o, CUS)
            got = V.emulate(hr, o)
            for k, e in exp.items():
                assert V.int_mismatches(got[k], V.int_expected(hr, e)) == 0, (row, kind, k)
        o = V.operands(hr, "random", CUS, g)
        exp = V.reference(hr, o, CUS)
        got = V.emulate(hr, o)
        for k, e in exp.items():
            worst, over = V.bound_ratio(got[k], e)
            print("%s group %d %s: worst |got - ref| / bound = %.3g" % (row.id, g, k, worst))
            assert over == 0 and worst <= 1.0, (row, k, worst, over)
            if e.is_bf16:
                assert worst > 0.05, "a bound that loose would gate nothing"


def _tile(row):
    """(row-tile edge, column-tile edge) of the output tile, parsed from the kernel name"""
    nums = [int(v) for v in re.findall(r"\d+", row.name.replace("bf16", ""))]
    if row.name.startswith("conv_gemm"):
        return nums[0], nums[1]
    if row.name.startswith("conv_wgrad"):
        te = 256 if nums[1] == 1 else 128
        return te, te
    return None


@pytest.mark.parametrize("row", [r for r in V.ROWS if r.reachable], ids=repr)
def test_declared_edges_hold(row):
    N, H, W, Cin, Cout, ks, stride = row.dims(CUS)
    M, Ncol, K = row.gemm(CUS)
    t = _tile(row)
    assert row.name.count("<") == 1 and row.entry in V.ENTRIES
    assert Cin <= 520 and Cout <= 520 or row.note
    is_w = row.kind == "dw"
    for e in row.edges:
        if e == V.PR:
            assert (Ncol if is_w else M) % t[0] != 0
        elif e == V.PC:
            assert (K if is_w else Ncol) % t[1] != 0
        elif e == V.C8:
            assert Cout % 8 != 0 and row.round_once == row.res
        elif e == V.BB:
            assert N > 1 and (t is None or is_w or (M // N) % t[0] != 0)
        elif e == V.IB:
            assert ks == 3
        elif e == V.K1:
            assert -(-K // 64) == 1
        elif e == V.KODD:
            assert -(-K // 64) % 2 == 1
        elif e == V.KRAG:
            assert K % 64 != 0
        elif e == V.TAIL:
            assert M % 64 != 0
        elif e == "a block's second tile":
            tiles = -(-M // t[0]) * -(-Ncol // t[1])
            assert tiles > CUS * (2 if t[0] == 128 else 1)
        elif e == "uneven k ranges":
            assert (K // 64) % 4 != 0
    if (row.round_once or V.C8 in row.edges):
        assert Cout % 8 != 0 and V.C8 in row.edges
    if "4 stages" in row.name:
        assert -(-M // 128) * -(-Ncol // 128) <= CUS


def test_host_side_plans_agree_with_the_ledger():
    """what the library's host-only planning functions say about the rows: forward tile under knob 2, weight-gradient tile
    and split count under knob 3, the split-K plan"""
    from mdm_hip import _lib

    L = _lib.lib()
    BF16 = 1
    try:
        for row in V.ROWS:
            if not row.reachable:
                continue
            for k, v in row.knobs.items():
                assert L.mdm_dev_set_knob(k, v) == 0
            M, Ncol, K = row.gemm(CUS)
            t = _tile(row)
            if row.name.startswith("conv_gemm") and row.entry not in ("s2_dgrad", "up_fwd"):
                Mt = M * row.groups if row.entry == "linear_grouped" else M
                assert L.mdm_conv_fwd_tile(Mt, Ncol, BF16) == t[0] * 1000 + t[1], row
            if row.entry == "fwd" and row.name.startswith("conv_gemm_bl"):
                sp, ws = ctypes.c_int(0), ctypes.c_size_t(0)
                assert L.mdm_conv_fwd_plan(M, Ncol, K, BF16, ctypes.byref(sp), ctypes.byref(ws)) == 0
                if row.splitk:
                    assert "splitk x%d" % sp.value in row.name and ws.value == sp.value * M * Ncol * 4
            if row.entry in ("wgrad", "wgrad_blocked"):
                sp, ws = ctypes.c_int(0), ctypes.c_size_t(0)
                assert L.mdm_conv_wgrad_plan(M, Ncol, K, BF16, ctypes.byref(sp), ctypes.byref(ws)) == 0
                if t is not None:
                    assert L.mdm_conv_wgrad_tile(M, Ncol, K, BF16) == t[0], row
                assert (sp.value > 1) == (V.SPL in row.edges), (row, sp.value)
                assert ws.value >= sp.value * Ncol * K * 4
            for k in row.knobs:
                assert L.mdm_dev_set_knob(k, 0) == 0
    finally:
        for k in (2, 3):
            L.mdm_dev_set_knob(k, 0)


def test_every_kernel_name_format_has_a_row():
    src = open(os.path.join(ROOT, "ml-mdm_amd", "csrc", "gemm_conv.hip")).read()
    fmts = V.note_kernel_formats(src)
    assert len(fmts) >= 10
    for fmt in fmts:
        if fmt in V.FP32_ONLY_FORMATS:
            continue
        rx = V.format_regex(fmt)
        assert any(rx.match(r.name) for r in V.ROWS), "no ledger row for kernel-name format %r" % fmt
    # ... and every row's name is one the source can produce
    for r in V.ROWS:
        assert any(V.format_regex(f).match(r.name) for f in fmts), r
    # the variants the issue lists, by name
    names = {r.name for r in V.ROWS if r.reachable}
    for mode in (0, 1):
        for big in (0, 1):
            assert "conv_wgrad_bl_kernel<%d, %d>" % (mode, big) in names
        for tile in ((128, 32, 4, 1), (128, 64, 2, 2), (128, 128, 2, 2), (256, 256, 2, 4)):
            assert V.GK % (tile + (mode,)) in names
        for tile, tag in (((128, 128, 2, 2), ", 4 stages"), ((128, 128, 2, 2), ""), ((256, 192, 2, 4), ""), ((256, 256, 2, 4), ""),
                          ((128, 128, 2, 2), ", splitk x4")):
            assert V.BL % (tile + (mode, tag)) in names
    for big in (0, 1):
        assert "conv_wgrad_tr_kernel<1, %d>" % big in names
    assert V.GK % (128, 128, 2, 2, 2) in names
    for tile in ((128, 128, 2, 2), (256, 192, 2, 4), (256, 256, 2, 4)):
        assert V.BL % (tile + (1, ", sel4")) in names and V.BL % (tile + (0, ", grouped")) in names
    unreachable = [r for r in V.ROWS if not r.reachable]
    assert all(r.note for r in unreachable) and {r.name for r in unreachable} == {"conv_wgrad_tr_kernel<0, 0>", "conv_wgrad_tr_kernel<0, 1>"}


# ---- planted defects -----------------------------------------------------------------------------------------------
def _defects(row, o):
    """{name: fp32 pre-residual sum of a defective kernel} for a forward row"""
    import torch.nn.functional as F

    x, w, b = o["x"].float(), o["w"].float(), o["b"].float()
    N, H, W, Cin, Cout, ks, stride = row.dims(CUS)
    good = F.conv2d(x, w, b, padding=ks // 2)
    bn = _tile(row)[1]
    out = {}
    # one reduction term (tap, input channel) dropped for every output
    w2 = w.clone()
    w2[:, 5, ks // 2, ks // 2] = 0
    out["one reduction term dropped"] = F.conv2d(x, w2, b, padding=ks // 2)
    # two reduction columns swapped: two taps (3x3) / two input channels (1x1)
    w2 = w.clone()
    if ks == 3:
        w2[:, :, 0, 0], w2[:, :, 2, 2] = w[:, :, 2, 2], w[:, :, 0, 0]
    else:
        w2[:, 0], w2[:, 1] = w[:, 1], w[:, 0]
    out["two taps swapped"] = F.conv2d(x, w2, b, padding=ks // 2)
    # bias missing on the last column tile
    y = good.clone()
    c0 = (Cout - 1) // bn * bn
    y[:, c0:] -= b[c0:].view(1, -1, 1, 1)
    out["bias missing on the last column tile"] = y
    # the first output row of sample 1 computed from sample 0's pixels (a batch boundary inside a row tile)
    y = good.clone()
    y[1, :, 0, 0] = good[0, :, 0, 0]
    out["a row taken from the neighbouring sample"] = y
    if ks == 3:
        # the left image border read as valid: the flat-index neighbour (last pixel of the row above) instead of zero
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 1:, 0] = xp[:, :, :-1, W]
        out["one image border read as valid"] = F.conv2d(xp, w, b)
    return out


@pytest.mark.parametrize("rid", ["bl256_3x3_fwd", "bl128s4_1x1_fwd"])
def test_gates_catch_planted_defects(rid):
    """bl256_3x3_fwd is 2 x 12 x 12, 256 -> 264, 3x3 (K = 2304); bl128s4_1x1_fwd is 3 x 10 x 12, 64 -> 132, 1x1"""
    row = V.BY_ID[rid]
    passes_old_gate = {}
    for kind in ("int", "random"):
        o = V.operands(row, kind, CUS)
        e = V.reference(row, o, CUS)["y"]
        good = V.emulate(row, o)["y"]
        if kind == "int":
            assert V.int_mismatches(good, V.int_expected(row, e)) == 0
        else:
            assert V.bound_ratio(good, e)[1] == 0 and V.old_relerr(good, e.ref) < 3e-2
        for name, s in _defects(row, o).items():
            bad = V.epilogue(row, s, o["res"])
            if kind == "int":
                n = V.int_mismatches(bad, V.int_expected(row, e))
                print("%s, integer data, %s: %d of %d elements differ" % (rid, name, n, bad.numel()))
                assert n > 0, name
            else:
                worst, over = V.bound_ratio(bad, e)
                old = V.old_relerr(bad, e.ref)
                passes_old_gate[name] = old < 3e-2
                print("%s, random data, %s: %d of %d elements over the bound (worst %.1f x); old relerr %.4f" % (rid, name, over, bad.numel(), worst, old))
                assert over > 0 and worst > 1.0, name
    # the reason for this file, on record: the old gate (max error < 3 % of the largest reference value) lets the dropped
    # term through at K = 2304 (0.027; at K = 64 the same defect is 0.16 and fails it); the structural defects fail both
    assert passes_old_gate.pop("one reduction term dropped") == (rid == "bl256_3x3_fwd")
    assert not any(passes_old_gate.values()), passes_old_gate
