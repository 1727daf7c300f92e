"""The attention variant ledger (tests/attn_variant_cases.py) and its gates, checked without a GPU: the fp64 reference sits
at bound ratio 0 on every row, a CPU emulation with the kernels' roundings at the counted rounding points stays inside the
derived bounds, the exact conditions of the uniform kind hold for it, planted defects fail the gates (and the old one-number
gate of tests/test_ops_gpu.py lets the flat single-row ones through), every declared edge holds arithmetically at 256 CUs,
the required coverage is there, and every kernel-name format of the launch functions has a row.

Worst |got - ref| / bound of the emulation per tensor over all rows (large rows at L = 200 / 9 heads), as this file prints:
    bf16 random    out 0.32, out_cross 0.41, lse_self 0.017, lse_cross 0.016, dq 0.10, dk 0.12, dv 0.34, dkc 0.077, dvc 0.44
    bf16 uniform   out 0.19, out_cross 0.098, lse_self 0.0078, lse_cross 0.0041, dq 0.064, dk 0, dv 0.37, dkc 0, dvc 0.061
    fp32 random    out 0.003, out_cross 0.0055, lse_self 0.011, lse_cross 0.017, dq 0.0006, dk 0.0004, dv 0.0026, dkc 0.0004, dvc 0.0017
    fp32 uniform   out 0.003, out_cross 0.004, lse_self 0.0078, lse_cross 0.0041, dq 0.0004, dk 0, dv 0.0044, dkc 0, dvc 0.0005
(bf16: one rounding at 2^-8 with the overall factor 2 is met at 0.3 - 0.45 by the tensors that are a rounding plus a short
sum; the fp32 bounds add up n roundings of 2^-24 that a real sum averages out.  The fp64 reference itself gives 0 everywhere.)
"""
import os
import re

import pytest
import torch

import attn_variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256   # what device_cus() assumes without a GPU


def _host_row(row):
    """the row itself, or -- where the shape is large (L = 1000, as many heads as CUs) -- a copy with L = 200 / 9 heads: the
    arithmetic of the gate does not depend on which kernel runs"""
    B, L, S, H = row.dims(CUS)
    if L < 1000 and B * H < 64:
        return row
    shape = (B if B * H < 64 else 9, min(L, 200), S, H)
    return V.Row(row.id, row.entry, row.dtype, row.d, shape, row.mask, row.flat, row.name, row.edges, row.fwd, row.bwd)


@pytest.mark.parametrize("row", V.ROWS, ids=repr)
def test_reference_is_at_zero_and_the_emulation_within_the_bound(row):
    hr = _host_row(row)
    bwd = row.entry == "bwd"
    for kind in V.KINDS:
        o = V.operands(hr, kind, CUS)
        exp = V.reference(hr, o)
        exp.pop("_aux")
        assert set(exp) >= {"out", "lse_self"} and (not bwd or set(exp) >= {"dq", "dk", "dv"})
        ref = V.attention(o, backward=bwd)
        got = V.attention(o, torch.float32, emulate=True, backward=bwd)
        for k, e in exp.items():
            assert V.bound_ratio(ref[k], e) == (0.0, 0), (row, kind, k)
            assert bool(torch.isfinite(e.ref).all()) or k == "lse_cross"
            worst, over = V.bound_ratio(got[k], e)
            print("HOST %s %s %s: worst |got - ref| / bound = %.3g" % (row.id, kind, k, worst))
            assert over == 0 and worst <= 1.0, (row, kind, k, worst, over)
        if kind == "uniform":
            _check_uniform(hr, o, V.reference(hr, o), got)


def _check_uniform(row, o, exp, got):
    ue = V.uniform_expect(row, o, exp)
    for k in ("lse_self", "lse_cross"):
        if k in ue:
            # the fp64 reference IS ln(n_live) (-inf for the dead sample) ...
            same = (exp[k].ref == ue[k]) | ((exp[k].ref - ue[k]).abs() < 1e-12)
            assert bool(same.all()), (row, k)
            assert V.bound_ratio(got[k], exp[k])[1] == 0
    worst, over = V.bound_ratio(got["out"], ue["out"])
    assert over == 0, (row, worst)
    for k in ("dk", "dkc"):
        if k in got:
            assert bool((got[k] == 0).all()) and float(exp[k].bound().max()) == 0.0, (row, k)
    if row.dtype == "bf16" and "dv" in got:
        for k, cands in V.uniform_dv_candidates(row, o).items():
            assert 1 <= len(cands) <= 2 and V.heads_without_exact_match(got[k], cands, o["H"]) == 0, (row, k)
    if row.mask == "dead":
        B, L, S, H = row.dims(CUS)
        assert bool((got["out_cross"][0] == 0).all()) and bool(torch.isinf(got["lse_cross"][0]).all())
        for k in ("dkc", "dvc"):
            if k in got:
                assert bool((got[k][0] == 0).all())


def test_emulation_is_not_far_inside_the_bound():
    """a bound the emulation sits far inside would gate nothing.  out and dV are one rounding plus a short sum and come
    to 0.3 - 0.45 of their bound; dQ / dK sum the independent roundings of dS over all keys / queries, which a worst-case
    bound adds up and a real sum averages out (1 / sqrt(n)): 0.05 - 0.1 (the figures are in the module docstring)"""
    worst = {}
    for row in V.ROWS:
        if row.dtype != "bf16" or row.entry != "bwd" or row.dims(CUS)[1] > 320 or row.dims(CUS)[0] > 8:
            continue
        o = V.operands(row, "random", CUS)
        exp = V.reference(row, o)
        exp.pop("_aux")
        got = V.attention(o, torch.float32, emulate=True)
        for k, e in exp.items():
            worst[k] = max(worst.get(k, 0.0), V.bound_ratio(got[k], e)[0])
    print(worst)
    for k in ("out", "out_cross", "dq", "dk", "dv", "dkc", "dvc"):
        assert (0.25 if k in ("out", "out_cross", "dv", "dvc") else 0.03) < worst[k] <= 1.0, (k, worst[k])


# ---- planted defects -----------------------------------------------------------------------------------------------
FLAT = V.Row("defect_flat", "bwd", "bf16", 64, (2, 1000, 20, 1), "partial", True, V.P32)
PEAKED = V.Row("defect_peaked", "bwd", "bf16", 96, (2, 250, 20, 2), "partial", False, V.S32 % 96)


def _defect_list(L):
    def mk(**kw):
        d = V.Defect()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    return {
        "one key lost": mk(lose_key=L - 1),
        "last ragged query row counted twice in dK / dV": mk(dup_query=L - 1),
        "one dead text key treated as live": mk(live_dead=True),
        "dQ / dK without the scale": mk(no_scale=True),
        "delta from out instead of the self part": mk(delta_total=True),
        "an 8-row reduction group dropped": mk(drop_rows=(L - 16, L - 8)),
        "one unwritten output row": mk(nan_out_row=L - 1),
    }


def _fails_new_gate(got, exp, row=None, o=None):
    """{tensor: (worst ratio, elements over the bound)}; with ``row`` (uniform kind) the exact dV condition too"""
    over = {}
    for k, e in exp.items():
        w, n = V.bound_ratio(got[k], e)
        if n:
            over[k] = (w, n)
    if row is not None:
        for k, cands in V.uniform_dv_candidates(row, o).items():
            n = V.heads_without_exact_match(got[k], cands, o["H"])
            if n:
                over[k + " exact"] = (float("inf"), n)
    return over


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_gates_catch_planted_defects(regime):
    """every defect fails the new gates of at least one operand kind of the row (the GPU test runs both kinds of every row),
    in the flat regime (q, k at scale 0.3, L = 1000, d = 64) and in the peaked one (scale 1.2, L = 250, d = 96).
    What the old gate (max |a - b| / max |b| < 3e-2 over out, over dqkv as a whole and over dkvc as a whole) says about the
    same defective tensors, on record:
        flat:   PASSES the query row counted twice and the dropped 8-row group (both kinds) and the lost key (uniform kind;
                with random operands the lost key's own zeroed dK / dV row is a large local error): one row among a
                thousand weighs 1e-3.  The row counted twice is also inside the random kind's elementwise bound (1 / L <
                2^-8: one bf16 rounding of P moves dV further); the uniform kind's exact dV condition is what shows it.
        peaked: PASSES the query row counted twice and the dropped 8-row group with uniform operands, fails the rest.
    The missing scale, the wrong delta, the live dead key and the unwritten row fail both gates in both regimes."""
    row = PEAKED if regime == "peaked" else FLAT
    L = row.dims(CUS)[1]
    new, old = {}, {}
    for kind in V.KINDS:
        o = V.operands(row, kind, CUS)
        exp = V.reference(row, o)
        exp.pop("_aux")
        ref = V.attention(o)
        urow = row if kind == "uniform" else None
        good = V.attention(o, torch.float32, emulate=True)
        assert not _fails_new_gate(good, exp, urow, o) and V.old_gate_passes(good, ref)
        for name, d in _defect_list(L).items():
            bad = V.attention(o, torch.float32, emulate=True, defect=d)
            over = _fails_new_gate(bad, exp, urow, o)
            op = V.old_gate_passes(bad, ref)
            print("%s, %s kind, %s: over the bound in %s; old gate %s" % (regime, kind, name, {k: "%d (worst %.3g x)" % (n, w) for k, (w, n) in over.items()},
                                                                       "PASSES" if op else "fails"))
            new[name] = new.get(name, False) or bool(over)
            old[kind, name] = op
    assert all(new.values()), new
    # the reason this file exists
    if regime == "flat":
        assert old["uniform", "one key lost"]
        for kind in V.KINDS:
            assert old[kind, "last ragged query row counted twice in dK / dV"] and old[kind, "an 8-row reduction group dropped"]
    for kind in V.KINDS:
        assert not old[kind, "one unwritten output row"] and not old[kind, "dQ / dK without the scale"]


# ---- the ledger ------------------------------------------------------------------------------------------------------
def _family(row):
    n = row.name
    if n.startswith("attn_fwd"):
        return "fwd_f32" if "float" in n else "fwd_qt" + n[-2]
    if "small32" in n:
        return "small32"
    if "small" in n:
        return "small"
    if "dq32" in n:
        return "pair32"
    return "pair16_f32" if "float" in n else "pair16_bf16"


def _query_block(row):
    """queries per block of the (first) kernel of the row, None for the one-block-per-head kernels"""
    f = _family(row)
    if f.startswith("fwd"):
        return 64 * int(row.name[-2])
    if f.startswith("pair16"):
        return 64 * int(re.match(r"attn_bwd_dq_kernel<\w+,\d+,(\d)>", row.name).group(1))
    return 256 if f == "pair32" else None


@pytest.mark.parametrize("row", V.ROWS, ids=repr)
def test_declared_edges_and_names_hold(row):
    B, L, S, H = row.dims(CUS)
    assert row.d in (32, 64, 96, 128) and L <= 1100 and B * H <= 330
    for cus in ((CUS,) if callable(row.shape) else (64, 104, 256, 304)):
        # (fixed shapes sit far from every CU-count rule; the rows at a rule move with the count)
        Bc, Lc, Sc, Hc = row.dims(cus)
        assert V.launch_rule(row.entry, row.dtype, row.d, row.fwd, row.bwd, Bc, Lc, Sc, Hc, cus) == row.name, cus
    if callable(row.shape):
        for cus in (64, 104, 304):
            Bc, Lc, Sc, Hc = row.dims(cus)
            assert V.launch_rule(row.entry, row.dtype, row.d, row.fwd, row.bwd, Bc, Lc, Sc, Hc, cus) == row.name, cus
    qb = _query_block(row)
    for e in row.edges:
        if e == V.QB2:
            assert qb and -(-L // qb) >= 2 and L % qb != 0
        elif e == V.KODD:
            assert -(-L // 64) % 2 == 1
        elif e == V.KRAG:
            assert L % 64 != 0
        elif e == V.TXT:
            assert S > 0
        elif e == V.TXT2:
            assert 64 < S < 128
        elif e == V.BH8:
            # more than one block per (batch, head): query blocks, or the key blocks of the dK / dV kernel
            assert B * H in (3, 7, 9) and qb and (-(-L // qb) > 1 or row.entry == "bwd")
        elif e == V.OVER:
            assert B * H > CUS and qb is None
        elif e == V.L16:
            assert L < 16
        else:
            raise AssertionError(e)
    if row.mask != "none":
        assert S > 0
    if row.mask == "dead":
        assert B >= 2
    m = V.make_mask(row, B, S, torch.Generator().manual_seed(1))
    if m is not None:
        live = (m != 0).sum(1)
        if row.mask == "dead":
            assert int(live[0]) == 0 and bool((live[1:] > 0).all()) and bool(torch.signbit(m[0]).any() or S == 1)
        elif row.mask == "one":
            assert bool((live == 1).all()) and m[0, S - 1] != 0
        else:
            assert bool(((live & (live - 1)) == 0).all()) and bool((live > 0).all()) and (S <= 2 or bool((live < S).all()))
        if row.mask == "values" and S >= 4:
            assert bool(((m != 0) & (m != 1)).any()) and bool(torch.signbit(m[m == 0]).any())


def test_required_coverage():
    names = {r.name for r in V.ROWS}
    for d in (32, 64, 96, 128):
        for qt in (1, 2):
            assert V.FW % ("bf16", d, qt) in names
            rows = [r for r in V.ROWS if r.name == V.FW % ("bf16", d, qt) and {V.QB2, V.KODD, V.KRAG, V.TXT} <= set(r.edges)]
            assert rows, (d, qt)
        assert V.FW % ("float", d, 2) in names
        assert V.P16("bf16", d) in names and V.P16("float", d) in names and V.SM % d in names
    assert {V.S32 % 64, V.S32 % 96, V.P32} <= names
    assert {re.findall(r",(\d)>", V.P16(t, d))[0] for t in ("bf16", "float") for d in (32, 64, 96, 128)} == {"1", "2"}
    # the product's rule: both sides of every branch, knobs at 0
    rule = {r.id: r for r in V.ROWS if r.fwd == 0 and r.bwd == 0}
    for a, b in (("fwd_rule_fills", "fwd_rule_over"), ("fwd_rule_L64", "fwd_rule_L65"), ("rule_L256_d64", "rule_L257_d64"),
                 ("rule_L256_d96", "rule_L257_d96"), ("rule_S32", "rule_S33"), ("rule_S64_fills", "rule_S65_fills"),
                 ("rule_below_d32", "rule_fills_d32"), ("rule_below_d128", "rule_fills_d128")):
        assert rule[a].name != rule[b].name and rule[a].d == rule[b].d
    # edges per kernel family, as far as the family can see them
    LS, SS = {1, 15, 33, 64, 65, 129, 200, 256, 320, 1000}, {0, 1, 3, 20, 32, 33, 64, 65, 77}
    limit = {"small": (256, 64), "small32": (256, 32), "pair32": (1000, 32)}
    cov = {}
    for r in V.ROWS:
        B, L, S, H = r.dims(CUS)
        c = cov.setdefault(_family(r), {"L": set(), "S": set(), "mask": set(), "BH": set(), "flat": set()})
        c["L"].add(L), c["S"].add(S), c["mask"].add(r.mask if S else "none"), c["flat"].add(r.flat)
        if V.BH8 in r.edges:
            c["BH"].add(B * H)
        if V.OVER in r.edges:
            c["BH"].add("over")
    assert set(cov) == {"fwd_qt1", "fwd_qt2", "fwd_f32", "pair16_bf16", "pair16_f32", "small", "small32", "pair32"}
    for f, c in cov.items():
        lm, sm = limit.get(f, (1000, 77))
        assert {x for x in LS if x <= lm} <= c["L"], (f, sorted(LS - c["L"]))
        assert {x for x in SS if x <= sm} <= c["S"], (f, sorted(SS - c["S"]))
        assert set(V.MASKS) <= c["mask"], f
        assert c["flat"] == {True, False}, f
        assert ({"over"} if f in ("small", "small32") else {3, 7, 9}) <= c["BH"], (f, c["BH"])
    flat = [r.flat for r in V.ROWS]
    assert 0.4 < sum(flat) / len(flat) < 0.6


def test_every_kernel_name_format_has_a_row():
    src = open(os.path.join(ROOT, "ml-mdm_amd", "csrc", "attention.hip")).read()
    fmts = V.note_kernel_formats(src)
    assert len(fmts) == 5, fmts
    for fmt in fmts:
        rx = V.format_regex(fmt)
        assert any(rx.match(r.name) for r in V.ROWS), "no ledger row for kernel-name format %r" % fmt
    for r in V.ROWS:
        assert any(V.format_regex(f).match(r.name) for f in fmts), r
    # every launch of the two launch functions is followed by a note: as many notes as launch sites (the two-kernel
    # paths share one)
    body = src[src.index("static int attn_fwd_launch"):src.index('extern "C" int mdm_attn_fwd')]
    assert body.count("hipLaunchKernelGGL") == 8 and body.count("MDM_NOTE_ATTN(") == 6


def test_dev_symbols():
    """the knob takes 0 .. 2 and nothing else; the name is per thread and empty before the first launch of a thread"""
    import threading

    from mdm_hip import _lib

    L = _lib.lib()
    protos = {p[0] for p in _lib.header_prototypes(_lib.DEV_HEADER)}
    assert {"mdm_last_attn_kernel", "mdm_dev_set_attn_fwd", "mdm_dev_set_attn_bwd"} <= protos
    assert not protos & {p[0] for p in _lib.header_prototypes()}       # outside the ABI
    try:
        for mode in (0, 1, 2):
            assert L.mdm_dev_set_attn_fwd(mode) == 0
        for bad in (-1, 3, 100):
            assert L.mdm_dev_set_attn_fwd(bad) == -1
    finally:
        assert L.mdm_dev_set_attn_fwd(0) == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.mdm_last_attn_kernel()))
    t.start()
    t.join()
    assert seen == [b""]


def test_reference_is_quick():
    """the largest row's fp64 reference stays under about 2 s"""
    import time

    big = max(V.ROWS, key=lambda r: r.dims(CUS)[0] * r.dims(CUS)[3] * r.dims(CUS)[1] * (r.dims(CUS)[1] + r.dims(CUS)[2]) * (2 if r.entry == "bwd" else 1))
    o = V.operands(big, "random", CUS)
    t0 = time.perf_counter()
    V.reference(big, o)
    dt = time.perf_counter() - t0
    print("fp64 reference of %s: %.2f s" % (big.id, dt))
    assert dt < 2.0, dt   # (measured: well under 0.5 s)
