"""Every bf16 kernel variant of csrc/gemm_conv.hip, pinned by name and gated elementwise: each row of the ledger
(tests/conv_variant_cases.py) is launched through the C ABI the way mdm_hip.ops launches it, must have run the kernel
the row names (mdm_last_gemm_kernel), must reproduce integer data with ZERO differing elements and must stay inside the
derived elementwise bound on random data.  Outputs are pre-filled with NaN and followed by a guard that must stay NaN."""
import ctypes
import math

import pytest
import torch

import conv_variant_cases as V

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REACHABLE = [r for r in V.ROWS if r.reachable]


def dev():
    return torch.device("cuda:0")


def nhwc(t):
    """fp64 NCHW (bf16-representable) -> bf16 NHWC on the device"""
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(BF).to(dev())


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def f32(t):
    return None if t is None else t.float().contiguous().to(dev())


class Out:
    """an output buffer pre-filled with NaN, with a guard row of NaN behind it"""

    def __init__(self, shape, dtype):
        n, g = math.prod(shape), max(256, shape[-1])
        self.buf = torch.full((n + g,), float("nan"), dtype=dtype, device=dev())
        self.t = self.buf[:n].view(shape)
        self.guard = self.buf[n:]

    def guard_intact(self):
        return bool(torch.isnan(self.guard).all())


def blocked(dy):
    """[N, 2H, 2W, C] -> the 2x2-blocked [N, H, W, (ph, pw, c)] that mdm_space_to_depth2x makes"""
    N, H2, W2, C = dy.shape
    return dy.view(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * C).contiguous()


def launch(row, os_, cus):
    """run the row on the operands ``os_`` (one dict per group) -> ([{output: fp64 CPU tensor in reference layout}], [Out], name)"""
    from mdm_hip import _lib, ops

    L = _lib.lib()
    chk, p, st, BF16 = _lib.check, ops._p, ops._stream(), ops.BF16
    N, H, W, Cin, Cout, ks, stride = row.dims(cus)
    Ho, Wo = V.out_hw(H, W, ks, stride)
    o = os_[0]
    outs, got = [], [{} for _ in os_]
    e = row.entry
    if e in ("fwd", "dgrad"):
        w32 = f32(o["w"])
        if Cout % 8 == 0 and Cin % 8 == 0:
            wf, wd, bp, _, _, kbf, kbd = ops.packed_weight(w32, f32(o["b"]), BF)
        else:   # the C ABI takes any Cout; ops would pad it to a multiple of 8
            assert e == "fwd" and Cin % 8 == 0
            kbf = 64 if (ks == 3 and Cin % 64 == 0) else 0
            wf, bp = torch.empty(Cout * ks * ks * Cin, dtype=BF, device=dev()), f32(o["b"])
            chk(L.mdm_pack_weight(p(w32), p(wf), None, Cout, Cin, ks, Cin, Cout, kbf, 0, BF16, st), "mdm_pack_weight")
        if e == "fwd":
            x, res = nhwc(o["x"]), nhwc(o["res"])
            y = Out((N, Ho, Wo, Cout), BF)
            ws, wsb = None, 0
            if row.splitk:
                sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
                chk(L.mdm_conv_fwd_plan(N * Ho * Wo, Cout, ks * ks * Cin, BF16, ctypes.byref(sp), ctypes.byref(nb)), "mdm_conv_fwd_plan")
                assert sp.value > 1
                ws, wsb = ops._f32_ws(nb.value, dev()), nb.value
            chk(L.mdm_conv_fwd_ws(p(x), p(wf), p(bp), p(res), None, p(y.t), None, N, H, W, Cin, Ho, Wo, Cout, ks, stride, 0, 0, kbf,
                                  BF16, p(ws), wsb, st), "mdm_conv_fwd_ws")
            name = L.mdm_last_gemm_kernel().decode()
            outs, got[0]["y"] = [y], nchw(y.t)
        else:
            dy = nhwc(o["dy"])
            dx = Out((N, H, W, Cin), BF)
            tr = 1 if (ks == 3 and stride == 2) else 0
            chk(L.mdm_conv_fwd_ws(p(dy), p(wd), None, None, None, p(dx.t), None, N, Ho, Wo, Cout, H, W, Cin, ks, 1, tr, 0, kbd,
                                  BF16, None, 0, st), "mdm_conv_fwd_ws (input gradient)")
            name = L.mdm_last_gemm_kernel().decode()
            outs, got[0]["dx"] = [dx], nchw(dx.t)
    elif e == "s2_dgrad":
        wsel = ops.packed_s2_dgrad_weight(f32(o["w"]))
        dy, res = nhwc(o["dy"]), nhwc(o["res"])
        dx = Out((N, H, W, Cin), BF)
        chk(L.mdm_conv_s2_dgrad_res(p(dy), p(wsel), p(res), p(dx.t), N, Ho, Wo, Cout, Cin, BF16, st), "mdm_conv_s2_dgrad_res")
        name = L.mdm_last_gemm_kernel().decode()
        outs, got[0]["dx"] = [dx], nchw(dx.t)
    elif e in ("up_fwd", "up_dgrad"):
        w_ph, w_t, bias4 = ops.packed_upconv_weights(f32(o["w"]), f32(o["b"]))
        if e == "up_fwd":
            x = nhwc(o["x"])
            y = Out((N, 2 * H, 2 * W, Cout), BF)
            chk(L.mdm_conv_up_fwd(p(x), p(w_ph), p(bias4), p(y.t), N, H, W, Cin, Cout, BF16, st), "mdm_conv_up_fwd")
            name = L.mdm_last_gemm_kernel().decode()
            outs, got[0]["y"] = [y], nchw(y.t)
        else:
            dyb = blocked(nhwc(o["dy"]))
            dx = Out((N, H, W, Cin), BF)
            chk(L.mdm_conv_up_dgrad(p(dyb), p(w_t), p(dx.t), N, H, W, Cout, Cin, BF16, st), "mdm_conv_up_dgrad")
            name = L.mdm_last_gemm_kernel().decode()
            outs, got[0]["dx"] = [dx], nchw(dx.t)
    elif e == "linear_grouped":
        G, M = row.groups, N
        xs = [g_["x"].view(M, Cin).to(BF).to(dev()) for g_ in os_]
        packs = [ops.packed_weight(f32(g_["w"].view(Cout, Cin)), f32(g_["b"]), BF) for g_ in os_]
        ys = [Out((M, Cout), BF) for _ in range(G)]
        chk(L.mdm_linear_grouped(ops._ptr_array(xs), ops._ptr_array([pk[0] for pk in packs]), ops._ptr_array([pk[2] for pk in packs]),
                                 ops._ptr_array([y.t for y in ys]), G, M, Cin, Cout, BF16, st), "mdm_linear_grouped")
        name = L.mdm_last_gemm_kernel().decode()
        outs = ys
        for g in range(G):
            got[g]["y"] = ys[g].t.float().cpu().view(M, Cout, 1, 1)
    elif e == "wgrad":
        x, dy = nhwc(o["x"]), nhwc(o["dy"])
        M, K = N * Ho * Wo, ks * ks * Cin
        sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        chk(L.mdm_conv_wgrad_plan(M, Cout, K, BF16, ctypes.byref(sp), ctypes.byref(nb)), "mdm_conv_wgrad_plan")
        assert (sp.value > 1) == (V.SPL in row.edges), sp.value
        ws = ops._f32_ws(nb.value, dev())
        dw, db = Out((Cout, Cin, ks, ks), torch.float32), (Out((Cout,), torch.float32) if row.bias else None)
        chk(L.mdm_conv_wgrad(p(x), p(dy), 1 if row.bias else 0, p(ws), N, H, W, Cin, Ho, Wo, Cout, ks, stride, BF16, st), "mdm_conv_wgrad")
        name = L.mdm_last_gemm_kernel().decode()
        chk(L.mdm_conv_wgrad_reduce(p(ws), p(dw.t), p(db.t) if db else None, p(dy), M, Cin, Cout, ks, 0, BF16, st), "mdm_conv_wgrad_reduce")
        outs, got[0]["dw"] = [dw], dw.t.cpu()
        if db:
            outs.append(db)
            got[0]["db"] = db.t.cpu()
    elif e == "wgrad_blocked":
        x, dyb = nhwc(o["x"]), blocked(nhwc(o["dy"]))
        M, K = N * H * W, 9 * Cin
        sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        chk(L.mdm_conv_wgrad_plan(M, 4 * Cout, K, BF16, ctypes.byref(sp), ctypes.byref(nb)), "mdm_conv_wgrad_plan")
        assert (sp.value > 1) == (V.SPL in row.edges), sp.value
        ws = ops._f32_ws(nb.value, dev())
        dwb = torch.empty((4 * Cout, Cin, 3, 3), dtype=torch.float32, device=dev())   # 20 of its 36 (phase, tap) blocks stay unwritten
        db4 = torch.full((4 * Cout,), float("nan"), dtype=torch.float32, device=dev()) if row.bias else None
        dw, db = Out((Cout, Cin, 3, 3), torch.float32), (Out((Cout,), torch.float32) if row.bias else None)
        chk(L.mdm_conv_wgrad_blocked(p(x), p(dyb), 1 if row.bias else 0, p(ws), N, H, W, Cin, Cout, BF16, st), "mdm_conv_wgrad_blocked")
        name = L.mdm_last_gemm_kernel().decode()
        chk(L.mdm_conv_wgrad_reduce(p(ws), p(dwb), p(db4), p(dyb), M, Cin, 4 * Cout, 3, 0, BF16, st), "mdm_conv_wgrad_reduce")
        chk(L.mdm_upconv_wfold(p(dwb), p(dw.t), p(db4), p(db.t) if db else None, Cout, Cin, 0, st), "mdm_upconv_wfold")
        outs, got[0]["dw"] = [dw], dw.t.cpu()
        if db:
            outs.append(db)
            got[0]["db"] = db.t.cpu()
    else:
        assert e == "wgrad_grouped"
        G, M = row.groups, N
        xs = [g_["x"].view(M, Cin).to(BF).to(dev()) for g_ in os_]
        dys = [g_["dy"].view(M, Cout).to(BF).to(dev()) for g_ in os_]
        # the launch ADDS into its destinations: they start at zero (an unwritten element then shows as a wrong sum), the guard at NaN
        dws, dbs = [Out((Cout, Cin), torch.float32) for _ in range(G)], ([Out((Cout,), torch.float32) for _ in range(G)] if row.bias else None)
        for t in dws + (dbs or []):
            t.t.zero_()
        ops.wgrad_grouped(xs, dys, [t.t for t in dws], [t.t for t in dbs] if dbs else None)
        name = L.mdm_last_gemm_kernel().decode()
        outs = dws + (dbs or [])
        for g in range(G):
            got[g]["dw"] = dws[g].t.cpu().view(Cout, Cin, 1, 1)
            if dbs:
                got[g]["db"] = dbs[g].t.cpu()
    torch.cuda.synchronize()
    return got, outs, name


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("row", REACHABLE, ids=repr)
def test_conv_variant(row, kind, request):
    from mdm_hip import _lib

    L = _lib.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def knobs_off():
        for k in (2, 3):
            L.mdm_dev_set_knob(k, 0)

    request.addfinalizer(knobs_off)
    for k, v in row.knobs.items():
        assert L.mdm_dev_set_knob(k, v) == 0
    os_ = [V.operands(row, kind, cus, g) for g in range(row.groups)]
    got, outs, name = launch(row, os_, cus)
    knobs_off()
    assert name == row.name
    assert all(t.guard_intact() for t in outs), "wrote past the end of an output"
    for g, o in enumerate(os_):
        exp = V.reference(row, o, cus)
        assert set(exp) == set(got[g])
        if kind != "random":
            assert V.int_condition(exp) < V.INT_LIMIT
        for k, e in exp.items():
            assert not bool(torch.isnan(got[g][k]).any()), "%s: unwritten elements" % k
            if kind == "random":
                worst, over = V.bound_ratio(got[g][k], e)
                print("LEDGER %s group %d %s: worst |got - ref| / bound = %.3g" % (row.id, g, k, worst))
                assert over == 0, (row, k, worst, over)
            else:
                n = V.int_mismatches(got[g][k], V.int_expected(row, e))
                print("LEDGER %s %s group %d %s: %d of %d elements differ" % (row.id, kind, g, k, n, got[g][k].numel()))
                assert n == 0, (row, kind, k, n)
