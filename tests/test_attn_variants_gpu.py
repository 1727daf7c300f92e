"""Every kernel instantiation behind mdm_attn_fwd / mdm_attn_bwd, pinned by name and gated per element: each row of the
ledger (tests/attn_variant_cases.py) is launched through the C ABI the way mdm_hip.ops.AttentionFn launches it -- so that
lse_self / lse_cross, out_cross and the delta workspaces are visible --, must have run the kernel(s) the row names
(mdm_last_attn_kernel), and every output (out, out_cross, lse_self, lse_cross, dQ, dK, dV, dKc, dVc, each on its own) must
stay inside the bound derived in the ledger's docstring, with both operand kinds; the uniform kind adds its exact
conditions.  Every buffer the entry points write is pre-filled with NaN and followed by a guard that must stay NaN."""
import math

import pytest
import torch

import attn_variant_cases as V

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


class Out:
    """a buffer pre-filled with NaN, with a guard of NaN behind it"""

    def __init__(self, shape, dtype):
        n, g = math.prod(shape), max(256, shape[-1])
        self.buf = torch.full((n + g,), float("nan"), dtype=dtype, device=dev())
        self.t = self.buf[:n].view(shape)
        self.guard = self.buf[n:]

    def guard_intact(self):
        return bool(torch.isnan(self.guard).all())

    def ptr(self):
        return self.buf.data_ptr()


def _restore():
    from mdm_hip import _lib

    _lib.lib().mdm_dev_set_attn_fwd(0)
    _lib.lib().mdm_dev_set_attn_bwd(0)


def launch(row, o, cus):
    """-> ({tensor: fp64 CPU}, {buffer name: Out}, name after the forward, name after the backward or None)"""
    from mdm_hip import _lib, ops

    lib = _lib.lib()
    chk, p, st = _lib.check, ops._p, ops._stream()
    B, L, S, H = row.dims(cus)
    d, C = row.d, H * row.d
    tdt, code = (torch.bfloat16, ops.BF16) if row.dtype == "bf16" else (torch.float32, ops.F32)
    up = lambda t: None if t is None else t.to(tdt).contiguous().to(dev())
    qkv, kvc, dout = up(o["qkv"]), up(o["kvc"]), up(o["dout"])
    mask = None if o["mask"] is None else o["mask"].float().contiguous().to(dev())
    if mask is not None and row.mask in ("values", "dead"):
        assert bool(torch.signbit(mask[mask == 0]).any())       # the -0.0 reached the device as -0.0
    f32 = torch.float32
    bufs = {"out": Out((B, L, C), tdt), "lse_self": Out((B, H, L), f32)}
    if S:
        bufs["out_cross"], bufs["lse_cross"] = Out((B, L, C), tdt), Out((B, H, L), f32)
    bp = lambda k: bufs[k].ptr() if k in bufs else None
    assert lib.mdm_dev_set_attn_fwd(row.fwd if row.entry == "fwd" else 0) == 0
    chk(lib.mdm_attn_fwd(p(qkv), p(kvc), p(mask), bp("out"), bp("out_cross"), bp("lse_self"), bp("lse_cross"), B, L, S, H, d, code, st), "mdm_attn_fwd")
    name_fwd, name_bwd = lib.mdm_last_attn_kernel().decode(), None
    if row.entry == "bwd":
        bufs["dqkv"], bufs["delta_self"] = Out((B, L, 3 * C), tdt), Out((B, H, L), f32)
        if S:
            bufs["dkvc"], bufs["delta_cross"] = Out((B, S, 2 * C), tdt), Out((B, H, L), f32)
        assert lib.mdm_dev_set_attn_bwd(row.bwd) == 0
        chk(lib.mdm_attn_bwd(p(qkv), p(kvc), p(mask), bp("out"), bp("out_cross"), p(dout), bp("lse_self"), bp("lse_cross"), bp("delta_self"),
                             bp("delta_cross"), bp("dqkv"), bp("dkvc"), B, L, S, H, d, code, st), "mdm_attn_bwd")
        name_bwd = lib.mdm_last_attn_kernel().decode()
    torch.cuda.synchronize()
    _restore()
    cpu = lambda t: t.double().cpu()
    got = {k: cpu(bufs[k].t) for k in ("out", "out_cross", "lse_self", "lse_cross") if k in bufs}
    if row.entry == "bwd":
        g = cpu(bufs["dqkv"].t)
        got["dq"], got["dk"], got["dv"] = g[..., :C], g[..., C:2 * C], g[..., 2 * C:]
        if S:
            g = cpu(bufs["dkvc"].t)
            got["dkc"], got["dvc"] = g[..., :C], g[..., C:]
    return got, bufs, name_fwd, name_bwd


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("row", V.ROWS, ids=repr)
def test_attn_variant(row, kind, request):
    request.addfinalizer(_restore)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, L, S, H = row.dims(cus)
    o = V.operands(row, kind, cus)
    exp = V.reference(row, o)
    got, bufs, name_fwd, name_bwd = launch(row, o, cus)
    bad = []

    # ---- name ---------------------------------------------------------------------------------------------------------
    if row.entry == "fwd":
        if name_fwd != row.name:
            bad.append("ran %s, the row names %s" % (name_fwd, row.name))
    else:
        want_fwd = V.launch_rule("fwd", row.dtype, row.d, 0, 0, B, L, S, H, cus)
        if name_fwd != want_fwd or name_bwd != row.name:
            bad.append("ran %s and %s, expected %s and %s" % (name_fwd, name_bwd, want_fwd, row.name))

    # ---- memory -------------------------------------------------------------------------------------------------------
    for k, b in bufs.items():
        if not b.guard_intact():
            bad.append("%s: written past its end" % k)
        if k.startswith("delta") and not row.writes_delta:
            continue                                     # the one-block-per-head kernels keep delta in LDS
        nan = int(torch.isnan(b.t).sum())
        if nan:
            bad.append("%s: %d of %d elements left unwritten (or NaN)" % (k, nan, b.t.numel()))

    # ---- per element, every tensor on its own -------------------------------------------------------------------------
    aux = exp.pop("_aux")
    for k, e in exp.items():
        worst, over = V.bound_ratio(got[k], e)
        print("LEDGER %s %s %s: worst |got - ref| / bound = %.3g" % (row.id, kind, k, worst))
        if over:
            bad.append("%s: %d of %d elements over the bound, worst %.3g x" % (k, over, got[k].numel(), worst))
        fin = torch.isfinite(got[k]) | (torch.isinf(e.ref) & (got[k] == e.ref))
        if not bool(fin.all()):
            bad.append("%s: %d non-finite elements" % (k, int((~fin).sum())))

    # ---- the dead sample: no cross term, lse_cross = -inf (what attn_fwd_kernel computes), zero text gradients -----------
    if row.mask == "dead":
        if not bool((got["out_cross"][0] == 0).all()) or not bool((got["lse_cross"][0] == float("-inf")).all()):
            bad.append("dead sample: out_cross != 0 or lse_cross != -inf")
        for k in ("dkc", "dvc"):
            if k in got and not bool((got[k][0] == 0).all()):
                bad.append("dead sample: %s != 0" % k)

    # ---- the exact conditions of the uniform kind ---------------------------------------------------------------------
    if kind == "uniform":
        exp["_aux"] = aux
        ue = V.uniform_expect(row, o, exp)
        worst, over = V.bound_ratio(got["out"], ue["out"])
        print("LEDGER %s %s out (one rounding of the mean): worst |got - ref| / bound = %.3g" % (row.id, kind, worst))
        if over:
            bad.append("out is not one rounding of the mean over the live keys: %d elements, worst %.3g x" % (over, worst))
        for k in ("lse_self", "lse_cross"):
            if k in ue:
                w, n = V.bound_ratio(got[k], V.Expect(ue[k], exp[k].bound()))
                if n:
                    bad.append("%s != ln(live keys): %d rows, worst %.3g x" % (k, n, w))
        for k in ("dk", "dkc"):
            if k in got and not bool((got[k] == 0).all()):
                bad.append("%s is not exactly 0 with q = 0: %d elements" % (k, int((got[k] != 0).sum())))
        if row.dtype == "bf16" and row.entry == "bwd":
            for k, cands in V.uniform_dv_candidates(row, o).items():
                n = V.heads_without_exact_match(got[k], cands, H)
                if n:
                    bad.append("%s != bf16(bf16(1 / n) sum_i do_i) in %d of %d (batch, head) pairs" % (k, n, B * H))
    assert not bad, "%s %s %s: %s" % (row.id, kind, row.dims(cus), "; ".join(bad))
