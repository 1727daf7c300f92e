"""GPU: the launch sequence of the inference attention -- which C entries ``ops.attention`` and its views ``attention_pag``,
``attention_biased`` and ``attention_controlled`` call, in which order, with which integer arguments, and which batch row of
which operand stands behind every pointer.  A forwarding proxy around the loaded library notes the calls; every launch is
still made, so the outputs are compared too.  The expected sequences are written out below for the layer case of
tests/attn_control_cases.py (N = 7: 2 uncond, 2 sources, 2 edits, 1 perturbed; d = 64, H = 3, L = 80, S = 77, bf16: S is no
multiple of 4, L no multiple of a tile, every block non-empty); ``SelfAttention.forward`` under each switch is compared with
the same dispatcher called by hand on the tensors the layer passed."""
import ctypes

import pytest
import torch

import attn_control_cases as AC
import parity_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, H, L, S = 64, 3, 80, 77
C, LD, N = H * D, 80, 7
BF = 1   # the dtype code of bf16 (include/mdm_hip.h)
ENTRIES = ("mdm_attn_fwd", "mdm_attn_cross_addv", "mdm_attn_cross_bias", "mdm_ctrl_gather_qkv", "mdm_ctrl_mix_kv")
DISPATCHERS = ("attention", "attention_pag", "attention_biased", "attention_controlled")


class Recorder:
    """A forwarding proxy around the loaded library.  The calls of ENTRIES are noted with their raw arguments; ``labelled``
    then names every pointer "operand@batch row" (+ the offset inside the row, in elements, where there is one).  The
    outputs of the two control kernels join the operands from the call that writes them: an address may have belonged to
    a temporary that was freed before."""

    def __init__(self, real, protos):
        self._real, self._protos = real, protos
        self.calls, self.learned = [], []   # learned: (first call, label, address, rows, bytes per row, element size)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ENTRIES:
            return fn

        def call(*args):
            es = 2 if args[-2] == BF else 4
            if name == "mdm_ctrl_gather_qkv":
                _, R, L_, C_ = args[6:10]
                self.learned += [(len(self.calls), lab, p, R, L_ * 3 * C_ * es, es)
                                 for lab, p in (("qs", args[4]), ("qx", args[5]))]
            if name == "mdm_ctrl_mix_kv":
                _, R, S_, C_ = args[10:14]
                self.learned += [(len(self.calls), lab, p, R, S_ * 2 * C_ * es, es)
                                 for lab, p in (("kv_a", args[8]), ("kv_b", args[9]))]
            self.calls.append((name, args[:-1]))   # without the stream
            return fn(*args)

        return call

    def labelled(self, **operands):
        regions = [(0, lab, t.data_ptr(), t.shape[0], t.numel() // t.shape[0] * t.element_size(), t.element_size())
                   for lab, t in operands.items() if t is not None]
        out = []
        for i, (name, args) in enumerate(self.calls):
            row = [name]
            for ctype, v in zip(self._protos[name], args):
                if ctype is not ctypes.c_void_p or v is None:
                    row.append(v)
                    continue
                for since, lab, base, rows, row_bytes, es in regions + self.learned:
                    if since <= i and base <= v < base + rows * row_bytes:
                        r, off = divmod(v - base, row_bytes)
                        row.append("%s@%d" % (lab, r) + ("+%d" % (off // es) if off else ""))
                        break
                else:
                    row.append("tmp")   # allocated inside the call and gone after it: oc, the sources' masks
            out.append(tuple(row))
        return out


@pytest.fixture
def recorded(monkeypatch):
    """-> run(fn) = (what fn returns, the Recorder of its launches)"""
    from mdm_hip import _lib

    real = _lib.lib()
    protos = {n: types for hdr in (_lib.HEADER, _lib.EXT_HEADER) for n, _, types, _ in _lib.header_prototypes(hdr)}

    def run(fn):
        rec = Recorder(real, protos)
        with monkeypatch.context() as m:
            m.setattr(_lib, "lib", lambda: rec)
            return fn(), rec

    return run


def _case():
    case = AC.layer_case(D, H, L, S, seed=3)
    qkv, kvc, mask = case["qkv"].to(DEV, torch.bfloat16), case["kvc"].to(DEV, torch.bfloat16), case["mask"].to(DEV)
    return case, qkv, kvc, mask


def _rows_operands(rows):
    return dict(own=rows.own, src=rows.src, M=rows.M, D=rows.D, gate_c=rows.gate_c, gate_s=rows.gate_s)


def _zero(R):
    from mdm_hip import ops

    return ops._CTRL_ZERO.get((torch.device(DEV), R, L, LD))


# ---- the sequences -----------------------------------------------------------------------------------------------------
FWD_ALL = [("mdm_attn_fwd", "qkv@0", "kvc@0", "mask@0", "out@0", "tmp", None, None, 7, L, S, H, D, BF)]
PAG_1 = [("mdm_attn_fwd", "qkv@0", "kvc@0", "mask@0", "out@0", "tmp", None, None, 6, L, S, H, D, BF),
         ("mdm_attn_cross_addv", "qkv@6", "kvc@6", "mask@6", "out@6", 1, L, S, H, D, BF)]
PAG_N = [("mdm_attn_cross_addv", "qkv@0", "kvc@0", "mask@0", "out@0", 7, L, S, H, D, BF)]
BIASED_0 = [("mdm_attn_fwd", "qkv@0", None, None, "out@0", None, None, None, 7, L, 0, H, D, BF),
            ("mdm_attn_cross_bias", "qkv@0", "kvc@0", "mask@0", "bias@0", LD, "out@0", C, "out@0", 7, L, S, H, D, BF)]
BIASED_1 = [("mdm_attn_fwd", "qkv@0", None, None, "out@0", None, None, None, 6, L, 0, H, D, BF),
            ("mdm_attn_cross_bias", "qkv@0", "kvc@0", "mask@0", "bias@0", LD, "out@0", C, "out@0", 6, L, S, H, D, BF),
            ("mdm_attn_cross_bias", "qkv@6", "kvc@6", "mask@6", "bias@6", LD, "qkv@6+%d" % (2 * C), 3 * C, "out@6",
             1, L, S, H, D, BF)]
BIASED_N = [("mdm_attn_cross_bias", "qkv@0", "kvc@0", "mask@0", "bias@0", LD, "qkv@0+%d" % (2 * C), 3 * C, "out@0",
             7, L, S, H, D, BF)]
LEAD = [("mdm_attn_fwd", "qkv@0", "kvc@0", "mask@0", "out@0", "tmp", None, None, 4, L, S, H, D, BF)]
EDITED = [("mdm_ctrl_gather_qkv", "qkv@0", "own@0", "src@0", "gate_s@0", "qs@0", "qx@0", 7, 2, L, C, BF),
          ("mdm_attn_fwd", "qs@0", None, None, "out@4", None, None, None, 2, L, 0, H, D, BF),
          ("mdm_ctrl_mix_kv", "kvc@0", "own@0", "src@0", "M@0", LD, "D@0", "mask@0", "gate_c@0", "kv_a@0", "kv_b@0", 7, 2, S, C,
           BF),
          ("mdm_attn_cross_bias", "qx@0", "kv_a@0", "tmp", "zero@0", LD, "out@4", C, "out@4", 2, L, S, H, D, BF),
          ("mdm_attn_cross_bias", "qkv@4", "kv_b@0", "mask@4", "zero@0", LD, "out@4", C, "out@4", 2, L, S, H, D, BF)]
CONTROLLED_PAG_1 = LEAD + EDITED + [("mdm_attn_cross_addv", "qkv@6", "kvc@6", "mask@6", "out@6", 1, L, S, H, D, BF)]
CONTROLLED_TAIL = (LEAD + [("mdm_attn_fwd", "qkv@6", "kvc@6", "mask@6", "out@6", "tmp", None, None, 1, L, S, H, D, BF)]
                   + EDITED)
CONTROLLED_NO_TEXT = [("mdm_attn_fwd", "qkv@0", None, None, "out@0", None, None, None, 4, L, 0, H, D, BF),
                      EDITED[0],
                      EDITED[1],
                      ("mdm_attn_cross_addv", "qkv@6", None, None, "out@6", 1, L, 0, H, D, BF)]
CONTROLLED_ROW0_0 = [("mdm_ctrl_gather_qkv", "qkv@0", "own@0", "src@0", "gate_s@0", "qs@0", "qx@0", 2, 2, L, C, BF),
                     ("mdm_attn_fwd", "qs@0", None, None, "out@0", None, None, None, 2, L, 0, H, D, BF),
                     ("mdm_ctrl_mix_kv", "kvc@0", "own@0", "src@0", "M@0", LD, "D@0", "mask@0", "gate_c@0", "kv_a@0", "kv_b@0",
                      2, 2, S, C, BF),
                     ("mdm_attn_cross_bias", "qx@0", "kv_a@0", "tmp", "zero@0", LD, "out@0", C, "out@0", 2, L, S, H, D, BF),
                     ("mdm_attn_cross_bias", "qkv@0", "kv_b@0", "mask@0", "zero@0", LD, "out@0", C, "out@0", 2, L, S, H, D, BF)]


def test_attention_and_attention_pag(recorded):
    from mdm_hip import ops

    _, qkv, kvc, mask = _case()
    with torch.no_grad():
        for fn, want in ((lambda: ops.attention(qkv, kvc, mask, H), FWD_ALL),
                         (lambda: ops.attention_pag(qkv, kvc, mask, H, 1), PAG_1),
                         (lambda: ops.attention_pag(qkv, kvc, mask, H, N), PAG_N)):
            plain = fn()
            out, rec = recorded(fn)
            assert rec.labelled(qkv=qkv, kvc=kvc, mask=mask, out=out) == want
            assert torch.equal(out, plain)


def test_attention_biased(recorded):
    from mdm_hip import ops

    _, qkv, kvc, mask = _case()
    bias = torch.randn(N, L, LD, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        for rows, want in ((0, BIASED_0), (1, BIASED_1), (N, BIASED_N)):
            fn = lambda: ops.attention_biased(qkv, kvc, mask, bias, H, pag_rows=rows)
            plain = fn()
            out, rec = recorded(fn)
            assert rec.labelled(qkv=qkv, kvc=kvc, mask=mask, bias=bias, out=out) == want
            assert torch.equal(out, plain)


def test_attention_controlled(recorded):
    """a perturbed tail, the same tail as ordinary rows, no text keys, and the edited rows alone (row0 = 0, no tail); every
    setting under all four gate combinations: the gates are device values, the launches do not see them.  The last layout is
    none the model produces -- sources always lead the batch: each row is its own source and the handle's host copy of the
    sources is emptied, which leaves the sources' check nothing to refuse; it is here for the empty lead and the empty tail.
    A 4-D qkv gives the same launches and an [N, L, C] output."""
    from mdm_hip import ops

    case, qkv, kvc, mask = _case()
    alone = dict(case, row0=0, own=[0, 1], src=[0, 1])
    q2, k2, m2 = (t[4:6].contiguous() for t in (qkv, kvc, mask))
    settings = ((case, (qkv, kvc, mask), 1, CONTROLLED_PAG_1), (case, (qkv, kvc, mask), 0, CONTROLLED_TAIL),
                (case, (qkv, None, None), 1, CONTROLLED_NO_TEXT), (alone, (q2, k2, m2), 0, CONTROLLED_ROW0_0))
    with torch.no_grad():
        for cs, (q, k, m), pag_rows, want in settings:
            for g_c, g_s in ((0, 0), (1, 0), (0, 1), (1, 1)):
                rows = AC.Rows(cs, g_c, g_s, DEV)
                if cs is alone:
                    rows.src_host = ()   # the host copy exists for the check that the sources lead the batch: there are none
                fn = lambda: ops.attention_controlled(q, k, m, H, rows, pag_rows=pag_rows)
                plain = fn()   # (also makes the cached zero bias before the recorded call)
                out, rec = recorded(fn)
                zero = _zero(2) if k is not None else None
                got = rec.labelled(qkv=q, kvc=k, mask=m, out=out, zero=zero, **_rows_operands(rows))
                assert got == want, (pag_rows, g_c, g_s)
                assert torch.equal(out, plain)
        rows = AC.Rows(case, 1, 1, DEV)
        out4, rec = recorded(lambda: ops.attention_controlled(qkv.reshape(N, 8, 10, 3 * C), kvc, mask, H, rows, pag_rows=1))
        got = rec.labelled(qkv=qkv, kvc=kvc, mask=mask, out=out4, zero=_zero(2), **_rows_operands(rows))
        assert got == CONTROLLED_PAG_1 and tuple(out4.shape) == (N, L, C)
        assert torch.equal(out4, ops.attention_controlled(qkv, kvc, mask, H, rows, pag_rows=1))


# ---- SelfAttention.forward under each switch ----------------------------------------------------------------------------
class _Bias:
    def __init__(self, t):
        self.t = t

    def bias(self, N, H, W):
        return self.t


class _Ctrl:
    def __init__(self, rows):
        self.r = rows

    def rows(self, N, L, kvc):
        return self.r


class _Rec:
    def __init__(self):
        self.seen = []

    def record(self, qkv, kvc, cond_mask, heads, bias, N, H, W):
        self.seen.append(bias)


def test_self_attention_forward_issues_the_dispatchers_launches(recorded, monkeypatch):
    """a layer of the mini UNet that has text keys, N = 7 at 4 x 4 queries and 5 tokens: no switch, each switch alone and
    with perturbed rows, and control together with a bias -- the control wins, the recorder is still handed the bias"""
    from mdm_hip import ops, unet

    model = PC.build_module("mini_unet")[0].to(DEV).eval()
    layer = next(m for m in model.modules() if isinstance(m, unet.SelfAttention) and m.cond_dim)
    heads, Cl, Sl, side = layer.num_heads, layer.channels, 5, 4
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, side, side, Cl, generator=g).to(DEV)
    cond = torch.randn(N, Sl, layer.cond_dim, generator=g).to(DEV)
    mask = torch.ones(N, Sl)
    mask[3, 2:] = 0
    mask = mask.to(DEV)
    ld = AC.ld_of(Sl)
    bias = torch.randn(N, side * side, ld, generator=g).to(DEV)
    rows = AC.Rows(dict(row0=4, own=[4, 5], src=[2, 3], M=torch.randn(2, Sl, ld, generator=g) * 0.3,
                        D=torch.rand(2, Sl, generator=g)), 1, 1, DEV)
    note = _Rec()
    by_hand = {
        "plain": lambda q, k, m: ops.attention(q, k, m, heads),
        "pag": lambda q, k, m: ops.attention_pag(q, k, m, heads, 1),
        "biased": lambda q, k, m: ops.attention_biased(q, k, m, bias, heads, pag_rows=0),
        "biased_pag": lambda q, k, m: ops.attention_biased(q, k, m, bias, heads, pag_rows=1),
        "controlled": lambda q, k, m: ops.attention_controlled(q, k, m, heads, rows, pag_rows=1),
        "controlled_tail": lambda q, k, m: ops.attention_controlled(q, k, m, heads, rows, pag_rows=0),
    }
    cases = (({}, "plain"), ({"_pag_rows": 1}, "pag"), ({"_cross_bias": _Bias(bias)}, "biased"),
             ({"_cross_bias": _Bias(bias), "_pag_rows": 1}, "biased_pag"),
             ({"_attn_ctrl": _Ctrl(rows), "_pag_rows": 1}, "controlled"),
             ({"_attn_ctrl": _Ctrl(rows)}, "controlled_tail"),
             ({"_attn_ctrl": _Ctrl(rows), "_cross_bias": _Bias(bias), "_attn_rec": note, "_pag_rows": 1}, "controlled"))
    seen, depth = [], [0]
    for name in DISPATCHERS:   # whichever of them the layer calls: note the outermost call's tensors and what it returns
        def spy(*a, _real=getattr(ops, name), **kw):
            depth[0] += 1
            try:
                out = _real(*a, **kw)
            finally:
                depth[0] -= 1
            if depth[0] == 0:
                seen.append((a[0], a[1], a[2], out))
            return out

        monkeypatch.setattr(ops, name, spy)
    with torch.no_grad():
        for switches, hand in cases:
            with unet.switched([(layer, switches)]):
                layer(x, cond, mask)   # (makes the cached zero bias before the recorded call)
                del seen[:]
                _, rec = recorded(lambda: layer(x, cond, mask))
            (q, k, m, out), = seen
            zero = ops._CTRL_ZERO.get((torch.device(DEV), 2, side * side, (Sl + 3) // 4 * 4))
            operands = dict(qkv=q, kvc=k, mask=m, bias=bias, zero=zero, **_rows_operands(rows))
            got = rec.labelled(out=out, **operands)
            want_out, rec2 = recorded(lambda: by_hand[hand](q, k, m))
            want = rec2.labelled(out=want_out, **operands)
            assert got == want and len(got) >= 1, (sorted(switches), hand)
            assert ("bias@0" in str(got)) == hand.startswith("biased")
            assert torch.equal(out.reshape(want_out.shape), want_out)
    assert len(note.seen) == 2 and all(b is bias for b in note.seen)
