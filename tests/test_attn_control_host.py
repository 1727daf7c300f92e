"""CPU: prompt-to-prompt attention control -- the torch restatements of the two kernels against fp64, the fp64 layer formula
against the oracle's own attention layer, ``AttnControl`` (validation, ``aligned``, gates), the switch, the samplers on a
recording stub (the gates follow both intervals step by step, nothing is held across a yield, only the conditional block is
controlled), every refused pair, ``Inverted.repeat``, and the condition that keeps the GPU parity test from being vacuous: the
controlled oracle moves the edited rows."""
import ctypes

import pytest
import torch

import attn_control_cases as AC
import parity_cases as PC
import unet_oracle as O

EPS32 = 2.0 ** -24


# ---- the kernels in torch ops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,R", [(1, 32, 1), (5, 96, 3), (77, 32, 2)], ids=str)
def test_torch_mix_kv_and_gather_agree_with_fp64(S, C, R):
    """fp32 rounding: |err| <= (S + 2) eps32 sum_j |M_ij v_j| for the accumulated half (S FMAs and one store), bit equality
    for the copied halves and for both gate-0 outputs"""
    from mdm_hip import attn_control as A

    c = AC.mix_case(S, C, R)
    for mask in (c["mask"], None):
        M = c["M"] if mask is not None else torch.nan_to_num(c["M"].clamp(max=4.0), nan=0.0)   # (no mask: no 1e30 column is skipped)
        for gate in (1.0, 0.0):
            a, b = A.mix_kv(c["kvc"], c["own"], c["src"], M, c["D"], mask, gate)
            ra, rb = AC.mix_kv_ref(c["kvc"], c["own"], c["src"], M, c["D"], mask, gate)
            assert torch.equal(a[..., :C], c["kvc"][c["src"]][..., :C]) and torch.equal(b[..., :C], c["kvc"][c["own"]][..., :C])
            if gate == 0:
                assert not a[..., C:].any() and torch.equal(b[..., C:], c["kvc"][c["own"]][..., C:])
                continue
            live = torch.ones(R, S, dtype=torch.bool) if mask is None else mask[c["own"]] != 0
            Mabs = torch.where(live[:, None, :], M[:, :, :S].double().abs(), torch.zeros(R, S, S, dtype=torch.float64))
            bound = (S + 2) * EPS32 * torch.einsum("rij,rjc->ric", Mabs, c["kvc"][c["own"]][..., C:].double().abs())
            assert torch.isfinite(a).all() and bool(((a[..., C:].double() - ra[..., C:]).abs() <= bound + 1e-30).all())
            assert bool(((b[..., C:].double() - rb[..., C:]).abs() <= 2 * EPS32 * rb[..., C:].abs() + 1e-30).all())
    qkv = torch.randn(4, 16, 3 * C, generator=torch.Generator().manual_seed(S))
    for gate in (0.0, 1.0):
        qs, qx = A.gather_qkv(qkv, [2, 3], [0, 1], gate)
        sel = [0, 1] if gate else [2, 3]
        assert torch.equal(qs[..., :2 * C], qkv[sel][..., :2 * C]) and torch.equal(qs[..., 2 * C:], qkv[[2, 3]][..., 2 * C:])
        assert torch.equal(qx[..., :C], qkv[[0, 1]][..., :C])


def test_fp64_layer_with_both_gates_off_is_the_oracles_layer():
    """1e-5 rel-L2, the tenth-of-gate bound of test_regions_gpu for the same kind of restatement: with g_c = g_s = 0 the
    formula is A(r) v[r] + P(r) v_c[r]"""
    for name in ("mini_unet", "mini_unet_masked", "mini_nested"):
        plain, off = AC.oracle_outputs(name, None), AC.oracle_outputs(name, (0.0, 0.0))
        for p, o in zip(plain, off):
            err = O.rel_l2(o, p)
            print("%s: gates off against the oracle's own layer %.2e" % (name, err))
            assert err < 1e-5 and torch.equal(o[:2], p[:2])


@pytest.mark.parametrize("name", ["mini_unet", "mini_unet_masked", "mini_nested"])
def test_controlled_oracle_moves_the_edited_rows(name):
    """what keeps the GPU parity test from being vacuous: each gate alone, and both, move rows 2 and 3 of every output by
    more than 10 x 1e-4 rel-L2 from the uncontrolled oracle; rows 0 and 1, the sources, do not move by a bit"""
    plain = AC.oracle_outputs(name, None)
    for gates in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
        for i, (o, p) in enumerate(zip(AC.oracle_outputs(name, gates), plain)):
            moved = O.rel_l2(o[2:], p[2:])
            print("%s gates %s out %d: the control moves the edited rows by %.3e" % (name, gates, i, moved))
            assert moved > 10 * 1e-4 and torch.equal(o[:2], p[:2])


# ---- AttnControl ------------------------------------------------------------------------------------------------------------
def test_aligned_builds_the_stated_matrices():
    import mdm_hip

    S = 6
    c = mdm_hip.AttnControl.aligned(S, [0, 1, 0, 1], {2: [(0, 0), (1, 3), (4, 2)], 3: []},
                                    scale={2: torch.tensor([1.0, 2.0, 1.0, 1.0, 0.5, 3.0])})
    assert (c.rows, c.G, c.R, c.ld, c.source) == (4, 2, 2, 8, (0, 1, 0, 1))
    m = torch.zeros(S, S)
    m[0, 0], m[3, 1], m[2, 4] = 1.0, 2.0, 0.5                     # mapper[src, edit] * scale[edit]
    assert torch.equal(c.M[0, :, :S], m) and not c.M[:, :, S:].any()
    assert torch.equal(c.D[0], torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0, 3.0]))   # keep = 1 on the tokens in no pair, x scale
    assert not c.M[1].any() and torch.equal(c.D[1], torch.ones(S))              # no pairs: the edit keeps all its own attention
    # the list form, and the defaults: identity mapper, keep 0, scale 1
    d = mdm_hip.AttnControl.aligned(S, [0, 0], [None, [(j, j) for j in range(S)]])
    e = mdm_hip.AttnControl(S, [0, 0])
    assert torch.equal(d.M, e.M) and torch.equal(d.D, e.D) and torch.equal(e.M[0, :, :S], torch.eye(S)) and not e.D.any()
    with pytest.raises(ValueError, match="pair"):
        mdm_hip.AttnControl.aligned(S, [0, 0], {1: [(0, S)]})
    with pytest.raises(ValueError, match="edit token, source token"):
        mdm_hip.AttnControl.aligned(S, [0, 0], {1: [3]})


def test_every_validation_error():
    import mdm_hip

    A = mdm_hip.AttnControl
    ok = dict(S=4, source=[0, 0])
    bad = [
        (dict(S=0), "tokens"),
        (dict(source=[]), "non-empty"),
        (dict(source=3), "list of row indices"),
        (dict(source=[0, 0.5]), "row indices"),
        (dict(source=[0, 2]), "outside"),
        (dict(source=[1, 1, 2]), "all sources come before"),      # row 0 edits row 1: edits in front of a source
        (dict(source=[0, 0, 1]), "must itself be a source"),      # row 2 edits row 1, which is an edit
        (dict(mapper={1: torch.zeros(4, 3)}), "mapper"),
        (dict(mapper={0: torch.eye(4)}), "not an edited row"),
        (dict(mapper=[None]), "entries"),
        (dict(keep={1: torch.zeros(5)}), "keep"),
        (dict(scale={1: torch.tensor([1.0, float("nan"), 1.0, 1.0])}), "not finite"),
        (dict(keep={1: [0, 0, 0, 0]}), "keep"),
        (dict(cross_interval=(0.5, 0.2)), "cross_interval"),
        (dict(self_interval=0.5), "self_interval"),
        (dict(self_interval=(0.0, float("inf"))), "self_interval"),
        (dict(cross_layers=3), "cross_layers"),
        (dict(self_layers=None), "self_layers"),
        (dict(self_max_queries=-1), "self_max_queries"),
        (dict(self_max_queries=2.5), "self_max_queries"),
    ]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            A(**dict(ok, **change))
    assert "source[r] == r" in str(pytest.raises(ValueError, A, 4, [1, 1, 2]).value)   # the message says how to order the rows
    c = A(**ok)
    assert c.gates(200, 1000) == (1.0, 0.0) and c.gates(199, 1000) == (0.0, 0.0) and c.gates(600, 1000) == (1.0, 1.0)
    assert c.gates(1000, 1000) == (1.0, 1.0) and A(4, [0, 0], cross_interval=(0, 0.5)).gates(501, 1000) == (0.0, 0.0)


def test_handles_layouts_and_the_switch():
    import mdm_hip
    from mdm_hip import attn_control as A
    from mdm_hip.unet import SWITCHES, SelfAttention

    assert SelfAttention._attn_ctrl is None and "_attn_ctrl" in SWITCHES
    c = AC.model_control()
    M, D = AC.model_tables()
    assert torch.equal(c.M[:, :, :8].double(), M) and torch.equal(c.D.double(), D)   # the module and the cases agree on M, D
    for guidance, pag, total, row0, src in ((False, False, 4, 2, (0, 1)), (True, False, 8, 6, (4, 5)), (True, True, 12, 6, (4, 5)),
                                            (False, True, 8, 2, (0, 1))):
        h = c.rows_for(guidance, pag)
        assert (h.total, h.row0, h.R, h.src_host) == (total, row0, 2, src) and h is c.rows_for(guidance, pag)
        assert h.own.tolist() == [row0, row0 + 1] and h.src.tolist() == list(src) and h.own.dtype == torch.int32
        assert h is not c.rows_for(guidance, pag, cached=False)
    m = PC.build_module("mini_nested")[0]
    layers = {n: mod for n, mod in m.named_modules() if isinstance(mod, SelfAttention)}
    text = {n for n, mod in layers.items() if mod.cond_dim}
    cross, self_ = c.layer_sets(m)
    assert set(cross) == text and set(self_) == set(layers)
    h = c.rows_for()
    with A.applied(m, h, c):
        for n, mod in layers.items():
            lc = mod._attn_ctrl
            assert lc.handle is h and lc.self_ and lc.cross == (n in text)
        # the rows of a layer: the threshold of the self gate, the text keys of the cross gate, the batch it was made for
        lc = next(mod._attn_ctrl for n, mod in layers.items() if n in text)
        kvc = torch.zeros(4, 8, 4)
        r = lc.rows(4, 64, kvc)
        assert r.gate_c is h.gate_c and r.gate_s is h.gate_s and (r.row0, r.R, r.src_host) == (2, 2, (0, 1))
        assert lc.rows(4, 65, kvc).gate_s is h.zero and lc.rows(4, 64, None).gate_c is h.zero and float(h.zero) == 0
        with pytest.raises(ValueError, match="mixed-resolution"):
            lc.rows(3, 64, kvc)
        with pytest.raises(ValueError, match="tokens"):
            lc.rows(4, 64, torch.zeros(4, 9, 4))
    assert all(mod._attn_ctrl is None and "_attn_ctrl" not in mod.__dict__ for mod in layers.values())
    mid = mdm_hip.AttnControl(8, AC.SOURCE, cross_layers="mid", self_layers=lambda n: False)
    with pytest.raises(ValueError, match="selects no attention layer"):
        mid.layer_sets(m)
    part = mdm_hip.AttnControl(8, AC.SOURCE, cross_layers="mid", self_layers=["inner_unet.up_blocks.0.attn.1"])
    with A.applied(m, part.rows_for(), part):
        on = {n: (mod._attn_ctrl.cross, mod._attn_ctrl.self_) for n, mod in layers.items() if mod._attn_ctrl is not None}
    assert on == {"inner_unet.mid_blocks.0.attn.0": (True, False), "inner_unet.up_blocks.0.attn.1": (False, True)}
    with pytest.raises(ValueError, match="BatchCtrl"):
        A.applied(m, object(), c)
    assert len(m.state_dict()) == len(PC.build_module("mini_nested")[2])


# ---- the samplers on a recording stub ---------------------------------------------------------------------------------------
B, S, D = 2, 5, 8


def _sampler(nested=False):
    from mdm_hip import samplers as SM

    cfg = SM.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP")
    return (SM.NestedSampler if nested else SM.Sampler)(cfg)


def _inputs(w, nested=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = 2 * B if w != 1 else B
    lm = torch.randn(rows, S, D, generator=g)
    mask = (torch.rand(rows, S, generator=g) < 0.7).float()
    x = [torch.randn(B, 3, 8, 8, generator=g) for _ in range(2)] if nested else torch.randn(B, 3, 8, 8, generator=g)
    return x, lm, mask, {}


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("w,pag_scale", [(2.0, 0.0), (1, 0.0), (2.0, 1.5), (1, 1.5)])
def test_stub_sees_the_handle_and_the_gates_of_every_step(w, pag_scale, nested):
    import mdm_hip

    smp, stub = _sampler(nested), AC.RecordingStub(nested)
    x, lm, mask, micros = _inputs(w, nested)
    ctl = mdm_hip.AttnControl(S, [0, 0], cross_interval=(0.3, 1.0), self_interval=(0.7, 1.0), cross_layers="all",
                              self_layers=["down_blocks.0.attn.1", "mid_blocks.0.attn.0"])
    n = 5
    kw = dict(resample_steps=True, num_inference_steps=n, ddim_eta=0, guidance_scale=w, pag_scale=pag_scale)
    steps = [int(t) for t in smp.set_timesteps(n)[:-1]]
    assert len({ctl.gates(t, 1000) for t in steps}) == 3   # the schedule crosses both thresholds
    idle = lambda: all(m._attn_ctrl is None for m in stub.attention().values())
    gen = smp.sample(stub, x, lm, mask, micros, control=ctl, yield_output=True, **kw)
    assert idle() and not stub.seen
    for k, _ in enumerate(gen, 1):
        assert idle() and len(stub.seen) == min(k, n)   # between the items of the generator: nothing is held across a yield
    assert len(stub.seen) == n
    # only the conditional block is controlled: its second row, an edit of its first; never a row of the other two blocks
    base = B if w != 1 else 0
    total = (1 + (w != 1) + bool(pag_scale)) * B
    for t, seen in zip(steps, stub.seen):
        gc, gs = ctl.gates(t, 1000)
        rows = (base + 1, 1, (base,), total, gc, gs)
        assert seen == {"mid_blocks.0.attn.0": (True, True) + rows, "down_blocks.0.attn.0": (True, False) + rows,
                        "down_blocks.0.attn.1": (False, True) + rows}
    assert all(c["pag_rows"] == (B if pag_scale else 0) for c in stub.calls)
    # control=None is the call without the keyword; so is a control whose rows are all sources (the stub ignores the handle,
    # so every call here returns the same images)
    stub.seen.clear()
    a = smp.sample(stub, x, lm, mask, micros, control=None, **kw)
    b = smp.sample(stub, x, lm, mask, micros, **kw)
    c = smp.sample(stub, x, lm, mask, micros, control=mdm_hip.AttnControl(S, [0, 1], cross_layers="not even resolved"), **kw)
    assert all(v is None for s in stub.seen for v in s.values()) and len(stub.seen) == 3 * n
    d = smp.sample(stub, x, lm, mask, micros, control=ctl, **kw)
    for u, v, o, p in zip(*(t if nested else [t] for t in (a, b, c, d))):
        assert torch.equal(u, v) and torch.equal(u, o) and torch.equal(u, p)
    # an exception in the denoiser leaves no handle behind
    stub.forward = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        smp.sample(stub, x, lm, mask, micros, control=ctl, **kw)
    assert idle()


def test_refusals():
    import mdm_hip
    from mdm_hip import LossGuide
    from mdm_hip.samplers import AttendExcite, MapGuide, SampleOptions, Sampler

    smp, stub = _sampler(), AC.RecordingStub()
    x, lm, mask, micros = _inputs(2.0)
    ctl = mdm_hip.AttnControl(S, [0, 0])
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    guide = LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    pairs = [
        (dict(guide=guide), "no backward"),
        (dict(map_guide=MapGuide(AttendExcite([1]), scale=1.0)), "source's maps"),
        (dict(regions=mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)), "biased probabilities"),
        (dict(tiles=mdm_hip.Tiles(8)), "windows"),
    ]
    for more, match in pairs:
        with pytest.raises(NotImplementedError, match=match):
            smp.sample(stub, x, lm, mask, micros, control=ctl, **more, **kw)
        with pytest.raises(NotImplementedError, match=match):
            smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, control=ctl, **more)
    assert {p for p in SampleOptions.REFUSED if "control" in p} == {("control", "guide"), ("control", "map_guide"),
                                                                    ("control", "regions"), ("control", "tiles")}
    with pytest.raises(ValueError, match="AttnControl"):
        smp.sample(stub, x, lm, mask, micros, control="swap", **kw)
    with pytest.raises(ValueError, match="rows"):
        smp.sample(stub, x, lm, mask, micros, control=mdm_hip.AttnControl(S, [0, 0, 0]), **kw)
    with pytest.raises(ValueError, match="selects no attention layer"):
        smp.sample(stub, x, lm, mask, micros, control=mdm_hip.AttnControl(S, [0, 0], cross_layers=lambda n: False), **kw)
    # inversion takes no control
    assert "control" in Sampler.INVERSION_REFUSED
    img = torch.zeros(B, 3, 8, 8)
    for fn in (smp.invert, smp.noise_maps):
        with pytest.raises(NotImplementedError, match="does not take control="):
            fn(stub, img, lm, mask, micros, num_inference_steps=2, resample_steps=True, guidance_scale=2.0, control=ctl)
    assert not stub.calls and SampleOptions().control is None


def test_ops_are_inference_only_gpu_only_and_declared():
    from mdm_hip import _lib, ops

    qkv, kvc = torch.randn(2, 16, 96), torch.randn(2, 3, 64)
    one, idx = torch.ones(1), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.MdmHipError, match="MI355X"):
        ops.attention_controlled(qkv, kvc, None, 1, AC.Rows(dict(row0=1, own=[1], src=[0], M=torch.zeros(1, 3, 4),
                                                                 D=torch.zeros(1, 3)), 1, 1, "cpu"))
    with pytest.raises(_lib.MdmHipError, match="MI355X"):
        ops.ctrl_mix_kv(kvc, idx, idx, torch.zeros(1, 3, 4), torch.zeros(1, 3), None, one)
    with pytest.raises(_lib.MdmHipError, match="MI355X"):
        ops.ctrl_gather_qkv(qkv, idx, idx, one)
    protos = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert protos["mdm_ctrl_mix_kv"][1] == ["kvc", "own_rows", "src_rows", "M", "m_ld", "D", "mask", "gate", "kv_a", "kv_b", "N",
                                            "R", "S", "C", "dtype", "stream"]
    assert protos["mdm_ctrl_gather_qkv"][1] == ["qkv", "own_rows", "src_rows", "gate", "qkv_self", "q_src", "N", "R", "L", "C",
                                                "dtype", "stream"]
    assert len(_lib.header_prototypes()) == 85 and _lib.ABI_VERSION == 6   # the drop-in header is as it was
    assert "attn_control.hip" in _lib.SOURCES
    # argument checks come before any launch
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    p, q, r = (ctypes.c_void_p(at + 1024 * i) for i in range(3))
    ok = dict(kvc=p, own_rows=p, src_rows=p, M=p, m_ld=8, D=p, mask=None, gate=p, kv_a=q, kv_b=r, N=2, R=1, S=5, C=32, dtype=0,
              stream=None)
    bad = [dict(kvc=None), dict(own_rows=None), dict(src_rows=None), dict(M=None), dict(D=None), dict(gate=None), dict(kv_a=None),
           dict(kv_b=None), dict(m_ld=4), dict(m_ld=6), dict(R=0), dict(S=0), dict(C=30), dict(dtype=2), dict(dtype=7), dict(kv_b=q),
           dict(kv_a=p), dict(kvc=ctypes.c_void_p(at + 4)), dict(dtype=1, C=36)]
    for change in bad:
        args = dict(ok, **change)
        assert L.mdm_ctrl_mix_kv(*[args[k] for k in protos["mdm_ctrl_mix_kv"][1]]) < 0, change
    ok = dict(qkv=p, own_rows=p, src_rows=p, gate=p, qkv_self=q, q_src=r, N=2, R=1, L=16, C=32, dtype=0, stream=None)
    bad = [dict(qkv=None), dict(gate=None), dict(qkv_self=None), dict(q_src=None), dict(R=0), dict(L=0), dict(C=30), dict(dtype=2),
           dict(q_src=q), dict(qkv_self=p), dict(q_src=ctypes.c_void_p(at + 2048 + 8))]
    for change in bad:
        args = dict(ok, **change)
        assert L.mdm_ctrl_gather_qkv(*[args[k] for k in protos["mdm_ctrl_gather_qkv"][1]]) < 0, change


def test_inverted_repeat_orders_rows_by_block():
    from mdm_hip.diffusion import Inverted

    x = torch.arange(2 * 3.0).reshape(2, 3, 1, 1)
    z = [[x + 10, x[:, :, :1] + 20], None, [x + 30, x + 40]]
    inv = Inverted("ddpm", [x, x + 1], 700, z, num_inference_steps=3, ddim_eta=1.0)
    rep = inv.repeat(3)
    blocks = lambda t: torch.cat([t, t, t])
    assert torch.equal(rep.x_t[0], blocks(x)) and torch.equal(rep.x_t[1], blocks(x + 1)) and rep.x_t[0].shape[0] == 6
    assert rep.step_noise[1] is None and torch.equal(rep.step_noise[0][1], blocks(z[0][1]))
    assert torch.equal(rep.step_noise[2][0], blocks(x + 30))
    assert (rep.method, rep.t, rep.num_inference_steps, rep.ddim_eta, rep.resample_steps) == ("ddpm", 700, 3, 1.0, True)
    assert inv.x_t[0].shape[0] == 2 and inv.step_noise[0][0].shape[0] == 2   # the record itself is unchanged
    one = Inverted("ddim", x, 500, None, num_inference_steps=4).repeat(2)
    assert torch.equal(one.x_t, torch.cat([x, x])) and one.step_noise is None
    assert torch.equal(Inverted("ddim", x, 500).repeat(1).x_t, x)
    for n in (0, 1.5, True):
        with pytest.raises(ValueError, match="repeat"):
            inv.repeat(n)
