"""GPU: prompt-to-prompt attention control on the HIP path -- mdm_ctrl_mix_kv and mdm_ctrl_gather_qkv against fp64 and their
exact identities, ``ops.attention_controlled`` against the fp64 layer of tests/attn_control_cases.py (per-kernel gates of DESIGN
section 3), the mini models against the oracle with the same layers controlled in all four gate combinations, and the
samplers: eager equals graphed bit for bit, other tables and intervals replay the one graph, ``control=None`` and a control
without edits change no bit."""
import functools

import pytest
import torch

import attn_control_cases as AC
import parity_cases as PC
import test_pag_gpu as TP
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = {"fp32": 2e-5, "split": 2e-5, "bf16": 3e-2}   # max-abs over max-abs
MODES = list(GATE)
MIX_CASES = [(1, 32, 1), (5, 96, 3), (77, 288, 3), (130, 384, 2), (32, 1024, 3)]   # (S, C, R)
GATHER_CASES = [(16, 32), (80, 288), (256, 384)]                                   # (L, C)
LAYER_CASES = [(32, 3, 80, 5), (64, 1, 256, 77), (96, 3, 80, 130), (128, 3, 16, 130)]   # (d, H, L, S): every head dimension
GATES = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)]

_dtype, maxerr = TP._dtype, TP.maxerr


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _gate(v):
    return torch.full((1,), float(v), device=DEV)


def _mix(c, dt, gate, masked=True, rows=None, M=None, D=None, kvc=None):
    from mdm_hip import ops

    rows = range(len(c["own"])) if rows is None else rows
    M = c["M"] if M is None else M
    D = c["D"] if D is None else D
    kvc = c["kvc"].to(DEV, dt) if kvc is None else kvc
    sel = list(rows)
    return ops.ctrl_mix_kv(kvc, _i32([c["own"][k] for k in sel]), _i32([c["src"][k] for k in sel]), M[sel].to(DEV).contiguous(),
                           D[sel].to(DEV).contiguous(), c["mask"].to(DEV) if masked else None, _gate(gate))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S,C,R", MIX_CASES, ids=str)
def test_mix_kv_matches_fp64(S, C, R, dt):
    """fp32 and bf16 tensors, gate 0 and 1, with and without a mask; NaN in the pad columns of M and 1e30 in the columns of
    masked edit tokens (without the mask those columns hold ordinary values: nothing is skipped then)"""
    c = AC.mix_case(S, C, R)
    t = _dtype(dt)
    seen = dict(c, kvc=c["kvc"].to(t).float())   # the values the kernel sees
    for masked in (True, False):
        M = c["M"] if masked else torch.where(c["M"] > 1e29, torch.full_like(c["M"], 0.25), c["M"])
        for gate in (0.0, 1.0):
            a, b = _mix(c, t, gate, masked, M=M)
            ra, rb = AC.mix_kv_ref(seen["kvc"], c["own"], c["src"], M, c["D"], c["mask"] if masked else None, gate)
            assert a.dtype == t and tuple(a.shape) == (R, S, 2 * C) and torch.isfinite(a).all() and torch.isfinite(b).all()
            ea, eb = maxerr(a, ra), maxerr(b, rb)
            print("S=%d C=%d R=%d %s mask=%s gate=%d: kv_a %.2e, kv_b %.2e" % (S, C, R, dt, masked, gate, ea, eb))
            assert ea < GATE[dt] and eb < GATE[dt]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_mix_kv_exact_identities(dt):
    """bit for bit: the k_c halves; gate 0 gives zeros and v_c; a permutation M with D = 0 gives permuted v_c rows and zeros;
    small-integer M and v_c give the exact sums; pad and masked columns holding NaN or 1e30 leave no trace; R = 1 equals the
    same row inside R = 3; a base pointer offset by 16 bytes gives the same result"""
    t = _dtype(dt)
    for S, C, R in ((5, 96, 3), (77, 288, 3), (130, 384, 3)):
        c = AC.mix_case(S, C, R)
        kvc = c["kvc"].to(DEV, t)
        own, src = c["own"], c["src"]
        a, b = _mix(c, t, 1.0)
        assert torch.equal(a[..., :C], kvc[src][..., :C]) and torch.equal(b[..., :C], kvc[own][..., :C])
        a0, b0 = _mix(c, t, 0.0)
        assert torch.equal(a0[..., :C], a[..., :C]) and not a0[..., C:].any() and torch.equal(b0, kvc[own])
        # pad and masked columns: other junk in them, the same bits out
        junk = c["M"].clone()
        junk[:, :, S:] = 1e30
        for k in range(R):
            junk[k][:, :S][:, c["mask"][own[k]] == 0] = float("nan")
        ja, jb = _mix(c, t, 1.0, M=junk)
        assert torch.equal(ja, a) and torch.equal(jb, b)
        # a row's bits do not depend on R
        for k in range(R):
            a1, b1 = _mix(c, t, 1.0, rows=[k])
            assert torch.equal(a1[0], a[k]) and torch.equal(b1[0], b[k])
        # every input 16 bytes further on
        def shifted(x):
            n = 16 // x.element_size()
            buf = torch.empty(x.numel() + n, dtype=x.dtype, device=DEV)
            buf[n:].copy_(x.reshape(-1))
            return buf[n:].view(x.shape)

        from mdm_hip import ops

        sa, sb = ops.ctrl_mix_kv(shifted(kvc), shifted(_i32(own)), shifted(_i32(src)), shifted(c["M"].to(DEV)),
                                 shifted(c["D"].to(DEV)), shifted(c["mask"].to(DEV)), _gate(1.0))
        assert torch.equal(sa, a) and torch.equal(sb, b)
        # a permutation with D = 0, no mask: V'[i] = v_c[perm[i]] and V'' = 0
        g = torch.Generator().manual_seed(S)
        perm = torch.randperm(S, generator=g)
        P = torch.zeros(R, S, c["ld"])
        P[:, torch.arange(S), perm] = 1.0
        P[:, :, S:] = float("nan")
        pa, pb = _mix(c, t, 1.0, masked=False, M=P, D=torch.zeros(R, S))
        assert torch.equal(pa[..., C:], kvc[own][:, perm, C:]) and not pb[..., C:].any()
        # small integers: sums below 2^8 in magnitude are exact in bf16 too
        Mi = torch.zeros(R, S, c["ld"])
        Mi[:, :, :S] = torch.randint(-1, 2, (R, S, S), generator=g).float() * (torch.rand(R, S, S, generator=g) < 4.0 / S)
        vi = torch.randint(-4, 5, (R + 1, S, C), generator=g).float()
        Di = torch.randint(0, 3, (R, S), generator=g).float()
        ki = torch.cat([c["kvc"][..., :C], vi], dim=-1).to(DEV, t)
        ia, ib = _mix(c, t, 1.0, masked=False, M=Mi, D=Di, kvc=ki)
        want = torch.einsum("rij,rjc->ric", Mi[:, :, :S].double(), vi[own].double())
        assert float(want.abs().max()) < 256
        assert torch.equal(ia[..., C:].double().cpu(), want) and torch.equal(ib[..., C:].double().cpu(), (vi[own] * Di[..., None]).double())


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("L,C", GATHER_CASES, ids=str)
def test_gather_qkv_is_indexing(L, C, dt):
    """0 differing elements, both gates; what q_src leaves undefined (its k and v columns) is not compared"""
    from mdm_hip import ops

    t = _dtype(dt)
    qkv = torch.randn(6, L, 3 * C, generator=torch.Generator().manual_seed(L + C)).to(DEV, t)
    own, src = [3, 4, 5], [1, 0, 1]
    for gate in (0.0, 1.0):
        qs, qx = ops.ctrl_gather_qkv(qkv, _i32(own), _i32(src), _gate(gate))
        sel = src if gate else own
        want = torch.cat([qkv[sel][..., :2 * C], qkv[own][..., 2 * C:]], dim=-1)
        assert int((qs != want).sum()) == 0 and int((qx[..., :C] != qkv[src][..., :C]).sum()) == 0
    # N = R = 1, a row that is its own source: a copy
    marker = torch.full((1, L, 3 * C), 7.0, device=DEV, dtype=t)
    qs, _ = ops.ctrl_gather_qkv(marker, _i32([0]), _i32([0]), _gate(1.0))
    assert torch.equal(qs, marker)


# ---- the layer ------------------------------------------------------------------------------------------------------------
def _layer(case, H, mode, g_c, g_s, masked=True):
    from mdm_hip import ops

    dt = _dtype(mode)
    with torch.no_grad(), ops.fp32_split(mode == "split"):
        return ops.attention_controlled(case["qkv"].to(DEV, dt), case["kvc"].to(DEV, dt), case["mask"].to(DEV) if masked else None,
                                        H, AC.Rows(case, g_c, g_s, DEV), pag_rows=case["pag_rows"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,H,L,S", LAYER_CASES, ids=str)
def test_attention_controlled_matches_the_fp64_layer(d, H, L, S, mode):
    """N = 7: 2 uncond, 2 sources (one with a holed mask), 2 edits (one with a holed mask and 1e30 in the M columns of its
    masked tokens), 1 perturbed; all four gate combinations; with the mask and without"""
    case = AC.layer_case(d, H, L, S)
    dt = _dtype(mode)
    seen = dict(case, qkv=case["qkv"].to(dt).float(), kvc=case["kvc"].to(dt).float())
    for masked in (True, False):
        cs = seen if masked else dict(seen, M=torch.where(seen["M"] > 1e29, torch.zeros_like(seen["M"]), seen["M"]))
        run = case if masked else dict(case, M=cs["M"])
        for g_c, g_s in GATES:
            out = _layer(run, H, mode, g_c, g_s, masked)
            want = AC.layer_ref(cs, H, g_c, g_s, masked)
            err = maxerr(out, want)
            print("d=%d H=%d L=%d S=%d %s mask=%s gates=(%d, %d): %.2e" % (d, H, L, S, mode, masked, g_c, g_s, err))
            assert torch.isfinite(out).all() and err < GATE[mode]


@pytest.mark.parametrize("mode", MODES)
def test_attention_controlled_identities(mode):
    """both gates 0: bit for bit the same launches issued by hand through the existing ops; the ordinary rows are those of
    ``ops.attention`` / ``ops.attn_cross_addv`` whatever the gates; an identity mapper with keep 0 on an edit that repeats its
    source's qkv, kvc and mask gives the source's output to the mode's gate; a layer without text keys; the checks"""
    from mdm_hip import _lib, ops

    dt = _dtype(mode)
    d, H, L, S = 64, 3, 80, 77
    C = H * d
    case = AC.layer_case(d, H, L, S, seed=3)
    qkv, kvc, mask = case["qkv"].to(DEV, dt), case["kvc"].to(DEV, dt), case["mask"].to(DEV)
    sl = lambda t, rows: t[rows].contiguous()
    with torch.no_grad(), ops.fp32_split(mode == "split"):
        lead = ops.attention(sl(qkv, slice(0, 4)), sl(kvc, slice(0, 4)), sl(mask, slice(0, 4)), H)
        tail = ops.attn_cross_addv(sl(qkv, slice(6, 7)), sl(kvc, slice(6, 7)), sl(mask, slice(6, 7)), H)
        zero = torch.zeros(2, L, case["ld"], device=DEV)
        base = ops.attention(sl(qkv, [4, 5]), None, None, H)
        kv_a = torch.cat([sl(kvc, [2, 3])[..., :C], torch.zeros(2, S, C, device=DEV, dtype=dt)], dim=-1)
        ops.attn_cross_bias(sl(qkv, [2, 3]), kv_a, sl(mask, [2, 3]), zero, H, base=base)
        ops.attn_cross_bias(sl(qkv, [4, 5]), sl(kvc, [4, 5]), sl(mask, [4, 5]), zero, H, base=base)
        off = _layer(case, H, mode, 0, 0)
        assert torch.equal(off[:4], lead) and torch.equal(off[6:], tail) and torch.equal(off[4:6], base)
        on = _layer(case, H, mode, 1, 1)
        assert torch.equal(on[:4], lead) and torch.equal(on[6:], tail) and not torch.equal(on[4:6], base)
        # gates off: the uncontrolled layer up to the rounding of another order of the same sums
        plain = ops.attention(sl(qkv, [4, 5]), sl(kvc, [4, 5]), sl(mask, [4, 5]), H)
        assert maxerr(off[4:6], plain) < GATE[mode]
        # a perturbed block that this layer does not perturb runs as ordinary rows
        keep = _layer(dict(case, pag_rows=0), H, mode, 1, 1)
        assert torch.equal(keep[:6], on[:6]) and torch.equal(keep[6:], ops.attention(sl(qkv, [6]), sl(kvc, [6]), sl(mask, [6]), H))
        # an edit that repeats its source, identity mapper, keep 0: the source's output
        twin = dict(case, qkv=case["qkv"].clone(), kvc=case["kvc"].clone(), mask=case["mask"].clone(), D=torch.zeros(2, S))
        for name in ("qkv", "kvc", "mask"):
            twin[name][4:6] = twin[name][2:4]
        eye = torch.zeros(2, S, case["ld"])
        eye[:, :, :S] = torch.eye(S)
        twin["M"] = eye
        same = _layer(twin, H, mode, 1, 1)
        err = maxerr(same[4:6], same[2:4])
        print("%s: an edit that repeats its source, against the source %.2e" % (mode, err))
        assert err < GATE[mode]
        # no text keys: the self control alone
        nk = ops.attention_controlled(qkv, None, None, H, AC.Rows(case, 1, 1, DEV), pag_rows=1)
        qs = torch.cat([sl(qkv, [2, 3])[..., :2 * C], sl(qkv, [4, 5])[..., 2 * C:]], dim=-1)
        assert torch.equal(nk[4:6], ops.attention(qs, None, None, H)) and torch.equal(nk[6:], sl(qkv, [6])[..., 2 * C:])
        with pytest.raises(_lib.MdmHipError, match="perturbed rows"):
            ops.attention_controlled(qkv, kvc, mask, H, AC.Rows(case, 1, 1, DEV), pag_rows=2)
        with pytest.raises(_lib.MdmHipError, match="source rows"):
            ops.attention_controlled(qkv, kvc, mask, H, AC.Rows(dict(case, src=[2, 4]), 1, 1, DEV), pag_rows=1)
    leaf = qkv.clone().requires_grad_(True)
    with torch.enable_grad(), pytest.raises(_lib.MdmHipError, match="inference only"):
        ops.attention_controlled(leaf, kvc, mask, H, AC.Rows(case, 1, 1, DEV), pag_rows=1)


# ---- the models against the oracle with controlled layers ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward(name, mode, gates):
    """batch 4 (AC.model_inputs); ``gates``: None = no control, else (g_c, g_s) on every layer"""
    import contextlib

    from mdm_hip import attn_control as A, ops

    model = TP._gpu_model(name)
    inp = AC.model_inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    ctl = AC.model_control()
    on = contextlib.nullcontext()
    if gates is not None:
        h = ctl.rows_for(device=DEV, cached=False)
        h.set_gates(*gates)
        on = A.applied(model, h, ctl)
    with torch.no_grad(), auto, ops.fp32_split(mode == "split"), on:
        outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    return [o.float().cpu() for o in PC.as_list(outs)]


@pytest.mark.parametrize("gates", GATES, ids=str)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mini_unet", "mini_unet_masked", "mini_nested"])
def test_models_match_the_controlled_oracle(name, mode, gates):
    """fp32 / split: rel-L2 1e-4, the mini-model gate.  bf16: the edited rows' error is at most 2x the error of the same rows
    in a forward without control (the margin of test_regions_gpu.py and test_pag_gpu.py).  And the control reaches the
    kernels: with a gate on, rows 2-3 move by more than 10 x 1e-4 from the forward without control; the sources do not move
    by a bit"""
    outs, plain = _forward(name, mode, gates), _forward(name, mode, None)
    ref, ref_plain = AC.oracle_outputs(name, gates), AC.oracle_outputs(name, None)
    for i, (o, p, r, rp) in enumerate(zip(outs, plain, ref, ref_plain)):
        e_src, e_edit, e_plain = O.rel_l2(o[:2], r[:2]), O.rel_l2(o[2:], r[2:]), O.rel_l2(p[2:], rp[2:])
        moved = O.rel_l2(o[2:], p[2:])
        print("%s %s gates %s out %d: sources %.3e, edited rows %.3e, the same rows without control %.3e (ratio %.2f); the "
              "control moves them by %.3e" % (name, mode, gates, i, e_src, e_edit, e_plain, e_edit / max(e_plain, 1e-30), moved))
        assert torch.equal(o[:2], p[:2])
        if mode == "bf16":
            assert e_edit <= 2 * e_plain
        else:
            assert e_src < 1e-4 and e_edit < 1e-4
        if any(gates):
            assert moved > 10 * 1e-4


def test_graphed_denoiser_runs_eagerly_under_applied():
    from mdm_hip import attn_control as A
    from mdm_hip.graph import GraphedDenoiser

    model = TP._gpu_model("mini_unet")
    gd = GraphedDenoiser(model)
    inp = AC.model_inputs("mini_unet")
    args = (inp["x"].to(DEV), inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV))
    ctl = AC.model_control()
    with torch.no_grad():
        plain = gd(*args)
        assert torch.equal(plain, model(*args)) and len(gd._graphs) == 1
        with A.applied(model, ctl.rows_for(device=DEV), ctl):
            out = gd(*args)
            assert torch.equal(out, model(*args))
        assert len(gd._graphs) == 1 and not torch.equal(out[2:], plain[2:]) and torch.equal(out[:2], plain[:2])
        assert torch.equal(gd(*args), plain) and len(gd._graphs) == 1
        with A.applied(model, ctl.rows_for(device=DEV), ctl), pytest.raises(ValueError, match="mixed-resolution"):
            model(*(a[:3] for a in args), {})


# ---- the samplers ----------------------------------------------------------------------------------------------------------
W, SCALE = TP.W, TP.SCALE


def _fresh(name, w=W):
    from mdm_hip.graph import GraphedSampler

    s = TP._setup(name, w)
    s.gs = GraphedSampler(s.pipe, seed=TP.RNG_SEED)
    return s


def _control(shift=1, **kw):
    """two images: row 1 an edit of row 0.  4 steps start from t = 801, 601, 400, 200 of 1000: with these intervals the cross
    gate is on in the first three and the self gate in the first two"""
    import mdm_hip

    S = 8
    m = torch.zeros(S, S)
    for j in range(S):
        m[(j + shift) % S, j] = 1.0
    keep, scale = torch.zeros(S), torch.ones(S)
    keep[6:], scale[2] = 1.0, 1.5
    kw.setdefault("cross_interval", (0.3, 1.0))
    kw.setdefault("self_interval", (0.6, 1.0))
    return mdm_hip.AttnControl(S, [0, 0], mapper={1: m}, keep={1: keep}, scale={1: scale}, **kw)


@pytest.mark.parametrize("name,kw", [
    ("mini_unet", dict(ddim_eta=0)),
    ("mini_nested", dict(solver="dpmpp_2m")),
    ("mini_unet", dict(ddim_eta=0, pag_scale=SCALE, maps=True)),    # CFG + PAG + attn_maps
], ids=["unet-ddim0", "nested-dpmpp_2m", "unet-cfg-pag-maps"])
def test_graphed_sampler_equals_eager_sampler(name, kw):
    """bit for bit; a second call, with other mapper values and other intervals, replays the one cached graph; the control
    moves the edited image and leaves the source alone"""
    import mdm_hip

    s = _fresh(name)
    kw = dict(kw)
    with_maps = kw.pop("maps", False)
    controls = (_control(), _control(shift=3, cross_interval=(0.0, 0.7), self_interval=(0.3, 0.9)))
    for rep, (seed, ctl) in enumerate(zip((41, 42), controls)):
        xs = s.start(seed)
        recs = [mdm_hip.AttnMaps(8, 2) for _ in range(2)] if with_maps else [None, None]
        more = lambda r: dict(kw, attn_maps=r) if with_maps else kw
        want, out = s.eager(xs, control=ctl, **more(recs[0])), s.graphed(xs, control=ctl, **more(recs[1]))
        print("%s %s call %d: rel-L2 %.2e, max-abs %.2e" % (name, sorted(kw), rep, O.rel_l2(out, want), float((out - want).abs().max())))
        assert torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
        if with_maps:
            assert recs[0].counts() == recs[1].counts()
            for key, m in recs[0].maps().items():
                assert torch.equal(recs[1].maps()[key], m), key
    free = s.eager(xs, **kw)
    print("the control moves the edited image by %.2e" % maxerr(out[1:], free[1:]))
    assert maxerr(out[1:], free[1:]) > 1e-3
    if not with_maps:   # (under PAG the source's perturbed rows are untouched too, but its guided image is another test's)
        assert torch.equal(out[:1], free[:1])


def test_step_noise_replay_of_an_inverted_image_with_its_edit():
    """ancestral DDPM under ``step_noise``: the noise maps of ONE inverted image, rows repeated with ``Inverted.repeat``, the
    second row under another prompt and the control -- eager equals graphed bit for bit, and the source row is the replay
    without control"""
    s = _fresh("mini_unet")
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(5)
    img = (torch.randn(1, 3, s.side, s.side, generator=g) * 0.5).clamp(-1, 1).to(DEV)
    one = [0, 2]   # [uncond | cond] of the first image
    sched = dict(num_inference_steps=4, resample_steps=True)
    with torch.no_grad():
        inv = s.pipe.invert(img, s.cond[one], s.mask[one], dev, method="ddpm", guidance_scale=W, seed=4, **sched)
        both = inv.repeat(2)
        assert both.x_t.shape[0] == 2 and torch.equal(both.x_t[0], both.x_t[1])
        ctl = _control()
        want = s.pipe.sample_from(both, s.sample, dev, guidance_scale=W, control=ctl)
        out = s.pipe.sample_from(both, s.sample, dev, graphed=s.gs, guidance_scale=W, control=ctl)
        free = s.pipe.sample_from(both, s.sample, dev, guidance_scale=W)
    assert torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
    assert torch.equal(out[:1], free[:1]) and maxerr(out[1:], free[1:]) > 1e-3


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_control_none_and_a_control_without_edits_change_no_bit(name):
    import mdm_hip

    s = _fresh(name)
    xs = s.start(43)
    idle = mdm_hip.AttnControl(8, [0, 1])
    for run in (s.eager, s.graphed):
        plain = run(xs, ddim_eta=0)
        assert torch.equal(run(xs, ddim_eta=0, control=None), plain), run.__name__
        assert torch.equal(run(xs, ddim_eta=0, control=idle), plain), run.__name__
    assert len(s.gs._graphs) == 1   # neither adds a graph
    s.graphed(xs, ddim_eta=0, control=_control())
    s.graphed(xs, ddim_eta=0, control=_control(self_max_queries=63))   # a static part of the control: another graph
    assert len(s.gs._graphs) == 3
    with pytest.raises(ValueError, match="tokens"):
        s.graphed(xs, ddim_eta=0, control=mdm_hip.AttnControl(9, [0, 0]))
    with pytest.raises(ValueError, match="rows"):
        s.graphed(xs, ddim_eta=0, control=mdm_hip.AttnControl(8, [0, 0, 0]))
