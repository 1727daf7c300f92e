"""CPU: attention-map guidance -- the differentiable torch restatement of the maps against the fp64 definition and its
autograd gradient (tests/map_guide_cases.py), ``GradRows``, the closed forms of ``AttendExcite``, the checks of ``MapGuide``
and every refusal, the samplers on a stub denoiser with a differentiable map term, and the declaration of the entry."""
import os
import re

import pytest
import torch

import attn_map_cases as AC
import map_guide_cases as MC
import pag_cases as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, D = 2, 5, 8


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,L,S_", [(32, 1, 16, 1), (32, 3, 80, 5), (64, 3, 80, 130), (128, 1, 16, 77)], ids=lambda v: str(v))
def test_cross_probs_and_its_gradient_match_fp64(d, H, L, S_):
    """fp32 torch ops against fp64: values and d sum(dacc * M) / dq within 2e-5 of the reference's max-abs (the fp32 gate of
    the kernels); zero pad columns; nothing flows to k, v or the rows outside the range"""
    from mdm_hip import attn_maps as A

    C = H * d
    qkv, kvc = PG.attn_inputs(L, S_, H, d)
    for mask in (PG.masks(S_), None):
        leaf = qkv.clone().requires_grad_(True)
        p = A.cross_probs(leaf, kvc, mask, H)
        ld = (S_ + 3) // 4 * 4
        assert tuple(p.shape) == (3, L, ld) and p.dtype == torch.float32 and not p[..., S_:].any()
        ref, live = AC.probs_ref(qkv[..., :C].transpose(1, 2), kvc[..., :C].transpose(1, 2), H, mask, None)
        assert float((p.detach()[..., :S_].double() - ref).abs().max() / ref.abs().max()) < 2e-5
        acc = A.cross_maps(qkv, kvc, mask, H, torch.zeros(3, L, ld))
        assert torch.allclose(p.detach(), acc, atol=1e-7)
        dacc = MC.kernel_dacc(L, S_, mask)
        g, = torch.autograd.grad((p * torch.nan_to_num(dacc, nan=0.0)).sum(), leaf)
        want = MC.dq_ref(qkv, kvc, mask, H, dacc)
        err = float((g[..., :C].double() - want).abs().max() / want.abs().max().clamp_min(1e-20))
        assert err < 2e-5, (mask is not None, err)
        assert not g[..., C:].any() and (mask is None or not g[2].any())   # k, v columns; the fully masked row
    leaf = qkv.clone().requires_grad_(True)
    part = A.cross_probs(leaf, kvc, PG.masks(S_), H, row0=1, rows=2)
    assert torch.equal(part, A.cross_probs(qkv[1:3], kvc[1:3], PG.masks(S_)[1:3], H))
    g, = torch.autograd.grad(part.sum() + (part ** 2).sum(), leaf)
    assert not g[0].any()


def test_grad_rows_keeps_the_maps_on_the_tape():
    import mdm_hip
    from mdm_hip import attn_maps as A

    assert "GradRows" in A.__all__ and "cross_probs" in A.__all__
    with pytest.raises(ValueError, match="GradRows"):
        A.GradRows(0, 0, 2, 2)
    with pytest.raises(ValueError, match="GradRows"):
        A.GradRows(5, 1, 2, 2)
    g = torch.Generator().manual_seed(3)
    kvc = torch.randn(4, 5, 128, generator=g)
    mask = torch.ones(4, 5)
    mask[3, 3:] = 0
    h = A.GradRows(5, 2, 2, 4)
    qs = {(4, 4): [torch.randn(4, 16, 192, generator=g).requires_grad_(True) for _ in range(3)],
          (2, 2): [torch.randn(4, 4, 192, generator=g).requires_grad_(True)]}
    for (hh, ww), lst in qs.items():
        for qkv in lst:
            h.record(qkv, kvc.clone().requires_grad_(True), mask, 2, None, 4, hh, ww)   # the text keys are constants
    assert h.counts() == {(4, 4): 3, (2, 2): 1} and h.ld == 8
    maps = h.maps()
    assert {k: tuple(v.shape) for k, v in maps.items()} == {(4, 4): (2, 5, 4, 4), (2, 2): (2, 5, 2, 2)}
    for (hh, ww), v in maps.items():
        assert v.requires_grad and torch.allclose(v.sum(dim=1), torch.ones(2, hh, ww), atol=1e-5)
        want = sum(AC.cross_maps_ref(q.detach(), kvc, mask, None, 2, torch.zeros(4, hh * ww, 8)) for q in qs[(hh, ww)]) / len(qs[(hh, ww)])
        assert torch.allclose(v.detach().double(), want[2:, :, :5].transpose(1, 2).reshape(2, 5, hh, ww), atol=1e-6)
    grads = torch.autograd.grad(maps[(4, 4)][:, 1].sum(), qs[(4, 4)] + qs[(2, 2)], allow_unused=True)
    assert all(g_ is not None and g_[2:].any() and not g_[:2].any() for g_ in grads[:3]) and grads[3] is None
    # the handle's checks: a bias, another batch, another token count
    with pytest.raises(NotImplementedError, match="bias"):
        h.record(qs[(2, 2)][0], kvc, mask, 2, torch.zeros(4, 4, 8), 4, 2, 2)
    with pytest.raises(ValueError, match="mixed-resolution nested batches are not supported"):
        h.record(qs[(2, 2)][0][:2], kvc[:2], mask[:2], 2, None, 2, 2, 2)
    with pytest.raises(ValueError, match="tokens"):
        h.record(qs[(2, 2)][0], kvc[:, :4], mask[:, :4], 2, None, 4, 2, 2)
    # it plugs into the existing switch
    stub = MC.MapStub()
    with A.applied(stub, h, "mid"):
        assert stub.mid_blocks[0].attn[0]._attn_rec is h
    assert stub.mid_blocks[0].attn[0]._attn_rec is None
    assert mdm_hip.MapGuide is mdm_hip.samplers.MapGuide and {"MapGuide", "AttendExcite"} <= set(mdm_hip.__all__)


# ---- AttendExcite ----------------------------------------------------------------------------------------------------------
def test_attend_excite_closed_forms():
    from mdm_hip import AttendExcite

    S_, h, w = 6, 4, 4
    # a one-hot map (token s owns pixel s) without smoothing: every token peaks at 1 -> loss 0
    M = torch.zeros(2, S_, h, w)
    for s in range(S_):
        M[:, s, s // w, s % w] = 1
    assert torch.equal(AttendExcite([1, 3], smooth=False)({(h, w): M}), torch.zeros(2))
    # a uniform map: every peak is 1 / S, smoothed or not (the Gaussian is normalised, reflect padding keeps constants)
    U = torch.full((2, S_, h, w), 1.0 / S_)
    for smooth in (False, True):
        assert torch.allclose(AttendExcite([0, 2], smooth=smooth)({(h, w): U}), torch.full((2,), 1 - 1.0 / S_), atol=1e-6)
    # excluded tokens renormalise: 6 uniform tokens, 2 excluded -> 1 / 4
    assert torch.allclose(AttendExcite([1, 2], smooth=False, exclude=(0, 5))({(h, w): U}), torch.full((2,), 0.75), atol=1e-6)
    # the Gaussian of sigma 0.5: a single 1 at an interior pixel peaks at its centre weight
    k = AttendExcite.kernel(torch.float32, "cpu")
    g = torch.exp(torch.tensor(-1.0 / (2 * 0.25)))
    assert torch.allclose(k.sum(), torch.tensor(1.0)) and torch.allclose(k[1, 1], 1 / (1 + 2 * g) ** 2, atol=1e-6)
    P = torch.zeros(1, 2, h, w)
    P[0, 0, 1, 2] = 1
    assert torch.allclose(AttendExcite([0])({(h, w): P}), 1 - k[1, 1].reshape(1), atol=1e-6)
    # the gradient is non-zero only for the worst token (of each image: one list per image)
    R = (torch.rand(2, S_, h, w, generator=torch.Generator().manual_seed(1)) * 0.5).requires_grad_(True)
    ae = AttendExcite([[1, 3], [0, 4]], smooth=False)
    loss = ae({(h, w): R})
    peaks = R.detach().amax(dim=(2, 3))
    worst = [min(r, key=lambda s: float(peaks[b, s])) for b, r in enumerate([[1, 3], [0, 4]])]
    assert torch.allclose(loss, torch.stack([1 - peaks[b, s] for b, s in enumerate(worst)]))
    dR, = torch.autograd.grad(loss.sum(), R)
    for b in range(2):
        hit = {s for s in range(S_) if dR[b, s].any()}
        assert hit == {worst[b]} and int((dR[b, worst[b]] != 0).sum()) == 1 and float(dR[b, worst[b]].sum()) == -1.0
    # resolution: None takes the single one, several need a choice
    two = {(h, w): U, (2, 2): U[..., :2, :2]}
    with pytest.raises(ValueError, match="resolution"):
        AttendExcite([0])(two)
    assert AttendExcite([0], resolution=(2, 2))(two).shape == (2,)
    with pytest.raises(ValueError, match="no maps of resolution"):
        AttendExcite([0], resolution=(8, 8))(two)
    for bad in (dict(tokens=[]), dict(tokens=[-1]), dict(tokens=[[0], []]), dict(tokens=[1.5]), dict(tokens=[1], exclude=(1,))):
        with pytest.raises(ValueError, match="AttendExcite"):
            AttendExcite(**bad)
    with pytest.raises(ValueError, match="token 9"):
        AttendExcite([9])({(h, w): U})
    with pytest.raises(ValueError, match="token lists for 3 images"):
        AttendExcite([[0], [1], [2]])({(h, w): U})


# ---- checks and refusals -----------------------------------------------------------------------------------------------------
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
    mask[:, 0] = 1   # every row has a live key
    x = [torch.randn(B, 3, 8, 8, generator=g) for _ in range(2)] if nested else torch.randn(B, 3, 8, 8, generator=g)
    return x, lm, mask, {}


def test_map_guide_argument_checks():
    from mdm_hip import AttendExcite, MapGuide

    fn = AttendExcite([1, 2])
    mg = MapGuide(fn, 2.0)
    assert (mg.layers, mg.interval, mg.iterations) == ("all", (0.5, 1.0), 1)
    assert [mg.on(t, 1000) for t in (1000, 751, 500, 499, 0)] == [True, True, True, False, False]
    assert MapGuide(fn, 1.0, interval=None).on(3, 1000)
    assert mg.scale_at(700, 1000) == 2.0 and MapGuide(fn, lambda t, T: 3.0 * t / T).scale_at(500, 1000) == 1.5
    for bad, exc in ((dict(fn=3, scale=1.0), TypeError), (dict(fn=fn, scale="big"), TypeError), (dict(fn=fn, scale=float("nan")), ValueError),
                     (dict(fn=fn, scale=1.0, interval=(0.5,)), ValueError), (dict(fn=fn, scale=1.0, interval=(0.6, 0.4)), ValueError),
                     (dict(fn=fn, scale=1.0, layers=3), ValueError), (dict(fn=fn, scale=1.0, iterations=0), ValueError),
                     (dict(fn=fn, scale=1.0, iterations=1.5), ValueError), (dict(fn=fn, scale=1.0, iterations=True), ValueError)):
        with pytest.raises(exc, match="MapGuide"):
            MapGuide(**bad)
    # what fn returns is checked where it is called
    smp, stub = _sampler(), MC.MapStub()
    x, lm, mask, micros = _inputs(2.0)
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    with pytest.raises(ValueError, match="one loss per image"):
        smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(lambda m: next(iter(m.values())).sum(), 1.0), **kw)
    with pytest.raises(ValueError, match="does not depend on the maps"):
        smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(lambda m: torch.zeros(B), 1.0), **kw)
    with pytest.raises(ValueError, match="selects no attention layer"):
        smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(fn, 1.0, layers=lambda n: False), **kw)
    assert all(m._attn_rec is None for m in stub.attention().values())
    assert all(p.requires_grad for p in stub.parameters())   # the freeze is undone, also by an exception


def test_refusals():
    import mdm_hip
    from mdm_hip import AttendExcite, LossGuide, MapGuide, SASolver, Tiles
    from mdm_hip.samplers import SampleOptions, _checked_rule

    mg = MapGuide(AttendExcite([1, 2]), 1.0)
    assert [f for f in SampleOptions.__dataclass_fields__][9] == "map_guide" and SampleOptions().map_guide is None
    assert {("map_guide", "guide"), ("map_guide", "tiles")} <= set(SampleOptions.REFUSED)
    with pytest.raises(NotImplementedError, match="two corrections of one step"):
        SampleOptions(map_guide=mg, guide=LossGuide(lambda x0: x0.pow(2).sum(dim=(1, 2, 3)))).check()
    with pytest.raises(NotImplementedError, match="window's queries"):
        SampleOptions(map_guide=mg, tiles=Tiles(8)).check()
    with pytest.raises(TypeError, match="MapGuide"):
        SampleOptions(map_guide="yes").check()
    with pytest.raises(NotImplementedError, match="SA solver"):
        _checked_rule(SASolver(), None, SampleOptions(map_guide=mg).check())
    # everything else composes
    SampleOptions(map_guide=mg, pag_scale=1.5, regions=mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B),
                  freeu=mdm_hip.FreeU(b=(1.1, 1.2), s=(0.9, 0.8)), attn_maps=mdm_hip.AttnMaps(S, B)).check()
    SampleOptions(map_guide=mg, cfg=mdm_hip.CFG(rescale=0.5)).check()
    smp, stub = _sampler(), MC.MapStub()
    x, lm, mask, micros = _inputs(2.0)
    kw = dict(resample_steps=True, num_inference_steps=2, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="SA solver"):
        smp.sample(stub, x, lm, mask, micros, map_guide=mg, solver="sa", **kw)
    with pytest.raises(NotImplementedError, match="two corrections"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, map_guide=mg, guide=LossGuide(lambda x0: x0.pow(2).sum(dim=(1, 2, 3))))
    assert not stub.calls


def test_graphed_sampler_refuses_map_guide():
    """before anything is built or captured: no GPU needed"""
    from mdm_hip import AttendExcite, MapGuide
    from mdm_hip.graph import GraphedSampler

    gs = GraphedSampler.__new__(GraphedSampler)
    with pytest.raises(NotImplementedError, match="GraphedSampler does not take map_guide="):
        gs.sample(B, {}, 8, torch.device("cpu"), map_guide=MapGuide(AttendExcite([1]), 1.0))


# ---- the samplers on the stub --------------------------------------------------------------------------------------------------
def _expected_move(stub, x, lm_c, mask_c, fn, scale, names, iterations=1):
    """the guidance pass by hand: the stub's map term through ``attn_maps.cross_probs`` on leaf x (top scale)"""
    from mdm_hip import attn_maps as A

    order = sorted(stub.attention())
    for _ in range(iterations):
        leaf = x.detach().clone().requires_grad_(True)
        ps = [A.cross_probs(stub.qkv_of(leaf, order.index(n)), stub.kvc_of(lm_c), mask_c, stub.HEADS) for n in names]
        M = (sum(ps) / len(ps))[..., :S].transpose(1, 2).reshape(B, S, 8, 8)
        loss = fn({(8, 8): M})
        g, = torch.autograd.grad(loss.sum(), leaf)
        x = torch.where((loss > 0).reshape(-1, 1, 1, 1), leaf.detach() - scale * g, leaf.detach())
    return x


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("w,pag_scale", [(2.0, 0.0), (1, 0.0), (2.0, 1.5)])
def test_stub_sees_the_guidance_pass(w, pag_scale, nested):
    """steps start from 751, 500, 250 of 1000; interval (0.4, 0.8) guides the first two, twice each: a guidance call sees B
    rows, the conditional text, grad mode with leaf x, frozen parameters and the recorder only; the step's own call
    follows on the moved x with the step's switches and no recorder of the guide"""
    import mdm_hip
    from mdm_hip import AttendExcite, MapGuide

    smp, stub = _sampler(nested), MC.MapStub(nested)
    x, lm, mask, micros = _inputs(w, nested)
    fn = AttendExcite([1, 2], exclude=(0,))
    names = ["down_blocks.0.attn.0", "mid_blocks.0.attn.0"]
    mg = MapGuide(fn, 0.8, interval=(0.4, 0.8), iterations=2)
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    maps = mdm_hip.AttnMaps(S, B)
    kw = dict(resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=w, pag_scale=pag_scale, regions=rp,
              attn_maps=maps)
    frozen = []
    orig = stub.forward
    stub.forward = lambda *a, **k: (frozen.append(all(not p.requires_grad for p in stub.parameters())), orig(*a, **k))[1]
    out = smp.sample(stub, x, lm, mask, micros, map_guide=mg, **kw)
    blocks = 1 + (w != 1) + bool(pag_scale)
    kinds = [c["x"][0].shape[0] if nested else c["x"].shape[0] for c in stub.calls]
    assert kinds == [B, B, blocks * B, B, B, blocks * B, blocks * B]                     # 2 + 1, 2 + 1, 1
    guide_calls = [0, 1, 3, 4]
    for i, (c, s) in enumerate(zip(stub.calls, stub.grad_seen)):
        if i in guide_calls:
            assert s["grad"] and s["leaf"] and frozen[i] and c["pag_rows"] == 0
            assert s["handles"] == {n: "GradRows" for n in names} and not any(b for _, b in s["switches"].values())
            assert torch.equal(c["lm"], lm[-B:]) and torch.equal(c["mask"], mask[-B:])
        else:
            assert not s["leaf"] and s["handles"] == {n: "BatchRows" for n in names} and c["pag_rows"] == (B if pag_scale else 0)
            assert any(b for _, b in s["switches"].values()) and torch.equal(c["lm"][: lm.shape[0]], lm)
        assert int(c["t"][0]) == [750, 750, 750, 499, 499, 499, 249][i]
    assert all(p.requires_grad for p in stub.parameters()) and all(m._attn_rec is None for m in stub.attention().values())
    assert sum(maps.counts().values()) == 3 * len(names)   # the guidance passes do not record into attn_maps
    # the step that follows sees the moved x_t (top scale; the stub's map term reads the top scale only)
    top = lambda c: c["x"][0] if nested else c["x"]
    for first, step in ((0, 2), (3, 5)):
        want = _expected_move(stub, top(stub.calls[first]), lm[-B:], mask[-B:], fn, 0.8, names, 2)
        got = top(stub.calls[step])[-B:]
        assert torch.allclose(got, want, atol=1e-6) and not torch.allclose(got, top(stub.calls[first]), atol=1e-4)
        assert torch.equal(top(stub.calls[step])[:B], got)   # every block of the batch repeats the moved x_t
        if nested:
            assert torch.equal(stub.calls[step]["x"][1][:B], stub.calls[first]["x"][1])   # no gradient: untouched
    # map_guide=None, scale = 0 and an interval without steps return the bits of the plain call
    stub.calls.clear()
    plain = smp.sample(stub, x, lm, mask, micros, **kw)
    n_plain = len(stub.calls)
    same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a if nested else [a], b if nested else [b]))
    assert n_plain == 3 and not same(out, plain)
    assert same(smp.sample(stub, x, lm, mask, micros, map_guide=None, **kw), plain) and len(stub.calls) == 2 * n_plain
    assert same(smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(fn, 1.0, interval=(0.0, 0.1)), **kw), plain)
    assert len(stub.calls) == 3 * n_plain   # no step in the interval: no call added
    assert same(smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(fn, 0.0, interval=None), **kw), plain)
    assert same(smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(fn, lambda t, T: 0.0), **kw), plain)


def test_a_sample_with_zero_loss_keeps_its_bits_and_diffusion_takes_the_keyword():
    from mdm_hip import MapGuide

    smp, stub = _sampler(), MC.MapStub()
    x, lm, mask, micros = _inputs(1)
    # loss 0 for image 0 (times a map term, so that it stays on the tape), positive for image 1
    fn = lambda m: next(iter(m.values())).amax(dim=(1, 2, 3)) * torch.tensor([0.0, 1.0])
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0)
    smp.sample(stub, x, lm, mask, micros, map_guide=MapGuide(fn, 5.0, interval=None), **kw)
    first, step = stub.calls[0]["x"], stub.calls[1]["x"]
    assert torch.equal(step[0], first[0]) and not torch.equal(step[1], first[1])
    # get_xt_minus_1 takes it too
    stub.calls.clear()
    smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, ddim_eta=0, map_guide=MapGuide(fn, 5.0))
    assert len(stub.calls) == 2 and stub.grad_seen[-2]["leaf"] and not stub.grad_seen[-1]["leaf"]


def test_the_entry_is_declared_in_the_extension_header_only():
    from mdm_hip import _lib, ops

    with pytest.raises(_lib.MdmHipError, match="MI355X"):
        ops.attn_cross_probs(torch.randn(1, 16, 96), torch.randn(1, 3, 64), None, 1)
    ext = open(os.path.join(ROOT, "include", "mdm_hip_ext.h")).read()
    main = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    assert re.search(r"\bint\s+mdm_attn_cross_maps_bwd\s*\(", ext) and "mdm_attn_cross_maps_bwd" not in main
    assert len(_lib.header_prototypes()) == 85 and _lib.ABI_VERSION == 6
    proto = {p[0]: p for p in _lib.header_prototypes(_lib.EXT_HEADER)}["mdm_attn_cross_maps_bwd"]
    assert proto[3] == ["qkv", "kvc", "mask", "dacc", "dacc_ld", "w", "dq", "dq_bs", "dq_rs", "B", "L", "S", "H", "d", "dtype", "stream"]
    src = open(os.path.join(ROOT, "ml-mdm_amd", "csrc", "attention.hip")).read()
    assert 'extern "C" int mdm_attn_cross_maps_bwd' in src
    body = src[src.index("void attn_cross_maps_bwd_kernel"):]
    assert "atomic" not in body.lower() and "MDM_NOTE_ATTN(" not in body
