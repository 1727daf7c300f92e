"""GPU: attention-map guidance on the HIP path -- mdm_attn_cross_maps_bwd against the fp64 autograd gradient of
tests/map_guide_cases.py (the project's kernel gates), its exact identities, the differentiable op, the mini models' input
gradient of a loss on the maps against the differentiable oracle, and the samplers with ``map_guide=`` against the guided
loop restated around the oracle."""
import functools

import pytest
import torch

import attn_map_cases as AC
import map_guide_cases as MC
import pag_cases as PG
import parity_cases as PC
import region_cases as RC
import test_pag_gpu as TP
import test_regions_gpu as TR
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = TR.GATE                   # fp32 / split 2e-5, bf16 3e-2: max-abs over max-abs
MODES = TR.MODES
KERNEL_CASES = TR.KERNEL_CASES   # (d, H, L, S): every head dimension, L = 16 / 64 / 80 (ragged) / 256, S = 1 .. 130, H = 1, 3
SENTINEL = 7.25

_dtype, maxerr = TP._dtype, TP.maxerr


def _bwd(qkv, kvc, mask, dacc, H, mode, w=1.0, row0=0, rows=None):
    """the kernel on CPU operands -> the whole qkv-shaped gradient (pre-filled with SENTINEL), on the device"""
    from mdm_hip import ops

    dt = _dtype(mode)
    with torch.no_grad(), ops.fp32_split(mode == "split"):   # (constructing the switch sets it: only ever inside a with)
        dqkv = torch.full(qkv.shape, SENTINEL, device=DEV, dtype=dt)
        out = ops.attn_cross_maps_bwd(qkv.to(DEV, dt), kvc.to(DEV, dt), None if mask is None else mask.to(DEV), H, dacc.to(DEV),
                                      dqkv, weight=w, row0=row0, rows=rows)
        assert out is dqkv
        return dqkv


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16),
                       b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16))


# ---- the kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,H,L,S", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_matches_the_fp64_gradient(d, H, L, S, mode):
    """B = 3, N(0, 1) dacc with NaN in the pad columns and in the masked keys' entries; with the mask of pag_cases (one
    full, one holed + tail-masked, one fully masked row) and without; operands rounded to the mode's dtype for both sides.
    Measured on one MI355X, worst over the cases: fp32 and split 6.1e-7, bf16 6.5e-3."""
    dt = _dtype(mode)
    C = H * d
    qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))   # the values the kernel sees
    for mask in (PG.masks(S), None):
        dacc = MC.kernel_dacc(L, S, mask)
        assert dacc.shape[-1] > S and dacc.shape[-1] % 4 == 0 and torch.isnan(dacc[..., S:]).all()
        out = _bwd(qkv, kvc, mask, dacc, H, mode, w=0.75).float().cpu()
        want = MC.dq_ref(qkv, kvc, mask, H, dacc, 0.75)
        err = maxerr(out[..., :C], want)
        print("d=%d H=%d L=%d S=%d %s mask=%s: %.2e" % (d, H, L, S, mode, mask is not None, err))
        assert torch.isfinite(out).all() and err < GATE[mode]
        assert torch.equal(out[..., C:], torch.full_like(out[..., C:], SENTINEL))   # the k and v columns
        if mask is not None:
            assert torch.equal(out[2, :, :C], torch.zeros(L, C))                    # the fully masked row


@pytest.mark.parametrize("mode", MODES)
def test_exact_identities(mode):
    """bit for bit, in every mode: one live key gives 0; q = 0 with 2^k live keys and dacc constant along the keys gives 0;
    rows outside [row0, row0 + rows) keep the sentinel and rows [1, 3) are the launch on the slice; two runs are equal"""
    for d, H, L, S in AC.EXACT_CASES:
        C = H * d
        dt = _dtype(mode)
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d, seed=7))
        # a single live key, another one per batch row
        one = torch.zeros(3, S)
        one[torch.arange(3), torch.tensor([0, S // 2, S - 1])] = 1
        dacc = MC.kernel_dacc(L, S, one)
        out = _bwd(qkv, kvc, one, dacc, H, mode).float().cpu()
        assert torch.equal(out[..., :C], torch.zeros(3, L, C)), (d, H, L, S)
        # q = 0, 2^k live keys, an integer constant per query
        ld = dacc.shape[-1]
        for k in range(4):
            if 2 ** k > S:
                continue
            mk = MC.first_keys_mask(S, 2 ** k)
            const = torch.randint(-7, 8, (3, L, 1), generator=torch.Generator().manual_seed(k)).float().expand(3, L, ld).clone()
            const[..., S:] = float("nan")
            const[..., 2 ** k:S] = float("nan")
            out = _bwd(torch.zeros_like(qkv), kvc, mk, const, H, mode).float().cpu()
            assert torch.equal(out[..., :C], torch.zeros(3, L, C)), (d, H, L, S, k)
        # rows [1, 3) of the batch of 3, the launch on the slice, two runs
        mask = PG.masks(S)
        dacc = MC.kernel_dacc(L, S, mask, seed=3)
        whole = _bwd(qkv, kvc, mask, dacc, H, mode)
        part = _bwd(qkv, kvc, mask, dacc[1:3].contiguous(), H, mode, row0=1, rows=2)
        alone = _bwd(qkv[1:3], kvc[1:3], mask[1:3], dacc[1:3].contiguous(), H, mode)
        assert _same_bits(whole, _bwd(qkv, kvc, mask, dacc, H, mode))
        assert _same_bits(part[1:3], whole[1:3]) and _same_bits(alone, whole[1:3])
        assert torch.equal(part[0].float().cpu(), torch.full((L, 3 * C), SENTINEL))
        assert torch.equal(part[1:3, :, C:].float().cpu(), torch.full((2, L, 2 * C), SENTINEL))


@pytest.mark.parametrize("mode", MODES)
def test_integer_operands_round_once(mode):
    """q = 0, d = 64, H = 1, 2^k live keys, integer dacc (|v| <= 7) and integer k_c (|v| <= 4): every intermediate is exactly
    representable, so dq is the fp64 value rounded once to the output dtype"""
    dt = _dtype(mode)
    d, H = 64, 1
    for L, S in ((80, 5), (64, 32), (16, 130)):
        g = torch.Generator().manual_seed(L + S)
        kvc = torch.randint(-4, 5, (3, S, 2 * d), generator=g).float()
        qkv = torch.zeros(3, L, 3 * d)
        for k in range(4):
            if 2 ** k > S:
                continue
            mk = MC.first_keys_mask(S, 2 ** k)
            dacc = torch.randint(-7, 8, (3, L, (S + 4) // 4 * 4), generator=g).float()
            out = _bwd(qkv, kvc, mk, dacc, H, mode).cpu()
            exact = MC.dq_uniform_ref(kvc, 2 ** k, dacc, d)
            assert float((exact - MC.dq_ref(qkv, kvc, mk, H, dacc)).abs().max()) < 1e-12   # the autograd reference, to its rounding
            want = exact.to(dt)
            assert (k == 0 or want.abs().max() > 0) and torch.equal(out[..., :d], want), (L, S, k)   # (by value: a zero of either sign)


@pytest.mark.parametrize("mode", MODES)
def test_op_forward_is_the_recorders_increment_and_backward_is_the_kernel(mode):
    from mdm_hip import ops

    dt = _dtype(mode)
    for d, H, L, S in ((64, 3, 80, 32), (96, 3, 80, 130)):
        C = H * d
        qkv, kvc = (t.to(DEV, dt) for t in PG.attn_inputs(L, S, H, d))
        mask = PG.masks(S).to(DEV)
        ld = (S + 3) // 4 * 4
        with ops.fp32_split(mode == "split"):
            leaf = qkv.clone().requires_grad_(True)
            with torch.enable_grad():
                probs = ops.attn_cross_probs(leaf, kvc, mask, H, row0=1, rows=2)
            assert probs.requires_grad and tuple(probs.shape) == (2, L, ld) and probs.dtype == torch.float32
            acc = ops.attn_cross_maps(qkv, kvc, mask, H, torch.zeros(2, L, ld, device=DEV), row0=1, rows=2)
            assert _same_bits(probs.detach(), acc)
            dacc = torch.randn(2, L, ld, generator=torch.Generator().manual_seed(5)).to(DEV)
            got, = torch.autograd.grad(probs, leaf, grad_outputs=dacc)
            want = ops.attn_cross_maps_bwd(qkv, kvc, mask, H, dacc, torch.zeros_like(qkv), row0=1, rows=2)
        assert _same_bits(got, want) and not got[0].any() and not got[..., C:].any() and got[1, :, :C].any()


def test_operand_checks():
    from mdm_hip import _lib, ops

    N, L, S, H, d = 2, 16, 5, 1, 32
    qkv, kvc = torch.randn(N, L, 3 * d, device=DEV), torch.randn(N, S, 2 * d, device=DEV)
    dacc, dqkv = torch.zeros(N, L, 8, device=DEV), torch.zeros(N, L, 3 * d, device=DEV)
    for bad, match in ((dict(dacc=torch.zeros(N, L, 6, device=DEV)), "dacc"), (dict(dacc=torch.zeros(N, L, 4, device=DEV)), "dacc"),
                       (dict(dacc=dacc.double()), "dacc"), (dict(dqkv=dqkv[:, :, :d]), "dqkv"), (dict(dqkv=dqkv.bfloat16()), "dqkv"),
                       (dict(row0=1, rows=2), "rows"), (dict(kvc=None), "no text keys"), (dict(heads=5), "heads"),
                       (dict(mask=torch.ones(N, S + 1, device=DEV)), "mask")):
        kw = dict(qkv=qkv, kvc=kvc, mask=None, heads=H, dacc=dacc, dqkv=dqkv)
        kw.update(bad)
        with pytest.raises(_lib.MdmHipError, match=match):
            ops.attn_cross_maps_bwd(**kw)
    # the entry's own checks: a negative status, nothing launched
    lib = _lib.lib()
    p = lambda t: t.data_ptr()
    good = [p(qkv), p(kvc), None, p(dacc), 8, 1.0, p(dqkv), L * 3 * d, 3 * d, N, L, S, H, d, 0, None]
    assert lib.mdm_attn_cross_maps_bwd(*good) == 0
    for i, v in ((4, 6), (4, 4), (3, p(dacc) + 4), (8, d - 4), (8, 3 * d + 1), (6, p(dqkv) + 4), (13, 48), (11, 0), (14, 9), (0, None)):
        args = list(good)
        args[i] = v
        assert lib.mdm_attn_cross_maps_bwd(*args) < 0, (i, v)
    torch.cuda.synchronize()
    with pytest.raises(_lib.MdmHipError, match="kvc requires grad"):
        with torch.enable_grad():
            ops.attn_cross_probs(qkv, kvc.clone().requires_grad_(True), None, H)
    with torch.no_grad():   # no tape: nothing to refuse
        assert not ops.attn_cross_probs(qkv, kvc.clone().requires_grad_(True), None, H).requires_grad


# ---- the models: d loss / d x_t from the middle of the network -----------------------------------------------------------------
def _hip_map_grads(name, mode):
    """batch 4 (PG.model_inputs) on leaf x of every scale, every layer with text keys recording through ``GradRows``;
    loss = sum of fixed random weights x maps -> (gradients per scale, maps)"""
    from mdm_hip import attn_maps as A, ops

    model = TP._gpu_model(name)
    inp = PG.model_inputs(name)
    xs = [t.to(DEV).requires_grad_(True) for t in PC.as_list(inp["x"])]
    handle = A.GradRows(inp["cond"].shape[1], 0, 4, 4)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    params = [p.grad for p in model.parameters()]
    with torch.enable_grad(), auto, ops.fp32_split(mode == "split"), A.applied(model, handle, "all"):
        model(xs if isinstance(inp["x"], list) else xs[0], inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
        maps = handle.maps()
        loss = sum((MC.map_weights(k, m.shape).to(DEV) * m).sum() for k, m in sorted(maps.items()))
        grads = torch.autograd.grad(loss, xs, allow_unused=True)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(params, [p.grad for p in model.parameters()]))   # autograd.grad: no parameter gradient
    return grads, {k: m.detach() for k, m in maps.items()}


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, bf16=False):
    return (MC.oracle_map_grads_bf16 if bf16 else MC.oracle_map_grads)(name, MC.map_weights)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_models_input_gradient_of_a_map_loss_matches_the_oracle(name, mode):
    """The first backward of this code base that starts in the middle of the network: the outputs take no part, and the
    pass-through and tap outputs behind the last recording layer get no gradient.  fp32 / split: rel-L2 < 1e-3 per tensor
    (the project's gradient gate); bf16: at most 1.5 x the oracle's own bf16-autocast error (test_input_grad_gpu.py's rule)"""
    grads, maps = _hip_map_grads(name, mode)
    _, ref, ref_maps = _oracle_grads(name)
    assert set(maps) == set(ref_maps) and all(g is not None for g in grads) and all(g is not None for g in ref)
    errs = [O.rel_l2(g.float().cpu(), r) for g, r in zip(grads, ref)]
    if mode == "bf16":
        _, bf, _ = _oracle_grads(name, True)
        bars = [O.rel_l2(b, r) for b, r in zip(bf, ref)]
        print("[map grad bf16 %s] rel-L2 vs fp32 oracle %s; the oracle's own under bf16 autocast %s" % (
            name, ["%.3e" % e for e in errs], ["%.3e" % b for b in bars]))
        assert all(torch.isfinite(g).all() for g in grads) and all(e <= 1.5 * b for e, b in zip(errs, bars)), (errs, bars)
    else:
        print("[map grad %s %s] rel-L2 vs oracle %s" % (mode, name, ["%.3e" % e for e in errs]))
        assert max(errs) < 1e-3, errs


# ---- the samplers ---------------------------------------------------------------------------------------------------------------
TOKENS = [1, 2]
INTERVAL = (0.5, 1.0)   # the steps start from 801, 601, 400, 200 of 1000: the first two are guided
SCALES = {"mini_unet": 40.0, "mini_nested": 40.0}   # chosen so that the ORACLE loop alone moves the result by > 1e-2 (checked on the CPU)
SAMPLER_CASES = [
    ("mini_unet", dict(ddim_eta=0)),
    ("mini_nested", dict(solver="dpmpp_2m")),
    ("mini_unet", dict(ddim_eta=0, pag_scale=TP.SCALE, regions=True, attn_maps=True)),
]
SAMPLER_IDS = ["unet-ddim0-cfg", "nested-dpmpp_2m", "unet-cfg-pag-regions-attn_maps"]


@functools.lru_cache(maxsize=None)
def _resolution(name):
    """the finest attention resolution with text keys of the model: what AttendExcite reads"""
    _, _, ref_maps = _oracle_grads(name)
    return max(ref_maps)


def _guide(name, scale=None, interval=INTERVAL):
    from mdm_hip import AttendExcite, MapGuide

    return MapGuide(AttendExcite(TOKENS, resolution=_resolution(name)), SCALES[name] if scale is None else scale, interval=interval)


@functools.lru_cache(maxsize=None)
def _cpu_pipe(name):
    pipe = TP._pipeline(name, PC.build_module(name)[0])
    pipe.eval()
    return pipe


def _oracle_loop(name, kw, xs, cond, mask, w, scale=None, interval=INTERVAL):
    """``map_guide_cases.restated_guided_loop`` for a case of SAMPLER_CASES, on CPU copies of the inputs"""
    from mdm_hip import attn_maps as A

    pipe = _cpu_pipe(name)
    model, cfg, sd = PC.build_module(name)
    names = A.layer_names(model, "all")
    mg = _guide(name, scale, interval)
    pag = regions = None
    if kw.get("pag_scale"):
        from mdm_hip import pag as P
        pag = (P.layer_names(model, "mid"), kw["pag_scale"])
    if kw.get("regions"):
        regions = (names, RC.model_regions(name))
    return MC.restated_guided_loop(pipe.sampler, pipe.get_model(), sd, cfg, [x.cpu() for x in xs], cond.cpu(), mask.cpu(), 4, w,
                                   mg.fn, mg.scale, mg.interval, names, solver=kw.get("solver"), pag=pag, regions=regions)


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("name,kw", SAMPLER_CASES, ids=SAMPLER_IDS)
def test_guided_sampling_matches_the_restated_loop_around_the_oracle(name, kw):
    """4 steps, CFG w = 2, AttendExcite on two tokens in the first two steps, fp32: the final x against the guided loop
    restated around the oracle, rel-L2 < 1e-3 (the sampling gate of DESIGN section 3); the guide is no bystander -- it moves
    the result by rel-L2 > 1e-2, in the oracle loop alone too; the recorded AttnMaps are those of the steps' own calls;
    two runs are bit-identical"""
    import mdm_hip

    s = TP._setup(name)
    xs = s.start(61)
    opts = {k: v for k, v in kw.items() if k not in ("regions", "attn_maps")}
    if kw.get("regions"):
        opts["regions"] = RC.model_regions(name, DEV)
    maps = mdm_hip.AttnMaps(s.cond.shape[1], 2) if kw.get("attn_maps") else None
    if maps is not None:
        opts["attn_maps"] = maps
    out = s.eager(xs, map_guide=_guide(name), **opts)
    counts = None if maps is None else maps.counts()
    got_maps = None if maps is None else {k: v.clone() for k, v in maps.maps().items()}
    if maps is not None:
        maps.reset()
    again = s.eager(xs, map_guide=_guide(name), **opts)
    assert _same(out, again)
    if maps is not None:
        maps.reset()
    free = s.eager(xs, **opts)
    want = _oracle_loop(name, kw, xs, s.cond, s.mask, s.w)
    want_free = _oracle_loop(name, kw, xs, s.cond, s.mask, s.w, interval=(2.0, 3.0))
    err, moved, moved_ref = O.rel_l2(out.float().cpu(), want), O.rel_l2(out, free), O.rel_l2(want, want_free)
    print("[map-guided sampling %s %s] rel-L2 vs the oracle loop %.3e; the guide moved the result by %.3e (oracle loop: %.3e)"
          % (name, sorted(kw), err, moved, moved_ref))
    assert torch.isfinite(out).all() and err < 1e-3
    assert moved > 1e-2 and moved_ref > 1e-2
    if maps is not None:   # 4 steps x the layers, nothing from the guidance passes; and the maps of the steps' own calls:
        from mdm_hip import attn_maps as A
        n_layers = len(A.layer_names(s.pipe.get_model().vision_model, "all"))
        assert sum(counts.values()) == 4 * n_layers
        # ... the unguided call's steps see another x_t from the second step on, so its maps differ, while a call that is
        # guided the same way records the same bits
        assert all(torch.equal(got_maps[k], maps.maps()[k]) is False for k in got_maps)
        maps.reset()
        s.eager(xs, map_guide=_guide(name), **opts)
        assert all(torch.equal(got_maps[k], maps.maps()[k]) for k in got_maps)


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_map_guide_none_is_the_call_without_the_argument(name):
    s = TR._fresh(name)
    xs = s.start(63)
    for kw in (dict(ddim_eta=0), dict(solver="dpmpp_2m")):
        plain = s.eager(xs, **kw)
        assert _same(s.eager(xs, map_guide=None, **kw), plain)
        assert _same(s.eager(xs, map_guide=_guide(name, interval=(0.0, 0.0)), **kw), plain)   # an interval without a step
        assert _same(s.graphed(xs, map_guide=None, **kw), s.graphed(xs, **kw))
    assert len(s.gs._graphs) == 2   # map_guide=None adds no graph


def test_refused_pairs_raise():
    from mdm_hip import LossGuide, Tiles

    s = TR._fresh("mini_unet")
    xs = s.start(64)
    mg = _guide("mini_unet")
    with pytest.raises(NotImplementedError, match="two corrections of one step"):
        s.eager(xs, map_guide=mg, guide=LossGuide(lambda x0: x0.pow(2).sum(dim=(1, 2, 3))))
    with pytest.raises(NotImplementedError, match="window's queries"):
        s.eager(xs, map_guide=mg, tiles=Tiles(16))
    with pytest.raises(NotImplementedError, match="SA solver"):
        s.eager(xs, map_guide=mg, solver="sa")
    with pytest.raises(NotImplementedError, match="GraphedSampler does not take map_guide="):
        s.graphed(xs, map_guide=mg)
    assert len(s.gs._graphs) == 0
