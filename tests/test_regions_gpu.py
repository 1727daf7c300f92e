"""GPU: regional prompts and token weights on the HIP path -- mdm_attn_cross_bias against the fp64 restatement of
tests/region_cases.py (per-kernel gates of DESIGN section 3), its exact identities, the row-split op, the mini models
against the oracle with the same layers biased, and the samplers: regions=None changes no bit, eager equals graphed bit for
bit, other masks replay the same graph."""
import functools

import pytest
import torch

import pag_cases as PG
import parity_cases as PC
import region_cases as RC
import test_pag_gpu as TP
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = {"fp32": 2e-5, "split": 2e-5, "bf16": 3e-2}   # max-abs over max-abs
MODES = list(GATE)
# (d, H, L, S): every head dimension, a ragged query tile (L = 80), S past two key tiles (130), ld > S everywhere
KERNEL_CASES = [(32, 1, 16, 1), (32, 3, 80, 5), (64, 3, 64, 32), (64, 1, 256, 77), (64, 3, 80, 130), (96, 3, 80, 130),
                (96, 1, 64, 5), (128, 1, 16, 130), (128, 3, 256, 32), (128, 3, 80, 77)]
INF = float("inf")

_dtype, maxerr = TP._dtype, TP.maxerr


def _run(qkv, kvc, mask, bias, H, mode, base=None):
    """``base``: None = v, else a CPU tensor that is copied to the device and added onto in place"""
    from mdm_hip import ops

    dt = _dtype(mode)
    with torch.no_grad(), ops.fp32_split(mode == "split"):   # (constructing the switch sets it: only ever inside a with)
        b = None if base is None else base.to(DEV, dt).clone()
        out = ops.attn_cross_bias(qkv.to(DEV, dt), kvc.to(DEV, dt), None if mask is None else mask.to(DEV), bias.to(DEV), H,
                                  base=b)
        assert base is None or out.data_ptr() == b.data_ptr()
        return out


@functools.lru_cache(maxsize=None)
def _base(L, C, seed=0):
    return torch.randn(3, L, C, generator=torch.Generator().manual_seed(5 * L + C + seed))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,H,L,S", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_matches_the_fp64_restatement(d, H, L, S, mode):
    """B = 3: N(0, 2) bias with a quarter of the entries -inf, an all-zero row, a band of queries with every key excluded,
    NaN in the pad columns; with the mask of pag_cases (one full, one holed + tail-masked, one fully masked row) and
    without; onto v and in place onto another base"""
    dt = _dtype(mode)
    qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))   # the values the kernel sees
    bias = RC.kernel_bias(L, S)
    assert bias.shape[-1] > S and bias.shape[-1] % 4 == 0 and torch.isnan(bias[..., S:]).all()
    other = _base(L, H * d).to(dt).float()
    for mask in (PG.masks(S), None):
        for base in (None, other):
            out = _run(qkv, kvc, mask, bias, H, mode, base)
            want = RC.cross_bias_ref(qkv, kvc, mask, bias, H, base)
            err = maxerr(out, want)
            print("d=%d H=%d L=%d S=%d %s mask=%s base=%s: %.2e" % (d, H, L, S, mode, mask is not None,
                                                                    "v" if base is None else "out", err))
            assert torch.isfinite(out).all() and err < GATE[mode]


@pytest.mark.parametrize("mode", MODES)
def test_exact_identities(mode):
    """bit for bit: zero bias on v = attn_cross_addv; -inf bias on the keys a mask zeroes = that mask with zero bias;
    queries with every key excluded hold base while their neighbours do not; one live key and small-integer base and v_c
    give base + v_c"""
    from mdm_hip import ops

    dt = _dtype(mode)
    for d, H, L, S in ((32, 3, 80, 5), (96, 1, 64, 77), (128, 3, 16, 130), (64, 3, 256, 32)):
        C = H * d
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d, seed=7))
        ld = RC.kernel_bias(L, S).shape[-1]
        zero = torch.zeros(3, L, ld)
        zero[..., S:] = float("nan")
        mask = PG.masks(S)
        with torch.no_grad(), ops.fp32_split(mode == "split"):
            for m in (None, mask):
                addv = ops.attn_cross_addv(qkv.to(DEV, dt), kvc.to(DEV, dt), None if m is None else m.to(DEV), H)
                assert torch.equal(_run(qkv, kvc, m, zero, H, mode), addv)
        dead = zero.clone()
        dead[..., :S] = torch.where(mask == 0, -INF, 0.0)[:, None, :]
        want = _run(qkv, kvc, mask, zero, H, mode)
        assert torch.equal(_run(qkv, kvc, None, dead, H, mode), want) and torch.equal(_run(qkv, kvc, mask, dead, H, mode), want)
        assert not torch.equal(want, _run(qkv, kvc, None, zero, H, mode))
        # the dead band of batch row 2 (region_cases.kernel_bias), in place onto another base
        base = _base(L, C, seed=1).to(dt)
        out = _run(qkv, kvc, None, RC.kernel_bias(L, S), H, mode, base.float()).cpu()
        lo, hi = RC.dead_band(L)
        assert torch.equal(out[2, lo:hi], base[2, lo:hi])
        live = [i for i in (lo - 1, hi) if 0 <= i < L]
        assert live and all(not torch.equal(out[2, i], base[2, i]) for i in live)
        # one live key per query (key l mod S), small integers in base and v_c
        g = torch.Generator().manual_seed(d + L)
        ib = torch.randint(-8, 9, (3, L, C), generator=g).float()
        kv = torch.cat([kvc[..., :C], torch.randint(-8, 9, (3, S, C), generator=g).float()], dim=-1)
        one = torch.full((3, L, ld), -INF)
        key = torch.arange(L) % S
        one[:, torch.arange(L), key] = 0.7
        out = _run(qkv, kv, None, one, H, mode, ib).cpu().float()
        assert torch.equal(out, ib + kv[:, key, C:])
        if mode != "bf16":   # onto v, which holds no small integers: exact only where the sum is not rounded to bf16
            assert torch.equal(_run(qkv, kv, None, one, H, mode).cpu(), qkv[..., 2 * C:] + kv[:, key, C:])


@pytest.mark.parametrize("mode", MODES)
def test_attention_biased_splits_the_batch_by_rows(mode):
    from mdm_hip import _lib, ops

    dt = _dtype(mode)
    N, L, S, H, d = 5, 80, 77, 3, 64
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(N, L, 3 * H * d, generator=g).to(DEV, dt)
    kvc = torch.randn(N, S, 2 * H * d, generator=g).to(DEV, dt)
    mask = (torch.rand(N, S, generator=g) < 0.7).float().to(DEV)
    bias = (torch.randn(N, L, 80, generator=g) * 2).to(DEV)
    bias[:, :, S:] = float("nan")
    zero = torch.zeros_like(bias)
    with torch.no_grad(), ops.fp32_split(mode == "split"):
        for m in (mask, None):
            # zero bias: the attention of today, within the mode's gate (another order of the same sums)
            err = maxerr(ops.attention_biased(qkv, kvc, m, zero, H), ops.attention(qkv, kvc, m, H))
            print("%s mask=%s: zero bias against ops.attention %.2e" % (mode, m is not None, err))
            assert err < GATE[mode]
            out = ops.attention_biased(qkv, kvc, m, bias, H, pag_rows=2)
            sl = lambda t, a, b: None if t is None else t[a:b].contiguous()
            assert torch.equal(out[3:], ops.attn_cross_bias(sl(qkv, 3, 5), sl(kvc, 3, 5), sl(m, 3, 5), sl(bias, 3, 5), H))
            assert torch.equal(out[:3], ops.attention_biased(sl(qkv, 0, 3), sl(kvc, 0, 3), sl(m, 0, 3), sl(bias, 0, 3), H))
            want = RC.cross_bias_ref(qkv[:3].float().cpu(), kvc[:3].float().cpu(), None if m is None else m[:3].cpu(),
                                     bias[:3].cpu(), H, base=ops.attention(qkv[:3].contiguous(), None, None, H).float().cpu())
            assert maxerr(out[:3], want) < GATE[mode]
            assert torch.equal(ops.attention_biased(qkv, kvc, m, bias, H, pag_rows=N), ops.attn_cross_bias(qkv, kvc, m, bias, H))
        with pytest.raises(_lib.MdmHipError, match="pag_rows"):
            ops.attention_biased(qkv, kvc, mask, bias, H, pag_rows=6)
        with pytest.raises(_lib.MdmHipError, match="bias"):
            ops.attention_biased(qkv, kvc, mask, bias[:, :, :76].contiguous(), H)
        with pytest.raises(_lib.MdmHipError, match="bias"):
            ops.attn_cross_bias(qkv, kvc, mask, bias[:, :, :78].contiguous(), H)
        with pytest.raises(_lib.MdmHipError, match="no text keys"):
            ops.attention_biased(qkv, None, None, bias, H)
    leaf = qkv.clone().requires_grad_(True)
    for fn in (ops.attention_biased, ops.attn_cross_bias):
        with torch.enable_grad(), pytest.raises(_lib.MdmHipError, match="inference only"):
            fn(leaf, kvc, mask, bias, H)
        with torch.no_grad():   # ... and no complaint where no tape is recorded
            fn(leaf, kvc, mask, bias, H)


# ---- the models against the oracle with biased layers ------------------------------------------------------------------
def _forward(name, mode, regions=False):
    """batch 4 (RC.model_inputs); ``regions``: rows 2-3 biased on every layer with text keys"""
    import contextlib

    from mdm_hip import ops, regions as R

    model = TP._gpu_model(name)
    inp = RC.model_inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), auto, ops.fp32_split(mode == "split"):
        with (R.applied(model, RC.model_regions(name, DEV), "all") if regions else contextlib.nullcontext()):
            outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    return [o.float().cpu() for o in PC.as_list(outs)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mini_unet", "mini_unet_masked", "mini_nested"])
def test_models_match_the_oracle_with_biased_layers(name, mode):
    """fp32 / split: rel-L2 1e-4, the mini-model gate.  bf16: the biased rows' error is at most 2x the error of the same
    rows in a forward without regions (one op swapped, the margin of test_pag_gpu.py).  And the bias reaches the kernel:
    rows 2-3 move by more than 10 x 1e-4 from the forward without regions, rows 0-1 (zero bias) stay within the gate."""
    from mdm_hip import regions as R

    names = R.layer_names(TP._gpu_model(name), "all")
    outs, plain = _forward(name, mode, True), _forward(name, mode)
    ref, ref_plain = RC.oracle_outputs(name, names), RC.oracle_outputs(name, ())
    for i, (o, p, r, rp) in enumerate(zip(outs, plain, ref, ref_plain)):
        e_zero, e_bias, e_plain = O.rel_l2(o[:2], r[:2]), O.rel_l2(o[2:], r[2:]), O.rel_l2(p[2:], rp[2:])
        moved, moved_ref = O.rel_l2(o[2:], p[2:]), O.rel_l2(r[2:], rp[2:])
        print("%s %s out %d: zero-bias rows %.3e, biased rows %.3e, the same rows without regions %.3e (ratio %.2f); the bias "
              "moves the rows by %.3e (oracle: %.3e)" % (name, mode, i, e_zero, e_bias, e_plain, e_bias / max(e_plain, 1e-30),
                                                         moved, moved_ref))
        # zero bias is no bias, in the oracle: the restated layer forms the cross term in fp64, the oracle's own in fp32 --
        # two roundings of the same fp32 network, held to a tenth of the mini-model gate
        assert O.rel_l2(r[:2], rp[:2]) < 1e-5
        if mode == "bf16":
            assert e_bias <= 2 * e_plain
        else:
            assert e_zero < 1e-4 and e_bias < 1e-4
        assert moved > 10 * 1e-4


def test_graphed_denoiser_runs_eagerly_under_applied():
    """never a graph captured with a caller's bias, never one captured without it replayed"""
    from mdm_hip import regions as R
    from mdm_hip.graph import GraphedDenoiser

    model = TP._gpu_model("mini_unet")
    gd = GraphedDenoiser(model)
    inp = RC.model_inputs("mini_unet")
    args = (inp["x"].to(DEV), inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV))
    rp = RC.model_regions("mini_unet", DEV)
    with torch.no_grad():
        plain = gd(*args)
        assert torch.equal(plain, model(*args)) and len(gd._graphs) == 1
        with R.applied(model, rp):
            biased = gd(*args)
            assert torch.equal(biased, model(*args))
        assert len(gd._graphs) == 1 and not torch.equal(biased[2:], plain[2:])
        assert torch.equal(gd(*args), plain) and len(gd._graphs) == 1


def test_mixed_resolution_batch_is_refused():
    from mdm_hip import regions as R

    model = TP._gpu_model("mini_unet")
    inp = RC.model_inputs("mini_unet")
    rp = RC.model_regions("mini_unet", DEV)
    with torch.no_grad(), R.applied(model, rp), pytest.raises(ValueError, match="mixed-resolution"):
        model(inp["x"][:3].to(DEV), inp["times"][:3].to(DEV), inp["cond"][:3].to(DEV), inp["mask"][:3].to(DEV), {})


# ---- the samplers ----------------------------------------------------------------------------------------------------------
W, SCALE = TP.W, TP.SCALE


def _fresh(name, w=W):
    from mdm_hip.graph import GraphedSampler

    s = TP._setup(name, w)
    s.gs = GraphedSampler(s.pipe, seed=TP.RNG_SEED)
    return s


def _known(s, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(2, 1, s.side, s.side, device=DEV)
    m[..., : s.side // 2] = 1
    return dict(known_images=(torch.randn(2, 3, s.side, s.side, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_regions_none_is_the_call_without_the_argument(name):
    s = _fresh(name)
    xs = s.start(43)
    for run in (s.eager, s.graphed):
        for kw in (dict(ddim_eta=0), dict(solver="dpmpp_2m")):
            assert torch.equal(run(xs, regions=None, region_layers="mid", **kw), run(xs, **kw)), (run.__name__, kw)
    assert len(s.gs._graphs) == 2   # regions=None adds no graph


@pytest.mark.parametrize("name,kw", [
    ("mini_unet", dict(ddim_eta=0)),
    ("mini_nested", dict(ddim_eta=0)),
    ("mini_nested", dict(solver="dpmpp_2m")),
    ("mini_unet", dict(known=True)),                     # ancestral DDPM with a known half
    ("mini_unet", dict(ddim_eta=0, pag_scale=SCALE)),    # CFG + PAG
], ids=["unet-ddim0", "nested-ddim0", "nested-dpmpp_2m", "unet-ddpm-known", "unet-cfg-pag"])
def test_graphed_sampler_equals_eager_sampler(name, kw):
    """bit for bit, also on a second call through the cached graph; and the regions act"""
    s = _fresh(name)
    rp = RC.model_regions(name, DEV)
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed)
        more = dict(kw)
        if more.pop("known", False):
            more.update(_known(s, seed))
        want, out = s.eager(xs, regions=rp, **more), s.graphed(xs, regions=rp, **more)
        print("%s %s call %d: rel-L2 %.2e, max-abs %.2e" % (name, sorted(kw), rep, O.rel_l2(out, want), float((out - want).abs().max())))
        assert torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
    free = s.eager(xs, **more)
    print("the regions move the image by %.2e" % maxerr(out, free))
    assert maxerr(out, free) > 1e-3


def test_other_masks_replay_the_same_graph_and_another_S_adds_one():
    import mdm_hip

    s = _fresh("mini_unet")
    xs = s.start(44)
    rp = RC.model_regions("mini_unet", DEV)
    a = s.graphed(xs, ddim_eta=0, regions=rp)
    assert len(s.gs._graphs) == 1 and torch.equal(a, s.eager(xs, ddim_eta=0, regions=rp))
    # other masks and weights, through set_spans and through another handle: the same graph
    left, right = RC.seam_regions(16, feather=2)
    spans = [(0, 3, right.transpose(-1, -2).contiguous(), 0.6), (3, 8, left.transpose(-1, -2).contiguous(), torch.full((2, 5), 2.0))]
    other = mdm_hip.RegionPrompts(8, 16, spans, rows=2, device=DEV)
    b = s.graphed(xs, ddim_eta=0, regions=other)
    assert len(s.gs._graphs) == 1 and not torch.equal(a, b) and torch.equal(b, s.eager(xs, ddim_eta=0, regions=other))
    rp.set_spans(spans)
    assert torch.equal(s.graphed(xs, ddim_eta=0, regions=rp), b) and len(s.gs._graphs) == 1
    rp.set_spans(RC.model_spans("mini_unet"))
    assert torch.equal(s.graphed(xs, ddim_eta=0, regions=rp), a) and len(s.gs._graphs) == 1
    # another layer set captures anew; the same set under another spelling does not
    c = s.graphed(xs, ddim_eta=0, regions=rp, region_layers="mid")
    assert len(s.gs._graphs) == 2 and not torch.equal(a, c)
    assert torch.equal(s.graphed(xs, ddim_eta=0, regions=rp, region_layers=["mid_blocks.0.attn.0"]), c) and len(s.gs._graphs) == 2
    # another S: four more text tokens
    sample = dict(s.sample)
    try:
        g = torch.Generator().manual_seed(9)
        more = torch.randn(4, 4, s.cond.shape[-1], generator=g).to(DEV)
        more[:2] = 0
        s.cond, s.mask = torch.cat([s.cond, more], dim=1), torch.cat([s.mask, torch.ones(4, 4, device=DEV)], dim=1)
        s.sample = {"lm_outputs": s.cond, "lm_mask": s.mask}
        rp12 = mdm_hip.RegionPrompts(12, 16, RC.model_spans("mini_unet") + [(8, 12, None, 1.3)], rows=2, device=DEV)
        d = s.graphed(xs, ddim_eta=0, regions=rp12)
        assert len(s.gs._graphs) == 3 and torch.equal(d, s.eager(xs, ddim_eta=0, regions=rp12))
        with pytest.raises(ValueError, match="tokens"):
            s.graphed(xs, ddim_eta=0, regions=rp)
    finally:
        s.cond, s.mask, s.sample = sample["lm_outputs"], sample["lm_mask"], sample
