"""GPU: cross-attention maps on the HIP path -- mdm_attn_cross_maps against the fp64 restatement of tests/attn_map_cases.py
(per-kernel gates of DESIGN section 3), its exact identities, its row sums, its agreement with the kernel it mirrors
(mdm_attn_cross_bias), the mini models under ``attn_maps.record`` against the oracle with a recording hook, and the
samplers: the images do not change by a bit, eager maps equal graphed maps bit for bit, ``attn_maps=None`` adds no graph."""
import pytest
import torch

import attn_map_cases as AC
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
KERNEL_CASES = TR.KERNEL_CASES   # (d, H, L, S): every head dimension, L = 16 / 80 (ragged), S = 1, 5, 77, 130, H = 1, 3
INF = float("inf")

_dtype, maxerr = TP._dtype, TP.maxerr


def _run(qkv, kvc, mask, bias, H, mode, acc, **kw):
    """CPU operands -> the device in the mode's dtype; ``acc`` is cloned, added onto in place and returned (on the device)"""
    from mdm_hip import ops

    dt = _dtype(mode)
    a = acc.to(DEV).clone()
    with ops.fp32_split(mode == "split"):   # (constructing the switch sets it: only ever inside a with)
        out = ops.attn_cross_maps(qkv.to(DEV, dt), kvc.to(DEV, dt), None if mask is None else mask.to(DEV), H, a,
                                  bias=None if bias is None else bias.to(DEV), **kw)
    assert out.data_ptr() == a.data_ptr()
    return out


def _same_bits(a, b):
    """equal bit for bit, NaN payloads included"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,H,L,S", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_matches_the_fp64_restatement(d, H, L, S, mode):
    """B = 3, with and without the mask of pag_cases (one full, one holed + tail-masked, one fully masked row), with and
    without the bias of region_cases (-inf entries, a dead band of queries, NaN pad columns), w = 0.75 onto a random acc
    whose pad columns hold NaN.  The operands are rounded to the mode's dtype for kernel and reference alike and the
    probabilities stay fp32, so bf16 is expected at the fp32 level too (printed; the gate is the mode's)."""
    dt = _dtype(mode)
    qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))   # the values the kernel sees
    acc0 = AC.kernel_acc(L, S)
    assert acc0.shape[-1] > S and acc0.shape[-1] % 4 == 0 and torch.isnan(acc0[..., S:]).all()
    for mask in (PG.masks(S), None):
        for bias in (RC.kernel_bias(L, S), None):
            out = _run(qkv, kvc, mask, bias, H, mode, acc0, weight=0.75).cpu()
            want = AC.cross_maps_ref(qkv, kvc, mask, bias, H, acc0, 0.75)
            err = maxerr(out[..., :S], want[..., :S])
            inc = float(((out[..., :S].double() - acc0[..., :S].double()) - (want[..., :S] - acc0[..., :S].double())).abs().max())
            print("d=%d H=%d L=%d S=%d %s mask=%s bias=%s: %.2e (the increment alone, absolute: %.2e)"
                  % (d, H, L, S, mode, mask is not None, bias is not None, err, inc))
            assert torch.isfinite(out[..., :S]).all() and err < GATE[mode]
            assert _same_bits(out[..., S:], acc0[..., S:])   # the pad columns still hold their NaN


@pytest.mark.parametrize("mode", MODES)
def test_exact_identities(mode):
    """bit for bit: w_host = 0 and *w_dev = 0 leave acc alone; one live key adds exactly 1 there and 0 elsewhere; q = 0 with
    2^k live keys adds exactly 2^-k; fully masked rows and dead-band queries are unchanged; -inf bias on the keys a mask
    zeroes = that mask with zero bias; a row range of a larger batch = the launch on that slice; two runs are equal"""
    dt = _dtype(mode)
    for d, H, L, S in AC.EXACT_CASES:
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d, seed=7))
        acc0, bias, mask = AC.kernel_acc(L, S, seed=1), RC.kernel_bias(L, S), PG.masks(S)
        ld = acc0.shape[-1]
        # the two gates
        one, zero_gate = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
        assert _same_bits(_run(qkv, kvc, mask, bias, H, mode, acc0, weight=0.0).cpu(), acc0)
        assert _same_bits(_run(qkv, kvc, mask, bias, H, mode, acc0, weight=0.0, gate=one).cpu(), acc0)
        assert _same_bits(_run(qkv, kvc, mask, bias, H, mode, acc0, gate=zero_gate).cpu(), acc0)
        full = _run(qkv, kvc, mask, bias, H, mode, acc0)
        assert _same_bits(_run(qkv, kvc, mask, bias, H, mode, acc0, gate=one), full)   # w = 1 * 1
        assert _same_bits(_run(qkv, kvc, mask, bias, H, mode, acc0), full)             # two identical runs
        assert not torch.equal(full.cpu()[0, :, :S], acc0[0, :, :S])
        # the fully masked batch row 2; the dead band of batch row 2 under the bias alone
        assert _same_bits(full.cpu()[2], acc0[2])
        nomask = _run(qkv, kvc, None, bias, H, mode, acc0).cpu()
        lo, hi = RC.dead_band(L)
        assert _same_bits(nomask[2, lo:hi], acc0[2, lo:hi])
        live = [i for i in (lo - 1, hi) if 0 <= i < L]
        assert live and all(not torch.equal(nomask[2, i, :S], acc0[2, i, :S]) for i in live)
        # -inf bias on the keys the mask zeroes
        zero = torch.zeros(3, L, ld)
        zero[..., S:] = float("nan")
        dead = zero.clone()
        dead[..., :S] = torch.where(mask == 0, -INF, 0.0)[:, None, :]
        want = _run(qkv, kvc, mask, zero, H, mode, acc0)
        assert _same_bits(_run(qkv, kvc, None, dead, H, mode, acc0), want)
        assert _same_bits(_run(qkv, kvc, mask, dead, H, mode, acc0), want)
        assert _same_bits(_run(qkv, kvc, mask, None, H, mode, acc0), want)   # zero bias = no bias
        # rows [1, 3) of the batch of 3 = the launch on that slice alone (a batch row's result does not depend on B)
        part = _run(qkv, kvc, mask, bias, H, mode, acc0[1:3], row0=1, rows=2)
        assert _same_bits(part, full[1:3])
        assert _same_bits(_run(qkv[1:3], kvc[1:3], mask[1:3], bias[1:3], H, mode, acc0[1:3]), full[1:3])
        assert _same_bits(_run(qkv[2:3], kvc[2:3], None, bias[2:3], H, mode, acc0[2:3]).cpu(), nomask[2:3])
    for H in (1, 2, 4):
        for d, L, S in ((32, 80, 5), (64, 16, 130), (128, 80, 77)):
            qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d, seed=3))
            acc0 = AC.kernel_acc(L, S, seed=2)
            ld = acc0.shape[-1]
            # one live key per query (key l mod S), by the bias and by the mask
            key = torch.arange(L) % S
            only = torch.full((3, L, ld), -INF)
            only[:, torch.arange(L), key] = 0.7
            hit = torch.zeros(3, L, ld)
            hit[:, torch.arange(L), key] = 1.0
            want = torch.where(hit != 0, acc0 + 1.0, acc0)
            assert _same_bits(_run(qkv, kvc, None, only, H, mode, acc0).cpu(), want)
            m1 = torch.zeros(3, S)
            m1[:, S // 2] = 1
            hit = torch.zeros(3, L, ld)
            hit[:, :, S // 2] = 1.0
            assert _same_bits(_run(qkv, kvc, m1, None, H, mode, acc0).cpu(), torch.where(hit != 0, acc0 + 1.0, acc0))
            # q = 0: uniform over the 2^k live keys, spread over the key tiles
            for k in range(0, 8):
                if 2 ** k > S:
                    break
                idx = torch.linspace(0, S - 1, 2 ** k).round().long().unique()
                if len(idx) != 2 ** k:
                    idx = torch.arange(2 ** k)
                mk = torch.zeros(3, S)
                mk[:, idx] = 1
                hit = torch.zeros(3, L, ld)
                hit[:, :, idx] = 1.0
                out = _run(torch.zeros_like(qkv), kvc, mk, None, H, mode, acc0).cpu()
                assert _same_bits(out, torch.where(hit != 0, acc0 + 2.0 ** -k, acc0)), (H, d, L, S, k)


@pytest.mark.parametrize("mode", MODES)
def test_row_sums(mode):
    """sum_s of the increment = w for the live queries, 0 for the others -- within the fp32 gate in every mode (the
    probabilities are never rounded)"""
    dt = _dtype(mode)
    for d, H, L, S in KERNEL_CASES:
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))
        mask, bias = PG.masks(S), RC.kernel_bias(L, S)
        C = H * d
        _, live = AC.probs_ref(qkv[..., :C].transpose(1, 2), kvc[..., :C].transpose(1, 2), H, mask, bias)
        out = _run(qkv, kvc, mask, bias, H, mode, torch.zeros(3, L, bias.shape[-1]), weight=1.75).cpu()
        sums = out[..., :S].double().sum(-1)
        err = float((sums[live] - 1.75).abs().max() / 1.75) if live.any() else 0.0
        print("d=%d H=%d L=%d S=%d %s: row sums off by %.2e" % (d, H, L, S, mode, err))
        assert err < GATE["fp32"] and torch.equal(sums[~live], torch.zeros_like(sums[~live]))
        assert torch.equal(out[..., S:], torch.zeros_like(out[..., S:]))


@pytest.mark.parametrize("mode", MODES)
def test_maps_times_values_is_the_cross_term_of_the_kernel_it_mirrors(mode):
    """H = 1 (one head: the head mean is that head's map), small-integer v_c: maps . v_c formed in fp64 against the cross
    term ops.attn_cross_bias adds onto a zero base, within that kernel's gate"""
    from mdm_hip import ops

    dt = _dtype(mode)
    for d, H, L, S in [c for c in KERNEL_CASES if c[1] == 1]:
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))
        C = H * d
        g = torch.Generator().manual_seed(d + L + S)
        kv = torch.cat([kvc[..., :C], torch.randint(-8, 9, (3, S, C), generator=g).float()], dim=-1)
        mask, bias = PG.masks(S), RC.kernel_bias(L, S)
        maps = _run(qkv, kv, mask, bias, H, mode, torch.zeros(3, L, bias.shape[-1])).cpu()
        with torch.no_grad(), ops.fp32_split(mode == "split"):
            cross = ops.attn_cross_bias(qkv.to(DEV, dt), kv.to(DEV, dt), mask.to(DEV), bias.to(DEV), H,
                                        base=torch.zeros(3, L, C, device=DEV, dtype=dt)).float().cpu()
        want = torch.einsum("bls,bsc->blc", maps[..., :S].double(), kv[..., C:].double())
        err = maxerr(cross, want)
        print("d=%d L=%d S=%d %s: %.2e" % (d, L, S, mode, err))
        assert err < GATE[mode]


def test_operand_checks():
    from mdm_hip import _lib, ops

    N, L, S, H, d = 2, 16, 5, 1, 32
    qkv, kvc = torch.randn(N, L, 3 * d, device=DEV), torch.randn(N, S, 2 * d, device=DEV)
    acc = torch.zeros(N, L, 8, device=DEV)
    for bad, match in ((dict(acc=torch.zeros(N, L, 6, device=DEV)), "acc"), (dict(acc=torch.zeros(N, L, 4, device=DEV)), "acc"),
                       (dict(acc=torch.zeros(1, L, 8, device=DEV)), "acc"), (dict(acc=acc.double()), "fp32"),
                       (dict(bias=torch.zeros(N, L, 6, device=DEV)), "bias"), (dict(gate=torch.ones(2, device=DEV)), "gate"),
                       (dict(row0=1, rows=2), "rows"), (dict(kvc=None), "no text keys")):
        kw = dict(qkv=qkv, kvc=kvc, mask=None, heads=H, acc=acc)
        kw.update(bad)
        with pytest.raises(_lib.MdmHipError, match=match):
            ops.attn_cross_maps(**kw)
    # legal where a tape is recorded: it reads detached values
    leaf = qkv.clone().requires_grad_(True)
    with torch.enable_grad():
        out = ops.attn_cross_maps(leaf * 1.0, kvc, None, H, acc)
    assert not out.requires_grad and float(out.sum()) == pytest.approx(N * L, rel=1e-5)


# ---- the models against the oracle with a recording hook --------------------------------------------------------------------
def _forward(name, mode, maps=None):
    """batch 4 (PG.model_inputs); ``maps``: record every layer with text keys, every row"""
    import contextlib

    from mdm_hip import attn_maps as A, ops

    model = TP._gpu_model(name)
    inp = PG.model_inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), auto, ops.fp32_split(mode == "split"):
        with (A.record(model, maps) if maps is not None else contextlib.nullcontext()):
            outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    return [o.float().cpu() for o in PC.as_list(outs)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_models_record_the_maps_of_the_oracle(name, mode):
    """fp32 / split: rel-L2 of every resolution's maps below 1e-4, the mini-model gate.  bf16: at most 2x the rel-L2 of the
    same bf16 forward's outputs from the oracle (the convention of test_regions_gpu.py).  The forward's outputs are the same
    bits with and without recording."""
    import mdm_hip
    from mdm_hip import attn_maps as A

    model = TP._gpu_model(name)
    names = A.layer_names(model, "all")
    S = PG.model_inputs(name)["cond"].shape[1]
    maps = mdm_hip.AttnMaps(S, 4)
    outs, plain = _forward(name, mode, maps), _forward(name, mode)
    assert all(torch.equal(o, p) for o, p in zip(outs, plain))
    ref, ref_outs = AC.oracle_maps(name, names)
    got = maps.maps()
    assert set(got) == set(ref) and sum(maps.counts().values()) == len(names)
    e_out = max(O.rel_l2(o, r) for o, r in zip(outs, ref_outs))
    for key in sorted(got):
        e = O.rel_l2(got[key].cpu().double(), ref[key])
        print("%s %s maps %s (%d layers): rel-L2 %.3e; the forward's outputs: %.3e" % (name, mode, key, maps.counts()[key], e, e_out))
        assert e <= 2 * e_out if mode == "bf16" else e < 1e-4
    hm = maps.heatmap(16)
    assert tuple(hm.shape) == (4, S, 16, 16) and torch.isfinite(hm).all()


def test_graphed_denoiser_runs_eagerly_under_record():
    """never a graph captured with a caller's recorder, never one captured without it replayed in its place"""
    import mdm_hip
    from mdm_hip import attn_maps as A
    from mdm_hip.graph import GraphedDenoiser

    model = TP._gpu_model("mini_unet")
    gd = GraphedDenoiser(model)
    inp = PG.model_inputs("mini_unet")
    args = (inp["x"].to(DEV), inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV))
    a, b = mdm_hip.AttnMaps(inp["cond"].shape[1], 4), mdm_hip.AttnMaps(inp["cond"].shape[1], 4)
    with torch.no_grad():
        plain = gd(*args)
        assert len(gd._graphs) == 1
        with A.record(model, a):
            assert torch.equal(gd(*args), plain)
        with A.record(model, b):
            assert torch.equal(model(*args), plain)
        assert len(gd._graphs) == 1 and a.counts() == b.counts() and sum(a.counts().values()) > 0
        assert all(torch.equal(a.maps()[k], b.maps()[k]) for k in a.maps())
        assert torch.equal(gd(*args), plain) and len(gd._graphs) == 1


# ---- the samplers ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    return torch.equal(a, b)


def _options(name, kw):
    kw = dict(kw)
    if kw.pop("regions", False):
        kw["regions"] = RC.model_regions(name, DEV)
    return kw


@pytest.mark.parametrize("name,kw,interval", AC.SAMPLER_CASES, ids=AC.SAMPLER_IDS)
def test_samplers_record_without_changing_a_bit(name, kw, interval):
    """eager and graphed, twice (the second call through the cached graph, with other noise): the images are those of the
    call without attn_maps bit for bit, the eager maps are the graphed maps bit for bit, and the counts are steps x layers"""
    import mdm_hip
    from mdm_hip import attn_maps as A

    s = TR._fresh(name)
    kw = _options(name, kw)
    S = s.cond.shape[1]
    names = A.layer_names(s.pipe.get_model().vision_model, "all")
    steps = s.pipe.sampler.set_timesteps(4)[:-1]
    for rep, seed in enumerate((51, 52)):
        xs = s.start(seed)
        me, mg = mdm_hip.AttnMaps(S, 2, interval=interval), mdm_hip.AttnMaps(S, 2, interval=interval)
        want = s.eager(xs, **kw)
        assert _same(s.eager(xs, attn_maps=me, **kw), want)
        assert _same(s.graphed(xs, attn_maps=mg, **kw), want) and len(s.gs._graphs) == 1
        n_on = sum(me.on(t, 1000) for t in steps)
        assert 0 < n_on and (interval is None) == (n_on == len(steps))
        assert me.counts() == mg.counts() and sum(me.counts().values()) == n_on * len(names)
        em, gm = me.maps(), mg.maps()
        for key in em:
            assert torch.equal(em[key], gm[key]), (rep, key)
            sums = em[key].sum(dim=1)
            print("%s call %d maps %s: %d pairs, token sums in [%.6f, %.6f]" % (name, rep, key, me.counts()[key],
                                                                                float(sums.min()), float(sums.max())))
            assert torch.allclose(sums, torch.ones_like(sums), atol=1e-4)   # every conditional row has live keys
        if "regions" in kw:   # tokens 0-3 live in the left region: exactly 0 where the pooled region is 0
            left = RC.seam_regions(RC.side_of(name))[0]
            for (h, w), m in em.items():
                gone = (torch.nn.functional.avg_pool2d(left, RC.side_of(name) // h) == 0)[:, 0].to(DEV)   # [2, h, w]
                assert gone.any() and not gone.all()
                for tok in range(4):
                    assert torch.equal(m[:, tok][gone], torch.zeros_like(m[:, tok][gone])) and float(m[:, tok][~gone].max()) > 0


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_attn_maps_none_is_the_call_without_the_argument(name):
    import mdm_hip

    s = TR._fresh(name)
    xs = s.start(53)
    for run in (s.eager, s.graphed):
        for kw in (dict(ddim_eta=0), dict(solver="dpmpp_2m")):
            assert _same(run(xs, attn_maps=None, **kw), run(xs, **kw)), (run.__name__, kw)
    assert len(s.gs._graphs) == 2   # attn_maps=None adds no graph
    # an interval that selects no step: the same images, and the maps stay zero, eager and graphed
    for run in (s.eager, s.graphed):
        m = mdm_hip.AttnMaps(s.cond.shape[1], 2, interval=(0.0, 0.0))
        assert _same(run(xs, ddim_eta=0, attn_maps=m), run(xs, ddim_eta=0))
        assert sum(m.counts().values()) == 0 and all(not v.any() for v in m.maps().values())
    assert len(s.gs._graphs) == 3   # the recorder's graph is one more
    # ... which another interval replays
    m = mdm_hip.AttnMaps(s.cond.shape[1], 2)
    s.graphed(xs, ddim_eta=0, attn_maps=m)
    assert len(s.gs._graphs) == 3 and sum(m.counts().values()) > 0
