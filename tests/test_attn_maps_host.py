"""CPU: cross-attention maps -- the torch restatement of mdm_attn_cross_maps against the fp64 definition of
tests/attn_map_cases.py, ``AttnMaps`` (validation, interval, counts, maps / heatmap), the switch, the samplers on a recording
stub (the handle is held on the selected layers around the denoiser call only, for the conditional rows), the refusals and
the declaration of the entry point."""
import os
import re

import pytest
import torch

import attn_map_cases as AC
import pag_cases as PG
import parity_cases as PC
import region_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,L,S", [(32, 1, 16, 1), (32, 3, 80, 5), (64, 3, 80, 130), (128, 1, 16, 77)], ids=lambda v: str(v))
def test_torch_restatement_matches_fp64(d, H, L, S):
    """fp32 torch ops against fp64, four operand combinations, onto a random acc with NaN pad columns: 2e-5 of the
    reference's max-abs (the fp32 gate of the kernels), row sums w for live queries, pad columns untouched"""
    from mdm_hip import attn_maps as A

    qkv, kvc = PG.attn_inputs(L, S, H, d)
    acc0 = AC.kernel_acc(L, S)
    for mask in (PG.masks(S), None):
        for bias in (RC.kernel_bias(L, S), None):
            acc = acc0.clone()
            out = A.cross_maps(qkv, kvc, mask, H, acc, bias=bias, weight=0.75)
            assert out is acc
            want = AC.cross_maps_ref(qkv, kvc, mask, bias, H, acc0, 0.75)
            err = float((acc[..., :S].double() - want[..., :S]).abs().max() / want[..., :S].abs().max())
            assert err < 2e-5, (mask is not None, bias is not None, err)
            assert torch.isnan(acc[..., S:]).all()
            _, live = AC.probs_ref(qkv[..., :H * d].transpose(1, 2), kvc[..., :H * d].transpose(1, 2), H, mask, bias)
            inc = (acc[..., :S] - acc0[..., :S]).sum(-1)
            assert torch.allclose(inc[live], torch.full_like(inc[live], 0.75), atol=1e-5)
            assert torch.equal(acc[..., :S][~live], acc0[..., :S][~live])   # no live key: unchanged
    # weight 0 and gate 0 leave acc alone; rows [row0, row0 + rows) are the launch on that slice
    for kw in (dict(weight=0.0), dict(gate=torch.zeros(1))):
        acc = acc0.clone()
        A.cross_maps(qkv, kvc, None, H, acc, **kw)
        assert torch.equal(acc[..., :S], acc0[..., :S])
    a, b = acc0[1:3].clone(), acc0[1:3].clone()
    A.cross_maps(qkv, kvc, PG.masks(S), H, a, bias=RC.kernel_bias(L, S), row0=1, rows=2)
    A.cross_maps(qkv[1:3], kvc[1:3], PG.masks(S)[1:3], H, b, bias=RC.kernel_bias(L, S)[1:3])
    assert torch.equal(a[..., :S], b[..., :S])


# ---- AttnMaps ------------------------------------------------------------------------------------------------------------
def test_attn_maps_validation_interval_counts_maps_and_heatmap():
    import mdm_hip
    from mdm_hip import attn_maps as A

    assert mdm_hip.AttnMaps is A.AttnMaps and "AttnMaps" in mdm_hip.__all__ and "attn_maps" in mdm_hip.__all__
    for bad in (dict(S=0, rows=2), dict(S=5, rows=0), dict(S=5, rows=2, interval=(0.5,)), dict(S=5, rows=2, interval=(0.6, 0.4)),
                dict(S=5, rows=2, interval=(0.0, INF)), dict(S=5, rows=2, interval="ab"), dict(S=5, rows=2, layers=3)):
        with pytest.raises(ValueError, match="AttnMaps"):
            A.AttnMaps(**bad)
    m = A.AttnMaps(5, 2, interval=(0.25, 0.75))
    assert m.ld == 8 and m.layers == "all" and m.maps() == {} and m.counts() == {}
    assert [m.on(t, 1000) for t in (1000, 751, 750, 500, 250, 249, 0)] == [False, False, True, True, True, False, False]
    assert A.AttnMaps(5, 2).on(torch.tensor(7), 1000)   # no interval: every step, no value read
    with pytest.raises(ValueError, match="nothing recorded"):
        m.heatmap(8)
    # two resolutions through the handle: 3 (step, layer) pairs at 4 x 4, 1 at 2 x 2; H = 2, d = 32
    g = torch.Generator().manual_seed(3)
    kvc = torch.randn(2, 5, 128, generator=g)
    mask = torch.ones(2, 5)
    mask[1, 3:] = 0
    h = A.BatchRows(m, 0, 2)
    qs = {(4, 4): [torch.randn(2, 16, 192, generator=g) for _ in range(3)], (2, 2): [torch.randn(2, 4, 192, generator=g)]}
    for (hh, ww), lst in qs.items():
        for qkv in lst:
            h.record(qkv, kvc, mask, 2, None, 2, hh, ww)
    assert m.counts() == {(4, 4): 3, (2, 2): 1}
    maps = m.maps()
    assert {k: tuple(v.shape) for k, v in maps.items()} == {(4, 4): (2, 5, 4, 4), (2, 2): (2, 5, 2, 2)}
    for (hh, ww), v in maps.items():
        assert v.dtype == torch.float32 and torch.allclose(v.sum(dim=1), torch.ones(2, hh, ww), atol=1e-5)   # a mean of softmaxes
        assert torch.equal(v[1, 3:], torch.zeros(2, hh, ww))                                                # masked tokens
        want = sum(AC.cross_maps_ref(q, kvc, mask, None, 2, torch.zeros(2, hh * ww, 8)) for q in qs[(hh, ww)]) / len(qs[(hh, ww)])
        assert torch.allclose(v.double(), want[..., :5].transpose(1, 2).reshape(2, 5, hh, ww), atol=1e-6)
    hm = m.heatmap((8, 12))
    assert tuple(hm.shape) == (2, 5, 8, 12) and torch.allclose(hm.sum(dim=1), torch.ones(2, 8, 12), atol=1e-5)
    up = lambda k: torch.nn.functional.interpolate(maps[k], size=(8, 8), mode="bilinear", align_corners=False)
    assert torch.allclose(m.heatmap(8), 0.75 * up((4, 4)) + 0.25 * up((2, 2)), atol=1e-6)
    with pytest.raises(ValueError, match="size"):
        m.heatmap((8, 8, 8))
    # the handle's checks: another batch (the message of RegionPrompts.layout_of), another token count
    with pytest.raises(ValueError, match="mixed-resolution nested batches are not supported"):
        h.record(qs[(2, 2)][0][:1], kvc[:1], mask[:1], 2, None, 1, 2, 2)
    with pytest.raises(ValueError, match="tokens"):
        h.record(qs[(2, 2)][0], kvc[:, :4], mask[:, :4], 2, None, 2, 2, 2)
    assert m.counts() == {(4, 4): 3, (2, 2): 1}
    assert m.reset() is m and m.maps() == {} and m.counts() == {}
    # the conditional block of [uncond | cond | perturbed]
    assert [(r.row0, r.rows, r.total) for r in (m.rows_for(), m.rows_for(True), m.rows_for(True, True), m.rows_for(False, True))] \
        == [(0, 2, 2), (2, 2, 4), (2, 2, 6), (0, 2, 4)]


def test_applied_and_record_set_and_restore():
    from mdm_hip import attn_maps as A
    from mdm_hip.unet import SWITCHES, SelfAttention

    m = PC.build_module("mini_nested")[0]
    layers = {n: mod for n, mod in m.named_modules() if isinstance(mod, SelfAttention)}
    text = {n for n, mod in layers.items() if mod.cond_dim}
    assert SelfAttention._attn_rec is None and "_attn_rec" in SWITCHES and all(mod._attn_rec is None for mod in layers.values())
    maps = A.AttnMaps(8, 2, layers="mid")
    handle = maps.rows_for(True)
    assert set(A.layer_names(m, "all")) == text
    mid = A.layer_names(m, "mid")
    with A.applied(m, handle, "mid"):
        assert all((mod._attn_rec is handle) == (n in mid) for n, mod in layers.items())
    assert all(mod._attn_rec is None and "_attn_rec" not in mod.__dict__ for mod in layers.values())
    with A.record(m, maps):   # the maps' own layers, every row
        got = {n: mod._attn_rec for n, mod in layers.items() if mod._attn_rec is not None}
        assert set(got) == set(mid) and all((r.row0, r.rows, r.total) == (0, 2, 2) for r in got.values())
    with A.record(m, maps, "all"):
        assert {n for n, mod in layers.items() if mod._attn_rec is not None} == text
    with pytest.raises(RuntimeError, match="boom"):
        with A.record(m, maps):
            raise RuntimeError("boom")
    assert all(mod._attn_rec is None for mod in layers.values())
    with pytest.raises(ValueError, match="record"):
        A.applied(m, object())
    with pytest.raises(ValueError, match="AttnMaps"):
        A.record(m, handle)
    with pytest.raises(ValueError, match="text keys"):
        A.layer_names(RC.RecordingStub(), ["down_blocks.0.attn.1"])
    assert len(m.state_dict()) == len(PC.build_module("mini_nested")[2])   # a plain attribute: the reference's state dict


# ---- the samplers on a recording stub -------------------------------------------------------------------------------------
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
def test_stub_sees_the_recorder_during_the_denoiser_call_only(w, pag_scale, nested):
    import mdm_hip

    smp, stub = _sampler(nested), AC.RecordingStub(nested)
    x, lm, mask, micros = _inputs(w, nested)
    maps = mdm_hip.AttnMaps(S, B, layers=["down_blocks.0.attn.0"])
    blocks = 1 + (w != 1) + bool(pag_scale)
    rows = (B if w != 1 else 0, B, blocks * B)   # the conditional block of [uncond | cond | perturbed]
    kw = dict(resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=w, pag_scale=pag_scale)
    idle = lambda: all(m._attn_rec is None for m in stub.attention().values())
    gen = smp.sample(stub, x, lm, mask, micros, attn_maps=maps, yield_output=True, **kw)
    assert idle() and not stub.rec_seen
    for n, _ in enumerate(gen, 1):
        assert idle() and len(stub.rec_seen) == min(n, 3)   # nothing is held across a yield
    assert stub.rec_seen == [{"mid_blocks.0.attn.0": None, "down_blocks.0.attn.0": rows, "down_blocks.0.attn.1": None}] * 3
    # "all": both layers with text keys, never the one without; with regions, both handles at once
    stub.rec_seen.clear()
    stub.seen.clear()
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    out = smp.sample(stub, x, lm, mask, micros, attn_maps=mdm_hip.AttnMaps(S, B), regions=rp, region_layers="mid", **kw)
    assert [sorted(n for n, v in s.items() if v) for s in stub.rec_seen] == [["down_blocks.0.attn.0", "mid_blocks.0.attn.0"]] * 3
    assert [sorted(n for n, v in s.items() if v) for s in stub.seen] == [["mid_blocks.0.attn.0"]] * 3
    # an interval: the steps start from 751, 500, 250 of 1000 -- only the middle one records
    stub.rec_seen.clear()
    smp.sample(stub, x, lm, mask, micros, attn_maps=mdm_hip.AttnMaps(S, B, interval=(0.5, 0.7)), **kw)
    assert [sorted(n for n, v in s.items() if v) for s in stub.rec_seen] == [[], ["down_blocks.0.attn.0", "mid_blocks.0.attn.0"], []]
    # attn_maps=None is the call without the argument, and resolves nothing
    stub.rec_seen.clear()
    a = smp.sample(stub, x, lm, mask, micros, attn_maps=None, **kw)
    b = smp.sample(stub, x, lm, mask, micros, **kw)
    assert all(v is None for s in stub.rec_seen for v in s.values()) and len(stub.rec_seen) == 6
    for u, v, o in zip(a if nested else [a], b if nested else [b], out if nested else [out]):
        assert torch.equal(u, v) and torch.equal(u, o)
    # an exception in the denoiser leaves no handle behind
    stub.forward = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        smp.sample(stub, x, lm, mask, micros, attn_maps=maps, **kw)
    assert idle()


def test_option_resolves_nothing_when_off_and_gains_a_component_when_on():
    import mdm_hip
    from mdm_hip.samplers import _UNCHANGED, SampleOptions

    stub = AC.RecordingStub()
    off = SampleOptions()
    assert off.attn_maps is None and off.switches(stub, 2.0, B) is _UNCHANGED
    assert off.layer_names(stub) == ((), ()) and off.graph_key(stub, 2.0, ((), ())) == ()
    maps = mdm_hip.AttnMaps(S, B, layers="mid", interval=(0.0, 0.5))
    on = SampleOptions(attn_maps=maps).check()
    names = on.layer_names(stub)
    assert names == ((), (), ("mid_blocks.0.attn.0",))
    assert on.graph_key(stub, 2.0, names) == (("attn_maps", S, 8, ("mid_blocks.0.attn.0",)),)
    assert on.switches(stub, 2.0, B, step=(900, 1000)) is _UNCHANGED   # outside the interval: nothing is set
    with on.switches(stub, 2.0, B, step=(400, 1000)):
        r = stub.mid_blocks[0].attn[0]._attn_rec
        assert (r.row0, r.rows, r.total) == (B, B, 2 * B) and stub.down_blocks[0].attn[0]._attn_rec is None
    assert stub.mid_blocks[0].attn[0]._attn_rec is None


def test_refusals():
    import mdm_hip
    from mdm_hip import Tiles
    from mdm_hip.samplers import SampleOptions

    smp, stub = _sampler(), AC.RecordingStub()
    x, lm, mask, micros = _inputs(2.0)
    maps = mdm_hip.AttnMaps(S, B)
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    assert ("attn_maps", "tiles") in SampleOptions.REFUSED
    with pytest.raises(NotImplementedError, match="window's queries"):
        smp.sample(stub, x, lm, mask, micros, attn_maps=maps, tiles=Tiles(8), **kw)
    with pytest.raises(NotImplementedError, match="window's queries"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, attn_maps=maps, tiles=Tiles(8))
    with pytest.raises(ValueError, match="AttnMaps"):
        smp.sample(stub, x, lm, mask, micros, attn_maps="yes", **kw)
    assert not stub.calls
    with pytest.raises(ValueError, match="rows"):
        smp.sample(stub, x, lm, mask, micros, attn_maps=mdm_hip.AttnMaps(S, B + 1), **kw)
    with pytest.raises(ValueError, match="selects no attention layer"):
        smp.sample(stub, x, lm, mask, micros, attn_maps=mdm_hip.AttnMaps(S, B, layers=lambda n: False), **kw)
    assert all(m._attn_rec is None for m in stub.attention().values())


def test_op_is_gpu_only_and_the_entry_is_declared_in_the_extension_header_only():
    from mdm_hip import _lib, ops

    with pytest.raises(_lib.MdmHipError, match="MI355X"):
        ops.attn_cross_maps(torch.randn(1, 16, 96), torch.randn(1, 3, 64), None, 1, torch.zeros(1, 16, 4))
    ext = open(os.path.join(ROOT, "include", "mdm_hip_ext.h")).read()
    main = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    assert re.search(r"\bint\s+mdm_attn_cross_maps\s*\(", ext) and "mdm_attn_cross_maps" not in main
    assert "mdm_attn_cross_maps" in {p[0] for p in _lib.header_prototypes(_lib.EXT_HEADER)}
    src = open(os.path.join(ROOT, "ml-mdm_amd", "csrc", "attention.hip")).read()
    assert 'extern "C" int mdm_attn_cross_maps' in src
    body = src[src.index("void attn_cross_maps_kernel"):]
    assert "atomic" not in body.lower() and "MDM_NOTE_ATTN(" not in body
