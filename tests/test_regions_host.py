"""CPU: regional prompts and token weights without a GPU -- the fp64 restatement's identities on biases that
``RegionPrompts`` builds, the bias values against hand-computed pooled logs, guidance / PAG rows, the in-place cache rewrite,
``concat``, the ``applied`` switch on CPU-constructed models and on a recording stub under the samplers, the refusals, and
the new C-ABI entry."""
import ctypes
import inspect
import math

import pytest
import torch

import parity_cases as PC
import region_cases as RC
import unet_oracle as O

INF = float("inf")


def _qkv(B=2, L=16, S=6, H=2, d=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = H * d
    return (torch.randn(B, L, 3 * C, generator=g, dtype=torch.float64), torch.randn(B, S, 2 * C, generator=g, dtype=torch.float64),
            H, C)


def _core(qkv, kvc, H, C, mask=None):
    kv = kvc.transpose(1, 2)
    return O.attention_core(qkv[..., :C].transpose(1, 2), kv[:, :C], kv[:, C:], H, mask).transpose(1, 2)


def test_restatement_identities_on_region_prompt_biases():
    """zero bias = attention_core; a zero weight (-inf bias) = mask 0; one weight on every token (a uniform shift) changes
    nothing; a single live key gives v_c; a query with no live key gets base"""
    import mdm_hip

    qkv, kvc, H, C = _qkv()
    B, L, S = 2, 16, 6
    v = qkv[..., 2 * C:]
    rp = mdm_hip.RegionPrompts(S, 4, [], rows=B)
    zero = rp.bias(B, 4, 4)
    assert zero.shape == (B, L, 8) and zero.dtype == torch.float32
    want = v + _core(qkv, kvc, H, C)
    assert float((RC.cross_bias_ref(qkv, kvc, None, zero, H) - want).abs().max()) < 1e-14
    # zero weight on tokens 1, 4 of row 0 and 0-2 of row 1 = mask 0 there
    w = torch.ones(B, S)
    w[0, [1, 4]] = 0
    w[1, :3] = 0
    dead = mdm_hip.RegionPrompts(S, 4, [(0, S, None, w)], rows=B).bias(B, 4, 4)
    assert torch.equal(dead[..., :S] == -INF, (w == 0)[:, None, :].expand(B, L, S))
    a = RC.cross_bias_ref(qkv, kvc, None, dead, H)
    assert torch.equal(a, RC.cross_bias_ref(qkv, kvc, w, zero, H))
    assert float((a - (v + _core(qkv, kvc, H, C, w))).abs().max()) < 1e-14
    # a uniform shift: weight 1.4 on every token
    shift = mdm_hip.RegionPrompts(S, 4, [(0, S, None, 1.4)], rows=B).bias(B, 4, 4)
    assert float((shift[..., :S] - math.log(1.4)).abs().max()) < 1e-7
    assert float((RC.cross_bias_ref(qkv, kvc, None, shift, H) - want).abs().max()) < 1e-14
    # a single live key: the cross term is v_c of that key; base = something else than v
    one = torch.zeros(B, S)
    one[:, 2] = 1
    single = mdm_hip.RegionPrompts(S, 4, [(0, S, None, one)], rows=B).bias(B, 4, 4)
    base = torch.randn(B, L, C, dtype=torch.float64)
    got = RC.cross_bias_ref(qkv, kvc, None, single, H, base=base)
    assert float((got - (base + kvc[:, 2:3, C:])).abs().max()) < 1e-14
    # no live key in the left half of the image: base there, bit for bit
    left = torch.zeros(B, 1, 4, 4)
    left[..., 2:] = 1
    none = mdm_hip.RegionPrompts(S, 4, [(0, S, left, 1.0)], rows=B).bias(B, 4, 4)
    got = RC.cross_bias_ref(qkv, kvc, None, none, H, base=base).reshape(B, 4, 4, C)
    assert torch.equal(got[:, :, :2], base.reshape(B, 4, 4, C)[:, :, :2])
    assert float((got[:, :, 2:] - (base + _core(qkv, kvc, H, C)).reshape(B, 4, 4, C)[:, :, 2:]).abs().max()) < 1e-14


def test_bias_values_padding_and_rows():
    import mdm_hip

    rows, S, side = 2, 5, 8
    g = torch.Generator().manual_seed(3)
    region = torch.rand(rows, 1, side, side, generator=g)
    region[0, 0, :4, :4] = 0                      # a whole 4 x 4 block of zeros: -inf at (h, w) = (2, 2)
    wt = torch.tensor([[2.0, 0.0], [0.5, 1.0]])
    rp = mdm_hip.RegionPrompts(S, side, [(0, 2, region, 1.5), (3, 5, None, wt)], rows=rows)
    assert rp.ld == 8 and mdm_hip.regions.RegionPrompts is mdm_hip.RegionPrompts and "RegionPrompts" in mdm_hip.__all__
    for h in (8, 4, 2):
        b = rp.bias(rows, h, h)
        assert b.shape == (rows, h * h, 8) and b.dtype == torch.float32
        r = side // h
        for row in range(rows):
            for y in range(h):
                for x in range(h):
                    mean = float(region[row, 0, y * r:(y + 1) * r, x * r:(x + 1) * r].double().mean())
                    want = math.log(1.5) + math.log(mean) if mean > 0 else -INF
                    for tok in (0, 1):
                        got = float(b[row, y * h + x, tok])
                        assert got == want if want == -INF else abs(got - want) < 1e-6 * max(1.0, abs(want)), (h, row, y, x)
        assert torch.equal(b[:, :, 2], torch.zeros(rows, h * h))                # a token in no span
        assert float((b[0, :, 3] - math.log(2.0)).abs().max()) < 1e-7 and bool((b[0, :, 4] == -INF).all())
        assert float((b[1, :, 3] - math.log(0.5)).abs().max()) < 1e-7 and bool((b[1, :, 4] == 0).all())
        assert bool((b[:, :, S:] == -INF).all())                                # the pad columns: excluded whatever reads them
        assert rp.bias(rows, h, h) is b                                         # cached
    assert float(rp.bias(rows, 2, 2)[0, 0, 0]) == -INF and float(rp.bias(rows, 4, 4)[0, 0, 0]) == -INF
    assert math.isfinite(float(rp.bias(rows, 2, 2)[0, 1, 0]))
    # guidance rows: [uncond | cond] -- zero bias in front; [uncond | cond | perturbed]: the cond rows once more
    cond = rp.bias(rows, 4, 4)
    two, three = rp.bias(2 * rows, 4, 4), rp.bias(3 * rows, 4, 4)
    assert bool((two[:rows, :, :S] == 0).all()) and bool((two[:rows, :, S:] == -INF).all()) and torch.equal(two[rows:], cond)
    assert torch.equal(three[: 2 * rows], two) and torch.equal(three[2 * rows:], cond)
    pert = rp.rows_for(guidance=False, pag_rows=True)                           # [cond | perturbed] at guidance 1
    assert pert.rows == 2 * rows and torch.equal(pert.bias(2 * rows, 4, 4), torch.cat([cond, cond]))
    assert rp.rows_for(True, True).bias(3 * rows, 4, 4) is three and rp.rows_for().bias(rows, 4, 4) is cond
    # a mixed-resolution nested batch: another number of rows
    with pytest.raises(ValueError, match="mixed-resolution"):
        rp.bias(rows + 1, 4, 4)
    with pytest.raises(ValueError, match="mixed-resolution"):
        pert.bias(rows, 4, 4)
    # set_spans rewrites every cached tensor in place
    ptrs = {k: t.data_ptr() for k, t in rp._cache.items()}
    before = three.clone()
    rp.set_spans([(0, 5, 1 - region, 1.0)])
    assert {k: t.data_ptr() for k, t in rp._cache.items()} == ptrs and rp.bias(3 * rows, 4, 4) is three
    assert not torch.equal(three, before) and bool((three[:rows, :, :S] == 0).all())
    fresh = mdm_hip.RegionPrompts(S, side, [(0, 5, 1 - region, 1.0)], rows=rows)
    assert torch.equal(three, fresh.bias(3 * rows, 4, 4)) and torch.equal(cond, fresh.bias(rows, 4, 4))
    # a rectangular image with square pixel blocks
    rect = mdm_hip.RegionPrompts(3, (8, 16), [(0, 3, torch.ones(1, 1, 8, 16), 2.0)], rows=1)
    assert rect.bias(1, 4, 8).shape == (1, 32, 4)


def test_every_value_error():
    import mdm_hip

    RP = mdm_hip.RegionPrompts
    ok = torch.ones(2, 1, 8, 8)
    for spans, match in (
        ([(0, 3, None, 1.0), (2, 5, None, 1.0)], "overlap"),
        ([(3, 3, None, 1.0)], "span"),
        ([(0, 6, None, 1.0)], "span"),
        ([(-1, 2, None, 1.0)], "span"),
        ([(0, 2, None)], "a span is"),
        ([(0, 2, torch.ones(2, 1, 4, 4), 1.0)], "region"),
        ([(0, 2, torch.ones(1, 1, 8, 8), 1.0)], "region"),
        ([(0, 2, ok * 1.5, 1.0)], r"leaves \[0, 1\]"),
        ([(0, 2, ok - 1.5, 1.0)], r"leaves \[0, 1\]"),
        ([(0, 2, None, 0.0)], "weight"),
        ([(0, 2, None, -1.0)], "weight"),
        ([(0, 2, None, INF)], "weight"),
        ([(0, 2, None, torch.ones(2, 3))], "weight"),
        ([(0, 2, None, -torch.ones(2, 2))], "weight"),
    ):
        with pytest.raises(ValueError, match=match):
            RP(5, 8, spans, rows=2)
    with pytest.raises(ValueError):
        RP(0, 8, [], rows=2)
    with pytest.raises(ValueError):
        RP(5, 8, [], rows=0)
    with pytest.raises(ValueError, match="image_size"):
        RP(5, (8, 8, 8), [], rows=2)
    rp = RP(5, 8, [(0, 2, ok, 1.0)], rows=2)
    for h, w in ((3, 3), (16, 16), (4, 8), (0, 0)):
        with pytest.raises(ValueError, match="divisible"):
            rp.bias(2, h, w)
    with pytest.raises(ValueError, match="overlap"):
        rp.set_spans([(0, 3, None, 1.0), (1, 2, None, 1.0)])
    assert rp.spans[0][1] == 2   # a refused set_spans leaves the spans alone


def test_concat():
    from mdm_hip import regions

    g = torch.Generator().manual_seed(5)
    rows, D = 2, 4
    a, b = torch.randn(rows, 3, D, generator=g), torch.randn(rows, 2, D, generator=g)
    ma, mb = torch.ones(rows, 3), torch.tensor([[1.0, 0.0], [1.0, 1.0]])
    reg = torch.ones(rows, 1, 8, 8)
    ent, spans = regions.concat([(a, ma, reg, 1.5), (b, mb)])
    assert torch.equal(ent["lm_outputs"], torch.cat([a, b], dim=1)) and torch.equal(ent["lm_mask"], torch.cat([ma, mb], dim=1))
    assert spans[0] == (0, 3, reg, 1.5) and spans[1] == (3, 5, None, 1.0)
    # a shorter unconditional text is padded: zero states, mask 0
    u, mu = torch.randn(rows, 2, D, generator=g), torch.ones(rows, 2)
    ent, spans = regions.concat([(a, ma, reg, 1.5), (b, mb)], uncond=(u, mu))
    lm, m = ent["lm_outputs"], ent["lm_mask"]
    assert lm.shape == (2 * rows, 5, D) and torch.equal(lm[:rows, :2], u) and bool((lm[:rows, 2:] == 0).all())
    assert torch.equal(m[:rows], torch.tensor([[1.0, 1, 0, 0, 0]] * rows)) and torch.equal(lm[rows:], torch.cat([a, b], dim=1))
    assert len(spans) == 2
    # a longer one pads the conditional text: zero states, mask 0 and a -inf bias column
    u, mu = torch.randn(rows, 7, D, generator=g), torch.ones(rows, 7)
    ent, spans = regions.concat([(a, ma, reg, 1.5), (b, mb)], uncond=(u, mu))
    lm, m = ent["lm_outputs"], ent["lm_mask"]
    assert lm.shape == (2 * rows, 7, D) and torch.equal(lm[:rows], u) and bool((lm[rows:, 5:] == 0).all())
    assert bool((m[rows:, 5:] == 0).all()) and torch.equal(m[rows:, :5], torch.cat([ma, mb], dim=1))
    rp = regions.RegionPrompts(7, 8, spans, rows=rows)
    bias = rp.bias(2 * rows, 4, 4)
    assert bool((bias[rows:, :, 5:7] == -INF).all()) and bool((bias[:rows, :, :7] == 0).all())
    assert float((bias[rows:, :, :3] - math.log(1.5)).abs().max()) < 1e-7
    doc = " ".join(regions.concat.__doc__.lower().split())
    assert "whole concatenated sequence" in doc and "forward_conditioning" in doc
    with pytest.raises(ValueError):
        regions.concat([])
    with pytest.raises(ValueError):
        regions.concat([(a, mb)])


def test_applied_sets_and_restores():
    import mdm_hip
    from mdm_hip import regions
    from mdm_hip.unet import SelfAttention

    m = PC.build_module("mini_nested")[0]
    layers = {n: mod for n, mod in m.named_modules() if isinstance(mod, SelfAttention)}
    text = {n for n, mod in layers.items() if mod.cond_dim}
    assert SelfAttention._cross_bias is None and text and all(mod._cross_bias is None for mod in layers.values())
    rp = mdm_hip.RegionPrompts(8, 32, [], rows=2)
    other = mdm_hip.RegionPrompts(8, 32, [], rows=2)
    assert set(regions.layer_names(m, "all")) == text
    mid = regions.layer_names(m, "mid")
    with regions.applied(m, rp, "mid"):
        assert all((mod._cross_bias is rp) == (n in mid) for n, mod in layers.items())
        with regions.applied(m, other):   # "all" is the default
            assert all((mod._cross_bias is other) == (n in text) for n, mod in layers.items())
        assert all((mod._cross_bias is rp) == (n in mid) for n, mod in layers.items())
    assert all(mod._cross_bias is None and "_cross_bias" not in mod.__dict__ for mod in layers.values())
    with pytest.raises(RuntimeError, match="boom"):
        with regions.applied(m, rp, "all"):
            raise RuntimeError("boom")
    assert all(mod._cross_bias is None for mod in layers.values())
    with pytest.raises(ValueError, match="no SelfAttention layer named"):
        regions.applied(m, rp, ["nope"])
    with pytest.raises(ValueError, match="bias"):
        regions.applied(m, object())
    assert len(m.state_dict()) == len(PC.build_module("mini_nested")[2])   # a plain attribute: the reference's state dict
    # a layer without text keys is never selected; a selection of such layers only is refused
    stub = RC.RecordingStub()
    assert regions.layer_names(stub, "all") == ("mid_blocks.0.attn.0", "down_blocks.0.attn.0")
    with pytest.raises(ValueError, match="text keys"):
        regions.layer_names(stub, ["down_blocks.0.attn.1"])


# ---- the samplers on a recording stub -----------------------------------------------------------------------------------
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
def test_stub_sees_the_handle_during_the_denoiser_call_only(w, pag_scale, nested):
    import mdm_hip

    smp, stub = _sampler(nested), RC.RecordingStub(nested)
    x, lm, mask, micros = _inputs(w, nested)
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    layout = (("uncond",) if w != 1 else ()) + ("cond",) + (("cond",) if pag_scale else ())
    kw = dict(resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=w, pag_scale=pag_scale)
    idle = lambda: all(m._cross_bias is None for m in stub.attention().values())
    gen = smp.sample(stub, x, lm, mask, micros, regions=rp, region_layers=["down_blocks.0.attn.0"], yield_output=True, **kw)
    assert idle() and not stub.seen
    for n, _ in enumerate(gen, 1):
        assert idle() and len(stub.seen) == min(n, 3)   # between the items of the generator: nothing is held across a yield
    assert len(stub.seen) == 3
    for seen in stub.seen:
        assert seen == {"mid_blocks.0.attn.0": None, "down_blocks.0.attn.0": (len(layout) * B, layout), "down_blocks.0.attn.1": None}
    assert all(c["pag_rows"] == (B if pag_scale else 0) for c in stub.calls)
    # "all": both layers with text keys, never the one without
    stub.seen.clear()
    out = smp.sample(stub, x, lm, mask, micros, regions=rp, **kw)
    assert [sorted(n for n, v in s.items() if v) for s in stub.seen] == [["down_blocks.0.attn.0", "mid_blocks.0.attn.0"]] * 3
    # regions=None is the call without the argument (the stub ignores the bias: so is every other call here)
    stub.seen.clear()
    a = smp.sample(stub, x, lm, mask, micros, regions=None, region_layers="nonsense is not even resolved", **kw)
    b = smp.sample(stub, x, lm, mask, micros, **kw)
    assert all(v is None for s in stub.seen for v in s.values()) and len(stub.seen) == 6
    for u, v, o in zip(a if nested else [a], b if nested else [b], out if nested else [out]):
        assert torch.equal(u, v) and torch.equal(u, o)
    # an exception in the denoiser leaves no handle behind
    stub.forward = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        smp.sample(stub, x, lm, mask, micros, regions=rp, **kw)
    assert idle()


def test_refusals():
    import mdm_hip
    from mdm_hip import LossGuide
    from mdm_hip.graph import GraphedDenoiser, GraphedSampler

    smp, stub = _sampler(), RC.RecordingStub()
    x, lm, mask, micros = _inputs(2.0)
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    guide = LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        smp.sample(stub, x, lm, mask, micros, guide=guide, regions=rp, **kw)
    with pytest.raises(NotImplementedError, match="no backward"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, guide=guide, regions=rp)
    with pytest.raises(ValueError, match="RegionPrompts"):
        smp.sample(stub, x, lm, mask, micros, regions="left", **kw)
    with pytest.raises(ValueError, match="rows"):
        smp.sample(stub, x, lm, mask, micros, regions=mdm_hip.RegionPrompts(S, 8, [], rows=B + 1), **kw)
    with pytest.raises(ValueError, match="selects no attention layer"):
        smp.sample(stub, x, lm, mask, micros, regions=rp, region_layers=lambda n: False, **kw)
    assert not stub.calls
    # the keywords reach these through their ** keywords: the fields of SampleOptions, with their defaults
    from mdm_hip.samplers import SampleOptions

    for fn, name in ((GraphedSampler.sample, "options"), (smp._sample, "post_args"), (smp.get_xt_minus_1, "options")):
        assert inspect.signature(fn).parameters[name].kind is inspect.Parameter.VAR_KEYWORD
    assert SampleOptions().regions is None and SampleOptions().region_layers == "all"
    assert "eager" in GraphedDenoiser.__doc__.lower()


def test_ops_are_inference_only_and_gpu_only():
    from mdm_hip import _lib, ops

    qkv, kvc, bias = torch.randn(1, 16, 96), torch.randn(1, 3, 64), torch.zeros(1, 16, 4)
    for fn in (ops.attn_cross_bias, ops.attention_biased):
        with pytest.raises(_lib.MdmHipError, match="MI355X"):
            fn(qkv, kvc, None, bias, 1)


def test_new_entry_is_declared_and_exported():
    from mdm_hip import _lib

    protos = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert protos["mdm_attn_cross_bias"][1] == ["qkv", "kvc", "mask", "bias", "bias_ld", "base", "base_ld", "out", "B", "L", "S",
                                                "H", "d", "dtype", "stream"]
    assert protos["mdm_attn_cross_bias"][0][4] is ctypes.c_int and protos["mdm_attn_cross_bias"][0][6] is ctypes.c_int
    assert len(_lib.header_prototypes()) == 85 and _lib.ABI_VERSION == 6   # the drop-in header is as it was
    assert "mdm_attn_cross_bias" not in {p[0] for p in _lib.header_prototypes()}
    L = _lib.lib()
    fn = L.mdm_attn_cross_bias
    assert fn.argtypes == protos["mdm_attn_cross_bias"][0]
    # argument checks come before any launch: null tensors, an unsupported head dim or dtype, a short or ragged bias row
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    ok = dict(qkv=p, kvc=p, mask=None, bias=p, bias_ld=8, base=p, base_ld=32, out=p, B=1, L=16, S=5, H=1, d=32, dtype=0,
              stream=None)
    bad = [dict(qkv=None), dict(kvc=None), dict(bias=None), dict(base=None), dict(out=None), dict(d=48), dict(dtype=7),
           dict(bias_ld=4), dict(bias_ld=6), dict(bias_ld=7), dict(S=0), dict(B=0), dict(L=0), dict(H=0), dict(base_ld=16),
           dict(base_ld=34)]
    for change in bad:
        args = dict(ok, **change)
        assert fn(*[args[k] for k in protos["mdm_attn_cross_bias"][1]]) < 0, change
