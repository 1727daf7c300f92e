"""CPU: perturbed-attention guidance without a GPU -- the layer selection and the ``perturbed`` switch on CPU-constructed
models, the assembly of the [uncond | cond | perturbed] batch on a recording stub, the torch combine and a 3-step
trajectory against fp64 restatements, the refusals, and the two new C-ABI entries."""
import ctypes

import pytest
import torch

import pag_cases as PG
import parity_cases as PC


def _models():
    import mdm_hip
    from mdm_hip import configs

    with torch.device("meta"):
        u64 = mdm_hip.UNet(3, 3, configs.unet64_config())
        n1024 = mdm_hip.NestedUNet(3, 3, configs.nested1024_config())
    return {"mini_unet": PC.build_module("mini_unet")[0], "unet64": u64, "mini_nested": PC.build_module("mini_nested")[0],
            "nested1024": n1024}


MODELS = None


def model(name):
    global MODELS
    if MODELS is None:
        MODELS = _models()
    return MODELS[name]


INNER = {"mini_unet": "", "unet64": "", "mini_nested": "inner_unet.", "nested1024": "inner_unet.inner_unet."}


@pytest.mark.parametrize("name", list(INNER))
def test_select_mid_deepest_all(name):
    from mdm_hip import pag
    from mdm_hip.unet import SelfAttention

    m, pfx = model(name), INNER[name]
    every = [n for n, mod in m.named_modules() if isinstance(mod, SelfAttention)]
    mid = pag.select(m)   # "mid" is the default
    assert [n for n, _ in mid] == [pfx + "mid_blocks.0.attn.0"] and mid[0][1] is m.get_submodule(mid[0][0])
    assert pag.layer_names(m, "mid") == (pfx + "mid_blocks.0.attn.0",)
    assert [n for n, _ in pag.select(m, "all")] == every and len(every) >= 4
    deep = [n for n, _ in pag.select(m, "deepest")]
    # the lowest resolution with attention: the last down block and the first up block of the innermost U-Net
    inner = m.get_submodule(pfx[:-1]) if pfx else m
    last = len(inner.down_blocks) - 1
    want = [n for n in every if n.startswith(pfx + "down_blocks.%d.attn." % last) or n.startswith(pfx + "up_blocks.0.attn.")]
    assert deep == want and len(deep) == len(inner.down_blocks[last].attn) + len(inner.up_blocks[0].attn)
    if name in ("unet64", "nested1024"):
        assert len(deep) == 25 and len(every) == 25 + 2 + 3 + 1   # levels 1 and 2: (2 + 3) x 1 and (2 + 3) x 5, + mid


def test_select_names_predicate_and_errors():
    import mdm_hip
    from mdm_hip import configs, pag

    m = model("mini_unet")
    assert [n for n, _ in pag.select(m, ["up_blocks.0.attn.1", "down_blocks.1.attn.0"])] == ["down_blocks.1.attn.0", "up_blocks.0.attn.1"]
    assert [n for n, _ in pag.select(m, lambda n: n.startswith("up_blocks"))] == ["up_blocks.0.attn.0", "up_blocks.0.attn.1"]
    with pytest.raises(ValueError, match="no SelfAttention layer named"):
        pag.select(m, ["mid_blocks.0.attn.7"])
    with pytest.raises(ValueError, match="selects no attention layer"):
        pag.select(m, lambda n: False)
    with pytest.raises(ValueError, match="known sets"):
        pag.select(m, "middle")
    cfg = configs.mini_unet_config()
    cfg.skip_mid_blocks = True
    with torch.device("meta"):
        nomid = mdm_hip.UNet(3, 3, cfg)
    with pytest.raises(ValueError, match="no mid blocks"):
        pag.select(nomid, "mid")
    assert len(pag.select(nomid, "all")) == 3
    assert mdm_hip.pag is pag and "pag" in mdm_hip.__all__


def test_perturbed_sets_and_restores():
    from mdm_hip import pag
    from mdm_hip.unet import SelfAttention

    m = model("mini_nested")
    layers = [mod for mod in m.modules() if isinstance(mod, SelfAttention)]
    mid = m.inner_unet.mid_blocks[0].attn[0]
    assert SelfAttention._pag_rows == 0 and all(l._pag_rows == 0 for l in layers)
    with pag.perturbed(m, "mid", rows=3):
        assert mid._pag_rows == 3 and all(l._pag_rows == 0 for l in layers if l is not mid)
        with pag.perturbed(m, "all", rows=2):
            assert all(l._pag_rows == 2 for l in layers)
        assert mid._pag_rows == 3 and all(l._pag_rows == 0 for l in layers if l is not mid)
    assert all(l._pag_rows == 0 and "_pag_rows" not in l.__dict__ for l in layers)
    with pytest.raises(RuntimeError, match="boom"):
        with pag.perturbed(m, "all", rows=1):
            raise RuntimeError("boom")
    assert all(l._pag_rows == 0 for l in layers)
    with pytest.raises(ValueError):
        pag.perturbed(m, "all", rows=-1)
    assert len(m.state_dict()) == len(PC.build_module("mini_nested")[2])   # a plain attribute: the state dict is the reference's


# ---- row assembly ----------------------------------------------------------------------------------------------------
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
    micros = {"scale": 10.0 + 50.0 * torch.rand(rows, generator=g), "note": "not per row"}
    x = [torch.randn(B, 3, 8, 8, generator=g) for _ in range(2)] if nested else torch.randn(B, 3, 8, 8, generator=g)
    return x, lm, mask, micros


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("w", [2.0, 1])
def test_row_assembly(w, nested):
    """batch 3B (2B at w = 1); the perturbed block carries the COND rows of lm_outputs, mask and the per-row micros; the
    model runs once, inside the context; pag_scale = 0 calls the model exactly as a call without the arguments"""
    smp, stub = _sampler(nested), PG.RecordingStub(nested)
    x, lm, mask, micros = _inputs(w, nested)
    kw = dict(time_step_last=400, guidance_scale=w, ddim_eta=0)
    smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, pag_scale=1.5, **kw)
    assert len(stub.calls) == 1
    c = stub.calls[0]
    reps = 3 if w != 1 else 2
    xs = c["x"] if nested else [c["x"]]
    for got, src in zip(xs, x if nested else [x]):
        assert got.shape[0] == reps * B and torch.equal(got, torch.cat([src] * reps))
    assert c["t"].shape[0] == reps * B and torch.equal(c["t"], torch.full((reps * B,), 699))
    assert c["pag_rows"] == B and stub.mid_blocks[0].attn[0]._pag_rows == 0
    assert torch.equal(c["lm"], torch.cat([lm, lm[-B:]])) and torch.equal(c["mask"], torch.cat([mask, mask[-B:]]))
    assert torch.equal(c["micros"]["scale"], torch.cat([micros["scale"], micros["scale"][-B:]]))
    assert not torch.equal(lm[:B], lm[-B:]) or w == 1   # uncond and cond rows are distinct: a swap would show
    # pag_scale = 0: the call of today
    stub.calls.clear()
    a = smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, pag_scale=0.0, pag_layers="nonsense is not even resolved", **kw)
    b = smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, **kw)
    ca, cb = stub.calls
    assert ca["pag_rows"] == 0 and cb["pag_rows"] == 0
    for u, v in zip(ca["x"] if nested else [ca["x"]], cb["x"] if nested else [cb["x"]]):
        assert u.shape[0] == (2 * B if w != 1 else B) and torch.equal(u, v)
    assert torch.equal(ca["lm"], lm) and torch.equal(ca["mask"], mask) and torch.equal(ca["micros"]["scale"], micros["scale"])
    for u, v in zip(a if nested else [a], b if nested else [b]):
        assert torch.equal(u, v)


# ---- combine and trajectory --------------------------------------------------------------------------------------------
def test_torch_combine_matches_fp64_restatement():
    from mdm_hip import samplers as SM

    g = torch.Generator().manual_seed(3)
    pu, pc, pp = (torch.randn(2, 3, 8, 8, generator=g) for _ in range(3))
    for w, s in ((2.0, 1.5), (7.5, 0.3), (1.0, 3.0)):
        for u in (pu, None):
            got = SM.pag_combine(pc, u, pp, w, s)
            want = PG.combine_ref(pc, u, pp, w, s)
            assert float(((got.double() - want).abs() / PG.combine_scale(pc, u, pp, w, s)).max()) < 1e-6
    # signs and roles, in numbers: p_u = 1, p_c = 2, p_hat = 4, w = 3, s = 0.5 -> 1 + 3 (2 - 1) + 0.5 (2 - 4) = 3
    one = torch.ones(1)
    assert float(SM.pag_combine(2 * one, one, 4 * one, 3.0, 0.5)) == 3.0
    assert float(SM.pag_combine(2 * one, None, 4 * one, 3.0, 0.5)) == 1.0


def _restated_trajectory(smp, stub, x, lm, mask, micros, w, s, n, nested):
    """fp64: n DDIM(0) steps of V-prediction with CLIP, the three predictions from three separate calls of the stub"""
    from mdm_hip import pag

    steps = smp.set_timesteps(n)
    xs = [v.double() for v in (x if nested else [x])]
    d = lambda t: t.double() if t.is_floating_point() else t
    cond_m = {k: (d(v[-B:]) if torch.is_tensor(v) else v) for k, v in micros.items()}
    unc_m = {k: (d(v[:B]) if torch.is_tensor(v) else v) for k, v in micros.items()}
    for i in range(n):
        t = torch.full((B,), int(steps[i]) - 1)
        run = lambda lm_, mic: [stub.one(v, t, d(lm_), mic, k) for k, v in enumerate(xs)]
        pc = run(lm[-B:], cond_m)
        pu = run(lm[:B], unc_m) if w != 1 else [None] * len(xs)
        with pag.perturbed(stub, "mid", rows=B):
            pp = run(lm[-B:], cond_m)
        g, gl = smp.gammas[steps[i]].double(), smp.gammas[steps[i + 1]].double()
        for k in range(len(xs)):
            p = PG.combine_ref(pc[k], pu[k], pp[k], w, s)
            x0 = (xs[k] * g.sqrt() - p * (1 - g).sqrt()).clip(-1, 1)
            eps = (xs[k] - x0 * g.sqrt()) / (1 - g).sqrt()
            xs[k] = x0 * gl.sqrt() + eps * (1 - gl).sqrt()
    return xs[0].clip(-1, 1)


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("w", [2.0, 1])
def test_three_step_ddim_trajectory_matches_restated_loop(w, nested):
    smp, stub = _sampler(nested), PG.RecordingStub(nested)
    x, lm, mask, micros = _inputs(w, nested, seed=5)
    out = smp.sample(stub, x, lm, mask, micros, resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=w,
                     pag_scale=1.5)
    assert len(stub.calls) == 3 and all(c["pag_rows"] == B for c in stub.calls)
    want = _restated_trajectory(smp, stub, x, lm, mask, micros, w, 1.5, 3, nested)
    err = float((out.double() - want).abs().max() / want.abs().max())
    print("w=%s nested=%s: %.2e" % (w, nested, err))
    assert err < 1e-5
    free = smp.sample(stub, x, lm, mask, micros, resample_steps=True, num_inference_steps=3, ddim_eta=0, guidance_scale=w)
    assert float((out - free).abs().max()) > 1e-3   # the guidance acts
    # dpmpp_2m takes the same combined prediction
    a = smp.sample(stub, x, lm, mask, micros, resample_steps=True, num_inference_steps=3, solver="dpmpp_2m", guidance_scale=w,
                   pag_scale=1.5)
    b = smp.sample(stub, x, lm, mask, micros, resample_steps=True, num_inference_steps=3, solver="dpmpp_2m", guidance_scale=w)
    assert torch.isfinite(a).all() and float((a - b).abs().max()) > 1e-3


# ---- refusals and the C ABI -----------------------------------------------------------------------------------------------
def test_refusals():
    from mdm_hip import LossGuide
    from mdm_hip.graph import GraphedSampler

    smp, stub = _sampler(), PG.RecordingStub()
    x, lm, mask, micros = _inputs(2.0)
    guide = LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        smp.sample(stub, x, lm, mask, micros, guide=guide, pag_scale=1.0, **kw)
    with pytest.raises(NotImplementedError):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, guide=guide, pag_scale=1.0)
    with pytest.raises(ValueError, match="pag_scale"):
        smp.sample(stub, x, lm, mask, micros, pag_scale=-0.5, **kw)
    with pytest.raises(ValueError, match="pag_scale"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, micros, pag_scale=-1)
    assert not stub.calls
    with pytest.raises(ValueError, match="selects no attention layer"):
        smp.sample(stub, x, lm, mask, micros, pag_scale=1.0, pag_layers="deepest", **kw)
    import inspect

    from mdm_hip.samplers import SampleOptions

    # the keywords reach GraphedSampler.sample through its **options: the fields of SampleOptions, with their defaults
    sig = inspect.signature(GraphedSampler.sample).parameters
    assert sig["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert SampleOptions().pag_scale == 0.0 and SampleOptions().pag_layers == "mid"


def test_new_entries_are_declared_and_exported():
    from mdm_hip import _lib

    protos = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes()}
    assert len(protos) == 85 and _lib.ABI_VERSION == 6
    assert protos["mdm_attn_cross_addv"][1] == ["qkv", "kvc", "mask", "out", "B", "L", "S", "H", "d", "dtype", "stream"]
    assert protos["mdm_pag_combine"][1] == ["pred", "pred_uncond", "pred_pert", "guidance", "pag_scale", "out", "n", "stream"]
    assert protos["mdm_pag_combine"][0][6] is ctypes.c_size_t
    L = _lib.lib()
    # argument checks come before any launch: null tensors, an unsupported head dim, text keys without a length
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mdm_attn_cross_addv(None, None, None, p, 1, 16, 0, 1, 32, 0, None) < 0
    assert L.mdm_attn_cross_addv(p, None, None, None, 1, 16, 0, 1, 32, 0, None) < 0
    assert L.mdm_attn_cross_addv(p, None, None, p, 1, 16, 0, 1, 48, 0, None) < 0
    assert L.mdm_attn_cross_addv(p, p, None, p, 1, 16, 0, 1, 32, 0, None) < 0
    assert L.mdm_attn_cross_addv(p, None, None, p, 1, 16, 0, 1, 32, 7, None) < 0
    assert L.mdm_pag_combine(None, None, p, 1.0, 1.0, p, 4, None) < 0
    assert L.mdm_pag_combine(p, None, p, 1.0, 1.0, p, 4, None) < 0   # out may alias pred only
