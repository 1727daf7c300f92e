"""CPU: FreeU without a GPU -- the closed form of the Fourier filter against its ``torch.fft`` definition, the oracle copy
with FreeU levels (identity at b = s = 1, non-trivial at the model-level settings), the block selection and every refusal
on CPU-constructed models, the ``applied`` switch, the samplers on a recording stub, and the new C-ABI entries."""
import ctypes

import pytest
import torch

import freeu_cases as FC
import parity_cases as PC
import unet_oracle as O
from mdm_hip import FreeU, freeu   # (the parent has neither: every test of this file fails there at import)


# ---- the closed form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (4, 6), (7, 16), (16, 16)])
def test_closed_form_is_the_fft_definition(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    r = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    for s in (0.2, 0.9, 1.0, 1.7):
        err = float((FC.closed_form(r, s) - FC.fourier_filter_ref(r, s)).abs().max())
        print("(%d, %d) s=%g: %.2e" % (H, W, s, err))
        assert err <= 1e-12
    # and the filter does what the paper says: a constant image is scaled by s, a checkerboard (the highest frequency) stays
    const = torch.full((1, 1, H, W), 2.0, dtype=torch.float64)
    assert float((FC.closed_form(const, 0.2) - 0.4).abs().max()) < 1e-12
    if H % 2 == 0 and W % 2 == 0 and H > 2 and W > 2:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        board = (1.0 - 2.0 * ((yy + xx) % 2)).double().reshape(1, 1, H, W)
        assert float((FC.closed_form(board, 0.2) - board).abs().max()) < 1e-12


def test_fp32_closed_form_error_is_the_recorded_figure():
    """the yardstick of the GPU tests' elementwise gate: measured here, recorded in freeu_cases.py"""
    err = FC.closed_form_fp32_error()
    print("fp32 closed form against the fp64 definition, worst |error| / max |input|: %.3e (recorded %.3e, c = %.3e)"
          % (err, FC.FP32_CLOSED_FORM_ERROR, FC.C_GATE))
    assert 0.5 * FC.FP32_CLOSED_FORM_ERROR <= err <= FC.FP32_CLOSED_FORM_ERROR
    assert FC.C_GATE == 8 * FC.FP32_CLOSED_FORM_ERROR


def test_freeu_ref_follows_the_definition():
    h, r = FC.kernel_inputs((2, 5, 3, 32, 24))
    out = FC.freeu_ref(h, r, 1.4, 0.2)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, 56, 5, 3)
    assert torch.equal(out[:, :16], h[:, :16].double() * 1.4) and torch.equal(out[:, 16:32], h[:, 16:].double())
    assert torch.equal(out[:, 32:], FC.fourier_filter_ref(r, 0.2))
    v2 = FC.freeu_ref(h, r, 1.4, 0.2, structure=True)
    m = v2[:, :16] / h[:, :16].double()
    assert float(m.min()) >= 1.0 - 1e-12 and float(m.max()) <= 1.4 + 1e-12
    assert abs(float(m[0].max()) - 1.4) < 1e-12 and abs(float(m[0].min()) - 1.0) < 1e-12   # hm spans [0, 1] per sample
    flat = torch.ones(1, 4, 3, 3)   # max mu == min mu: the v1 result
    assert torch.equal(FC.freeu_ref(flat, flat, 1.4, 1.0, True)[:, :2], flat[:, :2].double() * 1.4)


# ---- the oracle copy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_oracle_copy_is_the_oracle_at_unit_parameters(name):
    plain = FC.oracle_outputs(name)
    for structure in (False, True):
        for a, b in zip(plain, FC.oracle_outputs(name, (1.0, 1.0), (1.0, 1.0), structure)):
            assert torch.equal(a, b)
    want, _ = PC.oracle_run(name, with_grad=False)
    assert all(torch.equal(a, b) for a, b in zip(plain, want))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_model_level_settings_are_not_vacuous(name):
    plain = FC.oracle_outputs(name)
    for structure in (False, True):
        for i, (a, b) in enumerate(zip(plain, FC.oracle_outputs(name, FC.MODEL_B, FC.MODEL_S, structure))):
            moved = O.rel_l2(b, a)
            print("%s structure=%s out %d: b = %s, s = %s moves the oracle by rel-L2 %.3e" % (name, structure, i, FC.MODEL_B,
                                                                                              FC.MODEL_S, moved))
            assert moved > 1e-2


# ---- selection and validation --------------------------------------------------------------------------------------------
MODELS = {}


def model(name):
    if name not in MODELS:
        MODELS[name] = PC.build_module(name)[0]
    return MODELS[name]


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested", "mini_nested2"])
def test_select_deepest2(name):
    m, pfx = model(name), FC.INNER[name]
    cfg = FreeU(b=(1.1, 1.2), s=(0.9, 0.8))
    sel = freeu.select(m, cfg)
    assert [(n, b, s) for n, _, b, s in sel] == [(pfx + "up_blocks.0", 1.1, 0.9), (pfx + "up_blocks.1", 1.2, 0.8)]
    inner = m.get_submodule(pfx[:-1]) if pfx else m
    assert not hasattr(inner, "inner_unet")                     # the innermost net ...
    assert sel[0][1] is inner.up_blocks[0] and sel[1][1] is inner.up_blocks[1]   # ... lowest resolution first
    assert sel[0][1].upsample_output and all(mod is m.get_submodule(n) for n, mod, _, _ in sel)
    assert freeu.graph_key(m, cfg) == ("freeu", (pfx + "up_blocks.0", pfx + "up_blocks.1"), (1.1, 1.2), (0.9, 0.8), False)
    assert {k: v for k, v in FC.deepest2(name, (1.1, 1.2), (0.9, 0.8)).items()} == {n: (b, s) for n, _, b, s in sel}


def test_select_by_name_and_errors():
    m = model("mini_nested")
    cfg = FreeU(levels={"up_blocks.1": (1.3, 0.5), "inner_unet.up_blocks.0": (1.1, 0.9)}, structure=True)
    sel = freeu.select(m, cfg)   # named_modules() order: the inner net comes after the outer blocks
    assert [(n, b, s) for n, _, b, s in sel] == [("up_blocks.1", 1.3, 0.5), ("inner_unet.up_blocks.0", 1.1, 0.9)]
    assert freeu.graph_key(m, cfg)[-1] is True
    assert [n for n, _ in freeu.up_blocks(m)] == ["up_blocks.0", "up_blocks.1", "inner_unet.up_blocks.0", "inner_unet.up_blocks.1"]
    with pytest.raises(ValueError, match="no up block named"):
        freeu.select(m, FreeU(levels={"inner_unet.up_blocks.7": (1.1, 0.9)}))
    with pytest.raises(ValueError, match="no up block named"):
        freeu.select(m, FreeU(levels={"inner_unet.down_blocks.0": (1.1, 0.9)}))   # a ResNetBlock, not on the up path
    with pytest.raises(ValueError, match="selects no up block"):
        freeu.select(m, FreeU(levels={}))
    with pytest.raises(ValueError, match="selects no up block"):
        freeu.select(torch.nn.Linear(2, 2), FreeU(b=(1.1, 1.1), s=(0.9, 0.9)))
    with pytest.raises(ValueError, match="wanted a mdm_hip.FreeU"):
        freeu.select(m, (1.1, 0.9))


def test_parameter_refusals():
    inf, nan = float("inf"), float("nan")
    for bad in (0.0, -1.0, inf, nan):
        with pytest.raises(ValueError, match="b = "):
            FreeU(b=(1.2, bad), s=(0.9, 0.9))
        with pytest.raises(ValueError, match="b = "):
            FreeU(levels={"up_blocks.0": (bad, 0.9)})
    for bad in (-0.1, inf, nan):
        with pytest.raises(ValueError, match="s = "):
            FreeU(b=(1.2, 1.2), s=(bad, 0.9))
    FreeU(b=(1.2, 1.2), s=(0.0, 0.9))   # s = 0 removes the four bins: allowed
    cfg = FreeU(b=(1.2, 1.2), s=(0.9, 0.9))
    cfg.b = (1.2, nan)   # select checks again: a config edited after construction
    with pytest.raises(ValueError, match="b = "):
        freeu.select(model("mini_unet"), cfg)
    with pytest.raises(ValueError, match="threshold"):
        FreeU(b=(1.2, 1.2), s=(0.9, 0.9), threshold=2)
    with pytest.raises(ValueError, match="required"):
        FreeU()                                   # no defaults are shipped
    with pytest.raises(ValueError, match="required"):
        FreeU(b=(1.2, 1.2))
    with pytest.raises(ValueError, match="known sets"):
        FreeU(b=(1.2, 1.2), s=(0.9, 0.9), levels="deepest3")
    with pytest.raises(ValueError, match="pair"):
        FreeU(b=1.2, s=(0.9, 0.9))
    with pytest.raises(ValueError, match="not given beside"):
        FreeU(b=(1.2, 1.2), levels={"up_blocks.0": (1.1, 0.9)})


def test_applied_sets_and_restores():
    from mdm_hip.unet import ResNetBlock

    m = model("mini_nested")
    blocks = [mod for mod in m.modules() if isinstance(mod, ResNetBlock)]
    lo, hi = m.inner_unet.up_blocks[0], m.inner_unet.up_blocks[1]
    assert ResNetBlock._freeu is None and all(b._freeu is None for b in blocks)
    with freeu.applied(m, FreeU(b=(1.3, 1.2), s=(0.4, 0.5), structure=True)):
        assert lo._freeu == (1.3, 0.4, True) and hi._freeu == (1.2, 0.5, True) and lo._freeu_name == "inner_unet.up_blocks.0"
        assert all(b._freeu is None for b in blocks if b is not lo and b is not hi)
        with freeu.applied(m, FreeU(levels={"inner_unet.up_blocks.0": (1.1, 0.9), "up_blocks.0": (1.5, 1.0)})):
            assert lo._freeu == (1.1, 0.9, False) and m.up_blocks[0]._freeu == (1.5, 1.0, False) and hi._freeu == (1.2, 0.5, True)
        assert lo._freeu == (1.3, 0.4, True) and m.up_blocks[0]._freeu is None
    assert all(b._freeu is None and "_freeu" not in b.__dict__ and "_freeu_name" not in b.__dict__ for b in blocks)
    with pytest.raises(RuntimeError, match="boom"):
        with freeu.applied(m, FreeU(b=(1.3, 1.2), s=(0.4, 0.5))):
            raise RuntimeError("boom")
    assert all(b._freeu is None for b in blocks)
    assert len(m.state_dict()) == len(PC.build_module("mini_nested")[2])   # plain attributes: the state dict is the reference's


# ---- the samplers on the recording stub ------------------------------------------------------------------------------------
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
    return x, lm, mask


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
@pytest.mark.parametrize("kw", [dict(ddim_eta=0), dict(solver="dpmpp_2m"), dict(ddim_eta=0, pag_scale=1.5)],
                         ids=["ddim0", "dpmpp_2m", "pag"])
def test_switch_is_held_around_every_model_call(nested, kw):
    smp, stub = _sampler(nested), FC.RecordingStub(nested)
    if "pag_scale" in kw:   # the perturbed rows need an attention layer to select
        import pag_cases as PG

        stub.mid_blocks = PG.RecordingStub(nested).mid_blocks
    x, lm, mask = _inputs(2.0, nested)
    cfg = FreeU(b=(1.4, 1.2), s=(0.2, 0.5), structure=True)
    run = lambda **more: smp.sample(stub, x, lm, mask, {}, resample_steps=True, num_inference_steps=3, guidance_scale=2.0,
                                    **kw, **more)
    out = run(freeu=cfg)
    assert len(stub.calls) == 3
    assert all(c["freeu"] == (1.4, 0.2, True) and c["name"] == "up_blocks.0" for c in stub.calls)
    assert stub.up_blocks[0]._freeu is None and "_freeu" not in stub.up_blocks[0].__dict__
    stub.calls.clear()
    plain, none = run(), run(freeu=None)
    assert len(stub.calls) == 6 and all(c["freeu"] is None for c in stub.calls)
    assert torch.equal(plain, none) and not torch.equal(out, plain)
    # a yield_output generator holds the switch during the calls only, never across a yield
    stub.calls.clear()
    gen = run(freeu=cfg, yield_output=True)
    for _ in range(3):
        next(gen)
        assert stub.up_blocks[0]._freeu is None and stub.calls[-1]["freeu"] == (1.4, 0.2, True)


def test_get_xt_minus_1_takes_the_switch_too():
    smp, stub = _sampler(), FC.RecordingStub()
    x, lm, mask = _inputs(1)
    a = smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, time_step_last=400, ddim_eta=0, freeu=FreeU(b=(1.4, 1.4), s=(0.2, 0.2)))
    b = smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, time_step_last=400, ddim_eta=0)
    assert stub.calls[0]["freeu"] == (1.4, 0.2, False) and stub.calls[1]["freeu"] is None and not torch.equal(a, b)


def test_refusals_of_the_samplers_and_the_op():
    import inspect

    from mdm_hip import LossGuide, _lib, ops
    from mdm_hip.graph import GraphedSampler
    from mdm_hip.samplers import SampleOptions

    smp, stub = _sampler(), FC.RecordingStub()
    x, lm, mask = _inputs(2.0)
    cfg = FreeU(b=(1.4, 1.4), s=(0.2, 0.2))
    guide = LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        smp.sample(stub, x, lm, mask, {}, guide=guide, freeu=cfg, **kw)
    with pytest.raises(NotImplementedError, match="no backward"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, guide=guide, freeu=cfg)
    with pytest.raises(ValueError, match="wanted a mdm_hip.FreeU"):
        smp.sample(stub, x, lm, mask, {}, freeu=(1.4, 0.2), **kw)
    assert not stub.calls
    # the keyword reaches GraphedSampler.sample through its **options: the fields of SampleOptions, with their defaults
    sig = inspect.signature(GraphedSampler.sample).parameters
    assert sig["options"].kind is inspect.Parameter.VAR_KEYWORD and SampleOptions().freeu is None
    h, r = torch.randn(1, 4, 4, 16), torch.randn(1, 4, 4, 8)
    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.concat_freeu(h, r, 1.4, 0.2, False)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_the_plan_refuses_what_the_kernels_cannot_do():
    from mdm_hip import _lib

    assert len(_lib.header_prototypes()) == 85 and _lib.ABI_VERSION == 6   # the drop-in boundary is untouched
    ext = {name: argnames for name, _, _, argnames in _lib.header_prototypes(_lib.EXT_HEADER)}
    assert ext["mdm_freeu_plan"] == ["N", "H", "W", "C1", "C2", "dtype", "structure", "ws_bytes"]
    assert ext["mdm_freeu_stats"][:4] == ["h", "r", "ws", "ws_bytes"] and ext["mdm_freeu_apply"][-5:] == ["b", "s", "structure", "dtype", "stream"]
    L = _lib.lib()
    ws = ctypes.c_size_t(0)
    plan = lambda *a: L.mdm_freeu_plan(*a, ctypes.byref(ws))
    assert plan(2, 8, 8, 256, 256, 1, 0) == 0 and ws.value >= 2 * 7 * 256 * 4
    v1 = ws.value
    assert plan(2, 8, 8, 256, 256, 1, 1) == 0 and ws.value >= v1 + (2 * 64 + 4) * 4      # + mu and min / max
    assert plan(1, 2, 2, 16, 8, 1, 0) == 0 and plan(1, 2, 2, 8, 4, 0, 0) == 0             # the smallest legal shapes
    assert plan(1, 1, 8, 16, 8, 1, 0) < 0 and plan(1, 8, 1, 16, 8, 1, 0) < 0              # H == 1 or W == 1 breaks the identity
    assert plan(1, 8, 8, 24, 8, 1, 0) < 0 and plan(1, 8, 8, 16, 12, 1, 0) < 0             # bf16: C1 % 16, C2 % 8
    assert plan(1, 8, 8, 12, 4, 0, 0) < 0 and plan(1, 8, 8, 8, 6, 0, 0) < 0               # fp32: C1 % 8, C2 % 4
    assert plan(1, 8, 8, 16, 8, 7, 0) < 0 and L.mdm_freeu_plan(1, 8, 8, 16, 8, 1, 0, None) < 0
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # argument checks come before any launch
    assert L.mdm_freeu_stats(None, None, p, 1 << 16, 1, 8, 8, 16, 8, 0, 1, None) < 0      # no skip
    assert L.mdm_freeu_stats(None, p, p, 1 << 16, 1, 8, 8, 16, 8, 1, 1, None) < 0         # structure without the backbone
    assert L.mdm_freeu_stats(p, p, p, 16, 1, 8, 8, 16, 8, 0, 1, None) < 0                 # a workspace below the plan
    assert L.mdm_freeu_apply(p, p, p, 1 << 16, p, 1, 8, 8, 16, 8, 1.4, 0.2, 0, 1, None) < 0          # out aliases an input
    q = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for b, s in ((0.0, 0.2), (float("nan"), 0.2), (float("inf"), 0.2), (1.4, -0.1), (1.4, float("nan"))):
        assert L.mdm_freeu_apply(p, p, p, 1 << 16, q, 1, 8, 8, 16, 8, b, s, 0, 1, None) < 0
