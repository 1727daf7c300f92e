"""GPU: FreeU on the HIP path -- ``ops.concat_freeu`` (mdm_freeu_stats + mdm_freeu_apply) against the fp64 definition of
tests/freeu_cases.py, its exact identities, the mini models under ``freeu.applied`` against the oracle with FreeU levels,
and the eager samplers against the graphed one.

Elementwise gate (freeu_cases.C_GATE = c): |out - ref| <= c max|input| in fp32, 2^-8 |ref| + c max|input| in bf16, with
c = 8 x the fp32 closed form's own error against fp64 on the CPU, 7.3e-8 -> c = 5.84e-7.
Measured on an MI355X (worst over the five shapes and both parameter pairs): fp32 |error| / max|input| 8.6e-8 (v1) and
1.3e-7 (v2); bf16 uses at most 0.996 of its bound (the rounding of the result itself); rel-L2 fp32 3.7e-8, bf16 1.5e-3.
Mini models: fp32 3.2e-6, split 2.2e-5, bf16 1.69e-2 against the FreeU oracle's own 1.83e-2 ... 2.05e-2."""
import functools

import pytest
import torch

import freeu_cases as FC
import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_GATE = {"fp32": 2e-5, "bf16": 3e-2}   # rel-L2, the project's op gates
MODES = list(OP_GATE)


def _dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _seen(shape, mode):
    """the case's (h, r), NCHW fp32, holding the values the kernel sees in this mode"""
    return tuple(t.to(_dtype(mode)).float() for t in FC.kernel_inputs(shape))


def _run(h, r, b, s, structure, mode):
    """NCHW fp32 on the CPU in, NCHW of the mode's dtype on the CPU out"""
    from mdm_hip import ops

    dt = _dtype(mode)
    with torch.no_grad():
        out = ops.concat_freeu(FC.nhwc(h).to(DEV, dt), FC.nhwc(r).to(DEV, dt), b, s, structure)
    assert out.dtype == dt and tuple(out.shape) == (h.shape[0], h.shape[2], h.shape[3], h.shape[1] + r.shape[1])
    return FC.nchw(out.cpu())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", FC.KERNEL_SHAPES, ids=str)
def test_exact_identities(shape, mode):
    from mdm_hip import ops

    dt = _dtype(mode)
    h, r = _seen(shape, mode)
    C1, half = h.shape[1], h.shape[1] // 2
    hd, rd = h.to(dt), r.to(dt)
    with torch.no_grad():
        plain = FC.nchw(ops.concat(FC.nhwc(h).to(DEV, dt), FC.nhwc(r).to(DEV, dt)).cpu())
    assert torch.equal(plain, torch.cat([hd, rd], dim=1))
    for structure in (False, True):
        assert torch.equal(_run(h, r, 1.0, 1.0, structure, mode), plain)                   # b = s = 1: the plain concat
        out = _run(h, r, 1.4, 0.2, structure, mode)
        assert torch.equal(out[:, half:C1], hd[:, half:])                                   # the untouched backbone half
        assert not torch.equal(out[:, :half], hd[:, :half]) and not torch.equal(out[:, C1:], rd)
        assert torch.equal(_run(h, r, 1.4, 0.2, structure, mode), out)                      # two runs: bit-equal
        assert torch.equal(_run(h, r, 1.4, 1.0, structure, mode)[:, C1:], rd)               # s = 1: the skip as it is
        assert torch.equal(_run(h, r, 1.0, 0.2, structure, mode)[:, :half], hd[:, :half])   # b = 1: the backbone as it is
    for b in (1.4, 0.7, 2.5):   # v1: one fp32 multiply, rounded to the dtype
        assert torch.equal(_run(h, r, b, 0.2, False, mode)[:, :half], (h[:, :half] * b).to(dt))
    # v2 where max mu == min mu: integer-valued h whose channels are, at every pixel, a permutation of one vector per
    # sample -- every partial sum is exact in any order, so mu is the same number everywhere -- equals v1 (b = 2.5 is
    # outside [0.5, 2], where 1 + (b - 1) is not b in fp32: the rule is hm = 1, not a rounding of it)
    N, _, H, W = h.shape
    g = torch.Generator().manual_seed(C1 + H)
    vec = torch.randint(-8, 9, (N, C1), generator=g).float()
    perm = torch.rand(N, H, W, C1, generator=g).argsort(dim=-1)
    hi = torch.gather(vec[:, None, None, :].expand(N, H, W, C1), 3, perm).permute(0, 3, 1, 2).contiguous()
    for b in (1.4, 2.5):
        assert torch.equal(_run(hi, r, b, 0.2, True, mode), _run(hi, r, b, 0.2, False, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("structure", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("shape", FC.KERNEL_SHAPES, ids=str)
def test_elementwise_error_against_the_fp64_definition(shape, structure, mode):
    h, r = _seen(shape, mode)
    top = float(max(h.abs().max(), r.abs().max()))
    for b, s in FC.KERNEL_PARAMS:
        out = _run(h, r, b, s, structure, mode).double()
        ref = FC.freeu_ref(h, r, b, s, structure)
        err = (out - ref).abs()
        bound = FC.C_GATE * top + (2.0 ** -8 * ref.abs() if mode == "bf16" else 0.0)
        l2 = O.rel_l2(out, ref)
        print("%s %s %s b=%g s=%g: worst |error| / max|input| %.3e (c = %.3e), worst |error| / bound %.3f, rel-L2 %.3e"
              % (shape, "v2" if structure else "v1", mode, b, s, float(err.max()) / top, FC.C_GATE, float((err / bound).max()), l2))
        assert torch.isfinite(out).all()
        assert bool((err <= bound).all())
        assert l2 < OP_GATE[mode]


def test_refusals():
    from mdm_hip import _lib, ops

    h, r = torch.randn(1, 4, 4, 16, device=DEV), torch.randn(1, 4, 4, 8, device=DEV)
    with torch.no_grad():
        for bad in (torch.randn(1, 1, 4, 16, device=DEV), torch.randn(1, 4, 1, 16, device=DEV)):
            with pytest.raises(_lib.MdmHipError, match="H, W >= 2"):
                ops.concat_freeu(bad, torch.randn(*bad.shape[:3], 8, device=DEV), 1.4, 0.2, False)
        with pytest.raises(_lib.MdmHipError, match=r"up_blocks\.0.*C1 = 12"):
            ops.concat_freeu(torch.randn(1, 4, 4, 12, device=DEV), r, 1.4, 0.2, False, layer="up_blocks.0")
        with pytest.raises(_lib.MdmHipError, match="C2 = 8"):   # bf16 wants C1 % 16
            ops.concat_freeu(torch.randn(1, 4, 4, 24, device=DEV).bfloat16(), r.bfloat16(), 1.4, 0.2, False)
        with pytest.raises(_lib.MdmHipError, match="differ in C only"):
            ops.concat_freeu(h, torch.randn(1, 4, 5, 8, device=DEV), 1.4, 0.2, False)
        for b, s in ((0.0, 0.2), (float("nan"), 0.2), (1.4, -0.1), (1.4, float("inf"))):
            with pytest.raises(_lib.MdmHipError, match="finite"):
                ops.concat_freeu(h, r, b, s, False)
    leaf = h.clone().requires_grad_(True)
    with torch.enable_grad(), pytest.raises(_lib.MdmHipError, match="inference only"):
        ops.concat_freeu(leaf, r, 1.4, 0.2, False)
    with torch.no_grad():   # ... and no complaint where no tape is recorded
        ops.concat_freeu(leaf, r, 1.4, 0.2, False)


# ---- the models against the oracle with FreeU levels ----------------------------------------------------------------------
MODEL_MODES = ["fp32", "split", "bf16"]


@functools.lru_cache(maxsize=None)
def _gpu_model(name):
    return PC.build_module(name)[0].to(DEV).eval()


def _forward(name, mode, cfg=None):
    import contextlib

    from mdm_hip import freeu, ops

    model = _gpu_model(name)
    inp = PC.inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), auto, ops.fp32_split(mode == "split"):
        with (freeu.applied(model, cfg) if cfg is not None else contextlib.nullcontext()):
            outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    return [o.float().cpu() for o in PC.as_list(outs)]


@pytest.mark.parametrize("mode", MODEL_MODES)
@pytest.mark.parametrize("structure", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_models_match_the_oracle_with_freeu_levels(name, structure, mode):
    """fp32 / split: rel-L2 1e-4, the mini-model gate.  bf16: no further from the fp32 FreeU oracle than that oracle's own
    bf16 run on the CPU.  After the ``with`` block the model computes what it computed before, bit for bit."""
    from mdm_hip import FreeU

    cfg = FreeU(b=FC.MODEL_B, s=FC.MODEL_S, structure=structure)
    before = _forward(name, mode)
    outs = _forward(name, mode, cfg)
    after = _forward(name, mode)
    ref = FC.oracle_outputs(name, FC.MODEL_B, FC.MODEL_S, structure)
    own = FC.oracle_outputs(name, FC.MODEL_B, FC.MODEL_S, structure, torch.bfloat16) if mode == "bf16" else ref
    for i, (o, p, q, r, w) in enumerate(zip(outs, before, after, ref, own)):
        err, bar, moved = O.rel_l2(o, r), O.rel_l2(w, r), O.rel_l2(o, p)
        print("%s %s %s out %d: rel-L2 %.3e against the FreeU oracle (the oracle's own bf16 run: %.3e); FreeU moves the output "
              "by %.3e" % (name, "v2" if structure else "v1", mode, i, err, bar, moved))
        assert err <= bar if mode == "bf16" else err < 1e-4
        assert moved > 1e-2 and torch.equal(p, q)


def test_graphed_denoiser_keys_on_the_switch():
    from mdm_hip import FreeU, freeu
    from mdm_hip.graph import GraphedDenoiser

    model = _gpu_model("mini_unet")
    gd = GraphedDenoiser(model)
    inp = PC.inputs("mini_unet")
    args = (inp["x"].to(DEV), inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV))
    with torch.no_grad():
        plain = gd(*args)
        assert torch.equal(plain, model(*args)) and len(gd._graphs) == 1
        with freeu.applied(model, FreeU(b=FC.MODEL_B, s=FC.MODEL_S)):
            scaled = gd(*args)
            assert torch.equal(scaled, model(*args))
        assert len(gd._graphs) == 2 and not torch.equal(scaled, plain)
        assert torch.equal(gd(*args), plain) and len(gd._graphs) == 2


# ---- the samplers ----------------------------------------------------------------------------------------------------------
RNG_SEED = 21
W = 2.0


class Setup:
    """one mini pipeline on the GPU, its text inputs [uncond | cond], eager and graphed runs of 4 steps from given noise"""

    def __init__(self, name):
        from mdm_hip import diffusion as D
        from mdm_hip import samplers as S
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested = name, name == "mini_nested"
        scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                               loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=self.nested,
                               rescale_signal=1 if self.nested else None)
        net = PC.build_module(name)[0]
        if self.nested:
            self.pipe = D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                       use_double_loss=True, no_use_residual=True))
        else:
            self.pipe = D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
        self.pipe = self.pipe.to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].to(DEV), inp["mask"].to(DEV)
        self.cond, self.mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.sample = {"lm_outputs": self.cond, "lm_mask": self.mask}
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, self.side, self.side, generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, self.side // 2, self.side // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=4, guidance_scale=W, **kw)

    def graphed(self, xs, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, self.side, torch.device(DEV), num_inference_steps=4, start_noise=xs,
                                  seed=RNG_SEED, guidance_scale=W, **kw)


@functools.lru_cache(maxsize=None)
def _setup(name):
    return Setup(name)


def _fresh(name):
    from mdm_hip.graph import GraphedSampler

    s = _setup(name)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    return s


def _cfg(structure=False, b=FC.MODEL_B, s=FC.MODEL_S):
    from mdm_hip import FreeU

    return FreeU(b=b, s=s, structure=structure)


@pytest.mark.parametrize("name,structure,kw", [
    ("mini_unet", False, dict(ddim_eta=0)),
    ("mini_nested", True, dict(ddim_eta=0)),
    ("mini_nested", False, dict(solver="dpmpp_2m")),
    ("mini_unet", True, dict(known=True)),                            # ancestral DDPM with a known half
    ("mini_unet", False, dict(ddim_eta=0, pag_scale=1.5, regions=True)),   # CFG + PAG + regional prompts
], ids=["unet-ddim0", "nested-ddim0-v2", "nested-dpmpp_2m", "unet-ddpm-known-v2", "unet-pag-regions"])
def test_graphed_sampler_equals_eager_sampler(name, structure, kw):
    """bit for bit, also on a second call through the cached graph; and FreeU acts"""
    import region_cases as RC

    s = _fresh(name)
    cfg = _cfg(structure)
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed)
        more = dict(kw)
        if more.pop("known", False):
            g = torch.Generator().manual_seed(seed)
            m = torch.zeros(2, 1, s.side, s.side, device=DEV)
            m[..., : s.side // 2] = 1
            more.update(known_images=(torch.randn(2, 3, s.side, s.side, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)
        if more.pop("regions", False):
            more.update(regions=RC.model_regions(name, DEV))
        want, out = s.eager(xs, freeu=cfg, **more), s.graphed(xs, freeu=cfg, **more)
        print("%s %s call %d: rel-L2 %.2e, max-abs %.2e" % (name, sorted(kw), rep, O.rel_l2(out, want), float((out - want).abs().max())))
        assert torch.isfinite(out).all() and torch.equal(out, want) and len(s.gs._graphs) == 1
    free = s.eager(xs, **more)
    moved = float((out - free).abs().max() / free.abs().max())
    print("FreeU moves the image by %.2e" % moved)
    assert moved > 1e-3


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_graph_key_holds_the_parameters_and_none_is_the_plain_call(name):
    s = _fresh(name)
    xs = s.start(43)
    plain = s.graphed(xs, ddim_eta=0)
    assert len(s.gs._graphs) == 1 and torch.equal(plain, s.eager(xs, ddim_eta=0))
    a = s.graphed(xs, ddim_eta=0, freeu=_cfg())
    assert len(s.gs._graphs) == 2 and not torch.equal(a, plain)
    b = s.graphed(xs, ddim_eta=0, freeu=_cfg(b=(1.2, 1.4), s=(0.2, 0.6)))      # other b / s: a new graph
    assert len(s.gs._graphs) == 3 and not torch.equal(a, b)
    assert torch.equal(b, s.eager(xs, ddim_eta=0, freeu=_cfg(b=(1.2, 1.4), s=(0.2, 0.6))))
    c = s.graphed(xs, ddim_eta=0, freeu=_cfg(structure=True))                  # v2: another one
    assert len(s.gs._graphs) == 4 and not torch.equal(a, c)
    assert torch.equal(s.graphed(xs, ddim_eta=0, freeu=_cfg()), a) and len(s.gs._graphs) == 4   # an equal config replays
    # freeu=None after all that: the first plain result, bit for bit, eager and graphed, and no graph more
    assert torch.equal(s.graphed(xs, ddim_eta=0, freeu=None), plain) and len(s.gs._graphs) == 4
    assert torch.equal(s.eager(xs, ddim_eta=0, freeu=None), plain)
