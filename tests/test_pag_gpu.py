"""GPU: perturbed-attention guidance on the HIP path -- mdm_attn_cross_addv against the fp64 restatement of
tests/pag_cases.py (per-kernel gates of DESIGN section 3), its exact identities, its cross term against the one
mdm_attn_fwd writes, the row-split op, the mini models against the oracle with perturbed layers, the eager sampler against
a loop restated here, eager against graphed, and mdm_pag_combine against fp64."""
import functools

import pytest
import torch

import pag_cases as PG
import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = {"fp32": 2e-5, "split": 2e-5, "bf16": 3e-2}   # max-abs over max-abs
MODES = list(GATE)
# (d, H, L, S), pruned: every d, H in {1, 3}, L in {16, 64, 80 (ragged query tile), 256}, S in {1, 5, 32, 77, 130 (past two
# key tiles)}; d = 96 and d = 128 each with S = 130
KERNEL_CASES = [(32, 1, 16, 1), (32, 3, 80, 5), (64, 3, 64, 32), (64, 1, 256, 77), (64, 3, 80, 130), (96, 3, 80, 130),
                (96, 1, 64, 5), (128, 1, 16, 130), (128, 3, 256, 32), (128, 3, 80, 77)]


def _dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def maxerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _run(qkv, kvc, mask, H, mode):
    from mdm_hip import ops

    dt = _dtype(mode)
    with torch.no_grad(), ops.fp32_split(mode == "split"):   # (constructing the switch sets it: only ever inside a with)
        return ops.attn_cross_addv(qkv.to(DEV, dt), None if kvc is None else kvc.to(DEV, dt),
                                   None if mask is None else mask.to(DEV), H)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,H,L,S", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_matches_the_fp64_restatement(d, H, L, S, mode):
    """B = 3 with one full, one holed + tail-masked and one fully masked row of the mask; and without a mask"""
    dt = _dtype(mode)
    qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, S, H, d))   # the values the kernel sees
    for mask in (PG.masks(S), None):
        out = _run(qkv, kvc, mask, H, mode)
        want = PG.cross_addv_ref(qkv, kvc, mask, H)
        err = maxerr(out, want)
        print("d=%d H=%d L=%d S=%d %s mask=%s: %.2e" % (d, H, L, S, mode, mask is not None, err))
        assert torch.isfinite(out).all() and err < GATE[mode]


@pytest.mark.parametrize("mode", MODES)
def test_exact_identities(mode):
    """no text keys -> v; every key masked -> v; one unmasked key and small-integer v, v_c -> v + v_c: bit for bit"""
    dt = _dtype(mode)
    for d, H, L in ((32, 3, 80), (96, 1, 64), (128, 3, 16), (64, 3, 256)):
        C = H * d
        qkv, kvc = (t.to(dt).float() for t in PG.attn_inputs(L, 5, H, d, seed=7))
        v = qkv[..., 2 * C:].to(dt)
        assert torch.equal(_run(qkv, None, None, H, mode).cpu(), v)
        assert torch.equal(_run(qkv, kvc, torch.zeros(3, 5), H, mode).cpu(), v)
        out = _run(qkv, kvc, PG.masks(5), H, mode).cpu()
        assert torch.equal(out[2], v[2]) and not torch.equal(out[0], v[0])
        g = torch.Generator().manual_seed(d + L)
        qi = qkv.clone()
        qi[..., 2 * C:] = torch.randint(-8, 9, (3, L, C), generator=g).float()       # distinct per row, head and channel
        k1 = torch.cat([kvc[:, :1, :C], torch.randint(-8, 9, (3, 1, C), generator=g).float()], dim=-1)
        out = _run(qi, k1, None, H, mode).cpu().float()
        assert torch.equal(out, qi[..., 2 * C:] + k1[..., C:])


@pytest.mark.parametrize("d,H,L,S", [(32, 3, 80, 5), (96, 3, 80, 130), (128, 1, 256, 77)])
def test_cross_term_is_the_one_mdm_attn_fwd_writes(d, H, L, S):
    """fp32: out - v against out_cross of the shipped kernel for the same inputs (the mask convention is the shipped one)"""
    from mdm_hip import _lib, ops

    qkv, kvc = (t.to(DEV) for t in PG.attn_inputs(L, S, H, d))
    mask = PG.masks(S).to(DEV)
    C = H * d
    out = torch.empty(3, L, C, device=DEV)
    oc = torch.empty_like(out)
    _lib.check(_lib.lib().mdm_attn_fwd(qkv.data_ptr(), kvc.data_ptr(), mask.data_ptr(), out.data_ptr(), oc.data_ptr(), None, None,
                                       3, L, S, H, d, ops.F32, ops._stream()), "mdm_attn_fwd")
    with torch.no_grad():
        got = ops.attn_cross_addv(qkv, kvc, mask, H) - qkv[..., 2 * C:]
    err = maxerr(got, oc)
    print("d=%d L=%d S=%d: %.2e" % (d, L, S, err))
    assert err < GATE["fp32"] and float(oc[2].abs().max()) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_attention_pag_splits_the_batch_by_rows(mode):
    from mdm_hip import _lib, ops

    dt = _dtype(mode)
    N, L, S, H, d = 5, 80, 77, 3, 64
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(N, L, 3 * H * d, generator=g).to(DEV, dt)
    kvc = torch.randn(N, S, 2 * H * d, generator=g).to(DEV, dt)
    mask = (torch.rand(N, S, generator=g) < 0.7).float().to(DEV)
    with torch.no_grad(), ops.fp32_split(mode == "split"):
        for kv, m in ((kvc, mask), (kvc, None), (None, None)):
            sl = lambda t, a, b: None if t is None else t[a:b].contiguous()
            out = ops.attention_pag(qkv, kv, m, H, 2)
            assert torch.equal(out[:3], ops.attention(qkv[:3].contiguous(), sl(kv, 0, 3), sl(m, 0, 3), H))
            assert torch.equal(out[3:], ops.attn_cross_addv(qkv[3:].contiguous(), sl(kv, 3, 5), sl(m, 3, 5), H))
            assert torch.equal(ops.attention_pag(qkv, kv, m, H, N), ops.attn_cross_addv(qkv, kv, m, H))
        with pytest.raises(_lib.MdmHipError, match="rows"):
            ops.attention_pag(qkv, kvc, mask, H, 6)
    leaf = qkv.clone().requires_grad_(True)
    with torch.enable_grad(), pytest.raises(_lib.MdmHipError, match="inference only"):
        ops.attention_pag(leaf, kvc, mask, H, 2)
    with torch.no_grad():   # ... and no complaint where no tape is recorded
        ops.attention_pag(leaf, kvc, mask, H, 2)


# ---- the combine kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1000, 4099])
def test_pag_combine_matches_fp64(n):
    """gate: 1e-6 of |p_u| + |w| |p_c - p_u| + |s| |p_c - p_hat| -- the fp32 epsilon (6e-8) over at most six roundings"""
    from mdm_hip import ops

    g = torch.Generator().manual_seed(n)
    pu, pc, pp = (torch.randn(n, generator=g) for _ in range(3))
    for w, s in ((2.0, 1.5), (7.5, 0.25)):
        for u in (pu, None):
            want, scale = PG.combine_ref(pc, u, pp, w, s), PG.combine_scale(pc, u, pp, w, s)
            dev = [None if t is None else t.to(DEV) for t in (pc, u, pp)]
            out = ops.pag_combine(dev[0], dev[1], dev[2], w, s)
            err = float(((out.double().cpu() - want).abs() / scale).max())
            print("n=%d w=%g s=%g uncond=%s: %.2e" % (n, w, s, u is not None, err))
            assert err < 1e-6 and torch.equal(dev[0].cpu(), pc)
            buf = dev[0].clone()
            assert ops.pag_combine(buf, dev[1], dev[2], w, s, out=buf).data_ptr() == buf.data_ptr()
            assert torch.equal(buf, out)


# ---- the models against the oracle with perturbed layers -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_model(name):
    return PC.build_module(name)[0].to(DEV).eval()


def _forward(name, mode, layers=None):
    """batch 4 (PG.model_inputs); ``layers``: perturb them on the last 2 rows"""
    import contextlib

    from mdm_hip import ops, pag

    model = _gpu_model(name)
    inp = PG.model_inputs(name)
    x = [t.to(DEV) for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].to(DEV)
    auto = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), auto, ops.fp32_split(mode == "split"):
        with (pag.perturbed(model, layers, rows=2) if layers else contextlib.nullcontext()):
            outs = model(x, inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV), {})
    return [o.float().cpu() for o in PC.as_list(outs)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layers", ["mid", "all"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_unet_masked", "mini_nested"])
def test_models_match_the_oracle_with_perturbed_layers(name, layers, mode):
    """fp32 / split: rel-L2 1e-4, the mini-model gate.  bf16: the perturbed rows' error is at most 2x the unperturbed rows'
    error of the same forward (the same layers, one op swapped for a cheaper one).  And the flag reaches the kernel: the
    perturbed rows differ from an unperturbed forward of the same inputs by more than 10x the fp32 gate."""
    from mdm_hip import pag

    names = pag.layer_names(_gpu_model(name), layers)
    outs = _forward(name, mode, layers)
    plain = _forward(name, mode)
    ref = PG.oracle_outputs(name, names)
    ref_plain = PG.oracle_outputs(name, ())
    for i, (o, p, r, rp) in enumerate(zip(outs, plain, ref, ref_plain)):
        e_unp, e_pert = O.rel_l2(o[:2], r[:2]), O.rel_l2(o[2:], r[2:])
        moved, moved_ref = O.rel_l2(o[2:], p[2:]), O.rel_l2(r[2:], rp[2:])
        print("%s %s %s out %d: unperturbed rows %.3e, perturbed rows %.3e (ratio %.2f); perturbation moves the rows by %.3e "
              "(oracle: %.3e)" % (name, layers, mode, i, e_unp, e_pert, e_pert / max(e_unp, 1e-30), moved, moved_ref))
        if mode == "bf16":
            assert e_pert <= 2 * e_unp
        else:
            assert e_unp < 1e-4 and e_pert < 1e-4
        assert moved > 10 * 1e-4


def test_graphed_denoiser_keys_on_the_perturbed_rows():
    """the forward-only graph wrapper: the same shapes with and without perturbed rows are two graphs, each bit-equal to
    its eager forward"""
    from mdm_hip import pag
    from mdm_hip.graph import GraphedDenoiser

    model = _gpu_model("mini_unet")
    gd = GraphedDenoiser(model)
    inp = PG.model_inputs("mini_unet")
    args = (inp["x"].to(DEV), inp["times"].to(DEV), inp["cond"].to(DEV), inp["mask"].to(DEV))
    with torch.no_grad():
        plain = gd(*args)
        assert torch.equal(plain, model(*args))
        with pag.perturbed(model, "mid", rows=2):
            pert = gd(*args)
            assert torch.equal(pert, model(*args))
        assert len(gd._graphs) == 2 and not torch.equal(pert[2:], plain[2:])
        assert torch.equal(gd(*args), plain) and len(gd._graphs) == 2


# ---- the samplers --------------------------------------------------------------------------------------------------------
RNG_SEED = 21
W, SCALE = 2.0, 1.5


def _pipeline(name, net):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                              use_double_loss=True, no_use_residual=True))
    return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


class Setup:
    """one mini pipeline on the GPU, its text inputs ([uncond | cond] when w != 1), eager and graphed runs from given noise"""

    def __init__(self, name, w):
        from mdm_hip.graph import GraphedSampler

        self.name, self.nested, self.w = name, name == "mini_nested", w
        self.pipe = _pipeline(name, PC.build_module(name)[0]).to(torch.device(DEV))
        self.pipe.eval()
        inp = PC.inputs(name)
        cond, mask = inp["cond"].to(DEV), inp["mask"].to(DEV)
        if w != 1:
            cond, mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
        self.cond, self.mask = cond, mask
        self.sample = {"lm_outputs": cond, "lm_mask": mask}
        self.side = 32 if self.nested else 16
        self.gs = GraphedSampler(self.pipe, seed=RNG_SEED)

    def start(self, seed):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, self.side, self.side, generator=g).to(DEV)]
        if self.nested:
            xs.append(torch.randn(2, 3, self.side // 2, self.side // 2, generator=g).to(DEV))
        return xs

    def eager(self, xs, n=4, **kw):
        xs = [t.clone() for t in xs]
        self.pipe.sampler.use_device_rng(RNG_SEED, DEV)
        with torch.no_grad():
            return self.pipe.sampler.sample(self.pipe.get_model(), xs if self.nested else xs[0], self.cond, self.mask, {},
                                            resample_steps=True, num_inference_steps=n, guidance_scale=self.w, **kw)

    def graphed(self, xs, n=4, **kw):
        with torch.no_grad():
            return self.gs.sample(2, self.sample, self.side, torch.device(DEV), num_inference_steps=n, start_noise=xs,
                                  seed=RNG_SEED, guidance_scale=self.w, **kw)


@functools.lru_cache(maxsize=None)
def _setup(name, w=W):
    return Setup(name, w)


def _restated(s, xs, n, solver, scale, layers="mid"):
    """The loop of ``Sampler._sample`` written out: the HIP model on [uncond | cond | perturbed] under ``pag.perturbed``,
    the torch combine, and the sampler's torch step formulas (a custom clip_fn keeps GPU tensors off the step kernels)."""
    from mdm_hip import pag
    from mdm_hip import samplers as SM

    smp, model = s.pipe.sampler, s.pipe.get_model()
    clip = lambda x0, sc: smp.clip_sample(x0, sc)
    steps = smp.set_timesteps(n)
    xs = [x.clone() for x in xs]
    B = xs[0].shape[0]
    reps = 3 if s.w != 1 else 2
    cond, mask = torch.cat([s.cond, s.cond[-B:]]), torch.cat([s.mask, s.mask[-B:]])
    image_scales = smp._scale_info(model)[1]
    x0_prev = g_prev = None
    with torch.no_grad():
        for i in range(n):
            t = torch.full((reps * B,), int(steps[i]) - 1, dtype=torch.long, device=DEV)
            xin = [torch.cat([x] * reps) for x in xs]
            with pag.perturbed(model.vision_model, layers, rows=B):
                preds = model(xin if s.nested else xin[0], t, cond, mask, {})
            preds = list(preds) if s.nested else [preds[0]]
            g_t, g_s = smp._scale_gammas(model, int(steps[i]), B), smp._scale_gammas(model, int(steps[i + 1]), B)
            second = solver is not None and 0 < i < n - 1
            x0s = []
            for k, p in enumerate(preds):
                parts = p.float().chunk(reps)
                comb = SM.pag_combine(parts[-2], parts[0] if reps == 3 else None, parts[-1], s.w, scale)
                if solver is None:
                    x0, xs[k], _ = smp.get_prediction_xt_last(xs[k], comb, g_t[k], g_s[k], clip_fn=clip, ddim_eta=0,
                                                             image_scale=image_scales[k], return_eps=False)
                else:
                    x0, xs[k] = smp.get_prediction_xt_last_2m(xs[k], comb, g_t[k], g_s[k], g_prev=g_prev[k] if second else None,
                                                             x0_prev=x0_prev[k] if second else None, second_order=second,
                                                             clip_fn=clip, image_scale=image_scales[k])
                x0s.append(x0)
            x0_prev, g_prev = x0s, g_t
        return smp._postprocess(xs if s.nested else xs[0], clip=True)


@pytest.mark.parametrize("solver,n", [(None, 4), ("dpmpp_2m", 3)], ids=["ddim0", "dpmpp_2m"])
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_eager_sampler_matches_the_restated_loop(name, solver, n):
    """fp32, rel-L2 1e-5 -- the measure every sampler comparison of this suite uses (eager against graphed below, the
    reference pipeline in test_model_gpu).  The largest single deviation over the largest value is printed beside it: the
    two sides differ by fp32 rounding in the combine and in the step (kernel against torch ops), which w + s = 3.5 of
    guidance then amplifies through every later denoiser call; measured 2.1e-5 on mini_unet DDIM(0)."""
    s = _setup(name)
    xs = s.start(41)
    kw = dict(solver=solver) if solver else dict(ddim_eta=0)
    out = s.eager(xs, n=n, pag_scale=SCALE, **kw)
    want = _restated(s, xs, n, solver, SCALE)
    err, worst = O.rel_l2(out, want), maxerr(out, want)
    free = s.eager(xs, n=n, **kw)
    print("%s %s: rel-L2 %.2e (max-abs over max-abs %.2e) against the restated loop; guidance moves the image by %.2e"
          % (name, solver, err, worst, maxerr(out, free)))
    assert torch.isfinite(out).all() and err < 1e-5
    assert maxerr(out, free) > 1e-3


@pytest.mark.parametrize("name,w,kw", [
    ("mini_unet", W, dict(ddim_eta=0)),
    ("mini_nested", W, dict(solver="dpmpp_2m")),
    ("mini_unet", W, dict(known=True)),                   # ancestral DDPM with a known half
    ("mini_nested", 1, dict(ddim_eta=0, pag_layers="all")),
], ids=["unet-ddim0", "nested-dpmpp_2m", "unet-ddpm-known", "nested-w1-all"])
def test_graphed_sampler_matches_eager_sampler(name, w, kw):
    """as tests/test_inpaint_gpu.py compares them: rel-L2 1e-6, also on a second call through the cached graph"""
    from mdm_hip.graph import GraphedSampler

    s = _setup(name, w)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    kw = dict(kw)
    for rep, seed in enumerate((41, 42)):
        xs = s.start(seed)
        more = dict(kw)
        if more.pop("known", False):
            g = torch.Generator().manual_seed(seed)
            m = torch.zeros(2, 1, s.side, s.side, device=DEV)
            m[..., : s.side // 2] = 1
            more.update(known_images=(torch.randn(2, 3, s.side, s.side, generator=g) * 0.8).to(DEV), known_mask=m, known_seed=seed)
        want, out = s.eager(xs, pag_scale=SCALE, **more), s.graphed(xs, pag_scale=SCALE, **more)
        err = O.rel_l2(out, want)
        print("%s w=%s %s call %d: rel-L2 %.2e" % (name, w, sorted(kw), rep, err))
        assert err < 1e-6 and len(s.gs._graphs) == 1
    assert not torch.equal(out, s.graphed(xs, **{k: v for k, v in more.items() if k != "pag_layers"}))


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_pag_scale_zero_is_the_call_without_the_arguments(name):
    from mdm_hip.graph import GraphedSampler

    s = _setup(name)
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    xs = s.start(43)
    for run in (s.eager, s.graphed):
        for kw in (dict(ddim_eta=0), dict(solver="dpmpp_2m"), {}):
            assert torch.equal(run(xs, pag_scale=0.0, pag_layers="all", **kw), run(xs, **kw)), (run.__name__, kw)
    assert len(s.gs._graphs) == 3   # pag_scale = 0 adds no graph


def test_graph_key_holds_scale_and_layers():
    from mdm_hip.graph import GraphedSampler

    s = _setup("mini_unet")
    s.gs = GraphedSampler(s.pipe, seed=RNG_SEED)
    xs = s.start(44)
    a = s.graphed(xs, ddim_eta=0, pag_scale=1.5)
    assert len(s.gs._graphs) == 1
    b = s.graphed(xs, ddim_eta=0, pag_scale=3.0)
    assert len(s.gs._graphs) == 2 and not torch.equal(a, b)
    c = s.graphed(xs, ddim_eta=0, pag_scale=1.5, pag_layers="all")
    assert len(s.gs._graphs) == 3 and not torch.equal(a, c)
    # the same selection under another spelling is the same graph; so is a repeated call
    d = s.graphed(xs, ddim_eta=0, pag_scale=1.5, pag_layers=["mid_blocks.0.attn.0"])
    assert len(s.gs._graphs) == 3 and torch.equal(a, d)
    assert torch.equal(s.graphed(xs, ddim_eta=0, pag_scale=3.0), b) and len(s.gs._graphs) == 3
    assert O.rel_l2(b, s.eager(xs, ddim_eta=0, pag_scale=3.0)) < 1e-6
    s.graphed(xs, ddim_eta=0)
    assert len(s.gs._graphs) == 4
    with pytest.raises(ValueError, match="pag_scale"):
        s.graphed(xs, pag_scale=-1.0)
