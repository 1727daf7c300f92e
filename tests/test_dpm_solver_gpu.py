"""GPU: DPM-Solver++(2M) on the HIP path -- the mdm_sampler_step_2m kernel against the torch-op path of the same
method on CPU tensors (itself held to the fp64 restatement by tests/test_dpm_solver_host.py), the eager sampler against
GraphedSampler on the mini models, and the 2-step identity with DDIM(eta = 0) on a real denoiser."""
import pytest
import torch

import parity_cases as PC
import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _sampler(pred="V_PREDICTION", thr="CLIP", **kw):
    from mdm_hip import samplers as S

    return S.Sampler(S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type=pred,
                                     loss_target_type="DDPM", threshold_function=thr, **kw))


def _case(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    x_t = torch.randn(*shape, generator=g) * 1.3
    pc, pu = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    x0_prev = torch.rand(*shape, generator=g) * 2 - 1
    return x_t, pc, pu, x0_prev


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
@pytest.mark.parametrize("thr", ["NONE", "CLIP", "DYNAMIC", "DYNAMIC_IF"])
@pytest.mark.parametrize("cfg,scale", [(1.0, None), (3.0, 2.0)])
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("shape", [(3, 3, 20, 20), (3, 4, 5, 7)])
def test_kernel_matches_the_torch_formulas(pred, thr, cfg, scale, second, shape):
    """Sampler.get_prediction_xt_last_2m on GPU tensors (one mdm_sampler_step_2m launch; the dynamic thresholds add
    the x0 launch and the quantile) == the same call on CPU tensors.  Times at both ends and in the middle of the
    schedule, one per sample; fp32 on both sides, gate as test_sampler_step_matches_reference_formulas."""
    smp = _sampler(pred, thr)
    x_t, pc, pu, x0_prev = _case(shape)
    t = torch.tensor([700, 31, 999])
    gam, gl, gp = smp.read_gamma(t), smp.read_gamma(t - torch.tensor([40, 30, 99])), smp.read_gamma(t + torch.tensor([50, 20, 1]))
    kw = dict(second_order=second, prediction_type=smp._config.prediction_type, image_scale=scale, guidance_scale=cfg)
    ref = smp.get_prediction_xt_last_2m(x_t, pc, gam, gl, g_prev=gp, x0_prev=x0_prev, clip_fn=smp.clip_sample,
                                        pred_uncond=pu if cfg != 1 else None, **kw)
    smp_d = _sampler(pred, thr).to(DEV)
    out = smp_d.get_prediction_xt_last_2m(x_t.to(DEV), pc.to(DEV), gam.to(DEV), gl.to(DEV), g_prev=gp.to(DEV),
                                          x0_prev=x0_prev.to(DEV), clip_fn=smp_d.clip_sample,
                                          pred_uncond=pu.to(DEV) if cfg != 1 else None, **kw)
    errs = [relerr(a, b) for a, b in zip(out, ref)]
    print("x0 %.2e x_s %.2e" % tuple(errs))
    assert max(errs) < 1e-4


@pytest.mark.parametrize("gate", [0.0, 1.0])
def test_history_may_be_updated_in_place(gate):
    """x0_out aliased to x0_prev (what GraphedSampler does with its static history buffer) == separate buffers, bit for
    bit, with the order gate given as a device float[1]"""
    from mdm_hip import ops

    smp = _sampler().to(DEV)
    x_t, pc, pu, x0_prev = [v.to(DEV) for v in _case((3, 3, 36, 36), seed=9)]
    t = torch.tensor([700, 31, 999], device=DEV)
    gam, gl, gp = smp.read_gamma(t), smp.read_gamma(t - 25), smp.read_gamma(t + 1)
    order = torch.tensor([gate], device=DEV)
    PT = smp._config.prediction_type
    kw = dict(g_prev=gp, second_order=order, pred_uncond=pu, guidance_scale=2.0)
    x0_a, xl_a = ops.sampler_step_2m(x_t, pc, gam, gl, PT, x0_prev=x0_prev, **kw)
    hist = x0_prev.clone()
    x0_b, xl_b = ops.sampler_step_2m(x_t, pc, gam, gl, PT, x0_prev=hist, x0_out=hist, **kw)
    assert x0_b is hist and torch.equal(x0_a, hist) and torch.equal(xl_a, xl_b)
    # the gate is honoured: second order moves x_last, first order equals the call without history
    _, xl_1 = ops.sampler_step_2m(x_t, pc, gam, gl, PT, pred_uncond=pu, guidance_scale=2.0)
    assert torch.equal(xl_a, xl_1) == (gate == 0.0)


@pytest.mark.parametrize("pred", ["V_PREDICTION", "DDPM"])
def test_last_step_selects_first_order(pred):
    """gamma_last == 1 with the gate off and a history full of NaN: x_s == x0, finite -- the flag selects, it does not
    multiply (0 * inf), and the history is not read"""
    from mdm_hip import ops

    smp = _sampler(pred).to(DEV)
    x_t, pc, _, x0_prev = [v.to(DEV) for v in _case((3, 3, 20, 20))]
    x0_prev.fill_(float("nan"))
    t = torch.tensor([1, 40, 999], device=DEV)
    gam, gl, gp = smp.read_gamma(t), torch.ones(3, device=DEV), smp.read_gamma(t + 1)
    for order in (False, torch.zeros(1, device=DEV)):
        x0, x_s = ops.sampler_step_2m(x_t, pc, gam, gl, smp._config.prediction_type, g_prev=gp, x0_prev=x0_prev,
                                      second_order=order)
        assert torch.isfinite(x_s).all() and torch.equal(x_s, x0)
    ref = smp.get_prediction_xt_last_2m(x_t.cpu(), pc.cpu(), gam.cpu(), gl.cpu().reshape(-1, 1, 1, 1), clip_fn=smp.clip_sample)
    assert relerr(x_s, ref[1]) < 1e-4


def test_ops_argument_checks():
    from mdm_hip import _lib, ops

    smp = _sampler().to(DEV)
    x_t, pc, _, x0_prev = [v.to(DEV) for v in _case((3, 3, 20, 20))]
    gam = smp.read_gamma(torch.tensor([5, 6, 7], device=DEV))
    PT = smp._config.prediction_type
    with pytest.raises(_lib.MdmHipError):   # second order without history
        ops.sampler_step_2m(x_t, pc, gam, gam, PT, second_order=True)
    with pytest.raises(_lib.MdmHipError):   # the history lives on the device
        ops.sampler_step_2m(x_t, pc, gam, gam, PT, g_prev=gam, x0_prev=x0_prev.cpu(), second_order=True)
    with pytest.raises(_lib.MdmHipError):   # chw % 4
        ops.sampler_step_2m(x_t[:, :, :3, :3].contiguous(), pc[:, :, :3, :3].contiguous(), gam, gam, PT)


def _pipeline(name, net, threshold="CLIP"):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function=threshold, schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(net, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                              use_double_loss=True, no_use_residual=True))
    return D.Diffusion(net, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


def _setup(name, mode):
    model, _, _ = PC.build_module(name)
    pipe = _pipeline(name, model, threshold="DYNAMIC_IF" if mode == "dynamic" else "CLIP").to(torch.device(DEV))
    pipe.eval()
    inp = PC.inputs(name)
    cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
    kw = dict(guidance_scale=2.5 if mode == "cfg" else 1)
    if mode == "cfg":
        cond, mask = torch.cat([torch.zeros_like(cond), cond]), torch.cat([mask, mask])
    side = 32 if name == "mini_nested" else 16

    def start(seed):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, 3, side, side, generator=g).cuda()]
        if name == "mini_nested":
            xs.append(torch.randn(2, 3, side // 2, side // 2, generator=g).cuda())
        return xs

    def eager(xs, n, **more):
        xs = [t.clone() for t in xs]
        return pipe.sampler.sample(pipe.get_model(), xs if name == "mini_nested" else xs[0], cond, mask, {},
                                   resample_steps=True, num_inference_steps=n, **dict(kw, **more))

    return pipe, {"lm_outputs": cond, "lm_mask": mask}, side, kw, start, eager


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
@pytest.mark.parametrize("mode", ["plain", "cfg", "dynamic"])
def test_graphed_sampler_matches_eager_sampler(name, mode):
    """6 steps of dpmpp_2m: GraphedSampler (order gate and previous time from device tables, x0 history in a static
    buffer updated in place) == the eager sampler on the same start noise.  The second call replays the cached graph on
    OTHER start noise: it must not see the first call's history.  A 1- and a 2-step schedule survive the warm-up."""
    from mdm_hip.graph import GraphedSampler

    pipe, smp, side, kw, start, eager = _setup(name, mode)
    dev = torch.device(DEV)
    with torch.no_grad():
        gs = GraphedSampler(pipe)
        for rep, seed in enumerate((41, 42)):
            xs = start(seed)
            want = eager(xs, 6, solver="dpmpp_2m")
            out = gs.sample(2, smp, side, dev, num_inference_steps=6, start_noise=xs, solver="dpmpp_2m", **kw)
            err = O.rel_l2(out, want)
            print("call %d: rel-L2 %.2e" % (rep, err))
            assert err < 1e-6, rep
        assert len(gs._graphs) == 1
        ddim = gs.sample(2, smp, side, dev, num_inference_steps=6, start_noise=xs, ddim_eta=0, **kw)
        print("6 steps, 2M vs DDIM(0): rel-L2 %.2e" % O.rel_l2(ddim, want))
        assert len(gs._graphs) == 2   # the solver is part of the graph key
        for n in (1, 2):
            out = gs.sample(2, smp, side, dev, num_inference_steps=n, start_noise=xs, solver="dpmpp_2m", **kw)
            assert O.rel_l2(out, eager(xs, n, solver="dpmpp_2m")) < 1e-6, n
        assert len(gs._graphs) == 4
        with pytest.raises(ValueError):
            gs.sample(2, smp, side, dev, num_inference_steps=6, start_noise=xs, solver="dpmpp_2m", ddim_eta=0.0, **kw)


def test_two_steps_equal_ddim_on_a_real_denoiser():
    """mini_unet, 2 steps (first, last: no second-order step): solver == DDIM(eta = 0), eager and graphed, and
    Diffusion.sample forwards ``solver=``"""
    from mdm_hip.graph import GraphedSampler

    pipe, smp, side, kw, start, eager = _setup("mini_unet", "plain")
    dev = torch.device(DEV)
    xs = start(41)
    with torch.no_grad():
        a, b = eager(xs, 2, solver="dpmpp_2m"), eager(xs, 2, ddim_eta=0)
        assert relerr(a, b) < 1e-4
        gs = GraphedSampler(pipe)
        assert relerr(gs.sample(2, smp, side, dev, num_inference_steps=2, start_noise=xs, solver="dpmpp_2m"), b) < 1e-4
        torch.manual_seed(5)
        c = pipe.sample(2, smp, side, dev, resample_steps=True, num_inference_steps=6, solver="dpmpp_2m")
        torch.manual_seed(5)
        d = pipe.sample(2, smp, side, dev, resample_steps=True, num_inference_steps=6, ddim_eta=0)
        print("6 steps, 2M vs DDIM(0): %.2e" % relerr(c, d))
        assert torch.isfinite(c).all() and c.shape == d.shape
