"""The sampling options at the three entry points that take them -- ``Sampler.sample``, ``Sampler.get_xt_minus_1`` and
``GraphedSampler.sample`` (which validates before it touches the device: a stub pipeline on the CPU serves): one table of
refusals, written out, for all three; unknown keywords; what is not an option still reaches ``_postprocess``; and the
options are checked once per public call, not once per step."""
import types

import pytest
import torch

import pag_cases as PG

B, S, D = 2, 5, 8

NO_BACKWARD = "has no backward, so the guide's input gradient cannot pass it"
GRAPHED_GUIDE = (NotImplementedError,
                 "GraphedSampler does not take guide=: loss-guided sampling calls an arbitrary user function and an autograd "
                 "pass through the denoiser every step, and neither can be captured in a hipGraph; use the eager "
                 "Sampler.sample(..., guide=...)")


def _sampler(nested=False):
    from mdm_hip import samplers as SM

    cfg = SM.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP")
    return (SM.NestedSampler if nested else SM.Sampler)(cfg)


def _inputs(nested=False):
    g = torch.Generator().manual_seed(0)
    lm = torch.randn(2 * B, S, D, generator=g)
    mask = (torch.rand(2 * B, S, generator=g) < 0.7).float()
    x = [torch.randn(B, 3, 8, 8, generator=g) for _ in range(2)] if nested else torch.randn(B, 3, 8, 8, generator=g)
    return x, lm, mask


def _cases():
    """name -> (options, (class, message) of the eager entry points, that of GraphedSampler.sample)"""
    import mdm_hip

    guide = mdm_hip.LossGuide(lambda z: z.pow(2).sum(dim=(1, 2, 3)))
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    fu = mdm_hip.FreeU(b=(1.4, 1.4), s=(0.2, 0.2))
    cfg = mdm_hip.CFG()
    pag_cfg = (NotImplementedError,
               "pag_scale != 0 together with cfg=: mdm_pag_combine adds the perturbed-attention term to the plain combine; "
               "projecting, capping and rescaling an update of three predictions is not implemented")
    neg = (ValueError, "pag_scale must be >= 0 (got -0.5); 0 = no perturbed-attention guidance")
    left = (ValueError, "regions = 'left' (wanted a mdm_hip.RegionPrompts)")
    pair = (ValueError, "freeu = (1.4, 0.2) (wanted a mdm_hip.FreeU)")
    eta = (ValueError, "cfg = {'eta': 0} (wanted a mdm_hip.CFG)")
    return {
        "guide x pag": (dict(guide=guide, pag_scale=1.0), (NotImplementedError,
                        "guide= together with pag_scale != 0: the perturbed rows' attention kernel (mdm_attn_cross_addv) "
                        + NO_BACKWARD), GRAPHED_GUIDE),
        "guide x regions": (dict(guide=guide, regions=rp), (NotImplementedError,
                            "guide= together with regions=: the biased cross-attention kernel (mdm_attn_cross_bias) "
                            + NO_BACKWARD), GRAPHED_GUIDE),
        "guide x freeu": (dict(guide=guide, freeu=fu), (NotImplementedError,
                          "guide= together with freeu=: the fused concat (mdm_freeu_apply) " + NO_BACKWARD), GRAPHED_GUIDE),
        "guide x cfg": (dict(guide=guide, cfg=cfg), (NotImplementedError,
                        "guide= together with cfg=: the guide seeds the two halves of the doubled batch with the weights of "
                        "the plain combine (w and 1 - w); the projected / rescaled combine depends on per-sample statistics "
                        "of both predictions, and its Jacobian is not implemented"), GRAPHED_GUIDE),
        "pag x cfg": (dict(pag_scale=1.0, cfg=cfg), pag_cfg, pag_cfg),
        "guide type": (dict(guide="x"), (TypeError, "guide must be an mdm_hip.LossGuide (got 'str')"), GRAPHED_GUIDE),
        "pag range": (dict(pag_scale=-0.5), neg, neg),
        "regions type": (dict(regions="left"), left, left),
        "freeu type": (dict(freeu=(1.4, 0.2)), pair, pair),
        "cfg type": (dict(cfg=dict(eta=0)), eta, eta),
        # several things wrong: guide, pag, regions, freeu, cfg -- the first of them speaks
        "guide type first": (dict(guide="x", pag_scale=-0.5), (TypeError, "guide must be an mdm_hip.LossGuide (got 'str')"),
                             GRAPHED_GUIDE),
        "pag before regions": (dict(pag_scale=-0.5, regions="left", cfg=cfg), neg, neg),
        "regions before freeu": (dict(regions="left", freeu=(1.4, 0.2)), left, left),
        "freeu before cfg": (dict(freeu=(1.4, 0.2), cfg=dict(eta=0)), pair, pair),
    }


NAMES = ["guide x pag", "guide x regions", "guide x freeu", "guide x cfg", "pag x cfg", "guide type", "pag range",
         "regions type", "freeu type", "cfg type", "guide type first", "pag before regions", "regions before freeu",
         "freeu before cfg"]


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_point_refuses_alike(name):
    from mdm_hip.graph import GraphedSampler

    options, eager, graphed = _cases()[name]
    smp, stub = _sampler(), PG.RecordingStub()
    x, lm, mask = _inputs()
    gs = GraphedSampler(types.SimpleNamespace(sampler=smp))   # refuses before it asks its pipeline for anything
    calls = {
        "sample": (eager, lambda: smp.sample(stub, x, lm, mask, {}, resample_steps=True, num_inference_steps=2, ddim_eta=0,
                                             guidance_scale=2.0, **options)),
        "get_xt_minus_1": (eager, lambda: smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, guidance_scale=2.0, **options)),
        "graphed": (graphed, lambda: gs.sample(B, {"lm_outputs": lm, "lm_mask": mask}, 8, torch.device("cpu"),
                                               guidance_scale=2.0, **options)),
    }
    for where, ((cls, message), call) in calls.items():
        with pytest.raises(cls) as err:
            call()
        assert type(err.value) is cls and str(err.value) == message, where
    assert not stub.calls


def test_the_table_is_the_whole_table():
    assert sorted(NAMES) == sorted(_cases())


def test_unknown_keywords_are_type_errors():
    from mdm_hip.graph import GraphedSampler

    smp, stub = _sampler(), PG.RecordingStub()
    x, lm, mask = _inputs()
    with pytest.raises(TypeError, match="pag_scales"):
        smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, pag_scales=1.0)
    with pytest.raises(TypeError, match="region"):
        GraphedSampler(types.SimpleNamespace(sampler=smp)).sample(B, {"lm_outputs": lm, "lm_mask": mask}, 8,
                                                                  torch.device("cpu"), region=None)
    assert not stub.calls


def test_other_keywords_still_reach_postprocess():
    kw = dict(resample_steps=True, num_inference_steps=2, ddim_eta=0, guidance_scale=2.0, pag_scale=1.5)
    smp, stub = _sampler(), PG.RecordingStub()
    x, lm, mask = _inputs()
    plain = smp.sample(stub, x, lm, mask, {}, **kw)
    x0, x_t, extra = smp.sample(stub, x, lm, mask, {}, yield_full=True, **kw)
    assert torch.equal(x_t, plain) and x0.shape == x_t.shape and extra is not None
    smp, stub = _sampler(True), PG.RecordingStub(True)
    x, lm, mask = _inputs(True)
    plain = smp.sample(stub, x, lm, mask, {}, **kw)
    inner = smp.sample(stub, x, lm, mask, {}, output_inner=True, **kw)
    assert plain.shape == (B, 3, 8, 8) and inner.shape == (B, 3, 8, 16) and torch.equal(inner[..., 8:], plain)


@pytest.mark.parametrize("nested", [False, True], ids=["unet", "nested"])
def test_options_are_checked_once_per_public_call(nested, monkeypatch):
    import mdm_hip
    from mdm_hip.samplers import SampleOptions

    counts = []
    inner = SampleOptions.check
    monkeypatch.setattr(SampleOptions, "check", lambda self: counts.append(self) or inner(self))
    smp, stub = _sampler(nested), PG.RecordingStub(nested)
    x, lm, mask = _inputs(nested)
    rp = mdm_hip.RegionPrompts(S, 8, [(0, 2, None, 1.4)], rows=B)
    kw = dict(guidance_scale=2.0, ddim_eta=0, pag_scale=1.5, regions=rp)
    smp.sample(stub, x, lm, mask, {}, resample_steps=True, num_inference_steps=4, **kw)
    assert len(stub.calls) == 4 and len(counts) == 1
    for _ in smp.sample(stub, x, lm, mask, {}, resample_steps=True, num_inference_steps=3, yield_output=True, **kw):
        pass
    assert len(stub.calls) == 7 and len(counts) == 2
    smp.get_xt_minus_1(stub, 700, x, lm, mask, {}, time_step_last=400, **kw)
    assert len(stub.calls) == 8 and len(counts) == 3
