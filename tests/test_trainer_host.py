"""CPU: ``mdm_hip.trainer.train_batch`` keeps the call surface and the semantics of the reference's
``ml_mdm.trainer.train_batch`` (trainer.py:13-96): signature, gradient accumulation, NaN handling, scheduler / logger
calls, return value -- checked against tests/golden/train_batch.pt, which oracle/make_golden.py produced by running
the REAL reference trainer (+ its ModelEma and Diffusion) around the same stub denoiser, and against the reference
executed live when the reference tree is present.  (On CPU tensors the step takes its plain path; the fused path is
compared with the plain one on the GPU: tests/test_trainer_gpu.py.)"""
import inspect
import math
import os

import pytest
import torch

import make_golden as MG
import stub_models as SM

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "train_batch.pt"), weights_only=False)


def _pipe():
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION", loss_target_type="DDPM")
    return D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-6 * max(1.0, abs(b))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("tag,nan_at", [("plain", None), ("nan", 2)])
def test_train_batch_matches_reference_trainer_golden(tag, nan_at):
    from mdm_hip import trainer

    res = MG.run_train_batch(trainer, _pipe(), trainer.ModelEma, nan_at=nan_at)
    for k, v in GOLD[tag].items():
        assert _same(res[k], v), (k, res[k], v)


def test_signature_is_the_reference_one():
    from mdm_hip import trainer

    names = list(inspect.signature(trainer.train_batch).parameters)
    assert names == ["model", "sample", "optimizer", "scheduler", "logger", "args", "grad_scaler", "accumulate_gradient",
                     "num_grad_accumulations", "ema_model", "loss_factor"]   # reference trainer.py:13-25


def test_train_batch_matches_live_reference_trainer():
    """9 micro-steps with 3-step accumulation against the reference trainer executed live; where the reference tree is
    absent, against what it produced for the same run (tests/golden/train_batch.pt["acc3"])"""
    import ref_import

    from mdm_hip import trainer

    if not ref_import.available():
        ours = MG.run_train_batch(trainer, _pipe(), trainer.ModelEma, n_micro=9, accumulations=3)
        for k, v in GOLD["acc3"].items():
            assert _same(ours[k], v), (k, ours[k], v)
        return
    R = ref_import.load()
    assert list(inspect.signature(trainer.train_batch).parameters) == list(inspect.signature(R.trainer.train_batch).parameters)
    S, D = R.samplers, R.diffusion
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type=S.ScheduleType.DEEPFLOYD,
                           prediction_type=S.PredictionType.V_PREDICTION, loss_target_type=S.PredictionType.DDPM)
    rpipe = D.Diffusion(SM.StubUNet(), D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False))
    ref = MG.run_train_batch(R.trainer, rpipe, R.model_ema.ModelEma, n_micro=9, accumulations=3)
    ours = MG.run_train_batch(trainer, _pipe(), trainer.ModelEma, n_micro=9, accumulations=3)
    # ... and the reference's own ModelEma class drives our step just as well
    mixed = MG.run_train_batch(trainer, _pipe(), R.model_ema.ModelEma, n_micro=9, accumulations=3)
    for k, v in ref.items():
        assert _same(ours[k], v), (k, ours[k], v)
        assert _same(mixed[k], v), (k, mixed[k], v)
