"""GPU: the MXFP8 kernels (csrc/fp8.hip) against the restatement of tests/fp8_cases.py -- the quantiser bit for bit, the
GEMM exactly on integer data (every lane, K-order and scale mapping shows on every element) and within bf16 output rounding
on random data -- and the model with the fp8 handle attached against the fake-quant oracle, plus the identities that make
the path safe to use (detach restores, a changed weight re-quantises, no backward, no fp32, graphed sampling follows
attach).

Model gate (bf16): the fake-quant oracle's OWN error when it is run with bf16 tensors on the CPU against its fp32 run,
times 2 -- a rounding flip at fp8 granularity moves an element by a whole e4m3 step (2^-4 .. 2^-3 relative), so the factor is
looser than the 1.5 of the plain bf16 / LoRA gates.  Measured values are printed (pytest -s); DESIGN.md section 4.10 records the oracle side.
"""
import functools

import pytest
import torch

import fp8_cases as FC
import parity_cases as PC
import unet_oracle as O
from test_ops_gpu import TOL, relerr    # the project's per-op gates: bf16 3e-2 of the largest reference magnitude

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_CASES = ["mini_unet", "mini_unet_masked", "mini_nested"]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _mx8(q, s, K):
    from mdm_hip import ops

    return ops.Mx8(q.to(DEV), s.to(DEV), K)


# ---- 1. quantiser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,K", FC.QUANT_SHAPES)
def test_quantiser_is_bit_exact(dtype, M, K):
    from mdm_hip import ops

    g = _g(M * 7 + K)
    nb = K // 32
    # every block at a magnitude of its own in 2^-20 .. 2^20; block (0, 0) saturates (amax 250: e = -1, 500 lies in (448, 512));
    # the last block is all zero (the 1 x 32 case has one block only: its zero blocks are the three padding blocks)
    mag = torch.exp2(torch.randint(-20, 21, (M, nb, 1), generator=g).float())
    x = torch.randn(M, nb, 32, generator=g) * mag
    x[0, 0] = torch.randn(32, generator=g).clamp(-1, 1) * 100.0
    x[0, 0, 3] = 250.0
    if M * nb > 1:
        x[M - 1, nb - 1] = 0.0
    x = x.reshape(M, K).to(dtype)
    q_ref, s_ref = FC.quant_ref(x)
    out = ops.mx8_quant(x.to(DEV))
    assert out.q.shape == q_ref.shape and out.s.shape == s_ref.shape and out.K == K
    dq, ds = int((out.q.cpu() != q_ref).sum()), int((out.s.cpu() != s_ref).sum())
    print("[mx8_quant %s M=%d K=%d] differing codes %d / %d, scale bytes %d / %d" % (dtype, M, K, dq, q_ref.numel(), ds, s_ref.numel()))
    assert dq == 0 and ds == 0


def test_quantiser_on_zeros():
    from mdm_hip import ops

    for dtype in (torch.bfloat16, torch.float32):
        out = ops.mx8_quant(torch.zeros(3, 64, dtype=dtype, device=DEV))
        assert int(out.q.max()) == 0 and bool((out.s == 127).all()) and out.q.shape == (3, 128) and out.s.shape == (3, 4)


# ---- 2. GEMM, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", FC.GEMM_SHAPES)
def test_gemm_exact_on_integer_data(M, N, K):
    from mdm_hip import ops

    qa, sa, qw, sw = FC.exact_case(M, N, K)
    ref = FC.gemm_ref(qa, sa, qw, sw)
    assert torch.equal(ref.float().double(), ref)                       # exact in fp32 ...
    y = ops.mx8_gemm(_mx8(qa, sa, K), _mx8(qw, sw, K))
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    want = ref.float().to(torch.bfloat16)                               # ... so the bf16 output is the rounding of the exact value
    bad = int((y.cpu().float() != want.float()).sum())
    print("[mx8_gemm exact M=%d N=%d K=%d] wrong elements %d / %d (%d of the expected values need no rounding)" % (
        M, N, K, bad, M * N, int((want.double() == ref).sum())))
    assert torch.equal(y.cpu(), want)


# ---- 3. GEMM, random ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(M, N, K):
    g = _g(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5)
    qa, sa = FC.quant_ref(a)
    qw, sw = FC.quant_ref(w)
    bias = torch.randn(N, generator=g) * 0.5
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    return qa, sa, qw, sw, bias, res, FC.gemm_ref(qa, sa, qw, sw) + bias.double()


@pytest.mark.parametrize("epilogue", ["bias", "residual", "gelu", "gelu_emit"])
@pytest.mark.parametrize("M,N,K", FC.GEMM_SHAPES)
def test_gemm_random(M, N, K, epilogue):
    from mdm_hip import ops

    qa, sa, qw, sw, bias, res, pre = _random_case(M, N, K)
    a, w = _mx8(qa, sa, K), _mx8(qw, sw, K)
    gelu = epilogue.startswith("gelu")
    r = res.to(DEV) if epilogue == "residual" else None
    y = ops.mx8_gemm(a, w, bias.to(DEV), residual=r, gelu=gelu)
    again = ops.mx8_gemm(a, w, bias.to(DEV), residual=r, gelu=gelu)
    assert torch.equal(y, again)                                        # deterministic
    yd = y.cpu().double()
    if gelu:
        ref = FC.gelu_ref(pre)
        err = relerr(yd, ref)
        print("[mx8_gemm %s M=%d N=%d K=%d] max-abs / max-ref %.3e" % (epilogue, M, N, K, err))
        assert err < TOL[torch.bfloat16]                                # the epilogue's GELU is the approximate one: the bf16 op gate
        # elementwise too (the op gate alone would not notice a wrong order of GELU and rounding on small elements): the
        # epilogue applies the polynomial GELU to the bf16-rounded pre-activation, so the error is at most |gelu'| <= 1.13
        # times the input rounding, the polynomial's own gate of test_gelu_poly_against_erf_gelu (1.5e-4 absolute) and the
        # output rounding; 2^-8 (one bf16 ulp, twice the rounding error) for both roundings
        bound = 1.13 * 2.0 ** -8 * pre.abs() + 1.5e-4 + 2.0 ** -8 * ref.abs()
        print("[mx8_gemm %s M=%d N=%d K=%d] worst |y - gelu(pre)| / bound %.3f" % (epilogue, M, N, K, float(((yd - ref).abs() / bound).max())))
        assert bool(((yd - ref).abs() <= bound).all())
    else:
        ref = pre + (res.double() if r is not None else 0.0)
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * float(pre.abs().max())
        worst = float(((yd - ref).abs() / bound).max())
        print("[mx8_gemm %s M=%d N=%d K=%d] worst |y - ref| / bound %.3f" % (epilogue, M, N, K, worst))
        assert bool(((yd - ref).abs() <= bound).all())
    if epilogue == "gelu_emit":
        em = ops.mx8_gemm(a, w, bias.to(DEV), gelu=True, emit=True)
        want = ops.mx8_quant(y)
        assert em.K == N and em.q.shape == want.q.shape == (M, FC.round_up(N, 128)) and em.s.shape == want.s.shape
        assert torch.equal(em.q, want.q) and torch.equal(em.s, want.s)  # the fused form IS mx8_quant(bf16 output)
        q_ref, s_ref = FC.quant_ref(y.cpu())
        assert torch.equal(em.q.cpu(), q_ref) and torch.equal(em.s.cpu(), s_ref)
        em2 = ops.mx8_gemm(a, w, bias.to(DEV), gelu=True, emit=True)
        assert torch.equal(em.q, em2.q) and torch.equal(em.s, em2.s)


# ---- 4. model -------------------------------------------------------------------------------------------------------------------
def _model(name):
    return PC.build_module(name)[0].to(DEV)


def _outs(model, name, dtype=torch.bfloat16):
    inp = PC.inputs(name)
    x = [t.cuda() for t in inp["x"]] if isinstance(inp["x"], list) else inp["x"].cuda()
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        out = model(x, inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), {})
    return [o.detach().float().cpu() for o in PC.as_list(out)]


_oracle_cache = {}


def _oracle(name, kind, monkeypatch):
    """computed once per case and shared (never modified): 'plain' fp32, 'fq' fake-quant fp32, 'fq_bf16' fake-quant in bf16"""
    key = (name, kind)
    if key not in _oracle_cache:
        if kind == "plain":
            _oracle_cache[key] = [o.float() for o in PC.oracle_run(name, torch.float32, with_grad=False)[0]]
        else:
            dtype = torch.bfloat16 if kind == "fq_bf16" else torch.float32
            _oracle_cache[key] = [o.float() for o in FC.oracle_fake_quant_run(name, dtype, monkeypatch)]
    return _oracle_cache[key]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_bf16_within_the_fake_quant_oracles_own_bf16_error(name, monkeypatch):
    """Every figure is printed before it is asserted; DESIGN.md section 4.10 records the oracle side."""
    from mdm_hip import fp8

    model = _model(name)
    plain_hip = _outs(model, name)
    h = fp8.attach(model)
    assert all("ffn" in t and "qkv" in t and "proj_out" in t for _, _, t in h.layers)
    outs = _outs(model, name)
    ref, bar_outs, plain = _oracle(name, "fq", monkeypatch), _oracle(name, "fq_bf16", monkeypatch), _oracle(name, "plain", monkeypatch)
    err = [O.rel_l2(a, b) for a, b in zip(outs, ref)]
    bar = [O.rel_l2(a, b) for a, b in zip(bar_outs, ref)]
    # the path is taken: the distance to the PLAIN fp32 oracle is that of the fake-quant oracle run in bf16 (measured the same
    # way: independent code on the CPU), within the same factor 2 either way -- and the un-attached model lies below the band
    d_hip = [O.rel_l2(a, p) for a, p in zip(outs, plain)]
    d_bar = [O.rel_l2(f, p) for f, p in zip(bar_outs, plain)]
    d_off = [O.rel_l2(a, p) for a, p in zip(plain_hip, plain)]
    print("[fp8 model %s] rel-L2 vs fake-quant oracle %s (that oracle in bf16: %s); distance to the plain oracle %s "
          "(fake-quant oracle in bf16: %s; un-attached model: %s)" % (
              name, ["%.3e" % e for e in err], ["%.3e" % e for e in bar], ["%.3e" % e for e in d_hip],
              ["%.3e" % e for e in d_bar], ["%.3e" % e for e in d_off]))
    assert all(e <= 2 * b for e, b in zip(err, bar)), (err, bar)
    assert all(not torch.equal(a, b) for a, b in zip(outs, plain_hip))
    assert all(b / 2 <= d <= 2 * b for d, b in zip(d_hip, d_bar)), (d_hip, d_bar)
    assert all(d < b / 2 for d, b in zip(d_off, d_bar)), (d_off, d_bar)
    h.detach()


# ---- 5. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_detach_restores_and_a_changed_weight_requantises(name):
    from mdm_hip import fp8

    model = _model(name)
    before = _outs(model, name)
    h = fp8.attach(model)
    on = _outs(model, name)
    assert all(torch.equal(a, b) for a, b in zip(on, _outs(model, name)))          # deterministic
    assert all(not torch.equal(a, b) for a, b in zip(on, before))
    # other weight values through load_state_dict: no re-attach, the quantised copies follow the parameter version
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd2 = dict(sd)
    keys = [k for k in sd if k.endswith("qkv.weight") or k.endswith("ffn.3.weight")]
    assert keys
    for k in keys:
        sd2[k] = sd[k] * 1.5
    model.load_state_dict(sd2)
    changed = _outs(model, name)
    assert all(O.rel_l2(a, b) > 1e-3 for a, b in zip(changed, on))
    model.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(_outs(model, name), on))
    h.detach()
    assert all(torch.equal(a, b) for a, b in zip(_outs(model, name), before))      # bit for bit


def test_backward_and_fp32_activations_raise():
    from mdm_hip import _lib, fp8

    name = "mini_unet"
    model = _model(name)
    h = fp8.attach(model)
    inp = PC.inputs(name)
    args = (inp["x"].cuda(), inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), {})
    with pytest.raises(_lib.MdmHipError, match="inference-only"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model(*args)                                                # grad mode on, parameters require grad
    with pytest.raises(_lib.MdmHipError, match="bf16"):
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            model(*args)                                                # fp32 activations
    h.detach()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        PC.loss_of(model(*args), inp["gys"]).backward()                 # detached: trains as before
    assert all(m.qkv.weight.grad is not None for _, m, _ in h.layers)


def _pipe(name, model):
    from mdm_hip import diffusion as D
    from mdm_hip import samplers as S

    nested = name == "mini_nested"
    scfg = S.SamplerConfig(num_diffusion_steps=1000, schedule_type="DEEPFLOYD", prediction_type="V_PREDICTION",
                           loss_target_type="DDPM", threshold_function="CLIP", schedule_shifted=nested,
                           rescale_signal=1 if nested else None)
    if nested:
        return D.NestedDiffusion(model, D.NestedDiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False,
                                                                use_double_loss=True, no_use_residual=True)).to(torch.device(DEV))
    return D.Diffusion(model, D.DiffusionConfig(sampler_config=scfg, use_vdm_loss_weights=False)).to(torch.device(DEV))


def test_graphed_sampling_follows_attach():
    from mdm_hip import fp8
    from mdm_hip.graph import GraphedSampler

    name = "mini_unet"
    model = PC.build_module(name)[0]
    pipe = _pipe(name, model)
    pipe.eval()
    vm = pipe.model.vision_model
    inp = PC.inputs(name)
    cond, mask = inp["cond"].cuda(), inp["mask"].cuda()
    smp = {"lm_outputs": cond, "lm_mask": mask}
    side, n = 16, 4
    start = [torch.randn(2, 3, side, side, generator=_g(41)).cuda()]

    def eager():
        return pipe.sampler.sample(pipe.get_model(), start[0].clone(), cond, mask, {}, resample_steps=True,
                                   num_inference_steps=n, ddim_eta=0)

    def graphed(gs):
        return gs.sample(2, smp, side, torch.device(DEV), num_inference_steps=n, start_noise=start, ddim_eta=0)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        gs = GraphedSampler(pipe, seed=1)
        plain = graphed(gs).clone()                                     # captured BEFORE attach
        h = fp8.attach(vm)
        e_on = eager()
        assert O.rel_l2(e_on, plain) > 1e-3                             # fp8 changes the images
        g_on = graphed(gs).clone()                                      # the stale graph is not replayed: captured anew
        print("[fp8 graphed] eager vs graphed rel-L2 %.3e (differing elements %d / %d); fp8 vs plain %.3e" % (
            O.rel_l2(g_on, e_on), int((g_on != e_on).sum()), e_on.numel(), O.rel_l2(e_on, plain)))
        assert torch.equal(g_on, e_on) and len(gs._graphs) == 1         # eager and graphed: bit for bit
        assert torch.equal(graphed(gs), e_on) and len(gs._graphs) == 1  # ... and that one replays
        fresh = GraphedSampler(pipe, seed=1)
        assert torch.equal(graphed(fresh), g_on)
        h.detach()
        assert torch.equal(graphed(gs), plain) and len(gs._graphs) == 1
