"""GPU: the MXFP8 3x3 convolution (csrc/fp8.hip, the CONV form of mx8_gemm_kernel) against the restatement of
tests/fp8_conv_cases.py -- the activation with its zero row bit for bit, the convolution exactly on integer data (a wrong tap
order, shift, seam, scale byte or weight row shows on essentially every element) and on impulses at the image borders, within
bf16 output rounding on random data -- and the models with ``conv_targets`` attached against the fake-quant oracle, plus the
identities that make the path safe to use (detach restores, a changed weight re-quantises, no backward, no fp32, graphed
sampling follows attach).

Model gate (bf16), DESIGN.md section 4.10: rel-L2 against the fake-quant oracle in fp32 <= 2 x that oracle's OWN error when it
is run in bf16 on the CPU.  With ~20 quantised layers on random weights that figure is ~1.5e-1 (codes flip between bf16 and
fp32), so the model gate only shows that the path is wired; the sharp checks are the kernel tests.  Every figure is printed
before it is asserted (pytest -s)."""
import functools

import pytest
import torch

import fp8_cases as FC
import fp8_conv_cases as CC
import parity_cases as PC
import unet_oracle as O
from test_fp8_gpu import DEV, MODEL_CASES, _g, _model, _mx8, _outs, _pipe

pytestmark = pytest.mark.gpu


def _act(qa, sa, K):
    return _mx8(*CC.with_zero_row(qa, sa), K)


# ---- 1. the activation with its zero row ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(30, 32), (189, 288)])
def test_zero_row_form_is_the_quantiser_plus_a_zero_row(M, K):
    from mdm_hip import ops

    g = _g(M + K)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).float())).to(torch.bfloat16)
    q_ref, s_ref = FC.quant_ref(x)
    out = ops.mx8_quant_zrow(x.to(DEV))
    assert out.q.shape == (M + 1, q_ref.shape[1]) and out.s.shape == (M + 1, s_ref.shape[1]) and out.K == K
    q, s = out.q.cpu(), out.s.cpu()
    dq, ds = int((q[:M] != q_ref).sum()), int((s[:M] != s_ref).sum())
    print("[mx8_quant_zrow M=%d K=%d] differing codes %d / %d, scale bytes %d / %d; zero row: max code %d, scales %s" % (
        M, K, dq, q_ref.numel(), ds, s_ref.numel(), int(q[M].max()), sorted(set(s[M].tolist()))))
    assert dq == 0 and ds == 0
    assert int(q[M].max()) == 0 and bool((s[M] == 127).all())
    plain = ops.mx8_quant(x.to(DEV))                                    # the plain entry point is what it was
    assert torch.equal(plain.q.cpu(), q_ref) and torch.equal(plain.s.cpu(), s_ref)


# ---- 2. exact on integer data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,cin,cout", CC.CONV_SHAPES)
def test_conv_exact_on_integer_data(N, H, W, cin, cout):
    from mdm_hip import ops

    qa, sa, qw, sw = CC.exact_operands(N, H, W, cin, cout)
    ref = CC.conv_ref(qa, sa, qw, sw, (N, H, W))
    assert torch.equal(ref.float().double(), ref)                       # exact in fp32 (tests/test_fp8_conv_host.py) ...
    y = ops.mx8_conv3x3(_act(qa, sa, cin), _mx8(qw, sw, cin), (N, H, W))
    assert y.shape == (N, H, W, cout) and y.dtype == torch.bfloat16
    want = ref.float().to(torch.bfloat16)                               # ... so the output is the bf16 rounding of the exact value
    bad = int((y.cpu().float() != want.float()).sum())
    print("[mx8_conv3x3 exact %s] wrong elements %d / %d" % ((N, H, W, cin, cout), bad, want.numel()))
    assert bad == 0


# ---- 3. impulses at the borders -----------------------------------------------------------------------------------------------------
_IMP = (2, 5, 3, 64, 32)    # two channel blocks; every pixel of a 5 x 3 image touches a border


@functools.lru_cache(maxsize=None)
def _impulse_weight():
    N, H, W, cin, cout = _IMP
    tap = torch.arange(9, dtype=torch.float32).reshape(1, 1, 3, 3) + 1.0           # 1 .. 9: a value of its own per tap
    w = tap * torch.exp2((torch.arange(cout) % 4 - 2).float()).reshape(cout, 1, 1, 1) * torch.ones(1, cin, 1, 1)
    w[:, :32] = 7.0                                                     # the other channel block: must meet zeros only
    return CC.quant_weight_3x3(w)


@pytest.mark.parametrize("pixel", ["top_left", "top_right", "bottom_left", "last_of_image_0", "first_of_image_1"])
def test_impulse_at_a_border_pixel(pixel):
    """1.0 in channels 32 .. 63 of one pixel: each output pixel around it is 32 x the weight of exactly one tap, nothing
    crosses a row end (m +- 1) or the seam between the images (m +- W)"""
    from mdm_hip import ops

    N, H, W, cin, cout = _IMP
    m = {"top_left": 0, "top_right": W - 1, "bottom_left": (H - 1) * W, "last_of_image_0": H * W - 1, "first_of_image_1": H * W}[pixel]
    x = torch.zeros(N * H * W, cin)
    x[m, 32:] = 1.0
    qa, sa = FC.quant_ref(x)
    qw, sw = _impulse_weight()
    ref = CC.conv_ref(qa, sa, qw, sw, (N, H, W))
    want = ref.float().to(torch.bfloat16)
    assert torch.equal(want.double(), ref) and int((ref != 0).any(-1).sum()) == 4         # a corner reaches 4 pixels
    y = ops.mx8_conv3x3(_act(qa, sa, cin), _mx8(qw, sw, cin), (N, H, W))
    bad = int((y.cpu().float() != want.float()).sum())
    print("[mx8_conv3x3 impulse %s (row %d)] wrong elements %d / %d; pixels reached %d" % (
        pixel, m, bad, want.numel(), int((y.cpu().float() != 0).any(-1).sum())))
    assert bad == 0


# ---- 4. random data, 5. determinism ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(N, H, W, cin, cout):
    g = _g(N + H + W + cin + cout)
    M = N * H * W
    qa, sa = FC.quant_ref(torch.randn(M, cin, generator=g).to(torch.bfloat16))
    qw, sw = CC.quant_weight_3x3(torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5)
    bias = torch.randn(cout, generator=g) * 0.5
    res = torch.randn(N, H, W, cout, generator=g).to(torch.bfloat16)
    return qa, sa, qw, sw, bias, res, CC.conv_ref(qa, sa, qw, sw, (N, H, W)) + bias.double()


@pytest.mark.parametrize("epilogue", ["bias", "residual"])
@pytest.mark.parametrize("N,H,W,cin,cout", CC.CONV_SHAPES)
def test_conv_random(N, H, W, cin, cout, epilogue):
    """the project's elementwise bound of test_gemm_random: 2^-8 |ref| + 2^-8 max |pre-residual| against fp64 on the
    dequantised operands (one bf16 ulp -- twice the rounding error -- of the value and of the largest pre-residual value)"""
    from mdm_hip import ops

    qa, sa, qw, sw, bias, res, pre = _random_case(N, H, W, cin, cout)
    a, w = _act(qa, sa, cin), _mx8(qw, sw, cin)
    r = res.to(DEV) if epilogue == "residual" else None
    y = ops.mx8_conv3x3(a, w, (N, H, W), bias.to(DEV), residual=r)
    again = ops.mx8_conv3x3(a, w, (N, H, W), bias.to(DEV), residual=r)
    assert torch.equal(y, again)                                        # deterministic: no split-K
    yd = y.cpu().double()
    ref = pre + (res.double() if r is not None else 0.0)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * float(pre.abs().max())
    worst = float(((yd - ref).abs() / bound).max())
    print("[mx8_conv3x3 %s %s] worst |y - ref| / bound %.3f" % (epilogue, (N, H, W, cin, cout), worst))
    assert bool(((yd - ref).abs() <= bound).all())


def test_packed_weight_is_the_restatements():
    from mdm_hip import _lib, ops

    w = torch.nn.Parameter(torch.randn(64, 96, 3, 3, generator=_g(5)).to(DEV))
    b = torch.nn.Parameter(torch.randn(64, generator=_g(6)).to(DEV))
    with torch.no_grad():
        wq, bp = ops.packed_weight_mx8_3x3(w, b)
    q_ref, s_ref = CC.quant_weight_3x3(w.detach().cpu())
    assert wq.K == 96 and torch.equal(wq.q.cpu(), q_ref) and torch.equal(wq.s.cpu(), s_ref) and torch.equal(bp, b.detach())
    assert ops.packed_weight_mx8_3x3(w, b)[0] is wq                     # cached ...
    with torch.no_grad():
        w.mul_(2.0)                                                     # ... per parameter version, into the same buffers
        wq2, _ = ops.packed_weight_mx8_3x3(w, b)
    s2 = wq2.s.cpu()                                                    # x 2: the same codes, every scale one higher (K = 96: block 3 is padding)
    assert wq2.q.data_ptr() == wq.q.data_ptr() and torch.equal(wq2.q.cpu(), q_ref)
    assert torch.equal(s2[:, :3], s_ref[:, :3] + 1) and bool((s2[:, 3] == 127).all())
    with pytest.raises(_lib.MdmHipError):
        ops.packed_weight_mx8(w, b)                                     # the 1x1 entry keeps refusing 3x3 weights
    with pytest.raises(_lib.MdmHipError):
        ops.packed_weight_mx8_3x3(torch.nn.Parameter(torch.randn(32, 32, 1, 1).to(DEV)), None)


# ---- 6. models --------------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _oracle(name, kind, monkeypatch, attention=False):
    """computed once per case and shared (never modified): 'plain' fp32, 'fq' fake-quant fp32, 'fq_bf16' fake-quant in bf16"""
    key = (name, kind, attention and kind != "plain")
    if key not in _oracle_cache:
        if kind == "plain":
            _oracle_cache[key] = [o.float() for o in PC.oracle_run(name, torch.float32, with_grad=False)[0]]
        else:
            dtype = torch.bfloat16 if kind == "fq_bf16" else torch.float32
            _oracle_cache[key] = [o.float() for o in CC.oracle_fake_quant_run(name, dtype, monkeypatch, attention)]
    return _oracle_cache[key]


def _has_attention(model):
    from mdm_hip.unet import SelfAttention

    return any(isinstance(m, SelfAttention) for m in model.modules())


@pytest.mark.parametrize("which", ["convs", "convs_and_attention"])
@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_bf16_within_the_fake_quant_oracles_own_bf16_error(name, which, monkeypatch):
    """Measured on an MI355X (conv-only targets / attention targets too), rel-L2 against the fake-quant oracle, with that
    oracle's own bf16 error in brackets: see DESIGN.md section 4.10, which records both sides."""
    from mdm_hip import fp8

    model = _model(name)
    attention = which == "convs_and_attention"
    plain_hip = _outs(model, name)
    h = fp8.attach(model, targets=fp8.TARGETS if attention and _has_attention(model) else (), conv_targets=fp8.CONV_TARGETS)
    assert h.convs and all("conv1" in t and "conv2" in t for _, _, t in h.convs) and bool(h.layers) == (attention and _has_attention(model))
    outs = _outs(model, name)
    ref, bar_outs, plain = (_oracle(name, k, monkeypatch, attention) for k in ("fq", "fq_bf16", "plain"))
    err = [O.rel_l2(a, b) for a, b in zip(outs, ref)]
    bar = [O.rel_l2(a, b) for a, b in zip(bar_outs, ref)]
    d_hip = [O.rel_l2(a, p) for a, p in zip(outs, plain)]
    d_bar = [O.rel_l2(f, p) for f, p in zip(bar_outs, plain)]
    d_off = [O.rel_l2(a, p) for a, p in zip(plain_hip, plain)]
    print("[fp8 conv model %s, %s] rel-L2 vs fake-quant oracle %s (that oracle in bf16: %s); distance to the plain oracle %s "
          "(fake-quant oracle in bf16: %s; un-attached model: %s)" % (
              name, which, ["%.3e" % e for e in err], ["%.3e" % e for e in bar], ["%.3e" % e for e in d_hip],
              ["%.3e" % e for e in d_bar], ["%.3e" % e for e in d_off]))
    assert all(e <= 2 * b for e, b in zip(err, bar)), (err, bar)
    assert all(not torch.equal(a, b) for a, b in zip(outs, plain_hip))
    if not attention:
        # the path is taken: the distance to the PLAIN fp32 oracle is that of the fake-quant oracle run in bf16, within the
        # same factor 2 either way -- and the un-attached model lies below the band
        assert all(b / 2 <= d <= 2 * b for d, b in zip(d_hip, d_bar)), (d_hip, d_bar)
        assert all(d < b / 2 for d, b in zip(d_off, d_bar)), (d_off, d_bar)
    h.detach()


# ---- 7. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_detach_restores_and_a_changed_weight_requantises(name):
    from mdm_hip import fp8

    model = _model(name)
    before = _outs(model, name)
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    on = _outs(model, name)
    assert all(torch.equal(a, b) for a, b in zip(on, _outs(model, name)))          # deterministic
    assert all(not torch.equal(a, b) for a, b in zip(on, before))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd2 = dict(sd)
    keys = [k for k in sd if k.endswith("conv1.weight")]
    assert keys
    for k in keys:
        sd2[k] = sd[k] * 1.5
    model.load_state_dict(sd2)                                          # no re-attach: the quantised copies follow the version
    changed = _outs(model, name)
    assert all(O.rel_l2(a, b) > 1e-3 for a, b in zip(changed, on))
    model.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(_outs(model, name), on))
    h.detach()
    assert all(torch.equal(a, b) for a, b in zip(_outs(model, name), before))      # bit for bit


def test_min_channels_keeps_narrow_resnets_on_bf16():
    """mini_unet has 32- and 256-channel ResNets: with min_channels=64 the narrow ones run the bf16 kernels -- the output
    differs from both the all-fp8 and the all-bf16 model's"""
    from mdm_hip import fp8

    name = "mini_unet"
    model = _model(name)
    off = _outs(model, name)
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    full = _outs(model, name)
    h.detach()
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS, min_channels=64)
    part = _outs(model, name)
    h.detach()
    assert not torch.equal(part[0], full[0]) and not torch.equal(part[0], off[0])
    assert torch.equal(_outs(model, name)[0], off[0])


# ---- 8. graphed sampling ------------------------------------------------------------------------------------------------------------
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
        h = fp8.attach(vm, conv_targets=fp8.CONV_TARGETS)
        e_on = eager()
        assert O.rel_l2(e_on, plain) > 1e-3
        g_on = graphed(gs).clone()                                      # the stale graph is not replayed: captured anew
        print("[fp8 conv graphed] eager vs graphed rel-L2 %.3e (differing elements %d / %d); fp8 vs plain %.3e" % (
            O.rel_l2(g_on, e_on), int((g_on != e_on).sum()), e_on.numel(), O.rel_l2(e_on, plain)))
        assert torch.equal(g_on, e_on) and len(gs._graphs) == 1         # eager and graphed: bit for bit
        assert torch.equal(graphed(gs), e_on) and len(gs._graphs) == 1  # ... and that one replays (the zero row with it)
        h.detach()
        assert torch.equal(graphed(gs), plain) and len(gs._graphs) == 1


# ---- 9. refused inputs --------------------------------------------------------------------------------------------------------------
def test_backward_and_fp32_activations_raise():
    from mdm_hip import _lib, fp8, ops
    from mdm_hip.unet import ResNet

    name = "mini_unet"
    model = _model(name)
    h = fp8.attach(model, targets=(), conv_targets=fp8.CONV_TARGETS)
    inp = PC.inputs(name)
    args = (inp["x"].cuda(), inp["times"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), {})
    with pytest.raises(_lib.MdmHipError, match="inference-only"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model(*args)                                                # grad mode on, parameters require grad
    with pytest.raises(_lib.MdmHipError, match="bf16"):
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            model(*args)                                                # fp32 activations
    with pytest.raises(_lib.MdmHipError, match="bf16"):
        ops.mx8_quant_zrow(torch.zeros(4, 32, device=DEV))
    with pytest.raises(_lib.MdmHipError, match="inference-only"):
        ops.mx8_quant_zrow(torch.zeros(4, 32, device=DEV, dtype=torch.bfloat16, requires_grad=True))
    h.detach()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        PC.loss_of(model(*args), inp["gys"]).backward()                 # detached: trains as before
    assert all(m.conv1.weight.grad is not None for m in model.modules() if isinstance(m, ResNet))
