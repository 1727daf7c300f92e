"""Cases shared by the attention-map-guidance tests (CPU and GPU): the fp64 gradient of ``sum(dacc * M)`` with respect to q
by torch autograd through ``attn_map_cases.probs_ref``, kernel inputs with NaN where nothing may be computed on, the oracle
with a recording hook that stays on the autograd tape (``attn_map_cases.recording_oracle`` outside ``no_grad``; with PAG
and regions: the layer of ``region_cases.biased_attention_layer``), a stub denoiser with a differentiable map term, and
the guided sampling loop restated in torch ops around the oracle."""
import contextlib
import functools

import torch

import attn_map_cases as AC
import pag_cases as PG
import parity_cases as PC
import region_cases as RC
import unet_oracle as O


# ---- the kernel ----------------------------------------------------------------------------------------------------
def dq_ref(qkv, kvc, mask, heads, dacc, w=1.0):
    """fp64: d/dq of sum(w * dacc[..., :S] * M), M the head-mean probabilities of ``attn_map_cases.probs_ref`` without a
    bias.  qkv [B, L, 3C], kvc [B, S, 2C], mask [B, S] or None, dacc [B, L, >= S] (NaN allowed in the pad columns and in
    the masked keys' entries: they are replaced by 0, their probability is exactly 0) -> [B, L, C]"""
    C = qkv.shape[-1] // 3
    S = kvc.shape[1]
    q = qkv.double()[..., :C].transpose(1, 2).clone().requires_grad_(True)
    p, _ = AC.probs_ref(q, kvc.double()[..., :C].transpose(1, 2), heads, mask, None)
    g = dacc[..., :S].double()
    if mask is not None:
        g = torch.where((mask != 0)[:, None, :], g, torch.zeros_like(g))
    assert torch.isfinite(g).all()
    dq, = torch.autograd.grad((w * g * p).sum(), q)
    return dq.transpose(1, 2).contiguous()


def dq_uniform_ref(kvc, n_live, dacc, d):
    """fp64, q = 0 and H = 1 with the first ``n_live`` keys live, by the definition itself: P = 1 / n_live, delta = sum P g,
    dS = P (g - delta), dq = dS k_c / sqrt(d).  With n_live and d powers of two and small-integer g and k_c every operation
    is EXACT in fp64 (``dq_ref`` carries the rounding of its own scale, (d^-1/4)^2, and returns 1e-17 where this is 0)."""
    g = dacc[..., :n_live].double()
    P = 1.0 / n_live
    dS = P * (g - (P * g).sum(-1, keepdim=True))
    return torch.einsum("bls,bsc->blc", dS, kvc.double()[:, :n_live, :d]) / (d ** 0.5)


def kernel_dacc(L, S, mask=None, seed=0):
    """[3, L, ld] fp32: ``attn_map_cases.kernel_acc`` (N(0, 1), NaN in the pad columns) with NaN in the entries of the
    keys that ``mask`` excludes"""
    a = AC.kernel_acc(L, S, seed).clone()
    if mask is not None:
        a[..., :S] = torch.where((mask != 0)[:, None, :], a[..., :S], torch.full_like(a[..., :S], float("nan")))
    return a


def first_keys_mask(S, n):
    """[3, S]: the first ``n`` keys live in every batch row"""
    m = torch.zeros(3, S)
    m[:, :n] = 1
    return m


# ---- the oracle with recording layers on the tape ----------------------------------------------------------------------
def maps_of(store):
    """what ``recording_oracle`` left in ``store`` -> {(h, w): fp64 [B, S, h, w]}, the mean over the layers"""
    return {(h, w): (t / n).transpose(1, 2).reshape(t.shape[0], t.shape[2], h, w) for (h, w), (t, n) in store.items()}


def oracle_map_grads(name, weights_of):
    """fp32 oracle forward of ``pag_cases.model_inputs(name)`` (batch 4) on leaf x with every text layer recording, on the
    tape; loss = sum over resolutions of sum(weights * maps) -> (loss, [d loss / d x of every scale], maps detached).
    ``weights_of(key, shape)`` -> the fixed weights of a resolution.  ``autocast``: see ``oracle_map_grads_bf16``."""
    return _oracle_map_grads(name, weights_of, False)


def _oracle_map_grads(name, weights_of, bf16):
    from mdm_hip import attn_maps as A

    model, cfg, sd = PC.build_module(name)
    names = A.layer_names(model, "all")
    inp = PG.model_inputs(name)
    xs = [t.clone().requires_grad_(True) for t in PC.as_list(inp["x"])]
    store = {}
    auto = torch.autocast("cpu", dtype=torch.bfloat16) if bf16 else contextlib.nullcontext()
    with torch.enable_grad(), AC.recording_oracle(sd, names, store), auto:
        O.model_forward(sd, cfg, xs if isinstance(inp["x"], list) else xs[0], inp["times"], inp["cond"], inp["mask"], {})
    with torch.enable_grad():
        maps = maps_of(store)
        loss = sum((weights_of(k, m.shape).double() * m).sum() for k, m in sorted(maps.items()))
        grads = torch.autograd.grad(loss, xs, allow_unused=True)
    return loss.detach(), [None if g is None else g.detach() for g in grads], {k: m.detach() for k, m in maps.items()}


def oracle_map_grads_bf16(name, weights_of):
    """the same under bf16 autocast: the oracle's own bf16 error, the yardstick of the bf16 gate"""
    return _oracle_map_grads(name, weights_of, True)


def map_weights(key, shape):
    """fixed N(0, 1) weights of one resolution's maps"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(100 * key[0] + key[1]))


@contextlib.contextmanager
def options_oracle(sd, pag_names, pag_rows, region_names, rp):
    """Inside, ``unet_oracle.attention_layer`` is the layer of ``region_cases.biased_attention_layer`` for the layers
    ``region_names`` (bias ``rp``), with the trailing ``pag_rows`` rows perturbed in the layers ``pag_names``; a layer in
    ``pag_names`` only is ``pag_cases.perturbed_attention_layer``"""
    ids = lambda names: {id(sd[n + ".qkv.weight"]) for n in names}
    pag_ids, region_ids = ids(pag_names), ids(region_names)
    orig = O.attention_layer

    def layer(sd_, pfx, x, cond, cond_mask, heads=8):
        key = id(sd_[pfx + "qkv.weight"])
        rows = pag_rows if key in pag_ids else 0
        if key in region_ids:
            return RC.biased_attention_layer(sd_, pfx, x, cond, cond_mask, heads, rp, rows)
        if rows:
            return PG.perturbed_attention_layer(sd_, pfx, x, cond, cond_mask, heads, rows)
        return orig(sd_, pfx, x, cond, cond_mask, heads)

    O.attention_layer = layer
    try:
        yield
    finally:
        O.attention_layer = orig


def restated_guided_loop(smp, model, sd, cfg, xs, cond, mask, n, w, fn, scale, interval, names, solver=None, iterations=1,
                         pag=None, regions=None):
    """The guided loop of ``Sampler._sample`` written out in torch ops on CPU tensors around the ORACLE (``sd``, ``cfg``):
    per step inside ``interval`` (fractions of the schedule, for the time the step starts from), ``iterations`` times: the
    oracle on leaf x_t, the conditional rows with the conditional text, the layers ``names`` recording on the tape,
    loss = fn(maps), x_t <- x_t - scale d loss.sum() / d x_t; then the plain step -- the oracle on [uncond | cond
    (| perturbed)], the torch combine and the sampler's torch step formulas.  ``smp`` / ``model``: a CPU sampler and the
    module it reads the scale layout from; ``cond`` / ``mask``: [uncond | cond].  ``pag`` = (layer names, scale);
    ``regions`` = (layer names, RegionPrompts).  -> the final image(s), post-processed like ``sample``"""
    from mdm_hip import samplers as SM

    nested = len(xs) > 1
    clip = lambda x0, sc: smp.clip_sample(x0, sc)
    steps = smp.set_timesteps(n)
    xs = [x.clone() for x in xs]
    B = xs[0].shape[0]
    image_scales = smp._scale_info(model)[1]
    cond_c, mask_c = cond[-B:], mask[-B:]
    reps = 2 + (pag is not None)
    cond_all, mask_all = (torch.cat([cond, cond_c]), torch.cat([mask, mask_c])) if pag is not None else (cond, mask)
    call = lambda x, t, c, m: PC.as_list(O.model_forward(sd, cfg, x if nested else x[0], t, c, m, {}))
    x0_prev = g_prev = None
    for i in range(n):
        t0 = int(steps[i])
        if interval[0] <= t0 / smp.n_steps <= interval[1]:
            for _ in range(iterations):
                leaves = [x.detach().clone().requires_grad_(True) for x in xs]
                store = {}
                with torch.enable_grad(), AC.recording_oracle(sd, names, store):
                    call(leaves, torch.full((B,), t0 - 1, dtype=torch.long), cond_c, mask_c)
                    loss = fn({k: m.float() for k, m in maps_of(store).items()})
                    grads = torch.autograd.grad(loss.sum(), leaves, allow_unused=True)
                xs = [x if g is None else (x - scale * g).detach() for x, g in zip(leaves, grads)]
                xs = [x.detach() for x in xs]
        with torch.no_grad():
            t = torch.full((reps * B,), t0 - 1, dtype=torch.long)
            xin = [torch.cat([x] * reps) for x in xs]
            ctx = contextlib.nullcontext()
            if pag is not None or regions is not None:
                rp = None if regions is None else regions[1].rows_for(True, pag is not None, None)
                ctx = options_oracle(sd, pag[0] if pag else (), B if pag else 0, regions[0] if regions else (), rp)
            with ctx:
                preds = call(xin, t, cond_all, mask_all)
            g_t, g_s = smp._scale_gammas(model, t0, B), smp._scale_gammas(model, int(steps[i + 1]), B)
            second = solver is not None and 0 < i < n - 1
            x0s = []
            for k, p in enumerate(preds):
                parts = p.float().chunk(reps)
                if pag is not None:
                    comb = SM.pag_combine(parts[1], parts[0], parts[2], w, pag[1])
                else:
                    comb = parts[0] + w * (parts[1] - parts[0])
                if solver is None:
                    x0, xs[k], _ = smp.get_prediction_xt_last(xs[k], comb, g_t[k], g_s[k], clip_fn=clip, ddim_eta=0,
                                                             image_scale=image_scales[k], return_eps=False)
                else:
                    x0, xs[k] = smp.get_prediction_xt_last_2m(xs[k], comb, g_t[k], g_s[k], g_prev=g_prev[k] if second else None,
                                                             x0_prev=x0_prev[k] if second else None, second_order=second,
                                                             clip_fn=clip, image_scale=image_scales[k])
                x0s.append(x0)
            x0_prev, g_prev = x0s, g_t
    return smp._postprocess(xs if nested else xs[0], clip=True)


# ---- a stub denoiser with a differentiable map term ----------------------------------------------------------------------
class MapStub(AC.RecordingStub):
    """``attn_map_cases.RecordingStub`` whose attention layers that carry an ``_attn_rec`` handle call its ``record`` with a
    qkv that is a fixed linear function of the image (8 x 8 queries, C = 32, one head) and text keys that are a fixed
    linear function of ``lm``: a loss on the maps reaches x, the stub's output does not depend on the recording.  Every
    call also records the grad mode, whether x requires grad, and the type of handle it saw."""

    HEADS = 1

    def __init__(self, nested=False):
        super().__init__(nested)
        g = torch.Generator().manual_seed(77)
        self.wq = torch.randn(3, 96, generator=g)
        self.wk = torch.randn(8, 64, generator=g) / 3
        self.grad_seen = []

    def qkv_of(self, x, k=0):
        n, c, h, w = x.shape
        return (x.permute(0, 2, 3, 1).reshape(n, h * w, c) @ self.wq) * (1.0 + 0.5 * k)

    def kvc_of(self, lm):
        return lm @ self.wk

    def forward(self, x, t, lm, mask, micros={}):
        x0 = x[0] if self.nested else x
        self.grad_seen.append(dict(grad=torch.is_grad_enabled(), leaf=bool(x0.requires_grad),
                                   handles={n: type(m._attn_rec).__name__ for n, m in self.attention().items()
                                            if m._attn_rec is not None},
                                   switches={n: (m._pag_rows, m._cross_bias is not None) for n, m in self.attention().items()}))
        for k, (n, m) in enumerate(sorted(self.attention().items())):
            if m._attn_rec is not None and m.cond_dim:
                m._attn_rec.record(self.qkv_of(x0, k), self.kvc_of(lm), mask, self.HEADS, None, x0.shape[0], *x0.shape[2:])
        return super().forward(x, t, lm, mask, micros)
