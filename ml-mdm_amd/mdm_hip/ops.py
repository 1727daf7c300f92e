"""torch.autograd bindings of the libmdm_hip C ABI (include/mdm_hip.h).

PyTorch is used here for device memory (tensors as buffers), the current HIP
stream and the autograd tape only; every arithmetic step is a call into the
shared library through raw pointers.  Activations are NHWC tensors
``[N, H, W, C]`` (or ``[rows, C]`` for linear layers) of the compute dtype
(``torch.float32`` = exact parity mode, ``torch.bfloat16`` = throughput mode).
Parameters stay fp32 in the reference's layout; packed copies for the kernels
are cached per parameter version.
"""
import ctypes
import weakref

import torch

from . import _lib
from . import tiling as _tiling

F32, BF16, F32_SPLIT, F32_SPLIT_W = 0, 1, 2, 3

# fp32 tensors, products as three bf16 MFMAs on bf16 hi + lo halves (include/mdm_hip.h MDM_F32_SPLIT): the arithmetic of
# sampling at the reference's precision (it samples in fp32, diffusion.py:181-197) at about a third of the bf16 rate.  Only
# the forward matmul-class launches have the path (convolutions / linears, attention); training in fp32 stays exact.
_fp32_split = False
_weight_planes_on = True   # split the weights in the k-loop too (tests turn it off for the in-loop split)


class fp32_split:
    """``with ops.fp32_split():`` (or ``ops.fp32_split(True)`` / ``(False)`` as a switch) -- every matmul-class launch on
    fp32 tensors inside (convolutions, linears, the attention forward; ALSO the input-gradient GEMMs of a backward pass run
    inside the context: they share the forward kernels) forms its products as bf16x3.  No effect on bf16 tensors, on the
    weight-gradient and attention-backward kernels.  It is a sampling mode: a process-wide switch (not thread-safe), read at
    launch time -- a hipGraph captured by ``GraphedSampler`` keeps the arithmetic it was captured with, and the sampler
    keys its graphs on the switch."""

    def __init__(self, enabled: bool = True):
        global _fp32_split
        self._prev = _fp32_split
        _fp32_split = bool(enabled)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        global _fp32_split
        _fp32_split = self._prev


def fp32_split_enabled() -> bool:
    return _fp32_split


def _dt_mm(t: torch.Tensor) -> int:
    """dtype code of a forward matmul-class launch"""
    d = _dt(t)
    return F32_SPLIT if (d == F32 and _fp32_split) else d


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise _lib.MdmHipError("unsupported activation dtype %s" % t.dtype)


def _epv(t: torch.Tensor) -> int:
    return 4 if t.dtype == torch.float32 else 8


def _p(t):
    return None if t is None else t.data_ptr()


# The current stream's raw handle.  torch.cuda.current_stream() builds a Stream object through four Python layers (device
# index lookups, is_available(), an environment read): ~5 us a call, ~1100 calls per nested-256 train step -- a sixth of the
# host's time per step in a profile (tools/host_profile.py), on a step whose small inner-U-Net kernels leave the host little
# lead.  The C entry point behind it returns the same handle in ~0.2 us.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


_stream_objs = {}   # raw handle -> torch Stream object of a stream that has been current (torch never destroys its streams)


def _current_stream_obj():
    raw = _stream()
    st = _stream_objs.get(raw)
    if st is None:
        if len(_stream_objs) > 64:
            _stream_objs.clear()
        st = _stream_objs[raw] = torch.cuda.current_stream()
    return st


def _require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.MdmHipError(
            "mdm_hip ops run only on an MI355X (got a %s tensor); there is no CPU fallback" % t.device
        )


def _f32_ws(nbytes: int, device):
    return torch.empty((max(int(nbytes), 4) + 3) // 4, dtype=torch.float32, device=device)


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------------------
# packed-weight cache
# --------------------------------------------------------------------------------------
_wcache = {}  # id(param) -> (weakref to the param, {dtype: (version key, packed tensors)})
_pack_epoch = 0


def invalidate_packed_weights():
    """Force a re-pack of every cached kernel-layout weight on next use.  Needed after parameter updates that
    do not bump ``Tensor._version`` (torch's fused optimizers, our own fused optimizer kernel)."""
    global _pack_epoch
    _pack_epoch += 1


# --------------------------------------------------------------------------------------
# gradient sink: parameter gradients written straight into a flat arena
# --------------------------------------------------------------------------------------
_grad_sink = None


def set_grad_sink(sink):
    """``sink.slot(param)`` -> fp32 view of the parameter's slot in a flat gradient arena (or None) and
    ``sink.ready(param)`` is called once the gradient has been added there.  With a sink installed the backward
    kernels accumulate into the arena (C ABI ``accumulate`` flag) and return no gradient to autograd, which removes
    one ``grad += new`` kernel per parameter per step.  ``None`` restores plain autograd semantics."""
    global _grad_sink
    if _grad_sink is not None and sink is not _grad_sink:
        flush_wgrad_queue()   # queued work refers to the old sink's slots
    _grad_sink = sink


def _slot(param):
    if _grad_sink is None or param is None:
        return None
    return _grad_sink.slot(param)


def _sink_defer(param):
    """tell the sink that ready(param) will come after the autograd node returns (optional part of the protocol)"""
    f = getattr(_grad_sink, "defer", None)
    if f is not None and param is not None:
        f(param)


# Weight gradients are off the critical path of backward (nothing downstream reads them before the optimizer), so
# with a gradient sink installed they can run on a second HIP stream and fill the CUs that the many small kernels
# of the main chain (norm statistics, layer-norm, reductions, tiny GEMMs) leave idle.
_side_stream = None
_async_wgrad = False


def enable_async_wgrad(flag: bool):
    global _async_wgrad
    _async_wgrad = bool(flag)


def side_stream():
    """the weight-gradient stream"""
    global _side_stream
    if _side_stream is None:
        _side_stream = torch.cuda.Stream()
    return _side_stream


# Tensors the side stream is still reading.  Holding a reference does two things: the caching allocator cannot hand the
# block to someone else, and -- the subtle one -- autograd cannot accumulate INTO the tensor in place: a ConvFn /
# FFNFn backward hands `dy` on as the gradient of its residual input, and the engine's InputBuffer adds a second
# incoming gradient in place (on the main stream) only when it holds the sole reference to the first.  Entries are
# dropped once the side-stream event recorded behind their reader has completed, and all at once at the join.
_side_keep = []


def join_side_stream():
    """make the current stream wait for everything queued on the weight-gradient stream"""
    if _side_stream is not None:
        torch.cuda.current_stream().wait_stream(_side_stream)
    _side_keep.clear()   # every later main-stream write is ordered behind the side stream's reads now


def _off_critical_path(tensors, fn):
    """run fn() (kernel launches that only write gradient-arena slots) on the side stream when enabled"""
    if not (_async_wgrad and _grad_sink is not None):
        return fn()
    side = side_stream()
    if _raw_stream is None:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
            done = torch.cuda.Event()
            done.record(side)
    else:
        # the same, without the Python layers of current_stream() / the StreamContext (this runs ~120 times per step)
        cur = _current_stream_obj()
        side.wait_stream(cur)
        torch.cuda.set_stream(side)
        try:
            fn()
            done = torch.cuda.Event()
            done.record(side)
        finally:
            torch.cuda.set_stream(cur)
    # The operands stay referenced here until the side stream has passed `done` (the purge below) or the main stream has been
    # made to wait for the side stream (join_side_stream): their blocks cannot be handed out again before that, so no
    # Tensor.record_stream is needed.  (Rounds 2-6 called it as well: the caching allocator then records one event per block
    # on the side stream when the block is freed -- a purge of 64 entries freed ~330 blocks at once, 0.5-1.3 ms of
    # hipEventRecord calls = as many marker packets in the side stream's queue, and at the end of backward, where the main
    # stream waits for the side stream, a gap of that length with the whole GPU idle: tools/fwd_gaps.py --gaps;
    # the host itself is 57-117 ms ahead, profiles/r06_host_lead.txt.)
    live = [t for t in tensors if t is not None]
    _side_keep.append((done, live))
    if len(_side_keep) >= 64:
        _side_keep[:] = [e for e in _side_keep if not e[0].query()]


# --------------------------------------------------------------------------------------
# deferred, grouped weight gradients of same-shape 1x1 convolutions
# --------------------------------------------------------------------------------------
# With the gradient sink installed nothing downstream reads a weight gradient before the optimizer, so the launch can
# wait: the (x, dy) pairs of same-shape 1x1 convolutions are queued and, at a flush point (a resolution-level boundary
# of the U-Net, or the end of backward), each queue that fills the chip as ONE grouped launch goes out as
# mdm_conv_wgrad_grouped -- no split of the pixel reduction, no fp32 slabs, no reduce kernel; the others are launched
# one by one as before.  Costs memory (x and dy stay alive until the flush: ~10 GB for UNet-64 at batch 64), not time.
_defer_wgrad = False
_wgrad_queue = {}   # (M, Cin, Cout, device) -> [(x2d, dy2d, weight, bias, slot, bslot)]
_WG_MAX = 32


def enable_deferred_wgrad(flag: bool, max_group: int = 32):
    """``max_group``: layers per grouped launch (<= 32).  Smaller groups hand gradients to the all-reduce earlier
    (multi-GPU runs), larger ones fill the chip better."""
    global _defer_wgrad, _WG_MAX
    flush_wgrad_queue()
    _defer_wgrad = bool(flag)
    _WG_MAX = max(1, min(32, int(max_group)))


def wgrad_grouped(xs, dys, dws, dbs=None):
    """dws[g] (Cout, Cin) += dys[g]^T xs[g]; dbs[g] (Cout) += column sums of dys[g] -- one launch (C ABI
    mdm_conv_wgrad_grouped).  xs[g] [M, Cin], dys[g] [M, Cout] bf16."""
    G = len(xs)
    M, cin = xs[0].shape
    cout = dys[0].shape[1]
    for t in list(xs) + list(dys):
        _require_gpu(t)
    xs, dys = [_c(t) for t in xs], [_c(t) for t in dys]
    arr = lambda vals: (ctypes.c_void_p * G)(*vals)
    _lib.check(_lib.lib().mdm_conv_wgrad_grouped(arr([_p(t) for t in xs]), arr([_p(t) for t in dys]), arr([_p(t) for t in dws]),
                                                 arr([_p(t) for t in dbs]) if dbs is not None else None, G, M, cin, cout,
                                                 _dt(xs[0]), _stream()), "mdm_conv_wgrad_grouped")


def _queue_wgrad(x, dy, weight, bias, slot, bslot, M, cin, cout):
    key = (M, cin, cout, x.device.index)
    q = _wgrad_queue.setdefault(key, [])
    q.append((x, dy, weight, bias, slot, bslot))
    _sink_defer(weight)
    if bslot is not None:
        _sink_defer(bias)
    if len(q) == _WG_MAX:
        _flush_key(key)


def _flush_key(key):
    q = _wgrad_queue.pop(key, None)
    if not q:
        return
    M, cin, cout, _ = key
    L = _lib.lib()
    tile = ctypes.c_int(0)
    _lib.check(L.mdm_conv_wgrad_group_plan(M, cout, cin, BF16, len(q), ctypes.byref(tile)), "mdm_conv_wgrad_group_plan")
    tensors = [t for e in q for t in (e[0], e[1])]
    if tile.value and all((e[5] is not None) == (q[0][5] is not None) for e in q):
        G = len(q)
        arr = lambda vals: (ctypes.c_void_p * G)(*vals)
        xs, dys, dws = arr([_p(e[0]) for e in q]), arr([_p(e[1]) for e in q]), arr([_p(e[4]) for e in q])
        dbs = arr([_p(e[5]) for e in q]) if q[0][5] is not None else None

        def go():
            _prof_wrap("conv_wgrad grouped x%d M=%d N=%d K=%d" % (G, M, cout, cin), 2.0 * G * M * cout * cin, lambda: _lib.check(
                L.mdm_conv_wgrad_grouped(xs, dys, dws, dbs, G, M, cin, cout, BF16, _stream()), "mdm_conv_wgrad_grouped"))
            for e in q:
                _grad_sink.ready(e[2])
                if e[5] is not None:
                    _grad_sink.ready(e[3])
    else:
        def go():
            for x, dy, w, b, slot, bslot in q:
                _wgrad_launch(x, dy, M, 1, 1, cin, 1, 1, cout, 1, 1, out=slot, dbias=bslot)
                _grad_sink.ready(w)
                if bslot is not None:
                    _grad_sink.ready(b)

    _off_critical_path(tensors, go)


def flush_wgrad_queue():
    """launch every queued weight gradient (call at resolution-level boundaries and before the optimizer)"""
    for key in list(_wgrad_queue):
        _flush_key(key)
    flush_gn_params()


# --------------------------------------------------------------------------------------
# deferred GroupNorm parameter gradients
# --------------------------------------------------------------------------------------
# dgamma / dbeta of a GroupNorm are sums over the batch of per-sample terms.  Adding them into the gradient slot with
# atomics from inside the backward kernel costs as much as the kernel itself at the 16x16 level (64 samples x 1536
# addresses on two memory channels: 45 us against 24 us); a reduce kernel per layer is ~100 tiny launches per step.
# With the sink installed nothing reads these gradients before the optimizer, so the kernels store per-sample rows
# into a pooled buffer and ONE launch per flush point (mdm_gn_param_reduce_multi) adds the rows of every pending layer
# into their slots -- in a fixed order, so the result is deterministic as well.
_gn_pending = []     # (pg, pb, slot_g, slot_b, N, C, gamma, beta)
_gn_pool = {}        # device index -> [buffer (fp32), offset, high-water mark of the current step]
_gn_tables = {}      # tuple of (pointers, sizes) -> device descriptor table


def _gn_rows(N, C, device):
    """two [N, C] fp32 row blocks out of the pool (the same addresses every step: the descriptor table is reused)"""
    ent = _gn_pool.get(device.index)
    need = 2 * N * C
    if ent is None or ent[1] + need > ent[0].numel():
        # grow: pending entries keep their old buffer alive through the tensors they hold
        size = max(need, 0 if ent is None else 2 * ent[0].numel(), 16 << 20)
        ent = _gn_pool[device.index] = [torch.empty(size, dtype=torch.float32, device=device), 0]
    off = ent[1]
    ent[1] = off + need
    return ent[0][off:off + N * C], ent[0][off + N * C:off + need]


def flush_gn_params():
    """add the pending per-sample GroupNorm parameter-gradient rows into their gradient slots (one launch)"""
    if not _gn_pending:
        return
    dev = _gn_pending[0][0].device
    key = tuple((e[0].data_ptr(), e[1].data_ptr(), e[2].data_ptr(), e[3].data_ptr(), e[4], e[5]) for e in _gn_pending)
    ent = _gn_tables.get(key)
    if ent is None:
        import numpy as np
        rec = np.zeros(len(key), dtype=[("pg", "<u8"), ("pb", "<u8"), ("dg", "<u8"), ("db", "<u8"), ("N", "<i4"),
                                         ("C", "<i4"), ("first", "<i4"), ("pad", "<i4")])
        blocks = 0
        for i, (pg, pb, dg, db, N, C) in enumerate(key):
            rec[i] = (pg, pb, dg, db, N, C, blocks, 0)
            blocks += (C + 255) // 256
        table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        if len(_gn_tables) > 64:
            _gn_tables.clear()
        ent = _gn_tables[key] = (table, blocks)
    table, blocks = ent
    _lib.check(_lib.lib().mdm_gn_param_reduce_multi(_p(table), len(key), blocks, _stream()), "mdm_gn_param_reduce_multi")
    for e in _gn_pending:
        _grad_sink.ready(e[6])
        _grad_sink.ready(e[7])
    _gn_pending.clear()
    for ent in _gn_pool.values():
        ent[1] = 0   # the next rows are written by kernels queued behind the reduce on the same stream


class _FlushPointFn(torch.autograd.Function):
    """identity whose backward marks a point of the backward pass at which queued weight gradients are launched"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        flush_wgrad_queue()
        return dy


def wgrad_flush_point(x):
    return _FlushPointFn.apply(x) if (_defer_wgrad and x.requires_grad) else x


def _wgrad_into_sink(x, dy, weight, bias, slot, bslot, N, H, W, cin, Ho, Wo, cout, ks, stride):
    """weight (+ bias) gradient of a convolution whose destinations are gradient-arena slots: queued for a grouped
    launch when it qualifies, else launched now off the critical path"""
    M = N * Ho * Wo
    if _defer_wgrad and _async_wgrad and ks == 1 and x.dtype == torch.bfloat16 and M >= 4096:
        _queue_wgrad(x.reshape(M, cin), dy.reshape(M, cout), weight, bias, slot, bslot, M, cin, cout)
        return

    def go():
        _wgrad_launch(x, dy, N, H, W, cin, Ho, Wo, cout, ks, stride, out=slot, dbias=bslot)
        _grad_sink.ready(weight)
        if bslot is not None:
            _grad_sink.ready(bias)

    _off_critical_path((x, dy), go)


def _cache_slot(weight):
    k = id(weight)
    ent = _wcache.get(k)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _r, k=k: _wcache.pop(k, None)), {})
        _wcache[k] = ent
    return ent[1]


def _round_up(v, m):
    return (v + m - 1) // m * m


def packed_weight(weight: torch.Tensor, bias, dtype: torch.dtype, forward_only: bool = False):
    """(w_fwd, w_dgrad, bias_padded, Cin_pad, Cout_pad) for a reference-layout weight
    ``(Cout, Cin, k, k)`` or ``(Cout, Cin)``; refreshed when the parameter version changes.
    ``forward_only``: no input-gradient copy is built (w_dgrad is None) -- for a model that never runs backward (the
    frozen text encoder: the second copy of flan-t5-xl's weights would be 2.4 GB); cached apart from the default pack."""
    key = (dtype, "fwd") if forward_only else dtype
    ent = _cache_slot(weight)
    ver = (weight._version, None if bias is None else bias._version, weight.data_ptr(), _pack_epoch)
    if key in ent and ent[key][0] == ver:
        return ent[key][1]
    _require_gpu(weight)
    L = _lib.lib()
    cout, cin = weight.shape[0], weight.shape[1]
    ks = weight.shape[2] if weight.dim() == 4 else 1
    epv = 4 if dtype == torch.float32 else 8
    cin_pad, cout_pad = _round_up(cin, epv), _round_up(cout, epv)
    taps = ks * ks
    w32 = _c(weight.detach().float())
    need_d = cin_pad == cin and not forward_only
    prev = ent[key][1] if key in ent else None   # re-pack into the same buffers: their addresses stay valid (repack_all table)
    if prev is not None and prev[0].numel() == cout_pad * taps * cin_pad and prev[0].device == weight.device:
        wf, wd = prev[0], prev[1]
    else:
        wf = torch.empty(cout_pad * taps * cin_pad, dtype=dtype, device=weight.device)
        wd = torch.empty(cin * taps * cout_pad, dtype=dtype, device=weight.device) if need_d else None
        if cout_pad != cout:
            wf.zero_()
    # 3x3: channel-block-major reduction order whenever the channel count is a multiple of the k-tile
    bk = 32 if dtype == torch.float32 else 64
    kbf = bk if (ks == 3 and cin_pad % bk == 0) else 0
    kbd = bk if (ks == 3 and cout_pad % bk == 0) else 0
    _lib.check(
        L.mdm_pack_weight(_p(w32), _p(wf), _p(wd), cout, cin, ks, cin_pad, cout_pad, kbf, kbd,
                          F32 if dtype == torch.float32 else BF16, _stream()),
        "mdm_pack_weight",
    )
    _repacked(wf, wd)
    bp = None
    if bias is not None:
        bp = bias.detach().float()
        if cout_pad != cout:
            bp = torch.cat([bp, bp.new_zeros(cout_pad - cout)])
        bp = _c(bp)
    val = (wf, wd, bp, cin_pad, cout_pad, kbf, kbd)
    ent[key] = (ver, val)
    return val


def packed_s2_dgrad_weight(weight: torch.Tensor):
    """The stride-2 3x3 convolution's weight (Cout, Cin, 3, 3) in the layout of mdm_conv_s2_dgrad: bf16
    [(ph, pw, ci)][co / 64][tap j = 2 dh + dw][co % 64], where dx[2b + p] += dy[b + d] * W[kh(p, d)]:
    (p, d) -> kh = (0, 0) -> 1, (1, 0) -> 2, (1, 1) -> 0 (no tap for (0, 1)).  Cached per parameter version."""
    ent = _cache_slot(weight)
    ver = (weight._version, weight.data_ptr(), _pack_epoch)
    if "s2dgrad" in ent and ent["s2dgrad"][0] == ver:
        return ent["s2dgrad"][1]
    cout, cin = weight.shape[0], weight.shape[1]
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    old = ent.get("s2dgrad")
    packed = old[1] if old is not None and old[1].shape == (4 * cin, cout // 64, 4, 64) else \
        torch.empty((4 * cin, cout // 64, 4, 64), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.lib().mdm_s2dgrad_pack(_p(w), _p(packed), cout, cin, _stream()), "mdm_s2dgrad_pack")
    ent["s2dgrad"] = (ver, packed)
    return packed


_multi_tables = {}   # dtype -> (signature, device table, n, total blocks)


def repack_all(dtype: torch.dtype):
    """Refresh EVERY cached kernel-layout weight of ``dtype`` in one launch (C ABI mdm_pack_weights_multi) -- call right
    after an optimizer step that invalidated them.  Weights the tiled pack cannot express (channel padding, counts not
    a multiple of 32: the stem and the head) stay stale and are re-packed on their next use as before."""
    import numpy as np

    items = []
    for wref, ent in _wcache.values():
        w = wref()
        if w is None or dtype not in ent or not w.is_cuda:
            continue
        ver, val = ent[dtype]
        wf, wd, bp, cin_pad, cout_pad, kbf, kbd = val
        cout, cin = w.shape[0], w.shape[1]
        if cin_pad != cin or cout_pad != cout or cin % 32 or cout % 32 or w.dtype != torch.float32 or not w.is_contiguous():
            continue
        taps = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
        if taps not in (1, 9):
            continue
        items.append((w, ent, ver, val, cout, cin, taps, kbf, kbd))
    if not items:
        return
    sig = tuple((w.data_ptr(), val[0].data_ptr(), 0 if val[1] is None else val[1].data_ptr()) for w, _, _, val, *_ in items)
    tab = _multi_tables.get(dtype)
    if tab is None or tab[0] != sig:
        desc = np.zeros(len(items), dtype=[("w", "u8"), ("wf", "u8"), ("wd", "u8"), ("cout", "i4"), ("cin", "i4"),
                                           ("taps", "i4"), ("kbf", "i4"), ("kbd", "i4"), ("first", "i4")])
        first = 0
        for i, (w, _, _, val, cout, cin, taps, kbf, kbd) in enumerate(items):
            desc[i] = (w.data_ptr(), val[0].data_ptr(), 0 if val[1] is None else val[1].data_ptr(), cout, cin, taps, kbf, kbd, first)
            first += (cout // 32) * (cin // 32)
        assert desc.dtype.itemsize == 48
        dev_tab = torch.from_numpy(desc.view(np.uint8).copy()).to(items[0][0].device)
        tab = (sig, dev_tab, len(items), first)
        _multi_tables[dtype] = tab
    _lib.check(_lib.lib().mdm_pack_weights_multi(_p(tab[1]), tab[2], tab[3], F32 if dtype == torch.float32 else BF16, _stream()),
               "mdm_pack_weights_multi")
    for w, ent, ver, val, *_ in items:
        ent[dtype] = ((w._version, ver[1], w.data_ptr(), _pack_epoch), val)
        _repacked(val[0], val[1])


# --------------------------------------------------------------------------------------
# optional per-launch timing (bench.py roofline leg): HIP events on the launch stream around every GEMM-class launch
# (with its algorithmic FLOPs) and every large streaming launch (with its algorithmic HBM bytes)
# --------------------------------------------------------------------------------------
_prof = None
_prof_shapes = False


def profile_begin(shapes: bool = False):
    """Start recording.  ``shapes``: key the GEMM table by problem shape as well (tools/)."""
    global _prof, _prof_shapes
    _prof, _prof_shapes = [], shapes


def _prof_wrap(name, work, fn, kind="mfma", executed=None):
    """``work``: algorithmic FLOPs (bytes for kind="hbm") the launch is credited with; ``executed``: the FLOPs it actually
    issues when that differs (the sub-pixel resampling convolutions are credited with the dense 3x3 count of the layer
    they replace and execute 16 / 36 of it)"""
    if _prof is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    if kind == "mfma":
        real = _lib.lib().mdm_last_gemm_kernel()   # the kernel that actually ran (name as rocprofv3 prints it)
        if real:
            name = real.decode() + (name[name.index(" M="):] if " M=" in name else "")
    _prof.append((kind, name, work, e0, e1, work if executed is None else executed))
    return r


def profile_end(peak_tflops, peak_gbs=8000.0):
    """-> the ``roofline`` object of bench.py.  The named kernel is the GEMM-class kernel with the LARGEST TOTAL TIME in
    the step; ``gemm_weighted`` is the FLOP-weighted figure over every GEMM-class launch; ``hbm_kernels`` holds the
    streaming kernels as algorithmic GB/s against the HBM peak."""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    agg, hbm = {}, {}
    for kind, name, work, e0, e1, executed in rec:
        a = (hbm if kind == "hbm" else agg).setdefault(name, [0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += work
        a[2] += e0.elapsed_time(e1) * 1e-3
        a[3] += executed
    if not agg:
        return None
    table = {k: {"launches": v[0], "alg_tflop": round(v[1] / 1e12, 3), "time_ms": round(v[2] * 1e3, 3),
                 "tflops": round(v[1] / v[2] / 1e12, 1)} for k, v in agg.items()}
    for k, v in agg.items():
        if abs(v[3] - v[1]) > 1e-6 * v[1]:
            # credited with more FLOPs than it issues: "tflops" is algorithmic credit (it may exceed the MFMA peak),
            # "executed_tflops" is what the matrix pipe does
            table[k]["executed_tflops"] = round(v[3] / v[2] / 1e12, 1)
            table[k]["tflops_is"] = "credit for the dense 3x3 layer this sub-pixel kernel replaces (%.2fx the FLOPs it executes)" % (v[1] / v[3])
    dom = max(agg, key=lambda k: agg[k][2])
    n, fl, t = agg[dom][:3]
    ach = fl / t / 1e12
    tot_f, tot_t = sum(v[1] for v in agg.values()), sum(v[2] for v in agg.values())
    return {
        "bound": "mfma", "achieved": round(ach, 1), "peak": peak_tflops, "unit": "TFLOP/s", "frac": round(ach / peak_tflops, 4),
        "traffic": None, "kernel": dom, "dominant_by": "largest total time among the GEMM-class kernels of one step",
        "launches_per_step": n, "avg_launch_ms": round(t / n * 1e3, 4),
        "alg_gflop_per_launch": round(fl / n / 1e9, 2),
        "gemm_weighted": {"alg_tflop": round(tot_f / 1e12, 2), "time_ms": round(tot_t * 1e3, 2),
                          "tflops": round(tot_f / tot_t / 1e12, 1), "frac": round(tot_f / tot_t / 1e12 / peak_tflops, 4)},
        "all_gemm_kernels": table,
        "hbm_kernels": {k: {"launches": v[0], "alg_gb": round(v[1] / 1e9, 3), "time_ms": round(v[2] * 1e3, 3),
                            "gb_per_s": round(v[1] / v[2] / 1e9, 1), "frac_of_peak": round(v[1] / v[2] / 1e9 / peak_gbs, 4)}
                        for k, v in hbm.items()},
    }


# --------------------------------------------------------------------------------------
# raw launches
# --------------------------------------------------------------------------------------
_conv_plans = {}   # (M, Cout, K, dtype) -> (splits, workspace bytes) of mdm_conv_fwd_plan


def _conv_plan(M, Cout, K, dt):
    key = (M, Cout, K, dt)
    ent = _conv_plans.get(key)
    if ent is None:
        sp, wsb = ctypes.c_int(1), ctypes.c_size_t(0)
        _lib.check(_lib.lib().mdm_conv_fwd_plan(M, Cout, K, dt, ctypes.byref(sp), ctypes.byref(wsb)), "mdm_conv_fwd_plan")
        ent = _conv_plans[key] = (sp.value, wsb.value)
    return ent


def _repacked(*packs):
    """note that these kernel-layout weights were (re-)written: planes made from them are stale"""
    for t in packs:
        if t is not None:
            t._mdm_serial = getattr(t, "_mdm_serial", 0) + 1


def _weight_planes(w: torch.Tensor):
    """The packed fp32 weight ``w`` as bf16 hi / lo planes (C ABI mdm_split_weight_planes), cached on the packed tensor
    until it is re-packed: under MDM_F32_SPLIT the weight operand's split leaves the k-loop (97.8 -> 88.9 ms per
    iteration of the 64x64 sampler at batch 64; the products are bit-identical)."""
    ent, serial = getattr(w, "_mdm_planes", None), getattr(w, "_mdm_serial", 0)
    if ent is not None and ent[0] == serial:
        return ent[1]
    planes = torch.empty_like(w)
    _lib.check(_lib.lib().mdm_split_weight_planes(_p(w), _p(planes), w.numel(), _stream()), "mdm_split_weight_planes")
    w._mdm_planes = (serial, planes)
    return planes


def _conv_launch(x, w, bias, res, aux, y, ypre, N, H, W, Cin, Ho, Wo, Cout, ks, stride, transposed, act, kblk=0):
    # problems too small to fill the chip with output tiles (sampling at batch 1-4) run split over the reduction
    splits, wsb = _conv_plan(N * Ho * Wo, Cout, ks * ks * Cin, _dt(x)) if (stride == 1 and not transposed) else (1, 0)
    ws = _f32_ws(wsb, x.device) if splits > 1 else None
    dt = _dt_mm(x)
    if dt == F32_SPLIT and (ks * ks * Cin) % 8 == 0 and w.numel() % 8 == 0 and _weight_planes_on:
        w, dt = _weight_planes(w), F32_SPLIT_W

    def go():
        _lib.check(
            _lib.lib().mdm_conv_fwd_ws(_p(x), _p(w), _p(bias), _p(res), _p(aux), _p(y), _p(ypre), N, H, W, Cin, Ho, Wo, Cout,
                                       ks, stride, transposed, act, kblk, dt, _p(ws), wsb, _stream()),
            "mdm_conv_fwd",
        )

    if _prof is None:
        return go()
    code = _lib.lib().mdm_conv_fwd_tile(N * Ho * Wo, Cout, _dt(x))
    mode = "1x1" if ks == 1 else ("3x3_T2" if transposed else "3x3")
    name = "conv_gemm_kernel<%s,%dx%d,%s>" % ("f32" if x.dtype == torch.float32 else "bf16", code // 1000, code % 1000, mode)
    flops = 2.0 * N * Ho * Wo * Cout * ks * ks * Cin / (4 if transposed else 1)
    if _prof_shapes:
        name += " M=%d N=%d K=%d" % (N * Ho * Wo, Cout, ks * ks * Cin)
    return _prof_wrap(name, flops, go)


def _wgrad_launch(x, dy, N, H, W, Cin, Ho, Wo, Cout, ks, stride, out=None, dbias=None):
    """dW (Cout, Cin, ks, ks) fp32; with ``out`` (a gradient-arena slot) the result is ADDED into it.  ``dbias`` (fp32
    [Cout]) receives the bias gradient from the same launch, with the same overwrite / accumulate semantics."""
    L = _lib.lib()
    splits = ctypes.c_int(0)
    wsb = ctypes.c_size_t(0)
    M, K = N * Ho * Wo, ks * ks * Cin
    _lib.check(L.mdm_conv_wgrad_plan(M, Cout, K, _dt(x), ctypes.byref(splits), ctypes.byref(wsb)), "mdm_conv_wgrad_plan")
    ws = _f32_ws(wsb.value, x.device)
    dw = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=x.device) if out is None else out

    def go():
        _lib.check(L.mdm_conv_wgrad(_p(x), _p(dy), 0 if dbias is None else 1, _p(ws), N, H, W, Cin, Ho, Wo, Cout, ks, stride,
                                    _dt(x), _stream()),
                   "mdm_conv_wgrad")

    if _prof is None:
        go()
    else:
        te = L.mdm_conv_wgrad_tile(M, Cout, K, _dt(x))
        kn = "conv_wgrad_kernel" if x.dtype == torch.float32 else "conv_wgrad_tr_kernel"
        name = "%s<%s,%dx%d,%s>" % (kn, "f32" if x.dtype == torch.float32 else "bf16", te, te, "1x1" if ks == 1 else "3x3")
        if _prof_shapes:
            name += " M=%d N=%d K=%d" % (M, Cout, K)
        _prof_wrap(name, 2.0 * M * Cout * K, go)
    _lib.check(L.mdm_conv_wgrad_reduce(_p(ws), _p(dw), _p(dbias), _p(dy), M, Cin, Cout, ks, 0 if out is None else 1, _dt(x),
                                       _stream()), "mdm_conv_wgrad_reduce")
    return dw


def _colsum_launch(x2d, M, C, out=None):
    L = _lib.lib()
    nb = ctypes.c_int(0)
    wsb = ctypes.c_size_t(0)
    _lib.check(L.mdm_colsum_plan(M, C, ctypes.byref(nb), ctypes.byref(wsb)), "mdm_colsum_plan")
    ws = _f32_ws(wsb.value, x2d.device)
    acc = 0 if out is None else 1
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x2d.device)
    _lib.check(L.mdm_colsum(_p(x2d), _p(out), _p(ws), M, C, acc, _dt(x2d), _stream()), "mdm_colsum")
    return out


def _geom(x, ks, stride):
    """x: [N,H,W,C] or [R,C] -> (N,H,W,Ho,Wo)"""
    if x.dim() == 2:
        return x.shape[0], 1, 1, 1, 1
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    if ks == 1:
        return N, H, W, H, W
    return N, H, W, (H - 1) // stride + 1, (W - 1) // stride + 1


def _out_shape(x, Ho, Wo, C):
    return (x.shape[0], C) if x.dim() == 2 else (x.shape[0], Ho, Wo, C)


def _conv_forward(x, weight, bias, residual, stride):
    """the forward launch of y = conv(x, weight) + bias (+ residual) on contiguous operands -> (y, kernel size)"""
    ks = weight.shape[2] if weight.dim() == 4 else 1
    wf, wd, bp, cin_pad, cout_pad, kbf, kbd = packed_weight(weight, bias, x.dtype)
    if x.shape[-1] != cin_pad:
        raise _lib.MdmHipError("conv input has %d channels, packed weight expects %d" % (x.shape[-1], cin_pad))
    N, H, W, Ho, Wo = _geom(x, ks, stride)
    y = torch.empty(_out_shape(x, Ho, Wo, cout_pad), dtype=x.dtype, device=x.device)
    _conv_launch(x, wf, bp, residual, None, y, None, N, H, W, cin_pad, Ho, Wo, cout_pad, ks, stride, 0, 0, kbf)
    return y, ks


class ConvFn(torch.autograd.Function):
    """y = conv(x, weight) + bias (+ residual).  3x3 (stride 1/2, pad 1), 1x1, or linear ([R, Cin])."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, tap=False):
        """``tap``: also return x itself as a second output -- for a consumer that reads the same tensor (the skip
        connection of a down-sampling block): its gradient comes back to ``backward`` and is added in the input
        gradient's epilogue instead of by autograd's accumulation pass"""
        _require_gpu(x)
        x = _c(x)
        residual = _c(residual)
        y, ks = _conv_forward(x, weight, bias, residual, stride)
        ctx.save_for_backward(x, weight, bias)
        ctx.stride, ctx.ks = stride, ks
        ctx.has_res = residual is not None
        if tap:
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dtap=None):
        x, weight, bias = ctx.saved_tensors
        if dy is None:
            raise _lib.MdmHipError("conv(tap=True): the convolution's own output received no gradient")
        return _conv_backward(ctx, x, weight, bias, dy, dtap) + (None, None)


def _conv_backward(ctx, x, weight, bias, dy, dtap=None):
    """input / weight / bias / residual gradients of y = conv(x, weight) + bias (+ residual); ``ctx`` carries ks, stride,
    has_res and needs_input_grad[0:4] = (x, weight, bias, residual); ``dtap``: a second gradient of x, added to dx.
    -> (dx, dw, db, dres)"""
    dy = _c(dy)
    dtap = _c(dtap)
    ks, stride = ctx.ks, ctx.stride
    wf, wd, bp, cin_pad, cout_pad, kbf, kbd = packed_weight(weight, bias, x.dtype)
    cout, cin = weight.shape[0], weight.shape[1]
    N, H, W, Ho, Wo = _geom(x, ks, stride)
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        if wd is None:
            raise _lib.MdmHipError("input gradient requested for a channel-padded convolution")
        dx = torch.empty_like(x)
        if ks == 3 and stride == 2 and x.dtype == torch.bfloat16 and cout_pad == cout and cout % 64 == 0 and cin % 128 == 0 \
                and H % 2 == 0 and W % 2 == 0:
            # sub-pixel form: a 2x2 correlation over dy per phase of dx, stored pixel-shuffled (mdm_conv_s2_dgrad)
            wsel = packed_s2_dgrad_weight(weight)
            _prof_wrap("conv_gemm_bl_kernel<sel4> (3x3 stride-2 input gradient) M=%d N=%d K=%d" % (N * Ho * Wo, 4 * cin, 4 * cout),
                       2.0 * N * Ho * Wo * cout * 9 * cin, lambda: _lib.check(
                _lib.lib().mdm_conv_s2_dgrad_res(_p(dy), _p(wsel), _p(dtap), _p(dx), N, Ho, Wo, cout, cin, BF16, _stream()),
                "mdm_conv_s2_dgrad_res"), executed=2.0 * N * Ho * Wo * (4 * cin) * (4 * cout))
            dtap = None
        elif ks == 3 and stride == 2:
            _conv_launch(dy, wd, None, None, None, dx, None, N, Ho, Wo, cout_pad, H, W, cin, 3, 1, 1, 0, kbd)
        else:
            _conv_launch(dy, wd, None, None, None, dx, None, N, Ho, Wo, cout_pad, H, W, cin, ks, 1, 0, 0, kbd)
        if dtap is not None:   # shapes the sub-pixel kernel does not take
            dx = dx + dtap
    elif dtap is not None:
        dx = dtap
    padded = cout_pad != cout or cin_pad != cin
    want_b = bias is not None and ctx.needs_input_grad[2]
    if ctx.needs_input_grad[1]:
        slot = None if padded else _slot(weight)
        bslot = _slot(bias) if (slot is not None and want_b) else None
        if slot is not None:
            # weight (and, when it also lives in the arena, bias) gradient from one launch
            _wgrad_into_sink(x, dy, weight, bias, slot, bslot, N, H, W, cin_pad, Ho, Wo, cout_pad, ks, stride)
            if bslot is not None:
                want_b = False
        else:
            dbt = torch.empty(cout_pad, dtype=torch.float32, device=x.device) if want_b else None
            dwp = _wgrad_launch(x, dy, N, H, W, cin_pad, Ho, Wo, cout_pad, ks, stride, dbias=dbt)
            if padded:
                dwp = dwp[:cout, :cin].contiguous()
            dw = dwp.view(weight.shape)
            if want_b:
                db = dbt[:cout]
                want_b = False
    if want_b:
        slot = None if cout_pad != cout else _slot(bias)
        if slot is not None:
            _colsum_launch(dy, N * Ho * Wo, cout_pad, out=slot)
            _grad_sink.ready(bias)
        else:
            db = _colsum_launch(dy, N * Ho * Wo, cout_pad)[:cout]
    dres = dy if (ctx.has_res and ctx.needs_input_grad[3]) else None
    return dx, dw, db, dres


def conv(x, weight, bias=None, residual=None, stride=1):
    return ConvFn.apply(x, weight, bias, residual, stride)


def conv_tap(x, weight, bias=None, stride=1):
    """(conv(x), x'): x' is x for a second consumer whose gradient is then added inside the convolution's input-gradient
    kernel (mdm_conv_s2_dgrad_res for the stride-2 3x3 case) rather than by a separate accumulation pass"""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return ConvFn.apply(x, weight, bias, None, stride), x
    return ConvFn.apply(x, weight, bias, None, stride, True)


# --------------------------------------------------------------------------------------
# the stem (conv_in) as one node whose backward reaches the model's input
# --------------------------------------------------------------------------------------
STEM_DGRAD_MAX_CIN = 8


def conv3x3_stem_dgrad(dy, weight, bias=None):
    """dx [N, Cin, H, W] fp32 NCHW of y = conv3x3(pad(x), weight), stride 1, from dy [N, H, W, Cout_pad] of the compute
    dtype (C ABI mdm_conv3x3_stem_dgrad): reads the FORWARD pack of ``weight``, 1 <= Cin <= 8."""
    _require_gpu(dy)
    dy = _c(dy)
    if weight.dim() != 4 or weight.shape[2] != 3 or weight.shape[3] != 3:
        raise _lib.MdmHipError("conv3x3_stem_dgrad: a 3x3 convolution weight is expected")
    cin = weight.shape[1]
    if not 1 <= cin <= STEM_DGRAD_MAX_CIN:
        raise _lib.MdmHipError("input gradient of a channel-padded stem convolution is implemented for at most %d input "
                               "channels (got %d)" % (STEM_DGRAD_MAX_CIN, cin))
    wf, _, _, cin_pad, cout_pad, kbf, _ = packed_weight(weight, bias, dy.dtype)
    if dy.dim() != 4 or dy.shape[-1] != cout_pad or kbf:
        raise _lib.MdmHipError("conv3x3_stem_dgrad: dy %s does not match the packed weight (%d channels)"
                               % (tuple(dy.shape), cout_pad))
    N, H, W = dy.shape[0], dy.shape[1], dy.shape[2]
    dx = torch.empty((N, cin, H, W), dtype=torch.float32, device=dy.device)

    def go():
        _lib.check(_lib.lib().mdm_conv3x3_stem_dgrad(_p(dy), _p(wf), _p(dx), N, H, W, cout_pad, cin, _dt(dy), _stream()),
                   "mdm_conv3x3_stem_dgrad")

    if _prof is None:
        go()
    else:
        name = "stem_dgrad_kernel<%s,%d>" % ("f32" if dy.dtype == torch.float32 else "bf16", cin)
        if _prof_shapes:
            name += " M=%d N=%d K=%d" % (N * H * W, cin, 9 * cout_pad)
        _prof_wrap(name, float(dy.numel() * dy.element_size() + dx.numel() * 4), go, kind="hbm")
    return dx


class StemConvFn(torch.autograd.Function):
    """y = conv3x3(to_nhwc(x), weight) + bias from fp32 NCHW x: the launches of ToNHWCFn -> ConvFn forward (bit-identical
    output), their weight / bias gradients backward (_conv_backward: gradient sink and side stream included), and the
    input gradient from mdm_conv3x3_stem_dgrad, straight into fp32 NCHW."""

    @staticmethod
    def forward(ctx, x, weight, bias, dtype):
        _require_gpu(x)
        x = _c(x.float())
        N, C, H, W = x.shape
        epv = 4 if dtype == torch.float32 else 8
        xh = torch.empty((N, H, W, _round_up(C, epv)), dtype=dtype, device=x.device)
        _lib.check(_lib.lib().mdm_nchw_to_nhwc(_p(x), _p(xh), N, C, H, W, xh.shape[-1], _dt(xh), _stream()), "mdm_nchw_to_nhwc")
        y, _ = _conv_forward(xh, weight, bias, None, 1)
        ctx.save_for_backward(xh, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        xh, weight, bias = ctx.saved_tensors
        nig = ctx.needs_input_grad
        dy = _c(dy)
        dx = conv3x3_stem_dgrad(dy, weight, bias) if nig[0] else None
        _, dw, db, _ = _conv_backward(_ConvNeeds(3, 1, False, (False, nig[1], nig[2], False)), xh, weight, bias, dy)
        return dx, dw, db, None


def stem_conv(x_nchw, weight, bias=None, dtype=torch.float32):
    """``conv(to_nhwc(x_nchw, dtype), weight, bias)`` for the 3x3 stride-1 stem, differentiable in ``x_nchw``.  A stem whose
    input channels are NOT padded in ``dtype`` and exceed the kernel's limit takes the generic nodes (they have a dgrad
    pack); a padded one beyond 8 channels raises."""
    if weight.dim() != 4 or weight.shape[2] != 3:
        raise _lib.MdmHipError("stem_conv: a 3x3 convolution weight is expected")
    cin = weight.shape[1]
    if x_nchw.dim() != 4 or x_nchw.shape[1] != cin:
        raise _lib.MdmHipError("stem_conv: input %s vs weight %s" % (tuple(x_nchw.shape), tuple(weight.shape)))
    if cin > STEM_DGRAD_MAX_CIN:
        if cin % (4 if dtype == torch.float32 else 8) == 0:
            return conv(to_nhwc(x_nchw, dtype), weight, bias)
        raise _lib.MdmHipError("input gradient of a channel-padded stem convolution is implemented for at most %d input "
                               "channels (got %d)" % (STEM_DGRAD_MAX_CIN, cin))
    return StemConvFn.apply(x_nchw, weight, bias, dtype)


# --------------------------------------------------------------------------------------
# upsample2x (nearest) -> conv3x3 in its sub-pixel form
# --------------------------------------------------------------------------------------
def packed_upconv_weights(weight: torch.Tensor, bias):
    """(w_ph, w_t, bias4) of mdm_conv_up_fwd / mdm_conv_up_dgrad for a (Cout, Cin, 3, 3) weight; cached per version."""
    ent = _cache_slot(weight)
    ver = (weight._version, None if bias is None else bias._version, weight.data_ptr(), _pack_epoch)
    if "upconv" in ent and ent["upconv"][0] == ver:
        return ent["upconv"][1]
    cout, cin = weight.shape[0], weight.shape[1]
    prev = ent["upconv"][1] if "upconv" in ent else None
    if prev is not None and prev[0].device == weight.device:
        w_ph, w_t = prev[0], prev[1]
    else:
        w_ph = torch.empty(4 * cout * 4 * cin, dtype=torch.bfloat16, device=weight.device)
        w_t = torch.empty(cin * 16 * cout, dtype=torch.bfloat16, device=weight.device)
    _lib.check(_lib.lib().mdm_upconv_pack(_p(_c(weight.detach().float())), _p(w_ph), _p(w_t), cout, cin, _stream()), "mdm_upconv_pack")
    bias4 = _c(bias.detach().float().repeat(4)) if bias is not None else None
    val = (w_ph, w_t, bias4)
    ent["upconv"] = (ver, val)
    return val


def upsample_conv_supported(x, weight):
    """bf16, channel counts the 256-square weight-gradient tiles divide, power-of-two images (the sampling / fp32 /
    odd-size cases take upsample2x + conv)"""
    return x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and weight.dim() == 4 and weight.shape[2] == 3 and \
        weight.shape[0] % 256 == 0 and weight.shape[1] % 256 == 0 and x.shape[-1] == weight.shape[1] and \
        (x.shape[1] & (x.shape[1] - 1)) == 0 and (x.shape[2] & (x.shape[2] - 1)) == 0


class UpsampleConvFn(torch.autograd.Function):
    """y = conv3x3(upsample2x_nearest(x), weight) + bias (reference unet.py:567-569) without the upsampled tensor: per
    output phase a 2x2 correlation over the low-resolution x with the 3x3 taps that coincide summed -- 16 weight blocks
    instead of 36 in all three directions (C ABI mdm_conv_up_fwd / _dgrad / mdm_conv_wgrad_blocked + mdm_upconv_wfold)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu(x)
        x = _c(x)
        N, H, W, cin = x.shape
        cout = weight.shape[0]
        w_ph, _, bias4 = packed_upconv_weights(weight, bias)
        y = torch.empty((N, 2 * H, 2 * W, cout), dtype=x.dtype, device=x.device)
        _prof_wrap("conv_gemm_bl_kernel<sel4> (upsample2x + 3x3) M=%d N=%d K=%d" % (N * H * W, 4 * cout, 4 * cin),
                   2.0 * N * 4 * H * W * cout * 9 * cin, lambda: _lib.check(
            _lib.lib().mdm_conv_up_fwd(_p(x), _p(w_ph), _p(bias4), _p(y), N, H, W, cin, cout, BF16, _stream()), "mdm_conv_up_fwd"),
                   executed=2.0 * N * H * W * (4 * cout) * (4 * cin))
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        dy = _c(dy)
        N, H, W, cin = x.shape
        cout = weight.shape[0]
        L = _lib.lib()
        _, w_t, _ = packed_upconv_weights(weight, bias)
        dyb = torch.empty((N, H, W, 4 * cout), dtype=dy.dtype, device=dy.device)
        _lib.check(L.mdm_space_to_depth2x(_p(dy), _p(dyb), N, H, W, cout, BF16, _stream()), "mdm_space_to_depth2x")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _prof_wrap("conv_gemm_bl_kernel<sel4> (upsample2x + 3x3 input gradient) M=%d N=%d K=%d" % (N * H * W, cin, 16 * cout),
                       2.0 * N * 4 * H * W * cout * 9 * cin, lambda: _lib.check(
                L.mdm_conv_up_dgrad(_p(dyb), _p(w_t), _p(dx), N, H, W, cout, cin, BF16, _stream()), "mdm_conv_up_dgrad"),
                           executed=2.0 * N * H * W * cin * (16 * cout))
        if ctx.needs_input_grad[1]:
            want_b = bias is not None and ctx.needs_input_grad[2]
            slot = _slot(weight)
            bslot = _slot(bias) if (slot is not None and want_b) else None
            sunk = slot is not None and (bslot is not None or not want_b)
            M, K = N * H * W, 9 * cin
            splits, wsb = ctypes.c_int(0), ctypes.c_size_t(0)
            _lib.check(L.mdm_conv_wgrad_plan(M, 4 * cout, K, BF16, ctypes.byref(splits), ctypes.byref(wsb)), "mdm_conv_wgrad_plan")

            def go():
                ws = _f32_ws(wsb.value, x.device)
                dwb = torch.empty((4 * cout, cin, 3, 3), dtype=torch.float32, device=x.device)
                db4 = torch.empty(4 * cout, dtype=torch.float32, device=x.device) if want_b else None
                _prof_wrap("conv_wgrad_bl_kernel<1, 1> (upsample2x + 3x3, 16 of 36 blocks) M=%d N=%d K=%d" % (M, 4 * cout, K),
                           2.0 * 4 * M * cout * K, lambda: _lib.check(
                    L.mdm_conv_wgrad_blocked(_p(x), _p(dyb), 1 if want_b else 0, _p(ws), N, H, W, cin, cout, BF16, _stream()),
                    "mdm_conv_wgrad_blocked"), executed=2.0 * 4 * M * cout * K * 16.0 / 36.0)
                _lib.check(L.mdm_conv_wgrad_reduce(_p(ws), _p(dwb), _p(db4), _p(dyb), M, cin, 4 * cout, 3, 0, BF16, _stream()),
                           "mdm_conv_wgrad_reduce")
                dwo = slot if sunk else torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                dbo = (bslot if sunk else torch.empty(cout, dtype=torch.float32, device=x.device)) if want_b else None
                _lib.check(L.mdm_upconv_wfold(_p(dwb), _p(dwo), _p(db4), _p(dbo), cout, cin, 1 if sunk else 0, _stream()), "mdm_upconv_wfold")
                if sunk:
                    _grad_sink.ready(weight)
                    if want_b:
                        _grad_sink.ready(bias)
                return dwo, dbo

            if sunk:
                _off_critical_path((x, dyb), go)
            else:
                dw, db = go()
        return dx, dw, db


def upsample_conv(x, weight, bias=None):
    """conv3x3(upsample2x(x)): the sub-pixel form where it applies, else the two separate ops"""
    if upsample_conv_supported(x, weight):
        return UpsampleConvFn.apply(x, weight, bias)
    return ConvFn.apply(upsample2x(x), weight, bias, None, 1)


def linear(x, weight, bias=None, residual=None):
    shp = x.shape
    y = ConvFn.apply(x.reshape(-1, shp[-1]), weight, bias, None if residual is None else residual.reshape(-1, weight.shape[0]), 1)
    return y.reshape(*shp[:-1], weight.shape[0])


class FFNFn(torch.autograd.Function):
    """y = W2 gelu(W1 x + b1) + b2 + residual  (1x1 convs; unet.py:266-272, 311-312)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, keep):
        _require_gpu(x)
        x, residual = _c(x), _c(residual)
        wf1, _, bp1, c_in, c_hid, _, _ = packed_weight(w1, b1, x.dtype)
        wf2, _, bp2, _, c_out, _, _ = packed_weight(w2, b2, x.dtype)
        N, H, W, _, _ = _geom(x, 1, 1)
        # what backward needs of the pre-activation: itself for fp32 tensors; for bf16 tensors one byte per element, the
        # code of gelu'(pre) (include/mdm_hip.h, MDM_ACT_GELU) -- half the bytes of this store-bound launch's second output
        byte_code = x.dtype == torch.bfloat16 and _lib.lib().mdm_dev_ffn_aux_bytes() == 1
        pre = torch.empty(_out_shape(x, H, W, c_hid), dtype=torch.uint8 if byte_code else x.dtype, device=x.device) if keep else None
        a = torch.empty(_out_shape(x, H, W, c_hid), dtype=x.dtype, device=x.device)
        _conv_launch(x, wf1, bp1, None, None, a, pre, N, H, W, c_in, H, W, c_hid, 1, 1, 0, 1)
        y = torch.empty(_out_shape(x, H, W, c_out), dtype=x.dtype, device=x.device)
        _conv_launch(a, wf2, bp2, residual, None, y, None, N, H, W, c_hid, H, W, c_out, 1, 1, 0, 0)
        ctx.save_for_backward(x, w1, b1, w2, b2, pre, a)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, b1, w2, b2, pre, a = ctx.saved_tensors
        dy = _c(dy)
        _, wd1, _, c_in, c_hid, _, _ = packed_weight(w1, b1, x.dtype)
        _, wd2, _, _, c_out, _, _ = packed_weight(w2, b2, x.dtype)
        N, H, W, _, _ = _geom(x, 1, 1)
        M = N * H * W
        dpre = torch.empty_like(a)
        _conv_launch(dy, wd2, None, None, pre, dpre, None, N, H, W, c_out, H, W, c_hid, 1, 1, 0, 2)
        def wb_grads(xin, g, w, b, cin_, cout_):
            """(dW, db) of a 1x1 conv from ONE wgrad launch; None entries went into the gradient arena"""
            sw, sb = _slot(w), _slot(b)
            if sw is not None and sb is not None:
                _wgrad_into_sink(xin, g, w, b, sw, sb, N, H, W, cin_, H, W, cout_, 1, 1)
                return None, None
            dbt = torch.empty(cout_, dtype=torch.float32, device=xin.device)
            return _wgrad_launch(xin, g, N, H, W, cin_, H, W, cout_, 1, 1, dbias=dbt).view(w.shape), dbt

        # a frozen layer (neither the weight nor its bias wants a gradient) launches no weight-gradient GEMM
        dw1 = db1 = dw2 = db2 = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            dw2, db2 = wb_grads(a, dy, w2, b2, c_hid, c_out)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _conv_launch(dpre, wd1, None, None, None, dx, None, N, H, W, c_hid, H, W, c_in, 1, 1, 0, 0)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw1, db1 = wb_grads(x, dpre, w1, b1, c_in, c_hid)
        dres = dy if (ctx.has_res and ctx.needs_input_grad[5]) else None
        return dx, dw1, db1, dw2, db2, dres, None


def ffn(x, w1, b1, w2, b2, residual):
    # autograd.Function.forward runs with grad mode off, so the "will there be a backward" decision is taken here
    return FFNFn.apply(x, w1, b1, w2, b2, residual, torch.is_grad_enabled())


# --------------------------------------------------------------------------------------
# low-rank adapters (mdm_hip/lora.py): y = W x + b + s B (A x) beside a frozen W, b
# --------------------------------------------------------------------------------------
_adapter_epoch = 0   # moves whenever adapters are attached / detached / merged / unmerged: captured graphs are keyed on it


def adapter_epoch() -> int:
    return _adapter_epoch


def bump_adapter_epoch():
    global _adapter_epoch
    _adapter_epoch += 1


def _lora_mats(big, small, what):
    """checks shared by the three kernels: ``big`` [M, C] and ``small`` [*, *] contiguous GPU tensors of one dtype"""
    _require_gpu(big)
    _require_gpu(small)
    if big.dtype != small.dtype or not big.is_contiguous() or not small.is_contiguous():
        raise _lib.MdmHipError("%s: operands must be contiguous tensors of one dtype (%s, %s)" % (what, big.dtype, small.dtype))


def lora_down(x, a):
    """t [M, r] = x [M, C] a^T  (a [r, C], both of x's dtype)"""
    _lora_mats(x, a, "lora_down")
    M, C = x.shape
    r = a.shape[0]
    if a.shape[1] != C:
        raise _lib.MdmHipError("lora_down: x has %d columns, a has %d" % (C, a.shape[1]))
    t = torch.empty((M, r), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().mdm_lora_down(_p(x), _p(a), _p(t), M, C, r, _dt(x), _stream()), "mdm_lora_down")
    return t


def lora_up_add(y, t, b, s, accumulate=True):
    """y [M, N] (+)= s t [M, r] b^T in place  (b [N, r]); ``accumulate=False`` overwrites y without reading it"""
    _lora_mats(y, b, "lora_up_add")
    _lora_mats(y, t, "lora_up_add")
    M, N = y.shape
    r = t.shape[1]
    if t.shape[0] != M or tuple(b.shape) != (N, r):
        raise _lib.MdmHipError("lora_up_add: y %s, t %s, b %s do not fit" % (tuple(y.shape), tuple(t.shape), tuple(b.shape)))
    _lib.check(_lib.lib().mdm_lora_up_add(_p(y), _p(t), _p(b), M, N, r, float(s), 1 if accumulate else 0, _dt(y), _stream()),
               "mdm_lora_up_add")
    return y


def lora_wgrad(p, q, s, out=None):
    """d [r, C] fp32 = s p [M, r]^T q [M, C]; with ``out`` the result is ADDED into it.  Deterministic (no atomics)."""
    _lora_mats(q, p, "lora_wgrad")
    M, C = q.shape
    r = p.shape[1]
    if p.shape[0] != M:
        raise _lib.MdmHipError("lora_wgrad: p has %d rows, q has %d" % (p.shape[0], M))
    L = _lib.lib()
    splits, wsb = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(L.mdm_lora_wgrad_plan(M, r, C, _dt(q), ctypes.byref(splits), ctypes.byref(wsb)), "mdm_lora_wgrad_plan")
    ws = _f32_ws(wsb.value, q.device)
    d = torch.empty((r, C), dtype=torch.float32, device=q.device) if out is None else out
    if d.dtype != torch.float32 or not d.is_contiguous() or tuple(d.shape) != (r, C):
        raise _lib.MdmHipError("lora_wgrad: out must be a contiguous fp32 [%d, %d] tensor" % (r, C))
    _lib.check(L.mdm_lora_wgrad(_p(p), _p(q), _p(d), _p(ws), M, r, C, float(s), 0 if out is None else 1, _dt(q), _stream()),
               "mdm_lora_wgrad")
    return d


def _lora_packs(A, B, dtype):
    """(A [r, C], A^T [C, r], B [N, r], B^T [r, N]) of the activation dtype for the fp32 adapter parameters; cached per
    parameter version and re-made INTO THE SAME BUFFERS (a captured graph holds their addresses)"""
    ent = _cache_slot(A)
    key = ("lora", dtype)
    ver = (A._version, B._version, A.data_ptr(), B.data_ptr(), _pack_epoch)
    if key in ent and ent[key][0] == ver:
        return ent[key][1]
    _require_gpu(A)
    _require_gpu(B)
    prev = ent[key][1] if key in ent else None
    if prev is None or prev[0].shape != A.shape or prev[2].shape != B.shape or prev[0].device != A.device:
        r, C = A.shape
        N = B.shape[0]
        prev = tuple(torch.empty(shp, dtype=dtype, device=A.device) for shp in ((r, C), (C, r), (N, r), (r, N)))
    with torch.no_grad():
        prev[0].copy_(A)
        prev[1].copy_(A.t())
        prev[2].copy_(B)
        prev[3].copy_(B.t())
    ent[key] = (ver, prev)
    return prev


class LoraFn(torch.autograd.Function):
    """y += s (x A^T) B^T, IN PLACE on y = the base projection's fresh output (its producer, ConvFn, saves its inputs
    only).  x [..., C] is that projection's input; A [r, C], B [N, r] are the fp32 adapter parameters."""

    @staticmethod
    def forward(ctx, y, x, A, B, s):
        _require_gpu(x)
        _require_gpu(y)
        r, C = A.shape
        N = B.shape[0]
        if not y.is_contiguous() or y.dtype != x.dtype or y.shape[-1] != N or x.shape[-1] != C or B.shape[1] != r:
            raise _lib.MdmHipError("lora: y %s / x %s / A %s / B %s do not fit (y must be contiguous, of x's dtype)"
                                   % (tuple(y.shape), tuple(x.shape), tuple(A.shape), tuple(B.shape)))
        x2 = _c(x).reshape(-1, C)
        M = x2.shape[0]
        a_c, _, b_c, _ = _lora_packs(A, B, x.dtype)
        t = lora_down(x2, a_c)
        lora_up_add(y.view(M, N), t, b_c, s)
        ctx.mark_dirty(y)
        ctx.save_for_backward(x2, t, A, B)
        ctx.s, ctx.xshape = s, x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, t, A, B = ctx.saved_tensors
        M, C = x2.shape
        N = B.shape[0]
        dy2 = _c(dy).reshape(M, N)
        _, at_c, _, bt_c = _lora_packs(A, B, x2.dtype)
        dx = dA = dB = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            g = lora_down(dy2, bt_c)                                    # G = dY B
            if ctx.needs_input_grad[1]:                                 # the low-rank part of dX = s G A
                dx = lora_up_add(torch.empty_like(x2), g, at_c, ctx.s, accumulate=False).view(ctx.xshape)
            if ctx.needs_input_grad[2]:
                dA = lora_wgrad(g, x2, ctx.s)                           # s G^T X
        if ctx.needs_input_grad[3]:
            dB = lora_wgrad(t, dy2, ctx.s).t()                          # (s T^T dY)^T
        return dy, dx, dA, dB, None


def lora(y, x, A, B, s):
    """the adapter term of one projection, added into its output y (returned): see LoraFn"""
    return LoraFn.apply(y, x, A, B, float(s))


# ---- the 3x3 form: y = conv3x3(x, W) + b + s B conv3x3(x, A), A [r, Cin, 3, 3], on NHWC activations ----------------------
def _lora_nhwc(act, small, what, c_dim):
    """``act`` [N, H, W, C] and the packed ``small`` [*, 9, *] (its dimension ``c_dim`` is C): contiguous GPU tensors of one dtype"""
    _lora_mats(act, small, what)
    if act.dim() != 4 or small.dim() != 3 or small.shape[1] != 9 or small.shape[c_dim] != act.shape[3]:
        raise _lib.MdmHipError("%s: activation %s (NHWC) and packed matrix %s do not fit" % (what, tuple(act.shape), tuple(small.shape)))


def lora_down_conv3x3(x, a):
    """t [N, H, W, r]: t[n, y, x] = sum over the 9 taps of x[n, y + ky - 1, x + kx - 1] a[:, 3 ky + kx, :]^T  (x NHWC,
    a packed [r, 9, C]; pixels outside the image count as zeros)"""
    _lora_nhwc(x, a, "lora_down_conv3x3", 2)
    N, H, W, C = x.shape
    r = a.shape[0]
    t = torch.empty((N, H, W, r), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().mdm_lora_down_conv3x3(_p(x), _p(a), _p(t), N, H, W, C, r, _dt(x), _stream()), "mdm_lora_down_conv3x3")
    return t


def lora_up_add_conv3x3(y, t, b, s, accumulate=True):
    """y [N, H, W, Cout] (+)= s sum over the taps of t[n, y + ky - 1, x + kx - 1] b[:, 3 ky + kx, :]^T in place  (t
    [N, H, W, r], b packed [Cout, 9, r]); ``accumulate=False`` overwrites y without reading it"""
    _lora_nhwc(y, b, "lora_up_add_conv3x3", 0)
    _lora_mats(y, t, "lora_up_add_conv3x3")
    N, H, W, Cout = y.shape
    r = b.shape[2]
    if tuple(t.shape) != (N, H, W, r):
        raise _lib.MdmHipError("lora_up_add_conv3x3: y %s, t %s, b %s do not fit" % (tuple(y.shape), tuple(t.shape), tuple(b.shape)))
    _lib.check(_lib.lib().mdm_lora_up_add_conv3x3(_p(y), _p(t), _p(b), N, H, W, Cout, r, float(s), 1 if accumulate else 0, _dt(y),
                                                  _stream()), "mdm_lora_up_add_conv3x3")
    return y


def lora_wgrad_conv3x3(p, q, s, out=None):
    """d [r, 9, C] fp32: d[:, 3 ky + kx, :] = s sum over the pixels of p[n, y, x]^T q[n, y + ky - 1, x + kx - 1]  (p
    [N, H, W, r], q [N, H, W, C]); with ``out`` the result is ADDED into it.  Deterministic (no atomics)."""
    _lora_mats(q, p, "lora_wgrad_conv3x3")
    if q.dim() != 4 or p.dim() != 4 or p.shape[:3] != q.shape[:3]:
        raise _lib.MdmHipError("lora_wgrad_conv3x3: p %s and q %s must be NHWC tensors over the same pixels" % (tuple(p.shape), tuple(q.shape)))
    N, H, W, C = q.shape
    r = p.shape[3]
    L = _lib.lib()
    splits, wsb = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(L.mdm_lora_wgrad_conv3x3_plan(N, H, W, r, C, _dt(q), ctypes.byref(splits), ctypes.byref(wsb)), "mdm_lora_wgrad_conv3x3_plan")
    ws = _f32_ws(wsb.value, q.device)
    d = torch.empty((r, 9, C), dtype=torch.float32, device=q.device) if out is None else out
    if d.dtype != torch.float32 or not d.is_contiguous() or tuple(d.shape) != (r, 9, C):
        raise _lib.MdmHipError("lora_wgrad_conv3x3: out must be a contiguous fp32 [%d, 9, %d] tensor" % (r, C))
    _lib.check(L.mdm_lora_wgrad_conv3x3(_p(p), _p(q), _p(d), _p(ws), N, H, W, r, C, float(s), 0 if out is None else 1, _dt(q),
                                        _stream()), "mdm_lora_wgrad_conv3x3")
    return d


def _lora_conv_packs(A, B, dtype):
    """(A as [r, 9, C], its flipped transpose [C, 9, r] with [c][tap][j] = A[j][8 - tap][c], B [N, r], B^T [r, N]) of the
    activation dtype for A [r, C, 3, 3], B [N, r]; cached and re-made into the same buffers as _lora_packs does"""
    ent = _cache_slot(A)
    key = ("lora3x3", dtype)
    ver = (A._version, B._version, A.data_ptr(), B.data_ptr(), _pack_epoch)
    if key in ent and ent[key][0] == ver:
        return ent[key][1]
    _require_gpu(A)
    _require_gpu(B)
    r, C = A.shape[0], A.shape[1]
    N = B.shape[0]
    prev = ent[key][1] if key in ent else None
    if prev is None or prev[0].shape != (r, 9, C) or prev[2].shape != B.shape or prev[0].device != A.device:
        prev = tuple(torch.empty(shp, dtype=dtype, device=A.device) for shp in ((r, 9, C), (C, 9, r), (N, r), (r, N)))
    with torch.no_grad():
        prev[0].view(r, 3, 3, C).copy_(A.permute(0, 2, 3, 1))
        prev[1].view(C, 3, 3, r).copy_(A.flip(2, 3).permute(1, 2, 3, 0))
        prev[2].copy_(B)
        prev[3].copy_(B.t())
    ent[key] = (ver, prev)
    return prev


class LoraConvFn(torch.autograd.Function):
    """y += s conv3x3(x, A) B^T, IN PLACE on y = the base 3x3 convolution's fresh output (as LoraFn).  x [N, H, W, C] is
    that convolution's input; A [r, C, 3, 3], B [N, r] are the fp32 adapter parameters."""

    @staticmethod
    def forward(ctx, y, x, A, B, s):
        _require_gpu(x)
        _require_gpu(y)
        if A.dim() != 4 or tuple(A.shape[2:]) != (3, 3) or B.dim() != 2 or x.dim() != 4 or not y.is_contiguous() or y.dtype != x.dtype \
                or tuple(y.shape) != tuple(x.shape[:3]) + (B.shape[0],) or x.shape[3] != A.shape[1] or B.shape[1] != A.shape[0]:
            raise _lib.MdmHipError("lora_conv: y %s / x %s / A %s / B %s do not fit (x, y NHWC; y contiguous, of x's dtype)"
                                   % (tuple(y.shape), tuple(x.shape), tuple(A.shape), tuple(B.shape)))
        x = _c(x)
        r, N = A.shape[0], B.shape[0]
        a_p, _, b_c, _ = _lora_conv_packs(A, B, x.dtype)
        t = lora_down_conv3x3(x, a_p)
        lora_up_add(y.view(-1, N), t.view(-1, r), b_c, s)
        ctx.mark_dirty(y)
        ctx.save_for_backward(x, t, A, B)
        ctx.s = s
        return y

    @staticmethod
    def backward(ctx, dy):
        x, t, A, B = ctx.saved_tensors
        r, C = A.shape[0], A.shape[1]
        N = B.shape[0]
        dy2 = _c(dy).reshape(-1, N)
        _, af_c, _, bt_c = _lora_conv_packs(A, B, x.dtype)
        dx = dA = dB = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            g = lora_down(dy2, bt_c).view(x.shape[:3] + (r,))             # G = dY B
            if ctx.needs_input_grad[1]:                                   # the low-rank part of dX: the transposed 3x3 of G
                dx = lora_up_add_conv3x3(torch.empty_like(x), g, af_c, ctx.s, accumulate=False)
            if ctx.needs_input_grad[2]:                                   # [r, 9, C] -> A's [r, C, 3, 3]
                dA = lora_wgrad_conv3x3(g, x, ctx.s).view(r, 3, 3, C).permute(0, 3, 1, 2).contiguous()
        if ctx.needs_input_grad[3]:
            dB = lora_wgrad(t.view(-1, r), dy2, ctx.s).t()                # (s T^T dY)^T
        return dy, dx, dA, dB, None


def lora_conv(y, x, A, B, s):
    """the adapter term of one 3x3 convolution, added into its output y (returned): see LoraConvFn"""
    return LoraConvFn.apply(y, x, A, B, float(s))


# --------------------------------------------------------------------------------------
# MXFP8 sampling path (mdm_hip/fp8.py, csrc/fp8.hip): E4M3 codes + one E8M0 scale byte per 32 K elements.  No autograd.
# --------------------------------------------------------------------------------------
class Mx8:
    """rows [M, K] in MXFP8: ``q`` uint8 [M, Kp] (e4m3fn codes), ``s`` uint8 [M, Kp / 32] (E8M0 scale bytes), Kp = K
    rounded up to 128 (padding: code 0, scale 127)"""

    __slots__ = ("q", "s", "K")

    def __init__(self, q, s, K):
        self.q, self.s, self.K = q, s, K

    @property
    def rows(self):
        return self.q.shape[0]

    @property
    def Kp(self):
        return self.q.shape[1]


def _mx8_inference_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise _lib.MdmHipError("the MXFP8 layers are inference-only (no backward): run them under torch.no_grad()")


def mx8_quant(x, out=None):
    """x [..., K] (bf16 or fp32, K % 8 == 0) -> Mx8 of the rows [M, K].  ``out``: an Mx8 of the same shape to write into."""
    _require_gpu(x)
    _mx8_inference_only(x)
    x = _c(x.detach())
    K = x.shape[-1]
    M = x.numel() // K
    if K % 8 or M < 1:
        raise _lib.MdmHipError("mx8_quant: %d rows of %d elements; the row length must be a multiple of 8" % (M, K))
    Kp = _round_up(K, 128)
    if out is None:
        out = Mx8(torch.empty((M, Kp), dtype=torch.uint8, device=x.device),
                  torch.empty((M, Kp // 32), dtype=torch.uint8, device=x.device), K)
    _lib.check(_lib.lib().mdm_mx8_quant(_p(x), _dt(x), M, K, Kp, _p(out.q), _p(out.s), _stream()), "mdm_mx8_quant")
    return out


def mx8_gemm(a, w, bias=None, residual=None, gelu=False, emit=False):
    """Y [M, N] = a w^T (+ bias) (+ GELU) (+ residual) for Mx8 operands a [M, K], w [N, K]: a bf16 tensor, or with
    ``emit`` the Mx8 of that bf16 tensor (bit-equal to ``mx8_quant`` of it) for a GEMM that consumes it directly.
    bias fp32 [N]; residual bf16 with M N elements."""
    M, N = a.rows, w.rows
    if a.Kp != w.Kp or a.K != w.K:
        raise _lib.MdmHipError("mx8_gemm: the operands have %d and %d columns" % (a.K, w.K))
    if N % 32:
        raise _lib.MdmHipError("mx8_gemm: %d output channels; the MXFP8 GEMM needs a multiple of 32" % N)
    _mx8_inference_only(bias, residual)
    dev = a.q.device
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
        raise _lib.MdmHipError("mx8_gemm: the bias must be a contiguous fp32 vector of %d elements" % N)
    if residual is not None:
        _require_gpu(residual)
        if residual.dtype != torch.bfloat16 or residual.numel() != M * N:
            raise _lib.MdmHipError("mx8_gemm: the residual must be a bf16 tensor of %d x %d elements (got %s, %d)"
                                   % (M, N, residual.dtype, residual.numel()))
        residual = _c(residual.detach())
    act = 1 if gelu else 0
    L = _lib.lib()
    if emit:
        Np = _round_up(N, 128)
        out = Mx8(torch.empty((M, Np), dtype=torch.uint8, device=dev), torch.empty((M, Np // 32), dtype=torch.uint8, device=dev), N)
        _lib.check(L.mdm_mx8_gemm(_p(a.q), _p(a.s), _p(w.q), _p(w.s), _p(bias), _p(residual), None, _p(out.q), _p(out.s),
                                  M, N, a.Kp, act, _stream()), "mdm_mx8_gemm")
        return out
    y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    _lib.check(L.mdm_mx8_gemm(_p(a.q), _p(a.s), _p(w.q), _p(w.s), _p(bias), _p(residual), _p(y), None, None,
                              M, N, a.Kp, act, _stream()), "mdm_mx8_gemm")
    return y


def packed_weight_mx8(weight: torch.Tensor, bias):
    """(Mx8 of the weight as [Cout, Cin], fp32 bias or None) for a reference-layout 1x1 weight ``(Cout, Cin[, 1, 1])``,
    quantised from the fp32 master and cached per parameter version exactly like ``packed_weight``: a ``load_state_dict``,
    an EMA swap or a LoRA ``merge()`` re-quantises on the next use (into the same buffers)."""
    ent = _cache_slot(weight)
    ver = (weight._version, None if bias is None else bias._version, weight.data_ptr(), _pack_epoch)
    if "mx8" in ent and ent["mx8"][0] == ver:
        return ent["mx8"][1]
    _require_gpu(weight)
    if weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        raise _lib.MdmHipError("packed_weight_mx8: only 1x1 / linear weights have an MXFP8 form (got %s)" % (tuple(weight.shape),))
    cout, cin = weight.shape[0], weight.shape[1]
    prev, bp = ent["mx8"][1] if "mx8" in ent else (None, None)
    if prev is not None and (tuple(prev.q.shape) != (cout, _round_up(cin, 128)) or prev.q.device != weight.device):
        prev = bp = None
    with torch.no_grad():
        wq = mx8_quant(weight.detach().float().reshape(cout, cin), out=prev)
        if bias is None:
            bp = None
        elif bp is not None and bp.shape == bias.shape and bp.device == bias.device:
            bp.copy_(bias.detach())     # the fp32 copy keeps its buffer too
        else:
            bp = bias.detach().float().contiguous().clone()
    ent["mx8"] = (ver, (wq, bp))
    return ent["mx8"][1]


def mx8_quant_zrow(x):
    """the activation of a 3x3 MXFP8 convolution: x [..., K] (bf16, K % 8 == 0) -> Mx8 of M + 1 rows -- ``mx8_quant`` of the
    rows [M, K] plus the zero row (codes 0, scales 127) that taps outside the image read, written by the same launch"""
    _require_gpu(x)
    _mx8_inference_only(x)
    if x.dtype != torch.bfloat16:
        raise _lib.MdmHipError("mx8_quant_zrow: the MXFP8 convolutions take bf16 activations (got %s)" % x.dtype)
    x = _c(x.detach())
    K = x.shape[-1]
    M = x.numel() // K
    if K % 8 or M < 1:
        raise _lib.MdmHipError("mx8_quant_zrow: %d rows of %d elements; the row length must be a multiple of 8" % (M, K))
    Kp = _round_up(K, 128)
    out = Mx8(torch.empty((M + 1, Kp), dtype=torch.uint8, device=x.device),
              torch.empty((M + 1, Kp // 32), dtype=torch.uint8, device=x.device), K)
    _lib.check(_lib.lib().mdm_mx8_quant_zrow(_p(x), _dt(x), M, K, Kp, _p(out.q), _p(out.s), _stream()), "mdm_mx8_quant_zrow")
    return out


def mx8_conv3x3(a, w, shape, bias=None, residual=None):
    """Y [N, H, W, Cout] (bf16) = conv3x3(a, w) (+ bias) (+ residual), stride 1, zero padding 1: ``a`` the Mx8 of
    ``mx8_quant_zrow`` (N H W + 1 rows of Cin), ``w`` the Mx8 of ``packed_weight_mx8_3x3`` ([Cout 9, Cin]), ``shape`` =
    (N, H, W); bias fp32 [Cout]; residual bf16 with N H W Cout elements."""
    _require_gpu(a.q)
    N, H, W = (int(v) for v in shape)
    if min(N, H, W) < 1 or a.rows != N * H * W + 1:
        raise _lib.MdmHipError("mx8_conv3x3: the activation has %d rows, %d x %d x %d pixels need %d (the zero row last: "
                               "mx8_quant_zrow)" % (a.rows, N, H, W, N * H * W + 1))
    if w.rows % 9 or a.Kp != w.Kp or a.K != w.K:
        raise _lib.MdmHipError("mx8_conv3x3: the activation has %d channels, the weight %d rows of %d" % (a.K, w.rows, w.K))
    cin, cout = a.K, w.rows // 9
    if cin % 32 or cout % 32:
        raise _lib.MdmHipError("mx8_conv3x3: %d -> %d channels; the MXFP8 convolution needs multiples of 32" % (cin, cout))
    _mx8_inference_only(bias, residual)
    dev = a.q.device
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout or not bias.is_contiguous()):
        raise _lib.MdmHipError("mx8_conv3x3: the bias must be a contiguous fp32 vector of %d elements" % cout)
    if residual is not None:
        _require_gpu(residual)
        if residual.dtype != torch.bfloat16 or residual.numel() != N * H * W * cout:
            raise _lib.MdmHipError("mx8_conv3x3: the residual must be a bf16 tensor of %d x %d elements (got %s, %d)"
                                   % (N * H * W, cout, residual.dtype, residual.numel()))
        residual = _c(residual.detach())
    y = torch.empty((N, H, W, cout), dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib().mdm_mx8_conv3x3(_p(a.q), _p(a.s), _p(w.q), _p(w.s), _p(bias), _p(residual), _p(y), N, H, W, cin, cout,
                                          _stream()), "mdm_mx8_conv3x3")
    return y


def packed_weight_mx8_3x3(weight: torch.Tensor, bias):
    """(Mx8 of the weight as [Cout 9, Cin], row o 9 + ky 3 + kx, fp32 bias or None) for a reference-layout 3x3 weight
    ``(Cout, Cin, 3, 3)``: a block is 32 input channels of one (o, tap).  Quantised from the fp32 master and cached per
    parameter version under a key of its own, exactly like ``packed_weight_mx8``."""
    ent = _cache_slot(weight)
    ver = (weight._version, None if bias is None else bias._version, weight.data_ptr(), _pack_epoch)
    if "mx8_3x3" in ent and ent["mx8_3x3"][0] == ver:
        return ent["mx8_3x3"][1]
    _require_gpu(weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise _lib.MdmHipError("packed_weight_mx8_3x3: only 3x3 weights (got %s)" % (tuple(weight.shape),))
    cout, cin = weight.shape[0], weight.shape[1]
    prev, bp = ent["mx8_3x3"][1] if "mx8_3x3" in ent else (None, None)
    if prev is not None and (tuple(prev.q.shape) != (cout * 9, _round_up(cin, 128)) or prev.q.device != weight.device):
        prev = bp = None
    with torch.no_grad():
        wq = mx8_quant(weight.detach().float().permute(0, 2, 3, 1).reshape(cout * 9, cin), out=prev)
        if bias is None:
            bp = None
        elif bp is not None and bp.shape == bias.shape and bp.device == bias.device:
            bp.copy_(bias.detach())
        else:
            bp = bias.detach().float().contiguous().clone()
    ent["mx8_3x3"] = (ver, (wq, bp))
    return ent["mx8_3x3"][1]


# --------------------------------------------------------------------------------------
# normalisation
# --------------------------------------------------------------------------------------
def _gn_ws(N, HW, C, G, device):
    wsb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().mdm_gn_plan(N, HW, C, G, ctypes.byref(wsb)), "mdm_gn_plan")
    return _f32_ws(wsb.value, device)


def _gn_forward(x, gamma, beta, film, groups, eps, act):
    """the GroupNorm forward launch on contiguous operands -> (y, stats [N, G, 2], coef [N, C, 2])"""
    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    g32, b32 = _c(gamma.detach().float()), _c(beta.detach().float())
    y = torch.empty_like(x)
    stats = torch.empty((N, groups, 2), dtype=torch.float32, device=x.device)
    coef = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
    ws = _gn_ws(N, HW, C, groups, x.device)
    _prof_wrap("group_norm fwd (HW=%d)" % HW, 2.0 * x.numel() * x.element_size(), lambda: _lib.check(
        _lib.lib().mdm_gn_fwd(_p(x), _p(g32), _p(b32), _p(film), _p(y), _p(stats), _p(coef), _p(ws), N, HW, C,
                              groups, float(eps), act, _dt(x), _stream()),
        "mdm_gn_fwd",
    ), kind="hbm")
    return y, stats, coef


class GroupNormFn(torch.autograd.Function):
    """y = act(GroupNorm(x) * (1 + film[:, :C]) + film[:, C:]);  act in {0: none, 1: SiLU}."""

    @staticmethod
    def forward(ctx, x, gamma, beta, film, groups, eps, act, passthrough):
        _require_gpu(x)
        x, film = _c(x), _c(film)
        y, stats, coef = _gn_forward(x, gamma, beta, film, groups, eps, act)
        ctx.save_for_backward(x, gamma, beta, film, stats, coef)
        ctx.groups, ctx.act = groups, act
        ctx.passthrough = passthrough
        # an unused pass-through output (the skip tap of a block whose activations nobody collects) must reach backward
        # as None, not as a materialised zero tensor that costs an allocation, a memset and a read pass of the kernel
        ctx.set_materialize_grads(False)
        if passthrough == 2:
            # third output = x once more, for a consumer OUTSIDE the block (the U-Net's skip connection): its gradient
            # arrives as dres2 and is added in the same kernel -- no accumulation kernel of the autograd engine
            return y, x.view_as(x), x.view_as(x)
        if passthrough:
            # second output = x itself: the caller routes the block's residual branch through it, so the gradient of
            # that branch arrives HERE (dres) and is added inside the GroupNorm backward kernel
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dres=None, dres2=None):
        x, gamma, beta, film, stats, coef = ctx.saved_tensors
        if dy is None:                       # only the pass-through outputs were used
            dy = torch.zeros_like(x)
        dx, dgamma, dbeta, dfilm = _gn_backward(dy, x, gamma, beta, film, stats, coef, dres, dres2, ctx.groups, ctx.act,
                                                ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, dgamma, dbeta, dfilm, None, None, None, None


def _gn_backward(dy, x, gamma, beta, film, stats, coef, dres, dres2, groups, act, need_params=True):
    """the GroupNorm backward launch (+ where its parameter gradients go): -> (dx, dgamma, dbeta, dfilm); dgamma / dbeta
    are None when they went into the gradient sink (now, or as per-sample rows reduced at the next flush point), and
    when neither gamma nor beta wants one (``need_params`` off: the single launch of before, its sums thrown away)"""
    dy = _c(dy)
    dres = _c(dres) if dres is not None else None
    dres2 = _c(dres2) if dres2 is not None else None
    if dres is None and dres2 is not None:
        dres, dres2 = dres2, None
    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    g32, b32 = _c(gamma.detach().float()), _c(beta.detach().float())
    dx = torch.empty_like(x)
    sg, sb = _slot(gamma), _slot(beta)
    sunk = sg is not None and sb is not None
    deferred = sunk and _defer_wgrad   # per-sample rows now, one multi-layer reduce at the next flush point
    # trainable gamma / beta without a sink and with three or more samples: the per-sample terms go to rows (plain stores)
    # and are summed in a fixed order below -- the kernel's fp32 atomics add them in whatever order the blocks finish, and
    # (a + b) + c != (a + c) + b: two runs of the same step differed in these gradients.  One or two samples: the atomic
    # sum is exact either way.  Frozen gamma and beta: nobody reads the sums, the one launch stays as it was.
    rows = need_params and not sunk and N >= 3
    if deferred:
        dgamma, dbeta = _gn_rows(N, C, x.device)
    elif rows:
        dgamma = torch.empty((N, C), dtype=torch.float32, device=x.device)
        dbeta = torch.empty((N, C), dtype=torch.float32, device=x.device)
    else:
        dgamma = sg if sunk else torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = sb if sunk else torch.empty(C, dtype=torch.float32, device=x.device)
    dfilm = torch.empty_like(film) if film is not None else None
    ws = _gn_ws(N, HW, C, groups, x.device)
    mode = 2 if (deferred or rows) else (1 if sunk else 0)
    npass = 3.0 + (dres is not None) + (dres2 is not None)
    _prof_wrap("group_norm bwd (HW=%d)" % HW, npass * x.numel() * x.element_size(), lambda: _lib.check(
        _lib.lib().mdm_gn_bwd(_p(dy), _p(x), _p(g32), _p(b32), _p(film), _p(stats), _p(coef), _p(dres), _p(dres2), _p(dx), _p(dgamma),
                              _p(dbeta), _p(dfilm), _p(ws), N, HW, C, groups, act, mode, _dt(x), _stream()),
        "mdm_gn_bwd",
    ), kind="hbm")
    if deferred:
        _gn_pending.append((dgamma, dbeta, sg, sb, N, C, gamma, beta))
        _sink_defer(gamma)
        _sink_defer(beta)
        return dx, None, None, dfilm
    if sunk:
        _grad_sink.ready(gamma)
        _grad_sink.ready(beta)
        return dx, None, None, dfilm
    if not need_params:
        return dx, None, None, dfilm
    if rows:
        pg, pb = dgamma, dbeta
        dgamma, dbeta = _prof_wrap("group_norm param rows sum (wgrad of gamma / beta, N=%d)" % N, 2.0 * 4 * (N + 1) * C,
                                   lambda: (pg.sum(0), pb.sum(0)), kind="hbm")
    return dx, dgamma, dbeta, dfilm


def group_norm(x, gamma, beta, groups, eps=1e-5, film=None, silu=False, passthrough=False):
    """``passthrough=True`` returns ``(y, x_res)``: use ``x_res`` (== x) for the residual branch of the block this
    norm opens, and the residual gradient is folded into the norm's backward kernel.  ``passthrough=2`` returns
    ``(y, x_res, x_skip)``: ``x_skip`` (== x again) is for a second consumer outside the block (a skip connection)."""
    return GroupNormFn.apply(x, gamma, beta, film, groups, eps, 1 if silu else 0, int(passthrough))


# --------------------------------------------------------------------------------------
# activation recomputation: GroupNorm(+FiLM)+SiLU -> (dropout) -> 3x3 convolution as ONE autograd node
# --------------------------------------------------------------------------------------
# A ResNet block keeps four full-size activations per call: x (for norm1), h1 = silu(norm1(x)) (for conv1's weight
# gradient), c1 = conv1(h1) (for norm2) and h2 = dropout(silu(norm2(c1) * (1 + ta) + tb)) (for conv2's).  h1 and h2 are
# act(a * x + b) of a tensor that is kept anyway, with the a, b that GroupNormFn keeps anyway (coef), under a dropout mask
# that is a pure function of (p, seed, offset): mdm_gn_reapply reproduces them bit for bit in one elementwise pass.  With
# the switch on, unet.ResNet routes norm -> (dropout) -> conv through GnConvFn, which issues the stored path's forward
# launches, saves what GroupNormFn and ConvFn save EXCEPT h, and re-applies h at the top of its backward.  Opt-in: one more
# read and write of h per ResNet convolution in backward against half of the block's activation memory.
_act_recompute = False


def enable_activation_recompute(flag: bool):
    """Recompute the normalised input of the ResNet 3x3 convolutions in backward instead of keeping it (default off).
    Read when a forward pass runs: a step's forward and backward may straddle a change.  Results are bit-identical either
    way.  Blocks with unmerged conv LoRA adapters (the adapter's backward reads h) or an MXFP8 handle keep the stored
    path for the convolutions concerned; attention layers, FFN hidden activations, conv3, the resampling convolutions and
    the queued operands of deferred 1x1 weight gradients are not covered."""
    global _act_recompute
    _act_recompute = bool(flag)


def activation_recompute_enabled() -> bool:
    return _act_recompute


def gn_reapply(x, coef, silu=True, p=0.0, seed=0, offset=0):
    """act(coef[..., 0] * x + coef[..., 1]) (+ the dropout mask of (p, seed, offset)): the output of the GroupNorm launch
    that wrote ``coef`` ([N, C, 2] fp32), and of the dropout launch behind it, bit for bit (C ABI mdm_gn_reapply)"""
    _require_gpu(x)
    x = _c(x)
    N, C = x.shape[0], x.shape[-1]
    if tuple(coef.shape) != (N, C, 2) or coef.dtype != torch.float32 or coef.device != x.device:
        raise _lib.MdmHipError("gn_reapply: coef must be fp32 [N=%d, C=%d, 2] on %s, got %s %s on %s" % (
            N, C, x.device, coef.dtype, tuple(coef.shape), coef.device))
    coef = _c(coef)
    HW = x.numel() // (N * C)
    y = torch.empty_like(x)
    nbytes = 2.0 * x.numel() * x.element_size()
    _prof_wrap("group_norm reapply (HW=%d)" % HW, nbytes, lambda: _lib.check(
        _lib.lib().mdm_gn_reapply(_p(x), _p(coef), _p(y), N, HW, C, 1 if silu else 0, float(p), int(seed), int(offset), _dt(x),
                                  _stream()), "mdm_gn_reapply"), kind="hbm")
    return y


class _ConvNeeds:
    """what _conv_backward reads of a ConvFn context"""

    __slots__ = ("ks", "stride", "has_res", "needs_input_grad")

    def __init__(self, ks, stride, has_res, needs):
        self.ks, self.stride, self.has_res, self.needs_input_grad = ks, stride, has_res, needs


class GnConvFn(torch.autograd.Function):
    """y = conv3x3(dropout_p(act(GroupNorm(x) * (1 + film[:, :C]) + film[:, C:])), weight) + bias (+ residual), with the
    pass-through outputs of GroupNormFn: the launches of GroupNormFn -> DropoutFn -> ConvFn and their gradients, but the
    convolution's input is re-applied in backward (mdm_gn_reapply) rather than saved."""

    @staticmethod
    def forward(ctx, x, gamma, beta, film, groups, eps, act, passthrough, p, weight, bias, residual):
        _require_gpu(x)
        x, film, residual = _c(x), _c(film), _c(residual)
        h, stats, coef = _gn_forward(x, gamma, beta, film, groups, eps, act)
        seed = off = 0
        if p > 0.0:
            h, seed, off = _dropout_forward(h, p)   # the counter moves here, once; backward replays (seed, off)
        y, ks = _conv_forward(h, weight, bias, residual, 1)
        del h   # nothing holds it past the convolution's launch
        ctx.save_for_backward(x, gamma, beta, film, stats, coef, weight, bias)
        ctx.groups, ctx.act, ctx.ks = groups, act, ks
        ctx.has_res = residual is not None
        ctx.drop = (float(p), seed, off)
        ctx.set_materialize_grads(False)   # an unused pass-through output reaches backward as None (see GroupNormFn)
        if passthrough == 2:
            return y, x.view_as(x), x.view_as(x)
        if passthrough:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dres=None, dres2=None):
        x, gamma, beta, film, stats, coef, weight, bias = ctx.saved_tensors
        if dy is None:
            raise _lib.MdmHipError("gn_conv: the convolution's output received no gradient")
        nig = ctx.needs_input_grad
        need_dh = nig[0] or nig[1] or nig[2] or nig[3]
        p, seed, off = ctx.drop
        if nig[9]:
            h = gn_reapply(x, coef, bool(ctx.act), p, seed, off)
        else:
            h = x   # a frozen weight: nothing reads h, _conv_backward takes only shape and dtype from it
        # the weight gradient may run on the side stream: _off_critical_path keeps h referenced until that launch has
        # consumed it, as it keeps a stored x
        dh, dw, db, dres_conv = _conv_backward(_ConvNeeds(ctx.ks, 1, ctx.has_res, (need_dh, nig[9], nig[10], nig[11])),
                                               h, weight, bias, dy)
        del h
        dx = dgamma = dbeta = dfilm = None
        if need_dh:
            if p > 0.0:
                dhd = torch.empty_like(dh)
                _lib.check(_lib.lib().mdm_dropout(_p(dh), _p(dhd), dh.numel(), p, seed, off, _dt(dh), _stream()), "mdm_dropout")
                dh = dhd
            dx, dgamma, dbeta, dfilm = _gn_backward(dh, x, gamma, beta, film, stats, coef, dres, dres2, ctx.groups, ctx.act,
                                                    nig[1] or nig[2])
        return dx, dgamma, dbeta, dfilm, None, None, None, None, None, dw, db, dres_conv


def gn_conv(x, gamma, beta, groups, weight, bias=None, eps=1e-5, film=None, silu=True, passthrough=False, p=0.0,
            residual=None):
    """``conv(dropout(group_norm(x, ..., film=film, silu=silu), p), weight, bias, residual)`` for a 3x3 stride-1
    convolution as one autograd node that does not keep the convolution's input (see enable_activation_recompute);
    ``passthrough`` as in group_norm: the result is ``y``, ``(y, x_res)`` or ``(y, x_res, x_skip)``.  ``p``: the dropout
    probability in effect (0: none), 0 <= p < 1, and the element count a multiple of 8 when p > 0."""
    if weight.dim() != 4 or weight.shape[2] != 3:
        raise _lib.MdmHipError("gn_conv: a 3x3 convolution weight is expected")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise _lib.MdmHipError("gn_conv: dropout probability %r outside [0, 1)" % p)
    if p > 0.0 and x.numel() % 8 != 0:
        raise _lib.MdmHipError("dropout: the element count must be a multiple of 8")
    return GnConvFn.apply(x, gamma, beta, film, groups, eps, 1 if silu else 0, int(passthrough), p, weight, bias, residual)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _require_gpu(x)
        x = _c(x)
        D = x.shape[-1]
        R = x.numel() // D
        g32, b32 = _c(gamma.detach().float()), _c(beta.detach().float())
        y = torch.empty_like(x)
        stats = torch.empty((R, 2), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().mdm_ln_fwd(_p(x), _p(g32), _p(b32), _p(y), _p(stats), R, D, float(eps), _dt(x), _stream()), "mdm_ln_fwd")
        ctx.save_for_backward(x, gamma, beta, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        dy = _c(dy)
        D = x.shape[-1]
        R = x.numel() // D
        g32 = _c(gamma.detach().float())
        dx = torch.empty_like(x)
        sg, sb = _slot(gamma), _slot(beta)
        sunk = sg is not None and sb is not None
        dgamma = sg if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
        dbeta = sb if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
        ws = torch.empty(((R + 63) // 64) * D * 2, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().mdm_ln_bwd(_p(dy), _p(x), _p(g32), _p(stats), _p(dx), _p(dgamma), _p(dbeta), _p(ws), R, D,
                                         1 if sunk else 0, _dt(x), _stream()), "mdm_ln_bwd")
        if sunk:
            _grad_sink.ready(gamma)
            _grad_sink.ready(beta)
            return dx, None, None, None
        return dx, dgamma, dbeta, None


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


# --------------------------------------------------------------------------------------
# text key / value projections of ALL attention layers at once
# --------------------------------------------------------------------------------------
def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


class TextKVFn(torch.autograd.Function):
    """kvc_l = Linear_l(LayerNorm_l(cond)) for every attention layer l (reference unet.py:263-264, 304: each layer
    normalises and projects the SAME text states).  Forward: one multi-LayerNorm launch + one grouped GEMM launch per
    output width; backward: grouped input-gradient GEMMs, one multi-LayerNorm backward (which also sums the L gradients
    of ``cond``), grouped weight gradients.  ~8 launches instead of ~8 per layer; bf16 only (the fp32 parity mode runs
    the layers one by one)."""

    @staticmethod
    def forward(ctx, cond, eps, *params):
        _require_gpu(cond)
        cond = _c(cond)
        B, S, D = cond.shape
        R, L = B * S, len(params) // 4
        lnw, lnb, ws, bs = params[0::4], params[1::4], params[2::4], params[3::4]
        lib = _lib.lib()
        g32 = [_c(t.detach().float()) for t in lnw]
        b32 = [_c(t.detach().float()) for t in lnb]
        cn = [torch.empty_like(cond) for _ in range(L)]
        stats = torch.empty((R, 2), dtype=torch.float32, device=cond.device)
        _lib.check(lib.mdm_ln_multi_fwd(_p(cond), _ptr_array(g32), _ptr_array(b32), _ptr_array(cn), L, _p(stats), R, D, float(eps),
                                        _dt(cond), _stream()), "mdm_ln_multi_fwd")
        groups = {}
        for l, w in enumerate(ws):
            groups.setdefault(w.shape[0], []).append(l)
        ys = [None] * L
        for cout, idx in groups.items():
            packs = [packed_weight(ws[l], bs[l], cond.dtype) for l in idx]
            for l in idx:
                ys[l] = torch.empty((B, S, cout), dtype=cond.dtype, device=cond.device)
            _prof_wrap("linear grouped x%d M=%d N=%d K=%d" % (len(idx), R, cout, D), 2.0 * len(idx) * R * cout * D, lambda: _lib.check(
                lib.mdm_linear_grouped(_ptr_array([cn[l] for l in idx]), _ptr_array([pk[0] for pk in packs]),
                                       _ptr_array([pk[2] for pk in packs]), _ptr_array([ys[l] for l in idx]), len(idx), R, D, cout,
                                       _dt(cond), _stream()), "mdm_linear_grouped"))
        ctx.save_for_backward(cond, stats, *cn, *params)
        ctx.L, ctx.groups = L, groups
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        saved = ctx.saved_tensors
        L, groups = ctx.L, ctx.groups
        cond, stats, cn, params = saved[0], saved[1], saved[2:2 + L], saved[2 + L:]
        lnw, lnb, ws, bs = params[0::4], params[1::4], params[2::4], params[3::4]
        B, S, D = cond.shape
        R = B * S
        lib = _lib.lib()
        dys = [_c(d) if d is not None else torch.zeros((B, S, ws[l].shape[0]), dtype=cond.dtype, device=cond.device)
               for l, d in enumerate(dys)]
        dcn = [torch.empty_like(cond) for _ in range(L)]
        grads = [None] * (4 * L)
        def dgrad(cout, idx):
            packs = [packed_weight(ws[l], bs[l], cond.dtype) for l in idx]
            _prof_wrap("linear grouped x%d M=%d N=%d K=%d" % (len(idx), R, D, cout), 2.0 * len(idx) * R * cout * D, lambda: _lib.check(
                lib.mdm_linear_grouped(_ptr_array([dys[l] for l in idx]), _ptr_array([pk[1] for pk in packs]), None,
                                       _ptr_array([dcn[l] for l in idx]), len(idx), R, cout, D, _dt(cond), _stream()),
                "mdm_linear_grouped"))

        nig = ctx.needs_input_grad
        for cout, idx in groups.items():   # (see SharedInputLinearsFn.backward: the weight gradients are handed over first)
            # weight / bias gradients: one grouped launch, into the gradient arena when there is one
            if not any(nig[2 + 4 * l + 2] or nig[2 + 4 * l + 3] for l in idx):
                continue   # every projection of this width is frozen: no weight-gradient launch
            slots = [(_slot(ws[l]), _slot(bs[l])) for l in idx]
            sunk = all(a is not None and b is not None for a, b in slots)
            if sunk:
                dws, dbs = [a for a, _ in slots], [b for _, b in slots]
            else:
                dws = [torch.zeros(ws[l].shape, dtype=torch.float32, device=cond.device) for l in idx]
                dbs = [torch.zeros(bs[l].shape, dtype=torch.float32, device=cond.device) for l in idx]
            xs2, dy2 = [cn[l].reshape(R, D) for l in idx], [dys[l].reshape(R, cout) for l in idx]

            def go(xs2=xs2, dy2=dy2, dws=dws, dbs=dbs, idx=idx, sunk=sunk, cout=cout):
                _prof_wrap("conv_wgrad grouped x%d M=%d N=%d K=%d" % (len(idx), R, cout, D), 2.0 * len(idx) * R * cout * D,
                           lambda: wgrad_grouped(xs2, dy2, dws, dbs))
                if sunk:
                    for l in idx:
                        _grad_sink.ready(ws[l])
                        _grad_sink.ready(bs[l])

            if sunk:
                _off_critical_path(xs2 + dy2, go)
            else:
                go()
                for k, l in enumerate(idx):
                    grads[4 * l + 2], grads[4 * l + 3] = dws[k], dbs[k]
        for cout, idx in groups.items():
            dgrad(cout, idx)
        g32 = [_c(t.detach().float()) for t in lnw]
        nslots = [(_slot(lnw[l]), _slot(lnb[l])) for l in range(L)]
        nsunk = all(a is not None and b is not None for a, b in nslots)
        if nsunk:
            dgs, dbs_ = [a for a, _ in nslots], [b for _, b in nslots]
        else:
            dgs = [torch.empty(D, dtype=torch.float32, device=cond.device) for _ in range(L)]
            dbs_ = [torch.empty(D, dtype=torch.float32, device=cond.device) for _ in range(L)]
        dcond = torch.empty_like(cond)
        _lib.check(lib.mdm_ln_multi_bwd(_ptr_array(dcn), _p(cond), _ptr_array(g32), _p(stats), _p(dcond), _ptr_array(dgs),
                                        _ptr_array(dbs_), L, R, D, 1 if nsunk else 0, _dt(cond), _stream()), "mdm_ln_multi_bwd")
        if nsunk:
            for l in range(L):
                _grad_sink.ready(lnw[l])
                _grad_sink.ready(lnb[l])
        else:
            for l in range(L):
                grads[4 * l], grads[4 * l + 1] = dgs[l], dbs_[l]
        return (dcond, None) + tuple(grads)


class SharedInputLinearsFn(torch.autograd.Function):
    """y_l = x W_l^T + b_l for several linear layers that read the SAME input (every ResNet's ``time_layer`` applied to
    silu(temb), reference unet.py:206, 227): one grouped GEMM per output width for the outputs, one for the input
    gradients, one grouped weight-gradient launch -- instead of three tiny launches per layer.  bf16 only."""

    @staticmethod
    def forward(ctx, x, *params):
        _require_gpu(x)
        x = _c(x)
        R, D = x.shape
        ws, bs = params[0::2], params[1::2]
        L = len(ws)
        lib = _lib.lib()
        groups = {}
        for l, w in enumerate(ws):
            groups.setdefault(w.shape[0], []).append(l)
        ys = [None] * L
        for cout, idx in groups.items():
            packs = [packed_weight(ws[l], bs[l], x.dtype) for l in idx]
            for l in idx:
                ys[l] = torch.empty((R, cout), dtype=x.dtype, device=x.device)
            _lib.check(lib.mdm_linear_grouped(_ptr_array([x] * len(idx)), _ptr_array([pk[0] for pk in packs]),
                                              _ptr_array([pk[2] for pk in packs]), _ptr_array([ys[l] for l in idx]), len(idx), R, D,
                                              cout, _dt(x), _stream()), "mdm_linear_grouped")
        ctx.save_for_backward(x, *params)
        ctx.groups = groups
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        ws, bs = params[0::2], params[1::2]
        L, groups = len(ws), ctx.groups
        R, D = x.shape
        lib = _lib.lib()
        dys = [_c(d) if d is not None else torch.zeros((R, ws[l].shape[0]), dtype=x.dtype, device=x.device) for l, d in enumerate(dys)]
        dxs = [torch.empty_like(x) for _ in range(L)]
        grads = [None] * (2 * L)
        def dgrad(cout, idx):
            packs = [packed_weight(ws[l], bs[l], x.dtype) for l in idx]
            _lib.check(lib.mdm_linear_grouped(_ptr_array([dys[l] for l in idx]), _ptr_array([pk[1] for pk in packs]), None,
                                              _ptr_array([dxs[l] for l in idx]), len(idx), R, cout, D, _dt(x), _stream()),
                       "mdm_linear_grouped")

        # These layers' gradients arrive when backward ENDS: nothing of the main stream is left to hide behind.  The weight
        # gradients (side stream) are handed over BEFORE the input-gradient launches, so that they wait for what precedes
        # those, not for them (the hand-off makes the side stream wait for everything queued on the main stream so far).
        nig = ctx.needs_input_grad
        for cout, idx in groups.items():
            if not any(nig[1 + 2 * l] or nig[2 + 2 * l] for l in idx):
                continue   # every layer of this width is frozen: no weight-gradient launch
            slots = [(_slot(ws[l]), _slot(bs[l])) for l in idx]
            sunk = all(a is not None and b is not None for a, b in slots)
            if sunk:
                dws, dbs = [a for a, _ in slots], [b for _, b in slots]
            else:
                dws = [torch.zeros(ws[l].shape, dtype=torch.float32, device=x.device) for l in idx]
                dbs = [torch.zeros(bs[l].shape, dtype=torch.float32, device=x.device) for l in idx]
            xs2, dy2 = [x] * len(idx), [dys[l] for l in idx]

            def go(xs2=xs2, dy2=dy2, dws=dws, dbs=dbs, idx=idx, sunk=sunk, cout=cout):
                _prof_wrap("conv_wgrad grouped x%d M=%d N=%d K=%d" % (len(idx), R, cout, D), 2.0 * len(idx) * R * cout * D,
                           lambda: wgrad_grouped(xs2, dy2, dws, dbs))
                if sunk:
                    for l in idx:
                        _grad_sink.ready(ws[l])
                        _grad_sink.ready(bs[l])

            if sunk:
                _off_critical_path([x] + dy2, go)
            else:
                go()
                for k, l in enumerate(idx):
                    grads[2 * l], grads[2 * l + 1] = dws[k], dbs[k]
        for cout, idx in groups.items():
            dgrad(cout, idx)
        dx = dxs[0] if L == 1 else torch.stack(dxs).sum(0)
        return (dx,) + tuple(grads)


def shared_input_linears_supported(x, layers):
    return x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[-1] % 64 == 0 and 0 < len(layers) and \
        all(w.shape[0] % 64 == 0 and b is not None for w, b in layers) and \
        max(sum(1 for w2, _ in layers if w2.shape[0] == w.shape[0]) for w, _ in layers) <= 32


def shared_input_linears(x, layers):
    """layers: [(weight [Cout_l, D], bias [Cout_l])] -> tuple of x W_l^T + b_l"""
    return SharedInputLinearsFn.apply(x, *[t for pair in layers for t in pair])


def text_kv_supported(cond, layers):
    """the grouped path needs bf16 text states of a width the buffer-addressed GEMM takes"""
    return cond.is_cuda and cond.dtype == torch.bfloat16 and cond.shape[-1] % 64 == 0 and 0 < len(layers) <= 32 and \
        all(w.shape[0] % 64 == 0 for _, _, w, _ in layers)


def text_kv(cond, layers, eps=1e-5):
    """layers: [(ln_weight, ln_bias, weight, bias)] -> tuple of kvc tensors [B, S, Cout_l]"""
    flat = [t for quad in layers for t in quad]
    return TextKVFn.apply(cond, eps, *flat)


# --------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------
class AttentionFn(torch.autograd.Function):
    """out = softmax(q k^T / sqrt(d)) v + softmax(q k_c^T / sqrt(d) [masked]) v_c."""

    @staticmethod
    def forward(ctx, qkv, kvc, mask, heads, keep):
        _require_gpu(qkv)
        qkv, kvc = _c(qkv), _c(kvc)
        B, C, L, _, _ = _attn_dims(qkv, kvc, heads)
        m32 = _c(mask.float()) if mask is not None else None
        out = torch.empty(qkv.shape[:-1] + (C,), dtype=qkv.dtype, device=qkv.device)
        lse_s = torch.empty((B, heads, L), dtype=torch.float32, device=qkv.device) if keep else None
        lse_c = torch.empty((B, heads, L), dtype=torch.float32, device=qkv.device) if (keep and kvc is not None) else None
        oc = torch.empty_like(out) if kvc is not None else None   # also the kernel's staging buffer for the cross part
        _fwd_launch(qkv, kvc, m32, out, 0, B, heads, oc=oc, lse=(lse_s, lse_c))
        ctx.save_for_backward(qkv, kvc, m32, out, oc, lse_s, lse_c)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, kvc, m32, out, oc, lse_s, lse_c = ctx.saved_tensors
        dout = _c(dout)
        B = qkv.shape[0]
        C = qkv.shape[-1] // 3
        L = qkv.numel() // (B * 3 * C)
        S = kvc.shape[1] if kvc is not None else 0
        heads = ctx.heads
        d = C // heads
        dqkv = torch.empty_like(qkv)
        dkvc = torch.empty_like(kvc) if kvc is not None else None
        delta_s = torch.empty_like(lse_s)
        delta_c = torch.empty_like(lse_c) if kvc is not None else None
        _prof_wrap("attn_bwd (delta + dq + dkv kernels)<d=%d> L=%d" % (d, L), 8.0 * B * heads * L * (L + S) * d, lambda: _lib.check(
            _lib.lib().mdm_attn_bwd(_p(qkv), _p(kvc), _p(m32), _p(out), _p(oc), _p(dout), _p(lse_s), _p(lse_c), _p(delta_s),
                                    _p(delta_c), _p(dqkv), _p(dkvc), B, L, S, heads, d, _dt(qkv), _stream()),
            "mdm_attn_bwd",
        ), kind="attn")
        return dqkv, dkvc, None, None, None


def _attn_dims(qkv, kvc, heads):
    B = qkv.shape[0]
    C = qkv.shape[-1] // 3
    L = qkv.numel() // max(B * 3 * C, 1)
    S = kvc.shape[1] if kvc is not None else 0
    return B, C, L, S, C // heads


# ---- the launchers: each C entry of the attention layer is called from one place -----------------------------------------
def _row_ptr(t, row):
    """the address of batch row ``row`` of a contiguous tensor (None for None)"""
    return None if t is None else t.data_ptr() + row * (t.numel() // t.shape[0]) * t.element_size()


def _fwd_launch(qkv, kvc, m32, out, first, n, heads, oc=None, lse=(None, None)):
    """mdm_attn_fwd on batch rows [first, first + n) of contiguous tensors, into the same rows of ``out``.  ``kvc=None``
    leaves the text keys out: S = 0 with null kvc, mask and oc.  ``oc``: the kernel's staging buffer for the cross part,
    allocated here for the launched rows unless given; ``lse``: the pair a backward needs."""
    _, _, L, S, d = _attn_dims(qkv, kvc, heads)
    if oc is None and kvc is not None:
        oc = torch.empty((n,) + tuple(out.shape[1:]), dtype=out.dtype, device=out.device)
    _prof_wrap("attn_fwd_kernel<d=%d> L=%d" % (d, L), 4.0 * n * heads * L * (L + S) * d, lambda: _lib.check(
        _lib.lib().mdm_attn_fwd(_row_ptr(qkv, first), _row_ptr(kvc, first), _row_ptr(m32, first), _row_ptr(out, first), _p(oc),
                                _p(lse[0]), _p(lse[1]), n, L, S, heads, d, _dt_mm(qkv), _stream()),
        "mdm_attn_fwd",
    ), kind="attn")


def _cross_addv_launch(qkv, kvc, m32, out, row0, rows, heads):
    """mdm_attn_cross_addv on batch rows [row0, row0 + rows) of contiguous tensors, into the same rows of ``out``"""
    _, C, L, S, d = _attn_dims(qkv, kvc, heads)
    _prof_wrap("attn_cross_addv_kernel<d=%d> L=%d" % (d, L), 4.0 * rows * heads * L * S * d, lambda: _lib.check(
        _lib.lib().mdm_attn_cross_addv(_row_ptr(qkv, row0), _row_ptr(kvc, row0), _row_ptr(m32, row0), _row_ptr(out, row0), rows,
                                       L, S, heads, d, _dt_mm(qkv), _stream()),
        "mdm_attn_cross_addv",
    ), kind="attn")


def _cross_bias_launch(geom, q, kv, m, bias, bias_ld, base, base_ld, out, rows):
    """mdm_attn_cross_bias on ``rows`` batch rows; ``geom`` = (L, S, heads, d, dtype code), everything else the address of a
    first row: ``q`` in [.., L, 3C], ``kv`` [.., S, 2C], ``m`` the fp32 mask or None, ``bias`` fp32 [.., L, bias_ld], ``base``
    the v columns of qkv (``base_ld`` = 3C) or [.., L, C] (C; ``out`` itself: in place), ``out`` [.., L, C]"""
    L, S, heads, d, dt = geom
    _prof_wrap("attn_cross_addv_kernel<d=%d, bias> L=%d" % (d, L), 4.0 * rows * heads * L * S * d, lambda: _lib.check(
        _lib.lib().mdm_attn_cross_bias(q, kv, m, bias, bias_ld, base, base_ld, out, rows, L, S, heads, d, dt, _stream()),
        "mdm_attn_cross_bias",
    ), kind="attn")


# ---- the operand checks ----------------------------------------------------------------------------------------------------
def _inference_only(what, kernel, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise _lib.MdmHipError("%s is inference only (%s has no backward): run it under torch.no_grad()" % (what, kernel))


def _check_f32_3d(what, name, t, rows, L, S, device, contiguous=True):
    """``t`` is fp32 [rows, L, ld], ld >= S, ld % 4 == 0, on ``device``; ``contiguous=False``: the caller copies it"""
    if (t.dim() != 3 or tuple(t.shape[:2]) != (rows, L) or t.shape[2] < S or t.shape[2] % 4 or t.dtype != torch.float32
            or t.device != device or (contiguous and not t.is_contiguous())):
        raise _lib.MdmHipError("%s: %s %s %s on %s (wanted %sfp32 [%d, %d, ld], ld >= %d, ld %% 4 == 0, on %s)" % (
            what, name, tuple(t.shape), t.dtype, t.device, "a contiguous " if contiguous else "", rows, L, S, device))


def _check_gate(what, gate, device):
    if gate.dtype != torch.float32 or gate.numel() != 1 or gate.device != device:
        raise _lib.MdmHipError("%s: gate is one fp32 value on the tensors' device (got %s %s on %s)"
                               % (what, gate.dtype, tuple(gate.shape), gate.device))


def _check_bias(what, qkv, kvc, bias):
    """the bias of mdm_attn_cross_bias -> as the kernel reads it (fp32, contiguous [N, L, ld])"""
    if kvc is None:
        raise _lib.MdmHipError("%s: no text keys (kvc is None) -- there are no logits to bias" % what)
    N, _, L, S, _ = _attn_dims(qkv, kvc, 1)
    _check_f32_3d(what, "bias", bias, N, L, S, qkv.device, contiguous=False)
    return _c(bias.detach())


def attn_cross_addv(qkv, kvc, mask, heads):
    """out = v + softmax(q k_c^T / sqrt(d) [masked]) v_c: the attention of perturbed-attention guidance's perturbed rows
    (self-attention map = identity; include/mdm_hip.h mdm_attn_cross_addv).  Forward only."""
    _require_gpu(qkv)
    qkv, kvc = _c(qkv), _c(kvc)
    m32 = _c(mask.float()) if (mask is not None and kvc is not None) else None
    out = torch.empty(qkv.shape[:-1] + (qkv.shape[-1] // 3,), dtype=qkv.dtype, device=qkv.device)
    _cross_addv_launch(qkv, kvc, m32, out, 0, qkv.shape[0], heads)
    return out


def attn_cross_bias(qkv, kvc, mask, bias, heads, base=None):
    """out = base + softmax(q k_c^T / sqrt(d) + bias [masked; bias <= -1e30 excludes]) v_c  (include/mdm_hip_ext.h
    mdm_attn_cross_bias).  ``bias``: fp32 [N, L, ld], ld >= S, ld % 4 == 0.  ``base=None``: v of ``qkv``, into a new tensor;
    a contiguous [N, L, C] tensor of qkv's dtype: the term is added onto it IN PLACE and it is returned.  Forward only."""
    if base is None:   # every row a perturbed one
        return _attn_blocks("attn_cross_bias", qkv, kvc, mask, heads, qkv.shape[0], bias, None)
    _require_gpu(qkv)
    _inference_only("attn_cross_bias", "mdm_attn_cross_bias", qkv, kvc, bias)
    bias = _check_bias("attn_cross_bias", qkv, kvc, bias)
    qkv, kvc = _c(qkv.detach()), _c(kvc.detach())
    m32 = _c(mask.float()) if mask is not None else None
    N, C, L, S, d = _attn_dims(qkv, kvc, heads)
    shape = qkv.shape[:-1] + (C,)
    if tuple(base.shape) != tuple(shape) or base.dtype != qkv.dtype or not base.is_contiguous() or base.device != qkv.device:
        raise _lib.MdmHipError("attn_cross_bias: base %s %s (wanted a contiguous %s %s)"
                               % (tuple(base.shape), base.dtype, tuple(shape), qkv.dtype))
    geom = (L, S, heads, d, _dt_mm(qkv))
    _cross_bias_launch(geom, _p(qkv), _p(kvc), _p(m32), _p(bias), bias.shape[-1], _p(base), C, _p(base), N)
    return base


def _ctrl_tables(what, own, src, gate, device):
    """the row tables and the gate of the attention-control kernels: int32 [R] twice and one fp32 value, on ``device``"""
    for name, t in (("own", own), ("src", src)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.device != device or not t.is_contiguous():
            raise _lib.MdmHipError("%s: %s rows are a contiguous int32 [R] on the tensors' device (got %s %s on %s)"
                                   % (what, name, t.dtype, tuple(t.shape), t.device))
    if own.numel() != src.numel() or own.numel() < 1:
        raise _lib.MdmHipError("%s: %d own rows for %d source rows" % (what, own.numel(), src.numel()))
    _check_gate(what, gate, device)
    return own.numel()


@torch.no_grad()
def ctrl_mix_kv(kvc, own, src, M, D, mask, gate):
    """The text keys / values of prompt-to-prompt's edited rows (include/mdm_hip_ext.h mdm_ctrl_mix_kv) -> (kv_a, kv_b),
    [R, S, 2C] each of kvc's dtype: kv_a[r] = (k_c[src[r]] | gate * sum_{j live} M[r][:, j] v_c[own[r]][j]), kv_b[r] =
    (k_c[own[r]] | (gate ? D[r] : 1) * v_c[own[r]]).  ``kvc`` [N, S, 2C]; ``own``, ``src``: int32 [R] batch rows on the device;
    ``M`` fp32 [R, S, ld] (ld >= S, ld % 4 == 0; columns [S, ld) are never read), ``D`` fp32 [R, S]; ``mask`` [N, S] or
    None; ``gate``: a device float[1].  CPU tensors: ``attn_control.mix_kv``."""
    _require_gpu(kvc)
    kvc = _c(kvc.detach())
    if kvc.dim() != 3 or kvc.shape[-1] % 2:
        raise _lib.MdmHipError("ctrl_mix_kv: kvc %s (wanted [N, S, 2C])" % (tuple(kvc.shape),))
    N, S, C = kvc.shape[0], kvc.shape[1], kvc.shape[2] // 2
    R = _ctrl_tables("ctrl_mix_kv", own, src, gate, kvc.device)
    _check_f32_3d("ctrl_mix_kv", "M", M, R, S, S, kvc.device)
    if tuple(D.shape) != (R, S) or D.dtype != torch.float32 or not D.is_contiguous() or D.device != kvc.device:
        raise _lib.MdmHipError("ctrl_mix_kv: D %s %s for R = %d, S = %d (wanted a contiguous fp32 [R, S])"
                               % (tuple(D.shape), D.dtype, R, S))
    m32 = None
    if mask is not None:
        if mask.numel() != N * S or mask.shape[0] != N or mask.device != kvc.device:
            raise _lib.MdmHipError("ctrl_mix_kv: mask %s for N = %d, S = %d" % (tuple(mask.shape), N, S))
        m32 = _c(mask.detach().float())
    kv_a = torch.empty((R, S, 2 * C), dtype=kvc.dtype, device=kvc.device)
    kv_b = torch.empty_like(kv_a)
    _prof_wrap("ctrl_mix_kv_kernel S=%d" % S, 2.0 * R * S * S * C, lambda: _lib.check(
        _lib.lib().mdm_ctrl_mix_kv(_p(kvc), _p(own), _p(src), _p(M), M.shape[2], _p(D), _p(m32), _p(gate), _p(kv_a), _p(kv_b),
                                   N, R, S, C, _dt(kvc), _stream()),
        "mdm_ctrl_mix_kv",
    ), kind="attn")
    return kv_a, kv_b


@torch.no_grad()
def ctrl_gather_qkv(qkv, own, src, gate):
    """The self-attention operands of prompt-to-prompt's edited rows (include/mdm_hip_ext.h mdm_ctrl_gather_qkv) ->
    (qkv_self, q_src), [R, L, 3C] each: qkv_self[r] has the q and k columns of row ``gate ? src[r] : own[r]`` and the v
    columns of row own[r]; q_src[r] has the q columns of row src[r] and NOTHING DEFINED in its k and v columns.  Copies, bit
    for bit.  CPU tensors: ``attn_control.gather_qkv``."""
    _require_gpu(qkv)
    qkv = _c(qkv.detach())
    if qkv.dim() < 3 or qkv.shape[-1] % 3:
        raise _lib.MdmHipError("ctrl_gather_qkv: qkv %s (wanted [N, L, 3C])" % (tuple(qkv.shape),))
    N, C = qkv.shape[0], qkv.shape[-1] // 3
    L = qkv.numel() // max(N * 3 * C, 1)
    R = _ctrl_tables("ctrl_gather_qkv", own, src, gate, qkv.device)
    qkv_self = torch.empty((R, L, 3 * C), dtype=qkv.dtype, device=qkv.device)
    q_src = torch.empty_like(qkv_self)
    _prof_wrap("ctrl_gather_qkv_kernel L=%d" % L, float(R * L * 7 * C * qkv.element_size()), lambda: _lib.check(
        _lib.lib().mdm_ctrl_gather_qkv(_p(qkv), _p(own), _p(src), _p(gate), _p(qkv_self), _p(q_src), N, R, L, C, _dt(qkv),
                                       _stream()),
        "mdm_ctrl_gather_qkv",
    ), kind="hbm")
    return qkv_self, q_src


_CTRL_ZERO = {}   # (device, R, L, ld) -> the static zero bias of the controlled rows' two cross launches


def _attn_blocks(what, qkv, kvc, mask, heads, pag_rows, bias, ctrl):
    """The inference attention of a model batch laid out [ordinary lead | controlled | ordinary-or-perturbed tail]: the checks,
    once, under the caller's name ``what``, then the launches block by block into one output (the block table: DESIGN
    section 4.25).  ``ctrl`` (None: no controlled block) places the controlled rows at [row0, row0 + R); the tail is perturbed
    where ``pag_rows``, its size, is not 0.  Order: the lead, a tail that is not perturbed, the controlled block, a perturbed
    tail."""
    _require_gpu(qkv)
    _inference_only(what, "mdm_attn_cross_addv" if bias is None and ctrl is None else "mdm_attn_cross_bias", qkv, kvc, bias)
    N, pag_rows = qkv.shape[0], int(pag_rows)
    row0, R = (N - pag_rows, 0) if ctrl is None else (int(ctrl.row0), int(ctrl.R))
    tail = row0 + R   # the block behind the controlled one: perturbed here (pag_rows), or ordinary rows in this layer
    if ctrl is None:
        if not (1 if bias is None else 0) <= pag_rows <= N:   # without a bias, no perturbed row means no switch is on
            raise _lib.MdmHipError("%s: %d perturbed rows (pag_rows) of a batch of %d" % (what, pag_rows, N))
    else:
        if R < 1 or row0 < 0 or tail > N or pag_rows not in (0, N - tail):
            raise _lib.MdmHipError("%s: edited rows [%d, %d) and %d perturbed rows of a batch of %d (wanted [uncond | sources, "
                                   "edits | perturbed])" % (what, row0, tail, pag_rows, N))
        if any(not 0 <= s < row0 for s in ctrl.src_host):
            raise _lib.MdmHipError("%s: source rows %r outside the leading %d rows" % (what, tuple(ctrl.src_host), row0))
        if bias is not None:
            raise _lib.MdmHipError("%s: a bias together with ctrl_rows -- the controlled rows' cross launches run with a zero "
                                   "bias; mixing biased probabilities is not implemented" % what)
    if bias is not None:
        bias = _check_bias(what, qkv, kvc, bias)
    qkv, kvc = _c(qkv.detach()), _c(kvc.detach() if kvc is not None else None)
    m32 = _c(mask.float()) if (mask is not None and kvc is not None) else None
    _, C, L, S, d = _attn_dims(qkv, kvc, heads)
    out = torch.empty(qkv.shape[:-1] + (C,), dtype=qkv.dtype, device=qkv.device)
    geom = (L, S, heads, d, _dt_mm(qkv))
    kv, m = (kvc, m32) if bias is None else (None, None)   # with a bias mdm_attn_fwd leaves the text keys to the cross launch

    def cross_bias(first, n, on_v):   # the biased text term of the rows [first, first + n): onto v, or in place onto out
        q, o = _row_ptr(qkv, first), _row_ptr(out, first)
        base, base_ld = (q + 2 * C * qkv.element_size(), 3 * C) if on_v else (o, C)
        _cross_bias_launch(geom, q, _row_ptr(kvc, first), _row_ptr(m32, first), _row_ptr(bias, first), bias.shape[-1], base,
                           base_ld, o, n)

    for first, n in ((0, row0), (tail, 0 if pag_rows else N - tail)):   # the ordinary blocks
        if n > 0:
            _fwd_launch(qkv, kv, m, out, first, n, heads)
            if bias is not None:
                cross_bias(first, n, False)
    if R:
        qs, qx = ctrl_gather_qkv(qkv, ctrl.own, ctrl.src, ctrl.gate_s)
        _fwd_launch(qs, None, None, out[row0:tail], 0, R, heads)
        if kvc is not None:
            kv_a, kv_b = ctrl_mix_kv(kvc, ctrl.own, ctrl.src, ctrl.M, ctrl.D, m32, ctrl.gate_c)
            ld = (S + 3) // 4 * 4
            zkey = (qkv.device, R, L, ld)
            zero = _CTRL_ZERO.get(zkey)
            if zero is None:
                if len(_CTRL_ZERO) > 64:
                    _CTRL_ZERO.clear()
                zero = _CTRL_ZERO[zkey] = torch.zeros(R, L, ld, dtype=torch.float32, device=qkv.device)
            m_src = None if m32 is None else m32.reshape(N, S).index_select(0, ctrl.src)
            o = _row_ptr(out, row0)
            _cross_bias_launch(geom, _p(qx), _p(kv_a), _p(m_src), _p(zero), ld, o, C, o, R)
            _cross_bias_launch(geom, _row_ptr(qkv, row0), _p(kv_b), _row_ptr(m32, row0), _p(zero), ld, o, C, o, R)
    if pag_rows and bias is None:
        _cross_addv_launch(qkv, kvc, m32, out, tail, pag_rows, heads)
    elif pag_rows:
        cross_bias(tail, pag_rows, True)
    return out


def attention(qkv, kvc, mask, heads, pag_rows=0, bias=None, ctrl_rows=None):
    """The attention of one layer.  No switch: ``AttentionFn``, with its backward.  ``pag_rows``: the trailing rows get the
    identity self-attention map (``attention_pag``); ``bias``: fp32 [N, L, ld] added to the text logits
    (``attention_biased``); ``ctrl_rows``: prompt-to-prompt control (``attention_controlled``) -- inference only, one batch
    layout and one sequence of launches (``_attn_blocks``)."""
    if not pag_rows and bias is None and ctrl_rows is None:
        return AttentionFn.apply(qkv, kvc, mask, heads, torch.is_grad_enabled())
    return _attn_blocks("attention", qkv, kvc, mask, heads, pag_rows, bias, ctrl_rows)


def attention_pag(qkv, kvc, mask, heads, rows):
    """``attention`` on the leading N - rows batch rows, ``attn_cross_addv`` on the trailing ``rows`` (the perturbed block
    of a perturbed-attention-guidance batch), into one output [N, L, C].  The leading part is the same entry with the same
    B as ``attention`` on that slice alone.  Inference only: the perturbed kernel has no backward."""
    return _attn_blocks("attention_pag", qkv, kvc, mask, heads, rows, None, None)


def attention_biased(qkv, kvc, mask, bias, heads, pag_rows=0):
    """``attention`` with ``bias`` [N, L, ld] added to the text logits (regional prompts, token weights): on the leading
    N - pag_rows batch rows ``mdm_attn_fwd`` without text keys writes the self part and ``mdm_attn_cross_bias`` adds the
    biased cross part in place; the trailing ``pag_rows`` (the perturbed block of perturbed-attention guidance) are the same
    kernel on base = v.  Inference only: the kernel has no backward."""
    return _attn_blocks("attention_biased", qkv, kvc, mask, heads, pag_rows, bias, None)


def attention_controlled(qkv, kvc, mask, heads, ctrl_rows, pag_rows=0):
    """``attention`` of a model batch [uncond | sources, edits | perturbed] under prompt-to-prompt control
    (``mdm_hip.AttnControl``; include/mdm_hip_ext.h): an edited row r computes with the maps of its source row s,
        out_h[r] = A_h(g_s ? s : r) v_h[r] + P_h(s) V'_h[r] + P_h(r) V''_h[r].
    ``ctrl_rows``: the handle of one layer -- ``row0`` / ``R`` (the edited rows are [row0, row0 + R); what follows them is the
    perturbed block: ``pag_rows`` is its size in a layer that perturbs it, 0 in one that runs it as ordinary rows), ``own`` /
    ``src`` (int32 [R] on the device: absolute batch rows), ``src_host`` (the
    source rows again, for the checks), ``M`` fp32 [R, S, ld] and ``D`` fp32 [R, S] (unused without text keys), ``gate_c`` /
    ``gate_s`` (device float[1] each).  Launches: ``mdm_attn_fwd`` with the text keys on the leading ``row0`` rows, exactly as
    ``attention_pag`` runs them; on the edited rows ``mdm_ctrl_gather_qkv``, ``mdm_attn_fwd`` without text keys on what it
    gathered, ``mdm_ctrl_mix_kv`` and two ``mdm_attn_cross_bias`` in place with a zero bias -- (q of s, kv_a, the mask of s),
    then (q of r, kv_b, the mask of r); ``mdm_attn_cross_addv`` on the perturbed rows.  With both gates 0 an edited row has
    the uncontrolled value up to rounding, not bit for bit: its self and text parts are added in another order.  Inference
    only: the cross kernels have no backward."""
    qkv = qkv.reshape(qkv.shape[0], -1, qkv.shape[-1])   # [N, L, 3C]: the output is [N, L, C] whatever the rank of qkv
    return _attn_blocks("attention_controlled", qkv, kvc, mask, heads, pag_rows, None, ctrl_rows)


@torch.no_grad()
def attn_cross_maps(qkv, kvc, mask, heads, acc, bias=None, weight=1.0, gate=None, row0=0, rows=None):
    """acc[r - row0] += weight * gate / heads * sum_h softmax(q_h k_c,h^T / sqrt(d) [+ bias] [masked; bias <= -1e30
    excludes]) for the batch rows r in [row0, row0 + rows) of ``qkv`` [N, L, 3C] / ``kvc`` [N, S, 2C] / ``mask`` [N, S] /
    ``bias`` (fp32 [N, L, ld], as ``attn_cross_bias`` takes it) -- the probabilities of the text cross-attention, mean over
    heads (include/mdm_hip_ext.h mdm_attn_cross_maps).  ``acc``: fp32 [rows, L, ld], ld >= S, ld % 4 == 0, contiguous,
    updated in place and returned; its columns [S, ld) are left alone.  ``gate``: a device float[1] or None (= 1) -- 0
    leaves ``acc`` untouched, which lets one captured graph skip steps.  Reads detached values under no_grad: legal inside
    a forward that records autograd.  CPU tensors: ``attn_maps.cross_maps``."""
    _require_gpu(qkv)
    if kvc is None:
        raise _lib.MdmHipError("attn_cross_maps: no text keys (kvc is None) -- there is no cross-attention to record")
    qkv, kvc = _c(qkv.detach()), _c(kvc.detach())
    N, C, L, S, d = _attn_dims(qkv, kvc, heads)
    row0 = int(row0)
    rows = N - row0 if rows is None else int(rows)
    if not (0 <= row0 and 0 < rows and row0 + rows <= N):
        raise _lib.MdmHipError("attn_cross_maps: rows [%d, %d) of a batch of %d" % (row0, row0 + rows, N))
    _check_f32_3d("attn_cross_maps", "acc", acc, rows, L, S, qkv.device)
    if bias is not None:
        bias = _check_bias("attn_cross_maps", qkv, kvc, bias)
    if gate is not None:
        _check_gate("attn_cross_maps", gate, qkv.device)
    m32 = _c(mask.detach().float()) if mask is not None else None
    _prof_wrap("attn_cross_maps_kernel<d=%d> L=%d" % (d, L), 2.0 * rows * heads * L * S * d, lambda: _lib.check(
        _lib.lib().mdm_attn_cross_maps(_row_ptr(qkv, row0), _row_ptr(kvc, row0), _row_ptr(m32, row0), _row_ptr(bias, row0),
                                       0 if bias is None else bias.shape[-1], _p(acc), acc.shape[-1], float(weight), _p(gate),
                                       rows, L, S, heads, d, _dt_mm(qkv), _stream()),
        "mdm_attn_cross_maps",
    ), kind="attn")
    return acc


def _cross_probs_check(what, qkv, kvc, mask, heads, row0, rows):
    """the operands of mdm_attn_cross_maps / mdm_attn_cross_maps_bwd as ``attn_cross_probs`` takes them -> (row0, rows)"""
    _require_gpu(qkv)
    if kvc is None:
        raise _lib.MdmHipError("%s: no text keys (kvc is None) -- there is no cross-attention to differentiate" % what)
    if torch.is_grad_enabled() and kvc.requires_grad:
        raise _lib.MdmHipError("%s: kvc requires grad, and mdm_attn_cross_maps_bwd forms the gradient of q only -- gradients "
                               "to the text keys are not implemented: detach kvc, or freeze what makes it" % what)
    if qkv.dim() < 3 or qkv.shape[-1] % 3 or kvc.dim() != 3 or kvc.shape[0] != qkv.shape[0] or \
            2 * (qkv.shape[-1] // 3) != kvc.shape[-1] or kvc.dtype != qkv.dtype or kvc.device != qkv.device:
        raise _lib.MdmHipError("%s: qkv %s %s and kvc %s %s (wanted [N, L, 3C] and [N, S, 2C] of one dtype on one device)"
                               % (what, tuple(qkv.shape), qkv.dtype, tuple(kvc.shape), kvc.dtype))
    N, C = qkv.shape[0], qkv.shape[-1] // 3
    if heads < 1 or C % heads:
        raise _lib.MdmHipError("%s: %d heads for C = %d" % (what, heads, C))
    if mask is not None and (mask.numel() != N * kvc.shape[1] or mask.shape[0] != N or mask.device != qkv.device):
        raise _lib.MdmHipError("%s: mask %s on %s for N = %d, S = %d" % (what, tuple(mask.shape), mask.device, N, kvc.shape[1]))
    row0 = int(row0)
    rows = N - row0 if rows is None else int(rows)
    if not (0 <= row0 and 0 < rows and row0 + rows <= N):
        raise _lib.MdmHipError("%s: rows [%d, %d) of a batch of %d" % (what, row0, row0 + rows, N))
    return row0, rows


def attn_cross_maps_bwd(qkv, kvc, mask, heads, dacc, dqkv, weight=1.0, row0=0, rows=None):
    """The q columns of the batch rows [row0, row0 + rows) of ``dqkv`` (shaped and typed like ``qkv`` [N, L, 3C],
    contiguous) <- the gradient of ``weight`` x the head-mean text probabilities of those rows with respect to q, given
    ``dacc`` fp32 [rows, L, ld] (ld >= S, ld % 4 == 0; the columns [S, ld) and the entries of masked keys may hold
    anything): include/mdm_hip_ext.h mdm_attn_cross_maps_bwd.  Nothing else of ``dqkv`` is touched.  -> dqkv"""
    row0, rows = _cross_probs_check("attn_cross_maps_bwd", qkv, kvc, mask, heads, row0, rows)
    qkv, kvc = _c(qkv.detach()), _c(kvc.detach())
    N, C, L, S, d = _attn_dims(qkv, kvc, heads)
    _check_f32_3d("attn_cross_maps_bwd", "dacc", dacc, rows, L, S, qkv.device)
    if (dqkv.numel() != qkv.numel() or dqkv.shape[0] != N or dqkv.shape[-1] != 3 * C or dqkv.dtype != qkv.dtype
            or not dqkv.is_contiguous() or dqkv.device != qkv.device):
        raise _lib.MdmHipError("attn_cross_maps_bwd: dqkv %s %s (wanted a contiguous %s %s)"
                               % (tuple(dqkv.shape), dqkv.dtype, tuple(qkv.shape), qkv.dtype))
    m32 = _c(mask.detach().float()) if mask is not None else None
    flops = (4.0 if S <= 64 else 6.0) * rows * heads * L * S * d   # QK^T per sweep (one, or two beyond a key tile) + dS K
    _prof_wrap("attn_cross_maps_bwd_kernel<d=%d> L=%d" % (d, L), flops, lambda: _lib.check(
        _lib.lib().mdm_attn_cross_maps_bwd(_row_ptr(qkv, row0), _row_ptr(kvc, row0), _row_ptr(m32, row0), _p(dacc.detach()),
                                           dacc.shape[-1], float(weight), _row_ptr(dqkv, row0), L * 3 * C, 3 * C, rows, L, S,
                                           heads, d, _dt_mm(qkv), _stream()),
        "mdm_attn_cross_maps_bwd",
    ), kind="attn")
    return dqkv


class AttnCrossProbsFn(torch.autograd.Function):
    """the head-mean text probabilities of a row range, differentiable in qkv: mdm_attn_cross_maps onto zeros forward,
    mdm_attn_cross_maps_bwd into the q columns of a zero qkv-shaped gradient backward; kvc and the mask are constants"""

    @staticmethod
    def forward(ctx, qkv, kvc, mask, heads, row0, rows):
        qd, kd = _c(qkv.detach()), _c(kvc.detach())
        _, _, L, S, _ = _attn_dims(qd, kd, heads)
        acc = torch.zeros(rows, L, (S + 3) // 4 * 4, dtype=torch.float32, device=qd.device)
        attn_cross_maps(qd, kd, mask, heads, acc, row0=row0, rows=rows)
        ctx.save_for_backward(qd, kd, mask)
        ctx.geom = (heads, row0, rows)
        return acc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dacc):
        qd, kd, mask = ctx.saved_tensors
        heads, row0, rows = ctx.geom
        dqkv = torch.zeros_like(qd)
        attn_cross_maps_bwd(qd, kd, mask, heads, _c(dacc.float()), dqkv, row0=row0, rows=rows)
        return dqkv, None, None, None, None, None


def attn_cross_probs(qkv, kvc, mask, heads, row0=0, rows=None):
    """-> fp32 [rows, L, ld], ld = S rounded up to 4 with zero pad columns: the probabilities of the text cross-attention,
    mean over heads, of the batch rows [row0, row0 + rows) of ``qkv`` [N, L, 3C] / ``kvc`` [N, S, 2C] / ``mask`` [N, S] --
    bit for bit what ``attn_cross_maps`` adds onto zeros -- and DIFFERENTIABLE in ``qkv``: the backward fills the q columns
    of those rows of a zero qkv-shaped gradient (include/mdm_hip_ext.h mdm_attn_cross_maps_bwd).  ``kvc`` and ``mask`` are
    constants: a ``kvc`` that requires grad is refused under grad mode.  No bias: a biased map has no backward.  CPU
    tensors: ``attn_maps.cross_probs``."""
    row0, rows = _cross_probs_check("attn_cross_probs", qkv, kvc, mask, heads, row0, rows)
    return AttnCrossProbsFn.apply(qkv, kvc.detach(), mask, heads, row0, rows)


# --------------------------------------------------------------------------------------
# streaming helpers
# --------------------------------------------------------------------------------------
class ToNHWCFn(torch.autograd.Function):
    """fp32 NCHW (reference layout) -> compute-dtype NHWC with zero channel padding."""

    @staticmethod
    def forward(ctx, x, dtype, cpad):
        _require_gpu(x)
        x = _c(x.float())
        N, C, H, W = x.shape
        y = torch.empty((N, H, W, cpad), dtype=dtype, device=x.device)
        _lib.check(_lib.lib().mdm_nchw_to_nhwc(_p(x), _p(y), N, C, H, W, cpad, _dt(y), _stream()), "mdm_nchw_to_nhwc")
        ctx.C = C
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        N, H, W, Cs = dy.shape
        dx = torch.empty((N, ctx.C, H, W), dtype=torch.float32, device=dy.device)
        _lib.check(_lib.lib().mdm_nhwc_to_nchw(_p(dy), _p(dx), N, ctx.C, H, W, Cs, _dt(dy), _stream()), "mdm_nhwc_to_nchw")
        return dx, None, None


class FromNHWCFn(torch.autograd.Function):
    """compute-dtype NHWC (first C channels) -> fp32 NCHW."""

    @staticmethod
    def forward(ctx, x, C):
        _require_gpu(x)
        x = _c(x)
        N, H, W, Cs = x.shape
        y = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().mdm_nhwc_to_nchw(_p(x), _p(y), N, C, H, W, Cs, _dt(x), _stream()), "mdm_nhwc_to_nchw")
        ctx.Cs, ctx.dtype = Cs, x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy.float())
        N, C, H, W = dy.shape
        dx = torch.empty((N, H, W, ctx.Cs), dtype=ctx.dtype, device=dy.device)
        _lib.check(_lib.lib().mdm_nchw_to_nhwc(_p(dy), _p(dx), N, C, H, W, ctx.Cs, _dt(dx), _stream()), "mdm_nchw_to_nhwc")
        return dx, None


def to_nhwc(x_nchw, dtype, cpad=None):
    epv = 4 if dtype == torch.float32 else 8
    cpad = _round_up(x_nchw.shape[1], epv) if cpad is None else cpad
    return ToNHWCFn.apply(x_nchw, dtype, cpad)


def from_nhwc(x, C):
    return FromNHWCFn.apply(x, C)


class ConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_gpu(a)
        a, b = _c(a), _c(b)
        C1, C2 = a.shape[-1], b.shape[-1]
        M = a.numel() // C1
        out = torch.empty(a.shape[:-1] + (C1 + C2,), dtype=a.dtype, device=a.device)
        _prof_wrap("concat", 2.0 * out.numel() * out.element_size(),
                   lambda: _lib.check(_lib.lib().mdm_concat(_p(a), _p(b), _p(out), M, C1, C2, 0, _dt(a), _stream()), "mdm_concat"), kind="hbm")
        ctx.C1, ctx.C2 = C1, C2
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _c(dout)
        C1, C2 = ctx.C1, ctx.C2
        M = dout.numel() // (C1 + C2)
        da = torch.empty(dout.shape[:-1] + (C1,), dtype=dout.dtype, device=dout.device)
        db = torch.empty(dout.shape[:-1] + (C2,), dtype=dout.dtype, device=dout.device)
        _lib.check(_lib.lib().mdm_concat(_p(da), _p(db), _p(dout), M, C1, C2, 1, _dt(dout), _stream()), "mdm_concat")
        return da, db


def concat(a, b):
    return ConcatFn.apply(a, b)


_freeu_plans = {}   # (N, H, W, C1, C2, dtype code, structure) -> workspace bytes of mdm_freeu_plan


def concat_freeu(x, skip, b, s, structure=False, layer=None):
    """``concat(x, skip)`` with FreeU (Si et al., CVPR 2024) applied to both on the way (include/mdm_hip_ext.h
    mdm_freeu_stats + mdm_freeu_apply): the first C1 / 2 channels of the backbone ``x`` [N, H, W, C1] times ``b`` (with
    ``structure``, FreeU v2: times 1 + (b - 1) hm, hm the per-sample min-max normalised channel mean of x), and the 2 x 2
    lowest spatial frequencies of ``skip`` [N, H, W, C2] times ``s``.  b = s = 1 is ``concat`` bit for bit.  ``layer``: the
    name an error message gives.  Forward only: the kernels have no backward."""
    _require_gpu(x)
    _require_gpu(skip)
    what = "concat_freeu" if layer is None else "concat_freeu (%s)" % layer
    if torch.is_grad_enabled() and (x.requires_grad or skip.requires_grad):
        raise _lib.MdmHipError("%s is inference only (mdm_freeu_apply has no backward): run it under torch.no_grad()" % what)
    if x.dim() != 4 or skip.dim() != 4 or x.shape[:3] != skip.shape[:3] or x.dtype != skip.dtype or x.device != skip.device:
        raise _lib.MdmHipError("%s: backbone %s %s and skip %s %s (wanted NHWC tensors of one dtype that differ in C only)"
                               % (what, tuple(x.shape), x.dtype, tuple(skip.shape), skip.dtype))
    b, s, structure = float(b), float(s), bool(structure)
    if not (0 < b < float("inf")) or not (0 <= s < float("inf")):
        raise _lib.MdmHipError("%s: b = %r, s = %r (wanted finite b > 0 and s >= 0)" % (what, b, s))
    N, H, W, C1 = x.shape
    C2 = skip.shape[-1]
    if H < 2 or W < 2:
        raise _lib.MdmHipError("%s: a %d x %d feature map -- the closed form of the Fourier filter needs H, W >= 2" % (what, H, W))
    epv = _epv(x)
    if C1 % (2 * epv) or C2 % epv or C1 == 0 or C2 == 0:
        raise _lib.MdmHipError("%s: C1 = %d, C2 = %d in %s (wanted C1 %% %d == 0 and C2 %% %d == 0)"
                               % (what, C1, C2, x.dtype, 2 * epv, epv))
    x, skip = _c(x.detach()), _c(skip.detach())
    L, dt = _lib.lib(), _dt(x)
    key = (N, H, W, C1, C2, dt, structure)
    wsb = _freeu_plans.get(key)
    if wsb is None:
        v = ctypes.c_size_t(0)
        _lib.check(L.mdm_freeu_plan(N, H, W, C1, C2, dt, int(structure), ctypes.byref(v)), what + ": mdm_freeu_plan")
        wsb = _freeu_plans[key] = v.value
    ws = _f32_ws(wsb, x.device)
    out = torch.empty((N, H, W, C1 + C2), dtype=x.dtype, device=x.device)
    esz = x.element_size()
    _prof_wrap("freeu_stats", float((skip.numel() + (x.numel() if structure else 0)) * esz), lambda: _lib.check(
        L.mdm_freeu_stats(_p(x), _p(skip), _p(ws), wsb, N, H, W, C1, C2, int(structure), dt, _stream()),
        what + ": mdm_freeu_stats"), kind="hbm")
    _prof_wrap("freeu_apply", 2.0 * out.numel() * esz, lambda: _lib.check(
        L.mdm_freeu_apply(_p(x), _p(skip), _p(ws), wsb, _p(out), N, H, W, C1, C2, b, s, int(structure), dt, _stream()),
        what + ": mdm_freeu_apply"), kind="hbm")
    return out


class Upsample2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        x = _c(x)
        N, H, W, C = x.shape
        y = torch.empty((N, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().mdm_upsample2x(_p(x), _p(y), N, H, W, C, _dt(x), _stream()), "mdm_upsample2x")
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        N, H2, W2, C = dy.shape
        dx = torch.empty((N, H2 // 2, W2 // 2, C), dtype=dy.dtype, device=dy.device)
        _lib.check(_lib.lib().mdm_downsum2x(_p(dy), _p(dx), N, H2 // 2, W2 // 2, C, _dt(dy), _stream()), "mdm_downsum2x")
        return dx


def upsample2x(x):
    return Upsample2xFn.apply(x)


def _ew(a, b, op):
    out = torch.empty_like(a)
    _lib.check(_lib.lib().mdm_elementwise(_p(a), _p(b), _p(out), a.numel(), op, _dt(a), _stream()), "mdm_elementwise")
    return out


class SiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        x = _c(x)
        ctx.save_for_backward(x)
        return _ew(x, None, 0)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _ew(x, _c(dy), 1)


def silu(x):
    return SiluFn.apply(x)


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_gpu(a)
        return _ew(_c(a), _c(b), 2)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        raise _lib.MdmHipError("add: shape/dtype mismatch %s %s vs %s %s" % (a.shape, a.dtype, b.shape, b.dtype))
    return AddFn.apply(a, b)


class CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        _require_gpu(x)
        x = _c(x)
        ctx.src = x.dtype
        if x.dtype == dtype:
            return x.view_as(x)
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        _lib.check(_lib.lib().mdm_cast(_p(x), _p(y), x.numel(), _dt(x), _dt(y), _stream()), "mdm_cast")
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy.dtype == ctx.src:
            return dy, None
        dy = _c(dy)
        dx = torch.empty(dy.shape, dtype=ctx.src, device=dy.device)
        _lib.check(_lib.lib().mdm_cast(_p(dy), _p(dx), dy.numel(), _dt(dy), _dt(dx), _stream()), "mdm_cast")
        return dx, None


def cast(x, dtype):
    return CastFn.apply(x, dtype)


def sincos_embedding(times_f32, freqs_f32, dtype):
    """[B] x [half] -> [B, 2*half] = (sin | cos); no gradient (unet.py:835-836)."""
    _require_gpu(times_f32)
    t = _c(times_f32.detach().float())
    f = _c(freqs_f32.detach().float().reshape(-1))
    B, half = t.numel(), f.numel()
    out = torch.empty((B, 2 * half), dtype=dtype, device=t.device)
    _lib.check(_lib.lib().mdm_sincos_emb(_p(t), _p(f), _p(out), B, half, _dt(out), _stream()), "mdm_sincos_emb")
    return out


class MaskedMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        _require_gpu(x)
        x = _c(x)
        B, S, D = x.shape
        m32 = _c(mask.float()) if mask is not None else None
        y = torch.empty((B, D), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().mdm_masked_mean(_p(x), _p(m32), _p(y), B, S, D, _dt(x), _stream()), "mdm_masked_mean")
        ctx.save_for_backward(m32)
        ctx.shape = (B, S, D)
        return y

    @staticmethod
    def backward(ctx, dy):
        (m32,) = ctx.saved_tensors
        dy = _c(dy)
        B, S, D = ctx.shape
        dx = torch.empty((B, S, D), dtype=dy.dtype, device=dy.device)
        _lib.check(_lib.lib().mdm_masked_mean_bwd(_p(dy), _p(m32), _p(dx), B, S, D, 0, _dt(dy), _stream()), "mdm_masked_mean_bwd")
        return dx, None


def masked_mean(x, mask):
    return MaskedMeanFn.apply(x, mask)


# --------------------------------------------------------------------------------------
# per-pixel arithmetic around the denoiser: NCHW fp32 images (row a7 x / std)
# --------------------------------------------------------------------------------------
def _img(t):
    """fp32, contiguous, on the GPU"""
    _require_gpu(t)
    t = t.detach()
    if t.dtype != torch.float32:
        raise _lib.MdmHipError("image-side ops take fp32 tensors (got %s)" % t.dtype)
    return _c(t)


def _vec(t, B):
    """per-sample scalars ([B], [B,1,1,1] ...) -> contiguous fp32 [B] on the GPU"""
    t = _c(t.detach().reshape(-1).float())
    if t.numel() != B:
        raise _lib.MdmHipError("expected %d per-sample values, got %d" % (B, t.numel()))
    return t


class DeviceRng:
    """{seed, offset} of the library's counter-based normal generator (Philox4x32-10 + Box-Muller), kept ON THE DEVICE so
    that draws and advances are plain stream work (capturable in a hipGraph).  Element i of a draw is lane i & 3 of
    counter block offset + i // 4; oracle/philox_ref.py regenerates the same numbers on the host."""

    def __init__(self, seed: int, device, offset: int = 0):
        self.state = torch.tensor([seed & (2**63 - 1), offset], dtype=torch.int64, device=device)

    def advance(self, n_elements: int):
        _lib.check(_lib.lib().mdm_rng_advance(_p(self.state), (int(n_elements) + 3) // 4, _stream()), "mdm_rng_advance")

    def randn(self, shape, stream_id: int = 0):
        out = torch.empty(shape, dtype=torch.float32, device=self.state.device)
        n = out.numel()
        if n % 4:
            raise _lib.MdmHipError("randn: element count must be a multiple of 4")
        _lib.check(_lib.lib().mdm_randn(_p(out), n, _p(self.state), stream_id, _stream()), "mdm_randn")
        self.advance(n)
        return out


_PT = {"DDPM": 0, "DDIM": 1, "V_PREDICTION": 2}


def _ptype(pt):
    return _PT[pt.name] if hasattr(pt, "name") else int(pt)


def sampler_step(x_t, pred, g, g_last, prediction_type, ddim_eta=None, need_noise=False, noise=None, rng=None,
                 rng_stream=0, clip="CLIP", image_scale=1.0, pred_uncond=None, guidance_scale=1.0, thr=None,
                 noise_gate=None):
    """One reverse-diffusion update (reference samplers.py:281-345 + 445-456 + 500-508) as ONE kernel.
    -> (x0, x_last).  ``clip``: "NONE" | "CLIP" | "DYNAMIC" (needs ``thr`` [B]) | "X0_ONLY" (returns the unclipped
    x0 * image_scale and None: the input of the dynamic-threshold quantile)."""
    x_t, pred = _img(x_t), _img(pred)
    B = x_t.shape[0]
    chw = x_t.numel() // B
    g, gl = _vec(g, B), _vec(g_last, B)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    nz = _img(noise) if noise is not None else None
    th = _vec(thr, B) if thr is not None else None
    gate = _c(noise_gate.detach().reshape(-1).float()) if noise_gate is not None else None
    cm = {"NONE": 0, "CLIP": 1, "DYNAMIC": 2, "X0_ONLY": 3}[clip]
    x0 = torch.empty_like(x_t)
    xl = torch.empty_like(x_t) if cm != 3 else None
    mode, eta = (0, 0.0) if ddim_eta is None else (1, float(ddim_eta))
    gen = bool(need_noise) and nz is None and not (mode == 1 and eta <= 0)
    if gen and rng is None:
        raise _lib.MdmHipError("sampler_step: need_noise without noise= or rng=")
    _lib.check(
        _lib.lib().mdm_sampler_step(_p(x_t), _p(pred), _p(pu), float(guidance_scale), _p(g), _p(gl), _p(nz), _p(gate), _p(th),
                                    _p(rng.state) if rng is not None else None, int(rng_stream), _p(x0), _p(xl), B, chw,
                                    _ptype(prediction_type), mode, eta, 1 if need_noise else 0, cm,
                                    float(image_scale) if image_scale else 1.0, _stream()),
        "mdm_sampler_step",
    )
    return x0, xl


_ORDER_ON = {}   # device -> float[1] of 1.0: the order gate of an eager second-order step (no fill launch per step)


def sampler_step_2m(x_t, pred, g, g_last, prediction_type, g_prev=None, x0_prev=None, second_order=False, clip="CLIP",
                    image_scale=1.0, pred_uncond=None, guidance_scale=1.0, thr=None, x0_out=None):
    """One DPM-Solver++(2M) update (Lu et al. 2022, multistep, data prediction; include/mdm_hip.h) as ONE kernel.
    -> (x0, x_last).  ``second_order``: False / True, or a device float[1] gate (0 = first order) so that one captured
    graph serves every step.  Second order needs ``x0_prev`` and ``g_prev`` (the x0 of the step before and the gamma
    it was formed at).  ``x0_out`` may be ``x0_prev`` itself: the history is then updated in place.
    ``clip``: "NONE" | "CLIP" | "DYNAMIC" (needs ``thr`` [B], from ``sampler_step(clip="X0_ONLY")`` + ``abs_quantile``)."""
    x_t, pred = _img(x_t), _img(pred)
    B = x_t.shape[0]
    chw = x_t.numel() // B
    g, gl = _vec(g, B), _vec(g_last, B)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    th = _vec(thr, B) if thr is not None else None
    cm = {"NONE": 0, "CLIP": 1, "DYNAMIC": 2}[clip]
    gate = gp = xp = None
    if torch.is_tensor(second_order):
        gate = _c(second_order.detach().reshape(-1).float())
        _require_gpu(gate)
    elif second_order:
        gate = _ORDER_ON.get(x_t.device)
        if gate is None:
            gate = _ORDER_ON[x_t.device] = torch.ones(1, dtype=torch.float32, device=x_t.device)
    if gate is not None:
        if x0_prev is None or g_prev is None:
            raise _lib.MdmHipError("sampler_step_2m: second order needs x0_prev= and g_prev=")
        xp, gp = _img(x0_prev), _vec(g_prev, B)
        if xp.shape != x_t.shape:
            raise _lib.MdmHipError("sampler_step_2m: x0_prev %s vs x_t %s" % (tuple(xp.shape), tuple(x_t.shape)))
    if x0_out is None:
        x0 = torch.empty_like(x_t)
    else:
        x0 = x0_out
        _require_gpu(x0)
        if x0.dtype != torch.float32 or not x0.is_contiguous() or x0.shape != x_t.shape:
            raise _lib.MdmHipError("sampler_step_2m: x0_out must be a contiguous fp32 tensor shaped like x_t")
    xl = torch.empty_like(x_t)
    _lib.check(
        _lib.lib().mdm_sampler_step_2m(_p(x_t), _p(pred), _p(pu), float(guidance_scale), _p(g), _p(gl), _p(gp), _p(gate),
                                       _p(th), _p(xp), _p(x0), _p(xl), B, chw, _ptype(prediction_type), cm,
                                       float(image_scale) if image_scale else 1.0, _stream()),
        "mdm_sampler_step_2m",
    )
    return x0, xl


_SA_GATES = {}   # (device, (p, c, tau, tau_corr)) -> device float[4]: an eager trajectory meets a handful of them


def sa_gate(device, predictor, corrector, tau=0.0, tau_corr=0.0):
    """the device float[4] gate of ``sampler_step_sa`` for host values, checked and cached per device"""
    if int(predictor) != predictor or not 1 <= predictor <= 3:
        raise ValueError("sampler_step_sa: predictor order %r (wanted 1, 2 or 3)" % (predictor,))
    if int(corrector) != corrector or not 0 <= corrector <= 3:
        raise ValueError("sampler_step_sa: corrector order %r (wanted 0 .. 3)" % (corrector,))
    if not (tau >= 0 and tau_corr >= 0):
        raise ValueError("sampler_step_sa: tau = %r, %r (wanted >= 0)" % (tau, tau_corr))
    key = (torch.device(device), (int(predictor), int(corrector), float(tau), float(tau_corr)))
    gate = _SA_GATES.get(key)
    if gate is None:
        gate = _SA_GATES[key] = torch.tensor(key[1], dtype=torch.float32, device=device)
    return gate


def sampler_step_sa(x_t, pred, g, g_last, prediction_type, gate, h0=None, h1=None, psum=None, g_h0=None, g_h1=None,
                    max_predictor=3, max_corrector=3, noise=None, rng=None, rng_stream=0, clip="CLIP", image_scale=1.0,
                    pred_uncond=None, guidance_scale=1.0, thr=None, x0_out=None):
    """One SA-Solver update (Xue et al. 2023; include/mdm_hip_ext.h has the definition) as ONE kernel -> (x0, x_last).
    ``gate``: (predictor order, corrector order, tau, tau of the corrected step) as host numbers, or a device float[4]
    so that one captured graph serves every step; the orders are clamped to ``max_predictor`` / ``max_corrector``, which
    also say which of the state the call needs.  ``h0`` / ``h1``: the x0 of the two steps before, formed at ``g_h0`` /
    ``g_h1``; ``psum``: the predictor's sum the launch before stored.  All three are updated IN PLACE (h1 <- h0,
    h0 <- x0, psum <- this launch's sum).  ``x0_out`` may be ``h0`` itself.  ``noise``, or ``rng`` (drawn in the kernel;
    the caller advances it by ``x_t.numel()``): the z of tau > 0; with neither, tau counts as 0.
    ``clip``: as ``sampler_step_2m``."""
    x_t, pred = _img(x_t), _img(pred)
    B = x_t.shape[0]
    chw = x_t.numel() // B
    g, gl = _vec(g, B), _vec(g_last, B)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    nz = _img(noise) if noise is not None else None
    th = _vec(thr, B) if thr is not None else None
    cm = {"NONE": 0, "CLIP": 1, "DYNAMIC": 2}[clip]
    if int(max_predictor) != max_predictor or int(max_corrector) != max_corrector:
        raise _lib.MdmHipError("sampler_step_sa: orders are integers (got %r, %r)" % (max_predictor, max_corrector))
    if torch.is_tensor(gate):
        gate = _c(gate.detach().reshape(-1).float())
        _require_gpu(gate)
        if gate.numel() != 4:
            raise _lib.MdmHipError("sampler_step_sa: the gate is a device float[4] (got %d values)" % gate.numel())
    else:
        gate = sa_gate(x_t.device, *gate)
    state = lambda t, what: None if t is None else _inplace_img(t, x_t, "sampler_step_sa: " + what)
    h0, h1, psum = state(h0, "h0"), state(h1, "h1"), state(psum, "psum")
    g0 = _vec(g_h0, B) if g_h0 is not None else None
    g1 = _vec(g_h1, B) if g_h1 is not None else None
    x0 = torch.empty_like(x_t) if x0_out is None else _inplace_img(x0_out, x_t, "sampler_step_sa: x0_out")
    xl = torch.empty_like(x_t)
    _lib.check(
        _lib.lib().mdm_sampler_step_sa(_p(x_t), _p(pred), _p(pu), float(guidance_scale), _p(g), _p(gl), _p(g0), _p(g1),
                                       _p(gate), _p(th), _p(nz), _p(rng.state) if rng is not None else None,
                                       int(rng_stream), _p(h0), _p(h1), _p(psum), _p(x0), _p(xl), B, chw,
                                       _ptype(prediction_type), cm, float(image_scale) if image_scale else 1.0,
                                       int(max_predictor), int(max_corrector), _stream()),
        "mdm_sampler_step_sa",
    )
    return x0, xl


def _inplace_img(t, like, what):
    """an fp32, contiguous GPU tensor shaped like ``like`` that a kernel writes through its own pointer (no copy made)"""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != like.shape:
        raise _lib.MdmHipError("%s must be a contiguous fp32 tensor of shape %s" % (what, tuple(like.shape)))
    _require_gpu(t)
    return t.detach()


def sampler_known_blend(x, known, mask, g, inv_scale=1.0, noise=None, rng=None, rng_stream=1):
    """Known-region replacement (RePaint, Lugmayr et al. 2022; include/mdm_hip.h) as ONE kernel, IN PLACE on ``x``
    [B, C, H, W], the state at noise level ``g`` [B]:  k = sqrt(g) known inv_scale + sqrt(1 - g) n;  x = k where
    ``mask`` [B, 1, H, W] is 1, untouched where it is 0, m k + (1 - m) x in between.  ``n`` is ``noise``, or drawn in
    the kernel from ``rng`` (which the caller advances by ``x.numel()``, as for ``sampler_step``).  -> x"""
    if x.dim() != 4:
        raise _lib.MdmHipError("sampler_known_blend: x must be [B, C, H, W] (got %s)" % (tuple(x.shape),))
    B, C, H, W = x.shape
    if known.shape != x.shape:
        raise _lib.MdmHipError("sampler_known_blend: known %s vs x %s" % (tuple(known.shape), tuple(x.shape)))
    if tuple(mask.shape) != (B, 1, H, W):
        raise _lib.MdmHipError("sampler_known_blend: mask must be %s (got %s)" % ((B, 1, H, W), tuple(mask.shape)))
    if (H * W) % 4:
        raise _lib.MdmHipError("sampler_known_blend: H * W must be a multiple of 4 (got %d x %d)" % (H, W))
    x = _inplace_img(x, x, "sampler_known_blend: x")
    known, mask = _img(known), _img(mask)
    g = _vec(g, B)
    nz = _img(noise) if noise is not None else None
    if nz is not None and nz.shape != x.shape:
        raise _lib.MdmHipError("sampler_known_blend: noise %s vs x %s" % (tuple(nz.shape), tuple(x.shape)))
    if nz is None and rng is None:
        raise _lib.MdmHipError("sampler_known_blend: give noise= or rng=")
    _lib.check(
        _lib.lib().mdm_sampler_known_blend(_p(x), _p(known), _p(mask), _p(g), float(inv_scale), _p(nz),
                                           _p(rng.state) if nz is None else None, int(rng_stream), B, C, H * W, _stream()),
        "mdm_sampler_known_blend",
    )
    return x


def sampler_jump(x_s, g_t, g_s, noise=None, rng=None, rng_stream=1, gate=None, out=None):
    """The forward transition of a resampling jump, level ``g_s`` back to the noisier ``g_t`` ([B] each), as ONE kernel:
    x_t = sqrt(g_t / g_s) x_s + sqrt(1 - g_t / g_s) n.  ``gate``: a device float[1] (0 = x_t is x_s, no noise) so that
    one captured graph serves every iteration; None = on.  ``out`` may be ``x_s`` itself.  The caller advances ``rng``.
    -> x_t"""
    x_s = _img(x_s)
    B = x_s.shape[0]
    chw = x_s.numel() // B
    if chw % 4:
        raise _lib.MdmHipError("sampler_jump: C * H * W must be a multiple of 4 (got %s)" % (tuple(x_s.shape),))
    g_t, g_s = _vec(g_t, B), _vec(g_s, B)
    nz = _img(noise) if noise is not None else None
    if nz is not None and nz.shape != x_s.shape:
        raise _lib.MdmHipError("sampler_jump: noise %s vs x_s %s" % (tuple(nz.shape), tuple(x_s.shape)))
    if nz is None and rng is None:
        raise _lib.MdmHipError("sampler_jump: give noise= or rng=")
    if gate is not None:
        gate = _c(gate.detach().reshape(-1).float())
        _require_gpu(gate)
    out = torch.empty_like(x_s) if out is None else _inplace_img(out, x_s, "sampler_jump: out")
    _lib.check(
        _lib.lib().mdm_sampler_jump(_p(x_s), _p(g_t), _p(g_s), _p(nz), _p(gate), _p(rng.state) if nz is None else None,
                                    int(rng_stream), _p(out), B, chw, _stream()),
        "mdm_sampler_jump",
    )
    return out


def sampler_invert_step(x_s, pred, g_s, g_t, prediction_type, pred_uncond=None, guidance_scale=1.0, out=None):
    """The preimage of one DDIM(0) step with the prediction held fixed (include/mdm_hip_ext.h mdm_sampler_invert_step) as ONE
    kernel: from ``x_s`` at the cleaner level ``g_s`` to the x_t at ``g_t`` ([B] each, g_s > g_t; g_s == 1 allowed) that
    ``sampler_step(ddim_eta=0, clip="NONE")`` with the same prediction maps back to ``x_s``.  No threshold.  ``out``: the
    buffer x_t is written to (it aliases nothing).  -> x_t"""
    x_s, pred = _img(x_s), _img(pred)
    B = x_s.shape[0]
    chw = x_s.numel() // B
    if chw % 4:
        raise _lib.MdmHipError("sampler_invert_step: C * H * W must be a multiple of 4 (got %s)" % (tuple(x_s.shape),))
    if pred.shape != x_s.shape:
        raise _lib.MdmHipError("sampler_invert_step: pred %s vs x_s %s" % (tuple(pred.shape), tuple(x_s.shape)))
    g_s, g_t = _vec(g_s, B), _vec(g_t, B)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    if pu is not None and pu.shape != x_s.shape:
        raise _lib.MdmHipError("sampler_invert_step: pred_uncond %s vs x_s %s" % (tuple(pu.shape), tuple(x_s.shape)))
    out = torch.empty_like(x_s) if out is None else _inplace_img(out, x_s, "sampler_invert_step: out")
    _lib.check(
        _lib.lib().mdm_sampler_invert_step(_p(x_s), _p(pred), _p(pu), float(guidance_scale), _p(g_s), _p(g_t), _p(out), B, chw,
                                           _ptype(prediction_type), _stream()),
        "mdm_sampler_invert_step",
    )
    return out


def sampler_noise_map(x_t, x_s, pred, g, g_last, prediction_type, ddim_eta=None, clip="CLIP", image_scale=1.0,
                      pred_uncond=None, guidance_scale=1.0, thr=None):
    """The noise of one ancestral step solved for (include/mdm_hip_ext.h mdm_sampler_noise_map) as ONE kernel:
    z = (x_s - mu) / sigma with mu and sigma those of ``sampler_step`` on (x_t, pred) with the same arguments, so that
    ``sampler_step(..., need_noise=True, noise=z)`` maps ``x_t`` to ``x_s``; z = 0 for a sample with ``g_last == 1``.
    ``ddim_eta``: None (the DDPM posterior) or > 0.  ``clip``: "NONE" | "CLIP" | "DYNAMIC" (needs ``thr`` [B], from
    ``sampler_step(clip="X0_ONLY")`` + ``abs_quantile``).  -> z"""
    x_t, x_s, pred = _img(x_t), _img(x_s), _img(pred)
    B = x_t.shape[0]
    chw = x_t.numel() // B
    if chw % 4:
        raise _lib.MdmHipError("sampler_noise_map: C * H * W must be a multiple of 4 (got %s)" % (tuple(x_t.shape),))
    if x_s.shape != x_t.shape or pred.shape != x_t.shape:
        raise _lib.MdmHipError("sampler_noise_map: x_s %s and pred %s vs x_t %s"
                               % (tuple(x_s.shape), tuple(pred.shape), tuple(x_t.shape)))
    g, gl = _vec(g, B), _vec(g_last, B)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    if pu is not None and pu.shape != x_t.shape:
        raise _lib.MdmHipError("sampler_noise_map: pred_uncond %s vs x_t %s" % (tuple(pu.shape), tuple(x_t.shape)))
    th = _vec(thr, B) if thr is not None else None
    cm = {"NONE": 0, "CLIP": 1, "DYNAMIC": 2}[clip]
    mode, eta = (0, 0.0) if ddim_eta is None else (1, float(ddim_eta))
    if mode == 1 and eta <= 0:
        raise _lib.MdmHipError("sampler_noise_map: ddim_eta = %r adds no noise, there is no map to solve for" % (ddim_eta,))
    z = torch.empty_like(x_t)
    _lib.check(
        _lib.lib().mdm_sampler_noise_map(_p(x_t), _p(x_s), _p(pred), _p(pu), float(guidance_scale), _p(g), _p(gl), _p(th),
                                         _p(z), B, chw, _ptype(prediction_type), mode, eta, cm,
                                         float(image_scale) if image_scale else 1.0, _stream()),
        "mdm_sampler_noise_map",
    )
    return z


def guide_seed(v, x0, a, b, clip="CLIP", thr=None, image_scale=1.0):
    """Chain rule of loss-guided sampling through the step's x0 = a x_t + b pred, its image scale and its threshold
    (include/mdm_hip.h mdm_guide_seed) as ONE kernel: ``v`` = d loss / d x0 in image units, ``x0`` what the step kernel
    returned, ``a`` / ``b`` per-sample [B].  -> (direct, seed): the x_t term and what goes back through the denoiser.
    ``clip``: "NONE" | "CLIP" | "DYNAMIC" (needs ``thr`` [B]), the mode the step ran with."""
    v = _img(v)
    B = v.shape[0]
    chw = v.numel() // B
    if chw % 4:
        raise _lib.MdmHipError("guide_seed: C * H * W must be a multiple of 4 (got %s)" % (tuple(v.shape),))
    cm = {"NONE": 0, "CLIP": 1, "DYNAMIC": 2}[clip]
    x0 = _img(x0) if x0 is not None else None
    if cm and (x0 is None or x0.shape != v.shape):
        raise _lib.MdmHipError("guide_seed: clip=%r needs x0 shaped like v" % clip)
    th = _vec(thr, B) if thr is not None else None
    if cm == 2 and th is None:
        raise _lib.MdmHipError("guide_seed: clip='DYNAMIC' needs thr=")
    direct, seed = torch.empty_like(v), torch.empty_like(v)
    _lib.check(
        _lib.lib().mdm_guide_seed(_p(v), _p(x0), _p(_vec(a, B)), _p(_vec(b, B)), _p(th), float(image_scale) if image_scale else 1.0,
                                  cm, _p(direct), _p(seed), B, chw, _stream()),
        "mdm_guide_seed",
    )
    return direct, seed


def guide_apply(x, zeta, direct=None, jt=None):
    """x -= zeta[b] (direct + jt), IN PLACE on ``x`` as ONE kernel (mdm_guide_apply); either term may be None; a sample
    with zeta[b] == 0 keeps its bits.  -> x"""
    x = _inplace_img(x, x, "guide_apply: x")
    B = x.shape[0]
    chw = x.numel() // B
    if chw % 4:
        raise _lib.MdmHipError("guide_apply: C * H * W must be a multiple of 4 (got %s)" % (tuple(x.shape),))
    if direct is None and jt is None:
        raise _lib.MdmHipError("guide_apply: give direct= or jt=")
    d = _img(direct) if direct is not None else None
    j = _img(jt) if jt is not None else None
    for t in (d, j):
        if t is not None and t.shape != x.shape:
            raise _lib.MdmHipError("guide_apply: gradient %s vs x %s" % (tuple(t.shape), tuple(x.shape)))
    _lib.check(_lib.lib().mdm_guide_apply(_p(x), _p(d), _p(j), _p(_vec(zeta, B)), B, chw, _stream()), "mdm_guide_apply")
    return x


def pag_combine(pred, pred_uncond, pred_pert, guidance_scale=1.0, pag_scale=0.0, out=None):
    """Perturbed-attention guidance's combine (include/mdm_hip.h mdm_pag_combine) as ONE kernel:
    (pred_uncond + w (pred - pred_uncond), or pred when ``pred_uncond`` is None) + s (pred - pred_pert).  ``out`` may be
    ``pred`` itself.  -> out"""
    pred, pp = _img(pred), _img(pred_pert)
    pu = _img(pred_uncond) if pred_uncond is not None else None
    for t in (pp, pu):
        if t is not None and t.shape != pred.shape:
            raise _lib.MdmHipError("pag_combine: prediction %s vs %s" % (tuple(t.shape), tuple(pred.shape)))
    out = torch.empty_like(pred) if out is None else _inplace_img(out, pred, "pag_combine: out")
    _lib.check(_lib.lib().mdm_pag_combine(_p(pred), _p(pu), _p(pp), float(guidance_scale), float(pag_scale), _p(out),
                                          pred.numel(), _stream()), "mdm_pag_combine")
    return out


def _tile_count(H, W, window, stride):
    (h, w), (sy, sx) = window, stride
    if not (1 <= h <= H and 1 <= w <= W and 1 <= sy <= h and 1 <= sx <= w):
        raise _lib.MdmHipError("tiles: window %r, stride %r on a canvas %d x %d (wanted 1 <= stride <= window <= canvas per axis)"
                               % (tuple(window), tuple(stride), H, W))
    return _tiling.axis_count(H, h, sy) * _tiling.axis_count(W, w, sx)


def _tiles_out(out, shape, device, what):
    """the output of a tiles kernel: a new fp32 tensor of ``shape``, or the caller's, checked"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(shape):
        raise _lib.MdmHipError("%s must be a contiguous fp32 tensor of shape %s" % (what, tuple(shape)))
    _require_gpu(out)
    return out.detach()


def tiles_gather(x, window, stride, reps=1, out=None):
    """The windows of tiled sampling (include/mdm_hip_ext.h mdm_tiles_gather) as ONE kernel: x [B, C, H, W] -> the model's
    rows [reps B T, C, h, w], row (rep B + b) T + k window k of image b -- the ``reps`` blocks of the model batch are
    written by the same launch.  ``window`` = (h, w), ``stride`` = (sy, sx).  -> out"""
    x = _img(x)
    if x.dim() != 4:
        raise _lib.MdmHipError("tiles_gather: x must be [B, C, H, W] (got %s)" % (tuple(x.shape),))
    B, C, H, W = x.shape
    (h, w), (sy, sx) = window, stride
    T = _tile_count(H, W, window, stride)
    if int(reps) < 1:
        raise _lib.MdmHipError("tiles_gather: reps must be >= 1 (got %r)" % (reps,))
    out = _tiles_out(out, (int(reps) * B * T, C, h, w), x.device, "tiles_gather: out")
    n = float(B * T * C * h * w * 4)
    _prof_wrap("tiles_gather", n * (1 + int(reps)), lambda: _lib.check(
        _lib.lib().mdm_tiles_gather(_p(x), _p(out), B, C, H, W, h, w, sy, sx, int(reps), _stream()), "mdm_tiles_gather"),
        kind="hbm")
    return out


def tiles_merge(p, H, W, window, stride, blend="uniform", out=None):
    """The weighted mean of the windows' predictions over every canvas pixel (include/mdm_hip_ext.h mdm_tiles_merge) as
    ONE kernel: p [R T, C, h, w] -> [R, C, H, W], R the whole model batch.  ``blend``: "uniform" | "ramp".  -> out"""
    p = _img(p)
    (h, w), (sy, sx) = window, stride
    T = _tile_count(H, W, window, stride)
    if p.dim() != 4 or p.shape[0] % T or tuple(p.shape[2:]) != (h, w):
        raise _lib.MdmHipError("tiles_merge: predictions %s are not rows of %d windows of %d x %d" % (tuple(p.shape), T, h, w))
    R, C = p.shape[0] // T, p.shape[1]
    if blend not in _tiling.BLENDS:
        raise _lib.MdmHipError("tiles_merge: unknown blend %r (known: %s)" % (blend, ", ".join(_tiling.BLENDS)))
    bl = _tiling.BLENDS.index(blend)
    out = _tiles_out(out, (R, C, H, W), p.device, "tiles_merge: out")
    _prof_wrap("tiles_merge", float(p.numel() * 4 + out.numel() * 4), lambda: _lib.check(
        _lib.lib().mdm_tiles_merge(_p(p), _p(out), R, C, H, W, h, w, sy, sx, bl, _stream()), "mdm_tiles_merge"), kind="hbm")
    return out


_cfg_plans = {}   # (B, chw, rescale on) -> workspace bytes of mdm_cfg_plan


def _gate(gate, what):
    """a device float[1] that a kernel selects by (None = on)"""
    if gate is None:
        return None
    _require_gpu(gate)
    if gate.dtype != torch.float32 or gate.numel() != 1:
        raise _lib.MdmHipError("%s must be a device float[1] (got %s %s)" % (what, gate.dtype, tuple(gate.shape)))
    return _c(gate.detach().reshape(-1))


def cfg_combine(x_t, pred, pred_uncond, g, prediction_type, guidance_scale, eta=1.0, norm_threshold=0.0, momentum=0.0,
                rescale=0.0, image_scale=1.0, run_prev=None, run_out=None, run_gate=None, w_gate=None, out=None):
    """Projected and rescaled classifier-free guidance (mdm_hip/guidance.py; include/mdm_hip_ext.h mdm_cfg_stats +
    mdm_cfg_combine) as TWO kernels: per-sample statistics, then the combine.  -> (p_g, run)

    ``momentum != 0``: ``run`` is the update of this step, written to ``run_out`` (which may be ``run_prev`` itself; a new
    tensor if None), and ``run_prev`` the one of the step before (None = no history); ``momentum == 0``: no run buffers,
    ``run`` is None.  ``run_gate`` / ``w_gate``: device float[1] gates, None = on -- ``run_gate`` off: ``run_prev`` is not
    read (no history); ``w_gate`` off: p_g is ``pred`` and ``run`` is ``run_prev`` bit for bit (zeros where ``run_gate`` is
    off too), so that one captured graph serves every step.  ``out`` may be ``pred`` itself.  The workspace comes from the
    caching allocator: no host sync, capturable."""
    x_t, pred, pu = _img(x_t), _img(pred), _img(pred_uncond)
    B = x_t.shape[0]
    chw = x_t.numel() // B
    for t, what in ((pred, "pred"), (pu, "pred_uncond")):
        if t.shape != x_t.shape:
            raise _lib.MdmHipError("cfg_combine: %s %s vs x_t %s" % (what, tuple(t.shape), tuple(x_t.shape)))
    if chw % 4:
        raise _lib.MdmHipError("cfg_combine: C * H * W must be a multiple of 4 (got %s)" % (tuple(x_t.shape),))
    g = _vec(g, B)
    momentum, rescale = float(momentum), float(rescale)
    rp = ro = None
    if momentum != 0:
        if run_prev is not None:
            rp = _img(run_prev)
            if rp.shape != x_t.shape:
                raise _lib.MdmHipError("cfg_combine: run_prev %s vs x_t %s" % (tuple(rp.shape), tuple(x_t.shape)))
        ro = torch.empty_like(x_t) if run_out is None else _inplace_img(run_out, x_t, "cfg_combine: run_out")
    elif run_prev is not None or run_out is not None:
        raise _lib.MdmHipError("cfg_combine: run_prev= / run_out= belong to momentum != 0")
    rg, wg = _gate(run_gate, "cfg_combine: run_gate"), _gate(w_gate, "cfg_combine: w_gate")
    out = torch.empty_like(pred) if out is None else _inplace_img(out, pred, "cfg_combine: out")
    L = _lib.lib()
    key = (B, chw, rescale > 0)
    wsb = _cfg_plans.get(key)
    if wsb is None:
        v = ctypes.c_size_t(0)
        _lib.check(L.mdm_cfg_plan(B, chw, int(rescale > 0), ctypes.byref(v)), "mdm_cfg_plan")
        wsb = _cfg_plans[key] = v.value
    ws = _f32_ws(wsb, x_t.device)
    pt = _PT[prediction_type.upper()] if isinstance(prediction_type, str) else _ptype(prediction_type)   # names too, as the torch ops
    sc = float(image_scale) if image_scale else 1.0
    n = float(x_t.numel() * 4)
    _prof_wrap("cfg_stats", n * (3 + (rp is not None) + (ro is not None)), lambda: _lib.check(
        L.mdm_cfg_stats(_p(x_t), _p(pred), _p(pu), _p(g), _p(rp), _p(ro), _p(rg), _p(wg), momentum, int(rescale > 0), _p(ws),
                        wsb, B, chw, pt, _stream()), "mdm_cfg_stats"), kind="hbm")
    _prof_wrap("cfg_combine", n * 4, lambda: _lib.check(
        L.mdm_cfg_combine(_p(x_t), _p(pred), _p(pu), _p(g), _p(ro), _p(wg), _p(ws), wsb, _p(out), float(guidance_scale),
                          float(eta), float(norm_threshold), rescale, sc, B, chw, pt, _stream()), "mdm_cfg_combine"),
        kind="hbm")
    return out, ro


_aq_plans = {}   # (B, n) -> workspace bytes of mdm_abs_quantile_plan


def abs_quantile(x, q, cmin=None, cmax=None, return_stats=False):
    """thr[b] = clamp(quantile_q |x[b]|, cmin, cmax) over everything behind the first axis, by ``torch.quantile``'s rule
    (fp32 rank, linear interpolation) -- the per-sample threshold of the dynamic threshold functions as a radix select
    (include/mdm_hip_ext.h mdm_abs_quantile): FIVE launches, no sort, any row length below 2^31.  x: fp32 [B, ...] on the
    GPU; ``cmin`` / ``cmax`` None: no bound on that side.  -> thr [B], with ``return_stats`` (thr, stats [B, 2]): the two
    order statistics a[lo], a[hi] the quantile interpolates, bit for bit.  A row with a NaN gives NaN.  The workspace comes
    from the caching allocator: no host sync, capturable."""
    x = _img(x)
    if x.dim() < 2:
        raise _lib.MdmHipError("abs_quantile: x must be [B, ...] (got %s)" % (tuple(x.shape),))
    B = x.shape[0]
    n = x.numel() // B if B else 0
    L = _lib.lib()
    key = (B, n)
    wsb = _aq_plans.get(key)
    if wsb is None:
        v = ctypes.c_size_t(0)
        _lib.check(L.mdm_abs_quantile_plan(B, n, ctypes.byref(v)), "mdm_abs_quantile_plan")
        wsb = _aq_plans[key] = v.value
    ws = _f32_ws(wsb, x.device)
    thr = torch.empty(B, dtype=torch.float32, device=x.device)
    stats = torch.empty(B, 2, dtype=torch.float32, device=x.device) if return_stats else None
    lo = float("-inf") if cmin is None else float(cmin)
    hi = float("inf") if cmax is None else float(cmax)
    _prof_wrap("abs_quantile", float(x.numel() * 4 * 3), lambda: _lib.check(
        L.mdm_abs_quantile(_p(x), _p(ws), wsb, B, n, float(q), lo, hi, _p(thr), _p(stats), _stream()), "mdm_abs_quantile"),
        kind="hbm")
    return (thr, stats) if return_stats else thr


def noise_images(images, g, eps=None, rng=None, rng_stream=0, inv_scale=1.0):
    """x_t = sqrt(g) * images * inv_scale + sqrt(1 - g) * eps (reference samplers.py:244-246).  ``eps=None`` draws the
    noise inside the kernel from ``rng``.  -> (x_t, eps)"""
    images = _img(images)
    B = images.shape[0]
    chw = images.numel() // B
    g = _vec(g, B)
    x_t = torch.empty_like(images)
    if eps is None:
        if rng is None:
            raise _lib.MdmHipError("noise_images: give eps= or rng=")
        eps_out = torch.empty_like(images)
        _lib.check(_lib.lib().mdm_noise_images(_p(images), None, _p(g), float(inv_scale), _p(x_t), _p(eps_out), _p(rng.state),
                                               int(rng_stream), B, chw, _stream()), "mdm_noise_images")
        return x_t, eps_out
    eps = _img(eps)
    _lib.check(_lib.lib().mdm_noise_images(_p(images), _p(eps), _p(g), float(inv_scale), _p(x_t), None, None, 0, B, chw,
                                           _stream()), "mdm_noise_images")
    return x_t, eps


class DiffusionLossFn(torch.autograd.Function):
    """loss[b] = mean_chw (to_target_space(pred; x_t, g) - target(images, eps, g))^2 (reference diffusion.py:144-168
    with samplers.py:266-279, 347-390 folded in); differentiable w.r.t. ``pred`` only."""

    @staticmethod
    def forward(ctx, pred, x_t, images, eps, g, inv_scale, ptype, ttype):
        pred, x_t, images, eps = _img(pred), _img(x_t), _img(images), _img(eps)
        B = pred.shape[0]
        chw = pred.numel() // B
        g = _vec(g, B)
        wsb = ctypes.c_size_t(0)
        _lib.check(_lib.lib().mdm_diffusion_loss_plan(B, chw, ctypes.byref(wsb)), "mdm_diffusion_loss_plan")
        ws = _f32_ws(wsb.value, pred.device)
        loss = torch.empty(B, dtype=torch.float32, device=pred.device)
        _lib.check(_lib.lib().mdm_diffusion_loss_fwd(_p(x_t), _p(pred), _p(images), _p(eps), _p(g), float(inv_scale), _p(loss),
                                                     _p(ws), B, chw, ptype, ttype, _stream()), "mdm_diffusion_loss_fwd")
        ctx.save_for_backward(pred, x_t, images, eps, g)
        ctx.cfg = (float(inv_scale), ptype, ttype)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, x_t, images, eps, g = ctx.saved_tensors
        inv_scale, ptype, ttype = ctx.cfg
        B = pred.shape[0]
        chw = pred.numel() // B
        gl = _vec(gloss, B)
        dpred = torch.empty_like(pred)
        _lib.check(_lib.lib().mdm_diffusion_loss_bwd(_p(x_t), _p(pred), _p(images), _p(eps), _p(g), _p(gl), inv_scale, _p(dpred),
                                                     B, chw, ptype, ttype, _stream()), "mdm_diffusion_loss_bwd")
        return dpred, None, None, None, None, None, None, None


def diffusion_loss(pred, x_t, images, eps, g, prediction_type, target_type, inv_scale=1.0):
    if pred.dtype != torch.float32:
        raise _lib.MdmHipError("diffusion_loss: the model output at the boundary is fp32 (got %s)" % pred.dtype)
    return DiffusionLossFn.apply(pred, x_t, images, eps, g, float(inv_scale), _ptype(prediction_type), _ptype(target_type))


def avgpool(x, r):
    """F.avg_pool2d(x, r) on an NCHW fp32 image batch (the training pyramid, reference diffusion.py:346-348); no gradient"""
    x = _img(x)
    N, C, H, W = x.shape
    y = torch.empty((N, C, H // r, W // r), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mdm_avgpool(_p(x), _p(y), N, C, H, W, int(r), _stream()), "mdm_avgpool")
    return y


class SampleStdFn(torch.autograd.Function):
    """y = x / x.std((1, 2, 3), keepdim=True) (unbiased): the input normalisation of a nested level
    (reference models/unet.py:871-872)."""

    @staticmethod
    def forward(ctx, x):
        x = _img(x)
        N = x.shape[0]
        chw = x.numel() // N
        y = torch.empty_like(x)
        stats = torch.empty((N, 2), dtype=torch.float32, device=x.device)
        ws = torch.empty(N * 64 * 2, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().mdm_sample_std_fwd(_p(x), _p(y), _p(stats), _p(ws), N, chw, _stream()), "mdm_sample_std_fwd")
        ctx.save_for_backward(x, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats = ctx.saved_tensors
        dy = _c(dy.float())
        N = x.shape[0]
        chw = x.numel() // N
        dx = torch.empty_like(x)
        ws = torch.empty(N * 64 * 2, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().mdm_sample_std_bwd(_p(dy), _p(x), _p(stats), _p(dx), _p(ws), N, chw, _stream()), "mdm_sample_std_bwd")
        return dx


def sample_std_normalize(x):
    return SampleStdFn.apply(x)


def input_stage(u8_nhwc):
    """uint8 NHWC [B, H, W, 3] -> fp32 NCHW, (u - 127) / 128 (reference clis/train_parallel.py:194-195)"""
    _require_gpu(u8_nhwc)
    if u8_nhwc.dtype != torch.uint8 or u8_nhwc.dim() != 4 or u8_nhwc.shape[-1] != 3:
        raise _lib.MdmHipError("input_stage: expected a uint8 [B, H, W, 3] tensor")
    u = _c(u8_nhwc)
    B, H, W, _ = u.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=u.device)
    _lib.check(_lib.lib().mdm_input_stage(_p(u), _p(out), B, H, W, _stream()), "mdm_input_stage")
    return out


# --------------------------------------------------------------------------------------
# optimizer tail
# --------------------------------------------------------------------------------------
def sumsq(flat_f32, out=None, step_counter=None):
    """device scalar sum(g^2) of a flat fp32 arena (no host sync); ``step_counter`` (device int32[1]) += 1 when finite"""
    _require_gpu(flat_f32)
    out = torch.empty(1, dtype=torch.float32, device=flat_f32.device) if out is None else out
    ws = torch.empty(1024, dtype=torch.float32, device=flat_f32.device)
    _lib.check(_lib.lib().mdm_sumsq(_p(flat_f32), _p(out), _p(ws), flat_f32.numel(), _p(step_counter), _stream()), "mdm_sumsq")
    return out


def adamw_ema_step(p, g, m, v, ema, gnorm_sq, lr, beta1, beta2, eps, weight_decay, step, clip, ema_decay, zero_grad=True,
                   step_dev=None):
    """one fused clip + AdamW + EMA (+ zero-grad) pass over flat fp32 arenas; invalidates the packed-weight cache.
    ``step_dev`` (device int32[1]) overrides ``step`` for the bias correction."""
    _require_gpu(p)
    nbytes = 4.0 * p.numel() * ((4 if ema is None else 5) + (3 if ema is None else 4) + (1 if zero_grad else 0))
    _prof_wrap("adamw_ema_step", nbytes, lambda: _lib.check(
        _lib.lib().mdm_adamw_ema_step(_p(p), _p(g), _p(m), _p(v), _p(ema), _p(gnorm_sq), p.numel(), float(lr), float(beta1),
                                      float(beta2), float(eps), float(weight_decay), int(step), _p(step_dev), float(clip), float(ema_decay),
                                      1 if zero_grad else 0, _stream()),
        "mdm_adamw_ema_step",
    ), kind="hbm")
    invalidate_packed_weights()


# --------------------------------------------------------------------------------------
# dropout (nn.Dropout of a ResNet block, reference models/unet.py:208,234)
# --------------------------------------------------------------------------------------
_dropout_rng = [None, 0]   # [seed, next Philox counter block]; seeded from torch's generator on first use


def seed_dropout(seed: int, rank: int = None):
    """restart the dropout mask stream.  Default seed (first use): ``torch.initial_seed()``; the data-parallel rank is
    folded in (``rank`` default: torch.distributed's, else 0), so ranks that share a seed -- the reference seeds every
    rank alike, clis/train_parallel.py -- still draw different masks for their different samples."""
    if rank is None:
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
    _dropout_rng[0] = (int(seed) + 0x9E3779B97F4A7C15 * int(rank)) & 0xFFFFFFFFFFFFFFFF
    _dropout_rng[1] = 0


def get_dropout_rng_state():
    """(seed, offset) of the dropout mask stream -- not part of torch's RNG state: save it next to
    ``torch.cuda.get_rng_state()`` in a checkpoint if bit-reproducible resumption with dropout > 0 matters"""
    if _dropout_rng[0] is None:
        seed_dropout(torch.initial_seed())
    return (_dropout_rng[0], _dropout_rng[1])


def set_dropout_rng_state(state):
    _dropout_rng[0], _dropout_rng[1] = int(state[0]) & 0xFFFFFFFFFFFFFFFF, int(state[1])


def _dropout_forward(x, p):
    """draw the mask of a contiguous x from the dropout stream (which advances by x's counter blocks) -> (y, seed, offset)"""
    if _dropout_rng[0] is None:
        seed_dropout(torch.initial_seed())
    seed, off = _dropout_rng
    _dropout_rng[1] = off + (x.numel() + 3) // 4
    y = torch.empty_like(x)
    _lib.check(_lib.lib().mdm_dropout(_p(x), _p(y), x.numel(), float(p), seed, off, _dt(x), _stream()), "mdm_dropout")
    return y, seed, off


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _require_gpu(x)
        y, seed, off = _dropout_forward(_c(x), p)
        ctx.p, ctx.seed, ctx.off = float(p), seed, off
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        dx = torch.empty_like(dy)
        _lib.check(_lib.lib().mdm_dropout(_p(dy), _p(dx), dy.numel(), ctx.p, ctx.seed, ctx.off, _dt(dy), _stream()), "mdm_dropout")
        return dx, None


def dropout(x, p: float, training: bool = True):
    """``F.dropout(x, p, training)`` with a counter-based mask (Philox, regenerated in backward instead of stored).  The
    mask differs from torch's for the same seed -- as between any two generators -- the distribution is the same."""
    if not training or p <= 0.0:
        return x
    if p >= 1.0:
        return x * 0.0   # F.dropout(p = 1): everything dropped (the kernel's 1 / (1 - p) scale has no value there)
    if x.numel() % 8 != 0:
        raise _lib.MdmHipError("dropout: the element count must be a multiple of 8")
    return DropoutFn.apply(x, p)
