"""autograd wrappers over the C ABI (libasr_hip.so).

Each Function launches hand-written gfx950 kernels on torch's current stream
through ctypes; torch supplies only device memory, the stream and the autograd
tape.  No op here has a CPU path: CPU tensors raise NativeError.

Weight gradients are accumulated by the kernels directly into ``param.grad``
(views into the model's flat gradient buffer, see models/pytorch_v3/base.py);
the Functions therefore return ``None`` for weights.
"""
import collections
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _native as N

F32 = N.ASR_DT_F32
BF16 = N.ASR_DT_BF16

_compute = {'dtype': F32}


def set_compute_dtype(name):
    """'fp32' (exact-f32 MFMA, parity mode) or 'bf16' (bf16 MFMA, f32 accumulate)."""
    if name not in ('fp32', 'bf16'):
        raise ValueError('compute dtype must be fp32 or bf16')
    _compute['dtype'] = BF16 if name == 'bf16' else F32


def compute_dtype():
    return _compute['dtype']


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _grown_ws(cache, nbytes, device):
    """cache's (device -> tensor) workspace of at least nbytes: kept from the
    largest call so far, replaced only by a larger one."""
    ws = cache.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = cache[device] = _ws(nbytes, device)
    return ws


def h2d(a, device):
    """Host array -> device tensor without blocking the host: staged through
    pinned memory (torch's caching host allocator keeps the block until the
    copy has run).  A copy from pageable memory waits for the stream to reach
    it, i.e. for the work already queued -- the host then falls behind the
    GPU and the next kernels launch into an idle queue."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if _H2D_PINNED:
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


_H2D_PINNED = os.environ.get('ASR_H2D_PINNED', '1') != '0'   # (A/B: 0 = pageable copies)


# ---------------------------------------------------------------------------
# Per-step recurrence workspace arena.  Every tagged-granule launch needs its
# granule workspace zero (lstm_xg.hip); instead of one memset launch before
# each of the 2 x L layer passes of a step, the encoder forward clears one
# arena with a slot per pass (rec_arena_begin), each BLSTM forward takes a
# slot for itself and reserves one for its backward, and those launches are
# told so with the call (asr_lstm_opts_t.ws_prezeroed, like every recurrence
# launch setting: nothing is set in the library between calls) and skip their
# memset.  A slot is handed out once per
# generation; a backward whose reservation is from an older generation (the
# arena was cleared again by another forward since) takes a private workspace
# and the launch's own memset.  Only each slot's leading bytes are cleared --
# what a tagged-granule launch of the arena's own shape zeroes -- so a launch
# of another shape or compute dtype (a layer op called outside the model) gets
# a slot only when that prefix covers what it would clear itself.
# ---------------------------------------------------------------------------
_arena = {'buf': None, 'gen': 0, 'off': 0, 'slot': 0, 'end': 0, 'zero': 0, 'cd': None}
# recurrence launches whose workspace came from the arena / was their own
ARENA_STATS = {'granted': 0, 'private': 0}


def rec_arena_begin(dev, B, H, passes):
    """Clear the arena for `passes` recurrence launches of [B, *, H] (one fill
    on the current stream); ASR_REC_ARENA=0: off."""
    if os.environ.get('ASR_REC_ARENA', '1') == '0':
        _arena['slot'] = 0
        return
    cd = compute_dtype()
    nb = max(N.query('asr_lstm_workspace_bytes', B, H, cd, k) for k in (0, 1, 2))
    slot = (int(nb) + 255) // 256 * 256
    need = slot * int(passes)
    buf = _arena['buf']
    if buf is None or buf.device != dev or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
    # only each slot's leading bytes must be zero (one strided fill)
    zero = int(N.query('asr_lstm_ws_zero_bytes', B, H))
    zb = min(zero, slot)
    buf[:need].view(int(passes), slot)[:, :zb].zero_()
    # end: a reused buffer may be longer than this generation's cleared slots
    _arena.update(buf=buf, gen=_arena['gen'] + 1, off=0, slot=slot, end=need, zero=zero, cd=cd)


def _arena_take(nbytes, dev, zero_bytes):
    """(zeroed slot tensor, generation) from the current arena, or None.
    zero_bytes: asr_lstm_ws_zero_bytes of the launch's own shape, the leading
    bytes it would clear itself.  A slot's first min(zero, slot) bytes are
    zero, so a launch with nbytes <= slot and zero_bytes <= zero finds every
    byte it needs zero (it needs none past its nbytes); any other launch, or
    one in another compute dtype than the arena was sized for, is refused."""
    a = _arena
    if not a['slot'] or a['buf'] is None or a['buf'].device != dev or nbytes > a['slot']:
        return None
    if zero_bytes > a['zero'] or a['cd'] != compute_dtype():
        return None
    if a['off'] + a['slot'] > a['end']:
        return None
    t = a['buf'][a['off']:a['off'] + a['slot']]
    a['off'] += a['slot']
    return t, a['gen']


def _arena_valid(res):
    return res is not None and res[1] == _arena['gen']


def _rec_workspace(nbytes, dev, res):
    """(workspace, prezeroed) of one recurrence launch: the arena slot `res`
    (_arena_take's, now or reserved by the forward) if it is of the current
    generation and long enough, else a private buffer the launch clears."""
    pz = _arena_valid(res) and nbytes <= res[0].numel()
    ARENA_STATS['granted' if pz else 'private'] += 1
    return (res[0] if pz else _ws(nbytes, dev)), pz


def _lstm_opts(pz, **settings):
    """asr_lstm_opts_t* of one recurrence call: pz, _rec_workspace's prezeroed."""
    return ctypes.byref(N.LstmOpts(ws_prezeroed=int(pz), **settings))


# Gradient-ready notifications for the data-parallel bucketed all-reduce
# (utils/training/grad_buckets.py): 'recurrence' after a BLSTM layer's backward
# recurrence is enqueued, ('grads', gbufs) once its weight gradients are.
_grad_hook = [None]


def set_grad_ready_hook(fn):
    _grad_hook[0] = fn


def notify_grad_event(event, arg=None):
    fn = _grad_hook[0]
    if fn is not None:
        fn(event, arg)


def recurrence_status(device):
    """Device int32[2]: the persistent recurrences' give-up words since the
    last call (cleared), stream-ordered, no host sync."""
    st = torch.empty(2, dtype=torch.int32, device=device)
    N.call('asr_lstm_status_gather', N.ptr(st), 1, N.stream_handle(device))
    return st


class RecurrenceGaveUp(N.NativeError):
    """A persistent recurrence gave up a bounded wait: that pass's outputs are
    invalid (the pass itself can be run again)."""


def raise_if_recurrence_failed(device=None):
    """Host check (synchronises): RecurrenceGaveUp when a persistent recurrence
    gave up since the last gather (its outputs are invalid)."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    st = recurrence_status(device)
    if int(st.max().item()):
        raise RecurrenceGaveUp('persistent LSTM recurrence gave up a bounded wait (status %s): '
                               'outputs of this pass are invalid' % st.tolist())


def grad_buffer(p):
    """The gradient view a kernel accumulates into (allocated on first use)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


# ---------------------------------------------------------------------------
# GEMM plumbing
# ---------------------------------------------------------------------------
def rowmap(stride_t, stride_b=0, rows_per_b=0, t_mul=1, t_add=0, t_limit=0, perm=None):
    return N.RowMap(int(stride_b), int(stride_t), int(rows_per_b), int(t_mul), int(t_add),
                    int(t_limit), perm.data_ptr() if perm is not None else None)


def operand(t, trans, rmap, offset=0):
    dt = BF16 if t.dtype == torch.bfloat16 else F32
    es = t.element_size()
    nbytes = t.untyped_storage().nbytes() - (t.storage_offset() + offset) * es
    return N.Operand(t.data_ptr() + offset * es, dt, int(trans), rmap, int(nbytes))


def gemm_problem(a, b, c, c_map, M, N_, K, alpha=1.0, beta=0.0, bias=None, bias2=None, c_offset=0,
                 batch=1, batch_strides=(0, 0, 0), drop=None):
    """drop=(p, seed): the written values get asr_dropout's mask for their
    element offsets from c (dropout's backward fused into the product)."""
    c_bf16 = c.dtype == torch.bfloat16     # bf16 C: written as bf16 (beta 0, no split-K)
    return N.Gemm(a, b, c.data_ptr() + c.element_size() * c_offset, c_map,
                  bias.data_ptr() if bias is not None else None,
                  bias2.data_ptr() if bias2 is not None else None, int(M), int(N_), int(K),
                  float(alpha), float(beta), int(batch), int(batch_strides[0]),
                  int(batch_strides[1]), int(batch_strides[2]),
                  float(drop[0]) if drop else 0.0, int(drop[1]) if drop else 0,
                  BF16 if c_bf16 else F32)


# run_gemm's opts (asr_gemm_opts_t; None: the defaults)
SMALL_TILES = N.GemmOpts(small_tiles=1)
NOSPLIT = N.GemmOpts(nosplit=1)
N64_KMODE = N.GemmOpts(n64_kmode=1)


def run_gemm(problems, device, lse=None, cd=None, opts=None):
    """One launch of up to two products; long-K / few-tile products (weight
    gradients) get a split-K workspace from torch's caching allocator.
    lse (one product): f32 [ceil(N / 64), M, 2] tensor receiving the row
    log-sum-exp partials of the written C (asr_gemm_lse_ws).  cd: the
    products' compute dtype when it is not the session's (an op that is f32
    in both modes).  opts: the GemmOpts of the workspace query and the launch."""
    arr = (N.Gemm * len(problems))(*problems)
    parr = ctypes.cast(arr, ctypes.c_void_p)
    po = N.ptr_struct(opts)
    nb = N.query('asr_gemm_workspace_bytes', parr, len(problems), po)
    ws = _ws(nb, device) if nb else None
    if lse is not None:
        assert len(problems) == 1
        N.call('asr_gemm_lse_ws', parr, compute_dtype(), N.ptr(lse), N.ptr(ws), nb,
               N.stream_handle(device), po)
        return
    N.call('asr_gemm_ws', parr, len(problems), compute_dtype() if cd is None else cd, N.ptr(ws),
           nb, N.stream_handle(device), po)


def _ctc_lse_epilogue(V):
    """The CTC normaliser of a wide output layer (V > 1024) is formed in the
    head GEMM's epilogue (ASR_CTC_LSE_EPI=0: by the CTC forward's own pass
    over the logits)."""
    return V > 1024 and os.environ.get('ASR_CTC_LSE_EPI', '1') != '0'


def colsum_accumulate(g2d, out0, out1=None, alpha=1.0):
    M, Nn = g2d.shape
    nb = N.query('asr_colsum_workspace_bytes', M, Nn)
    ws = _ws(nb, g2d.device)
    N.call('asr_colsum_accumulate', N.ptr(g2d), g2d.stride(0), M, Nn, float(alpha), N.ptr(out0),
           N.ptr(out1), N.ptr(ws), nb, N.stream_handle(g2d.device))


# ---------------------------------------------------------------------------
# Linear (LinearND, linear.py:15-47): y = x W^T + b on the last dim
# ---------------------------------------------------------------------------
# bf16 mode stages f32 GEMM operands in bf16 (one conversion pass) when a
# product is at least this large, so it takes the bf16 fast / 8-wave kernels
# instead of the generic kernel converting inside its loads (the word-level CTC
# head, 8000 x 640 x 10001, ran at ~140 TF/s that way).  The padded pitches
# also put backward products whose K is the output width (the 29-class CTC
# head's dX, K = 29) on the fast kernels, so such layers are staged from
# 32 MFLOP (round 4: 250 MFLOP, the 5x512 CTC head, 32000 x 1024 x 29: -0.1
# ms/step; round 5 also the attention decoder's 29-class output layer, 4032 x
# 320 x 29, whose dX had stayed on the generic kernel); staging a layer whose
# width is already a multiple of 8 below 2 GFLOP measured slower.
_STAGE_FLOPS = 2e9
_STAGE_FLOPS_RAGGED = float(os.environ.get("ASR_LINEAR_STAGE_FLOPS", "3.2e7"))


def _staged(t, rows, cols, ld=None):
    """bf16 [rows, ld] copy of a dense f32 tensor viewed as rows x cols, the
    columns [cols, ld) zero (ld: cols rounded up to a multiple of 8 by default,
    so the copy is a legal 16-B-aligned GEMM operand)."""
    ld = (cols + 7) // 8 * 8 if ld is None else ld
    out = torch.empty(rows, ld, dtype=torch.bfloat16, device=t.device)
    N.call('asr_convert_rows_bf16_ld', N.ptr(t), rowmap(cols), int(rows), int(cols), int(ld),
           N.ptr(out), N.stream_handle(t.device))
    return out


# ---------------------------------------------------------------------------
# bf16 parameter shadow.  The fused optimizer step (optim.hip) rounds every
# updated parameter to bf16 beside its f32 write, into one shadow of the flat
# parameter buffer, so the next forward's BLSTM layers read their staged W_ih
# from it instead of converting it again (one pass over 8H x Din f32 per
# layer).  The shadow is trusted only while nothing else wrote the parameters
# since: the flat buffer's version (writes through flat views) and every
# parameter's own version (torch.optim, load_state_dict, in-place init) must be
# the ones recorded at the optimizer step.  ASR_PARAM_SHADOW=0 turns it off.
# ---------------------------------------------------------------------------
_shadows = {}   # id(flat param tensor) -> _ParamShadow (tensors compare elementwise)
SHADOW_STATS = {'hits': 0, 'linear_hits': 0}   # BLSTM / linear forwards that read the shadow


class _ParamShadow:
    __slots__ = ('flat', 'buf', 'flat_version', 'param_versions')

    def __init__(self, flat, buf):
        self.flat = weakref.ref(flat)
        self.buf = buf
        self.flat_version = None
        self.param_versions = None


def param_shadow(flat):
    """The bf16 shadow the optimizer step over `flat` should write, or None
    (fp32 mode, or switched off)."""
    if compute_dtype() != BF16 or os.environ.get('ASR_PARAM_SHADOW', '1') == '0':
        return None
    sh = _shadows.get(id(flat))
    if sh is None or sh.flat() is not flat or sh.buf.device != flat.device:
        for k in [k for k, v in _shadows.items() if v.flat() is None]:
            del _shadows[k]
        sh = _ParamShadow(flat, torch.empty(flat.numel(), dtype=torch.bfloat16,
                                            device=flat.device))
        _shadows[id(flat)] = sh
    return sh


def param_shadow_written(sh, flat, params):
    """Record the versions the shadow matches (call right after enqueueing the
    optimizer step that writes it; later writes are ordered after it and bump
    a version)."""
    sh.flat_version = flat._version
    sh.param_versions = {id(p): p._version for p in params}


def param_shadow_skipped(flat):
    """An optimizer step over `flat` ran without a shadow to write (fp32 mode,
    ASR_PARAM_SHADOW=0): the kernel changed the parameters without bumping a
    version, so a shadow written by an earlier step is void until a later
    step writes it again."""
    for sh in _shadows.values():
        if sh.flat() is flat:
            sh.param_versions = None


def _shadow_rows(w, params):
    """bf16 view of the shadow's copy of `w` (a dense view of a flat parameter
    buffer, spanning `params`), or None when there is no current shadow."""
    if w.dtype != torch.float32 or not w.is_contiguous():
        return None
    flat = w._base
    if flat is None:
        # a module's nn.Parameter (its .data a slice of the flat buffer): the
        # flat buffer by storage
        sp = w.untyped_storage().data_ptr()
        flat = next((sh.flat() for sh in _shadows.values()
                     if sh.flat() is not None and sh.flat().untyped_storage().data_ptr() == sp),
                    None)
        if flat is None:
            return None
    sh = _shadows.get(id(flat))
    if (sh is None or sh.flat() is not flat or sh.param_versions is None or
            flat._version != sh.flat_version):
        return None
    pv = sh.param_versions
    if not params or any(pv.get(id(p)) != p._version for p in params):
        return None
    off = w.storage_offset() - flat.storage_offset()
    if off < 0 or off + w.numel() > flat.numel():
        return None
    return sh.buf[off:off + w.numel()].view(w.shape)


def _wih_bf16(w_ih, params, H, Din):
    """Staged bf16 W_ih [8H, Din] of a BLSTM layer: the optimizer's shadow
    when current, else one conversion pass."""
    w = _shadow_rows(w_ih, params)
    if w is None:
        return convert_rows_bf16(w_ih, rowmap(Din), 8 * H, Din)
    SHADOW_STATS['hits'] += 1
    return w


def _linear_stages(M, K, Nout):
    """Whether LinearND's product is staged as bf16 operands (see _STAGE_FLOPS)."""
    flops = 2.0 * M * Nout * K
    return compute_dtype() == BF16 and (
        flops >= _STAGE_FLOPS or (Nout % 8 != 0 and flops >= _STAGE_FLOPS_RAGGED))


def _linear_forward(x, weight, bias, drop, lse=None, ld=None):
    """y = dropout(x) W^T + b (f32 [..., Nout]); returns (y, xo, wo, stage):
    the GEMM operands the backward reuses (bf16 staged copies when stage).
    lse: row log-sum-exp partials of y (run_gemm).  ld: y's row pitch (>=
    Nout; y is then a strided view of [M, ld] storage)."""
    N.require_device(x, weight)
    x = x.contiguous()
    K = x.shape[-1]
    Nout = weight.shape[0]
    M = x.numel() // K
    ld = Nout if ld is None else int(ld)
    if ld == Nout:
        y = torch.empty(*x.shape[:-1], Nout, dtype=torch.float32, device=x.device)
    else:
        ybuf = torch.empty(M * ld, dtype=torch.float32, device=x.device)
        lead = tuple(x.shape[:-1])
        strides = tuple(int(np.prod(lead[i + 1:])) * ld for i in range(len(lead))) + (1,)
        y = torch.as_strided(ybuf, lead + (Nout,), strides)
    stage = _linear_stages(M, K, Nout)
    fused_drop = drop is not None and stage and K % 8 == 0
    if drop is not None and not fused_drop:        # materialise dropout(x) first
        xd = torch.empty_like(x)
        N.call('asr_dropout', N.ptr(x), N.ptr(xd), x.numel(), float(drop[0]), int(drop[1]),
               N.stream_handle(x.device))
        x = xd
    # staged copies: x [M][Kp], weight [Np][Kp] (rows Nout.. and columns K.. zero)
    Kp, Np = ((K + 7) // 8 * 8, (Nout + 7) // 8 * 8) if stage else (K, Nout)
    if stage:
        # a dense weight (no padding) from the optimizer's bf16 shadow when current
        wo = _shadow_rows(weight, (weight,)) if (Np == Nout and Kp == K) else None
        if wo is not None:
            SHADOW_STATS['linear_hits'] += 1
        elif not fused_drop and K % 8 == 0 and os.environ.get('ASR_LINEAR_MULTI', '1') != '0':
            # input, weight and zero pad rows staged in one launch (the same bits)
            # (a declined launch -- an operand that is not 16-B aligned -- wrote
            # nothing: xm / wm are dropped and both are converted one by one below)
            xm = torch.empty(M, Kp, dtype=torch.bfloat16, device=x.device)
            wm = torch.empty(Np, Kp, dtype=torch.bfloat16, device=x.device)
            jobs = [(x, rowmap(K), M, K, xm.data_ptr()), (weight, rowmap(K), Nout, K, wm.data_ptr())]
            if Np > Nout:
                jobs.append((weight, rowmap(0, t_limit=1, rows_per_b=Np - Nout, t_add=1),
                             Np - Nout, Kp, wm.data_ptr() + Nout * Kp * 2))
            if M > 0 and _convert_multi(jobs, x.device):
                return _linear_gemm(xm, wm, y, ld, M, Nout, Kp, bias, lse, x.device) + (stage,)
        # fused_drop: K % 8 == 0, so Kp == K and the dropped copy is the operand
        xo = (convert_rows_bf16(x, rowmap(K), M, K, drop=drop) if fused_drop else
              _staged(x, M, K, Kp))
        if wo is None:
            wo = torch.empty(Np, Kp, dtype=torch.bfloat16, device=x.device)
            N.call('asr_convert_rows_bf16_ld', N.ptr(weight), rowmap(K), Nout, K, Kp, N.ptr(wo),
                   N.stream_handle(x.device))
            if Np > Nout:
                N.call('asr_convert_rows_bf16_ld', N.ptr(weight), rowmap(0, t_limit=1,
                       rows_per_b=Np - Nout, t_add=1), Np - Nout, Kp, Kp,
                       ctypes.c_void_p(wo.data_ptr() + Nout * Kp * 2), N.stream_handle(x.device))
    else:
        xo, wo = x, weight
    return _linear_gemm(xo, wo, y, ld, M, Nout, Kp, bias, lse, x.device) + (stage,)


def _linear_gemm(xo, wo, y, ld, M, Nout, Kp, bias, lse, dev):
    if M > 0:
        p = gemm_problem(operand(xo, 0, rowmap(Kp)), operand(wo, 0, rowmap(Kp)), y,
                         rowmap(ld), M, Nout, Kp, bias=bias)
        run_gemm([p], dev, lse=lse)
    return y, xo, wo


def _convert_multi(jobs, dev):
    """jobs: (src tensor, RowMap, rows, cols, dst address) -- asr_convert_rows_bf16
    of each in one launch; False when a job does not qualify (nothing launched)."""
    n = len(jobs)
    src = (ctypes.c_void_p * n)(*[j[0].data_ptr() for j in jobs])
    maps = (N.RowMap * n)(*[j[1] for j in jobs])
    rows = (ctypes.c_int * n)(*[int(j[2]) for j in jobs])
    cols = (ctypes.c_int * n)(*[int(j[3]) for j in jobs])
    dst = (ctypes.c_void_p * n)(*[j[4] for j in jobs])
    rc = N.lib().asr_convert_rows_bf16_multi(n, src, maps, rows, cols, dst,
                                              N.stream_handle(dev))
    if rc < 0:
        raise N.NativeError('asr_convert_rows_bf16_multi: launch failed')
    return rc == 1


def _linear_backward(xo, wo, bias, stage, xshape, weight, drop, dyo, need_dx, dy_bias=None,
                     wgrad=True):
    """dX and dW (+ db) of _linear_forward from dyo: the f32 dY, or with stage
    its bf16 copy [M][Np] whose columns Nout.. are zero (they meet W's zero
    rows).  dy_bias: the tensor the bias gradient is summed from (f32 [M,
    Nout] or the bf16 dyo).  wgrad=False: dX only (_linear_wgrad elsewhere)."""
    K = xshape[-1]
    Nout = weight.shape[0]
    M = int(np.prod(xshape[:-1]))
    dev = dyo.device
    Kp, Np = (xo.shape[-1], wo.shape[0]) if stage else (K, Nout)
    dx = None
    probs = []
    if need_dx:
        dx = torch.empty(xshape, dtype=torch.float32, device=dev)
        probs.append(gemm_problem(operand(dyo, 0, rowmap(Np)), operand(wo, 1, rowmap(Kp)),
                                  dx, rowmap(K), M, K, Np, drop=drop))
    if not wgrad:
        if probs:
            run_gemm(probs, dev)
        return dx
    gw = grad_buffer(weight)
    probs.append(gemm_problem(operand(dyo, 1, rowmap(Np)), operand(xo, 1, rowmap(Kp)), gw,
                              rowmap(K), Nout, K, M, beta=1.0))
    run_gemm(probs, dev)
    _linear_bias_grad(bias, dy_bias, M, Nout, dev)
    return dx


def _linear_wgrad(xo, wo, bias, stage, xshape, weight, dyo, dy_bias=None, gemm_opts=None):
    """dW (+ db) of _linear_backward alone."""
    K = xshape[-1]
    Nout = weight.shape[0]
    M = int(np.prod(xshape[:-1]))
    dev = dyo.device
    Kp, Np = (xo.shape[-1], wo.shape[0]) if stage else (K, Nout)
    run_gemm([gemm_problem(operand(dyo, 1, rowmap(Np)), operand(xo, 1, rowmap(Kp)),
                           grad_buffer(weight), rowmap(K), Nout, K, M, beta=1.0)], dev,
             opts=gemm_opts)
    _linear_bias_grad(bias, dy_bias, M, Nout, dev)


def _linear_bias_grad(bias, dy_bias, M, Nout, dev):
    if bias is not None:
        if dy_bias.dtype == torch.bfloat16:
            nb = N.query('asr_colsum_workspace_bytes', M, Nout)
            ws = _ws(nb, dev)
            N.call('asr_colsum_accumulate_bf16', N.ptr(dy_bias), dy_bias.shape[-1], M, Nout, 1.0,
                   N.ptr(grad_buffer(bias)), None, N.ptr(ws), nb, N.stream_handle(dev))
        else:
            colsum_accumulate(dy_bias.view(M, Nout), grad_buffer(bias))


def _wgrad_beside(dev, plan, fn, keep, gbufs):
    """Enqueue the weight-gradient work fn(gemm_opts) on the weight-gradient
    side stream of the recurrence shape plan = (B, H), gated on the next
    backward recurrence (as a BLSTM layer's own weight gradients); fn gives
    gemm_opts to each run_gemm; keep: tensors the side stream reads.  False
    when that shape runs weight gradients on the compute stream (the caller
    then runs fn(None) itself)."""
    side_ent = _wgrad_side_stream(dev, *plan)
    if side_ent is None:
        return False
    side, small, gated = side_ent
    main = torch.cuda.current_stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        if gated:
            N.call('asr_lstm_wgrad_gate', N.stream_handle(dev))
        fn(SMALL_TILES if small else None)
    _defer_side_join(dev, side, main, keep, gbufs)
    return True


# (B, H) of the encoder recurrence whose backward follows, while the decoder-side
# linear layers of an attention model are built (wgrad_beside_encoder): their
# weight gradients then run beside that recurrence instead of before it
_beside_plan = [None]


class wgrad_beside_encoder(object):
    def __init__(self, B, H):
        self.plan = (int(B), int(H))

    def __enter__(self):
        self.prev = _beside_plan[0]
        if os.environ.get('ASR_DEC_WGRAD_SIDE', '1') != '0':
            _beside_plan[0] = self.plan
        return self

    def __exit__(self, *a):
        _beside_plan[0] = self.prev
        return False


class LinearFn(torch.autograd.Function):
    """y = dropout(x) W^T + b.  drop=(p, seed): dropout of the INPUT with
    asr_dropout's mask, folded into the bf16 staging of x (forward) and the dX
    GEMM's epilogue (backward) when the product is staged; otherwise applied
    as a separate pass first."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop=None):
        y, xo, wo, stage = _linear_forward(x, weight, bias, drop)
        ctx.save_for_backward(xo, wo)
        ctx.meta = (bias, stage, tuple(x.shape), weight)
        ctx.drop = drop
        ctx.beside = _beside_plan[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        xo, wo = ctx.saved_tensors
        bias, stage, xshape, weight = ctx.meta
        dy = dy.contiguous()
        Nout = weight.shape[0]
        M = dy.numel() // Nout
        if M == 0:
            return torch.zeros(xshape, dtype=torch.float32, device=dy.device), None, None, None
        Np = wo.shape[0] if stage else Nout
        dyo = _staged(dy, M, Nout, Np) if stage else dy   # zero columns meet zero W rows
        # dropout's backward = its mask, applied by the dX epilogue
        if ctx.beside is not None:
            dx = _linear_backward(xo, wo, bias, stage, xshape, weight, ctx.drop, dyo,
                                  ctx.needs_input_grad[0], dy_bias=dy, wgrad=False)
            gb = (grad_buffer(weight),) + ((grad_buffer(bias),) if bias is not None else ())
            wgrad = lambda go: _linear_wgrad(xo, wo, bias, stage, xshape, weight, dyo,  # noqa: E731
                                             dy_bias=dy, gemm_opts=go)
            if not _wgrad_beside(dy.device, ctx.beside, wgrad, (xo, wo, dyo, dy), gb):
                wgrad(None)
            return dx, None, None, None
        dx = _linear_backward(xo, wo, bias, stage, xshape, weight, ctx.drop, dyo,
                              ctx.needs_input_grad[0], dy_bias=dy)
        return dx, None, None, None


def _ctc_forward(logits, st, sb, T, B, V, lse, labels_flat, label_lens, act_lens, max_label_len,
                 blank, zero_infinity, loss_scale):
    """asr_ctc_forward, or asr_ctc_forward_lse from the head GEMM's partials;
    returns (costs [B], loss [1], ws, nbytes), ws the state the backward reads."""
    dev = logits.device
    nbytes = N.query('asr_ctc_workspace_bytes', T, B, V, max_label_len)
    ws = _ws(nbytes, dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    common = (N.ptr(labels_flat), N.ptr(label_lens), N.ptr(act_lens), int(max_label_len),
              int(blank), int(bool(zero_infinity)), N.ptr(costs), N.ptr(loss), float(loss_scale),
              N.ptr(ws), nbytes, N.stream_handle(dev))
    if lse is not None:
        N.call('asr_ctc_forward_lse', N.ptr(logits), st, sb, T, B, V, N.ptr(lse), lse.shape[0],
               *common)
    else:
        N.call('asr_ctc_forward', N.ptr(logits), st, sb, T, B, V, *common)
    return costs, loss, ws, nbytes


class LinearCTCFn(torch.autograd.Function):
    """The CTC output layer and its loss as ONE op (LinearND + CTC: ctc.py:30-52
    with linear.py:32-47), for heads whose product is staged in bf16.
    Forward: the staged GEMM writes the f32 logits [B, T, V] (bias fused),
    then the CTC forward (emissions + lattices) reads them.  Backward: the CTC
    gradient is written straight into the bf16 dY operand of the two GEMMs --
    rows of Np = V rounded up to 8 columns, the padding zero
    (asr_ctc_backward_bf16) -- so the f32 d logits is never written and never
    restaged (at the 10001-word head of configs[4]: 320 MB written + 480 MB
    staging traffic per call saved).  The bias gradient is summed in f32 by
    the same pass before the rounding (asr_ctc_backward_bf16_db: per-block
    column partials, then a fixed-order sum).  dX and dW equal
    ctc_loss(linear(...))'s up to the bf16 rounding of dY the staged product
    applies anyway; the bias gradient equals the f32 column sum up to
    summation order."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop, labels_flat, label_lens, act_lens, max_label_len,
                loss_scale, blank, zero_infinity):
        N.require_device(labels_flat, label_lens, act_lens)
        V = weight.shape[0]
        M = x.numel() // x.shape[-1]
        lse = (torch.empty((V + 63) // 64, M, 2, dtype=torch.float32, device=x.device)
               if _ctc_lse_epilogue(V) and M > 0 else None)
        # wide heads: logits pitch V rounded up to 4 columns, so the gradient
        # pass reads 16-B aligned rows (ctc_grad_bf16's aligned form; a narrow
        # head keeps the dense layout, whose values the unfused ops reproduce
        # bit for bit)
        logits, xo, wo, stage = _linear_forward(x, weight, bias, drop, lse=lse,
                                                ld=(V + 3) // 4 * 4 if V > 1024 else V)
        assert stage, 'LinearCTCFn needs a staged (bf16) output layer'
        B, T, V = logits.shape
        costs, loss, ws, nbytes = _ctc_forward(
            logits, logits.stride(1), logits.stride(0), T, B, V, lse, labels_flat, label_lens,
            act_lens, max_label_len, blank, zero_infinity, loss_scale)
        ctx.save_for_backward(xo, wo, logits, labels_flat, label_lens, act_lens, ws)
        ctx.meta = (bias, tuple(x.shape), weight, int(max_label_len), int(blank),
                    float(loss_scale), nbytes)
        # produced by a BLSTM layer (through at most a few views / permutes):
        # its backward recurrence is the next one the gate can wait for
        ctx.from_blstm = _produced_by_blstm(x)
        ctx.drop = drop
        ctx.mark_non_differentiable(costs)
        return loss, costs

    @staticmethod
    def backward(ctx, g_loss, g_costs):
        xo, wo, logits, labels_flat, label_lens, act_lens, ws = ctx.saved_tensors
        bias, xshape, weight, max_label_len, blank, loss_scale, nbytes = ctx.meta
        B, T, V = logits.shape
        Np = wo.shape[0]
        dev = logits.device
        dyo = torch.empty(B * T, Np, dtype=torch.bfloat16, device=dev)
        g = g_loss.contiguous() if g_loss is not None else None
        args = (N.ptr(logits), logits.stride(1), logits.stride(0), T, B, V, N.ptr(labels_flat),
                N.ptr(label_lens),
                N.ptr(act_lens), max_label_len, blank, N.ptr(g),
                loss_scale if g is not None else 0.0, N.ptr(dyo), Np, T * Np, Np, N.ptr(ws), nbytes)
        # the bias gradient: f32 column sums formed inside the gradient pass before
        # the bf16 rounding (ASR_CTC_HEAD_DB=0, or a head too wide for that pass's
        # class table by the library's own condition: column sums of the rounded dY)
        bws = None
        if (bias is not None and os.environ.get('ASR_CTC_HEAD_DB', '1') != '0'
                and N.query('asr_ctc_bias_supported', V, Np, max_label_len)):
            bnb = N.query('asr_ctc_bias_workspace_bytes', T, B, V, Np)
            bws = _ws(bnb, dev)
            N.call('asr_ctc_backward_bf16_db', *args, N.ptr(grad_buffer(bias)), N.ptr(bws), bnb,
                   N.stream_handle(dev))
        else:
            N.call('asr_ctc_backward_bf16', *args, N.stream_handle(dev))
        bias_w = None if bws is not None else bias   # bias gradient still to be summed from dY
        if ctx.from_blstm is not None and os.environ.get('ASR_HEAD_WGRAD_SIDE', '1') != '0':
            # the head's weight gradient (only the optimizer needs it) beside the
            # top BLSTM layer's backward recurrence, as that layer's own weight
            # gradients run beside the next one: dX alone on the compute stream
            dx = _linear_backward(xo, wo, bias_w, True, xshape, weight, ctx.drop, dyo,
                                  ctx.needs_input_grad[0], dy_bias=dyo, wgrad=False)
            gb = (grad_buffer(weight),) + ((grad_buffer(bias),) if bias is not None else ())
            wgrad = lambda go: _linear_wgrad(xo, wo, bias_w, True, xshape, weight, dyo,  # noqa: E731
                                             dy_bias=dyo, gemm_opts=go)
            if not _wgrad_beside(dev, ctx.from_blstm, wgrad, (xo, wo, dyo), gb):
                wgrad(None)
            return (dx,) + (None,) * 10
        dx = _linear_backward(xo, wo, bias_w, True, xshape, weight, ctx.drop, dyo,
                              ctx.needs_input_grad[0], dy_bias=dyo)
        return (dx,) + (None,) * 10


class LinearCTC32Fn(torch.autograd.Function):
    """The CTC output layer and its loss as one op at reference precision (fp32
    mode; LinearND + CTC, ctc.py:30-52 with linear.py:32-47): the logits are
    written with a row pitch of V rounded up to 4 columns, and the CTC
    gradient with the same pitch, so the three products (logits, dX, dW) get
    16-B aligned rows and run on the f32 fast kernel (gemm_f32_fast) instead of
    the generic one (an unpadded 10001-column row is not 16-B aligned; the
    fast kernel zero-fills the k tail of the dX product in LDS).  Values equal
    ctc_loss(linear(...))'s up to the summation order of the products."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop, labels_flat, label_lens, act_lens, max_label_len,
                loss_scale, blank, zero_infinity):
        N.require_device(x, weight, labels_flat, label_lens, act_lens)
        # the producing BLSTM layer is found from the ORIGINAL input: the
        # contiguous copy and the materialised dropout below carry no grad_fn
        ctx.from_blstm = _produced_by_blstm(x)
        x = x.contiguous()
        B, T, K = x.shape
        V = weight.shape[0]
        Vp = (V + 3) // 4 * 4
        dev = x.device
        if drop is not None:   # materialise dropout(x); the dX epilogue applies the mask
            xd = torch.empty_like(x)
            N.call('asr_dropout', N.ptr(x), N.ptr(xd), x.numel(), float(drop[0]), int(drop[1]),
                   N.stream_handle(dev))
            x = xd
        logits = torch.empty(B * T, Vp, dtype=torch.float32, device=dev)
        lse = (torch.empty((V + 63) // 64, B * T, 2, dtype=torch.float32, device=dev)
               if _ctc_lse_epilogue(V) and B * T > 0 else None)
        if B * T > 0:
            run_gemm([gemm_problem(operand(x, 0, rowmap(K)), operand(weight, 0, rowmap(K)),
                                   logits, rowmap(Vp), B * T, V, K, bias=bias)], dev, lse=lse)
        costs, loss, ws, nbytes = _ctc_forward(logits, Vp, T * Vp, T, B, V, lse, labels_flat,
                                               label_lens, act_lens, max_label_len, blank,
                                               zero_infinity, loss_scale)
        ctx.save_for_backward(x, logits, labels_flat, label_lens, act_lens, ws)
        ctx.meta = (bias, weight, B, T, V, Vp, int(max_label_len), int(blank), float(loss_scale),
                    nbytes)
        ctx.drop = drop
        ctx.mark_non_differentiable(costs)
        return loss, costs

    @staticmethod
    def backward(ctx, g_loss, g_costs):
        x, logits, labels_flat, label_lens, act_lens, ws = ctx.saved_tensors
        bias, weight, B, T, V, Vp, max_label_len, blank, loss_scale, nbytes = ctx.meta
        dev = logits.device
        K = x.shape[-1]
        M = B * T
        dl = torch.empty(M, Vp, dtype=torch.float32, device=dev)
        g = g_loss.contiguous() if g_loss is not None else None
        N.call('asr_ctc_backward', N.ptr(logits), Vp, T * Vp, T, B, V, N.ptr(labels_flat),
               N.ptr(label_lens), N.ptr(act_lens), max_label_len, blank, N.ptr(g),
               loss_scale if g is not None else 0.0, N.ptr(dl), Vp, T * Vp, N.ptr(ws), nbytes,
               N.stream_handle(dev))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(B, T, K, dtype=torch.float32, device=dev)
            if M > 0:
                run_gemm([gemm_problem(operand(dl, 0, rowmap(Vp)), operand(weight, 1, rowmap(K)),
                                       dx, rowmap(K), M, K, V, drop=ctx.drop)], dev)

        def wgrad(gemm_opts):
            if M > 0:
                run_gemm([gemm_problem(operand(dl, 1, rowmap(Vp)), operand(x, 1, rowmap(K)),
                                       grad_buffer(weight), rowmap(K), V, K, M, beta=1.0)], dev,
                         opts=gemm_opts)
            if bias is not None:
                colsum_accumulate(dl[:, :V], grad_buffer(bias))
        gb = (grad_buffer(weight),) + ((grad_buffer(bias),) if bias is not None else ())
        if not (ctx.from_blstm is not None and os.environ.get('ASR_HEAD_WGRAD_SIDE', '1') != '0'
                and _wgrad_beside(dev, ctx.from_blstm, wgrad, (x, dl), gb)):
            wgrad(None)
        return (dx,) + (None,) * 10


def _produced_by_blstm(t, depth=4):
    """(B, H) of the BLSTMLayerFn whose output t derives from within `depth`
    autograd hops (views, permutes, fc layers), else None: its backward
    recurrence is the one a gated side stream waits for, so the overlap plan
    is built from ITS shape, not from t's width."""
    frontier = [t.grad_fn] if t.grad_fn is not None else []
    for _ in range(depth):
        nxt = []
        for fn in frontier:
            if fn is None:
                continue
            if type(fn).__name__.startswith('BLSTMLayerFn'):
                return getattr(fn, 'bh', None)
            nxt.extend(f for f, _ in getattr(fn, 'next_functions', ()))
        frontier = nxt
    return None


def linear_ctc_loss(x, weight, bias, labels_flat, label_lens, act_lens, max_label_len,
                    loss_scale=1.0, drop=None, blank=0, zero_infinity=True):
    """ctc_loss(linear(x, weight, bias, drop), ...) -> (loss [1], costs [B]);
    one fused op: LinearCTCFn when the output layer is staged in bf16,
    LinearCTC32Fn in fp32 mode (ASR_CTC_HEAD_FUSED=0 keeps the two ops)."""
    K = x.shape[-1]
    fused = os.environ.get('ASR_CTC_HEAD_FUSED', '1') != '0'
    if x.dim() == 3 and _linear_stages(x.numel() // K, K, weight.shape[0]) and fused:
        return LinearCTCFn.apply(x, weight, bias, drop, labels_flat, label_lens, act_lens,
                                 max_label_len, loss_scale, blank, zero_infinity)
    if x.dim() == 3 and compute_dtype() == F32 and fused:
        return LinearCTC32Fn.apply(x, weight, bias, drop, labels_flat, label_lens, act_lens,
                                   max_label_len, loss_scale, blank, zero_infinity)
    return ctc_loss(linear(x, weight, bias, drop), labels_flat, label_lens, act_lens,
                    max_label_len, loss_scale, blank, zero_infinity)


def linear(x, weight, bias=None, drop=None):
    """drop=(p, seed): y = dropout(x) W^T + b with dropout folded into the
    product (LinearFn)."""
    return LinearFn.apply(x, weight, bias, drop)


def _bias_pair_grad(dy2d, bias, bias2):
    """Column sums of dy2d added to the gradient of each bias that is given
    (one pass for the pair; a second bias without a first gets its own)."""
    gbs = [grad_buffer(b) for b in (bias, bias2) if b is not None]
    if gbs:
        colsum_accumulate(dy2d, *gbs)


class LinearExFn(torch.autograd.Function):
    """y = x @ W[:, c0:c0+K]^T + b + b2, with x rows optionally gathered from a
    3-D tensor at a fixed time index (x_src[b, t_index, :]).  Covers the
    decoder-input projection of all steps (columns [0, emb) of the LSTMCell
    W_ih plus both biases) and the init_dec_state 'first' / 'final' rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, bias2, c0, K, t_index):
        N.require_device(x, weight)
        x = x.contiguous()
        ldw = weight.shape[1]
        Nout = weight.shape[0]
        if t_index is None:
            M = x.numel() // K
            amap = rowmap(K)
            out_shape = tuple(x.shape[:-1]) + (Nout,)
            a_off = 0
        else:
            B, T, _ = x.shape
            M = B
            amap = rowmap(T * K)
            out_shape = (B, Nout)
            a_off = t_index * K
        y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        p = gemm_problem(operand(x, 0, amap, offset=a_off), operand(weight, 0, rowmap(ldw), offset=c0),
                         y, rowmap(Nout), M, Nout, K, bias=bias, bias2=bias2)
        run_gemm([p], x.device)
        ctx.save_for_backward(x, weight)
        ctx.meta = (bias, bias2, c0, K, t_index, M, amap, a_off)
        ctx.beside = _beside_plan[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        bias, bias2, c0, K, t_index, M, amap, a_off = ctx.meta
        dy = dy.contiguous()
        ldw, Nout = weight.shape[1], weight.shape[0]
        dx = None
        probs = []
        if ctx.needs_input_grad[0]:
            dx = torch.zeros_like(x) if t_index is not None else torch.empty_like(x)
            probs.append(gemm_problem(operand(dy, 0, rowmap(Nout)),
                                      operand(weight, 1, rowmap(ldw), offset=c0), dx, amap, M, K,
                                      Nout, c_offset=a_off))

        def wgrad(gemm_opts):
            run_gemm([gemm_problem(operand(dy, 1, rowmap(Nout)), operand(x, 1, amap, offset=a_off),
                                   grad_buffer(weight), rowmap(ldw), Nout, K, M, beta=1.0,
                                   c_offset=c0)], x.device, opts=gemm_opts)
            _bias_pair_grad(dy.view(M, Nout), bias, bias2)

        if ctx.beside is not None:
            # the weight / bias gradients beside the encoder's top backward
            # recurrence (as LinearFn's), only dX on the compute stream
            if probs:
                run_gemm(probs, x.device)
            gb = tuple(grad_buffer(t) for t in (weight, bias, bias2) if t is not None)
            if not _wgrad_beside(dy.device, ctx.beside, wgrad, (x, dy), gb):
                wgrad(None)
            return dx, None, None, None, None, None, None
        probs.append(gemm_problem(operand(dy, 1, rowmap(Nout)), operand(x, 1, amap, offset=a_off),
                                  grad_buffer(weight), rowmap(ldw), Nout, K, M, beta=1.0,
                                  c_offset=c0))
        run_gemm(probs, x.device)
        _bias_pair_grad(dy.view(M, Nout), bias, bias2)
        return dx, None, None, None, None, None, None


def linear_ex(x, weight, bias=None, bias2=None, c0=0, K=None, t_index=None):
    K = weight.shape[1] - c0 if K is None else K
    return LinearExFn.apply(x, weight, bias, bias2, c0, K, t_index)


class MeanTimeFn(torch.autograd.Function):
    """out[b] = mean_t x[b, t, :] over all T frames of [B, T, E] (padding
    included, as enc_out.mean(dim=1) in attention_seq2seq.py:832), as one
    batched GEMM ones(1 x T) . x[b] / T; backward dx[b, t] = dout[b] / T is the
    batched K = 1 product ones(T x 1) . dout[b] / T."""

    @staticmethod
    def forward(ctx, x):
        N.require_device(x)
        x = x.contiguous()
        B, T, E = x.shape
        ones = torch.ones(T, dtype=torch.float32, device=x.device)
        out = torch.empty(B, E, dtype=torch.float32, device=x.device)
        run_gemm([gemm_problem(operand(ones, 0, rowmap(T)), operand(x, 1, rowmap(E)), out,
                               rowmap(E), 1, E, T, alpha=1.0 / T, batch=B,
                               batch_strides=(0, T * E, E))], x.device)
        ctx.shape = (B, T, E)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, E = ctx.shape
        dout = dout.contiguous()
        ones = torch.ones(T, dtype=torch.float32, device=dout.device)
        dx = torch.empty(B, T, E, dtype=torch.float32, device=dout.device)
        run_gemm([gemm_problem(operand(ones, 0, rowmap(1)), operand(dout, 1, rowmap(E)), dx,
                               rowmap(E), T, E, 1, alpha=1.0 / T, batch=B,
                               batch_strides=(0, E, T * E))], dout.device)
        return dx


def mean_time(x):
    return MeanTimeFn.apply(x)


class Linear2Fn(torch.autograd.Function):
    """y = x1 W1^T + b1 + x2 W2^T + b2 (the attention bottleneck
    W_d(dec_out) + W_c(context), attention_seq2seq.py:788-790): two GEMMs into
    one output, no elementwise add pass."""

    @staticmethod
    def forward(ctx, x1, w1, b1, x2, w2, b2):
        N.require_device(x1, w1, x2, w2)
        x1, x2 = x1.contiguous(), x2.contiguous()
        K1, K2, Nout = x1.shape[-1], x2.shape[-1], w1.shape[0]
        M = x1.numel() // K1
        y = torch.empty(*x1.shape[:-1], Nout, dtype=torch.float32, device=x1.device)
        run_gemm([gemm_problem(operand(x1, 0, rowmap(K1)), operand(w1, 0, rowmap(K1)), y,
                               rowmap(Nout), M, Nout, K1, bias=b1, bias2=b2)], x1.device)
        run_gemm([gemm_problem(operand(x2, 0, rowmap(K2)), operand(w2, 0, rowmap(K2)), y,
                               rowmap(Nout), M, Nout, K2, beta=1.0)], x1.device)
        ctx.save_for_backward(x1, w1, x2, w2)
        ctx.biases = (b1, b2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, w1, x2, w2 = ctx.saved_tensors
        b1, b2 = ctx.biases
        dy = dy.contiguous()
        K1, K2, Nout = x1.shape[-1], x2.shape[-1], w1.shape[0]
        M = x1.numel() // K1
        dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
        run_gemm([gemm_problem(operand(dy, 0, rowmap(Nout)), operand(w1, 1, rowmap(K1)), dx1,
                               rowmap(K1), M, K1, Nout),
                  gemm_problem(operand(dy, 0, rowmap(Nout)), operand(w2, 1, rowmap(K2)), dx2,
                               rowmap(K2), M, K2, Nout)], x1.device)
        run_gemm([gemm_problem(operand(dy, 1, rowmap(Nout)), operand(x1, 1, rowmap(K1)),
                               grad_buffer(w1), rowmap(K1), Nout, K1, M, beta=1.0),
                  gemm_problem(operand(dy, 1, rowmap(Nout)), operand(x2, 1, rowmap(K2)),
                               grad_buffer(w2), rowmap(K2), Nout, K2, M, beta=1.0)], x1.device)
        _bias_pair_grad(dy.view(M, Nout), b1, b2)
        return dx1, None, None, dx2, None, None


def linear2(x1, w1, b1, x2, w2, b2):
    return Linear2Fn.apply(x1, w1, b1, x2, w2, b2)


# ---------------------------------------------------------------------------
# Teacher-forced location-attention decoder loop (attention_seq2seq.py:704-799)
# ---------------------------------------------------------------------------
def _attdec_forward(enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh, w_dec,
                    w_conv, conv_w, v, train_opts, keep_feat=False):
    """One asr_attdec_forward_ex call over S = pre_emb.shape[1] steps.  Returns
    (dims, (dec, cst, gates, x, ctx, aw), opts, buffers kept alive)."""
    N.require_device(enc, enc_a, lens, pre_emb, w_ih)
    B, T, E = enc.shape
    A = enc_a.shape[-1]
    D = w_hh.shape[1]
    S = pre_emb.shape[1]
    C, K = conv_w.shape[0], conv_w.shape[-1]
    dims = N.AttDecDims(B, T, E, A, C, K, D, S, float(sharpen), int(bool(sigmoid)))
    dev = enc.device
    cd = compute_dtype()
    f32 = dict(dtype=torch.float32, device=dev)
    dec = torch.empty(B, S, D, **f32)
    cst = torch.empty(B, S, D, **f32)
    gates = torch.empty(B, S, 4 * D, **f32)
    x = torch.empty(B, S, E + D, **f32)
    ctxv = torch.empty(B, S, E, **f32)
    aw = torch.empty(B, S, T, **f32)
    nb = N.query('asr_attdec_workspace_bytes', ctypes.byref(dims), cd, 0)
    ws = _ws(nb, dev)
    ld_ih = w_ih.shape[1]
    w_ih_ctx = ctypes.c_void_p(w_ih.data_ptr() + 4 * emb_dim)
    opts, keep = _attdec_opts(train_opts, B, S, D, emb_dim, w_ih, dev)
    # a backward will follow: the persistent pass keeps every step's conv
    # features for it (opts.conv_feat; ASR_ATT_CONV_FEAT=0: recomputed)
    feat = None
    if keep_feat and os.environ.get('ASR_ATT_CONV_FEAT', '1') != '0':
        fb = N.query('asr_attdec_conv_feat_bytes', ctypes.byref(dims))
        feat = torch.empty(max(int(fb) // 4, 1), dtype=torch.float32, device=dev)
        if opts is None:
            opts = N.AttDecOpts()    # all zero: what NULL means, plus the buffer
        opts.conv_feat = feat.data_ptr()
    N.call('asr_attdec_forward_ex', ctypes.byref(dims), N.ptr_struct(opts), cd, N.ptr(enc),
           N.ptr(enc_a), N.ptr(lens), w_ih_ctx, ld_ih, N.ptr(w_hh), N.ptr(w_dec),
           N.ptr(w_conv), N.ptr(conv_w), N.ptr(v), N.ptr(pre_emb),
           N.ptr(h0.contiguous() if h0 is not None else None), N.ptr(dec), N.ptr(cst),
           N.ptr(gates), N.ptr(x), N.ptr(ctxv), N.ptr(aw), N.ptr(ws), nb,
           N.stream_handle(dev))
    if feat is not None:
        ran = (ctypes.c_int * 2)()
        N.call("asr_attdec_persist_last", ctypes.cast(ran, ctypes.c_void_p))
        if ran[0] == 1:          # written only by the persistent forward pass
            keep['conv_feat'] = feat
    return dims, (dec, cst, gates, x, ctxv, aw), opts, keep


@torch.no_grad()
def att_decode_greedy(enc, enc_a, lens, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh, w_dec, w_conv,
                      conv_w, v, gen, max_len):
    """Greedy attention decoding (attention_seq2seq.py:917-1036, bahdanau
    order) as ONE fused decoder pass: every step t >= 1 is a sampled step whose
    input token is the in-loop first argmax of logits_{t-1} = fc(tanh(W_d dec +
    b_d + W_c ctx + b_c)) -- the same machinery as scheduled sampling, with no
    dropout.  S = max_len + 1 steps run so the argmax of step max_len - 1 is
    produced too.  gen: dict(w_d, b_d, w_c, b_c, w_fc, b_fc, emb_w, emb_trans,
    b_ih, b_hh).  Returns (tokens int64 [B, max_len], aw [B, max_len, T]) on
    the device, before the all-<eos> truncation."""
    enc, enc_a = enc.contiguous(), enc_a.contiguous()
    B = enc.shape[0]
    D = w_hh.shape[1]
    S = int(max_len) + 1
    pre_emb = torch.zeros(B, S, 4 * D, dtype=torch.float32, device=enc.device)  # never read
    flags = np.ones(S, np.int32)
    flags[0] = 0
    _, outs, _, keep = _attdec_forward(enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid,
                                       w_ih, w_hh, w_dec, w_conv, conv_w, v,
                                       dict(gen, ss_steps=flags))
    return keep['tok_ss'][:, 1:], outs[5][:, :S - 1]


_att_beam = {'path': None, 'ws': {}}


def _lm_struct(lm, who):
    """(asr_att_beam_lm_t of the lm dict -- cell, weight, emb, the per-layer lists
    w_ih / w_hh / b_ih / b_hh, w_out, b_out --, the tensors it points into: keep
    them until the call has been issued); who prefixes the ValueErrors."""
    if float(lm['weight']) < 0:
        raise ValueError('%s: lm weight = %r is negative' % (who, lm['weight']))
    if lm['cell'] not in ('lstm', 'gru'):
        raise ValueError("%s: lm cell = %r is not 'lstm' or 'gru'" % (who, lm['cell']))
    nl = N.ATT_BEAM_LM_MAX_LAYERS
    lk = [[t.contiguous().float() for t in lm[k][:nl]] for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')]
    lo = [lm[k].contiguous().float() for k in ('emb', 'w_out', 'b_out')]
    N.require_device(*(lo + [t for ts in lk for t in ts]))
    arr = lambda ts: (N.c_vp * nl)(*[t.data_ptr() for t in ts])   # noqa: E731
    lms = N.AttBeamLm(len(lm['w_ih']), int(lm['w_hh'][0].shape[1]), int(lo[0].shape[1]),
                      int(lo[0].shape[0]),
                      N.ATT_BEAM_CELL_GRU if lm['cell'] == 'gru' else N.ATT_BEAM_CELL_LSTM,
                      lo[0].data_ptr(), arr(lk[0]), arr(lk[1]), arr(lk[2]), arr(lk[3]),
                      lo[1].data_ptr(), lo[2].data_ptr(), float(lm['weight']))
    return lms, (lk, lo)


def last_att_beam_path():
    """'device' or 'host': what the last AttentionSeq2seq beam decode ran on
    (None before the first one); tests read it."""
    return _att_beam['path']


def _set_att_beam_path(path):
    _att_beam['path'] = path


@torch.no_grad()
def att_decode_beam(enc, enc_a, lens, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh, w_dec, w_conv,
                    conv_w, v, gen, beam_width, max_len, min_len, length_penalty, eos,
                    ctc_logits=None, ctc_weight=0, cell='lstm', lm=None):
    """Attention beam search on the device (asr_att_beam_decode, csrc/att_beam.hip;
    attention_seq2seq.py:1038-1237, bahdanau order): every utterance over its
    own lens[b] frames, f32 in both compute modes, no host read inside the
    step loop.  gen as att_decode_greedy.  ctc_weight > 0: the joint
    CTC/attention search (the call's ex->ctc) on ctc_logits [B, T, Vc],
    the raw f32 logits of the CTC head (blank 0, attention class c is CTC class
    c + 1); ctc_weight == 0 is the plain search.  cell: 'lstm' (w_ih [4D, .]),
    or 'gru' for a GRUCell decoder (w_ih [3D, .], gate rows r, z, n; ex->cell,
    plain or joint).  lm: shallow fusion with a
    language model (ex->lm), a dict of cell ('lstm'; 'gru' is
    refused: None), weight (>= 0; 0 is the search without it), emb [V, Y], the
    per-layer lists w_ih / w_hh / b_ih / b_hh, w_out [V, H] and b_out [V], all
    f32 on the device; an LM of another V raises.  Returns (tokens int64 [B, max_len],
    lengths int32 [B], scores float64 [B], aw float32 [B, max_len, T]) on the
    device, or None when the kernels do not cover the shape
    (ASR_ERR_UNSUPPORTED; the reason is asr_last_error's)."""
    N.require_device(enc, enc_a, w_ih)
    if cell not in ('lstm', 'gru'):
        raise ValueError("att_decode_beam: cell = %r is not 'lstm' or 'gru'" % (cell,))
    enc, enc_a = enc.contiguous().float(), enc_a.contiguous().float()
    B, T, E = enc.shape
    A = enc_a.shape[-1]
    D = w_hh.shape[1]
    gates = 4 if cell == 'lstm' else 3
    if w_ih.shape[0] != gates * D or w_hh.shape[0] != gates * D:
        raise ValueError('att_decode_beam: a %s cell needs w_ih / w_hh of %d x D rows, got %s, %s'
                         % (cell, gates, tuple(w_ih.shape), tuple(w_hh.shape)))
    C, K = conv_w.shape[0], conv_w.shape[-1]
    dev = enc.device
    V, Dz = gen['w_fc'].shape
    dims = N.AttDecDims(B, T, E, A, C, K, D, 1, float(sharpen), int(bool(sigmoid)))
    if torch.is_tensor(lens):
        lens_d = lens.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:
        lens_d = h2d(np.asarray(lens, np.int32).reshape(-1), dev)
    W, max_len = int(beam_width), int(max_len)
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('att_decode_beam: ctc_weight = %r outside [0, 1]' % (ctc_weight,))
    if lam > 0:
        if ctc_logits is None:
            raise ValueError('att_decode_beam: ctc_weight > 0 needs ctc_logits')
        ctc_logits = ctc_logits.contiguous().float()
        if ctc_logits.dim() != 3 or tuple(ctc_logits.shape[:2]) != (B, T):
            raise ValueError('att_decode_beam: ctc_logits %s is not [%d, %d, Vc]'
                             % (tuple(ctc_logits.shape), B, T))
        N.require_device(ctc_logits)
    if lm is not None and float(lm['weight']) == 0:
        lm = None
    lms, lm_keep = _lm_struct(lm, 'att_decode_beam') if lm is not None else (None, None)
    ctc = N.AttBeamCtc(ctc_logits.data_ptr(), int(ctc_logits.shape[2]), 0, 1, lam) if lam > 0 \
        else None
    ex = N.AttBeamEx(N.ATT_BEAM_CELL_GRU if cell == 'gru' else N.ATT_BEAM_CELL_LSTM,
                     ctypes.addressof(ctc) if ctc is not None else None,
                     ctypes.addressof(lms) if lms is not None else None)
    nb = N.query('asr_att_beam_ws_bytes', ctypes.byref(dims), W, int(V), int(emb_dim), int(Dz),
                 max_len, ctypes.byref(ex))
    if nb == 0:
        return None
    ws = _grown_ws(_att_beam['ws'], nb, dev)
    keep = [t.contiguous() for t in (w_ih, w_hh, gen['b_ih'], gen['b_hh'], w_dec, w_conv, conv_w,
                                     v, gen['w_d'], gen['w_c'], gen['w_fc'], gen['emb_w'])]
    kb = [None if gen[k] is None else gen[k].contiguous() for k in ('b_d', 'b_c', 'b_fc')]
    pv = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    opts = N.AttBeamOpts(W, int(V), int(emb_dim), int(Dz), max_len, int(min_len), int(eos),
                         int(gen['emb_trans']), float(length_penalty), keep[0].shape[1],
                         pv(keep[0]), pv(keep[1]), pv(keep[2]), pv(keep[3]), pv(keep[4]),
                         pv(keep[5]), pv(keep[6]), pv(keep[7]), pv(keep[8]), pv(kb[0]),
                         pv(keep[9]), pv(kb[1]), pv(keep[10]), pv(kb[2]), pv(keep[11]))
    tokens = torch.empty(B, max_len, dtype=torch.int64, device=dev)
    hl = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    aw = torch.empty(B, max_len, T, dtype=torch.float32, device=dev)
    h0c = h0.contiguous().float() if h0 is not None else None
    rc = N.lib().asr_att_beam_decode(
        ctypes.byref(dims), ctypes.byref(opts), ctypes.byref(ex), N.ptr(enc), N.ptr(enc_a),
        N.ptr(lens_d), N.ptr(h0c), N.ptr(ws), ws.numel(), N.ptr(tokens), N.ptr(hl), N.ptr(scores),
        N.ptr(aw), N.stream_handle(dev))
    del lm_keep
    if rc == N.ASR_ERR_UNSUPPORTED:
        return None
    if rc != N.ASR_OK:
        raise N.NativeError('asr_att_beam_decode failed (rc=%d): %s'
                            % (rc, N.lib().asr_last_error().decode(errors='replace')))
    return tokens, hl, scores, aw


_last_sampled = {'tok': None}


def last_sampled_tokens():
    """The sampled tokens [B, S] (int64, device; -1 at teacher-forced steps)
    of the last fused decoder forward that had sampled steps, else None (the
    decoder pass's tok_ss output; tests read it)."""
    return _last_sampled['tok']


class AttDecoderFn(torch.autograd.Function):
    """Returns (dec_out [B,S,D], ctx [B,S,E], aw [B,S,T]).  Weights:
    w_ih [4D, emb+E] (LSTMCell; only the context columns are used here, the
    embedding columns enter through pre_emb), w_hh [4D, D], w_dec [A, D],
    w_conv [A, C], conv_w [C,1,1,K], v [1, A]."""

    @staticmethod
    def forward(ctx, enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh,
                w_dec, w_conv, conv_w, v, train_opts):
        enc, enc_a, pre_emb = enc.contiguous(), enc_a.contiguous(), pre_emb.contiguous()
        dims, (dec, cst, gates, x, ctxv, aw), opts, keep = _attdec_forward(
            enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh, w_dec, w_conv,
            conv_w, v, train_opts, keep_feat=any(ctx.needs_input_grad))
        ctx.save_for_backward(enc, enc_a, lens, w_ih, w_hh, w_dec, w_conv, conv_w, v, dec, cst,
                              gates, x, aw)
        _last_sampled['tok'] = keep.get('tok_ss')
        ctx.meta = (dims, emb_dim, h0 is not None)
        ctx.opts = (opts, keep, train_opts)
        ctx.mark_non_differentiable(aw)
        return dec, ctxv, aw

    @staticmethod
    def backward(ctx, d_dec, d_ctx, d_aw):
        (enc, enc_a, lens, w_ih, w_hh, w_dec, w_conv, conv_w, v, dec, cst, gates, x,
         aw) = ctx.saved_tensors
        dims, emb_dim, has_h0 = ctx.meta
        B, T, E, A, C, K, D, S = (dims.B, dims.T, dims.E, dims.A, dims.C, dims.K, dims.D, dims.S)
        dev = enc.device
        cd = compute_dtype()
        f32 = dict(dtype=torch.float32, device=dev)
        d_dec = d_dec.contiguous() if d_dec is not None else torch.zeros(B, S, D, **f32)
        d_ctx = d_ctx.contiguous() if d_ctx is not None else torch.zeros(B, S, E, **f32)
        dctx_tot = torch.empty(B, S, E, **f32)
        d_enc_a = torch.empty(B, T, A, **f32)
        d_h0 = torch.empty(B, D, **f32) if has_h0 else None
        dwd = torch.empty(B, S, A, **f32)
        nrow = B * N.query('asr_attdec_chunks', ctypes.byref(dims))   # per frame chunk
        dv_part = torch.empty(nrow, A, **f32)
        dwc_part = torch.empty(nrow, A * C, **f32)
        dcw_part = torch.empty(nrow, C * K, **f32)
        nb = N.query('asr_attdec_workspace_bytes', ctypes.byref(dims), cd, 1)
        ws = _ws(nb, dev)
        ld_ih = w_ih.shape[1]
        w_ih_ctx = ctypes.c_void_p(w_ih.data_ptr() + 4 * emb_dim)
        opts, keep, train_opts = ctx.opts
        sampled = 'emb_ss' in keep
        if sampled:
            d_pre = torch.empty(B, S, 4 * D, **f32)
            dg_ss = torch.empty(B, S, 4 * D, **f32)
            opts.d_pre, opts.dg_ss = d_pre.data_ptr(), dg_ss.data_ptr()
        if opts is not None:   # only the buffer a persistent forward wrote
            feat = keep.get('conv_feat')
            opts.conv_feat = feat.data_ptr() if feat is not None else None
        N.call('asr_attdec_backward_ex', ctypes.byref(dims), N.ptr_struct(opts), cd,
               N.ptr(enc), N.ptr(enc_a), N.ptr(lens), w_ih_ctx, ld_ih, N.ptr(w_hh),
               N.ptr(w_dec), N.ptr(w_conv), N.ptr(conv_w), N.ptr(v), N.ptr(dec), N.ptr(cst),
               N.ptr(aw), N.ptr(d_dec), N.ptr(d_ctx), N.ptr(gates), N.ptr(dctx_tot),
               N.ptr(d_enc_a), N.ptr(d_h0), N.ptr(dwd), N.ptr(dv_part), N.ptr(dwc_part),
               N.ptr(dcw_part), N.ptr(ws), nb, N.stream_handle(dev))
        dg = gates                          # dgates (row t = 0 is zero)
        d_pre_out = dg
        if sampled:
            # sampled steps were fed embed(argmax) (detached): their gate gradients
            # reach W_ih[:, :Y] through the embedding actually used and both
            # biases, never the teacher embedding (attention_seq2seq.py:744-748)
            emb_ss = keep['emb_ss']
            Y = emb_dim
            run_gemm([gemm_problem(operand(dg_ss, 1, rowmap(4 * D)), operand(emb_ss, 1, rowmap(Y)),
                                   grad_buffer(w_ih), rowmap(ld_ih), 4 * D, Y, B * S, beta=1.0)],
                     dev)
            colsum_accumulate(dg_ss.view(B * S, 4 * D), grad_buffer(train_opts['b_ih']),
                              grad_buffer(train_opts['b_hh']))
            d_pre_out = d_pre
        BS, G, ED = B * S, 4 * D, E + D
        # LSTMCell weights: dW_ih[:, emb:] += dG^T x[:, :E]; dW_hh += dG^T x[:, E:]
        run_gemm([gemm_problem(operand(dg, 1, rowmap(G)), operand(x, 1, rowmap(ED)),
                               grad_buffer(w_ih), rowmap(ld_ih), G, E, BS, beta=1.0,
                               c_offset=emb_dim),
                  gemm_problem(operand(dg, 1, rowmap(G)), operand(x, 1, rowmap(ED), offset=E),
                               grad_buffer(w_hh), rowmap(D), G, D, BS, beta=1.0)], dev)
        # attention weights
        run_gemm([gemm_problem(operand(dwd, 1, rowmap(A)), operand(dec, 1, rowmap(D)),
                               grad_buffer(w_dec), rowmap(D), A, D, BS, beta=1.0)], dev)
        colsum_accumulate(dv_part, grad_buffer(v))
        colsum_accumulate(dwc_part, grad_buffer(w_conv))
        colsum_accumulate(dcw_part, grad_buffer(conv_w))
        # d enc[b] = aw[b]^T dctx_tot[b]   (batched over utterances)
        d_enc = torch.empty_like(enc)
        run_gemm([gemm_problem(operand(aw, 1, rowmap(T)), operand(dctx_tot, 1, rowmap(E)), d_enc,
                               rowmap(E), T, E, S, batch=B,
                               batch_strides=(S * T, S * E, T * E))], dev)
        return (d_enc, d_enc_a, None, d_pre_out, d_h0, None, None, None, None, None, None, None,
                None, None, None)


class AttStepFn(torch.autograd.Function):
    """One location-attention step (AttentionMechanism.forward,
    attention_layer.py:123-251) on the decoder loop's kernels:
    (enc [B,T,E], enc_a [B,T,A], lens int32 [B], dec_out [B,D], aw_prev [B,T])
    -> (ctx [B,E], aw [B,T]).  Weight gradients (W_dec [A,D], W_conv [A,C],
    conv [C,1,1,K], V [1,A]) accumulate into their .grad."""

    @staticmethod
    def forward(ctx, enc, enc_a, lens, dec_out, aw_prev, w_dec, w_conv, conv_w, v, sharpen,
                sigmoid):
        N.require_device(enc, enc_a, lens, dec_out, aw_prev, w_dec)
        enc, enc_a = enc.contiguous(), enc_a.contiguous()
        dec_out, aw_prev = dec_out.contiguous(), aw_prev.contiguous()
        B, T, E = enc.shape
        A, D = w_dec.shape
        C, K = conv_w.shape[0], conv_w.shape[-1]
        dims = N.AttDecDims(B, T, E, A, C, K, D, 2, float(sharpen), int(bool(sigmoid)))
        dev = enc.device
        ctx_out = torch.empty(B, E, dtype=torch.float32, device=dev)
        aw_out = torch.empty(B, T, dtype=torch.float32, device=dev)
        nb = N.query('asr_att_step_workspace_bytes', ctypes.byref(dims))
        ws = _ws(nb, dev)
        N.call('asr_att_step_forward', ctypes.byref(dims), N.ptr(enc), N.ptr(enc_a), N.ptr(lens),
               N.ptr(w_dec), N.ptr(w_conv), N.ptr(conv_w), N.ptr(v), N.ptr(dec_out),
               N.ptr(aw_prev), N.ptr(ctx_out), N.ptr(aw_out), N.ptr(ws), nb,
               N.stream_handle(dev))
        ctx.save_for_backward(enc, enc_a, lens, dec_out, aw_prev, w_dec, w_conv, conv_w, v,
                              aw_out)
        ctx.dims = dims
        return ctx_out, aw_out

    @staticmethod
    def backward(ctx, d_ctx, d_aw):
        enc, enc_a, lens, dec_out, aw_prev, w_dec, w_conv, conv_w, v, aw_out = ctx.saved_tensors
        dims = ctx.dims
        B, T, E, A, C, K, D = dims.B, dims.T, dims.E, dims.A, dims.C, dims.K, dims.D
        dev = enc.device
        f32 = dict(dtype=torch.float32, device=dev)
        d_ctx = d_ctx.contiguous() if d_ctx is not None else torch.zeros(B, E, **f32)
        d_aw = d_aw.contiguous() if d_aw is not None else None
        d_enc_a = torch.empty(B, T, A, **f32)
        d_dec = torch.empty(B, D, **f32)
        d_aw_prev = torch.empty(B, T, **f32)
        dctx_tot = torch.empty(B, E, **f32)
        dwd = torch.empty(B, A, **f32)
        nrow = B * N.query('asr_attdec_chunks', ctypes.byref(dims))
        dv_part = torch.empty(nrow, A, **f32)
        dwc_part = torch.empty(nrow, A * C, **f32)
        dcw_part = torch.empty(nrow, C * K, **f32)
        nb = N.query('asr_att_step_workspace_bytes', ctypes.byref(dims))
        ws = _ws(nb, dev)
        N.call('asr_att_step_backward', ctypes.byref(dims), N.ptr(enc), N.ptr(enc_a), N.ptr(lens),
               N.ptr(w_dec), N.ptr(w_conv), N.ptr(conv_w), N.ptr(v), N.ptr(dec_out),
               N.ptr(aw_prev), N.ptr(aw_out), N.ptr(d_ctx), N.ptr(d_aw), N.ptr(d_enc_a),
               N.ptr(d_dec), N.ptr(d_aw_prev), N.ptr(dctx_tot), N.ptr(dwd), N.ptr(dv_part),
               N.ptr(dwc_part), N.ptr(dcw_part), N.ptr(ws), nb, N.stream_handle(dev))
        run_gemm([gemm_problem(operand(dwd, 1, rowmap(A)), operand(dec_out, 1, rowmap(D)),
                               grad_buffer(w_dec), rowmap(D), A, D, B, beta=1.0)], dev)
        colsum_accumulate(dv_part, grad_buffer(v))
        colsum_accumulate(dwc_part, grad_buffer(w_conv))
        colsum_accumulate(dcw_part, grad_buffer(conv_w))
        d_enc = torch.empty_like(enc)      # d enc[b] = aw_out[b]^T dctx_tot[b] (K = 1)
        run_gemm([gemm_problem(operand(aw_out, 1, rowmap(T)), operand(dctx_tot, 1, rowmap(E)),
                               d_enc, rowmap(E), T, E, 1, batch=B,
                               batch_strides=(T, E, T * E))], dev)
        return d_enc, d_enc_a, None, d_dec, d_aw_prev, None, None, None, None, None, None


class AttHeadsRefused(N.NativeError):
    """asr_att_heads_forward does not take the shape (ASR_ERR_UNSUPPORTED)."""


_att_heads = {'path': None}


def last_att_heads_path():
    """'heads' (one launch over all heads) or 'loop' (a refused shape: one
    att_step per head): what the last att_heads_step ran (tests read it)."""
    return _att_heads['path']


def _att_heads_params(B, T, E, A, C, K, D, H, kind, sharpen, sigmoid, weights):
    """asr_att_heads_t; weights: per head (w_dec, w_conv, conv_w, v) tensors
    (None where the kind has none)."""
    P = N.AttHeads(B, T, E, A, C, K, D, H,
                   N.ATT_HEADS_DOT if kind == 'dot' else N.ATT_HEADS_ADDITIVE, float(sharpen),
                   int(bool(sigmoid)))
    for h, ws in enumerate(weights[:N.ATT_HEADS_MAX]):
        for name, w in zip(('w_dec', 'w_conv', 'conv_w', 'v'), ws):
            getattr(P, name)[h] = None if w is None else w.data_ptr()
    return P


class AttHeadsStepFn(torch.autograd.Function):
    """One attention step over H heads in one launch (csrc/att_heads.hip;
    attention_layer.py:141-251): (enc [B,T,E], enc_a [H,B,T,A] head-major,
    lens int32 [B], dec_out [B,D], aw_prev [B,H,T]) -> (ctx [B,H*E],
    aw [B,H,T]).  kind 'additive' (per head W_dec [A,D], V [1,A] and, for
    location attention, W_conv [A,C], conv [C,1,1,K]; the flat ``weights`` are
    those four per head, absent ones left out) or 'dot' (no weights, A = D).
    f32 in both compute modes, its backward products included.  Weight
    gradients accumulate into their .grad."""

    @staticmethod
    def forward(ctx, enc, enc_a, lens, dec_out, aw_prev, kind, sharpen, sigmoid, C, *weights):
        N.require_device(enc, enc_a, lens, dec_out, aw_prev)
        enc, enc_a = enc.contiguous(), enc_a.contiguous()
        dec_out, aw_prev = dec_out.contiguous(), aw_prev.contiguous()
        B, T, E = enc.shape
        H, A = enc_a.shape[0], enc_a.shape[3]
        D = dec_out.shape[1]
        per = 0 if kind == 'dot' else (4 if C else 2)
        assert len(weights) == per * H
        heads = []
        for h in range(H):
            w = [t.contiguous() for t in weights[per * h:per * (h + 1)]]
            heads.append((None,) * 4 if kind == 'dot' else
                         (w[0], w[1], w[2], w[3]) if C else (w[0], None, None, w[1]))
        K = heads[0][2].shape[-1] if C else 1
        P = _att_heads_params(B, T, E, A, C, K, D, H, kind, sharpen, sigmoid, heads)
        dev = enc.device
        ctx_out = torch.empty(B, H * E, dtype=torch.float32, device=dev)
        aw_out = torch.empty(B, H, T, dtype=torch.float32, device=dev)
        rc = N.lib().asr_att_heads_forward(
            ctypes.byref(P), N.ptr(enc), N.ptr(enc_a), N.ptr(lens), N.ptr(dec_out),
            N.ptr(aw_prev), N.ptr(ctx_out), N.ptr(aw_out), None, 0, N.stream_handle(dev))
        if rc != N.ASR_OK:
            msg = N.lib().asr_last_error().decode(errors='replace')
            raise (AttHeadsRefused if rc == N.ASR_ERR_UNSUPPORTED else N.NativeError)(
                'asr_att_heads_forward failed (rc=%d): %s' % (rc, msg))
        ctx.save_for_backward(enc, enc_a, lens, dec_out, aw_prev, aw_out)
        ctx.heads = heads
        ctx.P = P
        return ctx_out, aw_out

    @staticmethod
    def backward(ctx, d_ctx, d_aw):
        enc, enc_a, lens, dec_out, aw_prev, aw_out = ctx.saved_tensors
        P, heads = ctx.P, ctx.heads
        B, T, E, A, C, K, D, H = P.B, P.T, P.E, P.A, P.C, P.K, P.D, P.H
        dot = P.kind == N.ATT_HEADS_DOT
        dev = enc.device
        f32 = dict(dtype=torch.float32, device=dev)
        d_ctx = d_ctx.contiguous() if d_ctx is not None else torch.zeros(B, H * E, **f32)
        d_aw = d_aw.contiguous() if d_aw is not None else None
        d_enc_a = torch.empty(H, B, T, A, **f32)
        d_dec = torch.empty(B, D, **f32)
        d_aw_prev = torch.empty(B, H, T, **f32)
        dctx_tot = torch.empty(B, H, E, **f32)
        dwd = dv_part = dwc_part = dcw_part = None
        if not dot:
            dwd = torch.empty(H, B, A, **f32)
            dv_part = torch.empty(H, B, A, **f32)
            if C:
                dwc_part = torch.empty(H, B, A * C, **f32)
                dcw_part = torch.empty(H, B, C * K, **f32)
        nb = N.query('asr_att_heads_workspace_bytes', ctypes.byref(P), 1)
        ws = _ws(nb, dev)
        N.call('asr_att_heads_backward', ctypes.byref(P), N.ptr(enc), N.ptr(enc_a), N.ptr(lens),
               N.ptr(dec_out), N.ptr(aw_prev), N.ptr(aw_out), N.ptr(d_ctx), N.ptr(d_aw),
               N.ptr(d_enc_a), N.ptr(d_dec), N.ptr(d_aw_prev), N.ptr(dctx_tot), N.ptr(dwd),
               N.ptr(dv_part), N.ptr(dwc_part), N.ptr(dcw_part), N.ptr(ws), nb,
               N.stream_handle(dev))
        if not dot:
            probs = [gemm_problem(operand(dwd[h], 1, rowmap(A)), operand(dec_out, 1, rowmap(D)),
                                  grad_buffer(heads[h][0]), rowmap(D), A, D, B, beta=1.0)
                     for h in range(H)]
            for i in range(0, H, 2):           # dW_dec_h += dwd_h^T dec, two heads a launch
                run_gemm(probs[i:i + 2], dev, cd=F32)
            for h in range(H):
                colsum_accumulate(dv_part[h], grad_buffer(heads[h][3]))
                if C:
                    colsum_accumulate(dwc_part[h], grad_buffer(heads[h][1]))
                    colsum_accumulate(dcw_part[h], grad_buffer(heads[h][2]))
        d_enc = torch.empty_like(enc)          # d enc[b] = aw[b]^T dctx_tot[b]  (K = H)
        run_gemm([gemm_problem(operand(aw_out, 1, rowmap(T)), operand(dctx_tot, 1, rowmap(E)),
                               d_enc, rowmap(E), T, E, H, batch=B,
                               batch_strides=(H * T, H * E, T * E))], dev, cd=F32)
        return (d_enc, d_enc_a, None, d_dec, d_aw_prev, None, None, None, None) + (None,) * (
            len(heads) * (0 if dot else (4 if C else 2)))


def att_heads_step(enc, enc_a, lens, dec_out, aw_prev, heads, kind, sharpen=1.0, sigmoid=False):
    """One attention step over all heads at the layer boundary:
    (enc [B,T,E], enc_a [B,T,A,H], lens int32 [B], dec_out [B,D], aw_prev
    [B,T,H]) -> (ctx [B,H*E] head-major, aw [B,T,H]).  heads: per head a dict
    of weight tensors -- 'additive': w_dec [A,D], v [1,A] and, for location
    attention, w_conv [A,C], conv_w [C,1,1,K]; 'dot': empty.  An enc_a that is
    the permuted view of a head-major [H,B,T,A] tensor
    (AttentionMechanism.enc_projection) is passed on without a copy, as is the
    aw this op returned.  A shape the kernels refuse runs one att_step per head
    ('additive') or raises ('dot': there is no other dot-product kernel)."""
    if kind not in ('additive', 'dot'):
        raise ValueError("kind must be 'additive' or 'dot'")
    H = len(heads)
    C = 0
    flat = []
    if kind == 'additive':
        C = heads[0]['conv_w'].shape[0] if heads[0].get('conv_w') is not None else 0
        for hd in heads:
            flat += [hd['w_dec'], hd['w_conv'], hd['conv_w'], hd['v']] if C else [hd['w_dec'],
                                                                                  hd['v']]
    try:
        ctx, aw = AttHeadsStepFn.apply(enc, enc_a.permute(3, 0, 1, 2), lens, dec_out,
                                       aw_prev.permute(0, 2, 1), kind, float(sharpen),
                                       bool(sigmoid), C, *flat)
        _att_heads['path'] = 'heads'
        return ctx, aw.permute(0, 2, 1)
    except AttHeadsRefused as e:
        if kind == 'dot':
            raise N.NativeError('dot-product attention: the shape is outside the multi-head '
                                'kernel and there is no per-head kernel for it (%s)' % e)
    _att_heads['path'] = 'loop'
    A = enc_a.shape[2]
    ctxs, aws = [], []
    for h, hd in enumerate(heads):
        if C:
            w_conv, conv_w = hd['w_conv'], hd['conv_w']
        else:       # content: one all-zero conv channel adds an exact 0.0
            w_conv = torch.zeros(A, 1, device=enc.device)
            conv_w = torch.zeros(1, 1, 1, 1, device=enc.device)
        c, a = att_step(enc, enc_a[..., h], lens, dec_out, aw_prev[..., h], hd['w_dec'], w_conv,
                        conv_w, hd['v'], sharpen, sigmoid)
        ctxs.append(c)
        aws.append(a)
    return torch.cat(ctxs, dim=-1), torch.stack(aws, dim=-1)


class LSTMCellFn(torch.autograd.Function):
    """nn.LSTMCell nonlinearity on gate pre-activations: (pre [B,4D], c_prev
    [B,D]) -> (h, c).  The GEMMs are linear2 (x W_ih^T + b_ih + h W_hh^T + b_hh)."""

    @staticmethod
    def forward(ctx, pre, c_prev):
        N.require_device(pre, c_prev)
        pre, c_prev = pre.contiguous(), c_prev.contiguous()
        B, G = pre.shape
        D = G // 4
        act = torch.empty_like(pre)
        h = torch.empty(B, D, dtype=torch.float32, device=pre.device)
        c = torch.empty(B, D, dtype=torch.float32, device=pre.device)
        N.call('asr_lstm_cell_forward', N.ptr(pre), N.ptr(c_prev), B, D, N.ptr(act), N.ptr(h),
               N.ptr(c), N.stream_handle(pre.device))
        ctx.save_for_backward(act, c_prev, c)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        act, c_prev, c = ctx.saved_tensors
        B, D = c.shape
        dpre = torch.empty_like(act)
        dc_prev = torch.empty_like(c)
        N.call('asr_lstm_cell_backward', N.ptr(act), N.ptr(c_prev), N.ptr(c),
               N.ptr(dh.contiguous() if dh is not None else None),
               N.ptr(dc.contiguous() if dc is not None else None), B, D, N.ptr(dpre),
               N.ptr(dc_prev), N.stream_handle(c.device))
        return dpre, dc_prev


class GRUCellFn(torch.autograd.Function):
    """nn.GRUCell nonlinearity on the two GEMM outputs (gi = x W_ih^T + b_ih,
    gh = h W_hh^T + b_hh, [B, 3D]) and h -> h' (csrc/gru.hip)."""

    @staticmethod
    def forward(ctx, gi, gh, h):
        N.require_device(gi, gh, h)
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        B, D = h.shape
        act = torch.empty_like(gi)
        hout = torch.empty_like(h)
        N.call('asr_gru_cell_forward', N.ptr(gi), N.ptr(gh), N.ptr(h), B, D, N.ptr(act),
               N.ptr(hout), N.stream_handle(h.device))
        ctx.save_for_backward(act, gh, h)
        return hout

    @staticmethod
    def backward(ctx, dh):
        act, gh, h = ctx.saved_tensors
        B, D = h.shape
        dgi, dgh = torch.empty_like(act), torch.empty_like(act)
        dh_prev = torch.empty_like(h)
        N.call('asr_gru_cell_backward', N.ptr(act), N.ptr(gh), N.ptr(h), N.ptr(dh.contiguous()),
               B, D, N.ptr(dgi), N.ptr(dgh), N.ptr(dh_prev), N.stream_handle(h.device))
        return dgi, dgh, dh_prev


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    """One nn.GRUCell step on the HIP GEMM + cell kernels."""
    return GRUCellFn.apply(linear(x, w_ih, b_ih), linear(h, w_hh, b_hh), h)


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One nn.LSTMCell step on the HIP GEMM + cell kernels."""
    pre = linear2(x, w_ih, b_ih, h, w_hh, b_hh)
    return LSTMCellFn.apply(pre, c)


def att_step(enc, enc_a, lens, dec_out, aw_prev, w_dec, w_conv, conv_w, v, sharpen=1.0,
             sigmoid=False):
    return AttStepFn.apply(enc, enc_a, lens, dec_out, aw_prev, w_dec, w_conv, conv_w, v, sharpen,
                           sigmoid)


def _attdec_opts(o, B, S, D, Y, w_ih, dev):
    """asr_attdec_opts_t from the training options dict (None = inference
    semantics: no dropout, teacher forcing).  Returns (opts | None, buffers to
    keep alive)."""
    keep = {}
    if not o:
        return None, keep
    opts = N.AttDecOpts()
    opts.dropout_hidden = float(o.get('dropout_hidden', 0.0))
    opts.seed_hidden = int(o.get('seed_hidden', 0))
    ss = o.get('ss_steps')
    if ss is not None and np.any(ss[1:]):
        flags = np.ascontiguousarray(ss, dtype=np.int32)
        keep['flags'] = flags
        f32 = dict(dtype=torch.float32, device=dev)
        keep['pre_ss'] = torch.empty(B, S, 4 * D, **f32)
        keep['emb_ss'] = torch.zeros(B, S, Y, **f32)
        keep['tok_ss'] = torch.full((B, S), -1, dtype=torch.int64, device=dev)
        opts.ss_steps_host = flags.ctypes.data
        opts.Y, opts.Dz, opts.V = Y, o['w_d'].shape[0], o['w_fc'].shape[0]
        for k in ('w_d', 'b_d', 'w_c', 'b_c', 'w_fc', 'b_fc', 'emb_w', 'b_ih', 'b_hh'):
            setattr(opts, k, o[k].data_ptr() if o.get(k) is not None else None)
        opts.drop_d, opts.seed_d = float(o.get('drop_d', 0.0)), int(o.get('seed_d', 0))
        opts.drop_c, opts.seed_c = float(o.get('drop_c', 0.0)), int(o.get('seed_c', 0))
        opts.drop_emb, opts.seed_emb = float(o.get('drop_emb', 0.0)), int(o.get('seed_emb', 0))
        opts.emb_trans = int(o.get('emb_trans', 0))
        opts.w_ih_emb, opts.ld_ih = w_ih.data_ptr(), w_ih.shape[1]
        opts.pre_ss = keep['pre_ss'].data_ptr()
        opts.emb_ss = keep['emb_ss'].data_ptr()
        opts.tok_ss = keep['tok_ss'].data_ptr()
    return opts, keep


def att_decoder(enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid, w_ih, w_hh, w_dec,
                w_conv, conv_w, v, train_opts=None):
    """train_opts (training mode): dict with dropout_hidden / seed_hidden and,
    for scheduled sampling, ss_steps (host int array [S]) plus the weights
    w_d, b_d, w_c, b_c, w_fc, b_fc, emb_w (emb_trans), b_ih, b_hh and the
    bottleneck / embedding dropout rates and seeds (drop_d, seed_d, drop_c,
    seed_c, drop_emb, seed_emb)."""
    return AttDecoderFn.apply(enc, enc_a, lens, pre_emb, h0, emb_dim, sharpen, sigmoid, w_ih,
                              w_hh, w_dec, w_conv, conv_w, v, train_opts)


# ---------------------------------------------------------------------------
# One bidirectional LSTM layer (nn.LSTM bidirectional + pack/pad, rnn.py)
# ---------------------------------------------------------------------------
class _InputMap(collections.namedtuple('_InputMap', 'perm t_mul t_add T T_src Dsrc Din')):
    """A recurrent layer's input addressing: row (b, t), t < T, of the layer
    input is the Din values at x_src[perm[b] if perm else b, t*t_mul + t_add]
    of x_src [B, T_src, Dsrc] (Din = 2 * Dsrc: that frame and the next one,
    'concat' subsampling read in place)."""
    __slots__ = ()

    def rows(self, ta=0, tb=None):
        """The row map reading X / scattering dX: rows t in [ta, tb) (default: all T)."""
        tb = self.T if tb is None else tb
        return rowmap(self.Dsrc, stride_b=self.T_src * self.Dsrc, rows_per_b=tb - ta,
                      t_mul=self.t_mul, t_add=self.t_add + ta * self.t_mul,
                      t_limit=self.T_src, perm=self.perm)

    @property
    def is_identity(self):
        return (self.perm is None and self.t_mul == 1 and self.t_add == 0
                and self.T == self.T_src and self.Din == self.Dsrc)

    def alloc_dx(self, B, dev):
        """dX [B, T_src, Dsrc]; zero where a non-identity map may leave frames unwritten."""
        fill = torch.empty if self.is_identity else torch.zeros
        return fill(B, self.T_src, self.Dsrc, dtype=torch.float32, device=dev)


class BLSTMLayerFn(torch.autograd.Function):
    """x_src [B, T_src, Din] f32; the layer input row (b, t) is
    x_src[perm[b] if perm else b, t*t_mul + t_add].  Parameters are passed as
    (w_ih [8H, Din], w_hh [8H, H], b_ih [8H], b_hh [8H]) where each is the
    forward-direction tensor immediately followed in memory by the reverse one
    (the flat layout of models/pytorch_v3/base.py).

    bf16 mode stages every GEMM operand in bf16 once (the gathered input X and
    W_ih by one conversion pass each; y and dG are written in bf16 by the
    recurrence kernels themselves), so all four layer GEMMs take the
    buffer->LDS bf16 fast path of gemm.hip.  fp32 mode reads the f32 tensors
    directly (exact-f32 MFMA, parity mode)."""

    @staticmethod
    def forward(ctx, x_src, lens, T, perm, t_mul, t_add, gbufs, concat, drop, next_rec, out_spec,
                w_ih, w_hh, b_ih, b_hh, *graph_params):
        N.require_device(x_src, lens, w_ih, w_hh, b_ih, b_hh)
        # the layer below handed its output over as staged bf16 (bf16_handoff)
        twin = _handoff_input(x_src, perm, t_mul, t_add, T, concat, drop, w_ih.shape[1])
        x_src = x_src.contiguous()
        fused_drop = drop is not None and compute_dtype() == BF16 and not concat
        if drop is not None and not fused_drop:   # materialise dropout(x_src) first
            xd = torch.empty_like(x_src)
            N.call('asr_dropout', N.ptr(x_src), N.ptr(xd), x_src.numel(), float(drop[0]),
                   int(drop[1]), N.stream_handle(x_src.device))
            x_src = xd
        B, T_src, Dsrc = x_src.shape
        # concat: the input row (b, t) spans source frames t*t_mul + t_add and the
        # next one (rnn.py:421-431), i.e. 2*Dsrc contiguous values
        Din = 2 * Dsrc if concat else Dsrc
        assert w_ih.shape[1] == Din, (tuple(w_ih.shape), Din)
        H = w_hh.shape[1]
        dev = x_src.device
        cd = compute_dtype()
        in_map = _InputMap(perm, t_mul, t_add, T, T_src, Dsrc, Din)
        a_map = in_map.rows()
        Dp = Din
        if twin is not None:
            x_op = twin.view(B * T, Din)
            w_op = _wih_bf16(w_ih, graph_params, H, Din)           # [8H, Din]
        elif cd == BF16:
            if Din % 8 and not fused_drop:
                # an input width that is not a multiple of 8 (TIMIT's 123) is
                # staged with zero-padded rows of Dp columns, so the fused
                # projection and the fast GEMMs take it (the zero columns add
                # nothing): no generic-kernel GEMMs on layer 0
                Dp = (Din + 7) // 8 * 8
                x_op = torch.empty(B * T, Dp, dtype=torch.bfloat16, device=dev)
                N.call('asr_convert_rows_bf16_ld', N.ptr(x_src), a_map, B * T, Din, Dp,
                       N.ptr(x_op), N.stream_handle(dev))
                w_op = _staged(w_ih, 8 * H, Din, Dp)                  # [8H, Dp]
            else:
                x_op = convert_rows_bf16(x_src, a_map, B * T, Din,    # [B*T, Din]
                                         drop=drop if fused_drop else None)
                w_op = _wih_bf16(w_ih, graph_params, H, Din)           # [8H, Din]
        else:
            x_op, w_op = x_src, w_ih
        y_bf = torch.empty(B, T, 2 * H, dtype=torch.bfloat16, device=dev) if cd == BF16 else None
        y = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev)
        cst = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev)
        nb = N.query('asr_lstm_workspace_bytes', B, H, cd, 0)
        zb = N.query('asr_lstm_ws_zero_bytes', B, H)
        ws, pz = _rec_workspace(nb, dev, _arena_take(nb, dev, zb))   # zeroed by rec_arena_begin
        # the backward's slot, reserved now so the arena's one fill covers it
        ctx.bws = (_arena_take(N.query('asr_lstm_workspace_bytes', B, H, cd, 2), dev, zb)
                   if pz else None)
        whh_r = w_hh.data_ptr() + 4 * H * H * 4
        # gx: f32 gate pre-activations -> activations [B, T, 8H], or packed fp16
        # activations [B, T, 2, H, 4] (fused bf16 path).  handoff: (bf16 tensor
        # the next layer stages from, its dropout)
        fuse_x, gx, handoff = False, None, None
        if cd == BF16 and _fuse_xproj_on():
            fuse_x, gx, handoff = _lstm_forward_fused(
                x_op, Dp, w_op, b_ih, b_hh, w_hh, lens, B, T, H, out_spec, y, cst, y_bf, ws, nb, pz)
        if not fuse_x:
            gx = torch.empty(B, T, 8 * H, dtype=torch.float32, device=dev)
            # (fp32: x_op is x_src read through the input map, w_op is w_ih, Dp = Din)
            x_map = rowmap(Dp) if cd == BF16 else a_map
            run_gemm([gemm_problem(operand(x_op, 0, x_map), operand(w_op, 0, rowmap(Dp)), gx,
                                   rowmap(8 * H), B * T, 8 * H, Dp, bias=b_ih, bias2=b_hh)], dev)
            N.call('asr_lstm_forward', N.ptr(gx), N.ptr(w_hh), ctypes.c_void_p(whh_r), F32,
                   N.ptr(lens), B, T, H, cd, N.ptr(y), N.ptr(cst), N.ptr(y_bf), N.ptr(ws), nb,
                   N.stream_handle(dev), _lstm_opts(pz))
        ctx.save_for_backward(x_op, w_op, lens, w_hh, b_ih, b_hh, gx, cst,
                              y_bf if y_bf is not None else y)
        ctx.meta = (in_map, gbufs, cd, B, Dp, w_ih)
        ctx.bh = (B, H)     # the recurrence shape a gated side stream waits on
        ctx.drop = drop
        ctx.next_rec = bool(next_rec)
        ctx.n_graph = len(graph_params)
        ctx.handoff_in = twin is not None
        if handoff is not None:
            # y was not written: only the next BLSTM layer may consume it, through
            # the bf16 tensor (_handoff_input raises for any other use it sees)
            y._asr_handoff = handoff
        return y

    @staticmethod
    def backward(ctx, dy):
        x_op, w_op, lens, w_hh, b_ih, b_hh, act, cst, y_op = ctx.saved_tensors
        in_map, gbufs, cd, B, Dp, w_ih = ctx.meta
        H = w_hh.shape[1]
        dev = act.device
        dy = dy.contiguous()
        # dy still being written by the layer above's input-gradient GEMMs
        # (_dx_pipelined): only the packed-activation tagged-granule backward
        # reads it that way; anything else waits for them first
        pipe = getattr(dy, '_asr_dy_pipe', None)
        if pipe is not None and act.dtype != torch.float16:
            torch.cuda.current_stream(dev).wait_event(pipe[3])
            pipe = None
        if gbufs is None:
            gbufs = tuple(grad_buffer(p) for p in (w_ih, w_hh, b_ih, b_hh))
        # data parallel: every collective issued so far completes before this
        # persistent recurrence starts (a kernel co-resident with the
        # recurrence perturbs it)
        notify_grad_event('pre_recurrence')
        plan = _blstm_bwd_plan(ctx, act, pipe, in_map, B, H, dev)
        dg_op, act, gate = _blstm_bwd_recurrence(ctx, plan, dy, pipe, w_hh, lens, act, cst, gbufs,
                                                 cd, B, in_map.T, H, dev)
        # the one progress report serves the banded dX, else the banded dW
        dx_gate, w_gate = (gate, None) if plan.bands is not None else (None, gate)
        # weight gradients of the layer above, if they went to a side stream: join
        # them here (they run beside the recurrence just enqueued) so the
        # gradient-ready bucket sees them on the compute stream
        _join_side_wgrads(dev)
        notify_grad_event('recurrence')
        # the bottom layer's weight gradients have no recurrence left to run
        # beside: they take the main stream and the full-size GEMM kernels (on
        # the co-resident small tiles the 4x320 layer-0 dW_ih ran at 29 TF/s)
        side_ent = None if plan.last_main else _wgrad_side_stream(dev, B, H)
        dx, pipe_done, bands_done = _blstm_bwd_dx_ahead(ctx, plan, dx_gate, dg_op, w_op, in_map,
                                                        B, H, Dp, dev)
        _blstm_bwd_wgrads(ctx, plan, w_gate, side_ent, pipe_done, dg_op, act, x_op, y_op, in_map,
                          Dp, cd, gbufs, B, H, dev)
        dx = _blstm_bwd_dx_rest(ctx, plan, dx, bands_done, dg_op, w_op, in_map, B, H, Dp, dev)
        return (dx,) + (None,) * (14 + ctx.n_graph)


def _dx_bands(T, two):
    """The split input gradient's row bands as ordered groups of (ta, tb) ranges
    of t, one run_gemm launch per group: by when their gate gradients are
    final, [T/4, 3T/4) at processing step 3T/4 - 1, with two chunks also
    [T/8, T/4) and [3T/4, 7T/8) at 7T/8 - 1; the rest, after the recurrence,
    last.  Every mode runs the groups in this order: dX by the same products."""
    t0 = te = T // 4
    groups = [[(t0, T - t0)]]
    if two:
        te = T // 8
        groups.append([(te, t0), (T - t0, T - te)])
    return groups + [[(0, te), (T - te, T)]]


class _ProgressReport:
    """The progress report of one packed-activation backward launch: at each of
    `steps` (one or two processing steps) the recurrence adds `arrivals` to the
    device counter, and a side stream gates (asr_lstm_progress_gate) on the
    counter reaching targets[k] before it reads what is final after steps[k].
    The counter only grows; the host's running total of it (_progress_counter)
    advances in commit() alone."""

    def __init__(self, dev, arrivals, steps):
        self.entry = _progress_counter(dev)
        self.counter, self.arrivals, self.steps = self.entry[0], int(arrivals), tuple(steps)
        self.targets = self.pre = None

    @classmethod
    def request(cls, dev, B, H, xu, steps):
        """For the next backward of [B, *, H] with xu units per work-group;
        None where it would not report."""
        arrivals = N.query('asr_lstm_bwd_progress_arrivals', B, H, xu)
        return cls(dev, arrivals, steps) if arrivals > 0 else None

    def arm(self, dev):
        """pre: all a gated consumer reads but the recurrence's writes is enqueued by now."""
        self.pre = torch.cuda.Event()
        self.pre.record(torch.cuda.current_stream(dev))

    def commit(self, done):
        """The gate targets of a launch that ran (done): each step's arrivals on
        top of the running total, which they advance.  Else None."""
        if done:
            self.targets = tuple(self.entry[1] + self.arrivals * k
                                 for k in range(1, len(self.steps) + 1))
            self.entry[1] = self.targets[-1]
        return self.targets


_BwdPlan = collections.namedtuple('_BwdPlan',
                                  'mode pin_kb xu last_main wgrad_banded bands dx report')


def _blstm_bwd_plan(ctx, act, pipe, in_map, B, H, dev):
    """What a BLSTM layer's backward runs, and its recurrence's launch settings
    (pin_kb, xu: the progress arrivals follow the units).  bands
    (_dx_bands) come with dx and, where the recurrence reports progress, the
    report gating them; None: dX pipelined or whole, decided after it."""
    T = in_map.T
    # the recurrence's LDS pin: co-resident GEMM work-groups only in the
    # opt-in mode 2 (84 KB); otherwise 140 KB excludes every GEMM kernel.
    # Units per work-group: 32 where that frees the CUs for mode 3.
    mode, xu = _overlap_plan(dev, B, H)
    pin_kb = 84 if mode == '2' else 0
    last_main = not ctx.next_rec and _wgrad_last_main_on()
    wgrad_banded = last_main and _wgrad_split_ok(ctx, T, mode)
    bands = dx = report = None
    if (act.dtype == torch.float16 and pipe is None and _dx_split_ok(ctx, B, T, dev, mode)
            and not _dx_pipeline_ok(ctx, B, T, in_map.Din, dev)):
        # beside the recurrence in mode 3; in the other modes the same bands after it
        bands = _dx_bands(T, _dx_split_chunks() == 2 and T >= 128)
        if mode == '3':
            report = _ProgressReport.request(dev, B, H, xu,
                                             [T - 1 - g[0][0] for g in bands[:-1]])
        # dX before the recurrence: its zero fill (non-identity maps) precedes
        # the side stream's writes
        dx = in_map.alloc_dx(B, dev)
    return _BwdPlan(mode, pin_kb, xu, last_main, wgrad_banded, bands, dx, report)


def _blstm_bwd_recurrence(ctx, plan, dy, pipe, w_hh, lens, act, cst, gbufs, cd, B, T, H, dev):
    """(dg_op, act, gate): the saved activations become the gate gradients dG
    in place (act: f32, unpacked if the packed-activation launch did not run);
    dg_op is dG as the GEMMs read it (bf16 mode: the bf16 copy); gate is the
    committed progress report or None."""
    fused_db = _bias_fused_on()
    whh_r = ctypes.c_void_p(w_hh.data_ptr() + 4 * H * H * 4)
    dg_bf = torch.empty(B, T, 8 * H, dtype=torch.bfloat16, device=dev) if cd == BF16 else None
    done, gate = False, None
    if act.dtype == torch.float16:
        # packed fp16 activations of asr_lstm_forward_xh: the tagged-granule
        # backward reads them directly; otherwise they are unpacked to f32
        done, gate = _blstm_bwd_packed(ctx, plan, dy, pipe, w_hh, whh_r, lens, act, cst, dg_bf,
                                       gbufs, cd, B, T, H, dev)
        if not done:
            a32 = torch.empty(B, T, 8 * H, dtype=torch.float32, device=dev)
            N.call('asr_lstm_unpack_act_h', N.ptr(act), B, T, H, N.ptr(a32),
                   N.stream_handle(dev))
            act = a32
    nb = N.query('asr_lstm_workspace_bytes', B, H, cd, 2 if fused_db else 1)
    ws = _ws(nb, dev)
    opts = _lstm_opts(False, bwd_pin_kb=plan.pin_kb, bwd_units=plan.xu)
    # the bias gradients (sum of dG over b, t) are accumulated by the same call
    if not done and fused_db:
        # bf16 mode: only the bf16 dG feeds the GEMMs, so the f32 dG is not stored
        fn = 'asr_lstm_backward_dgbf' if dg_bf is not None else 'asr_lstm_backward_db'
        N.call(fn, N.ptr(dy), N.ptr(w_hh), whh_r, F32, N.ptr(lens), B, T, H, cd, N.ptr(act),
               N.ptr(cst), N.ptr(dg_bf), N.ptr(gbufs[2]), N.ptr(gbufs[3]), N.ptr(ws), nb,
               N.stream_handle(dev), opts)
    elif not done:   # A/B: separate column-sum pass over dG
        N.call('asr_lstm_backward', N.ptr(dy), N.ptr(w_hh), whh_r, F32, N.ptr(lens), B, T, H,
               cd, N.ptr(act), N.ptr(cst), N.ptr(dg_bf), N.ptr(ws), nb, N.stream_handle(dev),
               opts)
        colsum_accumulate(act.view(B * T, 8 * H), gbufs[2], gbufs[3])
    return (dg_bf if dg_bf is not None else act), act, gate


def _blstm_bwd_packed(ctx, plan, dy, pipe, w_hh, whh_r, lens, act, cst, dg_bf, gbufs, cd, B, T, H,
                      dev):
    """The packed-activation tagged-granule backward, given the plan's
    progress report (with none, banded weight gradients in mode 3 ask for one
    at their middle band's step) and the dy flags of a pipelined layer above.
    (ran, committed report or None); not ran: ASR_ERR_UNSUPPORTED, no report --
    its consumers run the same bands after the recurrence."""
    nb = N.query('asr_lstm_workspace_bytes', B, H, cd, 2)
    res, ctx.bws = ctx.bws, None      # a reserved slot serves one backward
    ws, pz = _rec_workspace(nb, dev, res)
    settings = dict(bwd_pin_kb=plan.pin_kb, bwd_units=plan.xu)
    if pipe is not None:
        settings.update(dy_flags=pipe[0].data_ptr(), dy_c0=pipe[1], dy_epoch=pipe[2])
    report = plan.report
    if report is None and plan.wgrad_banded and plan.mode == '3':
        report = _ProgressReport.request(dev, B, H, plan.xu, [T - 1 - T // 4])
    if report is not None:
        report.arm(dev)
        q1, q2 = (report.steps + (-1,))[:2]
        settings.update(progress=report.counter.data_ptr(), progress_q1=q1, progress_q2=q2)
    try:
        rc = N.query('asr_lstm_backward_dgbf_h', N.ptr(dy), N.ptr(w_hh), whh_r, F32,
                     N.ptr(lens), B, T, H, cd, N.ptr(act), N.ptr(cst), N.ptr(dg_bf),
                     N.ptr(gbufs[2]), N.ptr(gbufs[3]), N.ptr(ws), nb, N.stream_handle(dev),
                     _lstm_opts(pz, **settings))
    finally:
        if pipe is not None:
            # (after the launch: later compute-stream work sees all of dy)
            torch.cuda.current_stream(dev).wait_event(pipe[3])
    if rc not in (0, N.ASR_ERR_UNSUPPORTED):
        raise N.NativeError('asr_lstm_backward_dgbf_h failed (rc=%d): %s' % (
            rc, N.lib().asr_last_error().decode(errors='replace')))
    committed = report is not None and report.commit(rc == 0) is not None
    return rc == 0, report if committed else None


def _blstm_bwd_wgrads(ctx, plan, gate, side_ent, dx_done, dg_op, act, x_op, y_op, in_map, Dp, cd,
                      gbufs, B, H, dev):
    """The weight gradients where the plan and side_ent (_wgrad_side_stream's
    entry or None) place them: the compute stream, whole or in time bands, or
    a side stream (behind the pipelined dX's event dx_done, if any)."""
    T = in_map.T
    # X as the dW_ih operand: the bf16 copy is already gathered (identity map)
    x_map = rowmap(Dp) if cd == BF16 else in_map.rows()
    if side_ent is None:
        if plan.wgrad_banded:
            _wgrad_main_banded(gate, dg_op, x_op, y_op, T, gbufs, B, H, dev)
        else:
            _blstm_wgrad(dg_op, act, x_op, x_map, y_op, T, gbufs, dev)
        notify_grad_event('grads', gbufs)      # final on the compute stream
        return
    # weight gradients on a side stream, overlapping this layer's dX
    # GEMM and the previous layer's backward recurrence; joined back
    # into the main stream at the end of the backward pass
    side, small, gated = side_ent
    main = torch.cuda.current_stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        if dx_done is not None:
            # the pipelined input gradient first, so the CUs the next
            # recurrence leaves free serve dX -- which that recurrence waits
            # for -- before the weight gradients, which only the optimizer needs
            side.wait_event(dx_done)
        elif gated and ctx.next_rec:
            # hold the GEMMs back until the previous layer's backward
            # recurrence (launched next on the main stream) is resident
            N.call('asr_lstm_wgrad_gate', N.stream_handle(dev))
        # (tools/cores_locate.py replaces _blstm_wgrad with stand-in
        # side-stream workloads taking the same positional arguments;
        # nothing diagnostic runs here)
        _blstm_wgrad(dg_op, act, x_op, x_map, y_op, T, gbufs, dev, SMALL_TILES if small else None)
    _defer_side_join(dev, side, main, (dg_op, act, x_op, y_op) +
                     ((in_map.perm,) if in_map.perm is not None else ()), gbufs)


def _wgrad_main_banded(gate, dg_op, x_op, y_op, T, gbufs, B, H, dev):
    """Time bands: the middle one first (with gate, the recurrence's progress
    report: beside its last quarter, on the side stream), then the outer two."""
    tq = T // 4
    Dx = x_op.shape[-1]
    if gate is not None:
        side = _wgrad_side_stream(dev, B, H)[0]
        side.wait_event(gate.pre)
        with torch.cuda.stream(side):
            N.call('asr_lstm_progress_gate', N.ptr(gate.counter), gate.targets[0],
                   N.stream_handle(dev))
            _blstm_wgrad_rows(dg_op, x_op, Dx, y_op, T, gbufs, dev, tq, T - tq)
            mid_done = torch.cuda.Event()
            mid_done.record(side)
        for tt in (dg_op, x_op, y_op, gate.counter):
            tt.record_stream(side)
        torch.cuda.current_stream(dev).wait_event(mid_done)
    else:
        _blstm_wgrad_rows(dg_op, x_op, Dx, y_op, T, gbufs, dev, tq, T - tq)
    _blstm_wgrad_rows(dg_op, x_op, Dx, y_op, T, gbufs, dev, 0, tq)
    _blstm_wgrad_rows(dg_op, x_op, Dx, y_op, T, gbufs, dev, T - tq, T)


def _blstm_bwd_dx_ahead(ctx, plan, gate, dg_op, w_op, in_map, B, H, Dp, dev):
    """The input gradient enqueued before the weight gradients: (dx, the
    pipelined form's event, the gated bands' event), None where not that form."""
    if plan.bands is not None and gate is not None:
        # all band groups but the last on the weight-gradient side stream
        side = _wgrad_side_stream(dev, B, H)[0]
        side.wait_event(gate.pre)     # not the recurrence itself: the gate waits on its progress
        if _dx_split_sync_on():       # diagnostics: after the whole recurrence
            rec_done = torch.cuda.Event()
            rec_done.record(torch.cuda.current_stream(dev))
            side.wait_event(rec_done)
        with torch.cuda.stream(side):
            _dx_run_bands(plan.bands[:-1], dg_op, w_op, plan.dx, in_map, H, Dp, ctx.drop, dev, gate)
            done = torch.cuda.Event()
            done.record(side)
        perm = in_map.perm
        for tt in (dg_op, w_op, plan.dx, gate.counter) + ((perm,) if perm is not None else ()):
            tt.record_stream(side)
        return plan.dx, None, done
    # pipelined input gradient (_dx_pipelined): enqueued first, and the
    # side-stream weight gradients start after it
    if (plan.bands is None and ctx.needs_input_grad[0]
            and _dx_pipeline_ok(ctx, B, in_map.T, in_map.Din, dev)):
        dx = in_map.alloc_dx(B, dev)     # (a handed-over input: the identity map)
        return dx, _dx_pipelined(dx, dg_op, w_op, B, in_map.T, H, in_map.Din, Dp, ctx.drop,
                                 dev), None
    return plan.dx, None, None


def _dx_run_bands(groups, dg_op, w_op, dx, in_map, H, Dp, drop, dev, gate=None):
    """One launch per band group, in order, on the current stream; gate: each
    first waits for the recurrence's progress to reach its target."""
    for k, group in enumerate(groups):
        if gate is not None:
            N.call('asr_lstm_progress_gate', N.ptr(gate.counter), gate.targets[k],
                   N.stream_handle(dev))
        run_gemm([_dx_rows_problem(dg_op, w_op, dx, in_map, H, Dp, drop, ta, tb)
                  for ta, tb in group], dev, opts=NOSPLIT)   # per output element: one launch's sum


def _blstm_bwd_dx_rest(ctx, plan, dx, bands_done, dg_op, w_op, in_map, B, H, Dp, dev):
    """The input gradient enqueued after the weight gradients; returns dX."""
    if plan.bands is not None and bands_done is not None:
        # the outer rows on the compute stream, then the side stream's rows joined
        _dx_run_bands(plan.bands[-1:], dg_op, w_op, dx, in_map, H, Dp, ctx.drop, dev)
        torch.cuda.current_stream(dev).wait_event(bands_done)
    elif plan.bands is not None:
        # the split's row bands in its order, on the compute stream
        _dx_run_bands(plan.bands, dg_op, w_op, dx, in_map, H, Dp, ctx.drop, dev)
    elif dx is None and ctx.needs_input_grad[0]:
        # dX [BT, Din] = dG [BT, 8H] W_ih [8H, Din], scattered back through the
        # input map; dropout's backward (the forward mask over x_src's flat
        # offsets) is applied by the GEMM's epilogue as it writes dX
        dx = in_map.alloc_dx(B, dev)
        run_gemm([gemm_problem(operand(dg_op, 0, rowmap(8 * H)), operand(w_op, 1, rowmap(Dp)), dx,
                               in_map.rows(), B * in_map.T, in_map.Din, 8 * H, drop=ctx.drop)], dev)
    return dx


def _dx_rows_problem(dg_op, w_op, dx, in_map, H, Dp, drop, ta, tb):
    """dX rows (b, t) for t in [ta, tb) of every utterance: dG [B, T, 8H] W_ih
    [8H, Din], written through the layer's input map (the dropout mask by dX's
    element offsets, as the whole-product form)."""
    n = tb - ta
    a_map = rowmap(8 * H, stride_b=in_map.T * 8 * H, rows_per_b=n, t_add=ta)
    return gemm_problem(operand(dg_op, 0, a_map), operand(w_op, 1, rowmap(Dp)), dx,
                        in_map.rows(ta, tb), dg_op.shape[0] * n, in_map.Din, 8 * H, drop=drop)


def _lstm_forward_fused(x_op, Dp, w_op, b_ih, b_hh, w_hh, lens, B, T, H, out_spec, y, cst, y_bf,
                        ws, nb, pz):
    """The input projection inside the persistent forward recurrence (no gx
    GEMM): (ran, gx, handoff); not ran (ASR_ERR_UNSUPPORTED): this shape /
    configuration does not take it.  gx: the gate activations as packed fp16
    (8 B per cell instead of 16; ASR_XG_ACT_H=0 keeps the f32 layout).  With
    out_spec's y_f32 off, the next BLSTM layer stages its input from bf16
    written here, its dropout applied (handoff): no f32 y, no conversion pass."""
    dev = x_op.device
    y_f32, out_drop = out_spec
    packed = _act_h_on()
    gx = (torch.empty(B, T, 2, H, 4, dtype=torch.float16, device=dev) if packed
          else torch.empty(B, T, 8 * H, dtype=torch.float32, device=dev))
    args = (N.ptr(x_op), Dp, N.ptr(w_op), N.ptr(b_ih), N.ptr(b_hh), N.ptr(w_hh),
            ctypes.c_void_p(w_hh.data_ptr() + 4 * H * H * 4), N.ptr(lens), B, T, H, N.ptr(gx))
    handoff = None
    tail = (N.ptr(ws), nb, N.stream_handle(dev), _lstm_opts(pz))
    if packed and not y_f32:
        fn = 'asr_lstm_forward_xh_drop'
        y_d = (torch.empty(B, T, 2 * H, dtype=torch.bfloat16, device=dev)
               if out_drop is not None else None)
        p, seed = out_drop if out_drop is not None else (0.0, 0)
        rc = N.query(fn, *args, None, N.ptr(cst), N.ptr(y_bf), N.ptr(y_d), ctypes.c_float(p),
                     ctypes.c_ulonglong(seed), *tail)
        if rc == 0:
            handoff = (y_d if y_d is not None else y_bf, out_drop)
    else:
        fn = 'asr_lstm_forward_xh' if packed else 'asr_lstm_forward_x'
        rc = N.query(fn, *args, N.ptr(y), N.ptr(cst), N.ptr(y_bf), *tail)
    if rc not in (0, N.ASR_ERR_UNSUPPORTED):
        raise N.NativeError('%s failed (rc=%d): %s' % (
            fn, rc, N.lib().asr_last_error().decode(errors='replace')))
    return rc == 0, gx, handoff


class BGRULayerFn(torch.autograd.Function):
    """Bidirectional GRU layer (nn.GRU, rnn.py:173-191 / :226-233) on the HIP
    recurrence of csrc/gru.hip.  Same input addressing as BLSTMLayerFn (row map
    with perm / subsampling / 'concat' rows read in place); parameters are the
    combined [fwd; rev] views (w_ih [6H, Din], w_hh [6H, H], b_ih, b_hh [6H]).
    The recurrence runs in f32 in both modes; the GEMMs take the library's
    bf16 operand staging in bf16 mode."""

    @staticmethod
    def forward(ctx, x_src, lens, T, perm, t_mul, t_add, gbufs, concat, w_ih, w_hh, b_ih, b_hh,
                *graph_params):
        N.require_device(x_src, lens, w_ih, w_hh, b_ih, b_hh)
        x_src = x_src.contiguous()
        B, T_src, Dsrc = x_src.shape
        Din = 2 * Dsrc if concat else Dsrc
        assert w_ih.shape[1] == Din, (tuple(w_ih.shape), Din)
        H = w_hh.shape[1]
        dev = x_src.device
        in_map = _InputMap(perm, t_mul, t_add, T, T_src, Dsrc, Din)
        gx = torch.empty(B, T, 6 * H, dtype=torch.float32, device=dev)
        run_gemm([gemm_problem(operand(x_src, 0, in_map.rows()), operand(w_ih, 0, rowmap(Din)), gx,
                               rowmap(6 * H), B * T, 6 * H, Din, bias=b_ih)], dev)
        y = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev)
        ghn = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev)
        N.call('asr_gru_forward', N.ptr(gx), N.ptr(w_hh), N.ptr(b_hh), N.ptr(lens), B, T, H,
               N.ptr(y), N.ptr(ghn), N.stream_handle(dev))
        ctx.save_for_backward(x_src, w_ih, w_hh, b_ih, b_hh, lens, gx, ghn, y)
        ctx.meta = (in_map, gbufs)
        ctx.n_graph = len(graph_params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x_src, w_ih, w_hh, b_ih, b_hh, lens, act, ghn, y = ctx.saved_tensors
        in_map, gbufs = ctx.meta
        B, T, Din = x_src.shape[0], in_map.T, in_map.Din
        H = w_hh.shape[1]
        dev = act.device
        dy = dy.contiguous()
        if gbufs is None:
            gbufs = tuple(grad_buffer(p) for p in (w_ih, w_hh, b_ih, b_hh))
        g_ih, g_hh, g_bih, g_bhh = gbufs
        nb = N.query('asr_gru_workspace_bytes', B, H)
        ws = _ws(nb, dev)
        dgh = torch.empty(B, T, 6 * H, dtype=torch.float32, device=dev)
        # the saved activations become dgx in place
        N.call('asr_gru_backward', N.ptr(dy), N.ptr(w_hh), N.ptr(lens), B, T, H, N.ptr(act),
               N.ptr(ghn), N.ptr(y), N.ptr(dgh), N.ptr(ws), nb, N.stream_handle(dev))
        BT = B * T
        # dW_ih [6H, Din] += dgx^T x (both directions in one problem)
        run_gemm([gemm_problem(operand(act, 1, rowmap(6 * H)), operand(x_src, 1, in_map.rows()),
                               g_ih, rowmap(Din), 6 * H, Din, BT, beta=1.0)], dev)
        # dW_hh[dir] += dgh_dir^T h_prev_dir ; h_prev = y[b, t-1, :H] (fwd), y[b, t+1, H:] (rev)
        hp_f = rowmap(2 * H, stride_b=T * 2 * H, rows_per_b=T, t_add=-1, t_limit=T)
        hp_r = rowmap(2 * H, stride_b=T * 2 * H, rows_per_b=T, t_add=1, t_limit=T)
        run_gemm([
            gemm_problem(operand(dgh, 1, rowmap(6 * H)), operand(y, 1, hp_f), g_hh, rowmap(H),
                         3 * H, H, BT, beta=1.0),
            gemm_problem(operand(dgh, 1, rowmap(6 * H), offset=3 * H),
                         operand(y, 1, hp_r, offset=H), g_hh, rowmap(H), 3 * H, H, BT, beta=1.0,
                         c_offset=3 * H * H),
        ], dev)
        colsum_accumulate(act.view(BT, 6 * H), g_bih)
        colsum_accumulate(dgh.view(BT, 6 * H), g_bhh)
        notify_grad_event('recurrence')
        notify_grad_event('grads', gbufs)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = in_map.alloc_dx(B, dev)
            run_gemm([gemm_problem(operand(act, 0, rowmap(6 * H)), operand(w_ih, 1, rowmap(Din)),
                                   dx, in_map.rows(), BT, Din, 6 * H)], dev)
        return (dx,) + (None,) * (11 + ctx.n_graph)


def bgru_layer(x_src, lens, T, w_ih, w_hh, b_ih, b_hh, perm=None, t_mul=1, t_add=0, gbufs=None,
               graph_params=(), concat=False):
    """The bidirectional GRU counterpart of blstm_layer (same addressing)."""
    return BGRULayerFn.apply(x_src, lens, T, perm, t_mul, t_add, gbufs, bool(concat),
                             w_ih, w_hh, b_ih, b_hh, *graph_params)


def _lstm_uni_gx(x_src, T, perm, t_mul, t_add, concat, w_ih, w_hh, b_ih, b_hh):
    """A unidirectional LSTM layer's input side, for training and streaming
    alike: (the row map of its T input frames into x_src [B, T_src, Dsrc], gx
    [B, T, 4H] = x W_ih^T + b_ih + b_hh from one GEMM)."""
    B, T_src, Dsrc = x_src.shape
    Din = 2 * Dsrc if concat else Dsrc
    assert w_ih.shape[1] == Din, (tuple(w_ih.shape), Din)
    H = w_hh.shape[1]
    in_map = _InputMap(perm, t_mul, t_add, T, T_src, Dsrc, Din)
    gx = torch.empty(B, T, 4 * H, dtype=torch.float32, device=x_src.device)
    run_gemm([gemm_problem(operand(x_src, 0, in_map.rows()), operand(w_ih, 0, rowmap(Din)), gx,
                           rowmap(4 * H), B * T, 4 * H, Din, bias=b_ih, bias2=b_hh)], x_src.device)
    return in_map, gx


class LSTMLayerFn(torch.autograd.Function):
    """Unidirectional LSTM layer (nn.LSTM(bidirectional=False), rnn.py:166-172 /
    :218-224) on the per-step recurrence of csrc/lstm_uni.hip.  Same input
    addressing as BLSTMLayerFn (row map with perm / subsampling / 'concat' rows
    read in place, drop = (p, seed) on x_src); parameters are one direction's
    tensors (w_ih [4H, Din], w_hh [4H, H], b_ih, b_hh [4H]).  The recurrence
    runs in the session's compute dtype; the layer GEMMs read the f32 tensors
    and, in bf16 mode, round them to bf16 in their loads."""

    @staticmethod
    def forward(ctx, x_src, lens, T, perm, t_mul, t_add, gbufs, concat, drop, w_ih, w_hh, b_ih,
                b_hh, *graph_params):
        N.require_device(x_src, lens, w_ih, w_hh, b_ih, b_hh)
        x_src = x_src.contiguous()
        dev = x_src.device
        if drop is not None:   # the layer reads dropout(x_src)
            xd = torch.empty_like(x_src)
            N.call('asr_dropout', N.ptr(x_src), N.ptr(xd), x_src.numel(), float(drop[0]),
                   int(drop[1]), N.stream_handle(dev))
            x_src = xd
        B, H = x_src.shape[0], w_hh.shape[1]
        cd = compute_dtype()
        nb = int(N.query('asr_lstm_uni_workspace_bytes', B, H, cd, 0))
        ws = _ws(nb, dev)
        in_map, gx = _lstm_uni_gx(x_src, T, perm, t_mul, t_add, concat, w_ih, w_hh, b_ih, b_hh)
        y = torch.empty(B, T, H, dtype=torch.float32, device=dev)
        cst = torch.empty(B, T, H, dtype=torch.float32, device=dev)
        N.call('asr_lstm_uni_forward', N.ptr(gx), N.ptr(w_hh), F32, N.ptr(lens), B, T, H, cd,
               N.ptr(y), N.ptr(cst), None, N.ptr(ws), nb, N.stream_handle(dev))
        ctx.save_for_backward(x_src, w_ih, w_hh, b_ih, b_hh, lens, gx, cst, y)
        ctx.meta = (in_map, gbufs, cd, drop)
        ctx.n_graph = len(graph_params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x_src, w_ih, w_hh, b_ih, b_hh, lens, act, cst, y = ctx.saved_tensors
        in_map, gbufs, cd, drop = ctx.meta
        B, T, Din = x_src.shape[0], in_map.T, in_map.Din
        H = w_hh.shape[1]
        dev = act.device
        dy = dy.contiguous()
        if gbufs is None:
            gbufs = tuple(grad_buffer(p) for p in (w_ih, w_hh, b_ih, b_hh))
        g_ih, g_hh, g_bih, g_bhh = gbufs
        nb = int(N.query('asr_lstm_uni_workspace_bytes', B, H, cd, 1))
        ws = _ws(nb, dev)
        # the saved activations become the gate gradients dG in place; the bias
        # gradients are its column sums (fixed order)
        N.call('asr_lstm_uni_backward', N.ptr(dy), N.ptr(w_hh), F32, N.ptr(lens), B, T, H, cd,
               N.ptr(act), N.ptr(cst), None, N.ptr(g_bih), N.ptr(g_bhh), N.ptr(ws), nb,
               N.stream_handle(dev))
        notify_grad_event('recurrence')
        BT = B * T
        # dW_ih [4H, Din] += dG^T x ; dW_hh [4H, H] += dG^T h_prev, h_prev = y[b, t-1]
        hp = rowmap(H, stride_b=T * H, rows_per_b=T, t_add=-1, t_limit=T)
        run_gemm([gemm_problem(operand(act, 1, rowmap(4 * H)), operand(x_src, 1, in_map.rows()),
                               g_ih, rowmap(Din), 4 * H, Din, BT, beta=1.0)], dev)
        run_gemm([gemm_problem(operand(act, 1, rowmap(4 * H)), operand(y, 1, hp), g_hh, rowmap(H),
                               4 * H, H, BT, beta=1.0)], dev)
        notify_grad_event('grads', gbufs)
        dx = None
        if ctx.needs_input_grad[0]:
            # scattered back through the input map; dropout's backward (the
            # forward mask over x_src's flat offsets) in the GEMM's epilogue
            dx = in_map.alloc_dx(B, dev)
            run_gemm([gemm_problem(operand(act, 0, rowmap(4 * H)), operand(w_ih, 1, rowmap(Din)),
                                   dx, in_map.rows(), BT, Din, 4 * H, drop=drop)], dev)
        return (dx,) + (None,) * (12 + ctx.n_graph)


def lstm_layer(x_src, lens, T, w_ih, w_hh, b_ih, b_hh, perm=None, t_mul=1, t_add=0, gbufs=None,
               graph_params=(), concat=False, drop=None):
    """The unidirectional counterpart of blstm_layer (same addressing, same
    drop / gbufs / graph_params contract); output [B, T, H].  A shape the
    recurrence does not take (asr_hip.h) raises NativeError before any launch."""
    B, H = x_src.shape[0], w_hh.shape[1]
    if N.query('asr_lstm_uni_shape_ok', int(B), int(T), int(H)) != 1:
        raise N.NativeError('asr_lstm_uni_forward refused (rc=%d): B %d T %d H %d is outside the '
                            'shapes the unidirectional recurrence accepts'
                            % (N.ASR_ERR_UNSUPPORTED, B, T, H))
    return LSTMLayerFn.apply(x_src, lens, T, perm, t_mul, t_add, gbufs, bool(concat), drop,
                             w_ih, w_hh, b_ih, b_hh, *graph_params)


@torch.no_grad()
def lstm_stream_layer(x, lens, Tc, w_ih, w_hh, b_ih, b_hh, state, t_mul=1, t_add=0, concat=False):
    """One chunk of a unidirectional LSTM layer with carried state (inference;
    csrc/lstm_stream.hip).  x [B, T_src, Dsrc] f32: row (b, t), t < Tc, of the
    layer input is x[b, t * t_mul + t_add] (concat: followed by the next frame),
    LSTMLayerFn.forward's input-projection GEMM and row map without a perm.
    lens int32 [B] on the device: valid frames of each row in this chunk (0 ..
    Tc).  state = (h, c), [B, H] f32, the state before the chunk; w_hh f32, or
    in bf16 mode a bf16 copy made once by the caller.  Returns (y [B, Tc, H],
    (h, c) after each row's last valid frame): y is 0 and the state frozen for
    t >= lens[b], so feeding an utterance in chunks gives what feeding it
    whole gives.  The returned state never shares memory with `state`."""
    h_in, c_in = (s.contiguous() for s in state)
    N.require_device(x, lens, w_ih, w_hh, b_ih, b_hh, h_in, c_in)
    x = x.contiguous()
    dev = x.device
    B, H, Tc = x.shape[0], w_hh.shape[1], int(Tc)
    assert tuple(h_in.shape) == tuple(c_in.shape) == (B, H) and lens.dtype == torch.int32
    cd = compute_dtype()
    if N.query('asr_lstm_uni_shape_ok', int(B), Tc, int(H)) != 1:
        raise N.NativeError('asr_lstm_stream_forward refused (rc=%d): B %d Tc %d H %d is outside '
                            'the shapes the unidirectional recurrence accepts'
                            % (N.ASR_ERR_UNSUPPORTED, B, Tc, H))
    w_dt = BF16 if w_hh.dtype == torch.bfloat16 else F32
    nb, ws = 0, None
    if cd == BF16 and w_dt == F32:
        nb = int(N.query('asr_lstm_stream_workspace_bytes', B, H, cd))
        ws = _ws(nb, dev)
    _, gx = _lstm_uni_gx(x, Tc, None, t_mul, t_add, concat, w_ih, w_hh, b_ih, b_hh)
    y = torch.empty(B, Tc, H, dtype=torch.float32, device=dev)
    h_out, c_out = torch.empty_like(h_in), torch.empty_like(c_in)
    N.call('asr_lstm_stream_forward', N.ptr(gx), N.ptr(w_hh), w_dt, N.ptr(lens), B, Tc, H, cd,
           N.ptr(h_in), N.ptr(c_in), N.ptr(h_out), N.ptr(c_out),
           N.ptr(y), N.ptr(ws), nb, N.stream_handle(dev))
    return y, (h_out, c_out)


def _act_h_on():
    """Fused bf16 forward: keep the gate activations as packed fp16
    (asr_lstm_forward_xh; ASR_XG_ACT_H=0 keeps f32)."""
    return os.environ.get('ASR_XG_ACT_H', '1') != '0'


def _fuse_xproj_on():
    """bf16 mode: try the layer's input projection inside the persistent
    forward recurrence (asr_lstm_forward_x) first (ASR_FUSE_XPROJ=0 keeps the
    separate GEMM)."""
    return os.environ.get('ASR_FUSE_XPROJ', '1') != '0'


def _bias_fused_on():
    """The backward recurrence sums the bias gradients too (ASR_BIAS_FUSED=0: a separate pass)."""
    return os.environ.get('ASR_BIAS_FUSED', '1') != '0'


def _wgrad_last_main_on():
    """The bottom layer's weight gradients on the compute stream (ASR_WGRAD_LAST_MAIN=0: A/B)."""
    return os.environ.get('ASR_WGRAD_LAST_MAIN', '1') != '0'


def _dx_split_sync_on():
    """Diagnostics (ASR_DX_SPLIT_SYNC=1): the gated dX bands also wait for the whole recurrence."""
    return os.environ.get('ASR_DX_SPLIT_SYNC') == '1'


def convert_rows_bf16(src, rmap, nrows, ncols, drop=None):
    """Dense bf16 [nrows, ncols] copy of the rows of `src` selected by a row map;
    drop=(p, seed): of dropout(src) with asr_dropout's mask, in the same pass."""
    out = torch.empty(nrows, ncols, dtype=torch.bfloat16, device=src.device)
    if drop is not None:
        N.call('asr_convert_rows_bf16_dropout', N.ptr(src), rmap, int(nrows), int(ncols),
               N.ptr(out), float(drop[0]), int(drop[1]), N.stream_handle(src.device))
    else:
        N.call('asr_convert_rows_bf16', N.ptr(src), rmap, int(nrows), int(ncols), N.ptr(out),
               N.stream_handle(src.device))
    return out


def fuse_dropout_ok():
    """Inter-layer dropout is folded into the next BLSTM layer's bf16 input
    staging (bf16 mode; ASR_FUSE_DROPOUT=0 keeps the separate pass)."""
    return compute_dtype() == BF16 and os.environ.get('ASR_FUSE_DROPOUT', '1') != '0'


def _blstm_wgrad(dg, dg_f32, x_op, x_map, y_op, T, gbufs, dev, gemm_opts=None):
    """dW_ih, dW_hh of one BLSTM layer from its gate gradients (dg: bf16 copy
    in bf16 mode, else the f32 tensor).  db_ih / db_hh were accumulated by
    asr_lstm_backward_db.  gemm_opts: run_gemm's opts for both launches."""
    H = y_op.shape[2] // 2
    hp = lambda add: rowmap(2 * H, stride_b=T * 2 * H, rows_per_b=T, t_add=add,  # noqa: E731
                            t_limit=T)
    _wgrad_gemms(dg, x_op, y_op, gbufs, dev, dg.shape[0] * T, rowmap(8 * H), x_map, hp(-1), hp(1),
                 gemm_opts)


def _blstm_wgrad_rows(dg, x_op, Dx, y_op, T, gbufs, dev, ta, tb):
    """_blstm_wgrad over the rows (b, t), t in [ta, tb), of every utterance
    (bf16 mode: dg and x_op dense [B*T, width] rows): the weight gradients
    accumulated (beta = 1) from that band of time steps only."""
    H = y_op.shape[2] // 2
    n = tb - ta
    if n <= 0:
        return
    band = lambda ld, add=0: rowmap(ld, stride_b=T * ld, rows_per_b=n, t_add=ta + add,  # noqa: E731
                                    t_limit=T)
    _wgrad_gemms(dg, x_op, y_op, gbufs, dev, dg.shape[0] * n, band(8 * H), band(Dx),
                 band(2 * H, -1), band(2 * H, 1))


def _wgrad_gemms(dg, x_op, y_op, gbufs, dev, rows, dg_map, x_map, hp_f, hp_r, gemm_opts=None):
    """The two weight-gradient launches over `rows` rows addressed by the maps."""
    H = y_op.shape[2] // 2
    g_ih, g_hh = gbufs[:2]
    Din = g_ih.shape[-1]          # != x_op's width for 'concat' input rows
    # dW_ih [8H, Din] += dG^T x   (both directions in one problem)
    run_gemm([gemm_problem(operand(dg, 1, dg_map), operand(x_op, 1, x_map), g_ih, rowmap(Din),
                           8 * H, Din, rows, beta=1.0)], dev, opts=gemm_opts)
    # dW_hh[dir] += dG_dir^T h_prev_dir ; h_prev = y[b, t-1, :H] (fwd), y[b, t+1, H:] (rev)
    run_gemm([
        gemm_problem(operand(dg, 1, dg_map), operand(y_op, 1, hp_f), g_hh, rowmap(H), 4 * H, H,
                     rows, beta=1.0),
        gemm_problem(operand(dg, 1, dg_map, offset=4 * H), operand(y_op, 1, hp_r, offset=H), g_hh,
                     rowmap(H), 4 * H, H, rows, beta=1.0, c_offset=4 * H * H),
    ], dev, opts=gemm_opts)


def _wgrad_split_ok(ctx, T, mode):
    """The bottom BLSTM layer's weight gradients in three time bands (round 6,
    opt-in ASR_WGRAD_SPLIT=1; measured slower at ctc5x512, 17.48 vs 17.42
    ms/step: the band beside the recurrence costs it more than the 120 us it
    takes off the tail): the middle band [T/4, 3T/4) on the side
    stream beside the last quarter of the layer's own backward recurrence
    (gated on its progress report, mode 3), then [0, T/4) and [3T/4, T) on
    the compute stream -- in that order in every mode, so the sums are the
    same arithmetic with or without the overlap.  bf16 mode (dense staged
    operands), a layer with no recurrence left below it."""
    return (os.environ.get('ASR_WGRAD_SPLIT', '0') == '1' and not ctx.next_rec and T >= 64
            and compute_dtype() == BF16)


_side_streams = {}
_side_pending = []     # (side stream, gbufs, compute stream) of weight gradients not joined yet


def _defer_side_join(dev, side, main, keep, gbufs):
    """After weight-gradient work enqueued on `side`: the tensors of keep stay
    allocated until it has run, and the compute stream `main` joins it
    (_join_side_wgrads) at the end of the backward pass."""
    for t in keep:
        t.record_stream(side)
    if not _side_pending:
        torch.autograd.Variable._execution_engine.queue_callback(
            lambda: _join_side_wgrads(dev, notify=False))
    _side_pending.append((side, gbufs, main))


def _join_side_wgrads(dev, notify=True):
    """Make the compute stream wait for the side-stream weight gradients
    enqueued so far; notify 'grads' for each (gradient-ready buckets)."""
    if not _side_pending:
        return
    for side, gbufs, main in _side_pending:
        main.wait_stream(side)
        if notify:
            notify_grad_event('grads', gbufs)
    del _side_pending[:]


def discard_side_wgrads():
    """After a backward that raised: make each compute stream wait for the
    side-stream weight gradients still pending (so a later zero of the flat
    gradient cannot race a beta = 1 accumulation) and forget them WITHOUT
    notifying 'grads' (their values belong to the skipped batch; a bucket
    hook must not see them as ready).  The end-of-backward join callback of
    a failed backward never runs, so nothing else would clear them."""
    for side, _gbufs, main in _side_pending:
        main.wait_stream(side)
    del _side_pending[:]


def _num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _xg_grid(B, H, ncu, xu=16):
    """Work-groups of the persistent recurrence (lstm_xg.hip xg_rows): groups of
    R = 8 utterances (16 when 8 would not fit) x direction x H / xu slices --
    the backward's xu = 32 (asr_lstm_backward_grid) only with R = 8, H <= 512."""
    if H % 32 or H // 16 > 64 or os.environ.get('ASR_LSTM_XG', '1') == '0':
        return 1 << 30        # not the tagged-granule recurrence
    for R in (8, 16):
        g = 2 * ((B + R - 1) // R) * (H // 16)
        if g <= ncu:
            if xu == 32:
                return g // 2 if R == 8 and H <= 512 else 1 << 30
            return g
    return 1 << 30


def _overlap_plan(dev, B, H):
    """(mode, units): the resolved ASR_OVERLAP_WGRAD mode for a BLSTM layer's
    backward and the hidden units per work-group of its backward recurrence.
    Modes:
      '0'  weight gradients on the compute stream;
      '1'  a CU-masked side stream (upper half of the CUs), only when the
           persistent backward recurrence fits in the other half;
      '2'  (opt-in) a plain side stream whose GEMMs use the 128 x 128 kernel
           (64 KB of LDS) while the recurrence pins 84 KB, so GEMM work-groups
           are co-resident with the recurrence's on every CU (rounds 3-4: wrong
           values, a gfx950 packed-FP32 hazard the library no longer contains,
           DESIGN.md §5; bitwise mode 0 since, tests/test_coresidency_gpu.py);
      '3'  a plain side stream with the recurrence at its default 140 KB pin,
           so no GEMM work-group can share a CU with it: the weight-gradient
           GEMMs run on the CUs the recurrence leaves free.
    auto = '3' when the recurrence leaves at least 32 CUs free -- with 16 units
    per work-group (the H = 320 configs: 160 of 256 CUs) or else with 32
    (ctc5x512: 128 of 256 CUs; ASR_XG_BWD_XU=16 keeps 16 and mode '0') --
    otherwise '0'.  Units: ASR_XG_BWD_XU=16|32 forces them; auto takes 32 only
    for mode 3 when 16 would leave fewer than 32 CUs.  All modes need bf16 and
    the persistent recurrence."""
    mode = os.environ.get('ASR_OVERLAP_WGRAD', 'auto')
    xu_env = os.environ.get('ASR_XG_BWD_XU', 'auto')
    forced = 32 if xu_env == '32' else 16
    if compute_dtype() != BF16 or os.environ.get('ASR_LSTM_PERSIST', '1') == '0' or H % 32:
        return '0', forced
    ncu = _num_cus(dev)
    roomy16 = _xg_grid(B, H, ncu) + 32 <= ncu
    roomy32 = _xg_grid(B, H, ncu, 32) + 32 <= ncu
    if mode == 'auto':
        mode = '3' if roomy16 or (xu_env != '16' and roomy32) else '0'
    if mode == '1' and _xg_grid(B, H, 2 * (ncu - ncu // 2)) > ncu // 2:
        mode = '0'
    mode = mode if mode in ('1', '2', '3') else '0'
    if xu_env in ('16', '32'):
        return mode, forced
    return mode, (32 if mode == '3' and not roomy16 and roomy32 else 16)


def _overlap_mode(dev, B, H):
    """The resolved ASR_OVERLAP_WGRAD mode (see _overlap_plan)."""
    return _overlap_plan(dev, B, H)[0]


def _wgrad_side_stream(dev, B, H):
    """Where the weight-gradient GEMMs of a BLSTM layer's backward run:
    (stream, small_tiles, gated) or None (the compute stream); see
    _overlap_mode.  gated: the GEMMs wait for the next recurrence to be
    resident (asr_lstm_wgrad_gate) so they take the CUs it leaves free rather
    than CUs it needs."""
    mode = _overlap_mode(dev, B, H)
    if mode == '0':
        return None
    key = (dev.index, mode)
    ent = _side_streams.get(key)
    if ent is None:
        ncu = _num_cus(dev)
        if mode == '1':
            h = ctypes.c_void_p()
            with torch.cuda.device(dev):
                N.call('asr_stream_create_cu_masked', ncu // 2, ncu - ncu // 2, ctypes.byref(h))
            ent = torch.cuda.ExternalStream(h.value, device=dev)
        else:
            ent = torch.cuda.Stream(device=dev)
        _side_streams[key] = ent
    return ent, mode == '2', mode != '1'


_progress = {}   # device index -> [uint64 counter (device), running total of arrivals]


def _progress_counter(dev):
    ent = _progress.get(dev.index)
    if ent is None:
        ent = _progress[dev.index] = [torch.zeros(1, dtype=torch.int64, device=dev), 0]
    return ent


def _dx_split_chunks():
    """Row chunks the split input gradient computes beside the recurrence:
    ASR_DX_SPLIT=1 one ([T/4, 3T/4)), 2 two (and [T/8, T/4) + [3T/4, 7T/8))."""
    return 2 if os.environ.get('ASR_DX_SPLIT', '1') == '2' else 1


def _dx_split_ok(ctx, B, T, dev, mode):
    """Split input gradient (round 6, ASR_DX_SPLIT=0 turns it off): the
    backward recurrence reports when the gate gradients of the middle rows t in
    [T/4, 3T/4) are final (processing step 3T/4 - 1 of both directions), and
    their share of dX = dG W_ih runs on the weight-gradient side stream beside
    the last quarter of that recurrence, on the CUs it leaves free (mode 3);
    the outer rows follow on the compute stream.  Needs the packed-activation
    tagged-granule backward (the one that reports progress).  In the other
    overlap modes the same row bands run after the recurrence, so dX is the
    same arithmetic in every mode."""
    return (os.environ.get('ASR_DX_SPLIT', '1') != '0' and T >= 64
            and compute_dtype() == BF16 and ctx.needs_input_grad[0])


DX_CHUNK = int(os.environ.get('ASR_DX_CHUNK', '64'))   # processing steps per pipelined dX chunk
_dx_state = {}


def _dx_pipeline_ok(ctx, B, T, Din, dev):
    """The input gradient of this layer feeds only the backward recurrence of
    the BLSTM layer below (its input was handed over as bf16), that recurrence
    is the packed-activation tagged-granule kernel and it leaves >= 32 CUs
    free: dX may then be computed beside it.  Opt-in (ASR_DX_PIPE=1): at 5x512
    the free half of the chip runs these GEMMs and the weight gradients too
    slowly to stay ahead of the recurrence."""
    if not getattr(ctx, 'handoff_in', False) or os.environ.get('ASR_DX_PIPE', '0') not in ('1', '2'):
        return False
    if Din % 2 or not _act_h_on() or compute_dtype() != BF16 or (T + 1) // 2 > 4096 * DX_CHUNK:
        return False
    # the GEMMs need CUs beside that recurrence (140 KB LDS pin: none on its CUs)
    _, xu = _overlap_plan(dev, B, Din // 2)
    grid = N.query('asr_lstm_backward_grid', B, Din // 2, xu)
    return grid > 0 and grid + 32 <= _num_cus(dev)


def _dx_pipelined(dx, dg_op, w_op, B, T, H, Din, Dp, drop, dev):
    """dX [B, T, Din] = dG W_ih in chunks of time steps from both ends of the
    sequence inwards -- the order in which the layer below's backward
    recurrence reads them (steps q: rows t = q and T - 1 - q) -- each chunk
    signalled by a flag (asr_lstm_dy_signal) the recurrence polls before
    reading its dy rows.  ASR_DX_PIPE=1: every chunk (ASR_DX_CHUNK steps) on a
    high-priority side stream that first waits for that recurrence to be
    resident (asr_lstm_wgrad_gate), so the GEMMs take the CUs it leaves free.
    ASR_DX_PIPE=2: two chunks of about T / 4 steps -- the outer rows on the
    main stream with the whole chip before the recurrence is launched, the
    middle rows beside it, where the recurrence reaches them ~T/4 steps later.
    dx carries (flags, c0, epoch, done-event) as _asr_dy_pipe."""
    st = _dx_state.get(dev.index)
    if st is None:
        st = {'flags': torch.zeros(4096, dtype=torch.int32, device=dev),
              'stream': torch.cuda.Stream(device=dev, priority=-1), 'epoch': 0}
        _dx_state[dev.index] = st
    st['epoch'] = st['epoch'] % 0x7ffffff0 + 1
    epoch, flags, side = st['epoch'], st['flags'], st['stream']
    main = torch.cuda.current_stream(dev)
    half = (T + 1) // 2
    head_main = os.environ.get('ASR_DX_PIPE', '0') == '2'
    c0 = DX_CHUNK
    if head_main and 'ASR_DX_CHUNK' not in os.environ:
        c0 = (half + 1) // 2

    def chunk(k, gemm_opts=None):
        s0, s1 = k * c0, (k + 1) * c0
        probs = []
        for t0, t1 in ((s0, min(s1, half)), (max(T - s1, half), T - s0)):
            if t1 <= t0:
                continue
            n = t1 - t0
            a = operand(dg_op, 0, rowmap(8 * H, stride_b=T * 8 * H, rows_per_b=n, t_add=t0))
            c_map = rowmap(Din, stride_b=T * Din, rows_per_b=n, t_add=t0)
            probs.append(gemm_problem(a, operand(w_op, 1, rowmap(Dp)), dx, c_map, B * n,
                                      Din, 8 * H, drop=drop))
        run_gemm(probs, dev, opts=gemm_opts)
        N.call('asr_lstm_dy_signal', N.ptr(flags), k, epoch, N.stream_handle(dev))

    nch = (half + c0 - 1) // c0
    k0 = 0
    if head_main:   # the first chunk with the whole chip, before the recurrence
        chunk(0)
        k0 = 1
    side.wait_stream(main)
    small = os.environ.get('ASR_DX_SMALL', '1') != '0'   # 128 x 128 tiles: more work-groups
    with torch.cuda.stream(side):
        if k0 < nch:
            N.call('asr_lstm_wgrad_gate', N.stream_handle(dev))
        for k in range(k0, nch):
            chunk(k, SMALL_TILES if small else None)
        done = torch.cuda.Event()
        done.record(side)
    for t in (dx, dg_op, w_op, flags):
        t.record_stream(side)
    dx._asr_dy_pipe = (flags, c0, epoch, done)
    return done


def blstm_layer(x_src, lens, T, w_ih, w_hh, b_ih, b_hh, perm=None, t_mul=1, t_add=0, gbufs=None,
                graph_params=(), concat=False, drop=None, next_rec=False, bf16_handoff=False,
                out_drop=None):
    """gbufs: optional (g_w_ih, g_w_hh, g_b_ih, g_b_hh) gradient views to accumulate
    into; default: the tensors' own .grad.  graph_params: the nn.Parameters the
    combined [fwd; rev] views alias -- passed only so autograd records that the
    output depends on them (their gradients are written by the kernels).
    concat: input row t is [x_src[t*t_mul + t_add]; x_src[t*t_mul + t_add + 1]]
    ('concat' subsampling of the previous layer, read in place).
    drop: optional (p, seed): the layer reads dropout(x_src) (asr_dropout's mask),
    fused into the bf16 input staging; its input gradient gets the same mask.
    next_rec: another BLSTM layer's backward recurrence follows this layer's in
    the backward pass (the layer below), so ASR_OVERLAP_WGRAD=2 can run this
    layer's weight gradients beside it.
    bf16_handoff: the output's only consumer is the next BLSTM layer, reading
    it through an identity row map with drop=out_drop (its fused dropout, or
    None): in bf16 mode the fused forward then writes that layer's staged
    bf16 input (dropout applied) instead of the f32 output, whose tensor is
    returned unwritten (for autograd; reading it otherwise raises in the next
    layer, and no other consumer may read it)."""
    spec = (not (bf16_handoff and compute_dtype() == BF16 and handoff_on()),
            out_drop if bf16_handoff else None)
    return BLSTMLayerFn.apply(x_src, lens, T, perm, t_mul, t_add, gbufs, bool(concat), drop,
                              bool(next_rec), spec, w_ih, w_hh, b_ih, b_hh, *graph_params)


def handoff_on():
    """ASR_BF16_HANDOFF=0: every BLSTM layer writes its f32 output and the next
    layer stages it (A/B)."""
    return os.environ.get('ASR_BF16_HANDOFF', '1') != '0'


def _handoff_input(x_src, perm, t_mul, t_add, T, concat, drop, din):
    """The bf16 tensor a BLSTM layer's input was handed over as (see
    blstm_layer's bf16_handoff), or None for an ordinary f32 input.  Raises if
    the input was handed over but this layer cannot read it that way (its f32
    values were never written)."""
    h = getattr(x_src, '_asr_handoff', None)
    if h is None:
        return None
    t, hdrop = h
    B = x_src.shape[0]
    ok = (compute_dtype() == BF16 and perm is None and t_mul == 1 and t_add == 0 and
          not concat and x_src.shape[1] == T and x_src.shape[2] == din and din % 8 == 0 and
          drop == hdrop and t.shape == (B, T, din))
    if not ok:
        raise N.NativeError('BLSTM layer input was handed over as bf16 (its f32 values were '
                            'not written) but this layer cannot stage it that way')
    return t


# ---------------------------------------------------------------------------
# Elementwise: dropout (counter RNG), tanh, embedding
# ---------------------------------------------------------------------------
_seed = {'v': 1623}


def manual_seed(seed):
    _seed['v'] = int(seed)


_seed_log = {'on': False, 'seeds': []}   # tests: record the dropout seeds a step drew


def _next_seed():
    _seed['v'] = (_seed['v'] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
    if _seed_log['on']:
        _seed_log['seeds'].append(_seed['v'])
    return _seed['v']


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed=None):
        N.require_device(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        seed = _next_seed() if seed is None else int(seed)
        N.call('asr_dropout', N.ptr(x), N.ptr(y), x.numel(), float(p), seed,
               N.stream_handle(x.device))
        ctx.meta = (float(p), seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.meta
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        N.call('asr_dropout', N.ptr(dy), N.ptr(dx), dy.numel(), p, seed,
               N.stream_handle(dy.device))
        return dx, None, None


def dropout(x, p, seed=None):
    """nn.Dropout in training mode; element i of x is kept iff the counter RNG
    u01(seed, i) >= p (seed drawn from the module stream unless given)."""
    return DropoutFn.apply(x, p, seed) if p > 0 else x


def next_seed():
    return _next_seed()


class AddTanhFn(torch.autograd.Function):
    """y = tanh(a + b), one pass; d a = d b = dy (1 - y^2)."""

    @staticmethod
    def forward(ctx, a, b):
        N.require_device(a, b)
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        N.call('asr_add_tanh_forward', N.ptr(a), N.ptr(b), N.ptr(y), y.numel(),
               N.stream_handle(a.device))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        N.call('asr_tanh_backward', N.ptr(y), N.ptr(dy), N.ptr(dx), y.numel(),
               N.stream_handle(y.device))
        return dx, dx


def add_tanh(a, b):
    return AddTanhFn.apply(a, b)


class AddFn(torch.autograd.Function):
    """y = a + b (residual connections); d a = d b = dy."""

    @staticmethod
    def forward(ctx, a, b):
        N.require_device(a, b)
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        N.call('asr_add_forward', N.ptr(a), N.ptr(b), N.ptr(y), y.numel(),
               N.stream_handle(a.device))
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return AddFn.apply(a, b)


class AddBatchSumFn(torch.autograd.Function):
    """y[b] = h[b] + sum_b' lower[b'] -- the reference decoder's residual
    connection ``hx_list[l] += sum(hx_list[l - 1])`` (rnn_decoder.py:100-102),
    where Python's sum runs over the BATCH dimension of the lower layer's
    output.  Both sums are [1 x B] x [B x D] products and the broadcast is a
    K = 1 product accumulated onto a copy of h (asr_gemm)."""

    @staticmethod
    def _bsum_bcast(x, out):
        """out[b] += sum_b' x[b'] for x, out [B, D] (out already holds the addend)."""
        B, D = x.shape
        dev = x.device
        ones = torch.ones(B, 1, dtype=torch.float32, device=dev)
        sm = torch.empty(1, D, dtype=torch.float32, device=dev)
        run_gemm([gemm_problem(operand(ones, 1, rowmap(1)), operand(x, 1, rowmap(D)), sm,
                               rowmap(D), 1, D, B)], dev)
        run_gemm([gemm_problem(operand(ones, 0, rowmap(1)), operand(sm, 1, rowmap(D)), out,
                               rowmap(D), B, D, 1, beta=1.0)], dev)
        return out

    @staticmethod
    def forward(ctx, h, lower):
        N.require_device(h, lower)
        return AddBatchSumFn._bsum_bcast(lower.contiguous(), h.contiguous().clone())

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return dy, AddBatchSumFn._bsum_bcast(dy, torch.zeros_like(dy))


def add_batch_sum(h, lower):
    return AddBatchSumFn.apply(h, lower)


class TanhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N.require_device(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        N.call('asr_tanh_forward', N.ptr(x), N.ptr(y), x.numel(), N.stream_handle(x.device))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        N.call('asr_tanh_backward', N.ptr(y), N.ptr(dy), N.ptr(dx), y.numel(),
               N.stream_handle(y.device))
        return dx


def tanh(x):
    return TanhFn.apply(x)


class EmbeddingFn(torch.autograd.Function):
    """trans=0: weight [V, E] (nn.Embedding); trans=1: weight [E, V] (Embedding_LS).
    idx_host (optional numpy copy of idx): the backward groups rows by token on
    the host (CSR) instead of scanning every row per (token, column)."""

    @staticmethod
    def forward(ctx, idx, weight, trans, padding_idx, idx_host=None):
        N.require_device(idx, weight)
        idx = idx.contiguous().long()
        V, E = (weight.shape[1], weight.shape[0]) if trans else weight.shape
        out = torch.empty(*idx.shape, E, dtype=torch.float32, device=idx.device)
        N.call('asr_embedding_forward', N.ptr(idx), N.ptr(weight), idx.numel(), V, E, int(trans),
               N.ptr(out), N.stream_handle(idx.device))
        ctx.save_for_backward(idx, weight)
        ctx.meta = (trans, padding_idx, V, E, idx_host)
        ctx.beside = _beside_plan[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, weight = ctx.saved_tensors
        trans, padding_idx, V, E, idx_host = ctx.meta
        dout = dout.contiguous()
        pad = -1 if padding_idx is None else int(padding_idx)
        dev = idx.device
        if idx_host is not None:
            flat = np.clip(np.asarray(idx_host, np.int64).reshape(-1), 0, V - 1)
            order = np.argsort(flat, kind='stable').astype(np.int32)
            starts = np.zeros(V + 1, np.int32)
            np.cumsum(np.bincount(flat, minlength=V), out=starts[1:])
            order_d = h2d(order, dev)
            starts_d = h2d(starts, dev)

            def wgrad(_gemm_opts):   # (no GEMM in either form)
                N.call('asr_embedding_backward_csr', N.ptr(order_d), N.ptr(starts_d), N.ptr(dout),
                       V, E, int(trans), pad, N.ptr(grad_buffer(weight)), N.stream_handle(dev))
            keep = (order_d, starts_d, dout)
        else:
            def wgrad(_gemm_opts):
                N.call('asr_embedding_backward', N.ptr(idx), N.ptr(dout), idx.numel(), V, E,
                       int(trans), pad, N.ptr(grad_buffer(weight)), N.stream_handle(dev))
            keep = (idx, dout)
        # the embedding gradient has no consumer but the optimizer: beside the
        # encoder's top backward recurrence when the decoder is built under
        # wgrad_beside_encoder
        if ctx.beside is None or not _wgrad_beside(dev, ctx.beside, wgrad, keep,
                                                   (grad_buffer(weight),)):
            wgrad(None)
        return None, None, None, None, None


def embedding(idx, weight, padding_idx=None, idx_host=None):
    return EmbeddingFn.apply(idx, weight, 0, padding_idx, idx_host)


def embedding_t(idx, weight_ev, idx_host=None):
    return EmbeddingFn.apply(idx, weight_ev, 1, None, idx_host)


class CTCLossFn(torch.autograd.Function):
    """loss = loss_scale * sum_b CTC(logits_b, labels_b); logits [B, T, V] f32
    batch-major (no time-major transpose copy).  The gradient is produced in
    backward, already multiplied by grad_output * loss_scale, in one write."""

    @staticmethod
    def forward(ctx, logits, labels_flat, label_lens, act_lens, max_label_len, loss_scale,
                blank=0, zero_infinity=True):
        N.require_device(logits, labels_flat, label_lens, act_lens)
        logits = logits.contiguous()
        B, T, V = logits.shape
        costs, loss, ws, nbytes = _ctc_forward(logits, V, T * V, T, B, V, None, labels_flat,
                                               label_lens, act_lens, max_label_len, blank,
                                               zero_infinity, loss_scale)
        ctx.save_for_backward(logits, labels_flat, label_lens, act_lens, ws)
        ctx.meta = (int(max_label_len), int(blank), float(loss_scale), nbytes)
        ctx.mark_non_differentiable(costs)
        return loss, costs

    @staticmethod
    def backward(ctx, g_loss, g_costs):
        logits, labels_flat, label_lens, act_lens, ws = ctx.saved_tensors
        max_label_len, blank, loss_scale, nbytes = ctx.meta
        B, T, V = logits.shape
        grads = torch.empty_like(logits)
        g = g_loss.contiguous() if g_loss is not None else None
        N.call('asr_ctc_backward', N.ptr(logits), V, T * V, T, B, V, N.ptr(labels_flat),
               N.ptr(label_lens), N.ptr(act_lens), max_label_len, blank, N.ptr(g),
               loss_scale if g is not None else 0.0, N.ptr(grads), V, T * V, N.ptr(ws), nbytes,
               N.stream_handle(logits.device))
        return grads, None, None, None, None, None, None, None


class XentFn(torch.autograd.Function):
    """Fused CE (ignore -1) + uniform label smoothing over rows of logits."""

    @staticmethod
    def forward(ctx, logits, targets, lens, T, ce_scale, ls_scale):
        N.require_device(logits)
        logits = logits.contiguous()
        V = logits.shape[-1]
        R = logits.numel() // V
        nb = N.query('asr_xent_workspace_bytes', R)
        ws = _ws(nb, logits.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        tg = targets.contiguous().long() if targets is not None else None
        ln = lens.contiguous().int() if lens is not None else None
        N.call('asr_xent_forward', N.ptr(logits), R, V, int(T), N.ptr(tg), N.ptr(ln),
               float(ce_scale), float(ls_scale), N.ptr(loss), N.ptr(ws), nb,
               N.stream_handle(logits.device))
        ctx.save_for_backward(logits, ws)
        ctx.meta = (tg, ln, int(T), float(ce_scale), float(ls_scale), nb)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, ws = ctx.saved_tensors
        tg, ln, T, ce_scale, ls_scale, nb = ctx.meta
        V = logits.shape[-1]
        R = logits.numel() // V
        d = torch.empty_like(logits)
        g = g.contiguous()
        N.call('asr_xent_backward', N.ptr(logits), R, V, T, N.ptr(tg), N.ptr(ln), ce_scale,
               ls_scale, N.ptr(g), 1.0, N.ptr(d), N.ptr(ws), nb, N.stream_handle(logits.device))
        return d, None, None, None, None, None


def xent(logits, targets=None, lens=None, T=0, ce_scale=1.0, ls_scale=0.0):
    """Returns loss [1] = ce_scale * CE_sum + ls_scale * LS_sum (see asr_xent_forward)."""
    return XentFn.apply(logits, targets, lens, T, ce_scale, ls_scale)


def softmax(x):
    N.require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    V = x.shape[-1]
    N.call('asr_softmax', N.ptr(x), x.numel() // V, V, N.ptr(y), N.stream_handle(x.device))
    return y


def ctc_best_path(logits, lens, blank=0):
    """CTC greedy best path on device: returns (hyps int32 [B, T], hyp_lens int32 [B])."""
    N.require_device(logits, lens)
    logits = logits.contiguous()
    B, T, V = logits.shape
    hyps = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    hl = torch.empty(B, dtype=torch.int32, device=logits.device)
    N.call('asr_ctc_best_path', N.ptr(logits), V, T * V, T, B, V, N.ptr(lens.int().contiguous()),
           int(blank), N.ptr(hyps), N.ptr(hl), N.stream_handle(logits.device))
    return hyps, hl


def ctc_best_path_stream(logits, lens, prev, blank=0):
    """CTC best path of one chunk [B, Tc, V] of longer utterances.  lens int32
    [B]: the chunk's valid frames per row; prev int32 [B] on the device, updated
    in place: the label of each row's last valid frame so far (-1 before the
    first), through which repeats collapse across chunk boundaries.  Returns
    (hyps int32 [B, Tc], hyp_lens int32 [B]): the labels this chunk newly emits."""
    N.require_device(logits, lens, prev)
    logits = logits.contiguous()
    B, T, V = logits.shape
    assert prev.dtype == torch.int32 and prev.is_contiguous() and tuple(prev.shape) == (B,)
    lens = lens.int().contiguous()
    hyps = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    hl = torch.empty(B, dtype=torch.int32, device=logits.device)
    N.call('asr_ctc_best_path_stream', N.ptr(logits), V, T * V, T, B, V, N.ptr(lens), int(blank),
           N.ptr(prev), N.ptr(hyps), N.ptr(hl), N.stream_handle(logits.device))
    return hyps, hl


_beam_ws = {}    # device -> workspace of the largest ctc_beam_search call so far
_ctc_beam = {'path': None}


def last_ctc_beam_path():
    """Where the last CTC prefix beam search ran (None before the first one):
    'device' (asr_ctc_beam_search, no LM and no insertion bonus), 'device_lm'
    (asr_ctc_beam_search_lm), 'host' (the decoder's numpy search: the kernels
    refused the LM, or ASR_CTC_BEAM=host), or after a session's feed
    (asr_ctc_beam_stream_feed) 'stream' (no LM and no bonus) / 'stream_lm'."""
    return _ctc_beam['path']


def _ctc_lm_args(who, lm, V, beta):
    """What the CTC searches ask of lm (None: no LM) and beta before any call:
    (the LM struct, the tensors it points into), or (None, None)."""
    lms, keep = _lm_struct(lm, who) if lm is not None else (None, None)
    if lm is not None and (int(lm['emb'].shape[0]) != V or int(lm['w_out'].shape[0]) != V):
        raise ValueError('%s: the LM has %d classes, the CTC head %d (blank '
                         'included; <eos> takes its place)' % (who, lm['w_out'].shape[0], V))
    if not np.isfinite(beta):
        raise ValueError('%s: beta = %r is not finite' % (who, beta))
    return lms, keep


def ctc_beam_search(logits, lens, beam_width, blank=0, normalize=True, lm=None, beta=0.0):
    """CTC prefix beam search on device: logits [B, T, V] raw (normalize=True:
    the log-softmax is fused) or log-probabilities.  Returns (hyps int32 [B, T],
    hyp_lens int32 [B], scores float32 [B]).

    lm is None and beta == 0: asr_ctc_beam_search.  Otherwise
    asr_ctc_beam_search_lm (csrc/ctc_beam.hip states the contract): lm is
    RNNLM.device_weights() plus weight (alpha >= 0; 0: the LM term is absent), an
    LM of exactly V classes (CTC class c != blank is LM class c - (c > blank),
    <eos> = V - 1), all f32 on the device; beta is the insertion bonus per
    label.  Returns None when the kernels refuse the LM (ASR_ERR_UNSUPPORTED: a
    GRU LM, more layers than the limit; the reason is asr_last_error's)."""
    N.require_device(logits, lens)
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    dev = logits.device
    W, beta = int(beam_width), float(beta)
    lms, keep = _ctc_lm_args('ctc_beam_search', lm, V, beta)
    hyps = torch.empty(B, T, dtype=torch.int32, device=dev)
    hl = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    lens_d = lens.int().contiguous()
    if lm is None and beta == 0:
        ws = _grown_ws(_beam_ws, N.query('asr_ctc_beam_ws_bytes', T, B, V, W), dev)
        N.call('asr_ctc_beam_search', N.ptr(logits), V, T * V, T, B, V, N.ptr(lens_d), int(blank),
               W, int(bool(normalize)), N.ptr(ws), ws.numel(), N.ptr(hyps), N.ptr(hl),
               N.ptr(scores), N.stream_handle(dev))
        _ctc_beam['path'] = 'device'
        return hyps, hl, scores
    if lms is not None:
        nb = N.query('asr_ctc_beam_lm_ws_bytes', T, B, V, W, lms.layers, lms.H, lms.Y)
        if nb == 0 and 1 <= W <= 64:
            return None                  # the LM's shape is outside the kernels' limits
    else:
        nb = N.query('asr_ctc_beam_lm_ws_bytes', T, B, V, W, 0, 0, 0)
    ws = _grown_ws(_beam_ws, nb, dev)
    rc = N.lib().asr_ctc_beam_search_lm(
        N.ptr(logits), V, T * V, T, B, V, N.ptr(lens_d), int(blank), W, int(bool(normalize)),
        N.ptr_struct(lms), beta, N.ptr(ws), ws.numel(), N.ptr(hyps), N.ptr(hl), N.ptr(scores),
        N.stream_handle(dev))
    del keep
    if rc == N.ASR_ERR_UNSUPPORTED:
        return None
    if rc != N.ASR_OK:
        raise N.NativeError('asr_ctc_beam_search_lm failed (rc=%d): %s'
                            % (rc, N.lib().asr_last_error().decode(errors='replace')))
    _ctc_beam['path'] = 'device_lm'
    return hyps, hl, scores


class CtcBeamStreamState(object):
    """One streaming prefix-search session (ctc_beam_stream_state): the device
    state buffer, the session's constants and the LM struct with the tensors
    it points into."""
    __slots__ = ('buf', 'ws', 'B', 'V', 'W', 'max_frames', 'blank', 'normalize', 'beta', 'lms',
                 'keep', 'device')

    @property
    def lm_dims(self):
        """(layers, H, Y) of the state's layout: zeros where the LM term is absent."""
        if self.lms is None or self.lms.weight == 0:
            return 0, 0, 0
        return self.lms.layers, self.lms.H, self.lms.Y


def _beam_stream_rows(st, rows):
    if rows is None:
        return None
    mask = np.zeros(st.B, np.int32)
    mask[[int(r) for r in rows]] = 1
    return torch.from_numpy(mask).to(st.device)


def ctc_beam_stream_state(batch_size, num_classes, beam_width, max_frames, device, blank=0,
                          normalize=True, lm=None, beta=0.0):
    """A streaming CTC prefix-search session of `batch_size` rows over
    `num_classes` classes (asr_ctc_beam_stream_*; include/asr_hip.h states the
    contract), every row reset.  lm / beta as in ctc_beam_search; max_frames:
    the frames one utterance may hold between resets.  Raises
    NotImplementedError where the kernels refuse the LM (a GRU LM, more layers
    than the limit): a session has no host search."""
    st = CtcBeamStreamState()
    st.B, st.V, st.W, st.max_frames = int(batch_size), int(num_classes), int(beam_width), \
        int(max_frames)
    st.blank, st.normalize, st.beta, st.device = int(blank), bool(normalize), float(beta), device
    st.lms, st.keep = _ctc_lm_args('ctc_beam_stream', lm, st.V, st.beta)
    st.ws = {}                   # device -> the feeds' workspace
    nb = N.query('asr_ctc_beam_stream_state_bytes', st.max_frames, st.B, st.V, st.W, *st.lm_dims)
    # (a refused shape: the reset below names it)
    st.buf = _ws(max(nb, 16), device)
    ctc_beam_stream_reset(st)
    return st


def ctc_beam_stream_reset(st, rows=None):
    """The rows of `rows` (default: all) of a session at the empty prefix."""
    mask = _beam_stream_rows(st, rows)
    rc = N.lib().asr_ctc_beam_stream_reset(
        N.ptr(st.buf), st.buf.numel(), st.max_frames, st.B, st.V, st.W, N.ptr_struct(st.lms),
        N.ptr(mask), N.stream_handle(st.device))
    msg = N.lib().asr_last_error().decode(errors='replace') if rc != N.ASR_OK else ''
    if rc == N.ASR_ERR_UNSUPPORTED:
        raise NotImplementedError('asr_ctc_beam_stream_reset refused the LM: %s' % msg)
    if rc != N.ASR_OK:
        raise N.NativeError('asr_ctc_beam_stream_reset failed (rc=%d): %s' % (rc, msg))


def ctc_beam_stream_feed(st, logits, lens, final=None, stable=True):
    """One chunk [B, Tc, V] of a session: lens int32 [B] valid frames per row,
    final int32 [B] device tensor (or None).  Returns (hyps int32 [B,
    max_frames], hyp_lens int32 [B], scores float32 [B], stable_lens int32 [B]
    or None with stable=False): each row's current best prefix in full."""
    N.require_device(logits, lens, final)
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    assert (B, V) == (st.B, st.V), 'the chunk is [%d, ., %d], the session [%d, ., %d]' % (
        B, V, st.B, st.V)
    dev = logits.device
    ws = _grown_ws(st.ws, N.query('asr_ctc_beam_stream_ws_bytes', T, B, V, st.W), dev)
    hyps = torch.empty(B, st.max_frames, dtype=torch.int32, device=dev)
    hl = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    sl = torch.empty(B, dtype=torch.int32, device=dev) if stable else None
    if final is not None:
        final = final.int().contiguous()
    N.call('asr_ctc_beam_stream_feed', N.ptr(logits), V, T * V, T, B, V,
           N.ptr(lens.int().contiguous()), st.blank, st.W, int(st.normalize), N.ptr_struct(st.lms),
           st.beta, N.ptr(final), N.ptr(st.buf), st.buf.numel(), st.max_frames, N.ptr(ws),
           ws.numel(), N.ptr(hyps), st.max_frames, N.ptr(hl), N.ptr(scores), N.ptr(sl),
           N.stream_handle(dev))
    _ctc_beam['path'] = 'stream' if st.lm_dims[0] == 0 and st.beta == 0 else 'stream_lm'
    return hyps, hl, scores, sl


def ctc_beam_stream_nbest(st):
    """Every beam entry of a session in rank order: (hyps int32 [B, W,
    max_frames], lens int32 [B, W], scores float32 [B, W], counts int32 [B])."""
    dev = st.device
    hyps = torch.empty(st.B, st.W, st.max_frames, dtype=torch.int32, device=dev)
    lens = torch.empty(st.B, st.W, dtype=torch.int32, device=dev)
    scores = torch.empty(st.B, st.W, dtype=torch.float32, device=dev)
    counts = torch.empty(st.B, dtype=torch.int32, device=dev)
    layers, H, _ = st.lm_dims
    N.call('asr_ctc_beam_stream_nbest', N.ptr(st.buf), st.buf.numel(), st.max_frames, st.B, st.V,
           st.W, layers, H, N.ptr(hyps), st.max_frames, N.ptr(lens), N.ptr(scores), N.ptr(counts),
           N.stream_handle(dev))
    return hyps, lens, scores, counts


def ctc_beam_stream_status(st):
    """The rows' status words, int32 [B] on the device: bit 0: frames were
    dropped at max_frames; bit 1: the row was fed before any reset."""
    out = torch.empty(st.B, dtype=torch.int32, device=st.device)
    N.call('asr_ctc_beam_stream_status', N.ptr(st.buf), st.B, N.ptr(out),
           N.stream_handle(st.device))
    return out


# ---------------------------------------------------------------------------
# Hypothesis scoring (csrc/edit_distance.hip)
# ---------------------------------------------------------------------------
_edit = {'path': None, 'ws': {}}   # ws: device -> workspace of the largest call so far


def last_edit_distance_path():
    """'device' or 'host': where the last edit_distance ran (None before the
    first one).  'host': the kernel refused the shape (ASR_ERR_UNSUPPORTED)."""
    return _edit['path']


def edit_clean_host(seq, n, is_hyp, eos, space, token_map):
    """Steps 1-3 of asr_edit_distance's clean-up on a host row."""
    out = []
    for t in list(seq)[:max(0, int(n))]:
        t = int(t)
        if t < 0:
            continue
        if is_hyp and eos is not None and eos >= 0 and t == eos:
            break
        if token_map is not None and t < len(token_map):
            t = int(token_map[t])
            if t < 0:
                continue
        if space is not None and space >= 0 and t == space and (not out or out[-1] == space):
            continue
        out.append(t)
    if space is not None and space >= 0 and out and out[-1] == space:
        out.pop()
    return out


def edit_units_host(tokens, unit, space):
    """Steps 4-5: the units of a cleaned row (words as tuples of tokens)."""
    if unit != 'word':
        return list(tokens)
    words, cur = [], []
    for t in tokens:
        if t == space:
            words.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    if cur or words:
        words.append(tuple(cur))
    return words


def edit_counts_host(ref, hyp):
    """(distance, sub, ins, del) of two unit lists: compute_wer's table and
    backtrace (utils/evaluation/edit_distance.py:53-126) with the border rule
    of asr_edit_distance (x == 0: insertions, y == 0: deletions)."""
    R, H = len(ref), len(hyp)
    d = [list(range(H + 1))] + [[i] + [0] * H for i in range(1, R + 1)]
    for i in range(1, R + 1):
        di, dp, r = d[i], d[i - 1], ref[i - 1]
        for j in range(1, H + 1):
            di[j] = dp[j - 1] if r == hyp[j - 1] else 1 + min(dp[j - 1], di[j - 1], dp[j])
    x, y, sub, ins, dele = R, H, 0, 0, 0
    while x > 0 or y > 0:
        if x == 0:
            ins, y = ins + 1, y - 1
        elif y == 0:
            dele, x = dele + 1, x - 1
        elif ref[x - 1] == hyp[y - 1]:
            x, y = x - 1, y - 1
        elif d[x][y] == d[x][y - 1] + 1:
            ins, y = ins + 1, y - 1
        elif d[x][y] == d[x - 1][y - 1] + 1:
            sub, x, y = sub + 1, x - 1, y - 1
        else:
            dele, x = dele + 1, x - 1
    return d[R][H], sub, ins, dele


def edit_distance_host(hyp, hyp_lens, ref, ref_lens, unit='token', eos=None, space=None,
                       token_map=None):
    """asr_edit_distance restated on host arrays: int32 [B, 5]."""
    out = np.zeros((len(hyp), 5), np.int32)
    for b in range(len(hyp)):
        r = edit_units_host(edit_clean_host(ref[b], ref_lens[b], False, eos, space, token_map),
                            unit, space)
        h = edit_units_host(edit_clean_host(hyp[b], hyp_lens[b], True, eos, space, token_map),
                            unit, space)
        out[b, :4] = edit_counts_host(r, h)
        out[b, 4] = len(r)
    return out


def _i32_rows(t, keep_i64=False):
    if t.dtype != torch.int32 and not (keep_i64 and t.dtype == torch.int64):
        t = t.to(torch.int32)
    if t.dim() != 2:
        raise ValueError('edit_distance: [B, L] token tensors expected, got %r' % (tuple(t.shape),))
    if t.shape[1] == 0:      # no storage to point at: one column of padding instead
        return torch.full((t.shape[0], 1), -1, dtype=t.dtype, device=t.device)
    return t if t.stride(1) == 1 else t.contiguous()


@torch.no_grad()
def edit_distance(hyp, hyp_lens, ref, ref_lens, unit='token', eos=None, space=None,
                  token_map=None, totals=None):
    """Edit distance and error counts per utterance on the device
    (asr_edit_distance): hyp int32 / int64 [B, Lh] and ref [B, Lr] device
    tensors as the decoders return them, lengths [B].  unit 'token' or 'word'
    (needs `space`); eos: the hypothesis is cut before it; space: separator
    (runs collapse, leading / trailing go); token_map: int sequence or device
    int32 tensor, token -> token or -1 to delete.  Returns int32 [B, 5] =
    (distance, sub, ins, del, ref units) on the device; totals (int64 [5]
    device tensor) += its column sums, with no host synchronisation.  A shape
    the kernel refuses runs edit_distance_host on host copies instead and
    last_edit_distance_path() says so."""
    N.require_device(hyp, ref)
    if unit not in ('token', 'word'):
        raise ValueError("edit_distance: unit must be 'token' or 'word'")
    dev = hyp.device
    hyp, ref = _i32_rows(hyp, keep_i64=True), _i32_rows(ref)
    B = hyp.shape[0]
    as_lens = lambda l: (l if torch.is_tensor(l) else torch.as_tensor(   # noqa: E731
        np.asarray(l).astype(np.int32))).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    hl, rl = as_lens(hyp_lens), as_lens(ref_lens)
    if ref.shape[0] != B or hl.numel() != B or rl.numel() != B:
        raise ValueError('edit_distance: batch sizes differ')
    if totals is not None and (totals.dtype != torch.int64 or totals.numel() != 5 or
                               not totals.is_cuda or not totals.is_contiguous()):
        raise ValueError('edit_distance: totals must be a contiguous int64 [5] device tensor')
    out = torch.zeros(B, 5, dtype=torch.int32, device=dev)
    if B == 0:
        return out
    if token_map is not None and not torch.is_tensor(token_map):
        token_map = torch.as_tensor(np.asarray(token_map).astype(np.int32))
    if token_map is not None:
        token_map = token_map.to(device=dev, dtype=torch.int32).contiguous()
    max_h, max_r = hyp.shape[1], ref.shape[1]
    opts = N.EditOpts(N.ASR_ED_WORD if unit == 'word' else N.ASR_ED_TOKEN,
                      -1 if eos is None else int(eos), -1 if space is None else int(space),
                      None if token_map is None else token_map.data_ptr(),
                      0 if token_map is None else token_map.numel(),
                      int(hyp.dtype == torch.int64))
    nb = N.query('asr_edit_distance_ws_bytes', B, max_r, max_h)
    ws = _grown_ws(_edit['ws'], nb, dev)
    rc = getattr(N.lib(), 'asr_edit_distance')(
        N.ptr(hyp), max(hyp.stride(0), max_h), N.ptr(hl), N.ptr(ref), max(ref.stride(0), max_r),
        N.ptr(rl), B, max_r, max_h, ctypes.byref(opts), N.ptr(out), N.ptr(totals), N.ptr(ws),
        ws.numel(), N.stream_handle(dev))
    if rc == N.ASR_OK:
        _edit['path'] = 'device'
        return out
    if rc != N.ASR_ERR_UNSUPPORTED:
        raise N.NativeError('asr_edit_distance failed (rc=%d): %s'
                            % (rc, N.lib().asr_last_error().decode(errors='replace')))
    _edit['path'] = 'host'
    res = edit_distance_host(hyp.cpu().numpy(), hl.cpu().numpy(), ref.cpu().numpy(),
                             rl.cpu().numpy(), unit, eos, space,
                             None if token_map is None else token_map.cpu().numpy())
    out = torch.from_numpy(res).to(dev)
    if totals is not None:
        totals += out.sum(dim=0, dtype=torch.int64)
    return out


# ---------------------------------------------------------------------------
# CTC forced alignment (csrc/ctc_align.hip)
# ---------------------------------------------------------------------------
_align = {'path': None, 'ws': {}}   # ws: device -> workspace of the largest call so far


def last_ctc_align_path():
    """'device' or 'host': where the last ctc_align ran (None before the first
    one).  'host': the kernel refused the shape (ASR_ERR_UNSUPPORTED)."""
    return _align['path']


def ctc_align_limits():
    """(frames per backtrace chunk, frames whose backpointers stay in LDS) of
    asr_ctc_align (asr_ctc_align_limits)."""
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    N.call('asr_ctc_align_limits', ctypes.byref(c), ctypes.byref(r))
    return c.value, r.value


def ctc_align_host(logits, lens, labels_flat, label_lens, max_label_len, blank=0, normalize=True,
                   spans=True):
    """asr_ctc_align restated on host arrays in numpy float32 (the recurrence
    of include/asr_hip.h: raw logits, one rounding per add, first predecessor
    in the order s, s-1, s-2 on ties).  logits [B, T, V]; returns numpy
    (ali int32 [B, T], starts, ends int32 [B, max_label_len] or None, scores
    float32 [B]); the normalised score is summed in float64 and rounded once."""
    x = np.asarray(logits, dtype=np.float32)
    B, T, V = x.shape
    lens = np.asarray(lens).reshape(-1).astype(np.int64)
    label_lens = np.asarray(label_lens).reshape(-1).astype(np.int64)
    flat = np.asarray(labels_flat).reshape(-1).astype(np.int64)
    M = int(max_label_len)
    ninf = np.float32(-np.inf)
    ali = np.full((B, T), -1, np.int32)
    starts = np.full((B, M), -1, np.int32)
    ends = np.full((B, M), -1, np.int32)
    scores = np.full(B, ninf, np.float32)
    off = 0
    for b in range(B):
        L = int(label_lens[b])
        lab = flat[off:off + max(L, 0)]
        off += max(L, 0)
        Tb = max(min(int(lens[b]), T), 0)
        if L < 0 or L > M or len(lab) != L or ((lab < 0) | (lab >= V) | (lab == blank)).any():
            continue
        if Tb == 0:
            if L == 0:
                scores[b] = 0
            continue
        S = 2 * L + 1
        cls = np.full(S, blank, np.int64)
        cls[1::2] = lab
        skip = np.zeros(S, bool)
        skip[3::2] = lab[1:] != lab[:-1]
        g = x[b, :Tb][:, cls]
        v = np.full(S, ninf, np.float32)
        v[:min(S, 2)] = g[0, :2]
        bp = np.zeros((Tb, S), np.int8)
        with np.errstate(invalid='ignore'):
            for t in range(1, Tb):
                a1 = np.concatenate(([ninf], v[:-1]))
                a2 = np.where(skip, np.concatenate(([ninf, ninf], v[:-2]))[:S], ninf)
                m, d = v.copy(), bp[t]
                k = a1 > m
                m[k], d[k] = a1[k], 1
                k = a2 > m
                m[k], d[k] = a2[k], 2
                v = (m + g[t]).astype(np.float32)
        s = S - 1 if L == 0 or v[S - 1] >= v[S - 2] else S - 2
        if not v[s] > ninf:
            continue
        end_value = v[s]
        path = np.empty(Tb, np.int64)
        for t in range(Tb - 1, -1, -1):
            path[t] = s
            s -= int(bp[t, s])
        ali[b, :Tb] = cls[path]
        for j in range(L):
            at = np.nonzero(path == 2 * j + 1)[0]
            starts[b, j], ends[b, j] = at[0], at[-1]
        if normalize:
            rows = x[b, :Tb].astype(np.float64)
            mx = rows.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(rows - mx).sum(axis=1))
            scores[b] = np.float32((g[np.arange(Tb), path].astype(np.float64) - lse).sum())
        else:
            scores[b] = end_value
    return ali, (starts if spans else None), (ends if spans else None), scores


@torch.no_grad()
def ctc_align(logits, lens, labels_flat, label_lens, max_label_len, blank=0, normalize=True,
              spans=True):
    """CTC forced alignment on the device (asr_ctc_align): logits [B, T, V]
    (any strides with a unit class stride: a transposed time-major tensor is
    read in place), lens [B], labels_flat / label_lens as for ctc_loss.
    Returns device tensors (ali int32 [B, T]: the class of every frame of the
    best path, -1 beyond the length and on infeasible rows; starts, ends int32
    [B, max_label_len]: first / last frame of every label, or None without
    `spans`; scores float32 [B]: the path's log-probability, or with
    normalize=False the sum of its raw logits).  No host synchronisation.  A
    shape the kernel refuses (max_label_len > 511) runs ctc_align_host on host
    copies instead and last_ctc_align_path() says so."""
    N.require_device(logits, lens, labels_flat, label_lens)
    dev = logits.device
    if logits.dtype != torch.float32:
        logits = logits.float()
    if logits.dim() != 3:
        raise ValueError('ctc_align: [B, T, V] logits expected, got %r' % (tuple(logits.shape),))
    if logits.stride(2) != 1 or logits.stride(0) <= 0 or logits.stride(1) <= 0:
        logits = logits.contiguous()
    B, T, V = logits.shape
    M = int(max_label_len)
    lens = lens.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    label_lens = label_lens.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    labels_flat = labels_flat.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if lens.numel() != B or label_lens.numel() != B:
        raise ValueError('ctc_align: batch sizes differ')
    if labels_flat.numel() == 0:    # no storage to point at
        labels_flat = torch.zeros(1, dtype=torch.int32, device=dev)
    ali = torch.empty(B, T, dtype=torch.int32, device=dev)
    starts = torch.empty(B, M, dtype=torch.int32, device=dev) if spans else None
    ends = torch.empty(B, M, dtype=torch.int32, device=dev) if spans else None
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0 or T == 0:
        raise ValueError('ctc_align: empty batch or no frames')
    nb = N.query('asr_ctc_align_ws_bytes', T, B, V, M)
    ws = _grown_ws(_align['ws'], nb, dev)
    rc = getattr(N.lib(), 'asr_ctc_align')(
        N.ptr(logits), logits.stride(1), logits.stride(0), T, B, V, N.ptr(labels_flat),
        N.ptr(label_lens), N.ptr(lens), M, int(blank), int(bool(normalize)), N.ptr(ali),
        N.ptr(starts) if spans and M else None, N.ptr(ends) if spans and M else None,
        N.ptr(scores), N.ptr(ws), ws.numel(), N.stream_handle(dev))
    if rc == N.ASR_OK:
        _align['path'] = 'device'
        return ali, starts, ends, scores
    if rc != N.ASR_ERR_UNSUPPORTED:
        raise N.NativeError('asr_ctc_align failed (rc=%d): %s'
                            % (rc, N.lib().asr_last_error().decode(errors='replace')))
    _align['path'] = 'host'
    res = ctc_align_host(logits.cpu().numpy(), lens.cpu().numpy(), labels_flat.cpu().numpy(),
                         label_lens.cpu().numpy(), M, blank, normalize, spans)
    return tuple(None if r is None else torch.from_numpy(r).to(dev) for r in res)


def row_argmax(x):
    N.require_device(x)
    x = x.contiguous()
    V = x.shape[-1]
    out = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    N.call('asr_row_argmax', N.ptr(x), x.numel() // V, V, N.ptr(out), N.stream_handle(x.device))
    return out


def ctc_loss(logits, labels_flat, label_lens, act_lens, max_label_len, loss_scale=1.0, blank=0,
             zero_infinity=True):
    """Returns (loss [1], costs [B])."""
    return CTCLossFn.apply(logits, labels_flat, label_lens, act_lens, max_label_len, loss_scale,
                           blank, zero_infinity)


# ---------------------------------------------------------------------------
# VGG front-end (CNNEncoder, models/pytorch_v3/encoders/cnn.py:124-165)
# ---------------------------------------------------------------------------
def _tap_operand(t, trans, stride, group, pitch, sign):
    op = operand(t, trans, rowmap(stride))
    op.tap_group, op.tap_pitch, op.tap_sign = int(group), int(pitch), int(sign)
    return op


def _pool_dims(T, F, pt, pf, ceil):
    To, Fo = ctypes.c_int(), ctypes.c_int()
    N.call('asr_vgg_pool_dims', T, F, pt, pf, ceil, ctypes.byref(To), ctypes.byref(Fo))
    return To.value, Fo.value


def _halo_only(C, dtype):
    """A padded VGG operand whose producer writes every interior pixel needs
    only its halo zeroed (16-B rows; ASR_VGG_HALO_ONLY=0 zero-fills it whole)."""
    size = 2 if dtype == torch.bfloat16 else 4
    return C % 4 == 0 and (C * size) % 16 == 0 and os.environ.get('ASR_VGG_HALO_ONLY', '1') != '0'


def _zero_halo(buf, B, T, F, C):
    N.call('asr_vgg_zero_halo', N.ptr(buf), BF16 if buf.dtype == torch.bfloat16 else F32, int(B),
           int(T), int(F), int(C), N.stream_handle(buf.device))


_TWO_GIB = 1 << 31


def _conv_tr_ok(cin, cout, fp, P, out_bytes):
    """bf16 mode: the tap-resident convolution kernel (csrc/conv.hip) takes this
    channel pair and operand sizes -- every operand below 2 GiB, the kernel's
    buffer-resource limit (ASR_VGG_TR=0 keeps the tap-addressed GEMM, for A/B)."""
    return (compute_dtype() == BF16 and os.environ.get('ASR_VGG_TR', '1') != '0' and
            P * cin * 2 < _TWO_GIB and P * cout * out_bytes < _TWO_GIB and
            N.query('asr_conv3x3_tr_supported', int(cin), int(cout), int(fp)) == 1)


def _c1_wgrad_ok(B, T, F, co):
    """The first layer's weight gradient from the raw features
    (asr_conv3x3_c1_wgrad_xs) takes this shape: 64 output channels, the bf16 dz
    operand below 2 GiB and the LDS tile of one frequency row (F) within 64 KB;
    decided in the forward, which then skips the padded operand."""
    P = B * (T + 2) * (F + 2)
    lds = 256 * co * 2 + (256 + 2 * (F + 3)) * 4
    return co == 64 and P * co * 2 < _TWO_GIB and lds <= 64 * 1024


def conv3x3_tr(inp, P, cin, fp, sign, w, cout, bias, out):
    """out[p][n] = bias[n] + sum_tap sum_c inp[p + sign*shift(tap)][c] w[n][tap cin + c]
    on the tap-resident kernel (asr_conv3x3_tr); inp / w bf16, out f32 or bf16."""
    N.require_device(inp, w, out)
    od = BF16 if out.dtype == torch.bfloat16 else F32
    N.call('asr_conv3x3_tr', N.ptr(inp), int(P), int(cin), int(fp), int(sign), N.ptr(w),
           int(cout), N.ptr(bias), N.ptr(out), od, N.stream_handle(inp.device))


def conv3x3_tr_wgrad(x, dz, P, cin, fp, cout, packed):
    """packed[n][tap cin + c] = sum_p dz[p][n] x[p + shift(tap)][c] on the
    tap-resident weight-gradient kernel; False when the shape does not take it."""
    if compute_dtype() != BF16 or os.environ.get('ASR_VGG_TR', '1') == '0':
        return False
    if P * cin * 2 >= _TWO_GIB or P * cout * 2 >= _TWO_GIB:   # the kernel's buffer limit
        return False
    nb = N.query('asr_conv3x3_tr_wgrad_workspace_bytes', int(P), int(cin), int(cout), int(fp))
    if not nb:
        return False
    N.require_device(x, dz, packed)
    ws = _ws(nb, x.device)
    N.call('asr_conv3x3_tr_wgrad', N.ptr(x), N.ptr(dz), int(P), int(cin), int(fp), int(cout),
           N.ptr(packed), N.ptr(ws), nb, N.stream_handle(x.device))
    return True


class VGGFn(torch.autograd.Function):
    """The whole conv stack as one op.  Layer l input: zero-haloed channels-last
    [B][T_l+2][F_l+2][C_in] (compute dtype for GEMM layers, f32 for direct
    ones); conv output z_l f32 over the same padded pixels; the 3x3 conv of a
    layer with C_in, C_out multiples of 16 = ONE GEMM with tap-addressed
    operands (csrc/gemm.hip), other layers (C_in = 1) = asr_conv_direct_*;
    ReLU, pool, batch norm and dropout = asr_vgg_block_*.  Output
    [B, T', F'*C] f32."""

    @staticmethod
    def forward(ctx, xs, specs, training, p_drop, *params):
        N.require_device(xs)
        xs = xs.contiguous()
        dev = xs.device
        cd = compute_dtype()
        B, T, F = xs.shape
        f32 = dict(dtype=torch.float32, device=dev)
        opdt = torch.bfloat16 if cd == BF16 else torch.float32
        # GEMM layers need C_in and C_out multiples of 16; the single input
        # channel of layer 0 is padded to 16 (zero channels, zero weights)
        use_gemm = [sp['w'].shape[0] % 16 == 0 and (sp['w'].shape[1] % 16 == 0 or l == 0)
                    for l, sp in enumerate(specs)]
        cC = 1
        cCp = 16 if use_gemm[0] else 1
        # bf16, 64-channel first layer: its forward stencil and its weight gradient
        # (asr_conv3x3_c1_wgrad_xs) both read the raw features, so the padded
        # 16-channel operand is never built
        co0 = specs[0]['w'].shape[0]
        c1w = (cd == BF16 and use_gemm[0] and _c1_wgrad_ok(B, T, F, co0) and
               os.environ.get('ASR_VGG_C1_DIRECT', '1') != '0' and
               os.environ.get('ASR_VGG_C1_XS', '1') != '0' and
               os.environ.get('ASR_VGG_C1_WGRAD', '1') != '0')
        if c1w:
            x_op = xs
        else:
            x_op = torch.empty(B * (T + 2) * (F + 2), cCp, dtype=opdt if use_gemm[0] else
                               torch.float32, device=dev)
            N.call('asr_vgg_pad_input_ch', N.ptr(xs), B, T, F, cCp, cd if use_gemm[0] else F32,
                   N.ptr(x_op), N.stream_handle(dev))
        ctx.c1w = c1w
        cT, cF = T, F
        saved, layers = [], []
        L = len(specs)
        for l, sp in enumerate(specs):
            w = sp['w']
            Co = w.shape[0]
            npad = B * (cT + 2) * (cF + 2)
            # bf16 mode: the GEMM / stencil layers write the conv output as bf16
            # (read twice more: ReLU + pool, and the ReLU mask in the backward)
            c1_xs = (use_gemm[l] and cC == 1 and Co % 4 == 0 and 256 % (Co // 4) == 0 and
                     os.environ.get('ASR_VGG_C1_DIRECT', '1') != '0' and
                     os.environ.get('ASR_VGG_C1_XS', '1') != '0')
            z_bf = (cd == BF16 and Co % 4 == 0 and (c1_xs or not (cC == 1)) and use_gemm[l] and
                    os.environ.get('ASR_VGG_Z_BF16', '1') != '0')
            pt, pf, ceil = sp['pt'], sp['pf'], sp['ceil']
            # unpooled stencil layer followed by batch norm: the stencil writes P and
            # the BN moment partials itself (asr_vgg_c1_forward_relu_p), no z
            c1p = (c1_xs and z_bf and not pt and sp['gamma'] is not None and Co % 8 == 0 and
                   (not training or sp['run_mean'] is not None) and
                   os.environ.get('ASR_VGG_P_BF16', '1') != '0' and
                   os.environ.get('ASR_VGG_ROWS', '1') != '0' and
                   os.environ.get('ASR_VGG_C1_RELU_P', '1') != '0')
            z = (None if c1p else
                 torch.empty(npad, Co, dtype=torch.bfloat16 if z_bf else torch.float32, device=dev))
            if c1p:
                P = torch.empty(B * cT * cF, Co, dtype=torch.bfloat16, device=dev)
                nblk = N.query('asr_vgg_c1_relu_p_blocks', B, cT)
                mqp = torch.empty(2, nblk, Co, **f32) if training else None
                N.call('asr_vgg_c1_forward_relu_p', N.ptr(xs), int(cd == BF16), B, cT, cF, Co,
                       N.ptr(w), N.ptr(sp['b']), N.ptr(P),
                       N.ptr(sp['run_mean']) if training else None,
                       N.ptr(mqp[0]) if training else None, N.ptr(mqp[1]) if training else None,
                       N.stream_handle(dev))
            elif not use_gemm[l]:
                N.call('asr_conv_direct_forward', N.ptr(x_op), B, cT, cF, cC, Co, N.ptr(w),
                       N.ptr(sp['b']), N.ptr(z), N.stream_handle(dev))
            elif cC == 1 and Co % 4 == 0 and os.environ.get('ASR_VGG_C1_DIRECT', '1') != '0':
                # one input channel: a direct stencil from channel 0 of the padded
                # operand (the GEMM would run K = 144 for 9 useful taps); the
                # backward still takes the weight-gradient GEMM over this operand
                if c1_xs:
                    # from the raw features (contiguous rows; rounded to bf16 as the
                    # staged operand is in bf16 mode)
                    N.call('asr_conv3x3_c1_forward_xs', N.ptr(xs), int(cd == BF16), B, cT, cF, Co,
                           N.ptr(w), N.ptr(sp['b']), N.ptr(z), BF16 if z_bf else F32,
                           N.stream_handle(dev))
                else:
                    N.call('asr_conv3x3_c1_forward', N.ptr(x_op), cd, cCp, B, cT, cF, Co,
                           N.ptr(w), N.ptr(sp['b']), N.ptr(z), N.stream_handle(dev))
            else:
                wg = (torch.zeros if cCp != cC else torch.empty)(Co, 9 * cCp, dtype=opdt,
                                                                 device=dev)
                N.call('asr_conv_weight_pack_pad', N.ptr(w), Co, cC, cCp, 0, cd, N.ptr(wg),
                       N.stream_handle(dev))
                if _conv_tr_ok(cCp, Co, cF + 2, npad, z.element_size()):
                    # the input rows stay in an LDS ring across the nine taps
                    conv3x3_tr(x_op, npad, cCp, cF + 2, 1, wg, Co, sp['b'], z)
                else:
                    p = gemm_problem(_tap_operand(x_op, 0, cCp, cCp, cF + 2, 1),
                                     operand(wg, 0, rowmap(9 * cCp)), z, rowmap(Co), npad, Co,
                                     9 * cCp, bias=sp['b'])
                    run_gemm([p], dev)
            To, Fo = _pool_dims(cT, cF, pt, pf, ceil) if pt else (cT, cF)
            # P = max(0, max z) of a bf16 z is itself a bf16 value: stored bf16 it
            # is exact and halves P's write and four reads
            p_bf = z_bf and os.environ.get('ASR_VGG_P_BF16', '1') != '0'
            if not c1p:
                P = torch.empty(B * To * Fo, Co, dtype=torch.bfloat16 if p_bf else torch.float32,
                                device=dev)
            slot = torch.empty(B * To * Fo * Co, dtype=torch.uint8, device=dev) if pt else None
            bn = sp['gamma'] is not None
            mean = torch.empty(Co, **f32) if bn else None
            rstd = torch.empty(Co, **f32) if bn else None
            drop = float(p_drop) if training else 0.0
            seed = _next_seed() if drop > 0 else 0
            last = l == L - 1
            if last:
                out = torch.empty(B, To, Fo * Co, **f32)
                out_dt, flat = F32, 1
            else:
                nxt_dt = opdt if use_gemm[l + 1] else torch.float32
                if _halo_only(Co, nxt_dt):
                    # the block kernel writes every interior pixel: zero only the halo
                    out = torch.empty(B * (To + 2) * (Fo + 2), Co, dtype=nxt_dt, device=dev)
                    _zero_halo(out, B, To, Fo, Co)
                else:
                    out = torch.zeros(B * (To + 2) * (Fo + 2), Co, dtype=nxt_dt, device=dev)
                out_dt, flat = (cd if use_gemm[l + 1] else F32), 0
            nb = N.query('asr_vgg_block_workspace_bytes', B, To, Fo, Co)
            ws = _ws(nb, dev)
            if c1p:
                N.call('asr_vgg_block_forward_given_p', N.ptr(P), B, cT, cF, Co,
                       N.ptr(sp['gamma']), N.ptr(sp['beta']), N.ptr(sp['run_mean']),
                       N.ptr(sp['run_var']), int(bool(training)), float(sp['momentum']),
                       float(sp['eps']), N.ptr(mean), N.ptr(rstd), drop, seed, N.ptr(out),
                       out_dt, flat, N.ptr(mqp[0]) if training else None,
                       N.ptr(mqp[1]) if training else None, nblk if training else 0, N.ptr(ws),
                       nb, N.stream_handle(dev))
                z = P     # the backward masks from P (asr_vgg_block_backward_zdp: z == P)
            else:
                N.call('asr_vgg_block_forward_zp', N.ptr(z), BF16 if z_bf else F32, B, cT, cF,
                       Co, pt, pf, ceil, N.ptr(P), BF16 if p_bf else F32, N.ptr(slot),
                       N.ptr(sp['gamma']), N.ptr(sp['beta']), N.ptr(sp['run_mean']),
                       N.ptr(sp['run_var']), int(bool(training)), float(sp['momentum']),
                       float(sp['eps']), N.ptr(mean), N.ptr(rstd), drop, seed, N.ptr(out),
                       out_dt, flat, N.ptr(ws), nb, N.stream_handle(dev))
            saved += [x_op, z, P, slot, mean, rstd]
            layers.append((cT, cF, cC, cCp, Co, pt, pf, ceil, drop, seed, use_gemm[l]))
            x_op, cT, cF, cC, cCp = out, To, Fo, Co, Co
        ctx.save_for_backward(*[t if t is not None else torch.empty(0, device=dev)
                                for t in saved])
        ctx.layers = layers
        ctx.specs = specs
        ctx.B = B
        return x_op

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        specs, layers, B = ctx.specs, ctx.layers, ctx.B
        dev = dout.device
        cd = compute_dtype()
        f32 = dict(dtype=torch.float32, device=dev)
        opdt = torch.bfloat16 if cd == BF16 else torch.float32
        dnext, flat = dout.contiguous(), 1
        for l in range(len(layers) - 1, -1, -1):
            x_op, z, P, slot, mean, rstd = saved[6 * l:6 * l + 6]
            slot = slot if slot.numel() else None
            mean = mean if mean.numel() else None
            rstd = rstd if rstd.numel() else None
            cT, cF, cC, cCp, Co, pt, pf, ceil, drop, seed, gemm = layers[l]
            sp = specs[l]
            npad = B * (cT + 2) * (cF + 2)
            # dz is the GEMM operand (compute dtype) of GEMM layers; their conv
            # bias gradient is summed from the f32 values inside the kernel
            dz_f32 = not gemm
            if not dz_f32 and _halo_only(Co, opdt) and os.environ.get('ASR_VGG_POST_FULL',
                                                                   '1') != '0':
                # the full-resolution pass writes every interior pixel of dz
                dz = torch.empty(npad, Co, dtype=opdt, device=dev)
                _zero_halo(dz, B, cT, cF, Co)
            else:
                dz = torch.zeros(npad, Co, **f32) if dz_f32 else torch.zeros(npad, Co, dtype=opdt,
                                                                              device=dev)
            fused_bias = gemm and sp['b'] is not None
            To, Fo = _pool_dims(cT, cF, pt, pf, ceil) if pt else (cT, cF)
            nb = N.query('asr_vgg_block_workspace_bytes', B, To, Fo, Co)
            ws = _ws(nb, dev)
            bn = sp['gamma'] is not None
            N.call('asr_vgg_block_backward_zdp', N.ptr(dnext),
                   BF16 if dnext.dtype == torch.bfloat16 else F32, flat, N.ptr(z),
                   BF16 if z.dtype == torch.bfloat16 else F32, B, cT, cF, Co, pt,
                   pf, ceil, N.ptr(P), BF16 if P.dtype == torch.bfloat16 else F32, N.ptr(slot),
                   N.ptr(sp['gamma']), N.ptr(mean), N.ptr(rstd),
                   N.ptr(grad_buffer(sp['gamma']) if bn else None),
                   N.ptr(grad_buffer(sp['beta']) if bn else None), drop, seed, N.ptr(dz),
                   F32 if dz_f32 else cd,
                   N.ptr(grad_buffer(sp['b']) if fused_bias else None), N.ptr(ws), nb,
                   N.stream_handle(dev))
            w = sp['w']
            if not gemm:
                nb = N.query('asr_conv_direct_wgrad_workspace_bytes', B, cT, cF, cC, Co)
                ws = _ws(nb, dev)
                N.call('asr_conv_direct_wgrad', N.ptr(x_op), N.ptr(dz), B, cT, cF, cC, Co,
                       N.ptr(grad_buffer(w)),
                       N.ptr(grad_buffer(sp['b']) if sp['b'] is not None else None), N.ptr(ws),
                       nb, N.stream_handle(dev))
                if l == 0:
                    break
                dx = torch.empty(npad, cC, **f32)
                N.call('asr_conv_direct_dgrad', N.ptr(dz), B, cT, cF, cC, Co, N.ptr(w), N.ptr(dx),
                       N.stream_handle(dev))
                dnext, flat = dx, 0
                continue
            if (Co <= 64 and cd == BF16 and os.environ.get('ASR_VGG_DW_T', '0') == '1'
                    and not (l == 0 and ctx.c1w)):   # (there x_op is the raw features xs)
                # transposed image [9 Ci][Co] = X^T dz: C_out becomes the narrow N
                # of the 256 x 64 kernel (dz^T X puts C_out on half-empty 128-row
                # tiles).  Opt-in: measured 0.27 ms / step SLOWER at vgg_hier (the
                # K-major 256 x 64 tile needs 96 KB of LDS, one work-group per CU)
                packed_t = torch.empty(9 * cCp, Co, **f32)
                run_gemm([gemm_problem(_tap_operand(x_op, 1, cCp, cCp, cF + 2, 1),
                                       operand(dz, 1, rowmap(Co)), packed_t, rowmap(Co),
                                       9 * cCp, Co, npad)], dev, opts=N64_KMODE)
                N.call('asr_conv_weight_unpack_acc_pad_t', N.ptr(packed_t), Co, cC, cCp,
                       N.ptr(grad_buffer(w)), N.stream_handle(dev))
            else:
                # dW image [Co][9 Ci] = dz^T X (taps on the output index), K = padded pixels.
                # On a side stream (ASR_VGG_WGRAD_SIDE, default on): only the
                # optimizer reads it, so it runs beside this layer's input-gradient
                # convolution and the layer below's element-wise passes
                side = _vgg_wgrad_stream(dev)
                if side is not None:
                    main = torch.cuda.current_stream(dev)
                    side.wait_stream(main)
                with torch.cuda.stream(side) if side is not None else _nullctx():
                    packed = torch.empty(Co, 9 * cCp, **f32)
                    if l == 0 and ctx.c1w:   # x_op is the raw features xs
                        nb = N.query('asr_conv3x3_c1_wgrad_workspace_bytes', Co)
                        ws = _ws(nb, dev)
                        N.call('asr_conv3x3_c1_wgrad_xs', N.ptr(x_op), 1, B, cT, cF, Co, N.ptr(dz),
                               cCp, N.ptr(packed), N.ptr(ws), nb, N.stream_handle(dev))
                    elif not conv3x3_tr_wgrad(x_op, dz, npad, cCp, cF + 2, Co, packed):
                        run_gemm([gemm_problem(operand(dz, 1, rowmap(Co)),
                                               _tap_operand(x_op, 1, cCp, cCp, cF + 2, 1), packed,
                                               rowmap(9 * cCp), Co, 9 * cCp, npad)], dev)
                    N.call('asr_conv_weight_unpack_acc_pad', N.ptr(packed), Co, cC, cCp,
                           N.ptr(grad_buffer(w)), N.stream_handle(dev))
                if side is not None:
                    _defer_side_join(dev, side, main, (x_op, dz), (grad_buffer(w),))
            if l == 0:
                break
            # d input (padded rows of layer l's input) = dz (taps, mirrored) x W^T image
            wt = torch.empty(cC, 9 * Co, dtype=opdt, device=dev)
            N.call('asr_conv_weight_pack', N.ptr(w), Co, cC, 1, cd, N.ptr(wt),
                   N.stream_handle(dev))
            # bf16 mode: the input gradient goes to the layer below as bf16 when that
            # layer's pool / ReLU / BN backward reads it on its bf16 full-resolution
            # pass (half the bytes of the largest tensors of the VGG backward)
            lo = layers[l - 1]
            dx_bf = (cd == BF16 and lo[10] and cC % 4 == 0 and
                     saved[6 * (l - 1) + 1].dtype == torch.bfloat16 and
                     os.environ.get('ASR_VGG_POST_FULL', '1') != '0' and
                     os.environ.get('ASR_VGG_DX_BF16', '1') != '0')
            dx = torch.empty(npad, cC, dtype=torch.bfloat16 if dx_bf else torch.float32,
                             device=dev)
            if _conv_tr_ok(Co, cC, cF + 2, npad, dx.element_size()):
                conv3x3_tr(dz, npad, Co, cF + 2, -1, wt, cC, None, dx)
            else:
                run_gemm([gemm_problem(_tap_operand(dz, 0, Co, Co, cF + 2, -1),
                                       operand(wt, 0, rowmap(9 * Co)), dx, rowmap(cC), npad, cC,
                                       9 * Co)], dev)
            dnext, flat = dx, 0
        return (None, None, None, None) + (None,) * len(ctx.needs_input_grad[4:])


_vgg_side = {}


def _vgg_wgrad_stream(dev):
    """The stream the VGG convolutions' weight gradients run on, or None (the
    compute stream; ASR_VGG_WGRAD_SIDE=0)."""
    if os.environ.get('ASR_VGG_WGRAD_SIDE', '1') == '0':
        return None
    st = _vgg_side.get(dev.index)
    if st is None:
        st = _vgg_side[dev.index] = torch.cuda.Stream(device=dev)
    return st


class _nullctx(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


ACT_RELU, ACT_PRELU, ACT_HARDTANH = 0, 1, 2


def _spec_kernel(sp):
    """(kf, kt) of a layer spec: the Conv2d weight is [Co][Ci][kf][kt]."""
    return int(sp['w'].shape[2]), int(sp['w'].shape[3])


def _needs_taps(specs):
    """A net the 3x3 / ReLU kernels of VGGFn do not cover."""
    return any(_spec_kernel(sp) != (3, 3) or sp.get('act', ACT_RELU) != ACT_RELU for sp in specs)


def conv_taps_forward(x, B, T, F, cin, w_img, cout, kf, kt, bias, z, cd=None):
    """z interior = the kf x kt convolution of the haloed operand x (asr_conv_taps_forward)."""
    N.require_device(x, w_img, z)
    N.call('asr_conv_taps_forward', compute_dtype() if cd is None else cd, N.ptr(x), int(B), int(T),
           int(F), int(cin), N.ptr(w_img), int(cout), int(kf), int(kt), N.ptr(bias), N.ptr(z),
           N.stream_handle(x.device))


def conv_taps_dgrad(dz, B, T, F, cin, wt_img, cout, kf, kt, dx, cd=None):
    """dx interior [B][T+2][F+2][cin] from dz [B][To+2][Fo+2][cout] (asr_conv_taps_dgrad)."""
    N.require_device(dz, wt_img, dx)
    N.call('asr_conv_taps_dgrad', compute_dtype() if cd is None else cd, N.ptr(dz), int(B), int(T),
           int(F), int(cin), N.ptr(wt_img), int(cout), int(kf), int(kt), N.ptr(dx),
           N.stream_handle(dz.device))


def conv_taps_wgrad(x, dz, B, T, F, cin, cout, kf, kt, packed, cd=None):
    """packed [cout][kf kt cin] f32 = the weight-gradient image (asr_conv_taps_wgrad)."""
    N.require_device(x, dz, packed)
    cd = compute_dtype() if cd is None else cd
    nb = N.query('asr_conv_taps_wgrad_workspace_bytes', cd, int(B), int(T), int(F), int(cin),
                 int(cout), int(kf), int(kt))
    ws = _ws(nb, x.device)
    N.call('asr_conv_taps_wgrad', cd, N.ptr(x), N.ptr(dz), int(B), int(T), int(F), int(cin),
           int(cout), int(kf), int(kt), N.ptr(packed), N.ptr(ws), nb, N.stream_handle(x.device))


def conv_taps_weight_pack(w, cip, mode, cd=None):
    """The tap image of a Conv2d weight [Co][Ci][kf][kt] in the compute dtype: mode 0
    [Co][kf kt cip] (forward / weight gradient), mode 1 [Ci][kf kt Co] (input gradient)."""
    cd = compute_dtype() if cd is None else cd
    Co, Ci, kf, kt = w.shape
    dt = torch.bfloat16 if cd == BF16 else torch.float32
    out = (torch.empty(Co, kf * kt * cip, dtype=dt, device=w.device) if mode == 0 else
           torch.empty(Ci, kf * kt * Co, dtype=dt, device=w.device))
    N.call('asr_conv_taps_weight_pack', N.ptr(w), Co, Ci, int(cip), kf, kt, int(mode), cd,
           N.ptr(out), N.stream_handle(w.device))
    return out


class CNNTapsFn(torch.autograd.Function):
    """The conv stack of a CNNEncoder whose layers need kf x kt kernels
    (kf, kt in {3, 5}) or a PReLU / hard-tanh activation (the pure-CNN CTC
    recipe, encoders/cnn.py:61-122).  Layer l input: zero-haloed channels-last
    [B][T_l+2][F_l+2][C_in] in the compute dtype (the single input channel of
    layer 0 padded to 16 zero channels); convolution = asr_conv_taps_* writing
    the f32 conv output z over its own, smaller grid; activation, pool, batch
    norm and dropout = asr_cnn_act_*.  Output [B, T', F'*C] f32.  A shape the
    kernels do not take raises: there is no other path."""

    @staticmethod
    def forward(ctx, xs, specs, training, p_drop, *params):
        N.require_device(xs)
        xs = xs.contiguous()
        dev = xs.device
        cd = compute_dtype()
        B, T, F = xs.shape
        f32 = dict(dtype=torch.float32, device=dev)
        opdt = torch.bfloat16 if cd == BF16 else torch.float32
        cC, cCp = 1, 16
        x_op = torch.empty(B * (T + 2) * (F + 2), cCp, dtype=opdt, device=dev)
        N.call('asr_vgg_pad_input_ch', N.ptr(xs), B, T, F, cCp, cd, N.ptr(x_op),
               N.stream_handle(dev))
        cT, cF = T, F
        saved, layers = [], []
        L = len(specs)
        for l, sp in enumerate(specs):
            w = sp['w']
            Co = w.shape[0]
            kf, kt = _spec_kernel(sp)
            if N.query('asr_conv_taps_supported', cd, B, cT, cF, cCp, Co, kf, kt) != 1:
                raise N.NativeError(
                    'CNN layer %d (%d -> %d channels, kernel %dx%d, grid %dx%d): %s' %
                    (l, cC, Co, kf, kt, cT, cF,
                     N.lib().asr_last_error().decode(errors='replace')))
            zT, zF = cT + 3 - kt, cF + 3 - kf
            wg = conv_taps_weight_pack(w, cCp, 0)
            # the act pass reads only z's interior: no halo to clear
            z = torch.empty(B * (zT + 2) * (zF + 2), Co, **f32)
            conv_taps_forward(x_op, B, cT, cF, cCp, wg, Co, kf, kt, sp['b'], z)
            pt, pf, ceil = sp['pt'], sp['pf'], sp['ceil']
            To, Fo = _pool_dims(zT, zF, pt, pf, ceil) if pt else (zT, zF)
            if To < 1 or Fo < 1:
                raise N.NativeError('CNN layer %d: pool %dx%d leaves nothing of a %dx%d grid'
                                    % (l, pt, pf, zT, zF))
            P = torch.empty(B * To * Fo, Co, **f32)
            slot = torch.empty(B * To * Fo * Co, dtype=torch.uint8, device=dev) if pt else None
            bn = sp['gamma'] is not None
            mean = torch.empty(Co, **f32) if bn else None
            rstd = torch.empty(Co, **f32) if bn else None
            drop = float(p_drop) if training else 0.0
            seed = _next_seed() if drop > 0 else 0
            if l == L - 1:
                out = torch.empty(B, To, Fo * Co, **f32)
                out_dt, flat = F32, 1
            else:
                out = torch.empty(B * (To + 2) * (Fo + 2), Co, dtype=opdt, device=dev)
                if _halo_only(Co, opdt):
                    _zero_halo(out, B, To, Fo, Co)
                else:
                    out.zero_()
                out_dt, flat = cd, 0
            nb = N.query('asr_cnn_act_workspace_bytes', B, zT, zF, Co)
            ws = _ws(nb, dev)
            act = sp.get('act', ACT_RELU)
            N.call('asr_cnn_act_forward', N.ptr(z), B, zT, zF, Co, act, N.ptr(sp.get('slope')),
                   pt, pf, ceil, N.ptr(P), N.ptr(slot), N.ptr(sp['gamma']), N.ptr(sp['beta']),
                   N.ptr(sp['run_mean']), N.ptr(sp['run_var']), int(bool(training)),
                   float(sp['momentum']), float(sp['eps']), N.ptr(mean), N.ptr(rstd), drop, seed,
                   N.ptr(out), out_dt, flat, N.ptr(ws), nb, N.stream_handle(dev))
            saved += [x_op, z, P, slot, mean, rstd]
            layers.append((cT, cF, cC, cCp, Co, kf, kt, pt, pf, ceil, drop, seed))
            x_op, cT, cF, cC, cCp = out, To, Fo, Co, Co
        ctx.save_for_backward(*[t if t is not None else torch.empty(0, device=dev)
                                for t in saved])
        ctx.layers = layers
        ctx.specs = specs
        ctx.B = B
        ctx.training = bool(training)
        ctx.cd = cd
        return x_op

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        specs, layers, B, cd = ctx.specs, ctx.layers, ctx.B, ctx.cd
        dev = dout.device
        f32 = dict(dtype=torch.float32, device=dev)
        opdt = torch.bfloat16 if cd == BF16 else torch.float32
        dnext, flat = dout.contiguous(), 1
        for l in range(len(layers) - 1, -1, -1):
            x_op, z, P, slot, mean, rstd = saved[6 * l:6 * l + 6]
            slot = slot if slot.numel() else None
            mean = mean if mean.numel() else None
            rstd = rstd if rstd.numel() else None
            cT, cF, cC, cCp, Co, kf, kt, pt, pf, ceil, drop, seed = layers[l]
            sp = specs[l]
            zT, zF = cT + 3 - kt, cF + 3 - kf
            # dz: the convolutions' operand (compute dtype); the act pass writes its
            # whole interior
            dz = torch.empty(B * (zT + 2) * (zF + 2), Co, dtype=opdt, device=dev)
            if _halo_only(Co, opdt):
                _zero_halo(dz, B, zT, zF, Co)
            else:
                dz.zero_()
            bn = sp['gamma'] is not None
            act = sp.get('act', ACT_RELU)
            slope = sp.get('slope')
            nb = N.query('asr_cnn_act_workspace_bytes', B, zT, zF, Co)
            ws = _ws(nb, dev)
            N.call('asr_cnn_act_backward', N.ptr(dnext), flat, N.ptr(z), B, zT, zF, Co, act,
                   N.ptr(slope), pt, pf, ceil, N.ptr(P), N.ptr(slot), N.ptr(sp['gamma']),
                   N.ptr(mean), N.ptr(rstd), int(ctx.training),
                   N.ptr(grad_buffer(sp['gamma']) if bn else None),
                   N.ptr(grad_buffer(sp['beta']) if bn else None), drop, seed, N.ptr(dz), cd,
                   N.ptr(grad_buffer(sp['b']) if sp['b'] is not None else None),
                   N.ptr(grad_buffer(slope) if slope is not None else None), N.ptr(ws), nb,
                   N.stream_handle(dev))
            w = sp['w']
            packed = torch.empty(Co, kf * kt * cCp, **f32)
            conv_taps_wgrad(x_op, dz, B, cT, cF, cCp, Co, kf, kt, packed, cd)
            N.call('asr_conv_taps_weight_unpack_acc', N.ptr(packed), Co, cC, cCp, kf, kt,
                   N.ptr(grad_buffer(w)), N.stream_handle(dev))
            if l == 0:
                break
            wt = conv_taps_weight_pack(w, cC, 1, cd)
            dx = torch.empty(B * (cT + 2) * (cF + 2), cC, **f32)   # interior read only
            conv_taps_dgrad(dz, B, cT, cF, cC, wt, Co, kf, kt, dx, cd)
            dnext, flat = dx, 0
        return (None, None, None, None) + (None,) * len(ctx.needs_input_grad[4:])


def vgg_front(xs, specs, training, p_drop):
    params = [t for sp in specs for t in (sp['w'], sp['b'], sp['gamma'], sp['beta'])
              if t is not None]
    if _needs_taps(specs):
        params += [sp['slope'] for sp in specs if sp.get('slope') is not None]
        return CNNTapsFn.apply(xs, specs, training, p_drop, *params)
    return VGGFn.apply(xs, specs, training, p_drop, *params)
