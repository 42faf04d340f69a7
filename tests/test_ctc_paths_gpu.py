"""The CTC forward (ctc_prep, ctc_emit / ctc_emit_wide or ctc_lse_from_parts +
ctc_emit_gather, the lattice's cost, ctc_loss_reduce) and its float32 gradient
(ctc_grad<true> at V <= 256, ctc_grad<false> above) against the float64
reference and bounds of tests/ctc_paths_ref.py, through the C entry points
asr_ctc_forward / asr_ctc_forward_lse / asr_ctc_backward / asr_ctc_fwd_bwd:

    widths    V 2 3 5 64 255 256 | 257 773 1023 1024 | 1025 3077 4099 (dense)
    layouts   b time-major; c logits of pitch V rounded up to 4, dense gradient
              (rows whose logits and gradient differ in 16-B phase: ctc_grad's
              scalar path); d dense logits, gradient of pitch V + 3 -- at V 5,
              257, 1025, 3077.  Logit padding columns and every frame t >=
              act_lens[b] hold NaN; the gradient buffer is prefilled with a
              sentinel that must survive in the padding, and rows t >= act_lens
              must come back exactly 0
    blank     0, V - 1, V // 2 at V 5 and 1025, asr_ctc_backward and _fwd_bwd
    scaling   grad_scale NULL / a device scalar, scale 1/3 / 1
    shift     logits + 80 / - 80 at V 257 and 1025
    order     ASR_CTC_ORDER 0..3 at V 1025: bitwise equal
    partials  asr_ctc_forward_lse on host-built slab partials at V 64, 1024,
              1025, 2051 and with one slab all -inf; a wrong nslab refused
    B 300     ctc_prep's and ctc_loss_reduce's loops beyond one block
    infeasible  an utterance between two feasible ones, both zero_infinity
    masked    -inf logits over one thread's first quads / first unrolled round

asr_ctc_last_path names the normaliser (0 the emission pass, 1 the partials) and
the gradient kernel family (0: f32) of every run; every gradient runs twice and
is compared bit for bit.  Each run prints its worst |error| / bound.

Findings on an MI355X:
  * every run above: worst cost error 0.24 of its bound (V 2051 from partials),
    worst gradient error 0.14 of its bound; nothing needed a wider margin.
  * masked classes: before lse_acc4 / lse_acc1 / ctc_emit_wide's unrolled round
    guarded a running max of -inf, a thread whose first values were all -inf
    held exp(-inf - -inf) = NaN in its sum; where it later met a finite value
    the row's log-sum-exp was NaN, the lattice's fmax chain dropped the NaN
    emissions, log P came out -inf and the utterance was treated as infeasible:
    both masked cases returned cost 0 and an all-zero gradient for every
    utterance, silently (errors of 7e5 and 3e3 bounds).  With the guard they
    are finite and within 0.07 of the bounds.
  * ctc_grad<true>'s LDS atomicAdd sums: two runs were bitwise equal in every
    table-width run here (V 2 .. 256, blank 0 / middle / last, B 300).  With
    S <= 64 states each lane issues one atomicAdd, so a class's terms come from
    one DS instruction of one wave; nothing was changed.
"""
import ctypes

import numpy as np
import pytest
import torch

import ctc_paths_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e8)
ASR_ERR_ARG = -1
LOSS_SCALE = 1.0 / 3.0
GRAD_SCALE = 2.0


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


def _last_path():
    path = (ctypes.c_int * 2)()
    _N().call('asr_ctc_last_path', ctypes.cast(path, ctypes.c_void_p))
    return path[0], path[1]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _alloc(shape, fill, dev):
    return torch.full(shape, float(fill), dtype=torch.float32, device=dev)


def _layout(c, layout, dev):
    """(logits buffer, its [B, T, V] view, (stride_t, stride_b), gradient buffer,
    its [B, T, V] view, (gstride_t, gstride_b)).  Logits: NaN outside the live
    values; gradient: the sentinel everywhere."""
    B, T, V = c['B'], c['T'], c['V']
    if layout == 'b':                                   # time-major
        x = _alloc((T, B, V), np.nan, dev)
        g = _alloc((T, B, V), SENTINEL, dev)
        xv, gv = x.permute(1, 0, 2), g.permute(1, 0, 2)
        sx = sg = (B * V, V)
    else:
        P = V if layout in ('a', 'd') else (V + 3) // 4 * 4
        G = V + 3 if layout == 'd' else V
        assert layout in ('a', 'c', 'd') and (layout != 'c' or P > V)
        x = _alloc((B, T, P), np.nan, dev)
        g = _alloc((B, T, G), SENTINEL, dev)
        xv, gv = x[:, :, :V], g[:, :, :V]
        sx, sg = (P, T * P), (G, T * G)
    xv.copy_(torch.from_numpy(c['logits'].copy()))
    for b in range(B):
        xv[b, int(c['act_lens'][b]):] = float('nan')
    return x, xv, sx, g, gv, sg


def _run(c, dev, layout='a', api='backward', scale=LOSS_SCALE, grad_scale=GRAD_SCALE,
         zero_infinity=1, partials=False):
    """One forward (+ loss) and gradient.  api 'backward': asr_ctc_forward (or
    _forward_lse on the host-built partials) then asr_ctc_backward with scale
    and grad_scale (None: a NULL pointer); 'fwd_bwd': asr_ctc_fwd_bwd (scale 1,
    the gradient in the logits' layout)."""
    N = _N()
    B, T, V = c['B'], c['T'], c['V']
    x, xv, (st, sb), g, gv, (gst, gsb) = _layout(c, layout, dev)
    lab = torch.from_numpy(c['labels']).to(dev) if len(c['labels']) else \
        torch.zeros(1, dtype=torch.int32, device=dev)
    ll = torch.from_numpy(c['label_lens']).to(dev)
    al = torch.from_numpy(c['act_lens']).to(dev)
    mll, blank = int(c['max_label_len']), int(c['blank'])
    nbytes = N.query('asr_ctc_workspace_bytes', T, B, V, mll)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    costs = _alloc((B,), SENTINEL, dev)
    loss = _alloc((1,), SENTINEL, dev)
    stream = N.stream_handle(dev)
    tail = (N.ptr(lab), N.ptr(ll), N.ptr(al), mll, blank)
    if api == 'fwd_bwd':
        assert (gst, gsb) == (st, sb) and not partials
        N.call('asr_ctc_fwd_bwd', N.ptr(x), st, sb, T, B, V, *tail, zero_infinity, N.ptr(costs),
               N.ptr(g), N.ptr(ws), nbytes, stream)
        total = 1.0
    else:
        out = (zero_infinity, N.ptr(costs), N.ptr(loss), float(scale), N.ptr(ws), nbytes, stream)
        if partials:
            part = torch.from_numpy(R.slab_partials(c)).to(dev)
            N.call('asr_ctc_forward_lse', N.ptr(x), st, sb, T, B, V, N.ptr(part), part.shape[0],
                   *tail, *out)
        else:
            N.call('asr_ctc_forward', N.ptr(x), st, sb, T, B, V, *tail, *out)
        gs = None if grad_scale is None else _alloc((1,), grad_scale, dev)
        N.call('asr_ctc_backward', N.ptr(x), st, sb, T, B, V, *tail, N.ptr(gs), float(scale),
               N.ptr(g), gst, gsb, N.ptr(ws), nbytes, stream)
        total = float(np.float32(scale)) * (1.0 if grad_scale is None else grad_scale)
    path = _last_path()
    torch.cuda.synchronize()
    assert path == (1 if partials else 0, 0), path        # the normaliser named; the f32 gradient
    gfull = g.cpu().numpy()
    pad = gfull[:, :, V:] if layout == 'd' else gfull[:, :, :0]
    return dict(costs=costs.cpu().numpy(), loss=float(loss.item()), grad=gv.cpu().numpy(),
                pad=pad, total=total, scale=scale, api=api)


def _check(c, out, what, fails, zero_infinity=1):
    """One run against the reference: prints the worst |error| / bound of costs
    and gradient and appends to fails where one exceeds 1."""
    B, f = c['B'], c['feasible']
    costs64 = R.costs_ref(c)
    tol_g, tol_c = R.bound(c, scale=out['total'])
    ref_g = R.grad_ref(c) * out['total']
    costs, grad = out['costs'].astype(np.float64), out['grad'].astype(np.float64)
    assert np.all(_bits(out['pad']) == _bits(SENTINEL)), what       # padding untouched
    assert np.all(np.isfinite(grad)), (what, int((~np.isfinite(grad)).sum()))
    assert np.all(np.isfinite(costs[f])), (what, costs)
    for b in range(B):
        assert not grad[b, int(c['act_lens'][b]):].any(), (what, b)   # dead rows exactly 0
        if not f[b]:                                                   # the documented contract
            assert not grad[b].any(), (what, b)
            assert costs[b] == (0.0 if zero_infinity else np.inf), (what, costs[b])
    r_c = float(np.max(np.abs(costs - costs64)[f] / tol_c[f]))
    r_g = float(np.max(np.abs(grad - ref_g) / tol_g))
    print('  %-40s cost err/bound %.3f (max err %.2e)  grad err/bound %.3f (max err %.2e)' % (
        what, r_c, float(np.max(np.abs(costs - costs64)[f])), r_g,
        float(np.max(np.abs(grad - ref_g)))))
    if not r_c <= 1.0:
        fails.append((what, 'costs', r_c))
    if not r_g <= 1.0:
        fails.append((what, 'grad', r_g))
    if out['api'] == 'backward' and f.all():
        # ctc_loss_reduce: the float64 sum of the costs it read, and the reference's
        s32 = float(np.float32(out['scale']))
        tol_s = R.sum_bound(out['costs'], s32)
        assert abs(out['loss'] - s32 * costs.sum()) <= tol_s, (what, out['loss'])
        assert abs(out['loss'] - s32 * costs64.sum()) <= tol_s + s32 * tol_c.sum(), (what, out['loss'])


def _same(a, b, what):
    assert np.array_equal(_bits(a['grad']), _bits(b['grad'])), what
    assert np.array_equal(_bits(a['costs']), _bits(b['costs'])), what
    assert np.array_equal(_bits([a['loss']]), _bits([b['loss']])), what


def _twice(c, dev, what, **kw):
    """The run twice, bit for bit; checked against the reference."""
    a = _run(c, dev, **kw)
    b = _run(c, dev, **kw)
    fails = []
    _check(c, a, what, fails, kw.get('zero_infinity', 1))
    _same(a, b, what)
    assert not fails, fails
    return a


@pytest.mark.parametrize('V', R.TABLE_WIDTHS)
def test_narrow_emit_table_grad(V, cuda_dev):
    """ctc_emit + ctc_grad<true>: min(head_elems, V) at V 2 / 3, no quad, one
    partial quad round, the one-wave table's last widths."""
    print()
    _twice(R.case(V), cuda_dev, 'V%d dense' % V)


@pytest.mark.parametrize('V', R.COMPACT_WIDTHS)
def test_narrow_emit_compact_grad(V, cuda_dev):
    """ctc_emit + ctc_grad<false>: the first compact width; the 4x-unrolled
    quad loop not entered (257) and entered (773 and up); the last narrow width."""
    print()
    _twice(R.case(V), cuda_dev, 'V%d dense' % V)


@pytest.mark.parametrize('V', R.WIDE_WIDTHS)
def test_wide_emit(V, cuda_dev):
    """ctc_emit_wide (four waves through LDS): the first wide width; the
    unrolled 1024-quad round entered (3077: some threads; 4099: all, plus both
    tails) -- and ctc_grad<false>'s unrolled store loop."""
    print()
    _twice(R.case(V), cuda_dev, 'V%d dense' % V)


@pytest.mark.parametrize('layout', ['b', 'c', 'd'])
@pytest.mark.parametrize('V', R.LAYOUT_WIDTHS)
def test_layouts(V, layout, cuda_dev):
    """Time-major, padded logits against a dense gradient, a padded gradient:
    NaN in every logit that must not be read, the sentinel in every gradient
    float that must not be written."""
    print()
    c = R.case(V)
    a = _twice(c, cuda_dev, 'V%d layout %s' % (V, layout), layout=layout)
    if layout == 'd':
        assert a['pad'].shape == (c['B'], c['T'], 3)
    if layout == 'b':
        _twice(c, cuda_dev, 'V%d layout b fwd_bwd' % V, layout='b', api='fwd_bwd')


@pytest.mark.parametrize('api', ['backward', 'fwd_bwd'])
@pytest.mark.parametrize('c', R.blank_cases(), ids=lambda c: c['id'])
def test_blank_index(c, api, cuda_dev):
    print()
    _twice(c, cuda_dev, '%s %s' % (c['id'], api), api=api)


@pytest.mark.parametrize('scale,grad_scale', [(LOSS_SCALE, None), (1.0, GRAD_SCALE), (1.0, None)],
                         ids=['third_null', 'one_scalar', 'one_null'])
@pytest.mark.parametrize('V', [5, 257])
def test_scaling(V, scale, grad_scale, cuda_dev):
    """grad_scale NULL / a device scalar, scale 1/3 / 1, on both gradient
    kernels ((1/3, scalar) is every other test's setting)."""
    print()
    _twice(R.case(V), cuda_dev, 'V%d scale %.3f x %s' % (V, scale, grad_scale), scale=scale,
           grad_scale=grad_scale)


@pytest.mark.parametrize('c', R.shift_cases(), ids=lambda c: c['id'])
def test_shifted_logits(c, cuda_dev):
    print()
    _twice(c, cuda_dev, c['id'])


def test_row_order_switch_is_bitwise_neutral(cuda_dev, monkeypatch):
    """ASR_CTC_ORDER bit 0: ctc_emit_wide, bit 1: ctc_grad over descending rows."""
    print()
    c = R.case(1025)
    outs = []
    for order in range(4):
        monkeypatch.setenv('ASR_CTC_ORDER', str(order))
        outs.append(_twice(c, cuda_dev, 'V1025 ASR_CTC_ORDER=%d' % order))
    for o in outs[1:]:
        _same(outs[0], o, 'order')


@pytest.mark.parametrize('c', R.lse_cases(), ids=lambda c: c['id'])
def test_forward_from_slab_partials(c, cuda_dev):
    """ctc_lse_from_parts (one, exactly 16, 17 and 33 slabs; an empty slab) +
    ctc_emit_gather, on (max, sum exp) partials built on the host in float64."""
    print()
    _twice(c, cuda_dev, '%s partials' % c['id'], partials=True)


def test_forward_lse_refuses_a_wrong_slab_count(cuda_dev):
    N = _N()
    c = R.case(1025)
    B, T, V = c['B'], c['T'], c['V']
    before = _run(c, cuda_dev)           # (leaves the path record at (0, 0))
    x, _, (st, sb), _, _, _ = _layout(c, 'a', cuda_dev)
    part = torch.from_numpy(R.slab_partials(c)).to(cuda_dev)
    lab, ll, al = (torch.from_numpy(c[k]).to(cuda_dev) for k in ('labels', 'label_lens', 'act_lens'))
    nbytes = N.query('asr_ctc_workspace_bytes', T, B, V, 5)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cuda_dev)
    costs = _alloc((B,), SENTINEL, cuda_dev)
    for nslab in (16, 18):
        with pytest.raises(N.NativeError) as ei:
            N.call('asr_ctc_forward_lse', N.ptr(x), st, sb, T, B, V, N.ptr(part), nslab, N.ptr(lab),
                   N.ptr(ll), N.ptr(al), 5, 0, 1, N.ptr(costs), None, 1.0, N.ptr(ws), nbytes,
                   N.stream_handle(cuda_dev))
        assert 'rc=%d' % ASR_ERR_ARG in str(ei.value) and 'slabs' in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert _last_path() == (0, 0)                                  # nothing ran from partials
    assert np.all(_bits(costs.cpu().numpy()) == _bits(SENTINEL))   # nothing launched
    assert not ws.any().item()
    assert np.all(np.isfinite(before['costs']))


def test_batch_of_300(cuda_dev):
    """B 300 x T 3, V 5, label lengths 0 / 1 / 2 (309 labels): ctc_prep's
    offsets and label check and ctc_loss_reduce's sum beyond 256 utterances;
    _check holds loss_out to the float64 sum within gamma_B x sum |cost|."""
    print()
    c = R.batch300_case()
    assert c['B'] == 300 and c['max_label_len'] == 2
    _twice(c, cuda_dev, c['id'])
    _twice(c, cuda_dev, c['id'] + ' time-major', layout='b')


@pytest.mark.parametrize('zero_infinity', [0, 1])
@pytest.mark.parametrize('c', R.infeasible_cases(), ids=lambda c: c['id'])
def test_infeasible_utterance_between_feasible_ones(c, zero_infinity, cuda_dev):
    """include/asr_hip.h: cost 0 with zero_infinity, +inf without; gradient 0
    either way; the neighbours unaffected."""
    print()
    a = _twice(c, cuda_dev, '%s zero_infinity=%d' % (c['id'], zero_infinity),
               zero_infinity=zero_infinity)
    s32 = float(np.float32(LOSS_SCALE))
    if zero_infinity:
        assert abs(a['loss'] - s32 * a['costs'].astype(np.float64).sum()) <= R.sum_bound(a['costs'], s32)
    else:
        assert a['loss'] == np.inf
    _twice(c, cuda_dev, '%s fwd_bwd zero_infinity=%d' % (c['id'], zero_infinity), api='fwd_bwd',
           zero_infinity=zero_infinity)


@pytest.mark.parametrize('layout', ['a', 'b'])
@pytest.mark.parametrize('c', R.mask_cases(), ids=lambda c: c['id'])
def test_masked_classes(c, layout, cuda_dev):
    """-inf logits on non-label classes covering the first quads (V 257) / the
    whole first unrolled round (V 4099) of a row's first threads, at every row
    phase (V odd): costs and gradient finite and within bound, the gradient
    exactly 0 on the masked columns."""
    print()
    a = _twice(c, cuda_dev, '%s layout %s' % (c['id'], layout), layout=layout)
    assert not a['grad'][:, :, c['mask_cols']].any()
