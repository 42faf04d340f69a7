"""native_ops.lstm_layer (the unidirectional LSTM layer: csrc/lstm_uni.hip's
per-step recurrence and the layer GEMMs) against the float64 reference
tests/lstm_uni_ref.py, in both compute types, on lstm_uni_ref.CASES: the
smallest width, widths that are no multiple of a kernel's unit tile (scalar and
vector fragment loads), batch sizes of 1 and one short of / one past the
forward's and the backward's row tile, T = 1, lens [7, 4, 1], a non-identity
perm, Din = 9, t_mul = 2 / t_add = 1, concat, input dropout, and garbage in x
and dy at padded frames.

Every row: a cotangent at every frame (padded ones included), the four gradient
buffers filled with random values on entry (compared: grad - fill), y exactly
zero at padded frames, dx exactly zero at padded and unmapped source frames,
db_ih == db_hh bitwise, and per tensor max |got - f64| / max |f64| <= MARGIN x
the error of evaluating the same reference in float32 (fp32 mode), or x the
larger of that and of its bf16-emulated evaluation (bf16 mode).  err/bound is
printed per tensor.  Also: dy = NULL at the C ABI, a refused shape, and two
runs that agree bit for bit."""
import numpy as np
import pytest
import torch

import lstm_uni_ref as U
import rnn_layer_ref as R
from test_rnn_layer_gpu import _compare

pytestmark = pytest.mark.gpu

PARAMS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')
GRADS = dict(zip(PARAMS, U.OUT_KEYS[2:]))


def _params(inp, ref, dev, gen):
    """Device parameters, their .grad filled with U(+-1/4 of the reference
    gradient's largest value) -- one fill for both bias gradients, which must
    then stay equal bit for bit -- and the fills."""
    ps, fills = [], {}
    for k in PARAMS:
        p = inp[k].to(dev).requires_grad_(True)
        scale = 0.25 * float(np.abs(ref[GRADS[k]]).max())
        fill = ((torch.rand(p.shape, generator=gen) * 2 - 1) * scale).to(dev)
        if k == 'b_hh':
            fill = fills['db_ih']
        p.grad = fill.clone()
        ps.append(p)
        fills[GRADS[k]] = fill
    return ps, fills


def _run(case, precision, dev, seed):
    """One forward + backward of a case: (y, x.grad, params, fills)."""
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    c = U.CASES[case]
    inp, ref = U.case_inputs(case), U.reference(case)
    gen = torch.Generator().manual_seed(seed)
    ps, fills = _params(inp, ref, dev, gen)
    x = inp['x'].to(dev).requires_grad_(True)
    lens = torch.from_numpy(inp['lens']).to(dev)
    perm = None if inp['perm'] is None else torch.from_numpy(inp['perm']).to(dev)
    ops.set_compute_dtype(precision)
    try:
        y = ops.lstm_layer(x, lens, c['T'], *ps, perm=perm, t_mul=c['t_mul'], t_add=c['t_add'],
                           concat=c['concat'], drop=U.drop_of(c))
        y.backward(inp['dy'].to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype('fp32')
    return y, x.grad, ps, fills


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', sorted(U.CASES))
def test_layer_pass_matches_f64(case, precision, cuda_dev):
    c = U.CASES[case]
    inp, ref = U.case_inputs(case), U.reference(case)
    tag = case + '-' + precision
    y, dx, ps, fills = _run(case, precision, cuda_dev, len(tag))
    assert tuple(y.shape) == (c['B'], c['T'], c['H'])
    got = dict(y=y, dx=dx)
    got.update({GRADS[k]: p.grad - fills[GRADS[k]] for k, p in zip(PARAMS, ps)})
    assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
    bad = _compare(tag, got, ref, U.bounds(case, precision))
    assert not bad, (tag, bad)

    yh, dxh = y.detach().cpu().numpy(), dx.cpu().numpy()
    for b, n in enumerate(inp['lens']):
        assert not yh[b, n:].any(), ('y at padded frames of utterance', b)
    pm = np.arange(c['B']) if inp['perm'] is None else inp['perm']
    live = R.mapped_mask(dxh.shape, inp['lens'], pm, c['t_mul'], c['t_add'], c['T'], c['concat'])
    assert not dxh[~live].any(), 'dx at padded or unmapped source frames'
    assert torch.equal(ps[2].grad, ps[3].grad), 'db_ih != db_hh'


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_two_runs_agree_bit_for_bit(precision, cuda_dev):
    case = 'h24_b17'
    a, b = (_run(case, precision, cuda_dev, 5) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for p, q in zip(a[2], b[2]):
        assert torch.equal(p.grad, q.grad)


def _abi(dev, B, T, H, cd, dy):
    """asr_lstm_uni_forward + _backward on random gates: (rc_f, rc_b, dG, db)."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    g = torch.Generator().manual_seed(B * 1000 + H)
    gx = torch.randn(B, T, 4 * H, generator=g).to(dev)
    whh = (torch.rand(4 * H, H, generator=g) * 0.6 - 0.3).to(dev)
    lens = torch.from_numpy(R.make_lens(B, T)).to(dev)
    y = torch.full((B, T, H), 7.0, device=dev)
    cst = torch.full((B, T, H), 7.0, device=dev)
    db = torch.zeros(2, 4 * H, device=dev)
    nf = max(int(N.query('asr_lstm_uni_workspace_bytes', B, H, cd, 0)), 256)
    nb = max(int(N.query('asr_lstm_uni_workspace_bytes', B, H, cd, 1)), 256)
    ws = torch.empty(max(nf, nb), dtype=torch.uint8, device=dev)
    s = N.stream_handle(dev)
    rc_f = N.query('asr_lstm_uni_forward', N.ptr(gx), N.ptr(whh), N.ASR_DT_F32, N.ptr(lens), B, T, H,
                   cd, N.ptr(y), N.ptr(cst), None, N.ptr(ws), nf, s)
    rc_b = N.query('asr_lstm_uni_backward', N.ptr(dy), N.ptr(whh), N.ASR_DT_F32, N.ptr(lens), B, T, H,
                   cd, N.ptr(gx), N.ptr(cst), None, N.ptr(db[0]), N.ptr(db[1]), N.ptr(ws), nb, s)
    torch.cuda.synchronize()
    return rc_f, rc_b, gx, db, y


@pytest.mark.parametrize('cd', [0, 1], ids=['fp32', 'bf16'])
def test_null_dy_is_a_zero_cotangent(cd, cuda_dev):
    rc_f, rc_b, dg, db, y = _abi(cuda_dev, 5, 7, 24, cd, None)
    assert rc_f == 0 and rc_b == 0
    assert y.abs().max() > 0 and not (y == 7.0).any()
    assert not dg.any() and not db.any()


def test_a_shape_outside_the_accepted_set_is_refused_before_any_launch(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    H = 1032                       # above the widest accepted H
    assert N.query('asr_lstm_uni_shape_ok', 3, 2, H) == 0
    assert N.query('asr_lstm_uni_shape_ok', 3, 2, 1024) == 1
    rc_f, rc_b, gx, db, y = _abi(cuda_dev, 3, 2, H, 0, None)
    assert rc_f == N.ASR_ERR_UNSUPPORTED and rc_b == N.ASR_ERR_UNSUPPORTED
    assert bool((y == 7.0).all()) and not db.any()      # nothing was written
    x = torch.zeros(3, 2, 9, device=cuda_dev)
    lens = torch.tensor([2, 2, 1], dtype=torch.int32, device=cuda_dev)
    w = [torch.zeros(4 * H, 9, device=cuda_dev), torch.zeros(4 * H, H, device=cuda_dev),
         torch.zeros(4 * H, device=cuda_dev), torch.zeros(4 * H, device=cuda_dev)]
    with pytest.raises(N.NativeError, match='refused'):
        ops.lstm_layer(x, lens, 2, *w)
