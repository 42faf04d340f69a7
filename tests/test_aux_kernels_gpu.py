"""The auxiliary HIP kernels (losses, decoding, embedding, cells, elementwise,
column sums, optimizer) one by one against float64 references (aux_refs.py),
at the sizes where their wave strides, row tails, chunk carries, unrolls and
grid-stride loops change path.

Tolerances:
* selections and copies (embedding forward, argmax, best path, add, bf16
  shadow, guard) are exact;
* pure sums use |err| <= gamma_n sum |x_i| per output element;
* what contains exp / log / tanh / a division gets 16 x the error of a float32
  CPU evaluation of the same formula on the same inputs (the constants below;
  tests/test_aux_refs_cpu.py recomputes them).
"""
import ctypes

import numpy as np
import pytest
import torch

import aux_refs as R
from oracle import ctc_ref

pytestmark = pytest.mark.gpu

# max |float32 CPU evaluation - float64 reference| over the inputs of this file
# (aux_refs.measure_f32_errors()), in the unit named; a kernel may be 16 x off.
F32_XENT_LOSS = 1.17e-7    # |loss| error / sum of the magnitudes of the loss's terms
F32_XENT_DX = 8.59e-8      # |dx| error / (|g| (|ce_scale| + |ls_scale|))
F32_SOFTMAX_REL = 2.30e-7  # relative error of a softmax entry
F32_LSTM_FWD = 2.69e-7     # absolute, over h, c, act
F32_LSTM_BWD = 3.87e-7     # absolute, over dpre, dc_prev
F32_GRU_FWD = 2.25e-7      # absolute, over hout, act
F32_GRU_BWD = 2.11e-7      # absolute, over dgi, dgh, dh_prev
F32_TANH_FWD = 5.61e-8     # absolute (tanh and add_tanh)
F32_TANH_BWD = 3.54e-7     # absolute, dx = dy (1 - y^2)
F32_OPTIM_P = 6.96e-7      # absolute, parameters after steps 1..3
F32_OPTIM_M = 4.00e-7      # absolute, first moment / momentum buffer
F32_OPTIM_V = 1.48e-9      # absolute, Adam second moment
MARGIN = 16.0

F32_REF_ERR = dict(XENT_LOSS=F32_XENT_LOSS, XENT_DX=F32_XENT_DX, SOFTMAX_REL=F32_SOFTMAX_REL,
                   LSTM_FWD=F32_LSTM_FWD, LSTM_BWD=F32_LSTM_BWD, GRU_FWD=F32_GRU_FWD,
                   GRU_BWD=F32_GRU_BWD, TANH_FWD=F32_TANH_FWD, TANH_BWD=F32_TANH_BWD,
                   OPTIM_P=F32_OPTIM_P, OPTIM_M=F32_OPTIM_M, OPTIM_V=F32_OPTIM_V)


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


def _d(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _h(t):
    return t.detach().cpu().numpy()


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bad = err > tol
    assert not bad.any(), '%s: max error %.3e, allowed %.3e' % (
        what, err.max(), np.broadcast_to(tol, err.shape)[np.unravel_index(err.argmax(),
                                                                            err.shape)])


# ------------------------------------------------------------------ xent
def _xent_gpu(c, dev, shift=0.0, x=None, tgt='case'):
    ops = _ops()
    x = c['x'] if x is None else x
    logits = _d((x + np.float32(shift)).astype(np.float32), dev).requires_grad_(True)
    tgt = c['tgt'] if isinstance(tgt, str) else tgt
    loss = ops.xent(logits, _d(tgt, dev), _d(c['lens'], dev), c['T'], c['ce'], c['ls'])
    (loss * c['g']).backward()
    torch.cuda.synchronize()
    return float(loss.item()), _h(logits.grad)


def _xent_check(c, got, ref):
    (loss, dx), (l64, d64, S) = got, ref
    R_, V = c['x'].shape
    tol = (MARGIN * F32_XENT_LOSS + R.gamma(R_) + R.gamma(V)) * S
    assert np.isfinite(loss) and abs(loss - l64) <= tol, '%s: loss %r vs %r (allowed %.3e)' % (
        c['name'], loss, l64, tol)
    _close(dx, d64, MARGIN * F32_XENT_DX * abs(c['g']) * (abs(c['ce']) + abs(c['ls'])),
           c['name'] + ' dx')


@pytest.mark.parametrize('variant', R.XENT_VARIANTS)
def test_xent_forward_backward(variant, cuda_dev):
    """V across the 64-lane stride, R across the 4-rows-per-block tail."""
    for c in R.xent_cases():
        if c['name'].startswith(variant + '-'):
            _xent_check(c, _xent_gpu(c, cuda_dev), R.xent_ref(c))


@pytest.mark.parametrize('shift', [50.0, -50.0])
def test_xent_shift_invariance(shift, cuda_dev):
    """The loss does not depend on a common offset of the logits: the shifted
    run must meet the unshifted reference within the unshifted bound.  The
    label-smoothing term is formed as -(sum_v x[v] - V * lse) / V, which cancels
    |offset| * V against itself; at +-50 the result stays inside the bound, so
    the kernel keeps that form."""
    for c in R.xent_cases():
        if c['name'].split('-')[0] in ('ls_notgt', 'both'):
            _xent_check(c, _xent_gpu(c, cuda_dev, shift), R.xent_ref(c))


def test_xent_minus_inf_logits(cuda_dev):
    """CE only, some -inf entries (never the target): finite loss, exactly zero
    gradient at those entries."""
    for c in R.xent_cases():
        if not c['name'].startswith('ce-') or c['x'].shape[1] < 63:
            continue
        x = c['x'].copy()
        hole = np.zeros(x.shape, bool)
        hole[:, ::3] = True
        hole[np.arange(len(x)), c['tgt']] = False
        x[hole] = -np.inf
        loss, dx = _xent_gpu(c, cuda_dev, x=x)
        assert np.isfinite(loss) and np.isfinite(dx).all()
        assert (dx[hole] == 0).all()
        _xent_check(c, (loss, dx), R.xent(x, c['tgt'], None, 0, c['ce'], c['ls'], c['g']))


def test_xent_target_beyond_vocabulary_is_clamped(cuda_dev):
    """Documented in asr_hip.h: a target >= V is treated as V - 1."""
    c = next(c for c in R.xent_cases() if c['name'] == 'both-V65-R5')
    V = c['x'].shape[1]
    hi, last = c['tgt'].copy(), c['tgt'].copy()
    hi[[1, 3]] = (V, V + 7)
    last[[1, 3]] = V - 1
    a = _xent_gpu(c, cuda_dev, tgt=hi)
    b = _xent_gpu(c, cuda_dev, tgt=last)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])
    _xent_check(c, a, R.xent(c['x'], last, None, 0, c['ce'], c['ls'], c['g']))
    _xent_check(c, a, R.xent(c['x'], hi, None, 0, c['ce'], c['ls'], c['g']))


def test_softmax(cuda_dev):
    for c in R.xent_cases():
        if not c['name'].startswith('ce-'):
            continue
        y = _h(_ops().softmax(_d(c['x'], cuda_dev))).astype(np.float64)
        y64 = R.softmax(c['x'])
        rel = MARGIN * F32_SOFTMAX_REL
        _close(y, y64, rel * y64, c['name'] + ' softmax')
        # entries within rel of values summing to 1 -> the row sum within rel of 1
        assert np.abs(y.sum(-1) - 1).max() <= rel, c['name']


# ---------------------------------------------------- best path / argmax
def _best_path_check(logits, lens, blank, dev, abi_strides=False):
    B, T, V = logits.shape
    ref = ctc_ref.greedy_best_path(logits, np.minimum(lens, T), blank)
    if abi_strides:      # time-major storage [T][B][V'] with V' > V
        N = _N()
        Vp = V + 3
        tm = np.full((T, B, Vp), 1e30, np.float32)     # the pad would win if it were read
        tm[:, :, :V] = logits.transpose(1, 0, 2)
        lg = _d(tm, dev)
        hyps = torch.full((B, T), -7, dtype=torch.int32, device=dev)
        hl = torch.full((B,), -7, dtype=torch.int32, device=dev)
        N.call('asr_ctc_best_path', N.ptr(lg), B * Vp, Vp, T, B, V,
               N.ptr(_d(lens.astype(np.int32), dev)), int(blank), N.ptr(hyps), N.ptr(hl),
               N.stream_handle(dev))
    else:
        hyps, hl = _ops().ctc_best_path(_d(logits, dev), _d(lens.astype(np.int32), dev), blank)
    torch.cuda.synchronize()
    hyps, hl = _h(hyps), _h(hl)
    for b in range(B):
        assert hl[b] == len(ref[b]), (b, hl[b], len(ref[b]))
        np.testing.assert_array_equal(hyps[b, :hl[b]], ref[b])
    return ref


@pytest.mark.parametrize('V', [2, 29, 65, 130])
def test_best_path_random(V, cuda_dev):
    """T across the 64-frame chunk, V across the 64-lane stride; lens 0, 1, 64,
    65, T and beyond T.  Few classes -> many repeats and blanks per chunk."""
    rng = np.random.RandomState(1710 + V)
    for T in (1, 63, 64, 65, 128, 130):
        logits = rng.randn(3, T, V).astype(np.float32)
        _best_path_check(logits, np.array([0, 1, T + 5]), 0, cuda_dev)
        _best_path_check(logits, np.array([64, 65, T]), V - 1, cuda_dev)


def _one_hot_frames(labels, V):
    x = np.zeros((1, len(labels), V), np.float32)
    x[0, np.arange(len(labels)), labels] = 5.0
    return x


def test_best_path_chunk_boundaries(cuda_dev):
    T, V = 130, 5
    lab = np.array([1, 2, 3, 4] * 33)[:T]          # no repeats, no blank (0)
    rep = lab.copy()
    rep[62:66] = 1                                 # one label across frames 63 | 64
    rep[126:129] = 4                               # and across 127 | 128
    split = lab.copy()
    split[62:65] = (3, 0, 3)                       # label, blank at 63, same label at 64
    blank_chunk = lab.copy()
    blank_chunk[64:128] = 0                        # the second chunk is all blank
    blank_chunk[63] = blank_chunk[128] = 4         # same label on both sides: two tokens
    batch = np.concatenate([_one_hot_frames(s, V) for s in (rep, split, blank_chunk)])
    ref = _best_path_check(batch, np.array([T, T, T]), 0, cuda_dev)
    assert len(ref[0]) == T - 3 - 2 and len(ref[1]) == T - 1 and len(ref[2]) == T - 64
    # a non-zero blank: class 3 is dropped, the rest collapse as before
    _best_path_check(batch, np.array([T, 65, 129]), 3, cuda_dev)


def test_best_path_ties_and_strides(cuda_dev):
    """Exact ties: classes v and v + 64 meet in one lane, neighbours in two
    lanes; the first index wins as in np.argmax.  Then time-major strides."""
    rng = np.random.RandomState(1720)
    T, V = 70, 130
    logits = rng.randn(3, T, V).astype(np.float32)
    for t in range(T):
        top = logits[:, t].max() + 1
        a = (t * 7) % 64
        logits[0, t, [a, a + 64]] = top            # same lane
        logits[1, t, [a + 1, a]] = top             # neighbouring lanes
        logits[2, t, [a + 65, a, a + 64]] = top    # both
    _best_path_check(logits, np.array([T, T, T]), 0, cuda_dev)
    _best_path_check(logits, np.array([T, 64, 9]), 0, cuda_dev, abi_strides=True)


def test_row_argmax(cuda_dev):
    rng = np.random.RandomState(1730)
    for rows in (1, 4, 5):
        for V in (1, 64, 65, 10001):
            x = rng.randn(rows, V).astype(np.float32)
            got = _h(_ops().row_argmax(_d(x, cuda_dev)))
            np.testing.assert_array_equal(got, np.argmax(x, -1))
            if V > 1:                              # ties: in one lane and across lanes
                x[:, [V - 1, V // 2, max(V // 2 - 64, 0)]] = 9.0
                x[-1, :] = -np.inf                 # an all -inf row gives 0
                got = _h(_ops().row_argmax(_d(x, cuda_dev)))
                np.testing.assert_array_equal(got, np.argmax(x, -1))
                assert got[-1] == 0


def test_argmax_of_nan_rows_stays_in_range(cuda_dev):
    """A row / frame of all NaN gives index 0 (the lanes' initial index once
    escaped the reduction as 0x7fffffff)."""
    for V in (1, 64, 65, 10001):
        x = np.full((5, V), np.nan, np.float32)
        x[2] = np.arange(V)
        got = _h(_ops().row_argmax(_d(x, cuda_dev)))
        np.testing.assert_array_equal(got, [0, 0, V - 1, 0, 0])
    x = np.full((2, 66, 29), np.nan, np.float32)
    x[1] = _one_hot_frames(np.arange(66) % 29, 29)[0]
    hyps, hl = _ops().ctc_best_path(_d(x, cuda_dev), _d(np.array([66, 66], np.int32), cuda_dev),
                                    blank=28)
    hyps, hl = _h(hyps), _h(hl)
    assert hl[0] == 1 and hyps[0, 0] == 0          # every frame 0: one token
    ref = ctc_ref.greedy_best_path(x[1:], [66], 28)[0]
    np.testing.assert_array_equal(hyps[1, :hl[1]], ref)


# -------------------------------------------------------------- embedding
@pytest.mark.parametrize('trans', [0, 1])
def test_embedding_forward_exact(trans, cuda_dev):
    rng = np.random.RandomState(1740)
    V = 7
    for E in (1, 63, 64, 65, 130):
        w = rng.randn(V, E).astype(np.float32)
        wd = _d(w.T if trans else w, cuda_dev)
        for n in (1, 300):
            idx = rng.randint(0, V, n)
            f = _ops().embedding_t if trans else _ops().embedding
            np.testing.assert_array_equal(_h(f(_d(idx, cuda_dev), wd)), R.embedding_fwd(idx, w))


# rows per token: the slot (16) and 4-way unroll (64) boundaries of embedding_bwd_csr
EMB_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 130)


def _embedding_grad(idx, dout, w0, g0, trans, pad, host, dev):
    """weight.grad after backward through native_ops.embedding[_t], started
    from the non-zero gradient g0 ([V, E]); twice, bit-identical."""
    runs = []
    for _ in range(2):
        w = _d(w0.T if trans else w0, dev).requires_grad_(True)
        w.grad = _d(g0.T if trans else g0, dev)
        idx_d = _d(idx, dev)
        kw = dict(idx_host=idx if host else None)
        out = _ops().embedding_t(idx_d, w, **kw) if trans else _ops().embedding(idx_d, w, pad, **kw)
        np.testing.assert_array_equal(_h(out), R.embedding_fwd(idx, w0))
        out.backward(_d(dout, dev))
        torch.cuda.synchronize()
        runs.append(_h(w.grad).T if trans else _h(w.grad))
    np.testing.assert_array_equal(runs[0], runs[1])
    return runs[0]


def _embedding_check(idx, V, E, trans, pad, host, dev, rng):
    dout = rng.randn(len(idx), E).astype(np.float32)
    w0 = rng.randn(V, E).astype(np.float32)
    g0 = rng.randn(V, E).astype(np.float32)
    got = _embedding_grad(idx, dout, w0, g0, trans, pad, host, dev)
    ref, mag, cnt = R.embedding_bwd(idx, dout, V, pad, g0)
    _close(got, ref, R.gamma(cnt + 1)[:, None] * mag, 'embedding grad E=%d' % E)
    if pad is not None:
        np.testing.assert_array_equal(got[pad], g0[pad])
    return got


@pytest.mark.parametrize('host', [False, True], ids=['scan', 'csr'])
@pytest.mark.parametrize('trans', [0, 1])
def test_embedding_backward(trans, host, cuda_dev):
    rng = np.random.RandomState(1741)
    pad = None if trans else 9
    V = len(EMB_COUNTS) + 2
    idx = np.repeat(np.arange(V), EMB_COUNTS + (5, 3))     # token 9 (padding when trans = 0): 5
    rng.shuffle(idx)
    for E in (1, 63, 64, 65, 130):
        _embedding_check(idx, V, E, trans, pad, host, cuda_dev, rng)


@pytest.mark.parametrize('pad', [None, 0, 6])
def test_embedding_out_of_range_indices(pad, cuda_dev):
    """One rule in the forward and both backward forms: an index outside [0, V)
    is row clamp(idx, 0, V-1), and gets that row's gradient unless it is the
    padding row (the scan backward once dropped these rows)."""
    rng = np.random.RandomState(1742)
    V, E = 7, 65
    idx = rng.randint(0, V, 40)
    idx[[0, 7, 19]] = -1
    idx[[3, 11]] = V
    idx[5] = V + 100
    for host in (False, True):
        _embedding_check(idx, V, E, 0, pad, host, cuda_dev, np.random.RandomState(5))
        if pad is None:
            _embedding_check(idx, V, E, 1, None, host, cuda_dev, np.random.RandomState(5))


# ------------------------------------------------------------------ cells
def _lstm_gpu(c, nulls, dev):
    N = _N()
    B, D = c['B'], c['D']
    cp, dh, dc = (_d(c[k], dev) if on else None for k, on in zip(('c_prev', 'dh', 'dc'), nulls))
    pre = _d(c['pre'], dev)
    e = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    act, h, cc, dpre, dcp = e(B, 4 * D), e(B, D), e(B, D), e(B, 4 * D), e(B, D)
    st = N.stream_handle(dev)
    N.call('asr_lstm_cell_forward', N.ptr(pre), N.ptr(cp), B, D, N.ptr(act), N.ptr(h), N.ptr(cc),
           st)
    N.call('asr_lstm_cell_backward', N.ptr(act), N.ptr(cp), N.ptr(cc), N.ptr(dh), N.ptr(dc), B, D,
           N.ptr(dpre), N.ptr(dcp), st)
    torch.cuda.synchronize()
    return [_h(t) for t in (h, cc, act, dpre, dcp)]


@pytest.mark.parametrize('nulls', R.LSTM_NULLS, ids=['all', 'no_c_prev', 'no_dh', 'no_dc'])
def test_lstm_cell(nulls, cuda_dev):
    for c in R.cell_cases():
        got, ref = _lstm_gpu(c, nulls, cuda_dev), R.lstm_ref(c, nulls)
        for i, name in enumerate(('h', 'c', 'act', 'dpre', 'dc_prev')):
            _close(got[i], ref[i], MARGIN * (F32_LSTM_FWD if i < 3 else F32_LSTM_BWD),
                   'lstm_cell %s B=%d D=%d' % (name, c['B'], c['D']))


def _gru_gpu(c, dev):
    N = _N()
    B, D = c['B'], c['D']
    gi, gh, h, dh = (_d(c[k], dev) for k in ('gi', 'gh', 'h', 'dh'))
    e = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    act, hout, dgi, dgh, dhp = e(B, 3 * D), e(B, D), e(B, 3 * D), e(B, 3 * D), e(B, D)
    st = N.stream_handle(dev)
    N.call('asr_gru_cell_forward', N.ptr(gi), N.ptr(gh), N.ptr(h), B, D, N.ptr(act), N.ptr(hout),
           st)
    N.call('asr_gru_cell_backward', N.ptr(act), N.ptr(gh), N.ptr(h), N.ptr(dh), B, D, N.ptr(dgi),
           N.ptr(dgh), N.ptr(dhp), st)
    torch.cuda.synchronize()
    return [_h(t) for t in (hout, act, dgi, dgh, dhp)]


def test_gru_cell(cuda_dev):
    for c in R.cell_cases():
        got, ref = _gru_gpu(c, cuda_dev), R.gru_ref(c)
        for i, name in enumerate(('hout', 'act', 'dgi', 'dgh', 'dh_prev')):
            _close(got[i], ref[i], MARGIN * (F32_GRU_FWD if i < 2 else F32_GRU_BWD),
                   'gru_cell %s B=%d D=%d' % (name, c['B'], c['D']))


def test_cells_saturated_gates_stay_finite(cuda_dev):
    """Pre-activations of +-30: no NaN or inf anywhere, forward or backward."""
    rng = np.random.RandomState(1750)
    B, D = 3, 65
    f = lambda *s: rng.randn(*s).astype(np.float32)
    s = lambda *s_: (30 * rng.choice([-1.0, 1.0], s_)).astype(np.float32)
    c = dict(B=B, D=D, pre=s(B, 4 * D), c_prev=f(B, D), dh=f(B, D), dc=f(B, D), gi=s(B, 3 * D) / 2,
             gh=s(B, 3 * D) / 2, h=f(B, D))
    for out in _lstm_gpu(c, (1, 1, 1), cuda_dev) + _gru_gpu(c, cuda_dev):
        assert np.isfinite(out).all()


# ------------------------------------------------- tanh / add_tanh / add
def test_tanh_add_tanh_add(cuda_dev):
    """n across one block and, at 4096 * 256 + 3, into the grid-stride loop."""
    ops = _ops()
    for c in R.elem_cases():
        a, b, dy = (_d(c[k], cuda_dev) for k in ('a', 'b', 'dy'))
        what = 'n=%d' % c['n']
        np.testing.assert_array_equal(_h(ops.add(a, b)), c['a'] + c['b'])
        x = a.clone().requires_grad_(True)
        y = ops.tanh(x)
        y.backward(dy)
        y64, dx64 = R.tanh_fb(c['a'], c['dy'])
        _close(_h(y), y64, MARGIN * F32_TANH_FWD, 'tanh ' + what)
        _close(_h(x.grad), dx64, MARGIN * F32_TANH_BWD, 'tanh backward ' + what)
        p, q = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = ops.add_tanh(p, q)
        y.backward(dy)
        y64, dx64 = R.add_tanh_fb(c['a'], c['b'], c['dy'])
        _close(_h(y), y64, MARGIN * F32_TANH_FWD, 'add_tanh ' + what)
        _close(_h(p.grad), dx64, MARGIN * F32_TANH_BWD, 'add_tanh backward a ' + what)
        np.testing.assert_array_equal(_h(p.grad), _h(q.grad))


# ----------------------------------------------------------------- colsum
COLSUM_SHAPES = ((1, 1), (3, 65), (63, 64), (64, 16), (65, 17), (127, 130), (4099, 48),
                 (4160, 8200))


def _colsum_gpu(g, M, Nn, ld, alpha, out0, out1, bf16, dev):
    """g: device tensor [M, ld] (f32, or int16 holding bf16 bits)."""
    N = _N()
    nb = N.query('asr_colsum_workspace_bytes', M, Nn)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    N.call('asr_colsum_accumulate_bf16' if bf16 else 'asr_colsum_accumulate', N.ptr(g), ld, M, Nn,
           float(alpha), N.ptr(out0), N.ptr(out1), N.ptr(ws), nb, N.stream_handle(dev))


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', COLSUM_SHAPES, ids=lambda s: '%dx%d' % s)
def test_colsum_accumulate(shape, bf16, cuda_dev):
    """Across the M / 64 chunk rule, the 32-row unroll, the 4-wave split and N
    not a multiple of 64 or 16; ld > N, a second output, alpha != 1 and
    non-zero outputs everywhere but at the largest shape (ld = N, one output)."""
    M, Nn = shape
    big = M * Nn > 1 << 22
    ld = Nn if big else Nn + 5
    alpha = 1.0 if big else -0.75
    gen = torch.Generator(device='cpu').manual_seed(1760 + M)
    g = torch.randn(M, ld, generator=gen)
    if bf16:
        g = g.to(torch.bfloat16)
    gd = g.to(cuda_dev)
    g64 = g[:, :Nn].double()
    o0 = torch.randn(Nn, generator=gen)
    o1 = torch.randn(Nn, generator=gen)
    ref = [(o.double() + alpha * g64.sum(0)).numpy() for o in (o0, o1)]
    # M addends, the product by alpha, the accumulation onto the output
    tol = R.gamma(M + 2) * (abs(alpha) * g64.abs().sum(0) + o0.abs().double()).numpy()
    runs = []
    for _ in range(2):
        a, b = o0.to(cuda_dev), (None if big else o1.to(cuda_dev))
        _colsum_gpu(gd, M, Nn, ld, alpha, a, b, bf16, cuda_dev)
        torch.cuda.synchronize()
        runs.append((_h(a), None if big else _h(b)))
    _close(runs[0][0], ref[0], tol, 'colsum out0')
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    if not big:
        # both outputs receive the same sum (added onto different contents)
        tol1 = R.gamma(M + 2) * (abs(alpha) * g64.abs().sum(0) + o1.abs().double()).numpy()
        _close(runs[0][1], ref[1], tol1, 'colsum out1')
        np.testing.assert_array_equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------ grad_sqnorm
def _sqnorm_gpu(g, n, dev):
    N = _N()
    nb = N.query('asr_grad_sqnorm_workspace_bytes')
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    N.call('asr_grad_sqnorm', N.ptr(g), n, N.ptr(out), N.ptr(ws), nb, N.stream_handle(dev))
    torch.cuda.synchronize()
    return float(out.item())


def test_grad_sqnorm(cuda_dev):
    """float4 body, scalar tail, a second sweep of the 1024 x 256 x 4 grid."""
    rng = np.random.RandomState(1770)
    for n in (1, 3, 4, 5, 1023, 1024 * 256 * 4 - 1, 1024 * 256 * 4 + 3):
        g = (10.0 ** rng.uniform(-4, 2, n) * rng.choice([-1, 1], n)).astype(np.float32)
        g[-1] = 77.0                     # the tail carries weight
        ref = (g.astype(np.float64) ** 2).sum()
        got = _sqnorm_gpu(_d(g, cuda_dev), n, cuda_dev)
        # n squares (one rounding each) summed
        assert abs(got - ref) <= R.gamma(n + 1) * ref, (n, got, ref)


def test_grad_sqnorm_rejects_misaligned_pointer(cuda_dev):
    N = _N()
    g = torch.ones(9, dtype=torch.float32, device=cuda_dev)
    assert g.data_ptr() % 16 == 0
    nb = N.query('asr_grad_sqnorm_workspace_bytes')
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda_dev)
    out = torch.zeros(1, dtype=torch.float32, device=cuda_dev)
    rc = N.query('asr_grad_sqnorm', ctypes.c_void_p(g.data_ptr() + 4), 8, N.ptr(out), N.ptr(ws), nb,
                 N.stream_handle(cuda_dev))
    torch.cuda.synchronize()
    assert rc == -1                      # ASR_ERR_ARG
    assert b'16-B aligned' in N.lib().asr_last_error()
    assert out.item() == 0.0             # nothing was launched


# -------------------------------------------------------------- optimizer
def _bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()


def _optim_call(kind, p, g, m, v, n, hp, step, sqn, shadow, guard, dev):
    N = _N()
    args = [kind, N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, hp['lr'], hp['beta1'], hp['beta2'],
            hp['eps'], hp['wd'], step, hp['momentum'], hp['dampening'], N.ptr(sqn),
            hp['max_norm'], N.ptr(shadow)]
    if guard is None:
        N.call('asr_optim_step', *args, N.stream_handle(dev))
    else:
        N.call('asr_optim_step_guarded', *args, N.ptr(guard), N.stream_handle(dev))


@pytest.mark.parametrize('kind', [0, 1, 2, 3], ids=['adam', 'sgd', 'momentum', 'nesterov'])
def test_optim_step(kind, cuda_dev):
    """Three consecutive steps (Adam's bias correction, the momentum buffer's
    first step), weight decay, dampening, every clip mode; n into the
    grid-stride loop; the bf16 shadow is RNE of what the kernel wrote."""
    dev = cuda_dev
    for c in R.optim_cases():
        if c['kind'] != kind:
            continue
        n = c['n']
        p = _d(c['p'], dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        shadow = torch.zeros(n, dtype=torch.int16, device=dev)
        what = 'kind %d n=%d clip %s' % (kind, n, c['clip'])
        for step, hp, sqn, p64, m64, v64 in R.optim_run(c):
            sq = None if sqn is None else _d(np.array([sqn], np.float32), dev)
            _optim_call(kind, p, _d(c['g'][step - 1], dev), m, v, n, hp, step, sq, shadow, None,
                        dev)
            torch.cuda.synchronize()
            w = '%s step %d ' % (what, step)
            _close(_h(p), p64, MARGIN * F32_OPTIM_P, w + 'p')
            if kind != 1:
                _close(_h(m), m64, MARGIN * F32_OPTIM_M, w + 'm')
            if kind == 0:
                _close(_h(v), v64, MARGIN * F32_OPTIM_V, w + 'v')
            np.testing.assert_array_equal(_h(shadow), _bf16_bits(_h(p)))


@pytest.mark.parametrize('kind', [0, 2])
def test_optim_step_guarded_skips_the_update(kind, cuda_dev):
    dev = cuda_dev
    rng = np.random.RandomState(1780)
    n = 8192 * 256 + 257
    f = lambda: rng.randn(n).astype(np.float32)
    p0, m0, v0 = f(), f(), np.abs(f())
    hp = dict(R.optim_hp(kind), max_norm=1.0)
    sq = _d(np.array([float(n)], np.float32), dev)
    for guard in ([0, 3], [1, 0]):
        p, g, m, v = _d(p0, dev), _d(f(), dev), _d(m0, dev), _d(v0, dev)
        shadow = torch.zeros(n, dtype=torch.int16, device=dev)
        _optim_call(kind, p, g, m, v, n, hp, 2, sq, shadow, _d(np.array(guard, np.int32), dev), dev)
        torch.cuda.synchronize()
        for got, was in ((p, p0), (m, m0), (v, v0)):
            np.testing.assert_array_equal(_h(got).view(np.int32), was.view(np.int32))
        np.testing.assert_array_equal(_h(shadow), _bf16_bits(p0))
    # a zero guard word lets the step through
    p, g, m, v = _d(p0, dev), _d(f(), dev), _d(m0, dev), _d(v0, dev)
    _optim_call(kind, p, g, m, v, n, hp, 2, sq, None, _d(np.zeros(2, np.int32), dev), dev)
    torch.cuda.synchronize()
    assert (_h(p) != p0).mean() > 0.9
