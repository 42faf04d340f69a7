"""The autograd functions of native_ops.py that join the GEMM kernels into the
attention models -- linear_ex, linear2, mean_time, add_batch_sum, dropout --
against the float64 references of tests/glue_refs.py, forward and backward, in
both compute modes.

Operands are small integers, so every product and sum is exact in f32 and in
bf16 with f32 accumulation: linear_ex, linear2, add_batch_sum and dropout at
p = 0.5 must EQUAL float64.  mean_time multiplies an exact integer sum by
fl(1 / T): equal for T a power of two, else within 4 * 2^-24 |ref| (one
rounding of 1 / T, one of the product, a factor 2 to spare).  dropout at other
p: asr_dropout computes x * fl(1 / fl(1 - p)) (elementwise.hip, dropout_kernel:
a multiplication by the reciprocal, not the division), so y and dx are held to
2 * 2^-24 |ref| of fl32(x * mask / fl32(1 - p)), the division done here in
float32.  (For |x| <= 3 that is one ulp: 3 fl(1 / q) is within 0.75 ulp of
3 / q before its rounding, the reference within 0.5 ulp.)

Every input is a view into a larger NaN-filled allocation, so a read outside
the operand turns the result to NaN; every gradient buffer is a view into a
larger allocation whose surroundings must keep their fill, is prefilled with
an integer pattern, and must hold pattern + gradient inside the written
window and the pattern outside it.

Where the forward is one GEMM launch (linear_ex, mean_time) the kernel family
the dispatcher took is asserted from glue_refs' case tables, which derive it
from the predicates of csrc/gemm.hip (fast32_operand_ok, plan_stage,
big8_ok), so a case cannot quietly stop covering its path.

What the one-bias cases exposed (they fail on the code before this fix): with
the first bias absent and the second given (linear_ex(bias=None, bias2=b), linear2(b1=None, b2=b)) the
forwards added the second bias but the backwards summed bias gradients only
under ``if bias is not None`` -- the second bias got no gradient.  Both
backwards now sum into whichever biases are given (native_ops._bias_pair_grad).
"""
import numpy as np
import pytest
import torch

import glue_refs as R

pytestmark = pytest.mark.gpu

PAD = 8            # floats around every view: 32 B, views stay 16-B aligned
GUARD = 12345.0    # fill around the gradient buffers
MODES = ['fp32', 'bf16']


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _family():
    from pytorch_end2end_speech_recognition_amd import _native as NL
    return NL.query('asr_gemm_last_family') // 4


def _view(a, dev, grad=False, fill=float('nan')):
    """a (numpy f32) as a contiguous view PAD floats into a larger allocation
    filled with `fill`; a leaf that requires grad when asked."""
    if a is None:
        return None
    buf = torch.full((a.size + 2 * PAD,), fill, dtype=torch.float32, device=dev)
    v = buf[PAD:PAD + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    v._glue_buf = buf
    return v.requires_grad_(grad)


def _param(a, g0, dev):
    """A parameter view of a with .grad prefilled with g0 inside a guarded buffer."""
    if a is None:
        return None
    p = _view(a, dev, grad=True)
    p._glue_grad = _view(g0, dev, fill=GUARD)
    p.grad = p._glue_grad
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _check_grad(p, ref, name):
    """p.grad == ref, and the guard floats around the buffer untouched."""
    assert p.grad.data_ptr() == p._glue_grad.data_ptr(), name + ': gradient buffer replaced'
    np.testing.assert_array_equal(_np(p.grad), ref, err_msg=name)
    g = _np(p._glue_grad._glue_buf)
    assert (g[:PAD] == GUARD).all() and (g[-PAD:] == GUARD).all(), name + ': guard overwritten'


def _in_mode(mode, fn):
    ops = _ops()
    ops.set_compute_dtype(mode)
    try:
        fn(ops)
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype('fp32')


def _run_linear_ex(ops, dev, inp, family, need_dx=True):
    ref = R.linear_ex(**inp)
    c0, K, ti = inp['c0'], inp['K'], inp['t_index']
    x = _view(inp['x'], dev, grad=need_dx)
    w = _param(inp['w'], inp['gw0'], dev)
    b = _param(inp['b'], inp['gb0'], dev)
    b2 = _param(inp['b2'], inp['gb20'], dev)
    y = ops.linear_ex(x, w, b, b2, c0=c0, K=K, t_index=ti)
    fam = _family()
    assert fam == family, 'forward took family %s, the case is derived for %s' % (
        R.FAMILY_NAMES.get(fam, fam), R.FAMILY_NAMES[family])
    y.backward(_view(inp['dy'], dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(y), ref['y'], err_msg='y')
    if need_dx:
        np.testing.assert_array_equal(_np(x.grad), ref['dx'], err_msg='dx')
        if ti is not None:      # the scattered dX: exactly zero at every other time index
            other = [t for t in range(inp['x'].shape[1]) if t != ti]
            assert not _np(x.grad)[:, other, :].any()
    else:
        assert x.grad is None
    _check_grad(w, ref['gw'], 'gw')
    gw = _np(w.grad)
    # columns of the weight gradient outside the window are unchanged
    np.testing.assert_array_equal(gw[:, :c0], inp['gw0'][:, :c0])
    np.testing.assert_array_equal(gw[:, c0 + K:], inp['gw0'][:, c0 + K:])
    for p, key in ((b, 'gb'), (b2, 'gb2')):
        if p is not None:
            _check_grad(p, ref[key], key)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(R.LINEAR_EX_ALL))
def test_linear_ex_all_steps(name, mode, cuda_dev):
    """linear_ex over all steps: a column window [c0, c0 + K) of a wider weight,
    both biases; y, dx, and the weight / bias gradients accumulated onto
    prefilled buffers (the M = 2048 cases through split-K into the windowed,
    pitched C: splitk_reduce4 at c0 = 0 and 4, the scalar reduce at c0 = 2 and
    at pitch 50)."""
    family = R.LINEAR_EX_ALL[name][7 + MODES.index(mode)]
    _in_mode(mode, lambda ops: _run_linear_ex(ops, cuda_dev, R.linear_ex_all_inputs(name),
                                              family))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('case', R.LINEAR_EX_T, ids=lambda c: 'x'.join(map(str, c[:4])))
def test_linear_ex_time_index(case, last, need_dx, mode, cuda_dev):
    """linear_ex at a fixed time index: x rows read at pitch T K from base
    offset t_index K, dX scattered through the same map into a zeroed tensor;
    with and without an input gradient."""
    B, T, K, Nout = case[:4]
    family = case[4 + MODES.index(mode)]
    inp = R.linear_ex_t_inputs(B, T, K, Nout, T - 1 if last else 0)
    _in_mode(mode, lambda ops: _run_linear_ex(ops, cuda_dev, inp, family, need_dx))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('biases', R.LINEAR2_BIASES)
@pytest.mark.parametrize('M,K1,K2,Nout', R.LINEAR2)
def test_linear2(M, K1, K2, Nout, biases, mode, cuda_dev):
    """linear2: one C from two launches (beta = 0 with the bias pair, then
    beta = 1); the backward's two dX and two dW products of different K and N
    in one launch each (M = 1024: staged in bf16 mode, split-K dW)."""
    inp = R.linear2_inputs(M, K1, K2, Nout, biases)
    ref = R.linear2(**inp)

    def run(ops):
        dev = cuda_dev
        x1, x2 = _view(inp['x1'], dev, grad=True), _view(inp['x2'], dev, grad=True)
        w1, w2 = _param(inp['w1'], inp['gw10'], dev), _param(inp['w2'], inp['gw20'], dev)
        b1, b2 = _param(inp['b1'], inp['gb10'], dev), _param(inp['b2'], inp['gb20'], dev)
        y = ops.linear2(x1, w1, b1, x2, w2, b2)
        y.backward(_view(inp['dy'], dev))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(y), ref['y'], err_msg='y')
        np.testing.assert_array_equal(_np(x1.grad), ref['dx1'], err_msg='dx1')
        np.testing.assert_array_equal(_np(x2.grad), ref['dx2'], err_msg='dx2')
        _check_grad(w1, ref['gw1'], 'gw1')
        _check_grad(w2, ref['gw2'], 'gw2')
        for p, key in ((b1, 'gb1'), (b2, 'gb2')):
            if p is not None:
                _check_grad(p, ref[key], key)
    _in_mode(mode, run)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.MEAN_TIME, ids=lambda c: 'x'.join(map(str, c[:3])))
def test_mean_time(case, mode, cuda_dev):
    """mean_time: a batched M = 1 product whose ones operand has batch stride
    0, and its batched K = 1 backward with A pitch 1; (16, 2048, 512) is staged
    in bf16 mode (stage_map with an A batch stride of 0)."""
    B, T, E = case[:3]
    family = case[3 + MODES.index(mode)]
    inp = R.mean_time_inputs(B, T, E)
    ref = R.mean_time(**inp)

    def check(got, want, name):
        if T & (T - 1) == 0:
            np.testing.assert_array_equal(got, want, err_msg=name)
        else:
            err = np.abs(got.astype(np.float64) - want)
            bound = 4.0 * 2.0 ** -24 * np.abs(want)
            rel = err / np.maximum(np.abs(want), 1e-300)
            print('%s: max err / |ref| = %.3g' % (name, rel.max()))
            assert (err <= bound).all(), (name, float((err - bound).max()))

    def run(ops):
        x = _view(inp['x'], cuda_dev, grad=True)
        out = ops.mean_time(x)
        fam = _family()
        assert fam == family, 'forward took family %s, the case is derived for %s' % (
            R.FAMILY_NAMES.get(fam, fam), R.FAMILY_NAMES[family])
        out.backward(_view(inp['dout'], cuda_dev))
        torch.cuda.synchronize()
        check(_np(out), ref['out'], 'out')
        check(_np(x.grad), ref['dx'], 'dx')
    _in_mode(mode, run)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B,D', R.ADD_BATCH_SUM)
def test_add_batch_sum(B, D, mode, cuda_dev):
    """add_batch_sum: a [1 x B] x [B x D] product, then a K = 1 broadcast with
    beta = 1 onto a clone of h (h itself must stay as it was)."""
    inp = R.add_batch_sum_inputs(B, D)
    ref = R.add_batch_sum(**inp)

    def run(ops):
        h, lower = _view(inp['h'], cuda_dev, grad=True), _view(inp['lower'], cuda_dev, grad=True)
        y = ops.add_batch_sum(h, lower)
        y.backward(_view(inp['dy'], cuda_dev))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(y), ref['y'], err_msg='y')
        np.testing.assert_array_equal(_np(h), inp['h'], err_msg='h overwritten')
        np.testing.assert_array_equal(_np(lower), inp['lower'], err_msg='lower overwritten')
        np.testing.assert_array_equal(_np(h.grad), ref['dh'], err_msg='dh')
        np.testing.assert_array_equal(_np(lower.grad), ref['dlower'], err_msg='dlower')
    _in_mode(mode, run)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p', R.DROPOUT_P)
@pytest.mark.parametrize('n', R.DROPOUT_N)
def test_dropout(n, p, mode, cuda_dev):
    """dropout forward and backward with a given seed: the mask of both is
    oracle/rng.py's; values equal float64 at p = 0.5 and are within
    2 * 2^-24 |ref| of the float32 division otherwise (module docstring)."""
    inp = R.dropout_inputs(n)
    ref = R.dropout(inp['x'], p, R.DROPOUT_SEED, inp['dy'])

    def check(got, src, want64, name):
        np.testing.assert_array_equal(got != 0, ref['keep'], err_msg=name + ' mask')
        if p == 0.5:
            np.testing.assert_array_equal(got, want64, err_msg=name)
            return
        want = (src * ref['keep'].astype(np.float32)) / (np.float32(1.0) - np.float32(p))
        assert want.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bound = 2.0 * 2.0 ** -24 * np.abs(want.astype(np.float64))
        print('%s: mismatching elements %d of %d' % (name, int((got != want).sum()), n))
        assert (err <= bound).all(), (name, float((err - bound).max()))

    def run(ops):
        x = _view(inp['x'], cuda_dev, grad=True)
        y = ops.dropout(x, p, seed=R.DROPOUT_SEED)
        y.backward(_view(inp['dy'], cuda_dev))
        torch.cuda.synchronize()
        check(_np(y), inp['x'], ref['y'], 'y')
        check(_np(x.grad), inp['dy'], ref['dx'], 'dx')
    _in_mode(mode, run)


@pytest.mark.parametrize('n', R.DROPOUT_N[2:])
def test_dropout_module_seed_backward_mask(n, cuda_dev):
    """With the seed drawn from the module stream, the backward still applies
    the forward's mask."""
    inp = R.dropout_inputs(n)

    def run(ops):
        x = _view(inp['x'], cuda_dev, grad=True)
        y = ops.dropout(x, 0.5)
        y.backward(_view(inp['dy'], cuda_dev))
        torch.cuda.synchronize()
        keep = _np(y) != 0
        assert 0 < keep.sum() < n
        np.testing.assert_array_equal(_np(y), 2.0 * inp['x'] * keep)
        np.testing.assert_array_equal(_np(x.grad), 2.0 * inp['dy'] * keep)
    _in_mode('fp32', run)
