"""tests/glue_refs.py (the float64 numpy references of linear_ex, linear2,
mean_time, add_batch_sum and dropout) against torch.autograd in float64 on the
CPU, each op written the ordinary way, on the cases of
tests/test_glue_ops_gpu.py.  Integer operands make every sum exact in float64,
so the references must equal autograd's results; only the divisions of
mean_time and dropout are compared to 1e-15 relative."""
import numpy as np
import pytest
import torch

import glue_refs as R


def _t(a, grad=False):
    if a is None:
        return None
    return torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(grad)


def _acc(g0, p):
    """The gradient buffer after accumulation: g0 + p.grad."""
    return np.asarray(g0, np.float64) + p.grad.numpy()


def _check_linear_ex(inp):
    ref = R.linear_ex(**inp)
    x, w = _t(inp['x'], True), _t(inp['w'], True)
    b, b2 = _t(inp['b'], True), _t(inp['b2'], True)
    c0, K, ti = inp['c0'], inp['K'], inp['t_index']
    xs = x[:, ti, :] if ti is not None else x
    y = xs @ w[:, c0:c0 + K].T
    if b is not None:
        y = y + b
    if b2 is not None:
        y = y + b2
    y.backward(_t(inp['dy']))
    np.testing.assert_array_equal(ref['y'], y.detach().numpy())
    np.testing.assert_array_equal(ref['dx'], x.grad.numpy())
    np.testing.assert_array_equal(ref['gw'], _acc(inp['gw0'], w))
    # outside the window the buffer keeps its initial contents
    np.testing.assert_array_equal(ref['gw'][:, :c0], inp['gw0'][:, :c0])
    np.testing.assert_array_equal(ref['gw'][:, c0 + K:], inp['gw0'][:, c0 + K:])
    for key, p, g0 in (('gb', b, inp['gb0']), ('gb2', b2, inp['gb20'])):
        if p is None:
            assert ref[key] is None
        else:
            np.testing.assert_array_equal(ref[key], _acc(g0, p))
    if ti is not None:
        other = [t for t in range(inp['x'].shape[1]) if t != ti]
        assert not ref['dx'][:, other, :].any()


@pytest.mark.parametrize('name', sorted(R.LINEAR_EX_ALL))
def test_linear_ex_all_steps_reference(name):
    _check_linear_ex(R.linear_ex_all_inputs(name))


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('B,T,K,Nout', [c[:4] for c in R.LINEAR_EX_T])
def test_linear_ex_time_index_reference(B, T, K, Nout, last):
    _check_linear_ex(R.linear_ex_t_inputs(B, T, K, Nout, T - 1 if last else 0))


@pytest.mark.parametrize('biases', R.LINEAR2_BIASES)
@pytest.mark.parametrize('M,K1,K2,Nout', R.LINEAR2)
def test_linear2_reference(M, K1, K2, Nout, biases):
    inp = R.linear2_inputs(M, K1, K2, Nout, biases)
    ref = R.linear2(**inp)
    t = {k: _t(inp[k], True) for k in ('x1', 'w1', 'b1', 'x2', 'w2', 'b2')}
    y = t['x1'] @ t['w1'].T + t['x2'] @ t['w2'].T
    for k in ('b1', 'b2'):
        if t[k] is not None:
            y = y + t[k]
    y.backward(_t(inp['dy']))
    np.testing.assert_array_equal(ref['y'], y.detach().numpy())
    np.testing.assert_array_equal(ref['dx1'], t['x1'].grad.numpy())
    np.testing.assert_array_equal(ref['dx2'], t['x2'].grad.numpy())
    np.testing.assert_array_equal(ref['gw1'], _acc(inp['gw10'], t['w1']))
    np.testing.assert_array_equal(ref['gw2'], _acc(inp['gw20'], t['w2']))
    for key, k, g0 in (('gb1', 'b1', 'gb10'), ('gb2', 'b2', 'gb20')):
        if t[k] is None:
            assert ref[key] is None
        else:
            np.testing.assert_array_equal(ref[key], _acc(inp[g0], t[k]))


@pytest.mark.parametrize('B,T,E', [c[:3] for c in R.MEAN_TIME])
def test_mean_time_reference(B, T, E):
    inp = R.mean_time_inputs(B, T, E)
    ref = R.mean_time(**inp)
    x = _t(inp['x'], True)
    out = x.mean(1)
    out.backward(_t(inp['dout']))
    np.testing.assert_allclose(ref['out'], out.detach().numpy(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(ref['dx'], x.grad.numpy(), rtol=1e-15, atol=0)


@pytest.mark.parametrize('B,D', R.ADD_BATCH_SUM)
def test_add_batch_sum_reference(B, D):
    inp = R.add_batch_sum_inputs(B, D)
    ref = R.add_batch_sum(**inp)
    h, lower = _t(inp['h'], True), _t(inp['lower'], True)
    y = h + lower.sum(0)
    y.backward(_t(inp['dy']))
    np.testing.assert_array_equal(ref['y'], y.detach().numpy())
    np.testing.assert_array_equal(ref['dh'], h.grad.numpy())
    np.testing.assert_array_equal(ref['dlower'], lower.grad.numpy())


@pytest.mark.parametrize('p', R.DROPOUT_P)
@pytest.mark.parametrize('n', R.DROPOUT_N)
def test_dropout_reference(n, p):
    """y = x * m, m = keep / (1 - p) held constant: autograd gives dx = dy * m
    with the same mask; the mask is oracle/rng.py's u01(seed, i) >= p."""
    from oracle import rng
    inp = R.dropout_inputs(n)
    ref = R.dropout(inp['x'], p, R.DROPOUT_SEED, inp['dy'])
    keep = rng.u01(R.DROPOUT_SEED, n) >= np.float32(p)
    np.testing.assert_array_equal(ref['keep'], keep)
    m = _t(keep.astype(np.float64) / np.float64(np.float32(1.0) - np.float32(p)))
    x = _t(inp['x'], True)
    y = x * m
    y.backward(_t(inp['dy']))
    np.testing.assert_allclose(ref['y'], y.detach().numpy(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(ref['dx'], x.grad.numpy(), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(ref['y'] != 0, keep)
    np.testing.assert_array_equal(ref['dx'] != 0, keep)
    if p == 0.5:
        np.testing.assert_array_equal(ref['y'], 2.0 * inp['x'] * keep)
