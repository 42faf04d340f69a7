"""tests/vgg_block_ref.py (the float64 reference of the VGG block passes that
tests/test_vgg_block_gpu.py holds the HIP kernels to) against torch float64:
F.relu -> F.max_pool2d(return_indices) on the [B, C, F, T] view -> F.batch_norm
-> dropout mask, and autograd for every gradient.  Agreement is at float64
rounding: a tensor may differ by TOL_ULPS x eps64 x (terms summed into an
element) x (its largest magnitude).  Also: the pool extents against torch's
output shapes, the bf16 rounding against torch.bfloat16, the dropout mask
against oracle.rng, and the float32 error constants of every GPU case (printed;
DESIGN.md holds the table)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import vgg_block_ref as R
from oracle import rng

EPS64 = float(np.finfo(np.float64).eps)
TOL_ULPS = 8


def _close(got, ref, terms, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    tol = TOL_ULPS * EPS64 * terms * max(float(np.abs(ref).max()), 1.0)
    err = float(np.abs(got - ref).max())
    assert err <= tol, (what, err, tol)


def _torch_block(c, training, mask):
    """Forward and autograd of case c in torch float64 on the NCHW view."""
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    z = t64(c['z']).requires_grad_(True)                    # [B, T, F, C]
    x = Fn.relu(z.permute(0, 3, 2, 1))                      # [B, C, F, T]
    pt, pf = c['pt'], c['pf']
    slot = None
    if pt:
        x, idx = Fn.max_pool2d(x, (pf, pt), (pf, pt), 0, 1, bool(c['ceil_mode']), True)
        f, t = idx // c['T'], idx % c['T']
        fo = torch.arange(x.shape[2]).view(1, 1, -1, 1)
        to = torch.arange(x.shape[3]).view(1, 1, 1, -1)
        slot = ((f - fo * pf) * pt + (t - to * pt)).permute(0, 3, 2, 1).numpy().astype(np.uint8)
    P = x
    gamma = beta = rm = rv = None
    if c['gamma'] is not None:
        gamma, beta = t64(c['gamma']).requires_grad_(True), t64(c['beta']).requires_grad_(True)
        rm, rv = t64(c['run_mean']).clone(), t64(c['run_var']).clone()
        x = Fn.batch_norm(x, rm, rv, gamma, beta, training, c['momentum'], c['eps'])
    out = x.permute(0, 3, 2, 1)                             # [B, T', F', C]
    if mask is not None:
        out = out * t64(mask)
    (out * t64(c['dnext'])).sum().backward()
    g = lambda v: None if v is None else v.grad.numpy()
    return dict(P=P.permute(0, 3, 2, 1).detach().numpy(), slot=slot, out=out.detach().numpy(),
                run_mean=None if rm is None else rm.numpy(), run_var=None if rv is None else rv.numpy(),
                dz=z.grad.numpy(), dgamma=g(gamma), dbeta=g(beta))


POOLS = [(0, 0, 0), (2, 2, 0), (2, 2, 1), (2, 3, 1), (3, 2, 0), (3, 3, 1)]
SIZES = [(6, 8), (7, 5), (9, 10), (8, 7)]      # (T, F): even / odd in either place


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('bn,drop', [(True, 0.0), (False, 0.0), (True, 0.3), (False, 0.3)])
@pytest.mark.parametrize('pt,pf,ceil_mode', POOLS)
@pytest.mark.parametrize('T,F', SIZES)
def test_reference_matches_torch_float64(T, F, pt, pf, ceil_mode, bn, drop, training):
    # z on the 1/8 grid (exact ties in most windows); channel 0 has no positive
    # value at all (every window all-negative: P = 0, slot 0, no gradient)
    c = R.make_case(2, T, F, 3, pt, pf, ceil_mode, bn=bn, training=training, drop=drop,
                    seed=77 + T, dead_channel=True, data_seed=T * 16 + F)
    n = 2 * c['To'] * c['Fo']
    fw = R.block_forward(c['z'], pt, pf, ceil_mode, c['gamma'], c['beta'], c['run_mean'],
                         c['run_var'], training, c['momentum'], c['eps'], drop, c['seed'])
    tb = _torch_block(c, training, fw['mask'])
    assert np.array_equal(fw['P'], tb['P'])
    if pt:
        assert np.array_equal(fw['slot'], tb['slot'])
        # channel 0: every window is an exact tie of zeros, the first pixel wins
        assert not fw['slot'][..., 0].any()
    assert not fw['P'][..., 0].any()
    _close(fw['out'], tb['out'], n, 'out')
    if bn:
        _close(fw['run_mean'], tb['run_mean'], n, 'run_mean')
        _close(fw['run_var'], tb['run_var'], n, 'run_var')
        if not training:
            assert np.array_equal(fw['run_mean'], c['run_mean'])
            assert np.array_equal(fw['run_var'], c['run_var'])
    bw = R.block_backward(c['dnext'], fw['P'], fw['slot'], T, F, pt, pf, c['gamma'], fw['mean'],
                          fw['rstd'], fw['mask'], training)
    _close(bw['dz'], tb['dz'], n, 'dz')
    _close(bw['dbias'], tb['dz'].reshape(-1, 3).sum(0), 2 * T * F * n, 'dbias')
    if bn:
        _close(bw['dgamma'], tb['dgamma'], n, 'dgamma')
        _close(bw['dbeta'], tb['dbeta'], n, 'dbeta')
    # pixels no window covers get exactly zero
    cov = R.covered(T, F, pt, pf, ceil_mode)
    assert not bw['dz'][:, ~cov].any()
    if pt and not ceil_mode and (T % pt or F % pf):
        assert (~cov).any()


@pytest.mark.parametrize('ceil_mode', [0, 1])
@pytest.mark.parametrize('k', [2, 3])
def test_pool_dims_match_torch(k, ceil_mode):
    for T in range(1, 13):
        for F in range(1, 13):
            for pt, pf in ((k, k), (k, 5 - k)):
                To, Fo = R.pool_dims(T, F, pt, pf, ceil_mode)
                try:
                    s = Fn.max_pool2d(torch.zeros(1, 1, F, T), (pf, pt), (pf, pt), 0, 1,
                                      bool(ceil_mode)).shape
                except RuntimeError:      # torch refuses an empty output
                    assert To <= 0 or Fo <= 0, (T, F, pt, pf)
                    continue
                assert (Fo, To) == tuple(s[2:]), (T, F, pt, pf, ceil_mode)


def test_bf16_round_matches_torch():
    r = np.random.RandomState(0)
    x = np.concatenate([r.randn(4096).astype(np.float32) * 10.0 ** r.randint(-6, 6, 4096),
                        # exact ties (odd and even neighbours), zeros, bf16 values
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 1.5, 3.0e38,
                                  1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9], np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.bf16_round(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.bf16_bits(got), (want.view(np.uint32) >> 16).astype(np.uint16))
    y = r.randn(2, 3, 4, 5).astype(np.float32)
    assert np.array_equal(R.unpad(R.pad(y)), y)
    p = R.pad(y)
    assert p.shape == (2, 5, 6, 5) and not p[:, 0].any() and not p[:, :, -1].any()


def test_dropout_mask_is_oracle_rng_and_shared_by_backward():
    c = R.make_case(2, 7, 6, 8, 2, 2, 1, drop=0.3, seed=R.SEED)
    fw, bw = R.reference(c)
    m = rng.dropout_scale(R.SEED, (2, c['To'], c['Fo'], 8), 0.3)
    assert np.array_equal(fw['mask'], m)
    assert 0 < (m == 0).sum() < m.size
    assert set(np.unique(m)) == {np.float32(0), np.float32(1) / np.float32(1 - np.float32(0.3))}
    assert not fw['out'][m == 0].any()
    # a dropped output passes no gradient: with dnext zeroed at the KEPT
    # elements nothing is left, so backward used the forward's mask
    c2 = dict(c, dnext=np.where(m == 0, c['dnext'], 0).astype(np.float32))
    _, bw2 = R.reference(c2)
    assert not bw2['dz'].any() and not bw2['dbeta'].any() and bw['dz'].any()


@pytest.mark.parametrize('cc', R.GPU_CASES, ids=[cc['id'] for cc in R.GPU_CASES])
def test_float32_constants_of_gpu_cases(cc):
    """The float32-versus-float64 error of the block formulas on each GPU case
    (sequential float32 sums; the shifted variance where the kernels use it):
    the GPU bounds are MARGIN x these.  Sanity: no constant exceeds the
    worst-case bound of a sequential float32 sum over the case's rows, times
    the cancellation (1 + (far / 1)^2) of a shifted variance centred `far`
    standard deviations off."""
    c, k, shifted = R.gpu_case(cc)
    keys = ('out', 'dz', 'dbias') + (R.STAT_KEYS + ('dgamma', 'dbeta') if c['gamma'] is not None else ())
    assert set(k) == set(keys)
    print('CONST %-28s %s %s' % (cc['id'], 'shifted ' if shifted else 'two-pass',
                                 ' '.join('%s=%.2e' % (n, k[n]) for n in keys)))
    nsum = c['B'] * c['T'] * c['F']
    cancel = 1.0 + cc['kw'].get('far', 0.0) ** 2
    for n in keys:
        assert R.CONST_FLOOR <= k[n] <= nsum * R.F32_EPS * cancel, (n, k[n])
