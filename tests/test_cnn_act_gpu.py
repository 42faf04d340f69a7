"""The activation -> pool -> batch norm -> dropout block of csrc/cnn_act.hip
(PReLU, hard-tanh(0, 20); forward and backward) against the float64 reference
tests/cnn_taps_ref.block, through the C entry points.

Cases: PReLU with slope 0.2 and with a negative slope, hard-tanh on inputs
from below 0 to above 20; no pool, a floor pool and ceil pools over odd extents
(partial windows); batch norm in training and in eval, and none (conv bias
gradient); dropout; haloed f32 / bf16 and flat outputs.  In the 'neg-window'
case the last time row is all negative, so the partial ceil-mode window over it
holds only negative activations: its maximum must be that negative value, not 0.

Tolerances are those of the ReLU block's float64 tests
(tests/test_vgg_block_gpu.py:61, _check): MARGIN (16) x the float32-evaluation
error of the same formulas on the same inputs x max |reference|, plus one bf16
ulp (2^-8 |ref|) for a bf16 output.  The backward is given the kernel's own
P / slot / mean / rstd.  Two backward runs must be bitwise equal (every sum is
taken in a fixed order), the PReLU slope gradient included.
"""
import numpy as np
import pytest
import torch

import cnn_taps_ref as R
import vgg_block_ref as VR

BF16, F32 = 1, 0
RELU, PRELU, HTANH = R.ACT_RELU, R.ACT_PRELU, R.ACT_HARDTANH

# name: act, slope, (pt, pf, ceil), bn (None / 'train' / 'eval'), drop, out ('halo' / 'bf16' / 'flat'), C
CASES = {
    'prelu-nopool-bn': (PRELU, 0.2, (0, 0, 0), 'train', 0.0, 'halo', 16),
    'prelu-floor-bn': (PRELU, 0.2, (2, 3, 0), 'train', 0.0, 'bf16', 16),
    'prelu-neg-window': (PRELU, 0.2, (2, 2, 1), 'train', 0.0, 'flat', 16),
    'prelu-negslope-ceil': (PRELU, -0.3, (2, 2, 1), 'train', 0.2, 'halo', 24),
    'prelu-eval-bn': (PRELU, 0.2, (1, 3, 1), 'eval', 0.0, 'flat', 16),
    'prelu-nobn': (PRELU, -0.3, (2, 1, 0), None, 0.0, 'halo', 16),
    'htanh-ceil-bn': (HTANH, 0.0, (2, 2, 1), 'train', 0.0, 'halo', 16),
    'htanh-nobn-drop': (HTANH, 0.0, (0, 0, 0), None, 0.2, 'flat', 16),
    'htanh-eval-floor': (HTANH, 0.0, (2, 2, 0), 'eval', 0.0, 'bf16', 16),
    'relu-ceil-bn': (RELU, 0.0, (2, 2, 1), 'train', 0.0, 'halo', 16),
}
B, T, F = 2, 7, 5      # odd extents: every ceil pool has partial windows; 70 pixels
SEED = 0x5EED1234


def _case(name):
    act, slope, (pt, pf, ceil), bn, drop, outk, C = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    z = rng.randn(B, T, F, C).astype(np.float32)
    if act == HTANH:
        z = (z * 12 + 8).astype(np.float32)       # spans below 0 and above 20
    if name == 'prelu-neg-window':
        z[:, T - 1] = -np.abs(z[:, T - 1]) - 0.1   # the partial window's values are all negative
    To, Fo = R.pool_dims(T, F, pt, pf, ceil)
    c = dict(z=z, act=act, slope=np.float32(slope), pt=pt, pf=pf, ceil=ceil, bn=bn, drop=drop,
             outk=outk, C=C, To=To, Fo=Fo, gamma=None, beta=None, run_mean=None, run_var=None)
    if bn:
        c['gamma'] = (1 + 0.2 * rng.randn(C)).astype(np.float32)
        c['beta'] = (0.2 * rng.randn(C)).astype(np.float32)
        c['run_mean'] = (0.1 * rng.randn(C)).astype(np.float32)
        c['run_var'] = (1 + 0.2 * rng.rand(C)).astype(np.float32)
    c['dnext'] = rng.randn(B, To, Fo, C).astype(np.float32)
    c['mask'] = VR.drop_mask(SEED, (B, To, Fo, C), drop)
    return c


def _ref_args(c):
    return (c['z'], c['act'], c['slope'], c['pt'], c['pf'], c['ceil'], c['gamma'], c['beta'],
            c['run_mean'], c['run_var'], c['bn'] != 'eval', 0.1, 1e-5, c['mask'], c['dnext'])


def _padded(vals, shape, dev, dtype=torch.float32):
    """[B, t + 2, f + 2, C]: `vals` (None: NaN) inside a zero halo."""
    Bc, t, f, C = shape
    out = torch.zeros(Bc, t + 2, f + 2, C, dtype=dtype, device=dev)
    out[:, 1:-1, 1:-1] = (float('nan') if vals is None else
                          torch.from_numpy(np.ascontiguousarray(vals)).to(dev).to(dtype))
    return out


def _run(c, dev, nbwd=1):
    from pytorch_end2end_speech_recognition_amd import _native as N
    C, To, Fo, pt = c['C'], c['To'], c['Fo'], c['pt']
    d = lambda a: None if a is None else torch.from_numpy(np.array(a, np.float32)).to(dev)
    z = _padded(c['z'], (B, T, F, C), dev)
    slope = d(np.reshape(c['slope'], (1,)))
    P = torch.full((B, To, Fo, C), float('nan'), device=dev)
    slot = torch.zeros(B * To * Fo * C, dtype=torch.uint8, device=dev) if pt else None
    gamma, beta, rm, rv = d(c['gamma']), d(c['beta']), d(c['run_mean']), d(c['run_var'])
    bn = c['bn'] is not None
    mean = torch.full((C,), float('nan'), device=dev) if bn else None
    rstd = torch.full((C,), float('nan'), device=dev) if bn else None
    flat = int(c['outk'] == 'flat')
    odt = torch.bfloat16 if c['outk'] == 'bf16' else torch.float32
    out = (torch.full((B, To, Fo, C), float('nan'), device=dev) if flat else
           _padded(None, (B, To, Fo, C), dev, odt))
    nb = N.query('asr_cnn_act_workspace_bytes', B, T, F, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = N.stream_handle(dev)
    training = int(c['bn'] != 'eval')
    N.call('asr_cnn_act_forward', N.ptr(z), B, T, F, C, c['act'], N.ptr(slope), pt, c['pf'],
           c['ceil'], N.ptr(P), N.ptr(slot), N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv),
           training, 0.1, 1e-5, N.ptr(mean), N.ptr(rstd), c['drop'], SEED, N.ptr(out),
           BF16 if odt == torch.bfloat16 else F32, flat, N.ptr(ws), nb, st)
    res = dict(P=P, out=out, mean=mean, rstd=rstd, run_mean=rm, run_var=rv)
    # backward: dnext haloed (as a convolution's input gradient arrives) unless the output was flat
    dnext = d(c['dnext']) if flat else _padded(c['dnext'], (B, To, Fo, C), dev)
    bw = []
    for _ in range(nbwd):
        dz = _padded(None, (B, T, F, C), dev)
        base = 0.5
        dgamma = torch.full((C,), base, device=dev) if bn else None
        dbeta = torch.full((C,), base, device=dev) if bn else None
        dbias = torch.full((C,), base, device=dev)
        dslope = torch.full((1,), base, device=dev)
        N.call('asr_cnn_act_backward', N.ptr(dnext), flat, N.ptr(z), B, T, F, C, c['act'],
               N.ptr(slope), pt, c['pf'], c['ceil'], N.ptr(P), N.ptr(slot), N.ptr(gamma),
               N.ptr(mean), N.ptr(rstd), training, N.ptr(dgamma), N.ptr(dbeta), c['drop'], SEED,
               N.ptr(dz), F32, N.ptr(dbias), N.ptr(dslope), N.ptr(ws), nb, st)
        bw.append(dict(dz=dz, dgamma=dgamma, dbeta=dbeta, dbias=dbias, dslope=dslope))
    torch.cuda.synchronize()
    np64 = lambda t: None if t is None else t.detach().to(torch.float64).cpu().numpy()
    res = {k: np64(v) for k, v in res.items()}
    bw = [{k: np64(v) for k, v in b.items()} for b in bw]
    return res, bw, 0.5


def _check(what, got, ref, const, fails, bf16=False):
    """tests/test_vgg_block_gpu.py:61: |got - ref| <= MARGIN const scale (+ a bf16 ulp)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = VR.MARGIN * const * VR.scale_of(ref) + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)
    err = np.abs(got - ref)
    worst = float(np.max(err / tol))
    print('  %-9s err/bound %.3f  (max err %.3e, const %.2e)' % (what, worst, float(err.max()),
                                                                const))
    if not np.isfinite(worst) or worst > 1.0:
        fails.append((what, worst))


@pytest.fixture(scope='module')
def refs():
    """Each case's inputs, float64 reference and float32 constants, computed once."""
    out = {}
    for name in CASES:
        c = _case(name)
        out[name] = (c,) + R.block_constants(_ref_args(c))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_cnn_act_block_vs_float64(name, refs, cuda_dev):
    c, ref, k = refs[name]
    res, bw, base = _run(c, cuda_dev, nbwd=2)
    fails = []
    interior = lambda a: a[:, 1:-1, 1:-1]
    _check('P', res['P'], ref['P'], k['P'], fails)
    out = res['out'] if c['outk'] == 'flat' else interior(res['out'])
    _check('out', out, ref['out'], k['out'], fails, bf16=c['outk'] == 'bf16')
    if c['bn']:
        for s in ('mean', 'rstd'):
            _check(s, res[s], ref[s], k[s], fails)
    if c['bn'] == 'train':
        for s in ('run_mean', 'run_var'):
            _check(s, res[s], ref[s], k[s], fails)
    b0 = bw[0]
    _check('dz', interior(b0['dz']), ref['dz'], k['dz'], fails)
    _check('dbias', b0['dbias'] - base, ref['dbias'], k['dbias'], fails)
    if c['bn']:
        _check('dgamma', b0['dgamma'] - base, ref['dgamma'], k['dgamma'], fails)
        _check('dbeta', b0['dbeta'] - base, ref['dbeta'], k['dbeta'], fails)
    if c['act'] == PRELU:
        _check('dslope', b0['dslope'] - base, ref['dslope'], k['dslope'], fails)
    else:
        assert b0['dslope'][0] == base      # untouched without a slope
    assert not fails, fails
    if c['outk'] != 'flat':
        halo = res['out'].copy()
        halo[:, 1:-1, 1:-1] = 0
        assert not halo.any(), 'the forward wrote into the output halo'
    halo = b0['dz'].copy()
    halo[:, 1:-1, 1:-1] = 0
    assert not halo.any(), 'the backward wrote into the dz halo'
    for key in b0:
        if b0[key] is not None:
            assert np.array_equal(b0[key], bw[1][key]), '%s differs between two runs' % key


@pytest.mark.gpu
def test_partial_window_of_negative_values_keeps_its_maximum(refs, cuda_dev):
    """PReLU outputs can be negative: the ceil-mode window over the last (odd) time
    row holds only negative activations and must return their maximum -- the ReLU
    block's floor at 0 would be wrong here."""
    c, ref, _ = refs['prelu-neg-window']
    res, _, _ = _run(c, cuda_dev)
    last = res['P'][:, -1]
    assert (ref['P'][:, -1] < 0).all() and (last < 0).all()
    np.testing.assert_array_equal(last, ref['P'][:, -1].astype(np.float32).astype(np.float64))
