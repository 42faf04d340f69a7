"""tests/ctc_width_ref.py (the float64 reference and bounds that
tests/test_ctc_widths_gpu.py holds the CTC gradient kernels to), checked with
the reference alone: the gradient against finite differences of the float64
cost, the float32 restatement against the oracle's own formulas and within
its printed constant, every GPU case feasible with a finite cost, and every
bound small against the label columns it has to resolve."""
import numpy as np
import pytest

import ctc_width_ref as R
import vgg_block_ref as VR
from oracle import ctc_ref

CASES = R.cases()
IDS = [c['id'] for c in CASES]


def test_gradient_matches_finite_differences_v7():
    """dy_ref's formula (ctc_batch x scale; db its sum over (b, t)) on a V = 7
    case with a repeat and ragged lengths: central differences of the scaled
    float64 cost, step 1e-5 (truncation ~1e-10, rounding ~1e-10 on costs ~10)."""
    rng = np.random.RandomState(5)
    B, T, V = 2, 6, 7
    acts = rng.randn(B, T, V) * 2
    labels, label_lens, act_lens = np.array([3, 3, 6, 1]), np.array([3, 1]), np.array([6, 4])
    scale = R.LOSS_SCALE * R.GRAD_SCALE

    def loss(a):
        return scale * ctc_ref.ctc_batch(a, labels, label_lens, act_lens, time_major=False)[0].sum()

    costs, g = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    assert np.all(np.isfinite(costs)) and np.all(costs > 0)
    dy = g * scale
    h = 1e-5
    fd = np.zeros_like(acts)
    for i in np.ndindex(*acts.shape):
        ap, am = acts.copy(), acts.copy()
        ap[i] += h
        am[i] -= h
        fd[i] = (loss(ap) - loss(am)) / (2 * h)
    assert np.abs(fd - dy).max() <= 1e-8, np.abs(fd - dy).max()
    assert np.all(dy[1, 4:] == 0)
    np.testing.assert_allclose(dy.sum(axis=(0, 1)), fd.sum(axis=(0, 1)), atol=1e-7)


def test_dtype_restatement_is_the_oracles_formula():
    """ctc_single_dtype in float64 is ctc_ref.ctc_single (so its float32 run
    measures float32 evaluation of the same formulas, nothing else)."""
    c = R.case(2051)
    off = 0
    for b in range(c['B']):
        L, Tb = int(c['label_lens'][b]), int(c['act_lens'][b])
        lab = c['labels'][off:off + L]
        off += L
        c0, g0 = ctc_ref.ctc_single(c['logits'][b, :Tb], lab, c['blank'])
        c1, g1 = R.ctc_single_dtype(c['logits'][b, :Tb], lab, c['blank'], np.float64)
        assert abs(c0 - c1) <= 1e-12 * abs(c0)
        assert np.abs(g0 - g1).max() <= 1e-14


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_case_is_feasible_and_bound_resolves_label_columns(c):
    costs = R.costs_ref(c)
    dy64, db64 = R.dy_ref(c)
    dy32, db32 = R.dy_f32(c)
    tol_dy, tol_db, k = R.bound(c)
    print('CONST %-18s dy=%.2e db=%.2e  costs %s' % (
        c['id'], k['dy'], k['db'], ' '.join('%.1f' % x for x in costs)))
    # shape of the case: what the GPU file relies on
    V, blank = c['V'], c['blank']
    assert c['logits'].shape == (c['B'], c['T'], V) and c['logits'].dtype == np.float32
    assert int(c['label_lens'].max()) == c['max_label_len'] and blank not in c['labels']
    lab0 = c['labs'][0]
    assert any(a == b for a, b in zip(lab0, lab0[1:]))                       # adjacent repeat
    assert any(a // 8 == b // 8 and a != b for a, b in zip(lab0, lab0[1:]))  # one 8-column chunk
    assert (V - 1 if blank != V - 1 else V - 2) in lab0                      # the last class
    # feasible, finite cost
    assert np.all(np.isfinite(costs)) and np.all(costs > 0), costs
    f32_costs = R._f32(R._key(c))[0]
    np.testing.assert_allclose(f32_costs, costs, rtol=1e-4)
    # the float32 evaluation stays within its own constant, and the constant
    # is a float32 rounding figure: at most the worst case of T lattice steps
    # each rounding a log-probability of the cost's magnitude (an occupancy is
    # exp(alpha + beta - emit - log P)), and below a bf16 ulp
    assert VR.nerr(dy32, dy64) <= k['dy'] and VR.nerr(db32, db64) <= k['db']
    cap = min(c['T'] * VR.F32_EPS * float(costs.max()), 2.0 ** -8)
    assert k['dy'] <= cap and k['db'] <= cap, (k, cap)
    for b in range(c['B']):
        assert np.all(dy64[b, c['act_lens'][b]:] == 0)
    # the bound cannot hide a wrong class sum: on a label column, wherever the
    # occupancy exceeds 0.1, it is below 1/16 of |ref|
    scale = c['loss_scale'] * c['grad_scale']
    nres = 0
    for b, cl, occ in R.label_occupancy(c):
        Tb = len(occ)
        hot = occ > 0.1
        assert hot.any(), (b, cl)
        ref = np.abs(dy64[b, :Tb, cl][hot])
        assert np.all(tol_dy[b, :Tb, cl][hot] < ref / 16), (b, cl, tol_dy[b, :Tb, cl][hot], ref)
        nres += int(hot.sum())
    # ... and db on the label classes of utterance 0 (each sums at least one
    # such frame): the bound is below 1/16 of |db|
    for cl in set(int(x) for x in c['labs'][0]):
        assert tol_db < abs(db64[cl]) / 16, (cl, tol_db, db64[cl])
    assert nres >= len(c['labels'])
    assert scale == pytest.approx(2.0 / 3.0)
