"""tests/ctc_paths_ref.py (the cases, float64 reference and bounds that
tests/test_ctc_paths_gpu.py holds the CTC forward and its float32 gradient
to), checked with the reference alone: the constants written into the module
are current, every label class is occupied, the reference is shift-invariant
and finite on masked logits, the host-built slab partials recombine to the
float64 log-sum-exp, and each of five mistakes a kernel could make, applied to
the reference, exceeds the bound at least fourfold in some case."""
import numpy as np
import pytest

import ctc_paths_ref as R
import vgg_block_ref as VR
from oracle import ctc_ref

CASES = R.cases()
IDS = [c['id'] for c in CASES]


def test_every_case_has_constants():
    assert sorted(R.CONSTS) == sorted(IDS)
    assert set(R.WIDTHS) >= set(R.LAYOUT_WIDTHS)
    assert [R.nslab_of(V) for V in R.LSE_WIDTHS] == [1, 16, 17, 33]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_constants_are_current(c):
    """The (K_grad, K_cost) of CONSTS against a fresh measure(): the bounds they
    give differ by at most 2x either way."""
    kg, kc = R.measure(c)
    tg, tc = R.CONSTS[c['id']]
    print('    %-30s (%.3g, %.3g),' % (repr(c['id']) + ':', kg, kc))
    assert tg >= VR.CONST_FLOOR and tg / 2 <= kg <= tg * 2, (kg, tg)
    new, old = R.cost_tol_of(c, kc), R.cost_tol_of(c, tc)
    f = c['feasible']
    assert np.all(old[f] / 2 <= new[f]) and np.all(new[f] <= old[f] * 2), (kc, tc)
    # a float32 rounding figure: below T roundings of a log-probability of the
    # cost's magnitude (ctc_width_ref's cap), and far below the looser bound of
    # tests/test_ctc_gpu.py on the costs
    costs = R.costs_ref(c)
    cap = c['T'] * VR.F32_EPS * max(float(costs.max()), 1.0)
    assert tg <= cap, (tg, cap)
    big = f & (costs >= 1.0)    # (a relative bound says little on a cost near 0)
    assert np.all(old[big] <= 1e-4 * costs[big]), (old, costs)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_case_shape_and_occupancy(c):
    """What the GPU file relies on: the labels' shape, finite positive costs of
    the feasible utterances, zeros beyond the lengths, and every label class of
    every feasible utterance at occupancy >= 0.5 at some frame -- where the
    bound is below 1/16 of that occupancy, so it cannot hide a wrong class sum."""
    V, blank, B = c['V'], c['blank'], c['B']
    assert c['logits'].shape == (B, c['T'], V) and c['logits'].dtype == np.float32
    assert blank not in c['labels'] and int(c['label_lens'].max()) <= c['max_label_len']
    costs, g = R.costs_ref(c), R.grad_ref(c)
    f = c['feasible']
    assert np.all(np.isfinite(costs)) and np.all(costs[f] > 0) and np.all(costs[~f] == 0)
    assert np.all(np.isfinite(g))
    for b in range(B):
        assert np.all(g[b, c['act_lens'][b]:] == 0)
        if not f[b]:
            assert np.all(g[b] == 0)
    assert np.all(R.viterbi_cost(c)[f] >= costs[f])          # one alignment <= all of them
    if B == 3:
        lab0 = c['labs'][0]
        assert any(a == b for a, b in zip(lab0, lab0[1:]))                           # adjacent repeat
        assert (V - 1 if blank != V - 1 else V - 2) in lab0                          # the last class
        if V >= 5:
            assert any(a // 4 == b // 4 and a != b for a, b in zip(lab0, lab0[1:]))  # one quad
        assert f.tolist() == ([True, False, True] if 'infeasible' in c['id'] else [True] * 3)
    else:
        assert B == 300 and f.all() and sorted(set(c['label_lens'])) == [0, 1, 2]
        assert int(c['label_lens'].sum()) > 256                 # ctc_prep's label loop wraps
    tol_g, _ = R.bound(c)
    occs = R.label_occupancy(c)
    assert len(occs) >= int(f.sum()) - int((c['label_lens'] == 0).sum())
    for b, cl, occ in occs:
        assert occ.max() >= 0.5, (b, cl, occ.max())
        hot = occ >= 0.5
        Tb = len(occ)
        assert np.all(tol_g[b, :Tb, cl][hot] < occ[hot] / 16), (b, cl)


def test_oracle_restatement_is_the_oracle():
    """ctc_mutant(None) is ctc_ref.ctc_single (so a mutation measures that one
    mistake and nothing else)."""
    for c in (R.case(5), R.case(257), R.case(1025, blank=512)):
        c0, g0 = R.costs_ref(c), R.grad_ref(c)
        c1, g1 = R.mutant(c, None)
        assert np.abs(c0 - c1).max() <= 1e-12 * max(c0.max(), 1.0)
        assert np.abs(g0 - g1).max() <= 1e-14


@pytest.mark.parametrize('V', [257, 1025])
def test_reference_is_shift_invariant(V):
    c = R.case(V)
    x = c['logits'].astype(np.float64)
    c0, g0 = R.costs_ref(c), R.grad_ref(c)
    for s in R.SHIFTS:
        c1, g1 = ctc_ref.ctc_batch(x + s, c['labels'], c['label_lens'], c['act_lens'],
                                   blank=c['blank'], time_major=False)
        assert np.abs(c1 - c0).max() <= 1e-11 * c0.max()
        assert np.abs(g1 - g0).max() <= 1e-12
    for s in R.SHIFTS:   # the shifted cases hold the shift (rounded to float32 inputs)
        assert abs(float(np.median(R.case(V, shift=s)['logits'])) - s) < 1.0


@pytest.mark.parametrize('c', R.mask_cases() + [R.case(1025, mask='slab')],
                         ids=lambda c: c['id'])
def test_reference_is_finite_on_masked_logits(c):
    x = c['logits']
    cols = c['mask_cols']
    assert len(cols) and np.all(np.isneginf(x[:, :, cols]))
    other = np.ones(c['V'], bool)
    other[cols] = False
    assert np.all(np.isfinite(x[:, :, other]))
    costs, g = R.costs_ref(c), R.grad_ref(c)
    c32, g32 = R.eval_f32(c)
    for a in (costs, g, c32, g32):
        assert np.all(np.isfinite(a))
    assert np.all(g[:, :, cols] == 0) and np.all(g32[:, :, cols] == 0)
    if 'lead' in c['id']:
        # for each row phase h (floats before the first 16-B boundary) the row
        # head and the quads h + 4 q .. + 3 of q = 0, 1 (+ 256 k at V > 1024:
        # threads 0 and 1's whole first unrolled round) are masked
        for h in range(4):
            need = set(range(h))
            for q in (0, 1):
                for k in range(4 if c['V'] > 4096 else 1):
                    need |= set(range(h + 4 * (q + 256 * k), h + 4 * (q + 256 * k) + 4))
            assert need <= set(cols), h
    else:
        assert cols == list(range(192, 256))


@pytest.mark.parametrize('c', R.lse_cases(), ids=lambda c: c['id'])
def test_slab_partials_recombine_to_the_log_sum_exp(c):
    B, T, V = c['logits'].shape
    part = R.slab_partials(c)
    assert part.shape == (R.nslab_of(V), B * T, 2) and part.dtype == np.float32
    x = c['logits'].astype(np.float64).reshape(B * T, V)
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    live = np.concatenate([np.arange(T) < n for n in c['act_lens']])
    got = R.lse_from_partials(part)
    # each partial sum is rounded once to float32: 2^-24 relative in the sum
    assert np.abs(got - lse)[live].max() <= 2.0 ** -23
    assert np.all(np.isnan(part[:, ~live]))
    empty = np.isneginf(part[:, live, 0])
    assert np.all(part[:, live, 1][empty] == 0)
    assert empty.any() == ('slab' in c['id'])
    if 'slab' in c['id']:
        assert np.all(empty[3]) and not empty[:3].any() and not empty[4:].any()


SHARP_CASES = {
    'skip_across_repeat': [(5,), (257,), (1025,)],
    'last_class_not_normalised': [(5,), (257,), (1025,)],
    'slab_left_out': [(255,), (257,), (1025,)],
    'blank_states_not_folded': [(5,), (257,), (1025,)],
    'row_head_left_out': [(5,), (257,), (1025,)],
}


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_bounds_catch_the_mutation(mut):
    """A kernel with this mistake would exceed its bound at least fourfold in
    one of the cases (costs or gradient)."""
    worst = {}
    for key in SHARP_CASES[mut]:
        c = R.case(*key)
        costs, g = R.mutant(c, mut)
        worst[c['id']] = R.excess(c, costs, g)
    print('\n  %-28s %s' % (mut, '  '.join('%s %.3g' % kv for kv in worst.items())))
    assert max(worst.values()) >= 4.0, worst
    assert all(R.excess(R.case(*k), *R.mutant(R.case(*k), None)) <= 1e-3 for k in SHARP_CASES[mut])


def test_sum_bound_is_the_pure_summation_bound():
    costs = np.full(300, 3.0, np.float32)
    assert R.sum_bound(costs, 1.0 / 3.0) == pytest.approx(301 * 2.0 ** -24 * 300.0, rel=1e-4)
