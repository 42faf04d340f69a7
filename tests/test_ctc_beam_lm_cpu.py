"""CPU-only checks of the float64 restatement of the CTC prefix beam search with
a language model (tests/ctc_beam_lm_ref.py): alpha = beta = 0 against
ctc_beam_ref.beam_search, the score against the sum over all alignments where
nothing is pruned, and the qualification of the GPU cases
(tests/ctc_beam_lm_cases.py): every gap >= GAP for ALL of them, and each case's
score_tol from the restatement's own f32 evaluation."""
import numpy as np
import pytest

import ctc_beam_lm_cases as C
import ctc_beam_lm_ref as R
import ctc_beam_ref as R0


@pytest.mark.parametrize('V,W,blank', [(3, 2, 0), (6, 4, 5), (29, 10, 0), (29, 1, 3)])
def test_zero_weights_is_the_plain_search(V, W, blank):
    for seed in range(3):
        x = (np.random.RandomState(100 + seed).randn(10, V) * 3).astype(np.float32)
        lm = R.make_lm(seed, V, 1, 8, 4)
        a = R.search(x, W, blank, lm, 0.0, 0.0)
        b = R0.beam_search(R0.log_softmax(x), W, blank)
        np.testing.assert_array_equal(a['hyp'], b['hyp'])
        assert abs(a['score'] - b['score']) < 1e-12
        assert abs(a['prune_gap'] - b['prune_gap']) < 1e-9 or a['prune_gap'] == b['prune_gap']


@pytest.mark.parametrize('alpha,beta,lm_shape', [(0.5, 0.0, (1, 8, 4)), (0.0, 0.7, None),
                                                 (0.8, -0.4, (2, 32, 16))])
def test_score_is_the_bruteforce_sum_without_pruning(alpha, beta, lm_shape):
    """V 3, T 5, W 64: at most 63 prefixes, nothing is dropped."""
    for seed in range(3):
        blank = seed % 3
        x = (np.random.RandomState(40 + seed).randn(5, 3) * 2).astype(np.float32)
        lm = R.make_lm(seed, 3, *lm_shape) if lm_shape else None
        r = R.search(x, 64, blank, lm, alpha, beta)
        assert r['prune_gap'] == float('inf')
        exact = R.score_bruteforce(R0.log_softmax(x), lm, r['hyp'], alpha, beta, blank)
        assert abs(r['score'] - exact) < 1e-10
        # and no other prefix of up to 2 labels scores higher
        for other in [(), (0,), (1,), (2,), (0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]:
            if blank in other:
                continue
            assert R.score_bruteforce(R0.log_softmax(x), lm, other, alpha, beta, blank) \
                <= r['score'] + 1e-10


def test_lm_changes_the_result():
    """At least one case's hypotheses differ from the search without the terms."""
    differ = 0
    for name in ('v29_w20', 'v29_w20_b5', 'v29_beta_pos'):
        case = C.CASES[name]
        x, lens, _ = C.draw(case, C.SEEDS[name])
        for b, r in enumerate(C.ref(name)):
            plain = R.search(x[b, :lens[b]], case['W'], case['blank'])
            differ += not np.array_equal(plain['hyp'], r['hyp'])
    assert differ >= 3


@pytest.mark.parametrize('name', list(C.CASES) + ['identity'])
def test_case_qualifies(name):
    r64, r32 = C.ref(name, True), C.ref(name, False)
    for b, (a, r) in enumerate(zip(r32, r64)):
        print('ctc_beam_lm %s[%d]: final gap %.3e, pruning gap %.3e, score f64 %.9f f32 %.9f'
              % (name, b, r['final_gap'], r['prune_gap'], r['score'], a['score']))
        assert r['final_gap'] >= C.GAP and r['prune_gap'] >= C.GAP, (name, b)
        np.testing.assert_array_equal(a['hyp'], r['hyp'])
    print('ctc_beam_lm %s: score_tol %.3e' % (name, C.score_tol(name)))
    assert np.isfinite(C.score_tol(name))
    if name == 'identity':
        assert r64[0]['recreated']


def test_case_list_covers_the_dispatch():
    Vs = set(c['V'] for c in C.CASES.values())
    Ws = set(c['W'] for c in C.CASES.values())
    assert {2, 3, 29, 128, 129, 1000} <= Vs and {1, 2, 20, 64} <= Ws
    assert all(c['T'] <= 12 and len(c['lens']) == 3 for c in C.CASES.values())
    lens = set(l for c in C.CASES.values() for l in c['lens'])
    assert {0, 1} <= lens
    assert any(c['lm'] and c['lm'][0] == C.MAX_LAYERS for c in C.CASES.values())
    assert any(c['blank'] != 0 for c in C.CASES.values())


def test_symbols_and_workspace():
    from pytorch_end2end_speech_recognition_amd import _native as N
    for name in ('asr_ctc_beam_search_lm', 'asr_ctc_beam_lm_ws_bytes'):
        assert hasattr(N.lib(), name)
    assert N.ATT_BEAM_LM_MAX_LAYERS == C.MAX_LAYERS
    q = (12, 3, 29, 20)
    no_lm = N.query('asr_ctc_beam_lm_ws_bytes', *(q + (0, 0, 0)))
    lm = N.query('asr_ctc_beam_lm_ws_bytes', *(q + (2, 32, 16)))
    # LM state h and c [2][B][W][layers][H] and the row cache [2][B][W][V]
    assert lm - no_lm == 2 * (2 * 3 * 20 * 2 * 32 * 4) + 2 * 3 * 20 * 29 * 4
    assert N.query('asr_ctc_beam_lm_ws_bytes', *(q + (C.MAX_LAYERS + 1, 32, 16))) == 0
    assert N.query('asr_ctc_beam_lm_ws_bytes', *(q + (1, 6000, 16))) == 0
    assert N.query('asr_ctc_beam_lm_ws_bytes', 12, 3, 29, 65, 1, 8, 4) == 0


def test_refusals_need_no_device():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.decoders.beam_search_decoder \
        import BeamSearchDecoder

    class _LM(object):
        num_classes = 7

    with pytest.raises(ValueError):
        BeamSearchDecoder.check_lm(-0.1, 0.0, _LM(), 7)
    with pytest.raises(ValueError):
        BeamSearchDecoder.check_lm(0.3, 0.0, None, 7)
    with pytest.raises(ValueError):
        BeamSearchDecoder.check_lm(0.3, 0.0, _LM(), 6)
    with pytest.raises(ValueError):
        BeamSearchDecoder.check_lm(0.0, float('nan'), None, 6)
    BeamSearchDecoder.check_lm(0.0, 0.5, None, 6)
    BeamSearchDecoder.check_lm(0.3, 0.5, _LM(), 7)
