"""CTC prefix beam search, the parts that need no GPU: the float64 restatement
(ctc_beam_ref.py) against the reference's recorded hypotheses and against a
brute-force sum over alignments, the model of the device algorithm against
the restatement, and the presence of the decoder and its C entry points."""
import os

import numpy as np
import pytest

import ctc_beam_ref as R
from conftest import ROOT, golden


@pytest.fixture(scope='module')
def G():
    return golden('ctc_beam')


def _utterances(G):
    for name in [str(n) for n in G['names']]:
        x, lens = G[name + '/logits'], G[name + '/lens']
        for b in range(len(lens)):
            n = min(int(lens[b]), x.shape[1])
            yield name, b, x[b, :n], int(G[name + '/W']), int(G[name + '/blank'])


def test_recorded_cases_meet_the_gap_condition(G):
    names = [str(n) for n in G['names']]
    assert len(names) == 14                 # 6 shapes x 2, the ragged batch, the identity case
    for name in names:
        assert (G[name + '/final_gap'] >= 1e-3).all() and (G[name + '/prune_gap'] >= 1e-3).all()
    assert bool(G['identity/recreated'])
    assert 0 < float(G['score_tol']) < 1e-3


def test_restatement_reproduces_the_reference(G):
    for name, b, x, W, blank in _utterances(G):
        if len(x) == 0:
            assert len(G['%s/hyp%d' % (name, b)]) == 0
            continue
        assert not np.isnan(x).any()
        r = R.beam_search(R.log_softmax(x), W, blank)
        np.testing.assert_array_equal(r['hyp'], G['%s/hyp%d' % (name, b)], err_msg=name)
        assert abs(r['score'] - G[name + '/score'][b]) < 1e-9
        if name == 'identity':
            assert r['recreated']


def test_device_algorithm_model_matches_the_restatement(G):
    """The restricted candidate set with exact prefix identity gives the
    restatement's answer; with node ids for identity it fails the identity case."""
    for name, b, x, W, blank in _utterances(G):
        if len(x) == 0 or x.shape[1] > 300:
            continue
        lp = R.log_softmax(x)
        hyp, score = R.restricted_search(lp, W, blank)
        np.testing.assert_array_equal(hyp, G['%s/hyp%d' % (name, b)], err_msg=name)
        assert abs(score - G[name + '/score'][b]) < 1e-9
    lp = R.log_softmax(G['identity/logits'][0])
    hyp, score = R.restricted_search(lp, int(G['identity/W']), 0, exact_identity=False)
    assert (not np.array_equal(hyp, G['identity/hyp0']) or
            abs(score - G['identity/score'][0]) > 1e-2)


def test_bruteforce_agrees_without_pruning():
    """V 3, T 5, W 64: 63 prefixes at most, nothing is ever dropped, so the
    best prefix's score is its exact probability."""
    for seed in range(3):
        lp = R.log_softmax(np.random.RandomState(40 + seed).randn(5, 3) * 2)
        r = R.beam_search(lp, 64, blank=seed % 3)
        assert r['prune_gap'] == float('inf')
        assert abs(r['score'] - R.prefix_prob_bruteforce(lp, r['hyp'], seed % 3)) < 1e-12
        # and no other prefix of up to 2 labels is more probable
        for p in [(), (0,), (1,), (2,), (1, 2), (2, 1)]:
            if (seed % 3) not in p:
                assert R.prefix_prob_bruteforce(lp, p, seed % 3) <= r['score'] + 1e-12


def test_hand_made_merge_case():
    lp = np.log(np.array([[0.6, 0.4]] * 2))
    r = R.beam_search(lp, 2, 0)
    np.testing.assert_array_equal(r['hyp'], [1])
    assert abs(r['score'] - np.log(0.64)) < 1e-12


def test_decoder_and_entry_points_exist():
    from pytorch_end2end_speech_recognition_amd import _native
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc import decoders
    assert callable(decoders.BeamSearchDecoder(blank_index=0, space_index=-1))
    with pytest.raises(NotImplementedError):
        decoders.BeamSearchDecoder(0)(np.zeros((1, 2, 3), np.float32), [2], 2, alpha=0.5)
    header = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    for name in ('asr_ctc_beam_search', 'asr_ctc_beam_ws_bytes'):
        assert name in _native.SIGNATURES and name in header
