"""tests/ctc_beam_stream_ref.py against tests/ctc_beam_lm_ref.search, without a
GPU: the chunked restatement equals the whole-utterance one for every chunking
the device tests use, in f32 and f64; the stable length never decreases and the
stable prefix is a prefix of every later best hypothesis and of the final one;
the tie input has a tie at the pruning boundary; the recreation input reports
`recreated`; and which model-level inputs clear their score-gap margins (at
least one model per compute type must)."""
import numpy as np
import pytest

import ctc_beam_lm_cases as C
import ctc_beam_lm_ref as R
import ctc_beam_stream_ref as SR
import ctc_stream_ref as M

LM = dict(layers=1, H=8, Y=4)


def _row_sizes(name, b):
    return [int(take[b]) for take in SR.chunkings()[name]]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('chunking', ['whole', 'ones', 'split'])
@pytest.mark.parametrize('V,W,alpha,beta', [(6, 2, 0.0, 0.0), (6, 8, 0.7, -0.5), (29, 8, 0.0, 0.8),
                                            (29, 64, 0.7, 0.0)])
def test_chunked_equals_whole(V, W, alpha, beta, chunking, dtype):
    x = SR.logits(V)
    lm = R.make_lm(11, V, LM['layers'], LM['H'], LM['Y']) if alpha > 0 else None
    for b, n in enumerate(SR.LENS):
        want = R.search(x[b, :n], W, 0, lm, alpha, beta, dtype)
        s, trace = SR.run_chunked(x[b], n, _row_sizes(chunking, b), beam_width=W, lm_params=lm,
                                  alpha=alpha, beta=beta, dtype=dtype)
        hyp, score = s.best(final=True)
        np.testing.assert_array_equal(hyp, want['hyp'])
        assert score == want['score']
        assert s.prune_gap == want['prune_gap']
        # the stable prefix: monotone, and a prefix of every later best and of the final one
        stable = [st for _, st in trace]
        assert all(a <= b_ for a, b_ in zip(stable, stable[1:])), stable
        for i, (_, st) in enumerate(trace):
            for later, _ in trace[i:]:
                np.testing.assert_array_equal(later[:st], trace[i][0][:st])
            np.testing.assert_array_equal(hyp[:st], trace[i][0][:st])
        assert stable[-1] <= len(hyp)


def test_the_tie_input_has_a_tie_at_the_pruning_boundary():
    x = SR.tie_logits()
    tied = [R.search(x[b, :n], 8, 0, None, 0.0, 0.0, np.float32, normalize=False)['prune_gap'] == 0
            for b, n in enumerate(SR.LENS)]
    assert any(tied), tied
    for b, n in enumerate(SR.LENS):
        want = R.search(x[b, :n], 8, 0, None, 0.0, 0.0, np.float32, normalize=False)
        s, _ = SR.run_chunked(x[b], n, [1] * n, beam_width=8, dtype=np.float32, normalize=False)
        np.testing.assert_array_equal(s.best(final=True)[0], want['hyp'])


def test_the_identity_input_recreates_a_prefix():
    assert C.ref('identity')[0]['recreated']


def test_model_inputs_clear_their_margins():
    """Which (model, LM) configurations the model-level GPU test may compare with
    decode(): at least one per compute type; the others are compared with the
    search on the session's own logits only."""
    configs = [(name, False) for name in sorted(M.MODELS)] + [(SR.LM_MODEL, True)]
    for precision in ('fp32', 'bf16'):
        n_ok = 0
        for name, with_lm in configs:
            ok = SR.qualifies(name, precision, with_lm)
            for b, (pg, fg, n, hyp) in enumerate(SR.model_gaps(name, with_lm)):
                print('%s[%d] %s lm=%d: prune_gap %.3e final_gap %.3e, 4 x perturbation %.3e, '
                      'hyp %s: %s' % (name, b, precision, with_lm, pg, fg,
                                      4 * SR.score_perturbation(name, precision, n), hyp.tolist(),
                                      'qualifies' if ok[b] else 'own logits only'))
            n_ok += all(ok)
        assert n_ok >= 1, precision
