"""CTC.stream(beam_width=4, ...) -- CTCBeamStream: RNNEncoder.forward_chunk over
csrc/lstm_stream.hip, then asr_ctc_beam_stream_feed -- on the seeded models of
tests/ctc_stream_ref.py, fed on their schedules in both compute types; the
'fast' model also with an RNNLM (alpha 0.5, beta 0.3).

The final hypotheses and scores equal native_ops.ctc_beam_search on the
session's own concatenated last_logits exactly.  A streamed and a
whole-utterance evaluation agree within ctc_stream_ref.logit_bound only, so
decode(beam_width=4, ...) is compared only for the inputs whose float64 pruning
and final gaps exceed 4 x the score perturbation that bound implies
(ctc_beam_stream_ref.qualifies; tests/test_ctc_beam_stream_ref_cpu.py prints the
table and asserts that one model per compute type qualifies); the number of
rows compared with the own-logits search only is printed.  Every test here
needs CTC.stream's beam_width."""
import numpy as np
import pytest
import torch

import ctc_beam_stream_ref as SR
import ctc_stream_ref as M
import lstm_stream_ref as S

pytestmark = pytest.mark.gpu
W = SR.MODEL_W


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _model(name):
    model = M.build(name)
    model.set_cuda()
    model.eval()
    return model


def _lm():
    lm = SR.build_lm()
    lm.set_cuda()
    lm.eval()
    return lm


def _stream_all(model, name, **kw):
    """(session, the last feed's hypotheses, scores at each row's final feed,
    per-row concatenated logits, every feed's (hyps, stable lens))."""
    xs, totals = M.inputs(name)
    sizes = M.MODELS[name][2]
    st = model.stream(len(totals), beam_width=W, **kw)
    logits = [[] for _ in totals]
    trace = []
    chunks = S.chunk_lens(totals, sizes)
    for i, (s, n, cl) in enumerate(chunks):
        chunk = xs[:, s:s + n] if n else np.zeros((len(totals), 1, xs.shape[2]), np.float32)
        # a row's utterance ends with the chunk that holds its last frame
        fin = (np.asarray(cl) > 0) & (s + np.asarray(cl) == totals)
        hyps = st.feed(chunk, cl, final=fin)
        lg = st.last_logits.cpu().numpy()
        for b in range(len(totals)):
            logits[b].append(lg[b, :st.last_lens_np[b]])
        trace.append((hyps, st.stable_lens.copy(), st.scores.copy(), fin))
    return st, [np.concatenate(l, axis=0) for l in logits], trace


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,with_lm', [(n, False) for n in sorted(M.MODELS)] +
                         [(SR.LM_MODEL, True)])
def test_streamed_beam_search_equals_the_whole_utterance_search(name, with_lm, precision,
                                                                cuda_dev):
    ops = _ops()
    model = _model(name)
    kw = dict(rnnlm=_lm(), lm_weight=SR.LM_ALPHA, insertion_bonus=SR.LM_BETA) if with_lm else {}
    xs, totals = M.inputs(name)
    ops.set_compute_dtype(precision)
    try:
        st, logits, trace = _stream_all(model, name, **kw)
        whole, _, perm = model.decode(xs, totals, beam_width=W, **kw)
    finally:
        ops.set_compute_dtype('fp32')
    assert ops.last_ctc_beam_path() in ('device', 'device_lm')
    inv = np.argsort(perm)
    B = len(totals)
    # each row's result at its final feed
    got, got_sc = [None] * B, np.zeros(B, np.float32)
    for hyps, stable, scores, fin in trace:
        for b in np.nonzero(fin)[0]:
            got[b], got_sc[b] = hyps[b], scores[b]
            assert stable[b] == len(hyps[b])
    assert all(g is not None for g in got)

    # the offline search on the session's own logits: exact
    lens = np.array([len(l) for l in logits], np.int32)
    padded = np.zeros((B, max(int(lens.max()), 1), logits[0].shape[1]), np.float32)
    for b, l in enumerate(logits):
        padded[b, :len(l)] = l
    lm = dict(kw['rnnlm'].device_weights(), weight=SR.LM_ALPHA) if with_lm else None
    res = ops.ctc_beam_search(torch.from_numpy(padded).to(cuda_dev),
                              torch.from_numpy(lens).to(cuda_dev), W, 0, normalize=True, lm=lm,
                              beta=SR.LM_BETA if with_lm else 0.0)
    hyps, hl, sc = [t.cpu().numpy() for t in res]
    for b in range(B):
        np.testing.assert_array_equal(got[b], hyps[b, :hl[b]].astype(np.int64) - 1,
                                      err_msg='row %d vs the search on its own logits' % b)
    np.testing.assert_array_equal(got_sc.view(np.uint32), sc.view(np.uint32))

    # decode(): where the float64 gaps clear the logit bound's score perturbation
    ok = SR.qualifies(name, precision, with_lm)
    for b in range(B):
        if ok[b]:
            np.testing.assert_array_equal(got[b], np.asarray(whole[inv[b]]),
                                          err_msg='row %d vs decode()' % b)
    print('%s %s lm=%d: %d of %d rows compared with the own-logits search only'
          % (name, precision, with_lm, B - sum(ok), B))

    # the stable prefix never shrinks and every later hypothesis starts with it
    for i, (hyps_i, stable_i, _, _) in enumerate(trace):
        for hyps_j, stable_j, _, _ in trace[i:]:
            for b in range(B):
                assert stable_j[b] >= stable_i[b]
                np.testing.assert_array_equal(hyps_j[b][:stable_i[b]], hyps_i[b][:stable_i[b]])
    for b in range(B):
        np.testing.assert_array_equal(st.hyps()[b], trace[-1][0][b])
        np.testing.assert_array_equal(st.stable()[b], st.hyps()[b][:st.stable_lens[b]])
        nb = st.nbest()[b]
        assert 1 <= len(nb) <= W and all(a[1] >= b_[1] for a, b_ in zip(nb, nb[1:]))


def test_stream_defaults_stay_greedy_and_preconditions(cuda_dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import (CTCBeamStream,
                                                                                 CTCStream)
    model = _model('fast')
    assert type(model.stream(2)) is CTCStream
    assert type(model.stream(2, beam_width=4)) is CTCBeamStream
    assert type(model.stream(2, insertion_bonus=0.5)) is CTCBeamStream
    for bad in (0, 65):
        with pytest.raises(ValueError, match=r'outside \[1, 64\]'):
            model.stream(2, beam_width=bad)
    with pytest.raises(ValueError, match='needs a language model'):
        model.stream(2, beam_width=4, lm_weight=0.5)
    model.train()
    with pytest.raises(RuntimeError, match='eval mode only'):
        model.stream(2, beam_width=4)


def test_reset_restarts_only_that_row(cuda_dev):
    model = _model('fast')
    xs, totals = M.inputs('fast')
    assert list(totals) == [8, 5, 2]
    _, _, trace = _stream_all(model, 'fast')
    want = [None] * 3
    for hyps, _, _, fin in trace:
        for b in np.nonzero(fin)[0]:
            want[b] = hyps[b]
    st = model.stream(3, beam_width=W)
    st.feed(xs[:, :3], [3, 3, 2])
    st.reset(rows=[1])
    assert len(st.hyps()[1]) == 0 and st.stable_lens[1] == 0
    st.feed(xs[:, :3], [0, 3, 0])
    got = st.feed(xs[:, 3:], [5, 2, 0], final=True)
    # (another chunking of the same frames: logits within the bound; these rows' gaps are wide)
    assert all(SR.qualifies('fast', 'fp32'))
    for b in range(3):
        np.testing.assert_array_equal(got[b], want[b])


def test_a_feed_past_max_frames_raises_before_any_launch(cuda_dev):
    model = _model('fast')
    xs, _ = M.inputs('fast')
    st = model.stream(3, beam_width=W, max_frames=4)
    st.feed(xs[:, :3], [3, 3, 2])
    state = [t.clone() for t in st._state.h + st._state.c]
    search = st._search.buf.clone()
    with pytest.raises(ValueError, match='max_frames = 4'):
        st.feed(xs[:, 3:6], [3, 1, 0])
    assert all(torch.equal(a, b) for a, b in zip(state, st._state.h + st._state.c))
    assert torch.equal(search, st._search.buf)
    assert len(st.feed(xs[:, 3:4], [1, 1, 0])) == 3


def test_unsupported_models_and_language_models_are_refused(cuda_dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.hierarchical_ctc import \
        HierarchicalCTC
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
    from test_ctc_stream_ref_cpu import _golden_model
    hier = _golden_model('model_uni_hier', HierarchicalCTC)
    with pytest.raises(NotImplementedError, match='hierarchical'):
        hier.stream(2, beam_width=4)
    model = _model('fast')
    torch.manual_seed(0)
    gru = RNNLM(num_classes=1, embedding_dim=4, rnn_type='gru', bidirectional=False, num_units=8,
                num_layers=1, dropout_embedding=0, dropout_hidden=0, dropout_output=0)
    gru.set_cuda()
    gru.eval()
    with pytest.raises(NotImplementedError, match='only an LSTM language model'):
        model.stream(2, beam_width=4, rnnlm=gru, lm_weight=0.5)
