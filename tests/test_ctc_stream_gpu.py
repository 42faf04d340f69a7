"""CTC.stream (chunk-by-chunk greedy recognition: RNNEncoder.forward_chunk over
csrc/lstm_stream.hip, asr_ctc_best_path_stream) on the small seeded models of
tests/ctc_stream_ref.py -- a 2 x 16 fast-path encoder, per-layer modules with
projection and residual sums, 'drop' subsampling (stride 4) and 'concat'
subsampling (stride 2) -- in both compute types.  Models that do not subsample
run ragged B = 3 with an empty chunk; subsampling ones B = 1 and equal-length
B = 2.

Per model: the chunks' last_logits concatenated per row match the rows of the
whole-utterance _task_logits (un-permuted) within ctc_stream_ref.logit_bound --
one recurrent layer's bound, MARGIN x the largest recorded constant of
tests/lstm_stream_ref.py in the compute type, compounded over the model's
recurrent and linear layers, relative to the largest whole-utterance logit;
err/bound is printed.  The emitted labels equal the host GreedyDecoder on the
stream's own concatenated logits exactly, and equal decode(beam_width=1)
(tests/test_ctc_stream_ref_cpu.py: the float64 top-two gap of every frame is 4
x the bound of either compute type).  hyps()
accumulates the chunks, reset(rows=[1]) restarts only that row, the bf16 W_hh
copies are made once per session.  Every test here needs CTC.stream."""
import numpy as np
import pytest
import torch

import ctc_stream_ref as M
import lstm_stream_ref as S

pytestmark = pytest.mark.gpu


def _model(name):
    model = M.build(name)
    model.set_cuda()
    model.eval()
    return model


def _stream_all(model, name, final_last=True):
    """Feeds inputs(name) by the model's schedule: (stream, per-row list of the
    chunks' emitted labels, per-row concatenated logits numpy)."""
    xs, totals = M.inputs(name)
    sizes = M.MODELS[name][2]
    st = model.stream(len(totals))
    emitted = [[] for _ in totals]
    logits = [[] for _ in totals]
    chunks = S.chunk_lens(totals, sizes)
    for i, (s, n, cl) in enumerate(chunks):
        chunk = xs[:, s:s + n] if n else np.zeros((len(totals), 1, xs.shape[2]), np.float32)
        new = st.feed(chunk, cl, final=final_last and i == len(chunks) - 1)
        lg = st.last_logits.cpu().numpy()
        assert len(new) == len(totals)
        for b in range(len(totals)):
            emitted[b].append(new[b])
            logits[b].append(lg[b, :st.last_lens_np[b]])
    return st, emitted, [np.concatenate(l, axis=0) for l in logits]


def _whole(model, name):
    """(logits numpy [B, T', V] in the input's row order, lens, decode(1) hyps)."""
    xs, totals = M.inputs(name)
    with torch.no_grad():
        model.eval()
        lg, _, lens_np = model._task_logits(model.np2var(xs, dtype='float'), totals, 0)
    perm = model.encoder.last_perm_np.copy()
    lg, lens_np = lg.cpu().numpy(), np.asarray(lens_np).copy()
    inv = np.argsort(perm)
    hyps, _, perm2 = model.decode(xs, totals, beam_width=1)
    np.testing.assert_array_equal(perm, perm2)
    return lg[inv], lens_np[inv], [np.asarray(hyps[i]) for i in inv]


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', sorted(M.MODELS))
def test_streamed_logits_and_labels_equal_the_whole_utterance(name, precision, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.decoders.greedy_decoder \
        import GreedyDecoder
    model = _model(name)
    ops.set_compute_dtype(precision)
    try:
        st, emitted, logits = _stream_all(model, name)
        whole, lens, hyps = _whole(model, name)
    finally:
        ops.set_compute_dtype('fp32')
    totals = M.inputs(name)[1]
    np.testing.assert_array_equal(lens, totals // M.stride(name))
    top = max(float(np.abs(whole[b, :n]).max()) for b, n in enumerate(lens))
    bound = M.logit_bound(name, precision)
    worst = 0.0
    for b, n in enumerate(lens):
        assert logits[b].shape == (n, whole.shape[2]), (b, logits[b].shape, n)
        assert np.isfinite(logits[b]).all()
        worst = max(worst, float(np.abs(logits[b] - whole[b, :n]).max()) / top)
    print('%s-%s logits err/bound %.3g (err %.3e, bound %.3e)'
          % (name, precision, worst / bound, worst, bound))
    assert worst <= bound

    got = [np.concatenate(e) for e in emitted]
    # the host decoder (numpy path) on the stream's own logits: exact
    T = max(len(l) for l in logits)
    padded = np.zeros((len(lens), T, whole.shape[2]), np.float32)
    for b, l in enumerate(logits):
        padded[b, :len(l)] = l
    host = GreedyDecoder(blank_index=0)(padded, lens)
    for b in range(len(lens)):
        np.testing.assert_array_equal(got[b], host[b] - 1, err_msg='row %d vs host decoder' % b)
        np.testing.assert_array_equal(got[b], hyps[b], err_msg='row %d vs decode()' % b)
        np.testing.assert_array_equal(st.hyps()[b], got[b])
    assert any(len(g) for g in got)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_reset_restarts_only_that_row(precision, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    name = 'fast'
    model = _model(name)
    xs, totals = M.inputs(name)
    ops.set_compute_dtype(precision)
    try:
        _, want_emitted, want_logits = _stream_all(model, name)
        st = model.stream(3)
        assert list(totals) == [8, 5, 2]
        first = st.feed(xs[:, :3], [3, 3, 2])
        lg_first = st.last_logits.clone()
        # row 1 starts over and is fed its first 3 frames again; rows 0 and 2 pause
        st.reset(rows=[1])
        assert len(st.hyps()[1]) == 0
        np.testing.assert_array_equal(st.hyps()[0], first[0])
        again = st.feed(xs[:, :3], [0, 3, 0])
        assert torch.equal(st.last_logits[1], lg_first[1])
        np.testing.assert_array_equal(again[1], first[1])
        assert len(again[0]) == 0 and len(again[2]) == 0
        # the others continue as if nothing had happened: the rest of row 0
        rest = st.feed(xs[:, 3:], [5, 2, 0], final=True)
    finally:
        ops.set_compute_dtype('fp32')
    # (another chunking of the same frames: the GEMMs may sum in another order)
    lg = st.last_logits.cpu().numpy()
    tol = M.logit_bound(name, precision) * float(np.abs(want_logits[0]).max())
    np.testing.assert_allclose(lg[0, :5], want_logits[0][3:], rtol=0, atol=tol)
    np.testing.assert_allclose(lg[1, :2], want_logits[1][3:5], rtol=0, atol=tol)
    np.testing.assert_array_equal(np.concatenate([first[0], rest[0]]),
                                  np.concatenate(want_emitted[0]))
    np.testing.assert_array_equal(st.hyps()[1], np.concatenate(want_emitted[1]))
    st.reset()
    assert all(len(h) == 0 for h in st.hyps())
    np.testing.assert_array_equal(st.feed(xs[:, :3], [3, 3, 2])[2], first[2])


def test_the_bf16_w_hh_copies_are_made_once_per_session(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    model = _model('fast')
    xs, totals = M.inputs('fast')
    ops.set_compute_dtype('bf16')
    try:
        st = model.stream(3)
        st.feed(xs[:, :5], [5, 5, 4])
        cache = dict(st._state._whh_bf)
        assert sorted(cache) == [0, 1] and all(w.dtype == torch.bfloat16 for w in cache.values())
        st.feed(xs[:, 5:6], [1, 1, 0])
        assert all(st._state._whh_bf[l] is w for l, w in cache.items())
        model._flat_param.add_(0.0)          # a new version of the parameters
        st.feed(xs[:, 6:7], [1, 1, 0])
        assert all(st._state._whh_bf[l] is not w for l, w in cache.items())
    finally:
        ops.set_compute_dtype('fp32')


def test_a_chunk_length_off_the_stride_raises_before_any_launch(cuda_dev):
    model = _model('drop_b2')
    st = model.stream(2)
    xs, totals = M.inputs('drop_b2')
    with pytest.raises(ValueError, match='multiple of the subsampling stride 4'):
        st.feed(xs[:, :6], [6, 6])
    new = st.feed(xs[:, :8], [8, 8])
    assert tuple(st.last_logits.shape[:2]) == (2, 2) and len(new) == 2


def test_unsupported_models_are_refused(cuda_dev):
    from test_ctc_stream_ref_cpu import test_unsupported_configurations_are_refused_by_name
    test_unsupported_configurations_are_refused_by_name()
