"""The streaming CTC prefix beam search (asr_ctc_beam_stream_*, through
native_ops.ctc_beam_stream_*) against the whole-utterance search on the device
(native_ops.ctc_beam_search), BIT FOR BIT: random logits, B = 3, T = 23, lens
(23, 17, 9), fed whole, as 23 one-frame chunks and as (5, 1, 9, 8) with one row
given nothing in the second chunk; the result of the feed that carries a row's
final flag must equal the offline search on the whole logits (hyps, lengths,
scores as uint32).  tests/test_ctc_beam_stream_ref_cpu.py shows the same of the
numpy restatement, and that the tie and recreation inputs are what they claim.
Every test here needs the streaming ops."""
import numpy as np
import pytest
import torch

import ctc_beam_lm_cases as C
import ctc_beam_lm_ref as R
import ctc_beam_ref as R0
import ctc_beam_stream_ref as SR

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offline(x, lens, W, dev, normalize=True, lm=None, beta=0.0):
    """(hyps [B, T], lens [B], scores as uint32 [B]) of the whole-utterance search."""
    res = _ops().ctc_beam_search(_d(x, dev), _d(np.asarray(lens, np.int32), dev), W, 0,
                                 normalize=normalize, lm=lm, beta=beta)
    torch.cuda.synchronize()
    hyps, hl, sc = (t.cpu().numpy() for t in res)
    return hyps, hl, sc.view(np.uint32)


def _chunks(x, takes):
    """Per feed: (chunk [B, Tc, V] with each row's next frames, NaN beyond, the
    rows' frame counts, the rows that end with this feed)."""
    B = x.shape[0]
    total = np.sum(takes, axis=0)
    done = np.zeros(B, np.int64)
    for take in takes:
        Tc = max(int(take.max()), 1)
        chunk = np.full((B, Tc, x.shape[2]), np.nan, np.float32)
        for b in range(B):
            chunk[b, :take[b]] = x[b, done[b]:done[b] + take[b]]
        done = done + take
        yield chunk, take, (take > 0) & (done == total)


def _stream(x, takes, W, dev, normalize=True, lm=None, beta=0.0, max_frames=SR.T, each=None,
            st=None):
    """Feeds x by `takes`; (hyps [B, max_frames], lens, scores uint32) gathered
    per row from the feed that carried its final flag.  each(st, out,
    take, fin): called after every feed with the feed's host results."""
    ops = _ops()
    B, _, V = x.shape
    if st is None:
        st = ops.ctc_beam_stream_state(B, V, W, max_frames, dev, blank=0, normalize=normalize,
                                       lm=lm, beta=beta)
    hyps = np.zeros((B, max_frames), np.int32)
    hl = np.full(B, -1, np.int32)
    sc = np.zeros(B, np.uint32)
    for chunk, take, fin in _chunks(x, takes):
        out = ops.ctc_beam_stream_feed(st, _d(chunk, dev), _d(take.astype(np.int32), dev),
                                       _d(fin.astype(np.int32), dev))
        torch.cuda.synchronize()
        out = [t.cpu().numpy() for t in out]
        for b in np.nonzero(fin)[0]:
            hyps[b], hl[b], sc[b] = out[0][b], out[1][b], out[2].view(np.uint32)[b]
            assert out[3][b] == out[1][b], 'stable_lens == hyp_lens at final'
        if each is not None:
            each(st, out, take, fin)
    return hyps, hl, sc


def _assert_same(got, want, what):
    hyps, hl, sc = got
    whyps, whl, wsc = want
    np.testing.assert_array_equal(hl, whl, err_msg=what)
    np.testing.assert_array_equal(sc, wsc, err_msg=what + ' (scores as uint32)')
    for b, n in enumerate(whl):
        np.testing.assert_array_equal(hyps[b, :n], whyps[b, :n], err_msg='%s row %d' % (what, b))


@pytest.mark.parametrize('W', SR.WS)
@pytest.mark.parametrize('V', SR.VS)
def test_every_chunking_equals_the_offline_search(V, W, cuda_dev):
    x = SR.logits(V)
    for normalize in (True, False):
        xin = x if normalize else R0.log_softmax(x).astype(np.float32)
        want = _offline(xin, SR.LENS, W, cuda_dev, normalize)
        assert _ops().last_ctc_beam_path() == 'device'
        assert want[1].max() > 0
        for name, takes in SR.chunkings().items():
            got = _stream(xin, takes, W, cuda_dev, normalize)
            assert _ops().last_ctc_beam_path() == 'stream'
            _assert_same(got, want, 'V %d W %d normalize %d %s' % (V, W, normalize, name))


@pytest.mark.parametrize('beta', [0.0, -0.5, 0.8])
@pytest.mark.parametrize('layers', [1, 2])
def test_lm_fusion_equals_the_offline_search(layers, beta, cuda_dev):
    for V, W in ((29, 8), (200, 2)):
        x = SR.logits(V)
        lm = R.device_lm(R.make_lm(40 + layers, V, layers, 8, 4), cuda_dev, 0.7)
        want = _offline(x, SR.LENS, W, cuda_dev, lm=lm, beta=beta)
        assert _ops().last_ctc_beam_path() == 'device_lm'
        for name, takes in SR.chunkings().items():
            got = _stream(x, takes, W, cuda_dev, lm=lm, beta=beta)
            assert _ops().last_ctc_beam_path() == 'stream_lm'
            _assert_same(got, want, 'V %d layers %d beta %g %s' % (V, layers, beta, name))


@pytest.mark.parametrize('beta', [-0.5, 0.8])
def test_the_bonus_alone_equals_the_offline_search(beta, cuda_dev):
    x = SR.logits(29)
    want = _offline(x, SR.LENS, 8, cuda_dev, beta=beta)
    for name, takes in SR.chunkings().items():
        got = _stream(x, takes, 8, cuda_dev, beta=beta)
        assert _ops().last_ctc_beam_path() == 'stream_lm'
        _assert_same(got, want, 'beta %g %s' % (beta, name))


def test_ties_across_chunk_boundaries_keep_the_offline_order(cuda_dev):
    """Inputs quantised to multiples of 0.5, normalize=False: equal scores occur;
    the f32 restatement must see a tie at the pruning boundary."""
    x = SR.tie_logits()
    tied = [R.search(x[b, :n], 8, 0, None, 0.0, 0.0, np.float32, normalize=False)['prune_gap'] == 0
            for b, n in enumerate(SR.LENS)]
    assert any(tied), tied
    want = _offline(x, SR.LENS, 8, cuda_dev, normalize=False)
    for name in ('ones', 'split'):
        got = _stream(x, SR.chunkings()[name], 8, cuda_dev, normalize=False)
        _assert_same(got, want, 'ties ' + name)


def test_a_prefix_that_leaves_and_returns_in_another_feed(cuda_dev):
    """ctc_beam_lm_cases.IDENTITY: the restatement reports `recreated`; one-frame
    feeds put the leave and the return into different calls."""
    assert C.ref('identity')[0]['recreated']
    case = C.IDENTITY
    x, lens, lmp = C.draw(case, C.IDENTITY_SEED)
    lm = R.device_lm(lmp, cuda_dev, case['alpha'])
    want = _offline(x, lens, case['W'], cuda_dev, lm=lm, beta=case['beta'])
    n = int(lens[0])
    for takes in ([np.array([1])] * n, [np.array([3]), np.array([n - 3])]):
        got = _stream(x, takes, case['W'], cuda_dev, lm=lm, beta=case['beta'], max_frames=n)
        _assert_same(got, (want[0][:, :n], want[1], want[2]), 'identity')
    np.testing.assert_array_equal(want[0][0, :want[1][0]], C.ref('identity')[0]['hyp'])


@pytest.mark.parametrize('with_lm', [False, True])
def test_stable_lens_and_nbest(with_lm, cuda_dev):
    ops = _ops()
    V, W = 6, 8
    x = SR.logits(V, seed=1)
    lm = R.device_lm(R.make_lm(50, V, 1, 8, 4), cuda_dev, 0.7) if with_lm else None
    last = [0] * SR.B
    seen = []

    def each(st, out, take, fin):
        hyps, hl, sc, sl = out
        nh, nl, ns, nc = [t.cpu().numpy() for t in ops.ctc_beam_stream_nbest(st)]
        for b in range(SR.B):
            entries = [nh[b, i, :nl[b, i]] for i in range(nc[b])]
            assert 1 <= nc[b] <= W
            if not fin[b]:
                # (at final the output is re-ranked; the state is not)
                np.testing.assert_array_equal(entries[0], hyps[b, :hl[b]])
                assert ns[b, 0].view(np.uint32) == sc[b].view(np.uint32)
                assert sl[b] == SR.common_prefix_len(entries), (b, sl[b], entries)
            else:
                assert sl[b] == hl[b]
                assert any(np.array_equal(e, hyps[b, :hl[b]]) for e in entries)
            assert (np.diff(ns[b, :nc[b]]) <= 0).all(), ns[b]
            assert len(set(tuple(e) for e in entries)) == nc[b], 'distinct prefixes'
            if take[b] and not fin[b]:
                assert sl[b] >= last[b], 'monotone'
                last[b] = int(sl[b])
        seen.append(sl.copy())

    for name in ('ones', 'split'):
        last[:] = [0] * SR.B
        _stream(x, SR.chunkings()[name], W, cuda_dev, lm=lm, each=each)
    assert max(int(s.max()) for s in seen) > 0, 'no stable label was ever reported'


def test_reset_restarts_only_that_row(cuda_dev):
    ops = _ops()
    V, W = 29, 8
    x = SR.logits(V)
    lm = R.device_lm(R.make_lm(51, V, 2, 8, 4), cuda_dev, 0.7)
    want = _offline(x, SR.LENS, W, cuda_dev, lm=lm, beta=0.3)
    st = ops.ctc_beam_stream_state(SR.B, V, W, SR.T, cuda_dev, lm=lm, beta=0.3)
    lens = np.asarray(SR.LENS)
    first = np.minimum(lens, 6)
    dev = cuda_dev
    ops.ctc_beam_stream_feed(st, _d(x[:, :6], dev), _d(first.astype(np.int32), dev))
    # row 1 starts over; rows 0 and 2 pause while it is fed its first 6 frames again
    ops.ctc_beam_stream_reset(st, rows=[1])
    ops.ctc_beam_stream_feed(st, _d(x[:, :6], dev), _d(np.array([0, 6, 0], np.int32), dev))
    rest = lens - first
    chunk = np.full((SR.B, int(rest.max()), V), np.nan, np.float32)
    for b in range(SR.B):
        chunk[b, :rest[b]] = x[b, 6:lens[b]]
    out = ops.ctc_beam_stream_feed(st, _d(chunk, dev), _d(rest.astype(np.int32), dev),
                                   _d(np.ones(SR.B, np.int32), dev))
    torch.cuda.synchronize()
    hyps, hl, sc, _ = [t.cpu().numpy() for t in out]
    _assert_same((hyps, hl, sc.view(np.uint32)), want, 'after reset(rows=[1])')
    assert ops.ctc_beam_stream_status(st).cpu().numpy().tolist() == [0, 0, 0]


def test_max_frames_clamps_and_sets_the_status_word(cuda_dev):
    """max_frames = 8, fed 5 + 5 frames through the op: the last two frames are
    dropped, the row's status word says so, the result is the offline search on
    the first 8 frames."""
    ops = _ops()
    V, W = 29, 8
    x = SR.logits(V)[:, :10]
    want = _offline(np.ascontiguousarray(x[:, :8]), [8, 8, 8], W, cuda_dev)
    st = ops.ctc_beam_stream_state(SR.B, V, W, 8, cuda_dev)
    five = _d(np.array([5, 5, 3], np.int32), cuda_dev)
    ops.ctc_beam_stream_feed(st, _d(x[:, :5], cuda_dev), five)
    assert ops.ctc_beam_stream_status(st).cpu().numpy().tolist() == [0, 0, 0]
    # row 2 had 3 + 5 = 8 frames: exactly full, nothing dropped
    x2 = np.ascontiguousarray(x[:, 5:10]).copy()
    x2[2] = x[2, 3:8]
    out = ops.ctc_beam_stream_feed(st, _d(x2, cuda_dev), _d(np.array([5, 5, 5], np.int32), cuda_dev),
                                   _d(np.ones(SR.B, np.int32), cuda_dev))
    torch.cuda.synchronize()
    hyps, hl, sc, _ = [t.cpu().numpy() for t in out]
    assert ops.ctc_beam_stream_status(st).cpu().numpy().tolist() == [1, 1, 0]
    assert hyps.shape[1] == 8 and (hl <= 8).all()
    _assert_same((hyps, hl, sc.view(np.uint32)), want, 'clamped at max_frames')


def test_refusals(cuda_dev):
    ops = _ops()
    from pytorch_end2end_speech_recognition_amd._native import NativeError
    for W in (0, 65):
        with pytest.raises(NativeError, match=r'beam_width = %d outside \[1, 64\]' % W):
            ops.ctc_beam_stream_state(2, 29, W, 16, cuda_dev)
    st = ops.ctc_beam_stream_state(2, 29, 4, 16, cuda_dev)
    st.buf = st.buf[:st.buf.numel() - 16]
    x = _d(SR.logits(29)[:2, :4], cuda_dev)
    with pytest.raises(NativeError, match='state .* bytes'):
        ops.ctc_beam_stream_feed(st, x, _d(np.array([4, 4], np.int32), cuda_dev))
    gru = R.device_lm(R.make_lm(52, 29, 1, 8, 4), cuda_dev, 0.5)
    gru = dict(gru, cell='gru', w_ih=[w[:24] for w in gru['w_ih']], w_hh=[w[:24] for w in gru['w_hh']],
               b_ih=[b[:24] for b in gru['b_ih']], b_hh=[b[:24] for b in gru['b_hh']])
    with pytest.raises(NotImplementedError, match='only an LSTM language model'):
        ops.ctc_beam_stream_state(2, 29, 4, 16, cuda_dev, lm=gru)
