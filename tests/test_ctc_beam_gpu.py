"""CTC prefix beam search on the device (asr_ctc_beam_search) against the
reference's recorded hypotheses and the float64 restatement (ctc_beam_ref.py).

Every recorded utterance has a final gap and pruning gaps >= 1e-3 (asserted by
the generator and by test_ctc_beam_cpu.py), some hundred times what float32
rounding moves a score, so hypotheses must be EQUAL.  Scores are compared with
the float64 score within score_tol = 8 x the error of a float32 CPU evaluation
of the restatement (stored with the goldens).
"""
import json

import numpy as np
import pytest
import torch

import ctc_beam_ref as R
from conftest import golden, golden_params

pytestmark = pytest.mark.gpu

ASR_ERR_ARG = -1


@pytest.fixture(scope='module')
def G():
    return golden('ctc_beam')


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _search(x, lens, W, blank, dev, normalize=True):
    hyps, hl, sc = _ops().ctc_beam_search(_d(np.asarray(x, np.float32), dev),
                                          _d(np.asarray(lens, np.int32), dev), W, blank,
                                          normalize=normalize)
    torch.cuda.synchronize()
    hyps, hl, sc = hyps.cpu().numpy(), hl.cpu().numpy(), sc.cpu().numpy()
    return [hyps[b, :hl[b]] for b in range(len(hl))], sc


def _check_case(G, name, got, tol):
    hyps, sc = got
    for b in range(len(hyps)):
        ref = G['%s/hyp%d' % (name, b)]
        print('%s[%d] score %.7f ref %.7f diff %.2e (tol %.2e)' % (
            name, b, sc[b], G[name + '/score'][b], abs(sc[b] - G[name + '/score'][b]), tol))
        np.testing.assert_array_equal(hyps[b], ref, err_msg='%s[%d]' % (name, b))
        assert abs(float(sc[b]) - G[name + '/score'][b]) <= tol, (name, b)


def _names(G):
    return [str(n) for n in G['names']]


@pytest.mark.parametrize('normalize', [True, False])
def test_goldens(normalize, G, cuda_dev):
    """Raw logits with the fused log-softmax, and their log-softmax as input."""
    tol = float(G['score_tol'])
    for name in _names(G):
        x, lens = G[name + '/logits'], G[name + '/lens']
        if not normalize:
            with np.errstate(invalid='ignore'):
                x = R.log_softmax(x).astype(np.float32)      # NaN frames stay NaN
        _check_case(G, name, _search(x, lens, int(G[name + '/W']), int(G[name + '/blank']),
                                     cuda_dev, normalize), tol)


def test_hand_made_merge_case(G, cuda_dev):
    """Two frames of [blank 0.6, a 0.4]: the best path is [] (0.36), but [a]
    collects a-, -a, aa = 0.64."""
    lp = np.log(np.array([[[0.6, 0.4]] * 2]))
    hyps, _ = _ops().ctc_best_path(_d(lp.astype(np.float32), cuda_dev),
                                   _d(np.array([2], np.int32), cuda_dev), 0)
    torch.cuda.synchronize()
    hyps, sc = _search(lp, [2], 2, 0, cuda_dev, normalize=False)
    np.testing.assert_array_equal(hyps[0], [1])
    assert abs(float(sc[0]) - np.log(0.64)) <= float(G['score_tol'])
    hyps, sc = _search(lp, [2], 1, 0, cuda_dev, normalize=False)   # width 1: [] stays
    assert len(hyps[0]) == 0


def test_no_pruning_matches_bruteforce(G, cuda_dev):
    """V 3, T 5, W 64: at most 63 prefixes, nothing is dropped, so the score is
    the exact prefix probability (summed over all 3^5 alignments)."""
    for seed in range(3):
        x = (np.random.RandomState(40 + seed).randn(1, 5, 3) * 2).astype(np.float32)
        blank = seed % 3
        r = R.beam_search(R.log_softmax(x[0]), 64, blank)
        hyps, sc = _search(x, [5], 64, blank, cuda_dev)
        if r['final_gap'] >= 1e-3:
            np.testing.assert_array_equal(hyps[0], r['hyp'])
        exact = R.prefix_prob_bruteforce(R.log_softmax(x[0]), hyps[0], blank)
        assert abs(float(sc[0]) - exact) <= float(G['score_tol'])


def test_identity_under_recreation(G, cuda_dev):
    """A prefix leaves the beam and comes back while a child of its earlier
    node stayed: identifying prefixes by (parent id, label) gets this wrong
    (test_ctc_beam_cpu.py shows it on the model of the algorithm)."""
    assert bool(G['identity/recreated'])
    name = 'identity'
    _check_case(G, name, _search(G[name + '/logits'], G[name + '/lens'], int(G[name + '/W']), 0,
                                 cuda_dev), float(G['score_tol']))


def test_ragged_batch_rows_alone(G, cuda_dev):
    """Rows of the ragged batch ([0, 1, 17, 40, 45], T = 40, NaN beyond each
    length) give what they give alone without the padding, bit for bit."""
    x, lens, W = G['ragged/logits'], G['ragged/lens'], int(G['ragged/W'])
    T = x.shape[1]
    hyps, sc = _search(x, lens, W, 0, cuda_dev)
    assert len(hyps[0]) == 0 and sc[0] == 0.0
    assert np.isfinite(sc).all()
    for b in range(1, len(lens)):
        n = min(int(lens[b]), T)
        h1, s1 = _search(x[b:b + 1, :n], [n], W, 0, cuda_dev)
        np.testing.assert_array_equal(h1[0], hyps[b])
        assert s1[0] == sc[b]
    clean = np.where(np.isnan(x), np.float32(50.0), x)        # padding that would win if read
    h2, s2 = _search(clean, lens, W, 0, cuda_dev)
    for b in range(len(lens)):
        np.testing.assert_array_equal(h2[b], hyps[b])
    np.testing.assert_array_equal(s2, sc)


def test_time_major_padded_strides(G, cuda_dev):
    """[T][B][V'] storage with V' > V through the raw C ABI."""
    N = _N()
    x, lens, W = G['ragged/logits'], G['ragged/lens'], int(G['ragged/W'])
    B, T, V = x.shape
    Vp = V + 3
    tm = np.full((T, B, Vp), 1e30, np.float32)                # the pad would win if it were read
    tm[:, :, :V] = x.transpose(1, 0, 2)
    lg = _d(tm, cuda_dev)
    hyps = torch.full((B, T), -7, dtype=torch.int32, device=cuda_dev)
    hl = torch.full((B,), -7, dtype=torch.int32, device=cuda_dev)
    sc = torch.full((B,), -7.0, dtype=torch.float32, device=cuda_dev)
    nb = N.query('asr_ctc_beam_ws_bytes', T, B, V, W)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda_dev)
    N.call('asr_ctc_beam_search', N.ptr(lg), B * Vp, Vp, T, B, V, N.ptr(_d(lens, cuda_dev)), 0, W,
           1, N.ptr(ws), nb, N.ptr(hyps), N.ptr(hl), N.ptr(sc), N.stream_handle(cuda_dev))
    torch.cuda.synchronize()
    hyps, hl, sc = hyps.cpu().numpy(), hl.cpu().numpy(), sc.cpu().numpy()
    _check_case(G, 'ragged', ([hyps[b, :hl[b]] for b in range(B)], sc), float(G['score_tol']))
    for b in range(B):
        assert (hyps[b, hl[b]:] == -7).all()                  # nothing written past the hypothesis


def test_refusals(cuda_dev):
    """beam_width 0 and 65, blank = V, V = 1: the argument error, nothing launched."""
    N = _N()
    T, B, V = 4, 2, 5
    lg = torch.zeros(B, T, V, device=cuda_dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=cuda_dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda_dev)
    for W, blank, v in ((0, 0, V), (65, 0, V), (4, V, V), (4, -1, V), (4, 0, 1)):
        hyps = torch.full((B, T), -7, dtype=torch.int32, device=cuda_dev)
        hl = torch.full((B,), -7, dtype=torch.int32, device=cuda_dev)
        sc = torch.full((B,), -7.0, dtype=torch.float32, device=cuda_dev)
        rc = N.query('asr_ctc_beam_search', N.ptr(lg), V, T * V, T, B, v, N.ptr(lens), blank, W, 1,
                     N.ptr(ws), ws.numel(), N.ptr(hyps), N.ptr(hl), N.ptr(sc),
                     N.stream_handle(cuda_dev))
        torch.cuda.synchronize()
        assert rc == ASR_ERR_ARG, (W, blank, v, rc)
        assert (hl == -7).all() and (sc == -7).all() and (hyps == -7).all()
    assert N.query('asr_ctc_beam_ws_bytes', T, B, V, 0) == 0
    assert N.query('asr_ctc_beam_ws_bytes', T, B, V, 65) == 0
    with pytest.raises(N.NativeError):
        _ops().ctc_beam_search(lg, lens, 65)


# ------------------------------------------------------------- model level
def _ctc_model(name, cls_path, dev):
    import importlib
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    d = golden(name)
    mod, cls = cls_path.rsplit('.', 1)
    torch.manual_seed(1623)
    model = getattr(importlib.import_module(
        'pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.' + mod), cls)(
            **json.loads(str(d['kwargs'])))
    model.load_state_dict(golden_params(d)[0])
    model.set_cuda()
    return model, d


def _own_logits(model, d, multi):
    model.eval()
    with torch.no_grad():
        out = model._encode(model.np2var(d['xs'], dtype='float'), d['x_lens'], is_multi_task=multi)
    return out


def _kernel_hyps(logits, lens_d, W):
    hyps, hl, _ = _ops().ctc_beam_search(logits, lens_d, W, 0, normalize=True)
    hyps, hl = hyps.cpu().numpy(), hl.cpu().numpy()
    return [hyps[b, :hl[b]].astype(np.int64) - 1 for b in range(len(hl))]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_model_decode_beam(cuda_dev):
    model, d = _ctc_model('model_ctc_sub', 'ctc.CTC', cuda_dev)
    B = len(d['xs'])
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=4)
    assert aw is None and isinstance(hyps, np.ndarray) and hyps.dtype == object
    assert hyps.shape == (B,) and sorted(perm.tolist()) == list(range(B))
    logits, lens_d, _ = _own_logits(model, d, False)
    _same(hyps, _kernel_hyps(logits, lens_d, 4))
    assert all(h.min() >= 0 for h in hyps if len(h))          # shifted by -1, blank never emitted
    # decode_from_probs on the model's posteriors, where the restatement says
    # the answer is safe from float32 rounding
    checked = 0
    for temp in (1, 0.05):
        probs, lens, perm2 = model.posteriors(d['xs'], d['x_lens'], temperature=temp)
        np.testing.assert_array_equal(perm2, perm)
        got = model.decode_from_probs(probs, lens, beam_width=4)
        assert got.dtype == object and got.shape == (B,)
        for b in range(B):
            r = R.beam_search(np.log(probs[b, :lens[b]].astype(np.float64) + 1e-10), 4, 0)
            if r['final_gap'] >= 1e-3 and r['prune_gap'] >= 1e-3:
                np.testing.assert_array_equal(got[b], r['hyp'] - 1)
                if temp == 1:
                    np.testing.assert_array_equal(got[b], hyps[b])
                checked += 1
    assert checked > 0
    # beam_width == 1 is the best path as before
    h1, _, _ = model.decode(d['xs'], d['x_lens'], beam_width=1)
    bp, bl = _ops().ctc_best_path(logits, lens_d, 0)
    _same(h1, [bp[b, :bl[b]].cpu().numpy().astype(np.int64) - 1 for b in range(B)])


def test_hierarchical_task_index(cuda_dev):
    model, d = _ctc_model('model_hier', 'hierarchical_ctc.HierarchicalCTC', cuda_dev)
    logits, lens_d, logits_sub, lens_sub_d, _ = _own_logits(model, d, True)
    assert logits.shape[-1] != logits_sub.shape[-1]
    for W in (4, 10):
        h0, _, perm = model.decode(d['xs'], d['x_lens'], beam_width=W, task_index=0)
        h1, _, _ = model.decode(d['xs'], d['x_lens'], beam_width=W, task_index=1)
        _same(h0, _kernel_hyps(logits, lens_d, W))
        _same(h1, _kernel_hyps(logits_sub, lens_sub_d, W))
    # best path: the sub head, no longer the main head's hypotheses
    g0, _, _ = model.decode(d['xs'], d['x_lens'], beam_width=1, task_index=0)
    g1, _, _ = model.decode(d['xs'], d['x_lens'], beam_width=1, task_index=1)
    B = len(g0)
    bp, bl = _ops().ctc_best_path(logits_sub, lens_sub_d, 0)
    _same(g1, [bp[b, :bl[b]].cpu().numpy().astype(np.int64) - 1 for b in range(B)])
    bp, bl = _ops().ctc_best_path(logits, lens_d, 0)
    main = [bp[b, :bl[b]].cpu().numpy().astype(np.int64) - 1 for b in range(B)]
    _same(g0, main)
    # the two heads' best paths differ on this model, so the two task indices do
    assert any(not np.array_equal(a, b) for a, b in zip(g0, g1))
    p0, l0, _ = model.posteriors(d['xs'], d['x_lens'], task_idx=0)
    p1, l1, _ = model.posteriors(d['xs'], d['x_lens'], task_idx=1)
    assert p0.shape[-1] == logits.shape[-1] and p1.shape[-1] == logits_sub.shape[-1]
    np.testing.assert_array_equal(l1, lens_sub_d.cpu().numpy())
    with pytest.raises(NotImplementedError):
        model.decode(d['xs'], d['x_lens'], beam_width=4, task_index=2)
    with pytest.raises(NotImplementedError):
        model.posteriors(d['xs'], d['x_lens'], task_idx=2)
