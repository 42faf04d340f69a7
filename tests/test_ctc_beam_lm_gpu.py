"""CTC prefix beam search with a language model on the device
(asr_ctc_beam_search_lm) against the float64 restatement
(tests/ctc_beam_lm_ref.py) on the cases of tests/ctc_beam_lm_cases.py.

Every case has a final gap and pruning gaps >= 1e-3 in float64
(test_ctc_beam_lm_cpu.py asserts it), so hypotheses must be EQUAL; scores within
the case's score_tol = 8 x the deviation of the restatement's f32 evaluation
from its f64 one (computed, not stored).  Inputs that are no case of the list
use the list's largest score_tol."""
import numpy as np
import pytest
import torch

import ctc_beam_lm_cases as C
import ctc_beam_lm_ref as R
import ctc_beam_ref as R0

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _search(x, lens, W, blank, lm_params, alpha, beta, dev, normalize=True, cell='lstm',
            with_lm=None):
    """Through native_ops.ctc_beam_search(lm=, beta=).  with_lm: pass the LM
    dict even at alpha == 0 (the new entry point with the LM term absent)."""
    lm = None
    if lm_params is not None and (alpha > 0 or with_lm):
        lm = R.device_lm(lm_params, dev, alpha, cell)
    res = _ops().ctc_beam_search(_d(np.asarray(x, np.float32), dev),
                                 _d(np.asarray(lens, np.int32), dev), W, blank,
                                 normalize=normalize, lm=lm, beta=beta)
    if res is None:
        return None
    torch.cuda.synchronize()
    hyps, hl, sc = (t.cpu().numpy() for t in res)
    return [hyps[b, :hl[b]] for b in range(len(hl))], sc


@pytest.mark.parametrize('name', list(C.CASES))
def test_cases(name, cuda_dev):
    case = C.CASES[name]
    x, lens, lm = C.draw(case, C.SEEDS[name])
    # frames past an utterance's length are never read: NaN there
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    hyps, sc = _search(x, lens, case['W'], case['blank'], lm, case['alpha'], case['beta'],
                       cuda_dev)
    assert _ops().last_ctc_beam_path() == 'device_lm'
    tol = C.score_tol(name)
    for b, r in enumerate(C.ref(name)):
        print('%s[%d] score %.7f ref %.7f diff %.2e (tol %.2e)'
              % (name, b, sc[b], r['score'], abs(float(sc[b]) - r['score']), tol))
    for b, r in enumerate(C.ref(name)):
        np.testing.assert_array_equal(hyps[b], r['hyp'], err_msg='%s[%d]' % (name, b))
        assert abs(float(sc[b]) - r['score']) <= tol, (name, b)


def test_log_probabilities_as_input(cuda_dev):
    """normalize=False: the f32 log-softmax as input gives the same search."""
    name = 'v29_w20'
    case = C.CASES[name]
    x, lens, lm = C.draw(case, C.SEEDS[name])
    lp = R0.log_softmax(x).astype(np.float32)
    hyps, sc = _search(lp, lens, case['W'], case['blank'], lm, case['alpha'], case['beta'],
                       cuda_dev, normalize=False)
    for b, r in enumerate(C.ref(name)):
        np.testing.assert_array_equal(hyps[b], r['hyp'])
        assert abs(float(sc[b]) - r['score']) <= C.score_tol(name)


@pytest.mark.parametrize('name', ['v29_w20', 'v129_w20', 'v3_w2'])
def test_zero_weights_through_the_new_entry_point(name, cuda_dev):
    """alpha = beta = 0 with an LM given: asr_ctc_beam_search_lm with the terms
    absent returns the existing search's hypotheses."""
    case = C.CASES[name]
    x, lens, lm = C.draw(case, C.SEEDS[name])
    old = _search(x, lens, case['W'], case['blank'], None, 0.0, 0.0, cuda_dev)
    assert _ops().last_ctc_beam_path() == 'device'
    new = _search(x, lens, case['W'], case['blank'], lm, 0.0, 0.0, cuda_dev, with_lm=True)
    assert _ops().last_ctc_beam_path() == 'device_lm'
    for b in range(len(lens)):
        r = R0.beam_search(R0.log_softmax(x[b, :lens[b]]), case['W'], case['blank'])
        print('%s[%d] old %.7f new %.7f f64 %.7f' % (name, b, old[1][b], new[1][b], r['score']))
        np.testing.assert_array_equal(new[0][b], old[0][b])
        if r['final_gap'] >= C.GAP and r['prune_gap'] >= C.GAP:
            np.testing.assert_array_equal(new[0][b], r['hyp'])
        assert abs(float(new[1][b]) - r['score']) <= C.score_tol(name)


@pytest.mark.parametrize('alpha,beta', [(0.7, 0.0), (0.0, 0.4), (0.5, -0.2)])
def test_hand_made_merge_case(alpha, beta, cuda_dev):
    """Two frames of [blank 0.6, a 0.4], W 2: [a] collects a-, -a, aa = 0.64 and
    carries one LM edge, the <eos> term and one bonus."""
    lp = np.log(np.array([[[0.6, 0.4]] * 2]))
    lm = R.make_lm(6, 2, 1, 8, 4)       # an LM under which [a] still wins, by >= 0.1
    r = R.search(lp[0], 2, 0, lm, alpha, beta, normalize=False)
    assert list(r['hyp']) == [1] and r['final_gap'] >= C.GAP
    hyps, sc = _search(lp, [2], 2, 0, lm, alpha, beta, cuda_dev, normalize=False)
    np.testing.assert_array_equal(hyps[0], [1])
    m = R.LM(lm)
    want = np.log(0.64) + beta
    if alpha > 0:
        want += alpha * (m.row(())[0] + m.row((0,))[m.eos])
    print('merge alpha %g beta %g: %.7f want %.7f' % (alpha, beta, sc[0], want))
    assert abs(float(sc[0]) - want) <= C.score_tol_all()


@pytest.mark.parametrize('alpha,beta,lm_shape', [(0.5, 0.0, (1, 8, 4)), (0.0, 0.7, None),
                                                 (0.8, -0.4, (2, 32, 16))])
def test_no_pruning_matches_bruteforce(alpha, beta, lm_shape, cuda_dev):
    """V 3, T 5, W 64: nothing is dropped, so the score is the sum over all 3^5
    alignments plus the LM and bonus terms of the returned hypothesis."""
    for seed in range(3):
        blank = seed % 3
        x = (np.random.RandomState(40 + seed).randn(1, 5, 3) * 2).astype(np.float32)
        lm = R.make_lm(seed, 3, *lm_shape) if lm_shape else None
        r = R.search(x[0], 64, blank, lm, alpha, beta)
        hyps, sc = _search(x, [5], 64, blank, lm, alpha, beta, cuda_dev)
        if r['final_gap'] >= C.GAP:
            np.testing.assert_array_equal(hyps[0], r['hyp'])
        exact = R.score_bruteforce(R0.log_softmax(x[0]), lm, hyps[0], alpha, beta, blank)
        print('bruteforce seed %d: %.7f exact %.7f' % (seed, sc[0], exact))
        assert abs(float(sc[0]) - exact) <= C.score_tol_all()


def test_identity_under_recreation(cuda_dev):
    """A prefix leaves the beam and comes back while a child of its earlier node
    stayed; with alpha > 0 its LM state is made again from its parent's."""
    r = C.ref('identity')[0]
    assert r['recreated'] and C.IDENTITY['alpha'] > 0
    x, lens, lm = C.draw(C.IDENTITY, C.IDENTITY_SEED)
    hyps, sc = _search(x, lens, C.IDENTITY['W'], 0, lm, C.IDENTITY['alpha'], 0.0, cuda_dev)
    print('identity score %.7f ref %.7f' % (sc[0], r['score']))
    np.testing.assert_array_equal(hyps[0], r['hyp'])
    assert abs(float(sc[0]) - r['score']) <= C.score_tol('identity')


def test_kernels_refuse_deep_and_gru_lms(cuda_dev):
    x, lens, _ = C.draw(C.CASES['v29_w20'], 0)
    deep = R.make_lm(1, 29, C.MAX_LAYERS + 1, 8, 4)
    assert _search(x, lens, 4, 0, deep, 0.3, 0.0, cuda_dev) is None
    gru = {k.replace('lstm.', 'gru.'): v[:3 * 8] if 'lstm.' in k else v
           for k, v in R.make_lm(1, 29, 1, 8, 4).items()}
    assert _search(x, lens, 4, 0, gru, 0.3, 0.0, cuda_dev, cell='gru') is None


def test_native_refusals(cuda_dev):
    x, lens, lm = C.draw(C.CASES['v29_w20'], 0)
    with pytest.raises(ValueError):
        _search(x, lens, 4, 0, R.make_lm(1, 30, 1, 8, 4), 0.3, 0.0, cuda_dev)   # LM width
    with pytest.raises(ValueError):
        _search(x, lens, 4, 0, lm, -0.1, 0.0, cuda_dev, with_lm=True)


# ------------------------------------------------------------- model level
def _levenshtein(a, b):
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev, d[j] = d[j], cur
    return d[len(b)]


def _lm(num_classes, seed, rnn_type='lstm', num_layers=1):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
    torch.manual_seed(seed)
    lm = RNNLM(num_classes, embedding_dim=4, rnn_type=rnn_type, bidirectional=False, num_units=8,
               num_layers=num_layers, dropout_embedding=0, dropout_hidden=0, dropout_output=0)
    with torch.no_grad():
        for p in lm.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
    lm.set_cuda()
    lm.eval()
    return lm


def _model(hier, seed=1623):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.hierarchical_ctc import \
        HierarchicalCTC
    native_ops.set_compute_dtype('fp32')
    kw = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True, encoder_num_units=8,
              encoder_num_proj=0, encoder_num_layers=2 if hier else 1, fc_list=[],
              dropout_input=0, dropout_encoder=0, num_classes=5, parameter_init=0.1,
              subsample_list=[], subsample_type='drop')
    if hier:
        kw.update(encoder_num_layers_sub=1, fc_list_sub=[], main_loss_weight=0.5,
                  sub_loss_weight=0.5, num_classes=7, num_classes_sub=5)
    torch.manual_seed(seed)
    model = (HierarchicalCTC if hier else CTC)(**kw)
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.8, 0.8)
    model.set_cuda()
    rng = np.random.RandomState(3)
    x_lens = np.array([11, 8, 3], np.int32)
    xs = rng.randn(3, 11, 8).astype(np.float32) * 2
    for b in range(3):
        xs[b, x_lens[b]:] = 0
    return model, xs, x_lens


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _model_checks(model, xs, x_lens, lm, task, monkeypatch, W=4, alpha=0.5, beta=0.2):
    ops = _ops()
    kw = dict(rnnlm=lm, lm_weight=alpha, insertion_bonus=beta)
    monkeypatch.delenv('ASR_CTC_BEAM', raising=False)
    dev_h, aw, perm = model.decode(xs, x_lens, beam_width=W, task_index=task, **kw)
    assert aw is None and ops.last_ctc_beam_path() == 'device_lm'
    monkeypatch.setenv('ASR_CTC_BEAM', 'host')
    host_h, _, perm2 = model.decode(xs, x_lens, beam_width=W, task_index=task, **kw)
    assert ops.last_ctc_beam_path() == 'host'
    monkeypatch.delenv('ASR_CTC_BEAM')
    np.testing.assert_array_equal(perm, perm2)
    _same(dev_h, host_h)
    plain, _, _ = model.decode(xs, x_lens, beam_width=W, task_index=task)
    assert ops.last_ctc_beam_path() == 'device'
    # error_rate: decode()'s output scored on the host
    ys = np.random.RandomState(5).randint(0, 5, (3, 6)).astype(np.int32)
    y_lens = np.array([6, 4, 2], np.int32)
    res = model.error_rate(xs, x_lens, ys, y_lens, beam_width=W, task_index=task, **kw)
    assert ops.last_ctc_beam_path() == 'device_lm'
    res = res.cpu().numpy()
    for i, b in enumerate(perm):
        ref = list(ys[b, :y_lens[b]])
        assert res[i, 0] == _levenshtein(list(dev_h[i]), ref) and res[i, 4] == len(ref)
    # decode_from_probs on the head's posteriors
    probs, lens, _ = model.posteriors(xs, x_lens, task_idx=task)
    got = model.decode_from_probs(probs, lens, beam_width=W, **kw)
    checked = 0
    lmp = {k: v.detach().cpu() for k, v in lm.state_dict().items()}
    for b in range(len(got)):
        r = R.search(np.log(probs[b, :lens[b]].astype(np.float64) + 1e-10), W, 0, lmp, alpha, beta,
                     normalize=False)
        if r['final_gap'] >= C.GAP and r['prune_gap'] >= C.GAP:
            np.testing.assert_array_equal(got[b], r['hyp'] - 1)
            np.testing.assert_array_equal(got[b], dev_h[b])
            checked += 1
    assert checked > 0
    return dev_h, plain


def test_model_ctc_device_vs_host(cuda_dev, monkeypatch):
    model, xs, x_lens = _model(False)
    _model_checks(model, xs, x_lens, _lm(5, 11), 0, monkeypatch)
    # width 1 with an LM: a width-1 prefix search, not the best path kernel
    lm = _lm(5, 11)
    h1, _, _ = model.decode(xs, x_lens, beam_width=1, rnnlm=lm, lm_weight=0.5)
    assert _ops().last_ctc_beam_path() == 'device_lm'
    monkeypatch.setenv('ASR_CTC_BEAM', 'host')
    h1h, _, _ = model.decode(xs, x_lens, beam_width=1, rnnlm=lm, lm_weight=0.5)
    monkeypatch.delenv('ASR_CTC_BEAM')
    _same(h1, h1h)


@pytest.mark.parametrize('task', [0, 1])
def test_model_hierarchical_device_vs_host(task, cuda_dev, monkeypatch):
    model, xs, x_lens = _model(True)
    _model_checks(model, xs, x_lens, _lm(7 if task == 0 else 5, 12 + task), task, monkeypatch)
    with pytest.raises(ValueError):      # the LM of the other head's width
        model.decode(xs, x_lens, beam_width=4, task_index=task,
                     rnnlm=_lm(5 if task == 0 else 7, 12), lm_weight=0.5)


@pytest.mark.parametrize('rnn_type,layers', [('gru', 1), ('lstm', C.MAX_LAYERS + 1)])
def test_model_host_path_for_refused_lms(rnn_type, layers, cuda_dev, monkeypatch):
    """A GRU LM and an LM one layer beyond the limit: native_ops returns None,
    the model runs the host search and says so; the result is the restatement's
    where it is safe from rounding."""
    monkeypatch.delenv('ASR_CTC_BEAM', raising=False)
    model, xs, x_lens = _model(False)
    lm = _lm(5, 21, rnn_type, layers)
    logits, lens_d, _ = model._task_logits(model.np2var(xs, dtype='float'), x_lens, 0)
    dw = dict(lm.device_weights(), weight=0.5)
    assert _ops().ctc_beam_search(logits, lens_d.to(logits.device).int(), 4, 0, lm=dw) is None
    hyps, _, perm = model.decode(xs, x_lens, beam_width=4, rnnlm=lm, lm_weight=0.5)
    assert _ops().last_ctc_beam_path() == 'host'
    assert len(hyps) == 3
    if rnn_type == 'lstm':
        lmp = {k: v.detach().cpu() for k, v in lm.state_dict().items()}
        lg, ln = logits.detach().float().cpu().numpy(), lens_d.cpu().numpy()
        checked = 0
        for b in range(3):
            r = R.search(lg[b, :ln[b]], 4, 0, lmp, 0.5, 0.0)
            if r['final_gap'] >= C.GAP and r['prune_gap'] >= C.GAP:
                np.testing.assert_array_equal(hyps[b], r['hyp'] - 1)
                checked += 1
        assert checked > 0


def test_model_refusals(cuda_dev):
    model, xs, x_lens = _model(False)
    calls = []
    enc = model._task_logits
    model._task_logits = lambda *a, **k: calls.append(1) or enc(*a, **k)
    with pytest.raises(ValueError):
        model.decode(xs, x_lens, beam_width=4, rnnlm=_lm(6, 1), lm_weight=0.5)    # LM width
    with pytest.raises(ValueError):
        model.decode(xs, x_lens, beam_width=4, rnnlm=_lm(5, 1), lm_weight=-0.5)
    with pytest.raises(ValueError):
        model.decode(xs, x_lens, beam_width=4, lm_weight=0.5)                     # no LM
    with pytest.raises(ValueError):
        model.error_rate(xs, x_lens, np.zeros((3, 2), np.int32), np.array([2, 2, 2], np.int32),
                         beam_width=4, lm_weight=0.5)
    probs = np.full((3, 11, 6), 1.0 / 6, np.float32)
    with pytest.raises(ValueError):
        model.decode_from_probs(probs, x_lens, beam_width=4, lm_weight=0.5)
    assert not calls                    # each before the encoder ran
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.decoders.\
        beam_search_decoder import BeamSearchDecoder
    with pytest.raises(ValueError):
        BeamSearchDecoder(0)(np.log(probs), x_lens, beam_width=4, alpha=0.3)


def test_existing_path_unchanged(cuda_dev, monkeypatch):
    """Calls without the new arguments take asr_ctc_beam_search and never the
    new entry point, and return what the kernel returns."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    names = []
    real_call = N.call
    monkeypatch.setattr(N, 'call', lambda name, *a: names.append(name) or real_call(name, *a))
    model, xs, x_lens = _model(False)
    hyps, _, _ = model.decode(xs, x_lens, beam_width=4)
    assert _ops().last_ctc_beam_path() == 'device'
    assert 'asr_ctc_beam_search' in names and 'asr_ctc_beam_search_lm' not in names
    logits, lens_d, _ = model._task_logits(model.np2var(xs, dtype='float'), x_lens, 0)
    h, hl, _ = _ops().ctc_beam_search(logits, lens_d.to(logits.device).int(), 4, 0, normalize=True)
    h, hl = h.cpu().numpy(), hl.cpu().numpy()
    _same(hyps, [h[b, :hl[b]].astype(np.int64) - 1 for b in range(3)])
    for b in range(3):
        lg = logits[b, :int(lens_d[b])].detach().float().cpu().numpy()
        r = R0.beam_search(R0.log_softmax(lg), 4, 0)
        if r['final_gap'] >= C.GAP and r['prune_gap'] >= C.GAP:
            np.testing.assert_array_equal(hyps[b], r['hyp'] - 1)
    # lm_weight = 0 and insertion_bonus = 0 with an LM given is the same call
    names.clear()
    h0, _, _ = model.decode(xs, x_lens, beam_width=4, rnnlm=_lm(5, 1), lm_weight=0)
    assert 'asr_ctc_beam_search' in names and _ops().last_ctc_beam_path() == 'device'
    _same(h0, hyps)
