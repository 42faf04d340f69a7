"""Joint CTC/attention beam search without a GPU: the CTC prefix scorers (the
restatement tests/att_beam_ctc_ref.py and the host path's numpy scorer) against
brute force over all alignments, the restatement at weight 0 against
att_beam_ref.beam_decode, decode()'s argument checks (they run before the
encoder), and the joint workspace query."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import att_beam_ctc_ref as R
import att_beam_ref

NLAB = 3                      # attention classes 0..2 = CTC classes 1..3, <eos> = 3
PREFIXES = [h for n in (1, 2, 3) for h in itertools.product(range(NLAB), repeat=n)]


def _lp(L, seed):
    rng = np.random.RandomState(seed)
    lg = rng.uniform(-2, 2, (L, NLAB + 1))
    return lg - np.log(np.exp(lg).sum(axis=1, keepdims=True))


def _brute(lp):
    """{collapsed label sequence: probability} over every alignment of the L frames."""
    L = lp.shape[0]
    out = {}
    for path in itertools.product(range(NLAB + 1), repeat=L):
        pr = math.exp(sum(lp[t, k] for t, k in enumerate(path)))
        seq = tuple(k - 1 for j, k in enumerate(path) if k != 0 and (j == 0 or k != path[j - 1]))
        out[seq] = out.get(seq, 0.0) + pr
    return out


def _check(value, prob):
    """log(prob), or a dead prefix: LOGZERO up to the few units the recursion adds."""
    if prob == 0.0:
        assert value < -1e9
    else:
        assert value == pytest.approx(math.log(prob), rel=1e-10, abs=1e-10)


@pytest.mark.parametrize('L', [1, 2, 3, 4, 5])
def test_prefix_scorer_against_brute_force(L):
    lp = _lp(L, 10 + L)
    table = _brute(lp)
    assert sum(table.values()) == pytest.approx(1.0, rel=1e-12)
    sc = R.PrefixScorer(lp)
    dead = 0
    for h in PREFIXES:
        st = sc.empty()
        for j in range(len(h) - 1):
            st = sc.advance(st, list(h[:j]), h[j])
        starts = sum(pr for seq, pr in table.items() if seq[:len(h)] == h)
        psi = sc.psi(st, list(h[:-1]), h[-1])
        _check(psi, starts)
        full = sc.advance(st, list(h[:-1]), h[-1])
        assert full[2] == psi                                # psi travels with the row
        _check(sc.eos_term(full), table.get(h, 0.0))          # the <eos> term: exactly h
        # the candidate terms as the search forms them
        assert sc.delta(st, list(h[:-1]), h[-1], NLAB) == psi - st[2]
        assert sc.delta(full, list(h), NLAB, NLAB) == sc.eos_term(full) - psi
        dead += starts == 0.0
    # |h| > L, and a repeated label needs a blank between: h = (1, 1) is dead at L = 2
    assert dead > 0 if L < 5 else dead == 0
    _check(sc.eos_term(sc.empty()), table.get((), 0.0))


@pytest.mark.parametrize('L', [1, 2, 3, 4, 5])
def test_host_path_scorer_against_brute_force(L):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.ctc_prefix_score \
        import CtcPrefixScorer
    lp = _lp(L, 20 + L)
    table = _brute(lp)
    sc = CtcPrefixScorer(lp)
    for h in PREFIXES:
        st = sc.empty()
        for j in range(len(h) - 1):
            st = sc.advance(st, list(h[:j]), h[j], sc.psi(st, list(h[:j]), h[j]))
        psi = sc.psi(st, list(h[:-1]), h[-1])
        _check(psi, sum(pr for seq, pr in table.items() if seq[:len(h)] == h))
        full = sc.advance(st, list(h[:-1]), h[-1], psi)
        _check(sc.eos(full), table.get(h, 0.0))


BASE = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True, encoder_num_units=6,
            encoder_num_proj=0, encoder_num_layers=1, attention_type='location', attention_dim=7,
            decoder_type='lstm', decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
            dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
            num_classes=6, parameter_init=0.1, subsample_list=[False], subsample_type='drop',
            attention_conv_num_channels=3, attention_conv_width=5, bottleneck_dim=11,
            decoding_order='bahdanau', ctc_loss_weight=0.2, label_smoothing_prob=0,
            init_dec_state='zero')


def _model(**over):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    torch.manual_seed(1623)
    model = AttentionSeq2seq(**dict(BASE, **over))
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
    return model


def test_weight_zero_is_the_attention_search():
    model = _model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    lens = [9, 1, 5, 2]
    rng = np.random.RandomState(3)
    enc = rng.uniform(-1, 1, (len(lens), max(lens), 12)).astype(np.float32)
    for dtype in (torch.float32, torch.float64):
        g0, g1 = [], []
        a = att_beam_ref.beam_decode(sd, BASE, enc, lens, 3, 6, 2, 0.3, dtype, g0)
        r = R.beam_decode_joint(sd, BASE, enc, lens, 3, 6, 2, 0.3, dtype, g1, ctc_weight=0.0)
        assert a[1] == r[1] and g0 == g1
        for x, y in zip(a[0] + a[2], r[0] + r[2]):
            np.testing.assert_array_equal(x, y)
    # and a weight > 0 changes the scores
    j = R.beam_decode_joint(sd, BASE, enc, lens, 3, 6, 2, 0.3, torch.float64, ctc_weight=0.5)
    assert j[1] != r[1]


XS = np.zeros((2, 5, 8), np.float32)
X_LENS = np.array([5, 4])


def test_decode_without_ctc_head_raises_value_error():
    model = _model(ctc_loss_weight=0)
    with pytest.raises(ValueError, match='fc_ctc_0'):
        model.decode(XS, X_LENS, 3, 4, ctc_weight=0.3)


def test_decode_backward_decoder_raises_not_implemented():
    model = _model(backward_loss_weight=1.0)
    with pytest.raises(NotImplementedError, match='backward'):
        model.decode(XS, X_LENS, 3, 4, ctc_weight=0.3)


def test_decode_greedy_with_ctc_weight_raises_value_error():
    model = _model()
    with pytest.raises(ValueError, match='beam_width'):
        model.decode(XS, X_LENS, 1, 4, ctc_weight=0.3)
    with pytest.raises(ValueError, match='outside'):
        model.decode(XS, X_LENS, 3, 4, ctc_weight=1.5)


def test_hierarchical_main_task_has_no_ctc_head():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    kw = {k: v for k, v in BASE.items() if k != 'ctc_loss_weight'}
    kw.update(encoder_num_layers=2, encoder_num_layers_sub=1, encoder_num_units=6,
              decoder_num_units_sub=9, decoder_num_layers_sub=1, embedding_dim_sub=4,
              num_classes_sub=5, main_loss_weight=0.5, sub_loss_weight=0.3,
              ctc_loss_weight_sub=0.2, subsample_list=[False, False])
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    with pytest.raises(ValueError, match='fc_ctc_0'):
        model.decode(XS, X_LENS, 3, 4, task_index=0, ctc_weight=0.3)


def test_joint_workspace_adds_the_prefix_state():
    from pytorch_end2end_speech_recognition_amd import _native as N
    B, T, W = 32, 250, 10
    d = N.AttDecDims(B, T, 640, 128, 10, 201, 320, 1, 1.0, 0)
    ctc = N.AttBeamCtc(None, 30, 0, 1, 0.3)
    ex = ctypes.byref(N.AttBeamEx(N.ATT_BEAM_CELL_LSTM, ctypes.addressof(ctc), None))
    plain = N.query('asr_att_beam_ws_bytes', ctypes.byref(d), W, 29, 64, 256, 100, None)
    joint = N.query('asr_att_beam_ws_bytes', ctypes.byref(d), W, 29, 64, 256, 100, ex)
    add = 2 * B * T * 4 + (4 * B * W * T + 2 * B * W + 2 * B * W * W) * 8
    assert plain > 0 and add <= joint - plain <= add + 8 * 256
    assert N.query('asr_att_beam_ws_bytes', ctypes.byref(d), 33, 29, 64, 256, 100, ex) == 0
    # the byte counts of asr_att_beam_ws_bytes / asr_att_beam_ctc_ws_bytes before the two
    # queries became one (recorded from that build at these shapes)
    assert (plain, joint) == (35617024, 38297344)
    # an ex without either optional part is the plain query
    none = ctypes.byref(N.AttBeamEx(N.ATT_BEAM_CELL_GRU, None, None))
    assert N.query('asr_att_beam_ws_bytes', ctypes.byref(d), W, 29, 64, 256, 100, none) == plain
