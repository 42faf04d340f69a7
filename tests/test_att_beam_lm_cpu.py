"""Shallow fusion in attention beam search without a GPU: the restatement
(tests/att_beam_lm_ref.py) -- its LM step against torch.nn.LSTM in f64, gamma = 0
against att_beam_ctc_ref.beam_decode_joint bit for bit, its f32 and f64 modes on
every case the GPU test runs (the inputs meet the margin rule without the
device), the search against brute force over all sequences -- and decode()'s
argument checks, which run before the encoder."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import att_beam_ctc_ref
import att_beam_lm_cases as C
import att_beam_lm_ref as R
from att_beam_ref import _attend
from oracle import asr_ref


@pytest.mark.parametrize('layers', [1, 2])
def test_lm_step_matches_torch_lstm_f64(layers):
    _, lm_sd = C.lm_cpu(6, dict(num_layers=layers), 3)
    lp = R.lm_params(lm_sd, torch.float64)
    rnn = torch.nn.LSTM(5, 9, layers, batch_first=True).double()
    rnn.load_state_dict({k[len('lstm.'):]: v for k, v in lp.items() if k.startswith('lstm.')})
    toks = torch.tensor([[6, 0, 3, 3, 5], [6, 2, 1, 6, 4], [1, 1, 0, 2, 2]])
    with torch.no_grad():
        want_h, _ = rnn(lp['embed.embed.weight'][toks])
        want = want_h @ lp['output.fc.weight'].t() + lp['output.fc.bias']
    h = c = torch.zeros(3, layers, 9, dtype=torch.float64)
    for t in range(toks.shape[1]):
        lg, h, c = R.lm_step(lp, toks[:, t], h, c)
        np.testing.assert_allclose(lg.numpy(), want[:, t].numpy(), rtol=1e-12, atol=1e-12)


def test_gamma_zero_is_the_joint_search_bit_for_bit():
    _, kw, sd = C.model_cpu({}, {'eos': -1.5}, 1623)
    _, lm_sd = C.lm_cpu(kw['num_classes'], {}, 1623)
    lens = [9, 1, 5, 2]
    enc = np.random.RandomState(3).uniform(-1, 1, (len(lens), max(lens), 12)).astype(np.float32)
    for dtype in (torch.float32, torch.float64):
        for lam in (0.0, 0.3):
            g0, g1 = [], []
            a = att_beam_ctc_ref.beam_decode_joint(sd, kw, enc, lens, 3, 6, 2, 0.3, dtype, g0,
                                                   ctc_weight=lam)
            r = R.beam_decode_lm(sd, kw, enc, lens, 3, 6, 2, 0.3, dtype, g1, ctc_weight=lam,
                                 lm_sd=lm_sd, lm_weight=0.0)
            assert a[1] == r[1] and g0 == g1
            for x, y in zip(a[0] + a[2], r[0] + r[2]):
                np.testing.assert_array_equal(x, y)
    # and a weight > 0 changes the scores
    j = R.beam_decode_lm(sd, kw, enc, lens, 3, 6, 2, 0.3, torch.float64, ctc_weight=0.3,
                         lm_sd=lm_sd, lm_weight=0.5)
    assert j[1] != r[1]


@pytest.mark.parametrize('name', list(C.CASES))
def test_cases_meet_the_margin_rule_in_both_modes(name):
    r64, r32 = C.ref(name, True), C.ref(name, False)
    print('att_beam_lm %s: smallest margin f64 %.3e, f32 %.3e' % (name, min(r64[3]), min(r32[3])))
    assert min(r64[3]) >= 2 * C.GAP and min(r32[3]) >= 2 * C.GAP
    for b in range(len(C.LENS)):
        np.testing.assert_array_equal(r32[0][b], r64[0][b], err_msg='utterance %d' % b)


def test_diff_case_meets_the_margin_rule():
    kw_over, bias, lm_over, o, seed = C.DIFF
    r0 = C.restate(kw_over, bias, lm_over, seed, o, torch.float64, gam=0.0)
    r5 = C.restate(kw_over, bias, lm_over, seed, o, torch.float64, gam=0.5)
    assert min(r0[3]) >= 2 * C.GAP and min(r5[3]) >= 2 * C.GAP
    assert sum(not np.array_equal(a, b) for a, b in zip(r0[0], r5[0])) >= 3


def _sequence_score(p, lmp, kw, enc, seq, gam, penalty):
    """The fused score of one token sequence, teacher forced on one row."""
    eos = kw['num_classes']
    L = enc.shape[1]
    enc_a = asr_ref.linear_nd(p, 'attend_0_fwd.W_enc_head0', enc)
    h = c = enc.new_zeros(1, kw['decoder_num_units'])
    ctx, aw = enc.new_zeros(1, enc.shape[2]), enc.new_zeros(1, L)
    lh = lc = enc.new_zeros(1, R.lm_layers(lmp), lmp['lstm.weight_hh_l0'].shape[1])
    score, last = 0.0, eos
    for t, tok in enumerate(seq):
        if t > 0:
            x = torch.cat([p['embed_0.embed.weight'][[last]], ctx], dim=-1)
            h, c = asr_ref.lstm_cell(p, 'decoder_0_fwd.lstm_l0', x, h, c)
        ctx, aw = _attend(p, 'attend_0_fwd.', enc, enc_a, h, aw, 1, False)
        z = torch.tanh(asr_ref.linear_nd(p, 'W_d_0_fwd', h) + asr_ref.linear_nd(p, 'W_c_0_fwd', ctx))
        lp = torch.log_softmax(asr_ref.linear_nd(p, 'fc_0_fwd', z), dim=1)
        lg, lh, lc = R.lm_step(lmp, torch.tensor([last]), lh, lc)
        score += float(lp[0, tok]) + gam * float(torch.log_softmax(lg, dim=1)[0, tok]) + penalty
        last = tok
    return score


@torch.no_grad()
def test_search_against_brute_force():
    """V 3, max_decode_len 3, W 32: with min(W, V) = V candidates per row and
    W >= 3 + 9 + 27 nothing is ever pruned, so the candidate rule reaches every
    sequence; `complete` never fills, so the answer is the best sequence that
    ends in <eos> within 3 tokens -- its fused score the maximum over them."""
    gam, penalty = 0.7, 0.3
    _, kw, sd = C.model_cpu(dict(num_classes=2, ctc_loss_weight=0), {}, 1623)
    _, lm_sd = C.lm_cpu(2, {}, 1623)
    lens = [7, 1, 4]
    enc = np.random.RandomState(5).uniform(-1, 1, (len(lens), max(lens), 12))
    hyps, scores, _ = R.beam_decode_lm(sd, kw, enc, lens, 32, 3, 0, penalty, torch.float64,
                                       lm_sd=lm_sd, lm_weight=gam)
    p = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    lmp = R.lm_params(lm_sd, torch.float64)
    eos = 2
    seqs = [s + (eos,) for n in (0, 1, 2) for s in itertools.product(range(2), repeat=n)]
    for b, L in enumerate(lens):
        e = torch.as_tensor(enc[b:b + 1, :L])
        table = {s: _sequence_score(p, lmp, kw, e, s, gam, penalty) for s in seqs}
        best = max(table, key=table.get)
        assert tuple(hyps[b]) == best
        assert scores[b] == pytest.approx(table[best], rel=1e-12, abs=1e-12)
        # the LM matters on this input: without it another score wins
        assert table[best] != pytest.approx(_sequence_score(p, lmp, kw, e, best, 0.0, penalty))


XS = np.zeros((2, 5, 8), np.float32)
X_LENS = np.array([5, 4])


def _model(**over):
    return C.model_cpu(over, {}, 1623)[0]


def test_negative_lm_weight_raises_value_error():
    lm, _ = C.lm_cpu(6, {}, 1)
    with pytest.raises(ValueError, match='negative'):
        _model().decode(XS, X_LENS, 3, 4, rnnlm=lm, lm_weight=-0.1)
    with pytest.raises(ValueError, match='negative'):
        _model().decode(XS, X_LENS, 3, 4, lm_weight=-0.1)


def test_greedy_with_lm_weight_raises_value_error():
    lm, _ = C.lm_cpu(6, {}, 1)
    with pytest.raises(ValueError, match='beam_width'):
        _model().decode(XS, X_LENS, 1, 4, rnnlm=lm, lm_weight=0.3)


def test_class_count_mismatch_raises_value_error():
    lm, _ = C.lm_cpu(5, {}, 1)
    with pytest.raises(ValueError, match='num_classes'):
        _model().decode(XS, X_LENS, 3, 4, rnnlm=lm, lm_weight=0.3)


def test_backward_decoder_raises_not_implemented():
    lm, _ = C.lm_cpu(6, {}, 1)
    with pytest.raises(NotImplementedError, match='backward'):
        _model(backward_loss_weight=1.0).decode(XS, X_LENS, 3, 4, rnnlm=lm, lm_weight=0.3)


def test_hierarchical_checks_the_sub_task_class_count():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    kw = {k: v for k, v in C.BASE.items() if k != 'ctc_loss_weight'}
    kw.update(encoder_num_layers=2, encoder_num_layers_sub=1, decoder_num_units_sub=9,
              decoder_num_layers_sub=1, embedding_dim_sub=4, num_classes_sub=5,
              main_loss_weight=0.5, sub_loss_weight=0.3, ctc_loss_weight_sub=0.2,
              subsample_list=[False, False])
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    lm, _ = C.lm_cpu(6, {}, 1)          # the main task's classes, not the sub task's
    with pytest.raises(ValueError, match='num_classes'):
        model.decode(XS, X_LENS, 3, 4, task_index=1, rnnlm=lm, lm_weight=0.3)


def test_lm_workspace_adds_state_logits_and_candidate_terms():
    from pytorch_end2end_speech_recognition_amd import _native as N
    B, T, W, V, layers, H = 32, 250, 10, 29, 2, 512
    d = N.AttDecDims(B, T, 640, 128, 10, 201, 320, 1, 1.0, 0)
    q = (ctypes.byref(d), W, V, 64, 256, 100)
    ctc = N.AttBeamCtc(None, 30, 0, 1, 0.3)

    def query(lm_dims, with_ctc=False):
        """The query reads ctc != NULL, lm != NULL and the LM's layers / H / Y only."""
        lm = N.AttBeamLm(*lm_dims) if lm_dims else None
        ex = N.AttBeamEx(N.ATT_BEAM_CELL_LSTM, ctypes.addressof(ctc) if with_ctc else None,
                         ctypes.addressof(lm) if lm is not None else None)
        return N.query('asr_att_beam_ws_bytes', *(q + (ctypes.byref(ex),)))
    joint = query(None, with_ctc=True)
    lm = query((layers, H, 512))
    Rw = B * W
    add = (4 * Rw * layers * H + Rw * V + Rw * W) * 4
    assert joint > 0 and add <= lm - joint <= add + 4 * 256
    # the documented refusals: more than 4 layers, the cell's LDS need above 64 KiB
    assert query((5, H, 512)) == 0
    assert query((1, 6000, 512)) == 0
    # 2 max(Y, H) + H floats: 65 532 B fits, 65 544 B does not
    assert query((1, 5461, 5461)) > 0
    assert query((1, 5462, 5462)) == 0
    # the byte counts of asr_att_beam_ws_bytes / _ctc_ws_bytes / _lm_ws_bytes before the
    # three queries became one (recorded from that build at these shapes); the LM's size
    # holds the joint search's part whatever lambda is
    plain = N.query('asr_att_beam_ws_bytes', *(q + (None,)))
    assert (plain, joint, lm) == (35617024, 38297344, 43590144)
    assert query((layers, H, 512), with_ctc=True) == lm
