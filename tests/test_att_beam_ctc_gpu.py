"""Joint CTC/attention beam search (decode(..., ctc_weight > 0); csrc/att_beam.hip
beam_ctc_lse / _empty / _advance / _score, beam_select_ctc) against the float64
restatement tests/att_beam_ctc_ref.py and against the host path
(ASR_ATT_BEAM=host) on small random hybrid models.

The equality rule is tests/test_att_beam_gpu.py's: an utterance whose reference
margin is below GAP = 1e-3 is left out of the hypothesis check, at most one in
ten per case; the model seeds are picked on the CPU so that the f64 restatement
has every margin >= 2 GAP and itself leaves out none.  Scores: within 16 x the
largest f32-mode against f64-mode best-score difference of the restatement over
the cases (utterances whose hypotheses agree), recomputed and printed here; it
is asserted for best scores above -1e9 only -- a dead-prefix winner sits near
weight * LOGZERO, where a double's spacing exceeds the bound."""
import functools
import os

import numpy as np
import pytest
import torch

import att_beam_ctc_ref as R
import edit_distance_ref

pytestmark = pytest.mark.gpu

GAP = 1e-3
LENS = [65, 64, 7, 1, 33, 20, 64, 2, 50, 12]      # 64-lane edge, L = 1, L = 2
BASE = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True, encoder_num_units=6,
            encoder_num_proj=0, encoder_num_layers=1, attention_type='location', attention_dim=7,
            decoder_type='lstm', decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
            dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
            num_classes=6, parameter_init=0.1, subsample_list=[False], subsample_type='drop',
            attention_conv_num_channels=3, attention_conv_width=5, bottleneck_dim=11,
            decoding_order='bahdanau', ctc_loss_weight=0.2, label_smoothing_prob=0,
            init_dec_state='zero')

# name -> (model kwargs, output-bias additions {class: value} ('eos': the <eos> class),
#          decode options)
CASES = {
    'lam03': ({}, {'eos': -1.5}, dict(W=3, max_len=6, penalty=0.3, lam=0.3)),
    'lam07': ({}, {'eos': -1.5}, dict(W=3, max_len=6, penalty=0.3, lam=0.7)),
    'w2': ({}, {'eos': -1.5}, dict(W=2, max_len=8, penalty=0.3, lam=0.3)),
    'w32': (dict(num_classes=33), {'eos': -1.5}, dict(W=32, max_len=2, penalty=0.3, lam=0.3)),
    'v3_w4': (dict(num_classes=2), {'eos': -1.5}, dict(W=4, max_len=6, penalty=0.3, lam=0.3)),
    'v130': (dict(num_classes=129), {'eos': -1.5}, dict(W=3, max_len=3, penalty=0.3, lam=0.3)),
    'lam1': ({}, {'eos': -1.5}, dict(W=3, max_len=6, penalty=0.3, lam=1.0)),   # attention only prunes
    'repeat': ({}, {'eos': -3.0, 1: 3.0}, dict(W=3, max_len=6, lam=0.3)),      # c == last(g)
    'min4_eos': ({}, {'eos': 3.0}, dict(W=3, max_len=8, min_len=4, penalty=0.5, lam=0.3)),
    'eos_never': ({}, {'eos': -30.0}, dict(W=3, max_len=5, lam=0.3)),   # max_len > L: dead prefixes
    'eos_early': ({}, {'eos': 20.0}, dict(W=3, max_len=8, lam=0.1)),    # W complete early
    'first': (dict(init_dec_state='first', sharpening_factor=1.5), {}, dict(W=3, max_len=6, lam=0.3)),
    'content': (dict(attention_type='content'), {'eos': -1.5},
                dict(W=3, max_len=6, penalty=0.3, lam=0.3)),
    'dec2': (dict(decoder_num_layers=2), {}, dict(W=3, max_len=5, lam=0.3)),   # _fused_ok rejects: host
}
# the model seed per case: on the f64 restatement no utterance's margin is below 2 * GAP
SEEDS = {'lam03': 1627, 'lam07': 1628, 'w2': 1625, 'w32': 2056, 'v3_w4': 1625, 'v130': 1632,
         'lam1': 1627, 'repeat': 1625, 'min4_eos': 1624, 'eos_never': 1625, 'eos_early': 1623,
         'first': 1630, 'content': 1633, 'dec2': 1628}
# a model on which the restatement's weight 0 and weight 0.5 hypotheses differ (9 of 10
# utterances), both with every margin >= 2 * GAP
DIFF = ({}, {'eos': -1.5}, dict(W=3, max_len=6, penalty=0.3), 1637)


def _model_cpu(kw_over, bias, seed):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    kw = dict(BASE, **kw_over)
    torch.manual_seed(seed)
    model = AttentionSeq2seq(**kw)
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
        for c, v in bias.items():
            model.fc_0_fwd.fc.bias[kw['num_classes'] if c == 'eos' else c] += v
    return model, kw, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _model(kw_over, bias, seed):
    model, kw, sd = _model_cpu(kw_over, bias, seed)
    model.set_cuda()
    model.eval()
    return model, kw, sd


def _enc(seed=7):
    rng = np.random.RandomState(seed)
    enc = rng.uniform(-1, 1, (len(LENS), max(LENS), 12)).astype(np.float32)
    for b, L in enumerate(LENS):
        enc[b, L:] = 0
    return enc


def _restate(kw_over, bias, seed, o, dtype, lam=None):
    """(hyps, scores, aws, gaps) of the restatement."""
    _, kw, sd = _model_cpu(kw_over, bias, seed)
    gaps = []
    out = R.beam_decode_joint(sd, kw, _enc(), LENS, o['W'], o['max_len'], o.get('min_len', 0),
                              o.get('penalty', 0), dtype, gaps,
                              ctc_weight=o['lam'] if lam is None else lam)
    return out + (gaps,)


@functools.lru_cache(maxsize=None)
def _ref(name, f64=True):
    """The restatement of a case, computed once and shared."""
    kw_over, bias, o = CASES[name]
    return _restate(kw_over, bias, SEEDS[name], o, torch.float64 if f64 else torch.float32)


@functools.lru_cache(maxsize=None)
def _score_bound():
    """16 x the largest |f32 mode - f64 mode| best score of the restatement over
    the cases, over utterances whose hypotheses agree in both modes."""
    worst = 0.0
    for name in CASES:
        a, r = _ref(name, False), _ref(name, True)
        for h32, h64, s32, s64 in zip(a[0], r[0], a[1], r[1]):
            if np.array_equal(h32, h64) and s64 > -1e9:
                worst = max(worst, abs(s32 - s64))
    print('att_beam_ctc: restatement f32-vs-f64 score error %.3e, bound %.3e' % (worst, 16 * worst))
    return 16 * worst


def _decode(model, enc, mode, W, max_len, min_len=0, penalty=0, lam=0.0, gaps=None, kw=True):
    from pytorch_end2end_speech_recognition_amd import native_ops
    old = os.environ.get('ASR_ATT_BEAM')
    os.environ['ASR_ATT_BEAM'] = mode
    try:
        scores = []
        extra = dict(ctc_weight=lam) if kw else {}
        with torch.no_grad():
            hyps, aws = model._decode_infer_beam(
                torch.from_numpy(enc).cuda(), np.array(LENS), W, max_len, min_len, penalty, 0,
                _gaps=gaps, _scores=scores, **extra)
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ['ASR_ATT_BEAM']
        else:
            os.environ['ASR_ATT_BEAM'] = old
    return [np.asarray(h) for h in hyps], aws, scores, native_ops.last_att_beam_path()


# ------------------------------------------- 1. device vs restatement vs host
@pytest.mark.parametrize('name', list(CASES))
def test_device_matches_restatement_and_host(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, o = CASES[name]
    ref_h, ref_s, ref_aw, ref_gaps = _ref(name)
    assert min(ref_gaps) >= 2 * GAP                      # the reference alone leaves out 0 of 10
    model, _, _ = _model(kw_over, bias, SEEDS[name])
    enc = _enc()
    gaps = []
    host_h, host_aw, host_s, path = _decode(model, enc, 'host', gaps=gaps, **o)
    assert path == 'host' and len(gaps) == len(LENS)
    got_h, got_aw, got_s, path = _decode(model, enc, 'device', **o)
    assert path == ('host' if name == 'dec2' else 'device')
    left_out = [b for b, g in enumerate(gaps) if g < GAP]
    print('att_beam_ctc %s: left out %d of %d (smallest gap host %.3e, restatement %.3e)'
          % (name, len(left_out), len(LENS), min(gaps), min(ref_gaps)))
    assert len(left_out) * 10 <= len(LENS)
    bound = _score_bound()
    for b in range(len(LENS)):
        print('att_beam_ctc %s utt %d: score device %.9f host %.9f restatement %.9f'
              % (name, b, got_s[b], host_s[b], ref_s[b]))
        np.testing.assert_array_equal(got_h[b], ref_h[b], err_msg='utterance %d' % b)
        np.testing.assert_allclose(got_aw[b], ref_aw[b], rtol=1e-3, atol=1e-5)
        if ref_s[b] > -1e9:
            assert abs(got_s[b] - ref_s[b]) <= bound
        if b in left_out:
            continue
        np.testing.assert_array_equal(got_h[b], host_h[b], err_msg='utterance %d' % b)
        assert got_aw[b].shape == host_aw[b].shape == (len(host_h[b]), LENS[b])
        np.testing.assert_allclose(got_aw[b], host_aw[b], rtol=1e-3, atol=1e-5)
        if host_s[b] > -1e9:
            assert abs(got_s[b] - host_s[b]) <= bound


# -------------------------------------------- 2. the scorer changes the result
def test_ctc_weight_changes_hypotheses(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, o, seed = DIFF
    r0 = _restate(kw_over, bias, seed, o, torch.float64, lam=0.0)
    r5 = _restate(kw_over, bias, seed, o, torch.float64, lam=0.5)
    assert min(r0[3]) >= 2 * GAP and min(r5[3]) >= 2 * GAP
    differ = [b for b in range(len(LENS)) if not np.array_equal(r0[0][b], r5[0][b])]
    assert differ
    model, _, _ = _model(kw_over, bias, seed)
    got_h, _, _, path = _decode(model, _enc(), 'device', lam=0.5, **o)
    assert path == 'device'
    for b in range(len(LENS)):
        np.testing.assert_array_equal(got_h[b], r5[0][b], err_msg='utterance %d' % b)


# ------------------------------------------------ 3. weight 0 is today's path
def test_weight_zero_is_bit_equal_to_no_keyword(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, o = CASES['lam03']
    o = dict(o, lam=0.0)
    model, _, _ = _model(kw_over, bias, SEEDS['lam03'])
    enc = _enc()
    h0, aw0, s0, path = _decode(model, enc, 'device', kw=False, **o)
    assert path == 'device'
    h1, aw1, s1, path = _decode(model, enc, 'device', **o)
    assert path == 'device'
    assert s0 == s1
    for b in range(len(LENS)):
        np.testing.assert_array_equal(h0[b], h1[b])
        np.testing.assert_array_equal(aw0[b], aw1[b])


# ---------------------------------------------------- 4. both compute modes
def test_bf16_mode_equals_fp32_mode(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    kw_over, bias, o = CASES['first']
    model, _, _ = _model(kw_over, bias, SEEDS['first'])
    enc = _enc()
    native_ops.set_compute_dtype('fp32')
    h32, aw32, s32, _ = _decode(model, enc, 'device', **o)
    native_ops.set_compute_dtype('bf16')
    try:
        h16, aw16, s16, path = _decode(model, enc, 'device', **o)
    finally:
        native_ops.set_compute_dtype('fp32')
    assert path == 'device'
    assert s16 == s32
    for b in range(len(LENS)):
        np.testing.assert_array_equal(h16[b], h32[b])
        np.testing.assert_array_equal(aw16[b], aw32[b])


# ------------------------------------------------------------ 5. error_rate
def test_error_rate_with_ctc_weight(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    model, kw, _ = _model({}, {'eos': -1.5}, 1623)
    rng = np.random.RandomState(5)
    B, T = 6, 30
    x_lens = np.array([30, 25, 21, 14, 9, 4])
    xs = rng.uniform(-1, 1, (B, T, 8)).astype(np.float32)
    y_lens = np.array([5, 4, 6, 3, 2, 1])
    ys = np.full((B, 6), -1, np.int64)
    for b in range(B):
        xs[b, x_lens[b]:] = 0
        ys[b, :y_lens[b]] = rng.randint(0, kw['num_classes'], y_lens[b])
    out = model.error_rate(xs, x_lens, ys, y_lens, 3, max_decode_len=6, ctc_weight=0.3)
    assert native_ops.last_att_beam_path() == 'device'
    hyps, _, perm = model.decode(xs, x_lens, 3, 6, ctc_weight=0.3)
    hyps = [np.asarray(h) for h in hyps]
    plain, _, _ = model.decode(xs, x_lens, 3, 6)
    want = edit_distance_ref.score(hyps, [len(h) for h in hyps], ys[perm], y_lens[perm],
                                   eos=model.eos_0)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert sum(len(h) for h in hyps) > 0
    print('att_beam_ctc error_rate: %d of %d hypotheses differ from the weight 0 decode'
          % (sum(not np.array_equal(a, np.asarray(b)) for a, b in zip(hyps, plain)), B))


# --------------------------------------------------- 6. hierarchical, task 1
def test_hierarchical_sub_task(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    native_ops.set_compute_dtype('fp32')
    kw = {k: v for k, v in BASE.items() if k != 'ctc_loss_weight'}
    kw.update(encoder_num_layers=2, encoder_num_layers_sub=1, decoder_num_units_sub=9,
              decoder_num_layers_sub=1, embedding_dim_sub=4, num_classes_sub=5,
              main_loss_weight=0.5, sub_loss_weight=0.3, ctc_loss_weight_sub=0.2,
              subsample_list=[False, False], bottleneck_dim_sub=11)
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
        model.fc_1_fwd.fc.bias[5] -= 1.5
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.set_cuda()
    rng = np.random.RandomState(11)
    x_lens = np.array([40, 33, 31, 27, 20, 16, 9, 5, 2, 1])
    B = len(x_lens)
    xs = rng.uniform(-1, 1, (B, 40, 8)).astype(np.float32)
    for b in range(B):
        xs[b, x_lens[b]:] = 0
    with pytest.raises(ValueError):
        model.decode(xs, x_lens, 3, 5, task_index=0, ctc_weight=0.3)
    hyps, aw, perm = model.decode(xs, x_lens, 3, 5, length_penalty=0.3, task_index=1,
                                  ctc_weight=0.3)
    assert native_ops.last_att_beam_path() == 'device'
    with torch.no_grad():
        _, _, enc_sub, _, _ = model._encode(model.np2var(xs, dtype='float'), x_lens,
                                            is_multi_task=True)
    lens_sub = model.encoder.last_lens_sub_np
    gaps = []
    ref_h, _, ref_aw = R.beam_decode_joint(sd, kw, enc_sub.float().cpu().numpy(), lens_sub, 3, 5,
                                           0, 0.3, torch.float64, gaps, ctc_weight=0.3, task=1,
                                           num_classes=5, num_units=9)
    left_out = [b for b, g in enumerate(gaps) if g < GAP]
    print('att_beam_ctc hierarchical: left out %d of %d (smallest gap %.3e)'
          % (len(left_out), B, min(gaps)))
    assert len(left_out) * 10 <= B
    for b in range(B):
        if b in left_out:
            continue
        np.testing.assert_array_equal(np.asarray(hyps[b]), ref_h[b], err_msg='utterance %d' % b)
        np.testing.assert_allclose(aw[b], ref_aw[b], rtol=1e-3, atol=1e-5)
