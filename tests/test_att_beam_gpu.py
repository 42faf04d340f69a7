"""Attention beam search on the device (native_ops.att_decode_beam,
csrc/att_beam.hip) against the recorded reference fixtures, against the host
path (ASR_ATT_BEAM=host) on small random models at the sizes where the kernels
change path, on exact ties, in both compute modes, and decode_ctc's beam.

Device against host: an utterance whose host-side decision margin (_gaps) is
below 1e-3 -- about 100 x the f32 reordering error of these dot products --
is left out of the equality check; at most one in ten per case.  Scores:
within 16 x the largest f32-against-f64 score error of the CPU restatement
(tests/att_beam_ref.py) over the cases."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import att_beam_ref
from conftest import golden, golden_params

pytestmark = pytest.mark.gpu

GAP = 1e-3
LENS = [65, 64, 7, 1, 33, 20, 64, 2, 50, 12]      # 64-frame edge, L = 1, all different
BASE = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True, encoder_num_units=6,
            encoder_num_proj=0, encoder_num_layers=1, attention_type='location', attention_dim=7,
            decoder_type='lstm', decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
            dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
            num_classes=6, parameter_init=0.1, subsample_list=[False], subsample_type='drop',
            attention_conv_num_channels=3, attention_conv_width=5, bottleneck_dim=11,
            decoding_order='bahdanau', ctc_loss_weight=0, label_smoothing_prob=0,
            init_dec_state='zero')

# name -> (model kwargs, <eos> bias, decode options); SEEDS: the model seed per case, picked
# on the CPU restatement so that no utterance's margin is below 2 * GAP
CASES = {
    'v3_w4': (dict(num_classes=2), -1.5, dict(W=4, max_len=6, penalty=0.3)),   # k_top = V < W
    'v5_w4': (dict(num_classes=4), -1.5, dict(W=4, max_len=6, penalty=0.3)),
    'w2': ({}, -1.5, dict(W=2, max_len=8, penalty=0.3)),
    'w32': (dict(num_classes=33), -1.5, dict(W=32, max_len=2, penalty=0.3)),   # the largest W
    'v130': (dict(num_classes=129), -1.5, dict(W=3, max_len=3, penalty=0.3)),  # > 1 class pass per wave
    'min4_pen': ({}, 3.0, dict(W=3, max_len=8, min_len=4, penalty=0.5)),   # best class <eos>, skipped
    'maxlen1': ({}, 0.0, dict(W=3, max_len=1)),
    'eos_early': ({}, 4.0, dict(W=3, max_len=8)),                       # W complete early
    'eos_never': ({}, -30.0, dict(W=3, max_len=5)),                     # the final beam is returned
    'first': (dict(init_dec_state='first', sharpening_factor=1.5), 0.0, dict(W=3, max_len=6)),
    'content': (dict(attention_type='content'), -1.5, dict(W=3, max_len=6, penalty=0.3)),
    'dec2': (dict(decoder_num_layers=2), 0.0, dict(W=3, max_len=5)),    # _fused_ok rejects: host
}
SEEDS = {'v3_w4': 1625, 'v5_w4': 1626, 'w2': 1629, 'w32': 1623, 'v130': 1645, 'min4_pen': 1623,
         'maxlen1': 1623, 'eos_early': 1623, 'eos_never': 1626, 'first': 1626, 'content': 1626,
         'dec2': 1623}


def _model(kw_over, eos_bias, seed=1623, tie=False):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    kw = dict(BASE, **kw_over)
    torch.manual_seed(seed)
    model = AttentionSeq2seq(**kw)
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
        model.fc_0_fwd.fc.bias[kw['num_classes']] += eos_bias
        if tie:      # classes 1 and 2 tie bit for bit
            model.fc_0_fwd.fc.weight[2] = model.fc_0_fwd.fc.weight[1]
            model.fc_0_fwd.fc.bias[2] = model.fc_0_fwd.fc.bias[1]
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.set_cuda()
    model.eval()
    return model, kw, sd


def _enc(seed=7):
    rng = np.random.RandomState(seed)
    enc = rng.uniform(-1, 1, (len(LENS), max(LENS), 12)).astype(np.float32)
    for b, L in enumerate(LENS):
        enc[b, L:] = 0
    return enc


def _decode(model, enc, mode, W, max_len, min_len=0, penalty=0, gaps=None):
    from pytorch_end2end_speech_recognition_amd import native_ops
    old = os.environ.get('ASR_ATT_BEAM')
    os.environ['ASR_ATT_BEAM'] = mode
    try:
        scores = []
        with torch.no_grad():
            hyps, aws = model._decode_infer_beam(
                torch.from_numpy(enc).cuda(), np.array(LENS), W, max_len, min_len, penalty, 0,
                _gaps=gaps, _scores=scores)
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ['ASR_ATT_BEAM']
        else:
            os.environ['ASR_ATT_BEAM'] = old
    return [np.asarray(h) for h in hyps], aws, scores, native_ops.last_att_beam_path()


@functools.lru_cache(maxsize=None)
def _score_bound():
    """16 x the largest |f32 - f64| best-hypothesis score of the CPU
    restatement over the fused-eligible cases (utterances whose hypotheses
    agree in both dtypes)."""
    enc = _enc()
    worst = 0.0
    for name, (kw_over, bias, o) in CASES.items():
        if name == 'dec2':
            continue
        _, kw, sd = _model_cpu(kw_over, bias, SEEDS[name])
        a = att_beam_ref.beam_decode(sd, kw, enc, LENS, o['W'], o['max_len'], o.get('min_len', 0),
                                     o.get('penalty', 0), torch.float32)
        r = att_beam_ref.beam_decode(sd, kw, enc, LENS, o['W'], o['max_len'], o.get('min_len', 0),
                                     o.get('penalty', 0), torch.float64)
        for h32, h64, s32, s64 in zip(a[0], r[0], a[1], r[1]):
            if np.array_equal(h32, h64):
                worst = max(worst, abs(s32 - s64))
    print('att_beam: restatement f32-vs-f64 score error %.3e, bound %.3e' % (worst, 16 * worst))
    return 16 * worst


def _model_cpu(kw_over, eos_bias, seed=1623):
    """The same parameters as _model, without the device copy."""
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    kw = dict(BASE, **kw_over)
    torch.manual_seed(seed)
    model = AttentionSeq2seq(**kw)
    with torch.no_grad():
        for p in model.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
        model.fc_0_fwd.fc.bias[kw['num_classes']] += eos_bias
    return model, kw, {k: v.detach().clone() for k, v in model.state_dict().items()}


# ---------------------------------------------------------------- 1. fixtures
@pytest.mark.parametrize('name', ['beam_att', 'beam_att_first', 'beam_att_wide'])
def test_fixtures_on_device_path(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    d = golden(name)
    kw = json.loads(str(d['kwargs']))
    opts = json.loads(str(d['opts']))
    sd, _ = golden_params(d)
    torch.manual_seed(int(d['seed'][0]))
    model = AttentionSeq2seq(**kw)
    model.load_state_dict(sd)
    model.set_cuda()
    native_ops.set_compute_dtype('fp32')
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], **opts)
    assert native_ops.last_att_beam_path() == 'device'
    np.testing.assert_array_equal(perm, d['perm'])
    np.testing.assert_array_equal([len(h) for h in hyps], d['hyp_lens'])
    np.testing.assert_array_equal(np.concatenate([np.asarray(h) for h in hyps]), d['hyp_flat'])
    got = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in aw])
    np.testing.assert_allclose(got, d['aw_flat'], rtol=1e-3, atol=1e-5)


def test_hierarchical_fixture_on_device_path(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    d = golden('beam_hatt')
    kw = json.loads(str(d['kwargs']))
    opts = json.loads(str(d['opts']))
    sd, _ = golden_params(d)
    torch.manual_seed(int(d['seed'][0]))
    model = HierarchicalAttentionSeq2seq(**kw)
    model.load_state_dict(sd)
    model.set_cuda()
    native_ops.set_compute_dtype('fp32')
    for task in (0, 1):
        hyps, aw, perm = model.decode(d['xs'], d['x_lens'], task_index=task, **opts)
        assert native_ops.last_att_beam_path() == 'device'
        np.testing.assert_array_equal([len(h) for h in hyps], d['hyp_lens_%d' % task])
        np.testing.assert_array_equal(np.concatenate([np.asarray(h) for h in hyps]),
                                      d['hyp_flat_%d' % task])
        got = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in aw])
        np.testing.assert_allclose(got, d['aw_flat_%d' % task], rtol=1e-3, atol=1e-5)


# ------------------------------------------------------- 2. device vs host
@pytest.mark.parametrize('name', list(CASES))
def test_device_matches_host(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, o = CASES[name]
    model, _, _ = _model(kw_over, bias, SEEDS[name])
    enc = _enc()
    gaps = []
    ref_h, ref_aw, ref_s, path = _decode(model, enc, 'host', gaps=gaps, **o)
    assert path == 'host' and len(gaps) == len(LENS)
    got_h, got_aw, got_s, path = _decode(model, enc, 'device', **o)
    assert path == ('host' if name == 'dec2' else 'device')
    left_out = [b for b, g in enumerate(gaps) if g < GAP]
    print('att_beam %s: left out %d of %d (smallest gap %.3e)'
          % (name, len(left_out), len(LENS), min(gaps)))
    assert len(left_out) * 10 <= len(LENS)
    bound = _score_bound()
    for b in range(len(LENS)):
        if b in left_out:
            continue
        np.testing.assert_array_equal(got_h[b], ref_h[b], err_msg='utterance %d' % b)
        assert got_aw[b].shape == ref_aw[b].shape == (len(ref_h[b]), LENS[b])
        np.testing.assert_allclose(got_aw[b], ref_aw[b], rtol=1e-3, atol=1e-5)
        print('att_beam %s utt %d: score device %.9f host %.9f' % (name, b, got_s[b], ref_s[b]))
        assert abs(got_s[b] - ref_s[b]) <= bound


# ------------------------------------------------------------ 3. exact ties
def test_exact_ties_lower_class_first(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    model, _, _ = _model({}, 0.0, tie=True)
    enc = _enc()
    o = dict(W=3, max_len=6)
    ref_h, _, _, _ = _decode(model, enc, 'host', **o)
    got_h, _, _, path = _decode(model, enc, 'device', **o)
    assert path == 'device'
    flat = np.concatenate(ref_h)
    assert (flat == 1).any() or (flat == 2).any()      # the tied classes are in play
    for b in range(len(LENS)):
        np.testing.assert_array_equal(got_h[b], ref_h[b], err_msg='utterance %d' % b)


# ---------------------------------------------------- 4. both compute modes
def test_bf16_mode_equals_fp32_mode(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    model, _, _ = _model(dict(init_dec_state='first'), 0.0)
    enc = _enc()
    o = dict(W=4, max_len=8)
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


# ------------------------------------------------------- 5. decode_ctc beam
def test_decode_ctc_beam(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    d = golden('model_att_hybrid')
    kw = json.loads(str(d['kwargs']))
    sd, _ = golden_params(d)
    model = AttentionSeq2seq(**kw)
    model.load_state_dict(sd)
    model.set_cuda()
    native_ops.set_compute_dtype('fp32')
    hyps, perm = model.decode_ctc(d['xs'], d['x_lens'], beam_width=4)
    with torch.no_grad():
        model.eval()
        enc_out, lens_d, _ = model._encode(model.np2var(d['xs'], dtype='float'), d['x_lens'])
        logits = model.fc_ctc_0(enc_out)
        h, hl, _ = native_ops.ctc_beam_search(logits, lens_d, 4, blank=0)
    h, hl = h.cpu().numpy(), hl.cpu().numpy()
    assert len(hyps) == len(hl)
    for b in range(len(hl)):
        np.testing.assert_array_equal(hyps[b], h[b, :hl[b]].astype(np.int64) - 1)
