"""Shallow fusion in attention beam search (decode(..., rnnlm=, lm_weight > 0);
csrc/att_beam.hip beam_lm_cell / beam_lm_score / beam_select_lm /
beam_select_ctc_lm) against the float64 restatement tests/att_beam_lm_ref.py and
against the host path (ASR_ATT_BEAM=host) on the cases of
tests/att_beam_lm_cases.py.

The equality rule is tests/test_att_beam_ctc_gpu.py's: an utterance whose
host-side margin is below GAP = 1e-3 is left out of the hypothesis check, at most
one in ten per case; the seeds are picked on the CPU so that the restatement has
every margin >= 2 GAP (tests/test_att_beam_lm_cpu.py).  Scores: within 16 x the
largest f32-mode against f64-mode best-score difference of the restatement over
the cases, recomputed and printed here, for best scores above -1e9 (a
dead-prefix winner of the joint search sits near weight * LOGZERO)."""
import os

import numpy as np
import pytest
import torch

import att_beam_lm_cases as C
import edit_distance_ref

pytestmark = pytest.mark.gpu

GAP, LENS = C.GAP, C.LENS


def _pair(kw_over, bias, lm_over, seed, rnn_type='lstm'):
    model, kw, _ = C.model_cpu(kw_over, bias, seed)
    lm, _ = C.lm_cpu(kw['num_classes'], lm_over, seed, rnn_type)
    model.set_cuda()
    model.eval()
    lm.set_cuda()
    lm.eval()
    return model, lm


def _decode(model, lm, enc, mode, W, max_len, min_len=0, penalty=0, gam=0.0, lam=0.0, gaps=None,
            kw=True):
    from pytorch_end2end_speech_recognition_amd import native_ops
    old = os.environ.get('ASR_ATT_BEAM')
    os.environ['ASR_ATT_BEAM'] = mode
    try:
        scores = []
        extra = dict(rnnlm=lm, lm_weight=gam) if kw else {}
        if lam > 0:
            extra['ctc_weight'] = lam
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
@pytest.mark.parametrize('name', list(C.CASES))
def test_device_matches_restatement_and_host(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, lm_over, o = C.CASES[name]
    ref_h, ref_s, ref_aw, ref_gaps = C.ref(name)
    assert min(ref_gaps) >= 2 * GAP                      # the reference alone leaves out 0 of 10
    model, lm = _pair(kw_over, bias, lm_over, C.SEEDS[name])
    enc = C.enc_out()
    gaps = []
    host_h, host_aw, host_s, path = _decode(model, lm, enc, 'host', gaps=gaps, **o)
    assert path == 'host' and len(gaps) == len(LENS)
    got_h, got_aw, got_s, path = _decode(model, lm, enc, 'device', **o)
    assert path == ('host' if name == 'dec2' else 'device')
    left_out = [b for b, g in enumerate(gaps) if g < GAP]
    print('att_beam_lm %s: left out %d of %d (smallest gap host %.3e, restatement %.3e)'
          % (name, len(left_out), len(LENS), min(gaps), min(ref_gaps)))
    assert len(left_out) * 10 <= len(LENS)
    bound = C.score_bound()
    for b in range(len(LENS)):
        print('att_beam_lm %s utt %d: score device %.9f host %.9f restatement %.9f'
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


# ------------------------------------------------ 2. the LM changes the result
def test_lm_weight_changes_hypotheses(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, lm_over, o, seed = C.DIFF
    r0 = C.restate(kw_over, bias, lm_over, seed, o, torch.float64, gam=0.0)
    r5 = C.restate(kw_over, bias, lm_over, seed, o, torch.float64, gam=0.5)
    assert min(r0[3]) >= 2 * GAP and min(r5[3]) >= 2 * GAP
    differ = [b for b in range(len(LENS)) if not np.array_equal(r0[0][b], r5[0][b])]
    assert differ
    model, lm = _pair(kw_over, bias, lm_over, seed)
    got0, _, _, path = _decode(model, lm, C.enc_out(), 'device', gam=0.0, **o)
    assert path == 'device'
    got5, _, _, path = _decode(model, lm, C.enc_out(), 'device', gam=0.5, **o)
    assert path == 'device'
    for b in range(len(LENS)):
        np.testing.assert_array_equal(got0[b], r0[0][b], err_msg='utterance %d' % b)
        np.testing.assert_array_equal(got5[b], r5[0][b], err_msg='utterance %d' % b)


# ------------------------------------------------ 3. weight 0 is today's path
@pytest.mark.parametrize('lam', [0.0, 0.3])
def test_weight_zero_and_no_lm_are_bit_equal_to_no_keyword(lam, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, lm_over, o = C.CASES['g03']
    o = dict(o, lam=lam)
    model, lm = _pair(kw_over, bias, lm_over, C.SEEDS['g03'])
    enc = C.enc_out()
    h0, aw0, s0, path = _decode(model, lm, enc, 'device', kw=False, **o)
    assert path == 'device'
    for lm_arg, gam in ((lm, 0.0), (None, 0.3)):
        h1, aw1, s1, path = _decode(model, lm_arg, enc, 'device', **dict(o, gam=gam))
        assert path == 'device'
        assert s0 == s1
        for b in range(len(LENS)):
            np.testing.assert_array_equal(h0[b], h1[b])
            np.testing.assert_array_equal(aw0[b], aw1[b])


# ---------------------------------------------------- 4. both compute modes
def test_bf16_mode_equals_fp32_mode(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    kw_over, bias, lm_over, o = C.CASES['g03_lam03']
    model, lm = _pair(kw_over, bias, lm_over, C.SEEDS['g03_lam03'])
    enc = C.enc_out()
    native_ops.set_compute_dtype('fp32')
    h32, aw32, s32, _ = _decode(model, lm, enc, 'device', **o)
    native_ops.set_compute_dtype('bf16')
    try:
        h16, aw16, s16, path = _decode(model, lm, enc, 'device', **o)
    finally:
        native_ops.set_compute_dtype('fp32')
    assert path == 'device'
    assert s16 == s32
    for b in range(len(LENS)):
        np.testing.assert_array_equal(h16[b], h32[b])
        np.testing.assert_array_equal(aw16[b], aw32[b])


# ------------------------------------------------------------ 5. error_rate
def test_error_rate_with_lm(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    model, lm = _pair({}, {'eos': -1.5}, {}, 1623)
    rng = np.random.RandomState(5)
    B, T = 6, 30
    x_lens = np.array([30, 25, 21, 14, 9, 4])
    xs = rng.uniform(-1, 1, (B, T, 8)).astype(np.float32)
    y_lens = np.array([5, 4, 6, 3, 2, 1])
    ys = np.full((B, 6), -1, np.int64)
    for b in range(B):
        xs[b, x_lens[b]:] = 0
        ys[b, :y_lens[b]] = rng.randint(0, 6, y_lens[b])
    out = model.error_rate(xs, x_lens, ys, y_lens, 3, max_decode_len=6, rnnlm=lm, lm_weight=0.5)
    assert native_ops.last_att_beam_path() == 'device'
    old = os.environ.get('ASR_ATT_BEAM')
    os.environ['ASR_ATT_BEAM'] = 'host'
    try:
        hyps, _, perm = model.decode(xs, x_lens, 3, 6, rnnlm=lm, lm_weight=0.5)
    finally:
        if old is None:
            del os.environ['ASR_ATT_BEAM']
        else:
            os.environ['ASR_ATT_BEAM'] = old
    assert native_ops.last_att_beam_path() == 'host'
    hyps = [np.asarray(h) for h in hyps]
    want = edit_distance_ref.score(hyps, [len(h) for h in hyps], ys[perm], y_lens[perm],
                                   eos=model.eos_0)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert sum(len(h) for h in hyps) > 0


# --------------------------------------------------- 6. hierarchical, task 1
def test_hierarchical_sub_task(cuda_dev):
    import att_beam_lm_ref as R
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    native_ops.set_compute_dtype('fp32')
    kw = {k: v for k, v in C.BASE.items() if k != 'ctc_loss_weight'}
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
    # the LM's seed: the first from 1623 on with every restatement margin >= 2 GAP
    # (1.3e-2) on this model's sub-encoder output
    lm, lm_sd = C.lm_cpu(5, dict(num_layers=2), 1626)
    model.set_cuda()
    lm.set_cuda()
    rng = np.random.RandomState(11)
    x_lens = np.array([40, 33, 31, 27, 20, 16, 9, 5, 2, 1])
    B = len(x_lens)
    xs = rng.uniform(-1, 1, (B, 40, 8)).astype(np.float32)
    for b in range(B):
        xs[b, x_lens[b]:] = 0
    hyps, aw, perm = model.decode(xs, x_lens, 3, 5, length_penalty=0.3, task_index=1,
                                  ctc_weight=0.3, rnnlm=lm, lm_weight=0.5)
    assert native_ops.last_att_beam_path() == 'device'
    with torch.no_grad():
        _, _, enc_sub, _, _ = model._encode(model.np2var(xs, dtype='float'), x_lens,
                                            is_multi_task=True)
    lens_sub = model.encoder.last_lens_sub_np
    gaps = []
    ref_h, _, ref_aw = R.beam_decode_lm(sd, kw, enc_sub.float().cpu().numpy(), lens_sub, 3, 5,
                                        0, 0.3, torch.float64, gaps, ctc_weight=0.3, task=1,
                                        num_classes=5, num_units=9, lm_sd=lm_sd, lm_weight=0.5)
    left_out = [b for b, g in enumerate(gaps) if g < GAP]
    print('att_beam_lm hierarchical: left out %d of %d (smallest gap %.3e)'
          % (len(left_out), B, min(gaps)))
    assert len(left_out) * 10 <= B
    for b in range(B):
        if b in left_out:
            continue
        np.testing.assert_array_equal(np.asarray(hyps[b]), ref_h[b], err_msg='utterance %d' % b)
        np.testing.assert_allclose(aw[b], ref_aw[b], rtol=1e-3, atol=1e-5)


# ----------------------------------------------------------- 7. the refusals
def test_five_layer_and_gru_lm_run_the_host_path(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, _, o = C.CASES['g03']
    enc = C.enc_out()
    for lm_over, rnn_type in ((dict(num_layers=5), 'lstm'), ({}, 'gru')):
        model, lm = _pair(kw_over, bias, lm_over, C.SEEDS['g03'], rnn_type)
        dev_h, _, dev_s, path = _decode(model, lm, enc, 'device', **o)
        assert path == 'host'                         # ASR_ERR_UNSUPPORTED: the fall-back
        host_h, _, host_s, _ = _decode(model, lm, enc, 'host', **o)
        assert dev_s == host_s
        for a, b in zip(dev_h, host_h):
            np.testing.assert_array_equal(a, b)


def test_class_count_mismatch_is_an_argument_error(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    kw_over, bias, lm_over, o = C.CASES['g03']
    model, lm = _pair(kw_over, bias, lm_over, C.SEEDS['g03'])
    lm5, _ = C.lm_cpu(5, {}, 1)                      # 6 classes against the model's 7
    lm5.set_cuda()
    enc = torch.from_numpy(C.enc_out()).cuda()
    with pytest.raises(ValueError, match='num_classes'):
        model._decode_infer_beam(enc, np.array(LENS), 3, 4, 0, 0, 0, rnnlm=lm5, lm_weight=0.3)
    # below the model's check: the library's ASR_ERR_ARG, before any launch
    model._check_lm = lambda rnnlm, w, *a: w
    with pytest.raises(N.NativeError, match='classes'):
        model._decode_infer_beam_device(enc, np.array(LENS), 3, 4, 0, 0, rnnlm=lm5, lm_weight=0.3)
