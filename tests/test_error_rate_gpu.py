"""error_rate() of the CTC and attention models through an ErrorRateMeter
against the restatement (edit_distance_ref.py) applied to decode()'s host
output and the permuted ys; compute_wer / compute_cer / compute_per of
utils/evaluation/edit_distance.py against the reference's recorded results.
"""
import numpy as np
import pytest
import torch

import edit_distance_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu

B, T = 6, 40
X_LENS = np.array([33, 40, 9, 40, 21, 1], np.int32)     # not sorted: perm_idx matters
Y_LENS = np.array([5, 7, 2, 6, 4, 1], np.int32)


def _batch(V):
    rng = np.random.RandomState(3)
    xs = rng.randn(B, T, 8).astype(np.float32)
    ys = np.full((B, int(Y_LENS.max())), -1, np.int32)
    for b in range(B):
        xs[b, X_LENS[b]:] = 0
        ys[b, :Y_LENS[b]] = rng.randint(0, V, Y_LENS[b])
    return xs, ys


def _spread(model, seed):
    """Weights wide enough that the untrained model emits more than blanks /
    one class."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty(p.shape).uniform_(-0.6, 0.6, generator=g))


@pytest.fixture(scope='module')
def ctc_model(cuda_dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    torch.manual_seed(1623)
    model = CTC(input_size=8, encoder_type='lstm', encoder_bidirectional=True,
                encoder_num_units=16, encoder_num_proj=0, encoder_num_layers=2, fc_list=[],
                dropout_input=0, dropout_encoder=0, num_classes=6, parameter_init=0.1,
                subsample_list=[], subsample_type='drop')
    _spread(model, 11)
    model.set_cuda()
    return model


def _att(decoder_num_layers):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    torch.manual_seed(1623)
    model = AttentionSeq2seq(
        input_size=8, encoder_type='lstm', encoder_bidirectional=True, encoder_num_units=16,
        encoder_num_proj=0, encoder_num_layers=1, attention_type='location', attention_dim=7,
        decoder_type='lstm', decoder_num_units=9, decoder_num_layers=decoder_num_layers,
        embedding_dim=4, dropout_input=0, dropout_encoder=0, dropout_decoder=0,
        dropout_embedding=0, num_classes=6, parameter_init=0.1, subsample_list=[False],
        subsample_type='drop', attention_conv_num_channels=3, attention_conv_width=5,
        bottleneck_dim=11, decoding_order='bahdanau', ctc_loss_weight=0, label_smoothing_prob=0,
        init_dec_state='zero')
    _spread(model, 12)
    model.set_cuda()
    return model


@pytest.fixture(scope='module')
def att_model(cuda_dev):
    return _att(1)


@pytest.fixture(scope='module')
def att_model_steps(cuda_dev):
    """A 2-layer decoder: the step-by-step greedy and the host beam paths,
    whose hypotheses are host arrays and are uploaded."""
    return _att(2)


def _meter(**kw):
    from pytorch_end2end_speech_recognition_amd.utils.evaluation.edit_distance import \
        ErrorRateMeter
    return ErrorRateMeter('token', **kw)


def _check(model, beam_width, max_decode_len, eos):
    from pytorch_end2end_speech_recognition_amd import native_ops
    xs, ys = _batch(6)
    meter = _meter(eos=eos)
    want_total = np.zeros(5, np.int64)
    n_tokens = 0
    for _ in range(2):                                   # the meter keeps a running total
        out = model.error_rate(xs, X_LENS, ys, Y_LENS, beam_width,
                               max_decode_len=max_decode_len, meter=meter)
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (B, 5)
        assert native_ops.last_edit_distance_path() == 'device'
        hyps, _, perm = model.decode(xs, X_LENS, beam_width, max_decode_len)
        hyps = [np.asarray(h) for h in hyps]
        want = R.score(hyps, [len(h) for h in hyps], ys[perm], Y_LENS[perm], eos=eos)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        want_total += want.sum(axis=0)
        n_tokens += sum(len(R.clean(h, is_hyp=True, eos=eos)) for h in hyps)
    assert n_tokens > 0                                  # not a comparison of empty rows
    res = meter.result()
    assert [res[k] for k in ('distance', 'sub', 'ins', 'dele', 'ref_units')] == list(want_total)
    assert res['utterances'] == 2 * B and res['ref_units'] == 2 * int(Y_LENS.sum())
    assert res['rate'] == res['distance'] / res['ref_units']


@pytest.mark.parametrize('beam_width', [1, 4])
def test_ctc_error_rate(ctc_model, beam_width):
    _check(ctc_model, beam_width, None, None)


@pytest.mark.parametrize('beam_width', [1, 4])
def test_attention_error_rate(att_model, beam_width):
    _check(att_model, beam_width, 8, att_model.eos_0)


@pytest.mark.parametrize('beam_width', [1, 4])
def test_attention_error_rate_host_decode_paths(att_model_steps, beam_width):
    _check(att_model_steps, beam_width, 6, att_model_steps.eos_0)


def test_decode_unchanged_by_error_rate(att_model):
    """error_rate() leaves no capture behind: decode() returns host arrays."""
    xs, ys = _batch(6)
    att_model.error_rate(xs, X_LENS, ys, Y_LENS, 4, max_decode_len=8)
    hyps, aw, perm = att_model.decode(xs, X_LENS, 4, 8)
    assert hyps is not None and aw is not None and len(hyps) == B


def test_compute_wer_equals_reference(cuda_dev):
    from pytorch_end2end_speech_recognition_amd.utils.evaluation import edit_distance as E
    fx = golden('edit_distance')
    words = ['w%d' % k for k in range(30)]               # any hashable items
    for k in range(0, len(fx['result']), 3):
        ref = [words[t] for t in fx['ref'][k, :fx['ref_lens'][k]]]
        hyp = [words[t] for t in fx['hyp'][k, :fx['hyp_lens'][k]]]
        assert E.compute_wer(ref, hyp) == tuple(fx['result'][k])
    ref, hyp = ['a', 'b', 'c', 'd'], ['a', 'x', 'd']
    wer, sub, ins, dele = E.compute_wer(ref, hyp, normalize=True)
    assert (wer, sub, ins, dele) == (0.5, 1, 0, 1)
    assert E.compute_cer('kitten', 'sitting') == 3
    assert E.compute_cer('kitten', 'sitting', normalize=True) == 0.5
    assert E.compute_per(['k', 'ih', 't'], ['k', 't'], normalize=True) == 1 / 3
    assert E.compute_wer(['a'], []) == (1, 0, 0, 1)      # the reference raises here
