"""The cases tests/test_att_beam_lm_gpu.py runs on the device and
tests/test_att_beam_lm_cpu.py qualifies without one: small random hybrid models,
a small random LSTM language model, and the restatement (tests/att_beam_lm_ref.py)
of each case, computed once per process and shared.

The model seeds are picked so that on the f64 restatement every decision margin
is >= 2 GAP and the f32 restatement returns the same hypotheses
(test_att_beam_lm_cpu.py asserts both)."""
import functools

import numpy as np
import torch

import att_beam_gru_ref
import att_beam_lm_ref as R

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
# the LM: H 9 is no multiple of the cell kernel's 4 waves, Y 5
LM = dict(embedding_dim=5, num_units=9, num_layers=1, tie_weights=False)

# name -> (model kwargs, output-bias additions {class: value} ('eos': the <eos> class),
#          LM kwargs, decode options (gam: lm_weight, lam: ctc_weight))
CASES = {
    'g03': ({}, {'eos': -1.5}, {}, dict(W=3, max_len=6, penalty=0.3, gam=0.3)),
    'g10_l2': ({}, {'eos': -1.5}, dict(num_layers=2), dict(W=3, max_len=6, penalty=0.3, gam=1.0)),
    'g03_lam03': ({}, {'eos': -1.5}, dict(num_layers=2),
                  dict(W=3, max_len=6, penalty=0.3, gam=0.3, lam=0.3)),
    'tied': ({}, {'eos': -1.5}, dict(embedding_dim=7, num_units=7, tie_weights=True),
             dict(W=3, max_len=6, penalty=0.3, gam=0.3, lam=0.3)),
    'w2': ({}, {'eos': -1.5}, {}, dict(W=2, max_len=8, penalty=0.3, gam=0.3)),
    'w32': (dict(num_classes=33), {'eos': -1.5}, {}, dict(W=32, max_len=2, penalty=0.3, gam=0.3)),
    'v3_w4': (dict(num_classes=2), {'eos': -1.5}, {}, dict(W=4, max_len=6, penalty=0.3, gam=0.3)),
    'v130': (dict(num_classes=129), {'eos': -1.5}, dict(num_layers=2),
             dict(W=3, max_len=3, penalty=0.3, gam=1.0, lam=0.3)),
    'min4_eos': ({}, {'eos': 3.0}, {}, dict(W=3, max_len=8, min_len=4, penalty=0.5, gam=0.3)),
    'eos_never': ({}, {'eos': -30.0}, {}, dict(W=3, max_len=5, gam=0.3)),   # none complete
    'eos_early': ({}, {'eos': 20.0}, {}, dict(W=3, max_len=8, gam=0.3)),    # W complete early
    'len1': ({}, {'eos': -1.5}, {}, dict(W=3, max_len=1, gam=0.3)),
    'gru': (dict(decoder_type='gru'), {'eos': -1.5}, {},
            dict(W=3, max_len=6, penalty=0.3, gam=0.3, lam=0.3)),
    'dec2': (dict(decoder_num_layers=2), {}, {}, dict(W=3, max_len=5, gam=0.3)),   # host path
}
SEEDS = {'g03': 1635, 'g10_l2': 1627, 'g03_lam03': 1625, 'tied': 1628, 'w2': 1624, 'w32': 1623,
         'v3_w4': 1623, 'v130': 1632, 'min4_eos': 1625, 'eos_never': 1627, 'eos_early': 1623,
         'len1': 1624, 'gru': 1627, 'dec2': 1627}
# a model and LM on which the restatement's gamma 0 and gamma 0.5 hypotheses differ (7 of 10
# utterances), both with every margin >= 2 * GAP
DIFF = ({}, {'eos': -1.5}, {}, dict(W=3, max_len=6, penalty=0.3), 1748)


def model_cpu(kw_over, bias, seed):
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


def lm_cpu(num_classes, lm_over, seed, rnn_type='lstm'):
    """A random LM over num_classes + 1 classes (the model's seed + 1000)."""
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.lm.rnnlm import RNNLM
    kw = dict(LM, **lm_over)
    torch.manual_seed(seed + 1000)
    lm = RNNLM(num_classes, rnn_type=rnn_type, bidirectional=False, dropout_embedding=0,
               dropout_hidden=0, dropout_output=0, **kw)
    with torch.no_grad():
        for p in lm.parameters():
            torch.nn.init.uniform_(p, -0.6, 0.6)
    return lm, {k: v.detach().clone() for k, v in lm.state_dict().items()}


def enc_out(seed=7):
    rng = np.random.RandomState(seed)
    enc = rng.uniform(-1, 1, (len(LENS), max(LENS), 12)).astype(np.float32)
    for b, L in enumerate(LENS):
        enc[b, L:] = 0
    return enc


def restate(kw_over, bias, lm_over, seed, o, dtype, gam=None):
    """(hyps, scores, aws, gaps) of the restatement."""
    _, kw, sd = model_cpu(kw_over, bias, seed)
    _, lm_sd = lm_cpu(kw['num_classes'], lm_over, seed)
    gaps = []
    gru = kw['decoder_type'] == 'gru'
    with (att_beam_gru_ref._gru_for_lstm() if gru else _null()):
        out = R.beam_decode_lm(sd, kw, enc_out(), LENS, o['W'], o['max_len'], o.get('min_len', 0),
                               o.get('penalty', 0), dtype, gaps, ctc_weight=o.get('lam', 0.0),
                               lm_sd=lm_sd, lm_weight=o['gam'] if gam is None else gam)
    return out + (gaps,)


class _null(object):
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@functools.lru_cache(maxsize=None)
def ref(name, f64=True):
    """The restatement of a case, computed once and shared."""
    kw_over, bias, lm_over, o = CASES[name]
    return restate(kw_over, bias, lm_over, SEEDS[name], o,
                   torch.float64 if f64 else torch.float32)


@functools.lru_cache(maxsize=None)
def score_bound():
    """16 x the largest |f32 mode - f64 mode| best score of the restatement over
    the cases, over utterances whose hypotheses agree in both modes."""
    worst = 0.0
    for name in CASES:
        a, r = ref(name, False), ref(name, True)
        for h32, h64, s32, s64 in zip(a[0], r[0], a[1], r[1]):
            if np.array_equal(h32, h64) and s64 > -1e9:
                worst = max(worst, abs(s32 - s64))
    print('att_beam_lm: restatement f32-vs-f64 score error %.3e, bound %.3e' % (worst, 16 * worst))
    return 16 * worst
