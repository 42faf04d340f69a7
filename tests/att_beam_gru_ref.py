"""Restatement of AttentionSeq2seq._decode_infer_beam for a GRU decoder
(bahdanau order, one GRUCell layer, location or content attention) on CPU torch
in a chosen float dtype, from the encoder output on, with or without the joint
CTC/attention score.

Only the cell is stated here.  Everything after it -- attention, bottleneck,
log-softmax, top-k, the <eos> rule, the stable score sort, completion, the CTC
prefix scorer, the margins -- is att_beam_ctc_ref.beam_decode_joint as it is
(which takes att_beam_ref's attention step; its weight 0 is att_beam_ref's
search): that function steps its rows through ``asr_ref.lstm_cell(p, name, x, h,
c)``, and beam_decode below runs it with that one name bound to gru_cell for
the length of the call.  The c it carries stays zero and is never read.

The f32-against-f64 score error of this restatement sets the score bound of
tests/test_att_beam_gru_gpu.py."""
import contextlib

import numpy as np
import torch

import att_beam_ctc_ref
from oracle import asr_ref


def gru_cell(p, name, x, h):
    """nn.GRUCell, gate rows r, z, n (rnn_decoder.py:48,84-88 with rnn_type
    'gru'): r scales the hidden part of the n gate, its bias included."""
    gi = x @ p[name + '.weight_ih'].t() + p[name + '.bias_ih']
    gh = h @ p[name + '.weight_hh'].t() + p[name + '.bias_hh']
    D = h.shape[1]
    i_r, i_z, i_n = gi.split(D, dim=1)
    h_r, h_z, h_n = gh.split(D, dim=1)
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    return (1 - z) * n + z * h


def _as_lstm_cell(p, name, x, h, c):
    """gru_cell behind asr_ref.lstm_cell's signature: '<decoder>.lstm_l<k>' names
    the GRU layer '<decoder>.gru_l<k>'; c passes through."""
    return gru_cell(p, name.replace('.lstm_l', '.gru_l'), x, h), c


@contextlib.contextmanager
def _gru_for_lstm():
    old = asr_ref.lstm_cell
    asr_ref.lstm_cell = _as_lstm_cell
    try:
        yield
    finally:
        asr_ref.lstm_cell = old


def beam_decode(sd, cfg, enc_out, lens, beam_width, max_len, min_len=0, penalty=0,
                dtype=torch.float64, gaps=None, ctc_weight=0.0, dir='fwd', **sub_task):
    """(hyps, scores, aws) of att_beam_ctc_ref.beam_decode_joint for a model whose
    decoder is a GRU.  cfg['init_dec_state'] is the state the MODEL uses (it
    falls back to 'zero' when encoder and decoder types differ).  dir='bwd':
    the backward decoder's parameters (``*_bwd``), its hypotheses reversed as
    the model returns them; the attention weights stay in decoding order.
    sub_task: beam_decode_joint's task / num_classes / num_units."""
    if dir == 'bwd':
        sd = {(k.replace('_bwd', '_fwd') if '_bwd' in k else k): v for k, v in sd.items()
              if '_fwd' not in k}
    with _gru_for_lstm():
        hyps, scores, aws = att_beam_ctc_ref.beam_decode_joint(
            sd, cfg, enc_out, lens, beam_width, max_len, min_len, penalty, dtype, gaps,
            ctc_weight=ctc_weight, **sub_task)
    if dir == 'bwd':
        hyps = [np.ascontiguousarray(h[::-1]) for h in hyps]
    return hyps, scores, aws
