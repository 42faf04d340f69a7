#!/usr/bin/env python
"""Golden vectors of the unidirectional-encoder models
(encoder_bidirectional=False), tests/golden/model_uni_*.npz, recorded from the
REFERENCE itself on the CPU with make_golden.py's shims.  Numbers only: the
inputs, the reference's constructed state_dict, the encoder's output lengths
and perm, the loss(es) and every gradient.  Sizes are those of the model_ctc_* /
model_hier / model_att fixtures.

Runs only where the reference is present (as make_golden.py):
    python tests/golden/make_golden_uni.py
"""
import json
import sys

import numpy as np
import torch

import make_golden as G

CTC_BASE = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=False,
                encoder_num_units=6, encoder_num_proj=0, encoder_num_layers=2, fc_list=[],
                dropout_input=0, dropout_encoder=0, num_classes=5, parameter_init=0.1,
                subsample_list=[], subsample_type='drop')
CTC_SPECS = [
    # rnn.py:162-198: one multi-layer nn.LSTM
    ('model_uni_ctc_fast', CTC_BASE),
    # rnn.py:200-251, :409-439: per-layer modules, 'drop' subsampling, projection
    ('model_uni_ctc_sub_proj', dict(CTC_BASE, encoder_num_layers=3, encoder_num_proj=4,
                                    subsample_list=[False, True, False])),
    # 'concat' subsampling and residual sums from the last subsampling layer on
    ('model_uni_ctc_concat_res', dict(CTC_BASE, encoder_num_layers=4,
                                      subsample_list=[True, False, False, False],
                                      subsample_type='concat', encoder_residual=True)),
]
HIER = dict(input_size=16, encoder_type='lstm', encoder_bidirectional=False, encoder_num_units=6,
            encoder_num_proj=0, encoder_num_layers=3, encoder_num_layers_sub=2, fc_list=[],
            fc_list_sub=[], dropout_input=0, dropout_encoder=0, main_loss_weight=0.5,
            sub_loss_weight=0.5, num_classes=9, num_classes_sub=5, parameter_init=0.1,
            subsample_list=[], subsample_type='drop')
ATT = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=False, encoder_num_units=6,
           encoder_num_proj=0, encoder_num_layers=2, attention_type='location', attention_dim=7,
           decoder_type='lstm', decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
           dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
           num_classes=5, parameter_init=0.1, subsample_list=[False, True],
           subsample_type='drop', attention_conv_num_channels=3, attention_conv_width=5,
           bottleneck_dim=11, decoding_order='bahdanau', init_dec_state='final',
           ctc_loss_weight=0.3, label_smoothing_prob=0)


def _enc_lens(model, xs, x_lens, multi=False):
    """The encoder's output lengths and perm (eval mode, no dropout anyway)."""
    model.eval()
    with torch.no_grad():
        out = model.encoder(torch.from_numpy(xs), torch.from_numpy(x_lens), volatile=True)
    arrays = dict(out_lens=np.asarray(out[1].numpy(), np.int32),
                  perm=np.asarray(out[-1].numpy(), np.int64),
                  enc_shape=np.array(out[0].shape, np.int64))
    if multi:
        arrays['out_lens_sub'] = np.asarray(out[3].numpy(), np.int32)
    return arrays


def case_ctc():
    from models.pytorch_v3.ctc.ctc import CTC
    for name, kw in CTC_SPECS:
        torch.manual_seed(1623)
        model = CTC(**kw)
        model.train()
        sd0 = G._sd(model)
        rng = np.random.RandomState(3)
        B, T = 4, 24
        x_lens = np.array([20, 24, 15, 11], np.int32)
        y_lens = np.array([5, 3, 4, 2], np.int32)
        xs, ys = G._batch(rng, B, T, 8, y_lens, 5, x_lens)
        loss = model(xs, ys, x_lens, y_lens)
        loss.backward()
        G._save(name, kwargs=np.array(json.dumps(kw)), xs=xs, ys=ys, x_lens=x_lens, y_lens=y_lens,
                loss=loss.detach().numpy().reshape(1), **_enc_lens(model, xs, x_lens), **sd0,
                **G._grads(model))


def case_hier():
    from models.pytorch_v3.ctc.hierarchical_ctc import HierarchicalCTC
    torch.manual_seed(1623)
    model = HierarchicalCTC(**HIER)
    model.train()
    sd0 = G._sd(model)
    rng = np.random.RandomState(6)
    B, T = 3, 26
    x_lens = np.array([26, 21, 13], np.int32)
    y_lens = np.array([2, 3, 1], np.int32)
    y_lens_sub = np.array([5, 4, 3], np.int32)
    xs, ys = G._batch(rng, B, T, 16, y_lens, 9, x_lens)
    ys_sub = np.full((B, 5), -1, np.int32)
    for b in range(B):
        ys_sub[b, :y_lens_sub[b]] = rng.randint(0, 5, y_lens_sub[b])
    loss, loss_main, loss_sub = model(xs, ys, x_lens, y_lens, ys_sub, y_lens_sub)
    loss.backward()
    G._save('model_uni_hier', kwargs=np.array(json.dumps(HIER)), xs=xs, ys=ys, x_lens=x_lens,
            y_lens=y_lens, ys_sub=ys_sub, y_lens_sub=y_lens_sub,
            loss=loss.detach().numpy().reshape(1),
            loss_main=loss_main.detach().numpy().reshape(1),
            loss_sub=loss_sub.detach().numpy().reshape(1),
            **_enc_lens(model, xs, x_lens, multi=True), **sd0, **G._grads(model))


def case_att():
    from models.pytorch_v3.attention.attention_seq2seq import AttentionSeq2seq
    torch.manual_seed(1623)
    model = AttentionSeq2seq(**ATT)
    model.train()
    sd0 = G._sd(model)
    rng = np.random.RandomState(4)
    B, T = 3, 22
    x_lens = np.array([22, 19, 14], np.int32)
    y_lens = np.array([4, 6, 3], np.int32)
    xs, ys = G._batch(rng, B, T, 8, y_lens, 5, x_lens)
    loss = model(xs, ys, x_lens, y_lens)
    loss.backward()
    G._save('model_uni_att', kwargs=np.array(json.dumps(ATT)), xs=xs, ys=ys, x_lens=x_lens,
            y_lens=y_lens, loss=loss.detach().numpy().reshape(1),
            **_enc_lens(model, xs, x_lens), **sd0, **G._grads(model))


if __name__ == '__main__':
    G._install_shims()
    case_ctc()
    case_hier()
    case_att()
    sys.exit(0)
