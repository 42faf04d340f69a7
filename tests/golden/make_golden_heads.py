#!/usr/bin/env python
"""Generate the multi-head / dot-product attention fixtures under tests/golden/
from the REFERENCE itself (see make_golden.py, whose shims this reuses):

  att_step_heads.npz   AttentionMechanism.forward + backward for location H = 2
                       ('loc2/...') and dot_product H = 2 ('dot2/...')
  model_att_mha.npz, model_att_dot.npz, model_att_dot_mha.npz
                       AttentionSeq2seq at model_att_content's sizes: loss and
                       every gradient of the seed-1623 model, plus greedy and
                       beam-2 decodes of the same model re-initialised
                       uniform(+-0.8) under a recorded seed ('dec_sd/...')
  model_hatt_mha.npz   HierarchicalAttentionSeq2seq, num_heads 2, num_heads_sub 2

Only numbers are written: inputs, the reference's state_dict, outputs, gradients.

Usage (from the repo root, in the build container):
    python tests/golden/make_golden_heads.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

DEC_SCALE = 0.8
DEC_MAX_LEN = 8


def case_step_heads():
    from models.pytorch_v3.attention.attention_layer import AttentionMechanism
    out = {}
    for tag, kw in (
            ('loc2', dict(encoder_num_units=12, decoder_num_units=10, attention_type='location',
                          attention_dim=8, sharpening_factor=2.0, sigmoid_smoothing=False,
                          out_channels=3, kernel_size=7, num_heads=2)),
            ('dot2', dict(encoder_num_units=12, decoder_num_units=10,
                          attention_type='dot_product', attention_dim=8, sharpening_factor=1.0,
                          sigmoid_smoothing=False, out_channels=3, kernel_size=7, num_heads=2))):
        torch.manual_seed(1623)
        att = AttentionMechanism(**kw)
        sd0 = mg._sd(att, tag + '/sd0/')        # as constructed: RNG-order parity
        for p in att.parameters():
            torch.nn.init.uniform_(p, -0.3, 0.3)
        rng = np.random.RandomState(2)
        B, T, H = 3, 15, 2
        A = 10 if kw['attention_type'] == 'dot_product' else 8
        x_lens = np.array([15, 11, 15], np.int32)
        enc_out = torch.from_numpy(rng.randn(B, T, 12).astype(np.float32)).requires_grad_(True)
        enc_out_a = torch.from_numpy(rng.randn(B, T, A, H).astype(np.float32)).requires_grad_(True)
        dec_out = torch.from_numpy(rng.randn(B, 1, 10).astype(np.float32)).requires_grad_(True)
        aw = np.abs(rng.rand(B, T, H)).astype(np.float32)
        aw /= aw.sum(1, keepdims=True)
        aw_t = torch.from_numpy(aw).requires_grad_(True)
        ctx, aw_out = att(enc_out, enc_out_a, torch.from_numpy(x_lens), dec_out, aw_t)
        Rc = torch.from_numpy(rng.randn(*ctx.shape).astype(np.float32))
        Ra = torch.from_numpy(rng.randn(*aw_out.shape).astype(np.float32))
        ((ctx * Rc).sum() + (aw_out * Ra).sum()).backward()
        rec = dict(kwargs=np.array(json.dumps(kw)), x_lens=x_lens,
                   enc_out=enc_out.detach().numpy(), enc_out_a=enc_out_a.detach().numpy(),
                   dec_out=dec_out.detach().numpy(), aw_in=aw, ctx=ctx.detach().numpy(),
                   aw_out=aw_out.detach().numpy(), Rc=Rc.numpy(), Ra=Ra.numpy(),
                   d_enc_out=enc_out.grad.numpy(), d_enc_out_a=enc_out_a.grad.numpy(),
                   d_dec_out=dec_out.grad.numpy(),
                   d_aw_in=(np.zeros_like(aw) if aw_t.grad is None else aw_t.grad.numpy()))
        out.update({tag + '/' + k: v for k, v in rec.items()})
        out.update(sd0)
        out.update(mg._sd(att, tag + '/sd/'))
        out.update(mg._grads(att, tag + '/grad/'))
    mg._save('att_step_heads', **out)


def _decode_record(build, decode):
    """Greedy and beam-2 decodes of a uniform(+-DEC_SCALE) model: the first
    seed of 1623, ... whose greedy output has at least three distinct tokens."""
    for seed in range(1623, 1623 + 500):
        torch.manual_seed(seed)
        model = build()
        for p in model.parameters():
            torch.nn.init.uniform_(p, -DEC_SCALE, DEC_SCALE)
        with torch.no_grad():
            hyps, _, perm = decode(model, 1)
        hyps = np.asarray(hyps)
        if len(np.unique(hyps)) >= 3:
            break
    else:
        raise RuntimeError('no decode seed found')
    with torch.no_grad():
        beam, _, perm2 = decode(model, 2)
    hl = np.array([len(h) for h in beam], np.int32)
    toks = np.concatenate([np.asarray(h, np.int64).reshape(-1) for h in beam])
    rec = dict(dec_seed=np.array([seed]), dec_max_len=np.array([DEC_MAX_LEN]),
               greedy=hyps.astype(np.int64), greedy_perm=np.asarray(perm).astype(np.int64),
               beam_flat=toks, beam_lens=hl, beam_perm=np.asarray(perm2).astype(np.int64))
    rec.update(mg._sd(model, 'dec_sd/'))
    return rec


def case_models():
    from models.pytorch_v3.attention.attention_seq2seq import AttentionSeq2seq
    base = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True,
                encoder_num_units=6, encoder_num_proj=0, encoder_num_layers=2,
                attention_type='location', attention_dim=7, decoder_type='lstm',
                decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
                dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
                num_classes=5, parameter_init=0.1, subsample_list=[False, True],
                subsample_type='drop', attention_conv_num_channels=3,
                attention_conv_width=5, bottleneck_dim=11, decoding_order='bahdanau',
                init_dec_state='zero')
    specs = [('model_att_mha', dict(base, num_heads=2)),
             ('model_att_dot', dict(base, attention_type='dot_product')),
             ('model_att_dot_mha', dict(base, attention_type='dot_product', num_heads=2))]
    for name, kw in specs:
        torch.manual_seed(1623)
        model = AttentionSeq2seq(**kw)
        model.train()
        rng = np.random.RandomState(4)
        B, T = 3, 22
        x_lens = np.array([22, 19, 14], np.int32)
        y_lens = np.array([4, 6, 3], np.int32)
        xs, ys = mg._batch(rng, B, T, 8, y_lens, 5, x_lens)
        loss = model(xs, ys, x_lens, y_lens)
        loss.backward()
        rec = _decode_record(
            lambda: AttentionSeq2seq(**kw),
            lambda m, bw: m.decode(xs, x_lens, beam_width=bw, max_decode_len=DEC_MAX_LEN))
        mg._save(name, kwargs=np.array(json.dumps(kw)), xs=xs, ys=ys, x_lens=x_lens,
                 y_lens=y_lens, loss=loss.detach().numpy().reshape(1), **mg._sd(model),
                 **mg._grads(model), **rec)


def case_hier():
    from models.pytorch_v3.attention.hierarchical_attention_seq2seq import \
        HierarchicalAttentionSeq2seq
    kw = dict(input_size=8, encoder_type='lstm', encoder_bidirectional=True,
              encoder_num_units=6, encoder_num_proj=0, encoder_num_layers=3,
              encoder_num_layers_sub=2, attention_type='location', attention_dim=7,
              decoder_type='lstm', decoder_num_units=9, decoder_num_units_sub=7,
              decoder_num_layers=1, decoder_num_layers_sub=1, embedding_dim=4,
              embedding_dim_sub=3, dropout_input=0, dropout_encoder=0, dropout_decoder=0,
              dropout_embedding=0, num_classes=5, num_classes_sub=4, parameter_init=0.1,
              subsample_list=[False, True, False], subsample_type='drop',
              attention_conv_num_channels=3, attention_conv_width=5, bottleneck_dim=11,
              bottleneck_dim_sub=8, decoding_order='bahdanau', init_dec_state='zero',
              main_loss_weight=0.5, sub_loss_weight=0.5, ctc_loss_weight_sub=0, num_heads=2,
              num_heads_sub=2)
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    model.train()
    rng = np.random.RandomState(8)
    B, T = 3, 22
    x_lens = np.array([22, 19, 14], np.int32)
    y_lens = np.array([3, 4, 2], np.int32)
    y_lens_sub = np.array([6, 7, 4], np.int32)
    xs, ys = mg._batch(rng, B, T, 8, y_lens, 5, x_lens)
    ys_sub = np.full((B, int(y_lens_sub.max())), -1, np.int32)
    for b in range(B):
        ys_sub[b, :y_lens_sub[b]] = rng.randint(0, 4, y_lens_sub[b])
    loss, loss_main, loss_sub = model(xs, ys, x_lens, y_lens, ys_sub, y_lens_sub)
    loss.backward()
    rec = _decode_record(
        lambda: HierarchicalAttentionSeq2seq(**kw),
        lambda m, bw: m.decode(xs, x_lens, beam_width=bw, max_decode_len=DEC_MAX_LEN))
    mg._save('model_hatt_mha', kwargs=np.array(json.dumps(kw)), xs=xs, ys=ys, x_lens=x_lens,
             y_lens=y_lens, ys_sub=ys_sub, y_lens_sub=y_lens_sub,
             loss=loss.detach().numpy().reshape(1),
             loss_main=loss_main.detach().numpy().reshape(1),
             loss_sub=loss_sub.detach().numpy().reshape(1), **mg._sd(model), **mg._grads(model),
             **rec)


if __name__ == '__main__':
    mg._install_shims()
    mg._install_beam_shims()
    case_step_heads()
    case_models()
    case_hier()
