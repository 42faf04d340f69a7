#!/usr/bin/env python
"""Generate tests/golden/beam_att_gru.npz from the REFERENCE's AttentionSeq2seq
(see make_golden.py, whose shims this reuses): decode(beam_width=4) of the TIMIT
attention recipe's shape family -- GRU encoder, bridge layer, one-layer GRU
decoder, bahdanau order, one head of location attention, init_dec_state zero --
at test size, on a few short utterances.

Only numbers are written: the kwargs and decode options, the seed, the
reference's state_dict, the inputs, and the reference's hypotheses, lengths and
attention weights (beam_att.npz's keys).

The model is re-initialised uniform(+-0.6); the seed is the first of 1623, ...
whose reference output
  * has at least three distinct tokens and hypotheses of different lengths
    (min_decode_len 3: none shorter than two tokens, every utterance steps the
    cell), and
  * is what the float64 restatement (tests/att_beam_gru_ref.py) gives from the
    reference's own encoder output, with every decision margin >= 2e-3: no
    recorded utterance sits on a near-tie that f32 arithmetic on the device
    could flip.

Usage (from the repo root, in the build container):
    python tests/golden/make_golden_beam_gru.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repo root (oracle/)
import make_golden as mg  # noqa: E402

MARGIN = 2e-3
SCALE = 0.6


def main():
    import att_beam_gru_ref as R
    from models.pytorch_v3.attention.attention_seq2seq import AttentionSeq2seq
    kw = dict(input_size=8, encoder_type='gru', encoder_bidirectional=True,
              encoder_num_units=6, encoder_num_proj=0, encoder_num_layers=2,
              attention_type='location', attention_dim=7, decoder_type='gru',
              decoder_num_units=9, decoder_num_layers=1, embedding_dim=4,
              dropout_input=0, dropout_encoder=0, dropout_decoder=0, dropout_embedding=0,
              num_classes=6, parameter_init=0.1, subsample_list=[False, True],
              subsample_type='drop', bridge_layer=True, attention_conv_num_channels=3,
              attention_conv_width=5, bottleneck_dim=11, decoding_order='bahdanau',
              ctc_loss_weight=0, label_smoothing_prob=0, init_dec_state='zero')
    opts = dict(beam_width=4, max_decode_len=10, min_decode_len=3, length_penalty=0.1)
    rng0 = np.random.RandomState(6)
    B, T = 4, 22
    x_lens = np.array([22, 17, 20, 11], np.int32)
    xs = rng0.randn(B, T, 8).astype(np.float32)
    for b in range(B):
        xs[b, x_lens[b]:] = 0
    for seed in range(1623, 1623 + 500):
        torch.manual_seed(seed)
        model = AttentionSeq2seq(**kw)
        for p in model.parameters():
            torch.nn.init.uniform_(p, -SCALE, SCALE)
        with torch.no_grad():   # torch-0.3 volatile decoding (deepcopy of non-leaf states)
            hyps, aw, perm = model.decode(xs, x_lens, **opts)
        hl = np.array([len(h) for h in hyps], np.int32)
        toks = np.concatenate([np.asarray(h, np.int64) for h in hyps])
        if len(np.unique(toks)) < 3 or len(np.unique(hl)) < 2:
            continue
        assert hl.min() >= 2                 # min_decode_len
        with torch.no_grad():
            model.eval()
            enc, lens, _ = model._encode(model.np2var(xs), model.np2var(x_lens, dtype='int'))
        gaps = []
        r_h, _, r_aw = R.beam_decode(
            {k: v.detach() for k, v in model.state_dict().items()}, kw,
            enc.detach().double().numpy(), np.asarray(lens.detach()).reshape(-1),
            opts['beam_width'], opts['max_decode_len'], opts['min_decode_len'],
            opts['length_penalty'], torch.float64, gaps)
        same = all(np.array_equal(np.asarray(a, np.int64), b) for a, b in zip(hyps, r_h))
        if same and min(gaps) >= MARGIN:
            for a, b in zip(aw, r_aw):
                np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=1e-4, atol=1e-6)
            break
    else:
        raise RuntimeError('no seed found for beam_att_gru')
    print('seed %d: lengths %s, smallest margin %.3e' % (seed, hl.tolist(), min(gaps)))
    mg._save('beam_att_gru', kwargs=np.array(json.dumps(kw)), opts=np.array(json.dumps(opts)),
             seed=np.array([seed]), xs=xs, x_lens=x_lens, hyp_flat=toks, hyp_lens=hl,
             aw_flat=np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in aw]),
             perm=np.asarray(perm).astype(np.int64), **mg._sd(model))


if __name__ == '__main__':
    mg._install_shims()
    mg._install_beam_shims()
    main()
