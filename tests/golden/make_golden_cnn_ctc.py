#!/usr/bin/env python
"""Generate the pure-CNN CTC fixture tests/golden/model_cnn_ctc.npz from the
REFERENCE itself (see make_golden.py, whose shims this reuses): CTC with
encoder_type 'cnn' (ctc.py:197-222), a small net of the form of
examples/timit/s5/conf/ctc/cnn_ctc.yml.

  prelu/...   3 layers, kernels [3, 5], channels 16, 16, 32, pool [3, 1] after
              the first layer, PReLU, batch norm, fc_list [32]
  htanh/...   3 layers, kernels [3, 5], [5, 3], [3, 3], channels 16, a floor pool
              [2, 1] and a ceil pool [1, 2] (odd extent: a partial window),
              hard-tanh, no batch norm (conv biases), no fc layer

Each record: inputs, the state_dict as constructed, the encoder's output
lengths and time extent, the loss and every parameter gradient (PReLU slopes
included), and the batch-norm running statistics after the one training
forward.  Only numbers are written.

Usage (from the repo root, in the build container):
    python tests/golden/make_golden_cnn_ctc.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

BASE = dict(input_size=9, encoder_type='cnn', encoder_bidirectional=False, encoder_num_units=0,
            encoder_num_proj=0, encoder_num_layers=0, dropout_input=0, dropout_encoder=0,
            num_classes=5, parameter_init=0.1, subsample_list=[], subsample_type='drop',
            conv_strides=[[1, 1]] * 3)
SPECS = [
    ('prelu', dict(BASE, conv_channels=[16, 16, 32], conv_kernel_sizes=[[3, 5]] * 3,
                   poolings=[[3, 1], [], []], activation='prelu', batch_norm=True,
                   fc_list=[32])),
    # fc_list [16]: with no fc layer the reference sizes fc_out by encoder_num_units
    # (ctc.py:243), which a cnn encoder does not have
    ('htanh', dict(BASE, conv_channels=[16, 16, 16],
                   conv_kernel_sizes=[[3, 5], [5, 3], [3, 3]],
                   poolings=[[2, 1], [1, 2], []], activation='hard_tanh', batch_norm=False,
                   fc_list=[16])),
]


def main():
    from models.pytorch_v3.ctc.ctc import CTC
    out = {}
    for tag, kw in SPECS:
        torch.manual_seed(1623)
        model = CTC(**kw)
        model.train()
        sd0 = mg._sd(model, tag + '/sd/')
        rng = np.random.RandomState(11)
        B, T = 2, 19
        x_lens = np.array([19, 14], np.int32)
        y_lens = np.array([3, 2], np.int32)
        xs, ys = mg._batch(rng, B, T, 9, y_lens, 5, x_lens)
        loss = model(xs, ys, x_lens, y_lens)
        loss.backward()
        after = {tag + '/after/' + k: v.detach().numpy().copy()
                 for k, v in model.state_dict().items() if 'running' in k}
        model.eval()
        with torch.no_grad():
            enc_out, enc_lens = model.encoder(torch.from_numpy(xs), torch.from_numpy(x_lens))
        rec = dict(kwargs=np.array(json.dumps(kw)), xs=xs, ys=ys, x_lens=x_lens, y_lens=y_lens,
                   loss=loss.detach().numpy().reshape(1),
                   enc_lens=np.asarray(enc_lens.numpy()).astype(np.int32),
                   enc_T=np.int32(enc_out.shape[1]), enc_D=np.int32(enc_out.shape[2]))
        out.update({tag + '/' + k: v for k, v in rec.items()})
        out.update(sd0)
        out.update(after)
        out.update(mg._grads(model, tag + '/grad/'))
    out.update(recipe())
    mg._save('model_cnn_ctc', **out)


def recipe():
    """The shipped recipe itself: examples/timit/s5/conf/ctc/cnn_ctc.yml over its
    parent's values (num_classes as the TIMIT phone61 vocabulary gives it), the
    name the reference's load() builds for it and its parameter shapes."""
    import yaml
    from models.load_model import load
    conf = os.path.join(mg.REF, 'examples', 'timit', 's5', 'conf', 'ctc')
    with open(os.path.join(conf, 'cnn_ctc.yml')) as f:
        child = yaml.safe_load(f)
    with open(os.path.join(conf, os.path.basename(child['parent']))) as f:
        params = yaml.safe_load(f)['param']
    params.update(child['param'])
    params['num_classes'] = 61
    torch.manual_seed(1623)
    model = load(model_type='ctc', params=dict(params), backend='pytorch')
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    return {'recipe/params': np.array(json.dumps(params)), 'recipe/name': np.array(model.name),
            'recipe/shapes': np.array(json.dumps(shapes)),
            'recipe/output_size': np.int32(model.encoder.output_size)}


if __name__ == '__main__':
    mg._install_shims()
    main()
