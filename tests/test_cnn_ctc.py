"""The pure-CNN CTC model (CTC with encoder_type 'cnn', ctc.py:197-222; the
recipe examples/timit/s5/conf/ctc/cnn_ctc.yml) vs golden vectors recorded from
the reference (tests/golden/make_golden_cnn_ctc.py): a small net of the
recipe's form with PReLU and batch norm ('prelu') and a hard-tanh net with 5-tap
frequency kernels, a floor and a ceil pool and conv biases ('htanh').

CPU: load('ctc', ...) with the recipe's own values builds and carries the
reference's model.name and parameter shapes; the small nets' initial
state_dict is bit-identical under the reference's seed; x_lens equal the
golden; maxout raises.  GPU: loss, every gradient (PReLU slopes included) and
the batch-norm running statistics in fp32 mode against the golden; bf16 mode
against the fp32-mode result of the same model; one train_step moves every
parameter."""
import json

import numpy as np
import pytest
import torch

from conftest import golden

TAGS = ['prelu', 'htanh']


def _rec(tag):
    d = golden('model_cnn_ctc')
    pre = tag + '/'
    return {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}


def _build(kw):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    torch.manual_seed(1623)
    return CTC(**kw)


def test_recipe_loads_with_reference_name():
    from pytorch_end2end_speech_recognition_amd.models.load_model import load
    r = _rec('recipe')
    params = json.loads(str(r['params']))
    assert params['encoder_type'] == 'cnn' and params['activation'] == 'prelu'
    model = load(model_type='ctc', params=dict(params), backend='pytorch')
    assert model.name == str(r['name'])
    assert model.encoder.output_size == int(r['output_size'])
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert shapes == json.loads(str(r['shapes']))


@pytest.mark.parametrize('tag', TAGS)
def test_cnn_ctc_init_matches_reference_state_dict(tag):
    r = _rec(tag)
    model = _build(json.loads(str(r['kwargs'])))
    sd = model.state_dict()
    ref = {k[3:]: v for k, v in r.items() if k.startswith('sd/')}
    assert sorted(sd) == sorted(ref)
    for k, v in ref.items():
        np.testing.assert_array_equal(sd[k].numpy(), v, err_msg=k)


@pytest.mark.parametrize('tag', TAGS)
def test_cnn_ctc_x_lens_match_reference(tag):
    """ConvOutSize (cnn_utils.py:25-39) over 5-tap layers: 2 frames fewer per layer."""
    r = _rec(tag)
    model = _build(json.loads(str(r['kwargs'])))
    lens = [model.encoder.conv_out_len(int(x), 1) for x in r['x_lens']]
    np.testing.assert_array_equal(lens, r['enc_lens'])
    assert model.encoder.output_size == int(r['enc_D'])


def test_maxout_raises_as_the_reference_cannot_run_it():
    kw = json.loads(str(_rec('prelu')['kwargs']))
    with pytest.raises(NotImplementedError, match='maxout.*reference cannot run it'):
        _build(dict(kw, activation='maxout'))


@pytest.mark.parametrize('bad', [dict(conv_kernel_sizes=[[3, 7]] * 3),
                                 dict(conv_strides=[[1, 2]] * 3), dict(activation='tanh')])
def test_out_of_scope_layers_keep_raising(bad):
    kw = json.loads(str(_rec('prelu')['kwargs']))
    with pytest.raises(NotImplementedError, match='MI355X CNNEncoder: not yet supported'):
        _build(dict(kw, **bad))


def _step(model, r):
    model.zero_grad()
    loss = model(r['xs'], r['ys'], r['x_lens'], r['y_lens'])
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.detach().cpu().numpy().copy()
                         for k, p in model.named_parameters()}


def _loaded(r):
    model = _build(json.loads(str(r['kwargs'])))
    model.load_state_dict({k[3:]: torch.from_numpy(v.copy()) for k, v in r.items()
                           if k.startswith('sd/')})
    model.set_cuda()
    return model


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_cnn_ctc_fp32_matches_golden(tag, cuda_dev):
    """Tolerances of tests/test_vgg.py:90-92 (loss rtol 1e-4; gradients rtol 2e-3,
    atol 2e-5) and :96 for the running statistics."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    r = _rec(tag)
    model = _loaded(r)
    loss, grads = _step(model, r)
    np.testing.assert_allclose(loss, float(r['loss'][0]), rtol=1e-4)
    assert any('layers.1.weight' in k for k in grads) == (tag == 'prelu')   # the PReLU slope
    for k, g in grads.items():
        np.testing.assert_allclose(g, r['grad/' + k], rtol=2e-3, atol=2e-5, err_msg=k)
    after = model.state_dict()
    for k in r:
        if k.startswith('after/'):
            np.testing.assert_allclose(after[k[6:]].cpu().numpy(), r[k], rtol=1e-4, atol=1e-6,
                                       err_msg=k)
    np.testing.assert_array_equal(model.encoder.last_lens_np, r['enc_lens'])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_cnn_ctc_bf16_vs_fp32_mode(tag, cuda_dev):
    """bf16 mode against the fp32-mode result of the same model, with the
    tolerance test_vgg_bf16_fast_path_vs_oracle applies to the VGG front-end's
    parameters (tests/test_vgg.py:142-154): loss within 2e-2 relative; per
    encoder tensor max |diff| < 0.25 max |g|, relative Frobenius error < 0.3 and
    cosine > 0.97.  (A PReLU slope is a single number: the max-|diff| check is
    the one that applies to it.)"""
    from pytorch_end2end_speech_recognition_amd import native_ops
    r = _rec(tag)
    native_ops.set_compute_dtype('fp32')
    ref_loss, ref = _step(_loaded(r), r)
    native_ops.set_compute_dtype('bf16')
    try:
        loss, grads = _step(_loaded(r), r)
    finally:
        native_ops.set_compute_dtype('fp32')
    assert abs(loss - ref_loss) / abs(ref_loss) < 2e-2
    for k, gw in grads.items():
        if not k.startswith('encoder.'):
            continue
        ga = ref[k]
        scale = np.abs(ga).max() + 1e-6
        print('  %-32s max diff / scale %.4f' % (k, np.abs(gw - ga).max() / scale))
        assert np.abs(gw - ga).max() / scale < 0.25, (k, np.abs(gw - ga).max(), scale)
        if ga.size == 1:
            continue
        fro = np.linalg.norm(gw - ga) / (np.linalg.norm(ga) + 1e-12)
        cos = float((gw * ga).sum() / (np.linalg.norm(gw) * np.linalg.norm(ga) + 1e-30))
        assert fro < 0.3 and cos > 0.97, (k, fro, cos)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_cnn_ctc_train_step_moves_every_parameter(mode, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.utils.training.training_loop import train_step
    r = _rec('prelu')
    native_ops.set_compute_dtype(mode)
    try:
        model = _loaded(r)
        model.set_optimizer('adam', 1e-3, weight_decay=1e-6, lr_schedule=False)
        before = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        model, lv = train_step(model, dict(xs=r['xs'], ys=r['ys'], x_lens=r['x_lens'],
                                           y_lens=r['y_lens']), 5.0)
        torch.cuda.synchronize()
    finally:
        native_ops.set_compute_dtype('fp32')
    assert np.isfinite(lv)
    same = [k for k, p in model.named_parameters() if torch.equal(p.detach().cpu(), before[k])]
    assert not same, same
    assert sum('encoder.layers' in k and before[k].numel() == 1 for k in before) == 3   # slopes
