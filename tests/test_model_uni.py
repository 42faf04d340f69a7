"""The model classes with encoder_bidirectional=False vs the reference
(tests/golden/model_uni_*.npz, recorded by tests/golden/make_golden_uni.py).

CPU: construction under the reference's seed reproduces the reference's initial
state_dict bit for bit (the unidirectional modules' names, no _reverse tensors),
the flat buffer holds single-tensor groups, load_model gives the reference's
name, and a unidirectional GRU stays refused by name.  GPU, fp32 mode: loss and
every gradient within test_model_ctc.py's bounds (loss rtol 1e-4, gradients
rtol 1e-3 / atol 2e-5), the encoder's output lengths and perm, the eval loss,
one Adam step, CTC decoding with beam 1 and 4, attention beam search, and the
attention beam's device and host paths returning the same hypotheses."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_params

CTC_NAMES = ['model_uni_ctc_fast', 'model_uni_ctc_sub_proj', 'model_uni_ctc_concat_res']
NAMES = CTC_NAMES + ['model_uni_hier', 'model_uni_att']


def _cls(name):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.hierarchical_ctc import \
        HierarchicalCTC
    return {'model_uni_hier': HierarchicalCTC, 'model_uni_att': AttentionSeq2seq}.get(name, CTC)


def _build(name, kw):
    torch.manual_seed(1623)
    return _cls(name)(**kw)


def _load(name):
    d = golden(name)
    return d, json.loads(str(d['kwargs']))


@pytest.mark.parametrize('name', NAMES)
def test_init_matches_reference_state_dict(name):
    d, kw = _load(name)
    assert kw['encoder_bidirectional'] is False
    model = _build(name, kw)
    sd = model.state_dict()
    ref = {k[3:]: d[k] for k in d.files if k.startswith('sd/')}
    assert sorted(sd) == sorted(ref)
    assert not any('_reverse' in k for k in sd)
    for k, v in ref.items():
        np.testing.assert_array_equal(sd[k].numpy(), v, err_msg=k)
    enc = model.encoder
    assert enc.num_directions == 1 and model.encoder_num_units == kw['encoder_num_units']


@pytest.mark.parametrize('name', ['model_uni_ctc_fast', 'model_uni_ctc_sub_proj'])
def test_flat_order_yields_single_tensor_groups(name):
    d, kw = _load(name)
    model = _build(name, kw)
    enc = model.encoder
    groups = enc.flat_order()
    assert len(groups) == 4 * enc.num_layers and all(len(g) == 1 for g in groups)
    for l in range(enc.num_layers):
        (w_ih, w_hh, b_ih, b_hh), gs = enc._layer_tensors(l)
        H = enc.num_units
        assert w_ih.shape[0] == w_hh.shape[0] == b_ih.shape[0] == b_hh.shape[0] == 4 * H
        for t, g, (p,) in zip((w_ih, w_hh, b_ih, b_hh), gs, enc._layer_params(l)):
            assert t.data_ptr() == p.data_ptr() and g.data_ptr() == p.grad.data_ptr()
            assert tuple(t.shape) == tuple(p.shape) == tuple(g.shape)


def test_hierarchical_attention_builds_unidirectional():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.\
        hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    d = golden('model_hatt')
    kw = dict(json.loads(str(d['kwargs'])), encoder_bidirectional=False)
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    assert model.encoder.num_directions == 1
    assert not any('_reverse' in k for k in model.state_dict())


def test_unidirectional_gru_is_refused_by_name():
    d, kw = _load('model_uni_ctc_fast')
    with pytest.raises(NotImplementedError, match='unidirectional gru'):
        _build('model_uni_ctc_fast', dict(kw, encoder_type='gru'))


def _yml(name):
    import yaml
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name)
    return yaml.safe_load(open(path))['param']


def test_load_model_names_the_unidirectional_models():
    from pytorch_end2end_speech_recognition_amd.models.load_model import load
    params = _yml('char_blstm_ctc_100h.yml')
    params.update(num_classes=28, encoder_bidirectional=False)
    model = load('ctc', params, 'pytorch')
    # the reference's name: no leading 'b' (load_model.py:28-29)
    assert model.name == 'lstm320H4L_drop4_adam_lr1e-3_dropen0.2_input80'
    assert model.encoder.num_directions == 1
    assert model.fc_out.fc.weight.shape[1] == 320
    params = _yml('char_blstm_att_100h.yml')
    params.update(num_classes=28, encoder_bidirectional=False)
    bi = dict(params, encoder_bidirectional=True)
    uni, ref = load('attention', params, 'pytorch'), load('attention', bi, 'pytorch')
    assert ref.name.startswith('blstm') and uni.name == ref.name[1:]


# ---------------------------------------------------------------------- GPU
def _gpu_model(name):
    d, kw = _load(name)
    sd, g = golden_params(d)
    model = _build(name, kw)
    model.load_state_dict(sd)
    model.set_cuda()
    return d, kw, g, model


def _args(d):
    a = [d['xs'], d['ys'], d['x_lens'], d['y_lens']]
    if 'ys_sub' in d.files:
        a += [d['ys_sub'], d['y_lens_sub']]
    return a


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_model_matches_golden(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    d, kw, g, model = _gpu_model(name)
    model.zero_grad()
    out = model(*_args(d))
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss.item(), float(d['loss'][0]), rtol=1e-4)
    if isinstance(out, tuple):
        np.testing.assert_allclose(out[1].item(), float(d['loss_main'][0]), rtol=1e-4)
        np.testing.assert_allclose(out[2].item(), float(d['loss_sub'][0]), rtol=1e-4)
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[k], rtol=1e-3, atol=2e-5, err_msg=k)
    enc = model.encoder
    np.testing.assert_array_equal(enc.last_lens_np, d['out_lens'])
    np.testing.assert_array_equal(enc.last_perm_np, d['perm'])
    if 'out_lens_sub' in d.files:
        np.testing.assert_array_equal(enc.last_lens_sub_np, d['out_lens_sub'])
    ev = model(*_args(d), is_eval=True)
    ev = ev[0] if isinstance(ev, tuple) else ev
    assert isinstance(ev, float)
    np.testing.assert_allclose(ev, float(d['loss'][0]), rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_one_adam_step_runs(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    from pytorch_end2end_speech_recognition_amd.utils.training.training_loop import (
        train_hierarchical_step, train_step)
    native_ops.set_compute_dtype('fp32')
    d, kw, g, model = _gpu_model(name)
    model.set_optimizer('adam', 1e-3, weight_decay=1e-6, lr_schedule=False)
    before = model._flat_param.clone()
    batch = {k: d[k] for k in ('xs', 'ys', 'x_lens', 'y_lens', 'ys_sub', 'y_lens_sub')
             if k in d.files}
    step = train_hierarchical_step if 'ys_sub' in batch else train_step
    res = step(model, batch, 5.0)
    torch.cuda.synchronize()
    np.testing.assert_allclose(res[1], float(d['loss'][0]), rtol=1e-4)
    assert not torch.equal(before, res[0]._flat_param)
    assert bool(torch.isfinite(res[0]._flat_param).all())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['model_uni_ctc_fast', 'model_uni_ctc_sub_proj'])
def test_bf16_training_pass_with_dropout_is_finite_and_repeatable(name, cuda_dev):
    """bf16 mode with encoder dropout (between layers a plain pass, the last
    layer's folded into the head's product): finite, close to the golden loss
    of the dropout-free model only in scale, and the same bits under the same
    dropout seed."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    d, kw = _load(name)
    sd, _ = golden_params(d)
    model = _build(name, dict(kw, dropout_encoder=0.2, dropout_input=0.1))
    model.load_state_dict(sd)
    model.set_cuda()
    native_ops.set_compute_dtype('bf16')
    try:
        runs = []
        for _ in range(2):
            native_ops.manual_seed(77)
            model.zero_grad()
            loss = model(*_args(d))
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.item(), model._flat_grad.clone()))
    finally:
        native_ops.set_compute_dtype('fp32')
    assert np.isfinite(runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    assert runs[0][1].abs().max() > 0
    assert 0.5 < runs[0][0] / float(d['loss'][0]) < 2.0
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def _check_hyps(hyps, B, V):
    assert len(hyps) == B
    for h in hyps:
        h = np.asarray(h)
        assert h.ndim == 1 and (len(h) == 0 or (h.min() >= 0 and h.max() < V))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CTC_NAMES + ['model_uni_hier'])
def test_ctc_decoding_runs(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    d, kw, g, model = _gpu_model(name)
    B = len(d['xs'])
    for task, V in ((0, kw['num_classes']),) + (((1, kw['num_classes_sub']),)
                                                  if 'num_classes_sub' in kw else ()):
        for W in (1, 4):
            hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=W, task_index=task)
            assert aw is None
            np.testing.assert_array_equal(perm, d['perm'])
            _check_hyps(hyps, B, V)


def _att_beam(model, d, mode, monkeypatch):
    from pytorch_end2end_speech_recognition_amd import native_ops
    monkeypatch.setenv('ASR_ATT_BEAM', mode)
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=4, max_decode_len=8)
    return [np.asarray(h) for h in hyps], perm, native_ops.last_att_beam_path()


@pytest.mark.gpu
def test_attention_decoding_device_and_host_agree(cuda_dev, monkeypatch):
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('fp32')
    d, kw, g, model = _gpu_model('model_uni_att')
    B, V = len(d['xs']), kw['num_classes']
    for W in (1, 4):
        hyps, perm = model.decode_ctc(d['xs'], d['x_lens'], beam_width=W)
        np.testing.assert_array_equal(perm, d['perm'])
        _check_hyps(hyps, B, V)
    monkeypatch.delenv('ASR_ATT_BEAM', raising=False)
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=4, max_decode_len=8)
    np.testing.assert_array_equal(perm, d['perm'])
    _check_hyps(hyps, B, V + 1)       # <eos> may end a hypothesis
    assert native_ops.last_att_beam_path() == 'device'
    host, perm_h, path = _att_beam(model, d, 'host', monkeypatch)
    assert path == 'host'
    np.testing.assert_array_equal(perm_h, perm)
    assert len(host) == len(hyps)
    for a, b in zip(hyps, host):
        np.testing.assert_array_equal(np.asarray(a), b)
