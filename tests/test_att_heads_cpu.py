"""Multi-head and dot-product attention without a GPU: the reference module
tests/att_heads_ref.py against fixtures recorded from the reference project
(tests/golden/make_golden_heads.py), its gradients against finite differences,
and the model classes' construction: the same state_dict keys, shapes and
values as the reference under the same seed (registration / RNG order), and
the loader's naming."""
import json

import numpy as np
import pytest
import torch

import att_heads_ref as H
from conftest import golden

MODEL_FIXTURES = ['model_att_mha', 'model_att_dot', 'model_att_dot_mha']


def _ref_heads(d, tag, kind, nh, dtype):
    sd = {k[len(tag) + 4:]: torch.from_numpy(d[k].copy()).to(dtype)
          for k in d.files if k.startswith(tag + '/sd/')}
    heads = []
    for h in range(nh):
        hd = {}
        if kind != 'dot_product':
            hd = dict(w_dec=sd['W_dec_head%d.fc.weight' % h], v=sd['V_head%d.fc.weight' % h])
            if kind == 'location':
                hd.update(w_conv=sd['W_conv_head%d.fc.weight' % h],
                          conv_w=sd['conv_head%d.weight' % h])
        heads.append({k: v.requires_grad_(True) for k, v in hd.items()})
    return sd, heads


@pytest.mark.parametrize('tag', ['loc2', 'dot2'])
def test_reference_module_matches_reference_project(tag):
    """heads_step + W_mha in float64 against the reference project's
    AttentionMechanism.forward / backward (float32 record)."""
    d = golden('att_step_heads')
    kw = json.loads(str(d[tag + '/kwargs']))
    kind, nh = kw['attention_type'], kw['num_heads']
    dt = torch.float64
    sd, heads = _ref_heads(d, tag, kind, nh, dt)
    t = {k: torch.from_numpy(d[tag + '/' + k].copy()).to(dt).requires_grad_(True)
         for k in ('enc_out', 'enc_out_a', 'dec_out', 'aw_in')}
    w_mha = sd['W_mha.fc.weight'].requires_grad_(True)
    b_mha = sd['W_mha.fc.bias'].requires_grad_(True)
    mask = H.frame_mask(d[tag + '/x_lens'], t['enc_out'].shape[1], dt)
    ctx, aw = H.heads_step(t['enc_out'], t['enc_out_a'], mask, t['dec_out'][:, 0], t['aw_in'],
                           heads, kind, kw['sharpening_factor'], kw['sigmoid_smoothing'])
    ctx = (ctx @ w_mha.t() + b_mha).unsqueeze(1)
    np.testing.assert_allclose(ctx.detach().numpy(), d[tag + '/ctx'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(aw.detach().numpy(), d[tag + '/aw_out'], rtol=1e-4, atol=1e-7)
    Rc, Ra = (torch.from_numpy(d[tag + '/' + k]).to(dt) for k in ('Rc', 'Ra'))
    ((ctx * Rc).sum() + (aw * Ra).sum()).backward()
    for k in ('enc_out', 'enc_out_a', 'dec_out'):
        np.testing.assert_allclose(t[k].grad.numpy(), d[tag + '/d_' + k], rtol=1e-3, atol=1e-5,
                                   err_msg=k)
    d_aw = np.zeros_like(d[tag + '/aw_in']) if t['aw_in'].grad is None else t['aw_in'].grad.numpy()
    np.testing.assert_allclose(d_aw, d[tag + '/d_aw_in'], rtol=1e-3, atol=1e-5)
    got = {'W_mha.fc.weight': w_mha.grad, 'W_mha.fc.bias': b_mha.grad}
    for h, hd in enumerate(heads):
        for k, name in (('w_dec', 'W_dec_head%d.fc.weight'), ('v', 'V_head%d.fc.weight'),
                        ('w_conv', 'W_conv_head%d.fc.weight'), ('conv_w', 'conv_head%d.weight')):
            if k in hd:
                got[name % h] = hd[k].grad
    for k, g in got.items():
        np.testing.assert_allclose(g.numpy(), d[tag + '/grad/' + k], rtol=1e-3, atol=1e-5,
                                   err_msg=k)


@pytest.mark.parametrize('case', ['loc2_sig', 'dot3_sig'])
def test_reference_gradcheck(case):
    p = H.dims_of(case)
    inp = H.case_inputs(case)
    mk = lambda x: x.detach().double().clone().requires_grad_(True)   # noqa: E731
    acts = [mk(inp[k]) for k in H.ACT_KEYS]
    wkeys = H.WEIGHT_KEYS[p['kind']]
    flat = [mk(hd[k]) for hd in inp['heads'] for k in wkeys]
    mask = H.frame_mask(inp['lens'], p['T'], torch.float64)

    def fn(enc, enc_a, dec, awp, *ws):
        heads = [dict(zip(wkeys, ws[len(wkeys) * h:len(wkeys) * (h + 1)])) for h in range(p['H'])]
        return H.heads_step(enc, enc_a, mask, dec, awp, heads, p['kind'], p['sharpen'],
                            p['sigmoid'])
    assert torch.autograd.gradcheck(fn, acts + flat, eps=1e-6, atol=1e-6, rtol=1e-4)


def _assert_state_dict(sd, ref):
    assert sorted(sd) == sorted(ref)
    assert list(sd) == [k for k in sd if k in ref]
    for k, v in ref.items():
        assert tuple(sd[k].shape) == v.shape, k
        np.testing.assert_array_equal(sd[k].numpy(), v, err_msg=k)


@pytest.mark.parametrize('tag', ['loc2', 'dot2'])
def test_attention_mechanism_init_matches_reference(tag):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_layer \
        import AttentionMechanism
    d = golden('att_step_heads')
    kw = json.loads(str(d[tag + '/kwargs']))
    torch.manual_seed(1623)
    att = AttentionMechanism(**kw)
    pre = tag + '/sd0/'
    _assert_state_dict(att.state_dict(), {k[len(pre):]: d[k] for k in d.files
                                          if k.startswith(pre)})


@pytest.mark.parametrize('name', MODEL_FIXTURES)
def test_model_init_matches_reference_state_dict(name):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    d = golden(name)
    torch.manual_seed(1623)
    model = AttentionSeq2seq(**json.loads(str(d['kwargs'])))
    _assert_state_dict(model.state_dict(), {k[3:]: d[k] for k in d.files if k.startswith('sd/')})


def test_hierarchical_model_init_matches_reference_state_dict():
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention \
        .hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    d = golden('model_hatt_mha')
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**json.loads(str(d['kwargs'])))
    _assert_state_dict(model.state_dict(), {k[3:]: d[k] for k in d.files if k.startswith('sd/')})


@pytest.mark.parametrize('att_type', ['rnn_attention', 'coverage'])
def test_unbuilt_attention_types_still_raise(att_type):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_layer \
        import AttentionMechanism
    with pytest.raises(NotImplementedError):
        AttentionMechanism(12, 10, att_type, 8)


def test_load_model_two_heads():
    import os
    import yaml
    from pytorch_end2end_speech_recognition_amd.models.load_model import load
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                        'char_blstm_att_100h.yml')
    params = yaml.safe_load(open(path))['param']
    params['num_classes'] = 28
    params['num_heads'] = 2
    model = load('attention', params, 'pytorch')
    assert model.name.endswith('_head2')
    assert model.attend_0_fwd.num_heads == 2
    assert 'attend_0_fwd.W_mha.fc.weight' in model.state_dict()
    assert 'attend_0_fwd.V_head1.fc.weight' in model.state_dict()
