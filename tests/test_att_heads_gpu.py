"""The multi-head / dot-product attention step (csrc/att_heads.hip behind
native_ops.att_heads_step) against the float64 reference tests/att_heads_ref.py,
its run-to-run bitwise stability (the fixed head-sum order of d dec_out), its
agreement with att_step at one head, the module's dispatch, a refused shape,
and the models built on it against fixtures recorded from the reference
project (tests/golden/make_golden_heads.py).

Per tensor: max |got - f64| / max |f64| <= MARGIN x the error of evaluating
the same reference in float32, in both compute modes (the op is f32 in both).
err/bound is printed per tensor."""
import json

import numpy as np
import pytest
import torch

import att_heads_ref as H
import attdec_ref as R
from conftest import golden, golden_params

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _kind(p):
    return 'dot' if p['kind'] == 'dot_product' else 'additive'


def _run_case(case, dev):
    """{name: device tensor} of att_heads_step forward + backward on a case."""
    ops = _ops()
    p = H.dims_of(case)
    inp = H.case_inputs(case)
    mk = lambda x: x.to(dev).clone().requires_grad_(True)   # noqa: E731
    t = {k: mk(inp[k]) for k in H.ACT_KEYS}
    heads = [{k: mk(v) for k, v in hd.items()} for hd in inp['heads']]
    lens = torch.from_numpy(inp['lens']).to(dev)
    ctx, aw = ops.att_heads_step(t['enc'], t['enc_a'], lens, t['dec_out'], t['aw_prev'], heads,
                                 _kind(p), p['sharpen'], p['sigmoid'])
    assert ops.last_att_heads_path() == 'heads'
    ((ctx * inp['cot_ctx'].to(dev)).sum() + (aw * inp['cot_aw'].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    got = dict(ctx=ctx.detach(), aw=aw.detach())
    got.update({'d_' + k: t[k].grad for k in H.ACT_KEYS})
    for h, hd in enumerate(heads):
        got.update({'d_%s%d' % (k, h): hd[k].grad for k in H.WEIGHT_KEYS[p['kind']]})
    return got


def _compare(tag, got, ref, bound):
    bad, line = [], []
    for k in ref:
        g = got[k].detach().double().cpu().numpy()
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.isfinite(g).all(), (tag, k, 'not finite')
        ratio = R.nerr(g, ref[k]) / bound[k]
        line.append('%s %.3f' % (k, ratio))
        if not ratio <= 1.0:
            bad.append((k, 'err/bound %.3f' % ratio, 'bound %.2e' % bound[k]))
    print(tag, 'err/bound:', ' '.join(line))
    return bad


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', list(H.CASES))
def test_heads_step_matches_f64(case, precision, cuda_dev):
    ops = _ops()
    ops.set_compute_dtype(precision)
    try:
        got = _run_case(case, cuda_dev)
    finally:
        ops.set_compute_dtype('fp32')
    ref, cf = H.reference(case), H.case_constants(case)
    assert sorted(got) == sorted(H.tensor_names(case)) == sorted(ref)
    bad = _compare('%s/%s' % (case, precision), got, ref, {k: H.MARGIN * cf[k] for k in cf})
    assert not bad, bad
    if not H.dims_of(case)['sigmoid']:
        rows = got['aw'].sum(1).cpu().numpy()
        np.testing.assert_allclose(rows, 1.0, atol=1e-5)


@pytest.mark.parametrize('case', list(H.CASES))
def test_heads_step_is_bitwise_repeatable(case, cuda_dev):
    _ops().set_compute_dtype('fp32')
    a, b = _run_case(case, cuda_dev), _run_case(case, cuda_dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_one_head_agrees_with_att_step(cuda_dev):
    """At H = 1 on attdec_ref's step inputs, the new op and att_step both sit
    within their bounds of the same float64 values."""
    ops = _ops()
    ops.set_compute_dtype('fp32')
    inp = R.step_inputs()
    ref, cf, _ = R.step_reference()
    bound = {k: R.MARGIN * cf[k] for k in cf}
    lens = torch.from_numpy(np.asarray(inp['lens'], np.int32)).to(cuda_dev)
    for which in ('att_step', 'att_heads_step'):
        t = {k: inp[k].to(cuda_dev).clone().requires_grad_(True) for k in R.STEP_IN_KEYS}
        if which == 'att_step':
            ctx, aw = ops.att_step(t['enc'], t['enc_a'], lens, t['dec_out'], t['aw_prev'],
                                   t['w_dec'], t['w_conv'], t['conv_w'], t['v'], R.STEP_SHARPEN,
                                   R.STEP_SIGMOID)
        else:
            hd = {k: t[k] for k in ('w_dec', 'w_conv', 'conv_w', 'v')}
            ctx, aw = ops.att_heads_step(t['enc'], t['enc_a'].unsqueeze(3), lens, t['dec_out'],
                                         t['aw_prev'].unsqueeze(2), [hd], 'additive',
                                         R.STEP_SHARPEN, R.STEP_SIGMOID)
            assert ops.last_att_heads_path() == 'heads'
            aw = aw.squeeze(2)
        ((ctx * inp['cot_ctx'].to(cuda_dev)).sum() + (aw * inp['cot_aw'].to(cuda_dev)).sum()
         ).backward()
        torch.cuda.synchronize()
        got = dict(ctx=ctx.detach(), aw=aw.detach())
        got.update({'d_' + k: t[k].grad for k in R.STEP_IN_KEYS})
        bad = _compare(which, got, ref, bound)
        assert not bad, (which, bad)


def _mechanism(kw, dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_layer \
        import AttentionMechanism
    torch.manual_seed(1623)
    return AttentionMechanism(**kw).to(dev)


def test_one_head_location_stays_on_att_step(cuda_dev, monkeypatch):
    ops = _ops()
    ops.set_compute_dtype('fp32')
    d = golden('att_step')
    kw = json.loads(str(d['kwargs']))
    att = _mechanism(kw, cuda_dev)

    def boom(*a, **k):
        raise AssertionError('att_heads_step entered for one-head location attention')
    monkeypatch.setattr(ops, 'att_heads_step', boom)
    t = {k: torch.from_numpy(d[k].copy()).to(cuda_dev)
         for k in ('enc_out', 'enc_out_a', 'dec_out', 'aw_in')}
    lens = torch.from_numpy(d['x_lens']).to(cuda_dev)
    with torch.no_grad():
        ctx, aw = att(t['enc_out'], t['enc_out_a'], lens, t['dec_out'], t['aw_in'])
        B, T = t['aw_in'].shape[:2]
        c2, a2 = ops.att_step(t['enc_out'], t['enc_out_a'].reshape(B, T, -1), lens,
                              t['dec_out'].reshape(B, -1), t['aw_in'].reshape(B, T),
                              att.W_dec_head0.fc.weight, att.W_conv_head0.fc.weight,
                              att.conv_head0.weight, att.V_head0.fc.weight,
                              kw['sharpening_factor'], kw['sigmoid_smoothing'])
    assert tuple(ctx.shape) == (B, 1, 12) and tuple(aw.shape) == (B, T, 1)
    assert torch.equal(ctx[:, 0], c2) and torch.equal(aw[:, :, 0], a2)


@pytest.mark.parametrize('tag', ['loc2', 'dot2'])
def test_mechanism_matches_reference_project(tag, cuda_dev):
    """AttentionMechanism.forward / backward (att_heads_step + W_mha) against
    the reference project's record, at test_attention_step's tolerances."""
    ops = _ops()
    ops.set_compute_dtype('fp32')
    d = golden('att_step_heads')
    kw = json.loads(str(d[tag + '/kwargs']))
    att = _mechanism(kw, cuda_dev)
    pre = tag + '/sd/'
    att.load_state_dict({k[len(pre):]: torch.from_numpy(d[k].copy()) for k in d.files
                         if k.startswith(pre)})
    t = {k: torch.from_numpy(d[tag + '/' + k].copy()).to(cuda_dev).requires_grad_(True)
         for k in ('enc_out', 'enc_out_a', 'dec_out', 'aw_in')}
    lens = torch.from_numpy(d[tag + '/x_lens']).to(cuda_dev)
    ctx, aw = att(t['enc_out'], t['enc_out_a'], lens, t['dec_out'], t['aw_in'])
    Rc, Ra = (torch.from_numpy(d[tag + '/' + k]).to(cuda_dev) for k in ('Rc', 'Ra'))
    ((ctx * Rc).sum() + (aw * Ra).sum()).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(ctx.detach().cpu().numpy(), d[tag + '/ctx'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(aw.detach().cpu().numpy(), d[tag + '/aw_out'], rtol=1e-4,
                               atol=1e-6)
    for k in ('enc_out', 'enc_out_a', 'dec_out', 'aw_in'):
        np.testing.assert_allclose(t[k].grad.cpu().numpy(), d[tag + '/d_' + k], rtol=2e-3,
                                   atol=2e-5, err_msg=k)
    for k, p in att.named_parameters():
        # W_enc_head{h} is the caller's hoisted projection: no gradient here
        got = np.zeros(p.shape, np.float32) if p.grad is None else p.grad.cpu().numpy()
        assert (p.grad is None) == k.startswith('W_enc_head'), k
        np.testing.assert_allclose(got, d[tag + '/grad/' + k], rtol=2e-3, atol=2e-5, err_msg=k)


def test_refused_shape_falls_back_or_raises(cuda_dev):
    """E = 20000 encoder channels need more LDS than the kernels' 64 KiB budget
    (the backward keeps a head's d_ctx row there; forward and backward refuse
    the same shapes): decided on the host from the sizes alone.  Additive
    attention then runs one att_step per head; dot-product attention raises."""
    ops = _ops()
    from pytorch_end2end_speech_recognition_amd._native import NativeError
    ops.set_compute_dtype('fp32')
    g = torch.Generator().manual_seed(5)
    B, T, E, A, D, Hn = 1, 8, 20000, 8, 8, 2
    r = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 0.5).to(cuda_dev)   # noqa: E731
    enc, enc_a, dec = r(B, T, E), r(B, T, A, Hn), r(B, D)
    aw_prev = torch.full((B, T, Hn), 1.0 / T, device=cuda_dev)
    lens = torch.tensor([T - 3], dtype=torch.int32, device=cuda_dev)
    heads = [dict(w_dec=r(A, D), v=r(1, A)) for _ in range(Hn)]
    ctx, aw = ops.att_heads_step(enc, enc_a, lens, dec, aw_prev, heads, 'additive')
    torch.cuda.synchronize()
    assert ops.last_att_heads_path() == 'loop'
    assert tuple(ctx.shape) == (B, Hn * E) and tuple(aw.shape) == (B, T, Hn)
    mask = H.frame_mask(lens.cpu().numpy(), T, torch.float64)
    c64, a64 = H.heads_step(enc.cpu().double(), enc_a.cpu().double(), mask, dec.cpu().double(),
                            aw_prev.cpu().double(),
                            [{k: v.cpu().double() for k, v in hd.items()} for hd in heads],
                            'content', 1.0, False)
    np.testing.assert_allclose(ctx.cpu().numpy(), c64.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(aw.cpu().numpy(), a64.numpy(), rtol=1e-4, atol=1e-7)
    with pytest.raises(NativeError, match='dot-product'):
        ops.att_heads_step(enc, enc_a, lens, dec, aw_prev, [{}, {}], 'dot')


def _check_decodes(model, d, ops):
    model.load_state_dict({k[7:]: torch.from_numpy(d[k].copy()) for k in d.files
                           if k.startswith('dec_sd/')})
    max_len = int(d['dec_max_len'][0])
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=1, max_decode_len=max_len)
    np.testing.assert_array_equal(perm, d['greedy_perm'])
    np.testing.assert_array_equal(np.asarray(hyps), d['greedy'])
    assert np.asarray(aw).shape[:2] == d['greedy'].shape
    hyps, aw, perm = model.decode(d['xs'], d['x_lens'], beam_width=2, max_decode_len=max_len)
    assert ops.last_att_beam_path() == 'host'
    np.testing.assert_array_equal([len(h) for h in hyps], d['beam_lens'])
    np.testing.assert_array_equal(np.concatenate([np.asarray(h, np.int64) for h in hyps]),
                                  d['beam_flat'])


@pytest.mark.parametrize('name', ['model_att_mha', 'model_att_dot', 'model_att_dot_mha'])
def test_attention_model_matches_golden(name, cuda_dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention.attention_seq2seq \
        import AttentionSeq2seq
    ops = _ops()
    ops.set_compute_dtype('fp32')
    d = golden(name)
    kw = json.loads(str(d['kwargs']))
    sd, g = golden_params(d)
    torch.manual_seed(1623)
    model = AttentionSeq2seq(**kw)
    model.load_state_dict(sd)
    model.set_cuda()
    model.zero_grad()
    loss = model(d['xs'], d['ys'], d['x_lens'], d['y_lens'])
    assert tuple(loss.shape) == (1,)
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss.item(), float(d['loss'][0]), rtol=1e-4)
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[k], rtol=2e-3, atol=2e-5, err_msg=k)
    _check_decodes(model, d, ops)


def test_hierarchical_model_matches_golden(cuda_dev):
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.attention \
        .hierarchical_attention_seq2seq import HierarchicalAttentionSeq2seq
    ops = _ops()
    ops.set_compute_dtype('fp32')
    d = golden('model_hatt_mha')
    kw = json.loads(str(d['kwargs']))
    sd, g = golden_params(d)
    torch.manual_seed(1623)
    model = HierarchicalAttentionSeq2seq(**kw)
    model.load_state_dict(sd)
    model.set_cuda()
    model.zero_grad()
    loss, lm, ls = model(d['xs'], d['ys'], d['x_lens'], d['y_lens'], d['ys_sub'],
                         d['y_lens_sub'])
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss.item(), float(d['loss'][0]), rtol=1e-4)
    np.testing.assert_allclose(float(lm), float(d['loss_main'][0]), rtol=1e-4)
    np.testing.assert_allclose(float(ls), float(d['loss_sub'][0]), rtol=1e-4)
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[k], rtol=2e-3, atol=2e-5, err_msg=k)
    _check_decodes(model, d, ops)
