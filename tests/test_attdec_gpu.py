"""The attention decoder pass (csrc/decoder.hip behind asr_attdec_forward_ex /
asr_attdec_backward_ex) against the float64 reference tests/attdec_ref.py on
every path: the three persistent instantiations (pd_kind 0 / 1 / 2) in bf16 and
fp32, the per-step kernels (att_energy<10 | 3 | 0>, the vector and the scalar
cell product), the mixed forms, softmax and sigmoid weights, sharpening, no
initial state, hidden dropout, and the backward with and without the forward's
conv features.  attdec_ref.CASES / GPU_TABLE hold the shapes and what each
reaches; every case asserts the path that ran.

Per tensor -- the saved dec, c, gates, x, ctx, aw of native_ops._attdec_forward
and the ten gradients of native_ops.att_decoder under random cotangents on dec
and ctx -- max |got - f64| / max |f64| <= MARGIN x the error of evaluating the
same reference in float32 (fp32 mode), or x the larger of that and of its
bf16-emulated evaluation (bf16 mode).  err/bound is printed per tensor."""
import ctypes

import numpy as np
import pytest
import torch

import attdec_ref as R

pytestmark = pytest.mark.gpu

ENV_KEYS = ('ASR_ATT_PERSIST', 'ASR_ATT_PERSIST_BWD', 'ASR_ATT_PERSIST32', 'ASR_ATT_CONV_FEAT',
            'ASR_ATT_PERSIST_SS')


def _paths():
    from pytorch_end2end_speech_recognition_amd import _native as N
    p2, l4 = (ctypes.c_int * 2)(), (ctypes.c_int * 4)()
    N.call('asr_attdec_persist_last', p2)
    N.call('asr_attdec_last_launch', l4)
    return [int(v) for v in p2], [int(v) for v in l4]


def _bounds(cf, cb, precision):
    if precision == 'fp32':
        return {k: R.MARGIN * cf[k] for k in cf}
    return {k: R.MARGIN * max(cf[k], cb[k]) for k in cf}


def _compare(tag, got, ref, bound):
    """Prints err/bound of every tensor; returns the names over their bound."""
    bad, line = [], []
    for k, g in got.items():
        g = g.detach().double().cpu().numpy()
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.isfinite(g).all(), (tag, k, 'not finite')
        ratio = R.nerr(g, ref[k]) / bound[k]
        line.append('%s %.3f' % (k, ratio))
        if not ratio <= 1.0:
            bad.append((k, 'err/bound %.3f' % ratio, 'bound %.2e' % bound[k]))
    print(tag, 'err/bound:', ' '.join(line))
    return bad


@pytest.mark.parametrize('case,opt,precision,dispatch', R.GPU_TABLE,
                         ids=['-'.join(r) for r in R.GPU_TABLE])
def test_decoder_pass_matches_f64(case, opt, precision, dispatch, cuda_dev, monkeypatch):
    from pytorch_end2end_speech_recognition_amd import native_ops
    o = R.OPTIONS[opt]
    env = dict(R.DISPATCH[dispatch], **o.get('env', {}))
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = R.expected_path(case, precision, env)
    p = R.dims_of(case)
    inp = R.case_inputs(case)
    ref = R.reference(case, opt)
    bound = _bounds(*R.case_constants(case, opt), precision)
    t = {k: inp[k].detach().to(cuda_dev).requires_grad_(True) for k in R.IN_KEYS}
    if not o['h0']:
        t['h0'] = None
    lens = torch.from_numpy(inp['lens']).to(cuda_dev)
    train = {'dropout_hidden': o['drop'], 'seed_hidden': R.DROP_SEED} if o['drop'] else None
    w = [t[k] for k in ('w_ih', 'w_hh', 'w_dec', 'w_conv', 'conv_w', 'v')]
    tag = '-'.join((case, opt, precision, dispatch))
    native_ops.set_compute_dtype(precision)
    try:
        with torch.no_grad():
            det = lambda v: None if v is None else v.detach()     # noqa: E731
            _, outs, _, _ = native_ops._attdec_forward(
                det(t['enc']), det(t['enc_a']), lens, det(t['pre_emb']), det(t['h0']), p['Y'],
                o['sharpen'], o['sigmoid'], *[det(v) for v in w], train)
        torch.cuda.synchronize()
        pers, last = _paths()
        assert pers[0] == want['fwd'], ('forward path', pers, want)
        assert last[:2] == [want['fwd_tmpl'], want['chunks']], (last, want)
        saved = dict(zip(R.FWD_KEYS, [v.clone() for v in outs]))

        dec, ctx, aw = native_ops.att_decoder(
            t['enc'], t['enc_a'], lens, t['pre_emb'], t['h0'], p['Y'], o['sharpen'], o['sigmoid'],
            *w, train)
        ((dec * inp['cot_dec'].to(cuda_dev)).sum() + (ctx * inp['cot_ctx'].to(cuda_dev)).sum()).backward()
        torch.cuda.synchronize()
        pers, last = _paths()
        assert pers == [want['fwd'], want['bwd']], ('paths', pers, want)
        assert last == [want['fwd_tmpl'], want['chunks'], want['bwd_tmpl'], want['chunks']], (last, want)
    finally:
        native_ops.set_compute_dtype('fp32')

    grads = {'d_' + k: t[k].grad for k in R.IN_KEYS if t[k] is not None}
    assert all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
    bad = _compare(tag + ' saved', saved, ref, bound)
    bad += _compare(tag + ' outputs', dict(dec=dec, ctx=ctx, aw=aw), ref, bound)
    bad += _compare(tag + ' grads', grads, ref, bound)
    assert not bad, (tag, bad)

    # the embedding columns of W_ih enter through pre_emb only
    assert not grads['d_w_ih'][:, :p['Y']].any()
    a = saved['aw'].cpu().numpy()
    if o['sigmoid']:
        for b, n in enumerate(inp['lens']):
            assert (a[b, :, n:] == 0.5).all(), ('padded frames of utterance', b)
    else:
        np.testing.assert_allclose(a.sum(-1), 1.0, rtol=0, atol=1e-5)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_att_step_matches_f64(precision, cuda_dev):
    """asr_att_step_forward / _backward (sigmoid weights, sharpening 2, the
    generic3 dims) against one step of the same reference: ctx, aw and every
    gradient, cotangents on both outputs."""
    from pytorch_end2end_speech_recognition_amd import native_ops
    inp = R.step_inputs()
    ref, cf, cb = R.step_reference()
    bound = _bounds(cf, cb, precision)
    t = {k: inp[k].detach().to(cuda_dev).requires_grad_(True) for k in R.STEP_IN_KEYS}
    lens = torch.from_numpy(inp['lens']).to(cuda_dev)
    native_ops.set_compute_dtype(precision)
    try:
        ctx, aw = native_ops.att_step(t['enc'], t['enc_a'], lens, t['dec_out'], t['aw_prev'],
                                      t['w_dec'], t['w_conv'], t['conv_w'], t['v'],
                                      R.STEP_SHARPEN, R.STEP_SIGMOID)
        ((ctx * inp['cot_ctx'].to(cuda_dev)).sum() + (aw * inp['cot_aw'].to(cuda_dev)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        native_ops.set_compute_dtype('fp32')
    got = dict(ctx=ctx, aw=aw)
    got.update({'d_' + k: t[k].grad for k in R.STEP_IN_KEYS})
    assert all(g is not None for g in got.values())
    bad = _compare('att_step-' + precision, got, ref, bound)
    assert not bad, bad
    a = aw.detach().cpu().numpy()
    for b, n in enumerate(inp['lens']):
        assert (a[b, n:] == 0.5).all(), ('padded frames of utterance', b)
