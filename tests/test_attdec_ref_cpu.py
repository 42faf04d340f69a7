"""tests/attdec_ref.py (the float64 reference tests/test_attdec_gpu.py holds the
decoder kernels to) is right: one float64 step equals oracle.asr_ref's
location_attention + lstm_cell composed by hand (softmax and sigmoid), it
reproduces the attention-step vectors recorded from the reference project
(tests/golden/att_step.npz), torch.autograd.gradcheck passes on a two-step
instance (sigmoid, sharpening 2), the bf16 emulation rounds where it says, the
expected-path table matches the cases' purposes, and the error constants of
every GPU case are finite and non-zero (printed; DESIGN.md holds the table)."""
import json

import numpy as np
import pytest
import torch

import attdec_ref as R
from conftest import golden, golden_params
from oracle import asr_ref

PRE = 'att.'


def _rand_case(sigmoid, seed=3):
    g = torch.Generator().manual_seed(seed)
    B, T, E, A, C, K, D, Y = 3, 9, 5, 4, 2, 5, 6, 2
    r = lambda *s, sc=0.3: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * sc)  # noqa: E731
    t = dict(enc=r(B, T, E, sc=1.0), enc_a=r(B, T, A, sc=1.0), pre_emb=r(B, 2, 4 * D, sc=0.5),
             h0=r(B, D, sc=0.5), w_ih=r(4 * D, Y + E), w_hh=r(4 * D, D), w_dec=r(A, D),
             w_conv=r(A, C), conv_w=r(C, 1, 1, K), v=r(1, A))
    lens = np.array([9, 4, 1], np.int32)
    return t, lens, dict(B=B, T=T, E=E, A=A, C=C, K=K, D=D, Y=Y)


@pytest.mark.parametrize('sigmoid', [False, True])
def test_step_equals_oracle_composition(sigmoid):
    """Two rows of the pass (t = 0: attention on h0; t = 1: cell, then
    attention) against asr_ref.location_attention / lstm_cell with the
    embedding half of the cell input folded into pre_emb, as the kernels get it."""
    t, lens, p = _rand_case(sigmoid)
    sharpen = 1.7
    out = R.decoder_pass(t['enc'], t['enc_a'], lens, t['pre_emb'], t['h0'], t['w_ih'], t['w_hh'],
                         t['w_dec'], t['w_conv'], t['conv_w'], t['v'], sharpen, sigmoid)
    par = {PRE + 'conv_head0.weight': t['conv_w'], PRE + 'W_dec_head0.fc.weight': t['w_dec'],
           PRE + 'W_conv_head0.fc.weight': t['w_conv'], PRE + 'V_head0.fc.weight': t['v']}
    B, T, D, Y = p['B'], p['T'], p['D'], p['Y']
    aw0 = torch.zeros(B, T, dtype=torch.float64)
    ctx0, aw_0 = asr_ref.location_attention(par, PRE, t['enc'], t['enc_a'], lens, t['h0'], aw0,
                                            sharpen, sigmoid)
    # the cell on [emb; ctx_0]: the embedding columns' product and both biases are pre_emb
    g = torch.Generator().manual_seed(9)
    emb = torch.rand(B, Y, generator=g, dtype=torch.float64)
    b_ih = t['pre_emb'][:, 1] - emb @ t['w_ih'][:, :Y].t()       # per-utterance "bias"
    cellp = {'cell.weight_ih': t['w_ih'], 'cell.weight_hh': t['w_hh'], 'cell.bias_ih': b_ih,
             'cell.bias_hh': torch.zeros(4 * D, dtype=torch.float64)}
    h1, c1 = asr_ref.lstm_cell(cellp, 'cell', torch.cat([emb, ctx0], 1), t['h0'],
                               torch.zeros(B, D, dtype=torch.float64))
    ctx1, aw_1 = asr_ref.location_attention(par, PRE, t['enc'], t['enc_a'], lens, h1, aw_0,
                                            sharpen, sigmoid)
    tol = dict(rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(out['dec'][:, 0].numpy(), t['h0'].numpy(), **tol)
    np.testing.assert_allclose(out['ctx'][:, 0].numpy(), ctx0.numpy(), **tol)
    np.testing.assert_allclose(out['aw'][:, 0].numpy(), aw_0.numpy(), **tol)
    np.testing.assert_allclose(out['dec'][:, 1].numpy(), h1.numpy(), **tol)
    np.testing.assert_allclose(out['c'][:, 1].numpy(), c1.numpy(), **tol)
    np.testing.assert_allclose(out['ctx'][:, 1].numpy(), ctx1.numpy(), **tol)
    np.testing.assert_allclose(out['aw'][:, 1].numpy(), aw_1.numpy(), **tol)
    np.testing.assert_allclose(out['x'][:, 1].numpy(), torch.cat([ctx0, t['h0']], 1).numpy(), **tol)
    # what row 0 holds, and the padded frames' weights
    for k in ('c', 'gates', 'x'):
        assert not out[k][:, 0].any(), k
    if sigmoid:
        assert (out['aw'][1, :, 4:] == 0.5).all() and (out['aw'][2, :, 1:] == 0.5).all()
    else:
        np.testing.assert_allclose(out['aw'].sum(-1).numpy(), 1.0, rtol=1e-12)
        assert (out['aw'][2, :, 1:] > 0).all()      # padded frames keep a weight


def test_reproduces_recorded_attention_step():
    d = golden('att_step')
    kw = json.loads(str(d['kwargs']))
    p, g = golden_params(d)
    names = dict(w_dec='W_dec_head0.fc.weight', w_conv='W_conv_head0.fc.weight',
                 conv_w='conv_head0.weight', v='V_head0.fc.weight')
    w = {k: p[n].requires_grad_(True) for k, n in names.items()}
    enc = torch.from_numpy(d['enc_out']).requires_grad_(True)
    enc_a = torch.from_numpy(d['enc_out_a'][..., 0]).requires_grad_(True)
    dec_out = torch.from_numpy(d['dec_out'][:, 0]).requires_grad_(True)
    aw_in = torch.from_numpy(d['aw_in'][..., 0]).requires_grad_(True)
    mask = R.frame_mask(d['x_lens'], enc.shape[1], enc.dtype)
    ctx, aw = R.attention_step(enc, enc_a, mask, dec_out, aw_in, w['w_dec'], w['w_conv'],
                               w['conv_w'], w['v'], kw['sharpening_factor'],
                               kw['sigmoid_smoothing'])
    np.testing.assert_allclose(ctx.detach().numpy(), d['ctx'][:, 0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(aw.detach().numpy(), d['aw_out'][..., 0], rtol=1e-5, atol=1e-7)
    ((ctx * torch.from_numpy(d['Rc'][:, 0])).sum()
     + (aw * torch.from_numpy(d['Ra'][..., 0])).sum()).backward()
    tol = dict(rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(enc.grad.numpy(), d['d_enc_out'], **tol)
    np.testing.assert_allclose(enc_a.grad.numpy(), d['d_enc_out_a'][..., 0], **tol)
    np.testing.assert_allclose(dec_out.grad.numpy(), d['d_dec_out'][:, 0], **tol)
    np.testing.assert_allclose(aw_in.grad.numpy(), d['d_aw_in'][..., 0], **tol)
    for k, n in names.items():
        np.testing.assert_allclose(w[k].grad.numpy(), g[n], err_msg=n, **tol)


def test_gradcheck_two_steps_sigmoid_sharpened():
    g = torch.Generator().manual_seed(5)
    B, T, E, A, C, K, D, Y = 2, 4, 3, 3, 2, 3, 2, 1
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)  # noqa: E731
    args = (r(B, T, E), r(B, T, A), r(B, 2, 4 * D), r(B, D), r(4 * D, Y + E), r(4 * D, D), r(A, D),
            r(A, C), r(C, 1, 1, K), r(1, A))
    lens = np.array([4, 2], np.int32)
    drop = torch.tensor([[[1.25, 0.0]] * 2] * B, dtype=torch.float64)

    def fn(enc, enc_a, pre_emb, h0, w_ih, w_hh, w_dec, w_conv, conv_w, v):
        o = R.decoder_pass(enc, enc_a, lens, pre_emb, h0, w_ih, w_hh, w_dec, w_conv, conv_w, v,
                           2.0, True, drop)
        return o['dec'], o['ctx'], o['aw'], o['c']

    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_round_bf16_is_straight_through():
    x = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.3], requires_grad=True)
    y = R.round_bf16(x)
    np.testing.assert_array_equal(y.detach().numpy(),
                                  x.detach().to(torch.bfloat16).to(torch.float32).numpy())
    assert y[0] == 1.0 and y[1] == 1.0 and y[2] == 1.0 + 2.0 ** -6     # ties to even
    gin = torch.tensor([1.0 + 2.0 ** -9, 0.1, -7.77, 1e-3])
    y.backward(gin)
    np.testing.assert_array_equal(x.grad.numpy(), gin.to(torch.bfloat16).to(torch.float32).numpy())
    x.grad = None
    R.round_bf16(x, fwd=False, bwd=False).backward(gin)
    np.testing.assert_array_equal(x.grad.numpy(), gin.numpy())


def test_bf16_emulation_rounds_the_named_operands():
    """The emulated products against hand-rounded ones."""
    g = torch.Generator().manual_seed(2)
    rb = lambda a: a.to(torch.bfloat16).to(torch.float32)    # noqa: E731
    x = torch.randn(3, 8, generator=g, requires_grad=True)
    w = torch.randn(5, 8, generator=g, requires_grad=True)
    dy = torch.randn(3, 5, generator=g)
    R._cell_product(x, w, True).backward(dy)
    np.testing.assert_array_equal(x.grad.numpy(), (rb(dy) @ rb(w.detach())).numpy())
    np.testing.assert_array_equal(w.grad.numpy(), (rb(dy).t() @ rb(x.detach())).numpy())
    x.grad = w.grad = None
    y = R._wgrad_rounded(lambda a, b: a @ b.t(), x, w, True)
    np.testing.assert_array_equal(y.detach().numpy(), (x @ w.t()).detach().numpy())
    y.backward(dy)
    np.testing.assert_array_equal(x.grad.numpy(), (dy @ w.detach()).numpy())
    np.testing.assert_array_equal(w.grad.numpy(), (rb(dy).t() @ rb(x.detach())).numpy())


def test_expected_paths_match_the_cases_purposes():
    ep = lambda c, prec='bf16', **env: R.expected_path(c, prec, env)   # noqa: E731
    for prec in ('bf16', 'fp32'):
        for c in ('generic3', 'generic4', 'tiny', 't_edge505'):
            e = ep(c, prec)
            assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (1, 1, 0, 0), (c, e)
        for c in ('ten_rt', 'prod_geom'):
            e = ep(c, prec)
            assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (1, 1, 10, 10), (c, e)
        e = ep('ten_wideA', prec)
        assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (0, 0, 10, 10)
        e = ep('c16', prec)
        assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (0, 0, 0, 0)
        e = ep('t_edge513', prec)
        assert (e['fwd'], e['bwd'], e['chunks']) == (0, 0, 17)
        e = ep('k_wide', prec)
        assert (e['fwd'], e['bwd']) == (1, 0)
        # (E + D) % 8 != 0 keeps the forward per-step; the backward's 4 D % 8 == 0 holds
        e = ep('odd_ed', prec)
        assert (e['fwd'], e['bwd']) == (0, 1)
        e = ep('generic3', prec, ASR_ATT_PERSIST='0')
        assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (0, 0, 3, 3)
        e = ep('generic3', prec, ASR_ATT_PERSIST_BWD='0')
        assert (e['fwd'], e['bwd'], e['fwd_tmpl'], e['bwd_tmpl']) == (1, 0, 0, 3)
    assert R.pd_kind(R.dims_of('prod_geom')) == 2 and R.pd_kind(R.dims_of('ten_rt')) == 1


def test_lens_cover_the_short_utterances():
    for c in R.CASES:
        p = R.dims_of(c)
        lens = R.case_inputs(c)['lens']
        assert lens[0] == p['T'] and (np.diff(lens) <= 0).all() and lens.min() >= 1
        if p['B'] >= 2:
            assert lens[-1] == 1
        if p['B'] >= 3 and p['K'] >= 5:
            assert 1 <= lens[-2] < p['K'] / 2


def test_step_constants_are_finite_and_nonzero():
    f64, cf, cb = R.step_reference()
    assert set(f64) == {'ctx', 'aw'} | {'d_' + k for k in R.STEP_IN_KEYS}
    print(' '.join('%s %.1e/%.1e' % (k, cf[k], cb[k]) for k in sorted(cf)))
    for k in f64:
        assert np.isfinite(f64[k]).all() and np.abs(f64[k]).max() > 0, k
        assert R.CONST_FLOOR <= cf[k] < 1e-4 and R.CONST_FLOOR <= cb[k] < 0.1, (k, cf[k], cb[k])


_PAIRS = sorted({(c, R._ref_key(o)) for c, o, _, _ in R.GPU_TABLE})


@pytest.mark.parametrize('case,opt', _PAIRS, ids=['%s-%s' % p for p in _PAIRS])
def test_case_constants_are_finite_and_nonzero(case, opt):
    cf, cb = R.case_constants(case, opt)
    ref = R.reference(case, opt)
    want = set(R.FWD_KEYS) | set(R.GRAD_KEYS)
    if not R.OPTIONS[opt]['h0']:
        want.discard('d_h0')
    assert set(cf) == set(cb) == set(ref) == want
    print(case, opt, ' '.join('%s %.1e/%.1e' % (k, cf[k], cb[k]) for k in sorted(cf)))
    for k in cf:
        assert np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, k
        assert np.isfinite(cf[k]) and cf[k] >= R.CONST_FLOOR, k
        assert np.isfinite(cb[k]) and cb[k] >= R.CONST_FLOOR, k
        assert cf[k] < 1e-4 and cb[k] < 0.1, (k, cf[k], cb[k])   # a broken evaluation, not rounding
    # the first Y columns of W_ih never enter the pass
    assert not ref['d_w_ih'][:, :R.dims_of(case)['Y']].any()
    if R.OPTIONS[opt]['sigmoid']:
        lens = R.case_inputs(case)['lens']
        for b, n in enumerate(lens):
            assert (ref['aw'][b, :, n:] == 0.5).all()
    else:
        np.testing.assert_allclose(ref['aw'].sum(-1), 1.0, rtol=1e-12)
