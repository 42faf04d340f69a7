"""The BLSTM and BGRU layer passes (native_ops.blstm_layer / bgru_layer over
csrc/lstm.hip, lstm_persist.hip, lstm_xg.hip, gru.hip and the layer GEMMs)
against the float64 reference tests/rnn_layer_ref.py on every path: the fused
projection with packed and with f32 activations, the tagged-granule recurrence
after the GEMM, the separate bias column sum, 32 units per backward work-group,
the write-through hand-off, the counter form, the per-step kernels (fast, and
generic with vec = 1 and 0) and the f32 tagged-granule and per-step forms; perm
/ t_mul / t_add / concat addressing, an input width that is no multiple of 8,
input dropout, garbage in x at padded frames, a two-layer stack with the bf16
hand-off, and the GRU kernels with unit and batch tails.  rnn_layer_ref.CASES /
GPU_TABLE hold the shapes and what each reaches; every BLSTM row asserts the
path that ran.

Every row: a cotangent at every frame (padded ones included), the four gradient
buffers filled with random values on entry (compared: grad - fill), y exactly
zero at padded frames, dx exactly zero at padded and unmapped source frames,
db_ih == db_hh bitwise (BLSTM), no give-up of a persistent recurrence, and per
tensor max |got - f64| / max |f64| <= MARGIN x the error of evaluating the same
reference in float32 (fp32 mode), or x the larger of that and of its
bf16-emulated evaluation (bf16 mode).  err/bound is printed per tensor."""
import ctypes

import numpy as np
import pytest
import torch

import rnn_layer_ref as R

pytestmark = pytest.mark.gpu

PARAMS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')
GRADS = dict(zip(PARAMS, R.OUT_KEYS[2:]))


def _last_path():
    from pytorch_end2end_speech_recognition_amd import _native as N
    out = (ctypes.c_int * 2)()
    N.call('asr_lstm_last_path', ctypes.cast(out, ctypes.c_void_p))
    return [int(v) for v in out]


def _compare(tag, got, ref, bound):
    """Prints err/bound of every tensor; returns the names over their bound."""
    bad, line = [], []
    for k, g in got.items():
        g = g.detach().double().cpu().numpy()
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.isfinite(g).all(), (tag, k, 'not finite')
        err = R.nerr(g, ref[k])
        # (a bound of 0: a tensor that is exactly zero, dW_hh of a single frame)
        ratio = err / bound[k] if np.abs(ref[k]).max() > 0 else (np.inf if g.any() else 0.0)
        line.append('%s %.3f' % (k, ratio))
        if not ratio <= 1.0:
            bad.append((k, 'err/bound %.3f' % ratio, 'bound %.2e' % bound[k]))
    print(tag, 'err/bound:', ' '.join(line))
    return bad


def _params(inp, ref, sfx, dev, gen, kind):
    """Device parameters of one layer, their .grad filled with U(+-1/4 of the
    reference gradient's largest value), and the fills (BLSTM: one fill for
    both bias gradients, which must then stay equal bit for bit)."""
    ps, fills = [], {}
    for k in PARAMS:
        p = inp[k + sfx].to(dev).requires_grad_(True)
        scale = 0.25 * float(np.abs(ref[GRADS[k] + sfx]).max())
        fill = ((torch.rand(p.shape, generator=gen) * 2 - 1) * scale).to(dev)
        if k == 'b_hh' and kind == 'lstm':
            fill = fills['db_ih' + sfx]
        p.grad = fill.clone()
        ps.append(p)
        fills[GRADS[k] + sfx] = fill
    return ps, fills


@pytest.mark.parametrize('case,precision,dispatch', R.GPU_TABLE,
                         ids=['-'.join(r) for r in R.GPU_TABLE])
def test_layer_pass_matches_f64(case, precision, dispatch, cuda_dev, monkeypatch):
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    c = R.CASES[case]
    env = R.DISPATCH[dispatch]
    for k in R.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = R.expected_path(case, precision, env)
    inp, ref = R.case_inputs(case), R.reference(case)
    bound = R.bounds(case, precision, dispatch)
    tag = '-'.join((case, precision, dispatch))
    dev = cuda_dev
    gen = torch.Generator().manual_seed(len(tag))
    ps, fills = _params(inp, ref, '', dev, gen, c['kind'])
    x = inp['x'].to(dev).requires_grad_(True)
    lens = torch.from_numpy(inp['lens']).to(dev)
    perm = None if inp['perm'] is None else torch.from_numpy(inp['perm']).to(dev)
    kw = dict(perm=perm, t_mul=c['t_mul'], t_add=c['t_add'], concat=c['concat'])
    drop = (c['drop'], R.DROP_SEED) if c['drop'] else None
    ops.set_compute_dtype(precision)
    try:
        ops.recurrence_status(dev)               # clear what an earlier test left
        if c['kind'] == 'gru':
            y = ops.bgru_layer(x, lens, c['T'], *ps, **kw)
        elif c['stack']:
            hand = (0.2, R.HANDOFF_SEED)
            ps2, fills2 = _params(inp, ref, '2', dev, gen, c['kind'])
            fills.update(fills2)
            y1 = ops.blstm_layer(x, lens, c['T'], *ps, drop=drop, bf16_handoff=True, out_drop=hand,
                                 **kw)
            y = ops.blstm_layer(y1, lens, c['T'], *ps2, drop=hand, next_rec=True)
            ps = ps + ps2
        else:
            y = ops.blstm_layer(x, lens, c['T'], *ps, drop=drop, **kw)
        torch.cuda.synchronize()
        if want is not None:
            assert _last_path()[0] == want['fwd'], ('forward path', _last_path(), want)
        y.backward(inp['dy'].to(dev))
        torch.cuda.synchronize()
        if want is not None:
            assert _last_path() == [want['fwd'], want['bwd']], ('paths', _last_path(), want)
        st = ops.recurrence_status(dev)
        assert int(st.max()) == 0, ('a persistent recurrence gave up', st.tolist())
    finally:
        ops.set_compute_dtype('fp32')

    names = [GRADS[k] + s for s in (('', '2') if c['stack'] else ('',)) for k in PARAMS]
    got = dict(y=y, dx=x.grad)
    got.update({n: p.grad - fills[n] for n, p in zip(names, ps)})
    assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
    bad = _compare(tag, got, ref, bound)
    assert not bad, (tag, bad)

    yh, dxh = y.detach().cpu().numpy(), x.grad.cpu().numpy()
    for b, n in enumerate(inp['lens']):
        assert not yh[b, n:].any(), ('y at padded frames of utterance', b)
    pm = np.arange(c['B']) if inp['perm'] is None else inp['perm']
    live = R.mapped_mask(dxh.shape, inp['lens'], pm, c['t_mul'], c['t_add'], c['T'], c['concat'])
    assert not dxh[~live].any(), 'dx at padded or unmapped source frames'
    if c['kind'] == 'lstm':
        for s in ('', '2') if c['stack'] else ('',):
            gi, gh = (p.grad for n, p in zip(names, ps) if n in ('db_ih' + s, 'db_hh' + s))
            assert torch.equal(gi, gh), 'db_ih != db_hh' + s
