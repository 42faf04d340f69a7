"""HIP GEMM + BLSTM recurrence vs golden vectors recorded from the reference's
RNNEncoder, and vs the torch-CPU oracle at larger random shapes."""
import json

import numpy as np
import pytest
import torch

from conftest import golden, golden_params
from oracle import asr_ref

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _layer_names(prefix, l, fast):
    if fast:
        fmt = prefix + 'lstm.%s_l%d%s'
        return [[fmt % (n, l, s) for s in ('', '_reverse')]
                for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    fmt = prefix + 'lstm_l%d.%s_l0%s'
    return [[fmt % (l, n, s) for s in ('', '_reverse')]
            for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def run_encoder(p, n_layers, sub, xs_np, x_lens_np, dev, prefix=''):
    """Host glue of RNNEncoder.forward (rnn.py:284-487) over the HIP layer op."""
    ops = _ops()
    fast = sum(sub) == 0
    perm = np.argsort(-x_lens_np, kind='stable')
    lens = x_lens_np[perm].astype(np.int32)
    xs = torch.from_numpy(xs_np).to(dev).requires_grad_(True)
    perm_d = torch.from_numpy(perm.astype(np.int32)).to(dev)
    T = int(lens.max())
    params = []
    h, t_mul, t_add, pm = xs, 1, 0, perm_d
    for l in range(n_layers):
        names = _layer_names(prefix, l, fast)
        ws = [torch.cat([p[a], p[b]]).to(dev).requires_grad_(True) for a, b in names]
        params.append((names, ws))
        lens_d = torch.from_numpy(lens).to(dev)
        h = ops.blstm_layer(h, lens_d, T, *ws, perm=pm, t_mul=t_mul, t_add=t_add)
        pm, t_mul, t_add = None, 1, 0
        if not fast and l != n_layers - 1 and sub[l]:
            T = T // 2
            t_mul, t_add = 2, 1
            lens = np.full_like(lens, T)
    if t_mul != 1:
        raise AssertionError('last layer cannot subsample')
    return xs, h, lens, perm, params


@pytest.mark.parametrize('precision', ['fp32'])
@pytest.mark.parametrize('name', ['enc_fast', 'enc_sub'])
def test_encoder_matches_golden(name, precision, cuda_dev):
    _ops().set_compute_dtype(precision)
    d = golden(name)
    kw = json.loads(str(d['kwargs']))
    p, g = golden_params(d)
    sub = kw['subsample_list'] or [False] * kw['num_layers']
    xs, out, lens, perm, params = run_encoder(p, kw['num_layers'], sub, d['xs'], d['x_lens'],
                                              cuda_dev)
    np.testing.assert_array_equal(perm, d['perm'])
    np.testing.assert_array_equal(lens, d['out_lens'])
    np.testing.assert_allclose(out.detach().cpu().numpy(), d['out'], rtol=1e-4, atol=2e-6)
    (out * torch.from_numpy(d['R']).to(cuda_dev)).sum().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(xs.grad.cpu().numpy(), d['dxs'], rtol=1e-3, atol=1e-5)
    for names, ws in params:
        for (a, b), w in zip(names, ws):
            gw = w.grad.cpu().numpy()
            n = gw.shape[0] // 2
            np.testing.assert_allclose(gw[:n], g[a], rtol=1e-3, atol=1e-5, err_msg=a)
            np.testing.assert_allclose(gw[n:], g[b], rtol=1e-3, atol=1e-5, err_msg=b)


def _random_encoder(Din, H, n_layers, seed):
    rng = np.random.RandomState(seed)
    p = {}
    for l in range(n_layers):
        din = Din if l == 0 else 2 * H
        for s in ('', '_reverse'):
            p['lstm_l%d.weight_ih_l0%s' % (l, s)] = torch.from_numpy(
                rng.uniform(-0.1, 0.1, (4 * H, din)).astype(np.float32))
            p['lstm_l%d.weight_hh_l0%s' % (l, s)] = torch.from_numpy(
                rng.uniform(-0.1, 0.1, (4 * H, H)).astype(np.float32))
            p['lstm_l%d.bias_ih_l0%s' % (l, s)] = torch.from_numpy(
                rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32))
            p['lstm_l%d.bias_hh_l0%s' % (l, s)] = torch.from_numpy(
                rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32))
    return p


@pytest.mark.parametrize('precision,rtol,atol', [('fp32', 1e-4, 1e-5), ('bf16', 5e-2, 2e-2)])
def test_encoder_random_vs_oracle(precision, rtol, atol, cuda_dev):
    """H = 64 (vector fragment path), 3 layers with subsampling, ragged lengths."""
    _ops().set_compute_dtype(precision)
    B, T, Din, H = 6, 40, 24, 64
    sub = [True, False, False]
    p = _random_encoder(Din, H, 3, 11)
    rng = np.random.RandomState(12)
    x_lens = np.array([33, 40, 17, 25, 40, 8], np.int32)
    xs_np = rng.randn(B, T, Din).astype(np.float32)
    for b in range(B):
        xs_np[b, x_lens[b]:] = 0
    xs, out, lens, perm, params = run_encoder(p, 3, sub, xs_np, x_lens, cuda_dev)
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xc = torch.from_numpy(xs_np).requires_grad_(True)
    ref, rlens, rperm = asr_ref.blstm_encoder(pc, '', dict(num_layers=3, subsample_list=sub), xc,
                                              x_lens)
    np.testing.assert_array_equal(perm, rperm)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=rtol,
                               atol=atol)
    R = torch.from_numpy(rng.randn(*ref.shape).astype(np.float32))
    (ref * R).sum().backward()
    (out * R.to(cuda_dev)).sum().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(xs.grad.cpu().numpy(), xc.grad.numpy(), rtol=rtol * 10,
                               atol=atol * 10)
    for names, ws in params:
        for (a, b), w in zip(names, ws):
            gw = w.grad.cpu().numpy()
            ga = torch.cat([pc[a].grad, pc[b].grad]).numpy()
            scale = np.abs(ga).max() + 1e-6
            assert np.abs(gw - ga).max() / scale < (1e-4 if precision == 'fp32' else 5e-2), a
    _ops().set_compute_dtype('fp32')


def test_gemm_linear_vs_torch(cuda_dev):
    ops = _ops()
    ops.set_compute_dtype('fp32')
    rng = np.random.RandomState(3)
    # the last two take the split-K path for dW (reduction length M >= 4096,
    # few output tiles), incl. a ragged final K chunk (4500 = 3*1152 + 1044)
    for (M, K, Nn) in [(300, 123, 29), (7, 5, 3), (1000, 640, 320), (8192, 256, 29),
                       (4500, 96, 130)]:
        x = torch.from_numpy(rng.randn(M, K).astype(np.float32))
        w = torch.from_numpy(rng.randn(Nn, K).astype(np.float32) * 0.1)
        b = torch.from_numpy(rng.randn(Nn).astype(np.float32))
        xd, wd, bd = [t.to(cuda_dev).requires_grad_(True) for t in (x, w, b)]
        y = ops.linear(xd, wd, bd)
        xr, wr, br = [t.clone().requires_grad_(True) for t in (x, w, b)]
        yr = xr @ wr.t() + br
        np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4,
                                   atol=1e-4)
        dy = torch.from_numpy(rng.randn(M, Nn).astype(np.float32))
        y.backward(dy.to(cuda_dev))
        yr.backward(dy)
        torch.cuda.synchronize()
        for a, r in ((xd, xr), (wd, wr), (bd, br)):
            np.testing.assert_allclose(a.grad.cpu().numpy(), r.grad.numpy(), rtol=1e-4, atol=1e-3)


def _persist_status():
    import ctypes
    from pytorch_end2end_speech_recognition_amd import _native as N
    st = ctypes.c_int(0)
    N.call('asr_lstm_persist_status', ctypes.byref(st), 1, N.stream_handle())
    return st.value


_RECURRENCE_MODES = {
    'xg': {},                                   # tagged-granule persistent (lstm_xg.hip)
    'xg_sc1': {'ASR_XG_LOCAL': '0'},            # ... forced write-through hand-off
    'counter': {'ASR_LSTM_XG': '0'},            # counter-form persistent (lstm_persist.hip)
    'step': {'ASR_LSTM_PERSIST': '0'},          # one launch per time step (lstm.hip)
}


@pytest.mark.parametrize('B,T,H', [(20, 37, 64), (32, 120, 512), (7, 15, 320), (48, 50, 256),
                                   (64, 40, 512)])
def test_persistent_recurrence_matches_step_kernels(B, T, H, cuda_dev, monkeypatch):
    """bf16 mode: both persistent one-launch-per-pass recurrences (tagged-granule
    lstm_xg.hip and counter-form lstm_persist.hip) against the per-step kernels
    on the same inputs: outputs, input grads and every weight grad.  Ragged
    lengths, B not a multiple of the row group (padded rows), H = 320 (odd
    k-step count per wave), B = 64 (16-row groups)."""
    ops = _ops()
    ops.set_compute_dtype('bf16')
    rng = np.random.RandomState(B * 1000 + H)
    Din = 48
    lens = np.sort(rng.randint(1, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32))
    ws = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32))
          for s in ((8 * H, Din), (8 * H, H), (8 * H,), (8 * H,))]
    R = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    res = {}
    _persist_status()
    for mode, env in _RECURRENCE_MODES.items():
        for k in ('ASR_LSTM_XG', 'ASR_LSTM_PERSIST', 'ASR_XG_LOCAL'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        xd = x.to(cuda_dev).requires_grad_(True)
        wd = [w.to(cuda_dev).requires_grad_(True) for w in ws]
        lens_d = torch.from_numpy(lens).to(cuda_dev)
        y = ops.blstm_layer(xd, lens_d, T, *wd)
        (y * R).sum().backward()
        torch.cuda.synchronize()
        res[mode] = [y.detach().cpu().numpy(), xd.grad.cpu().numpy()] + \
            [w.grad.cpu().numpy() for w in wd]
        assert _persist_status() == 0, mode
    # forward output of every mode against the fp32 torch-CPU oracle
    H4 = 4 * H
    ref_y = torch.cat([asr_ref.lstm_direction(x, lens, ws[0][:H4], ws[1][:H4], ws[2][:H4],
                                              ws[3][:H4], False),
                       asr_ref.lstm_direction(x, lens, ws[0][H4:], ws[1][H4:], ws[2][H4:],
                                              ws[3][H4:], True)], dim=2).numpy()
    for mode in res:
        err = np.abs(res[mode][0] - ref_y).max() / (np.abs(ref_y).max() + 1e-6)
        assert err < 2e-2, (mode, 'y vs oracle', err)
    names = ['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']
    for mode in ('xg', 'xg_sc1', 'counter'):
        for n, a, b in zip(names, res[mode], res['step']):
            scale = np.abs(b).max() + 1e-6
            assert np.abs(a - b).max() / scale < 2e-2, (mode, n, np.abs(a - b).max(), scale)
        # padded frames are exactly zero
        for b in range(B):
            assert not res[mode][0][b, lens[b]:].any()
    ops.set_compute_dtype('fp32')


def _xg_mode():
    import ctypes
    from pytorch_end2end_speech_recognition_amd import _native as N
    m = ctypes.c_int(0)
    N.call('asr_lstm_xg_mode', ctypes.byref(m), 1)
    return m.value


@pytest.mark.parametrize('B,H', [(32, 512), (64, 512), (28, 256)])
def test_xg_local_and_write_through_agree_bitwise(B, H, cuda_dev, monkeypatch):
    """The tagged-granule recurrence picks its hand-off protocol from the
    placement it measures (XCD-local when every XCD holds whole groups, else
    write-through).  Both run the same arithmetic on the same data, so the
    outputs and all gradients must be bit-identical; and at the bench shape
    the XCD-local protocol must actually be the one that ran."""
    ops = _ops()
    ops.set_compute_dtype('bf16')
    rng = np.random.RandomState(B + H)
    T, Din = 64, 40
    lens = np.sort(rng.randint(T // 2, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32))
    ws = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32))
          for s in ((8 * H, Din), (8 * H, H), (8 * H,), (8 * H,))]
    R = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    out, modes = {}, {}
    for name, local in (('local', '1'), ('sc1', '0')):
        monkeypatch.setenv('ASR_XG_LOCAL', local)
        _xg_mode()
        xd = x.to(cuda_dev).requires_grad_(True)
        wd = [w.to(cuda_dev).requires_grad_(True) for w in ws]
        y = ops.blstm_layer(xd, torch.from_numpy(lens).to(cuda_dev), T, *wd)
        (y * R).sum().backward()
        torch.cuda.synchronize()
        modes[name] = _xg_mode()
        out[name] = [y.detach().cpu().numpy(), xd.grad.cpu().numpy()] + \
            [w.grad.cpu().numpy() for w in wd]
    assert _persist_status() == 0
    assert modes['sc1'] == 1, modes
    if B == 32:
        assert modes['local'] == 2, modes     # one group per XCD at the bench shape
    for a, b in zip(out['local'], out['sc1']):
        np.testing.assert_array_equal(a, b)
    ops.set_compute_dtype('fp32')


@pytest.mark.parametrize('B,T,H', [(20, 37, 64), (7, 15, 320), (32, 120, 320), (28, 50, 256),
                                   (64, 40, 320), (32, 60, 384), (16, 30, 512)])
def test_f32_persistent_recurrence(B, T, H, cuda_dev, monkeypatch):
    """fp32 mode: the tagged-granule recurrence at reference precision (f32
    granules, f32 MFMA; lstm_fwd_xg / lstm_bwd_xg <F32>) against the per-step
    f32 kernels (ASR_LSTM_XG32=0) and the fp32 torch-CPU oracle: outputs, input
    grads and every weight grad within 1e-4 of the largest magnitude (the tag
    bit perturbs one f32 ulp of every other hand-off value), padded frames
    exactly zero; XCD-local and write-through hand-offs bitwise equal.  Ragged
    lengths, B not a multiple of the row group, B = 64 (16-row groups), H = 512
    (persistent forward, per-step backward)."""
    ops = _ops()
    ops.set_compute_dtype('fp32')
    rng = np.random.RandomState(B * 1000 + H + 7)
    Din = 40
    lens = np.sort(rng.randint(1, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32))
    ws = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32))
          for s in ((8 * H, Din), (8 * H, H), (8 * H,), (8 * H,))]
    R = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    res, modes = {}, {}
    _persist_status()
    for name, env in (('xg32', {}), ('xg32_sc1', {'ASR_XG_LOCAL': '0'}),
                      ('step', {'ASR_LSTM_XG32': '0'})):
        for k in ('ASR_LSTM_XG32', 'ASR_XG_LOCAL'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _xg_mode()
        xd = x.to(cuda_dev).requires_grad_(True)
        wd = [w.to(cuda_dev).requires_grad_(True) for w in ws]
        y = ops.blstm_layer(xd, torch.from_numpy(lens).to(cuda_dev), T, *wd)
        (y * R).sum().backward()
        torch.cuda.synchronize()
        modes[name] = _xg_mode()
        res[name] = [y.detach().cpu().numpy(), xd.grad.cpu().numpy()] + \
            [w.grad.cpu().numpy() for w in wd]
        assert _persist_status() == 0, name
    assert modes['step'] == 0 and modes['xg32'] != 0 and modes['xg32_sc1'] == 1, modes
    H4 = 4 * H
    ref_y = torch.cat([asr_ref.lstm_direction(x, lens, ws[0][:H4], ws[1][:H4], ws[2][:H4],
                                              ws[3][:H4], False),
                       asr_ref.lstm_direction(x, lens, ws[0][H4:], ws[1][H4:], ws[2][H4:],
                                              ws[3][H4:], True)], dim=2).numpy()
    err = np.abs(res['xg32'][0] - ref_y).max() / (np.abs(ref_y).max() + 1e-6)
    assert err < 1e-4, ('y vs oracle', err)
    names = ['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']
    for n, a, b in zip(names, res['xg32'], res['step']):
        scale = np.abs(b).max() + 1e-6
        assert np.abs(a - b).max() / scale < 1e-4, (n, np.abs(a - b).max(), scale)
    for n, a, b in zip(names, res['xg32'], res['xg32_sc1']):
        np.testing.assert_array_equal(a, b, err_msg=n)
    for b in range(B):
        assert not res['xg32'][0][b, lens[b]:].any()


def test_f32_persistent_recurrence_tiny_inputs(cuda_dev, monkeypatch):
    """The reference's initialisation (gate biases 0, forget-gate biases 1 in
    b_ih and b_hh, W uniform +-0.1) with tiny inputs, as a random-init VGG
    front-end hands the first BLSTM layer (|x| ~ 1e-5): h stays ~1e-6 for many
    steps, where an activation with absolute error (tanh via 2 sigmoid(2x) - 1:
    ~1e-7) is a 5 % error per step -- vgg_hier's fp32 parity loss was 2e-4 off
    the float64 reference with it.  The persistent f32 kernels against the
    float64 oracle relative to the output's magnitude, beside the per-step
    kernels."""
    ops = _ops()
    ops.set_compute_dtype('fp32')
    rng = np.random.RandomState(77)
    B, T, H, Din = 6, 160, 320, 64
    lens = np.array([T, T - 2, T - 2, T - 7, T - 20, T - 31], np.int32)
    x = torch.from_numpy((rng.randn(B, T, Din) * 3e-6).astype(np.float32))
    ws = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32))
          for s in ((8 * H, Din), (8 * H, H))]
    for _ in range(2):
        bias = torch.zeros(8 * H)
        bias[H:2 * H] = 1.0
        bias[5 * H:6 * H] = 1.0
        ws.append(bias)
    H4 = 4 * H
    x64, w64 = x.double(), [w.double() for w in ws]
    ref = torch.cat([asr_ref.lstm_direction(x64, lens, w64[0][:H4], w64[1][:H4], w64[2][:H4],
                                            w64[3][:H4], False),
                     asr_ref.lstm_direction(x64, lens, w64[0][H4:], w64[1][H4:], w64[2][H4:],
                                            w64[3][H4:], True)], dim=2).numpy()
    scale = np.abs(ref).max()
    errs = {}
    for name, env in (('xg32', {}), ('step', {'ASR_LSTM_XG32': '0'})):
        monkeypatch.delenv('ASR_LSTM_XG32', raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _xg_mode()
        y = ops.blstm_layer(x.to(cuda_dev), torch.from_numpy(lens).to(cuda_dev), T,
                            *[w.to(cuda_dev) for w in ws])
        torch.cuda.synchronize()
        assert (_xg_mode() != 0) == (name == 'xg32'), name
        errs[name] = np.abs(y.cpu().numpy().astype(np.float64) - ref).max() / scale
    assert errs['xg32'] < 1e-4, errs
    assert errs['step'] < 1e-4, errs


def _logical(store, trans, nrows, K, stride_t, stride_b=0, rows_per_b=0, t_add=0, t_limit=0):
    """Materialise the logical [nrows, K] operand of asr_gemm from its flat
    storage and row map (include/asr_hip.h): trans=0 -> element (i, k) at
    row(i) + k; trans=1 -> at row(k) + i."""
    flat = store.reshape(-1)
    nlog = K if trans else nrows
    width = nrows if trans else K
    rpb = rows_per_b if rows_per_b > 0 else nlog + 1
    out = np.zeros((nlog, width), np.float32)
    for r in range(nlog):
        b, t = divmod(r, rpb)
        tp = t + t_add
        if tp < 0 or (t_limit > 0 and tp >= t_limit):
            continue
        o = b * stride_b + tp * stride_t
        out[r] = flat[o:o + width]
    return out.T if trans else out


@pytest.mark.parametrize('fast', ['1', '0'])
def test_gemm_bf16_operand_modes(fast, cuda_dev, monkeypatch):
    """bf16 operands through the range-checked buffer->LDS fast path (and the
    generic kernel for comparison): all four (A, B) layout modes, k-row maps
    with boundary zeros and per-utterance padding, a ragged K, split-K and a
    batched product, against float64 of the same bf16 values."""
    monkeypatch.setenv('ASR_GEMM_FAST', fast)
    ops = _ops()
    ops.set_compute_dtype('bf16')
    rng = np.random.RandomState(7)

    def bf(a):
        return torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16)

    cases = [
        # (M, N, K, a_trans, b_trans, k-row map for trans operands)
        (300, 200, 136, 0, 0, None),
        (200, 130, 4500, 1, 0, None),          # split-K (4 tiles, K >= 4096)
        (256, 96, 700, 1, 1, (350, -1)),       # h_{t-1} style map: 2 groups of 350
        (130, 257, 520, 0, 1, (260, 1)),       # h_{t+1} style map
    ]
    for M, Nn, K, at, bt, kmap in cases:
        ops_ = []
        mats = []
        for trans, nrows in ((at, M), (bt, Nn)):
            if not trans:
                store = rng.randn(nrows, K).astype(np.float32)
                rm = ops.rowmap(K)
                logical = _logical(bf(store).float().numpy(), 0, nrows, K, K)
            elif kmap is None:
                store = rng.randn(K, nrows).astype(np.float32)
                rm = ops.rowmap(nrows)
                logical = _logical(bf(store).float().numpy(), 1, nrows, K, nrows)
            else:
                rpb, tadd = kmap
                ngrp = K // rpb
                store = rng.randn(ngrp * (rpb + 1), nrows).astype(np.float32)
                rm = ops.rowmap(nrows, stride_b=(rpb + 1) * nrows, rows_per_b=rpb, t_add=tadd,
                                t_limit=rpb)
                logical = _logical(bf(store).float().numpy(), 1, nrows, K, nrows,
                                   stride_b=(rpb + 1) * nrows, rows_per_b=rpb, t_add=tadd,
                                   t_limit=rpb)
            t = bf(store).to(cuda_dev)
            ops_.append(ops.operand(t, trans, rm))
            mats.append((t, logical))
        C = torch.full((M, Nn), 0.5, dtype=torch.float32, device=cuda_dev)
        bias = torch.from_numpy(rng.randn(Nn).astype(np.float32)).to(cuda_dev)
        p = ops.gemm_problem(ops_[0], ops_[1], C, ops.rowmap(Nn), M, Nn, K, alpha=0.75,
                             beta=1.0, bias=bias)
        ops.run_gemm([p], cuda_dev)
        torch.cuda.synchronize()
        A = mats[0][1].astype(np.float64)
        Bm = mats[1][1].astype(np.float64)
        ref = 0.75 * A @ Bm.T + 0.5 + bias.cpu().numpy()[None, :]
        got = C.cpu().numpy()
        err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-6)
        assert err < 1e-4, (M, Nn, K, at, bt, err)
    # batched NT product (3 independent products, strided)
    Bt, M, Nn, K = 3, 70, 40, 64
    a = rng.randn(Bt, M, K).astype(np.float32)
    b = rng.randn(Bt, Nn, K).astype(np.float32)
    ad, bd = bf(a).to(cuda_dev), bf(b).to(cuda_dev)
    C = torch.zeros(Bt, M, Nn, dtype=torch.float32, device=cuda_dev)
    p = ops.gemm_problem(ops.operand(ad, 0, ops.rowmap(K)), ops.operand(bd, 0, ops.rowmap(K)), C,
                         ops.rowmap(Nn), M, Nn, K, batch=Bt,
                         batch_strides=(M * K, Nn * K, M * Nn))
    ops.run_gemm([p], cuda_dev)
    torch.cuda.synchronize()
    ref = np.einsum('bmk,bnk->bmn', bf(a).double().numpy(), bf(b).double().numpy())
    np.testing.assert_allclose(C.cpu().numpy(), ref, rtol=1e-4, atol=1e-3)
    ops.set_compute_dtype('fp32')


@pytest.mark.parametrize('B,T,H', [(32, 64, 512), (20, 37, 64), (7, 15, 320)])
def test_lstm_backward_db_is_column_sum_of_dg(B, T, H, cuda_dev, monkeypatch):
    """asr_lstm_backward_db (bias gradients summed inside the tagged-granule
    recurrence) against the column sums of the dG it wrote, in float64 on the
    host; and its dG / dG-bf16 bit-identical to asr_lstm_backward's."""
    import ctypes
    from pytorch_end2end_speech_recognition_amd import _native as N
    for k in ('ASR_LSTM_XG', 'ASR_LSTM_PERSIST', 'ASR_XG_LOCAL'):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.RandomState(B + T + H)
    lens = np.sort(rng.randint(1, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    lens_d = torch.from_numpy(lens).to(cuda_dev)
    gx = torch.from_numpy(rng.randn(B, T, 8 * H).astype(np.float32)).to(cuda_dev)
    whh = torch.from_numpy(rng.uniform(-0.1, 0.1, (8 * H, H)).astype(np.float32)).to(cuda_dev)
    dy = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    y = torch.empty(B, T, 2 * H, device=cuda_dev)
    cst = torch.empty(B, T, 2 * H, device=cuda_dev)
    ybf = torch.empty(B, T, 2 * H, dtype=torch.bfloat16, device=cuda_dev)
    BF = N.ASR_DT_BF16
    whh_r = ctypes.c_void_p(whh.data_ptr() + 4 * H * H * 4)
    nb = N.query('asr_lstm_workspace_bytes', B, H, BF, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda_dev)
    N.call('asr_lstm_forward', N.ptr(gx), N.ptr(whh), whh_r, N.ASR_DT_F32, N.ptr(lens_d), B, T, H,
           BF, N.ptr(y), N.ptr(cst), N.ptr(ybf), N.ptr(ws), nb, N.stream_handle(cuda_dev), None)
    outs = []
    for kind in (1, 2):
        act = gx.clone()
        dgbf = torch.empty(B, T, 8 * H, dtype=torch.bfloat16, device=cuda_dev)
        db = torch.full((2, 8 * H), 0.5, device=cuda_dev)     # accumulates (+=)
        nb = N.query('asr_lstm_workspace_bytes', B, H, BF, kind)
        ws = torch.empty(nb, dtype=torch.uint8, device=cuda_dev)
        if kind == 1:
            N.call('asr_lstm_backward', N.ptr(dy), N.ptr(whh), whh_r, N.ASR_DT_F32, N.ptr(lens_d),
                   B, T, H, BF, N.ptr(act), N.ptr(cst), N.ptr(dgbf), N.ptr(ws), nb,
                   N.stream_handle(cuda_dev), None)
        else:
            N.call('asr_lstm_backward_db', N.ptr(dy), N.ptr(whh), whh_r, N.ASR_DT_F32,
                   N.ptr(lens_d), B, T, H, BF, N.ptr(act), N.ptr(cst), N.ptr(dgbf), N.ptr(db[0]),
                   N.ptr(db[1]), N.ptr(ws), nb, N.stream_handle(cuda_dev), None)
        torch.cuda.synchronize()
        outs.append((act.cpu().numpy(), dgbf.cpu(), db.cpu().numpy()))
    (a1, g1, _), (a2, g2, db2) = outs
    np.testing.assert_array_equal(a1, a2)
    assert torch.equal(g1, g2)
    ref = a2.astype(np.float64).sum(axis=(0, 1)) + 0.5
    scale = np.abs(ref).max()
    for r in (0, 1):
        assert np.abs(db2[r] - ref).max() / scale < 1e-5, r


@pytest.mark.parametrize('sub', [False, True])
def test_dropout_fused_into_next_layer_staging_bitwise(sub, cuda_dev):
    """Inter-layer dropout folded into the next layer's bf16 input staging
    (asr_convert_rows_bf16_dropout; rnn.py:392-393) equals the separate
    dropout pass bit for bit: outputs, the input gradient (the same mask on
    the way back) and every weight gradient; with and without the 'drop'
    subsampling row map between the layers."""
    ops = _ops()
    ops.set_compute_dtype('bf16')
    try:
        rng = np.random.RandomState(3)
        B, T, F, H, p, seed = 4, 48, 24, 64, 0.3, 987654321
        lens = np.array([48, 40, 33, 20], np.int32)
        xs_np = rng.randn(B, T, F).astype(np.float32)
        w0 = [rng.uniform(-0.1, 0.1, s).astype(np.float32)
              for s in ((8 * H, F), (8 * H, H), (8 * H,), (8 * H,))]
        w1 = [rng.uniform(-0.1, 0.1, s).astype(np.float32)
              for s in ((8 * H, 2 * H), (8 * H, H), (8 * H,), (8 * H,))]

        def run(fused):
            xs = torch.from_numpy(xs_np).to(cuda_dev).requires_grad_(True)
            ws0 = [torch.from_numpy(a).to(cuda_dev).requires_grad_(True) for a in w0]
            ws1 = [torch.from_numpy(a).to(cuda_dev).requires_grad_(True) for a in w1]
            lens_d = torch.from_numpy(lens).to(cuda_dev)
            h = ops.blstm_layer(xs, lens_d, T, *ws0)
            T1, tm, ta = (T // 2, 2, 1) if sub else (T, 1, 0)
            lens1 = torch.from_numpy(np.full(B, T1, np.int32) if sub else lens).to(cuda_dev)
            if fused:
                y = ops.blstm_layer(h, lens1, T1, *ws1, t_mul=tm, t_add=ta, drop=(p, seed))
            else:
                y = ops.blstm_layer(ops.dropout(h, p, seed=seed), lens1, T1, *ws1, t_mul=tm,
                                    t_add=ta)
            g = torch.from_numpy(rng_g.randn(*y.shape).astype(np.float32)).to(cuda_dev)
            (y * g).sum().backward()
            torch.cuda.synchronize()
            return [y.detach().cpu().numpy(), xs.grad.cpu().numpy()] + \
                [w.grad.cpu().numpy() for w in ws0 + ws1]

        rng_g = np.random.RandomState(4)
        ref = run(False)
        rng_g = np.random.RandomState(4)
        got = run(True)
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)
    finally:
        ops.set_compute_dtype('fp32')


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,Din', [(32, 300, 512, 1024), (32, 200, 512, 80),
                                       (32, 160, 320, 640), (13, 90, 256, 120)])
def test_fused_input_projection_matches_gemm_path(B, T, H, Din, cuda_dev, monkeypatch):
    """The forward layer pass with the input projection inside the persistent
    recurrence (asr_lstm_forward_x, bf16) against the GEMM + recurrence path
    on the same inputs: outputs, cell states and saved gates agree to the
    projection's f32 summation order (the bf16 operands are identical), and the
    backward gradients that follow agree as well."""
    from pytorch_end2end_speech_recognition_amd import _native as NL
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    if not NL.query('asr_lstm_forward_x_ok', B, H, Din):
        pytest.skip('shape outside the fused path')
    rng = np.random.RandomState(B + T + H)
    lens = np.sort(rng.randint(T // 2, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32) * 0.5).to(cuda_dev)
    w_ih = torch.from_numpy(rng.uniform(-0.1, 0.1, (8 * H, Din)).astype(np.float32)).to(cuda_dev)
    w_hh = torch.from_numpy(rng.uniform(-0.05, 0.05, (8 * H, H)).astype(np.float32)).to(cuda_dev)
    b_ih = torch.from_numpy(rng.uniform(-0.1, 0.1, 8 * H).astype(np.float32)).to(cuda_dev)
    b_hh = torch.from_numpy(rng.uniform(-0.1, 0.1, 8 * H).astype(np.float32)).to(cuda_dev)
    lens_d = torch.from_numpy(lens).to(cuda_dev)
    dy = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    outs = {}
    ops.set_compute_dtype('bf16')
    try:
        for fuse in ('0', '1'):
            monkeypatch.setenv('ASR_FUSE_XPROJ', fuse)
            ws = [t.clone().requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh)]
            xx = x.clone().requires_grad_(True)
            y = ops.blstm_layer(xx, lens_d, T, *ws)
            (y * dy).sum().backward()
            torch.cuda.synchronize()
            outs[fuse] = [y.detach().cpu().numpy(), xx.grad.cpu().numpy()] + \
                [w.grad.cpu().numpy() for w in ws]
    finally:
        ops.set_compute_dtype('fp32')
    names = ['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']
    for n, a, b in zip(names, outs['0'], outs['1']):
        scale = np.abs(a).max() + 1e-12
        err = np.abs(a - b).max() / scale
        assert err < 2e-2, (n, err)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,Din', [(32, 120, 320, 123), (9, 40, 64, 13)])
def test_padded_input_width_matches_fp32(B, T, H, Din, cuda_dev):
    """A layer input whose width is not a multiple of 8 (TIMIT's 123 features,
    BASELINE configs[0]) is staged in bf16 with zero-padded rows, so it takes
    the fused projection and the fast GEMMs: y, dx and every weight gradient
    against the exact-f32 path (unpadded) within the bf16 bound."""
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    rng = np.random.RandomState(B + Din)
    lens = np.sort(rng.randint(T // 2, T + 1, B))[::-1].astype(np.int32)
    lens[0] = T
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32) * 0.5).to(cuda_dev)
    params = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32)).to(cuda_dev)
              for s in ((8 * H, Din), (8 * H, H), (8 * H,), (8 * H,))]
    lens_d = torch.from_numpy(lens).to(cuda_dev)
    dy = torch.from_numpy(rng.randn(B, T, 2 * H).astype(np.float32)).to(cuda_dev)
    outs = {}
    try:
        for cd in ('fp32', 'bf16'):
            ops.set_compute_dtype(cd)
            ws = [t.clone().requires_grad_(True) for t in params]
            xx = x.clone().requires_grad_(True)
            y = ops.blstm_layer(xx, lens_d, T, *ws)
            (y * dy).sum().backward()
            torch.cuda.synchronize()
            outs[cd] = [y.detach().cpu().numpy(), xx.grad.cpu().numpy()] + \
                [w.grad.cpu().numpy() for w in ws]
    finally:
        ops.set_compute_dtype('fp32')
    for n, a, b in zip(['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh'], outs['fp32'], outs['bf16']):
        err = np.abs(a - b).max() / (np.abs(a).max() + 1e-12)
        assert err < 2e-2, (n, err)
    for b in range(B):      # padded frames stay exactly zero
        assert not outs['bf16'][0][b, lens[b]:].any()


@pytest.mark.parametrize('cols,ld', [(10001, 10008), (123, 128), (37, 37)])
def test_convert_rows_unaligned_width(cols, ld, cuda_dev):
    """bf16 staging of rows whose width is not a multiple of 8 (the lane-
    consecutive convert_rows_cols path): dst[r][c] = bf16(src[row(r)][c]), the
    padding columns and the rows mapped outside [0, t_limit) zero; with the
    fused dropout, the element mask of asr_dropout over src."""
    ops = _ops()
    N = ops.N
    rng = np.random.RandomState(5)
    B, T = 3, 7
    src = torch.from_numpy(rng.randn(B, T, cols).astype(np.float32)).to(cuda_dev)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device=cuda_dev)
    # rows (b, t) -> src[perm[b]][t - 1]: t = 0 maps outside and is zero
    m = ops.rowmap(cols, stride_b=T * cols, rows_per_b=T, t_add=-1, t_limit=T, perm=perm)
    out = torch.full((B * T, ld), 7.0, dtype=torch.bfloat16, device=cuda_dev)
    N.call('asr_convert_rows_bf16_ld', N.ptr(src), m, B * T, cols, ld, N.ptr(out),
           N.stream_handle(cuda_dev))
    ref = torch.zeros(B, T, ld, dtype=torch.float32, device=cuda_dev)
    ref[:, 1:, :cols] = src[perm.long()][:, :T - 1]
    torch.testing.assert_close(out.float().view(B, T, ld), ref.to(torch.bfloat16).float(),
                               rtol=0, atol=0)
    if ld == cols:
        p, seed = 0.3, 424242
        outd = torch.empty(B * T, cols, dtype=torch.bfloat16, device=cuda_dev)
        N.call('asr_convert_rows_bf16_dropout', N.ptr(src), m, B * T, cols, N.ptr(outd), p, seed,
               N.stream_handle(cuda_dev))
        dropped = torch.empty_like(src)
        N.call('asr_dropout', N.ptr(src), N.ptr(dropped), src.numel(), p, seed,
               N.stream_handle(cuda_dev))
        refd = torch.zeros(B, T, cols, dtype=torch.float32, device=cuda_dev)
        refd[:, 1:] = dropped[perm.long()][:, :T - 1]
        torch.testing.assert_close(outd.float().view(B, T, cols),
                                   refd.to(torch.bfloat16).float(), rtol=0, atol=0)
