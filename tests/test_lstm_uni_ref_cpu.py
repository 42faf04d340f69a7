"""tests/lstm_uni_ref.py (the float64 reference tests/test_lstm_uni_gpu.py holds
native_ops.lstm_layer to) is right: it equals torch.nn.LSTM(bidirectional=False,
double) over pack_padded_sequence under autograd on small ragged cases with
perm, t_mul = 2, t_add = 1, concat and dropout -- y and every gradient, at the
float64 rounding level tests/test_rnn_layer_ref_cpu.py holds its reference to
-- garbage in x and dy at padded frames changes nothing, dy = None is a zero
cotangent, and the recorded error constants are reproduced."""
import numpy as np
import pytest
import torch

import lstm_uni_ref as U
import rnn_layer_ref as R
from oracle import rng
from test_rnn_layer_ref_cpu import TOL

F64 = torch.float64


def _small(seed, B=4, T=7, H=5, Dsrc=3, perm=False, t_mul=1, t_add=0, concat=False):
    g = torch.Generator().manual_seed(seed)
    Din = 2 * Dsrc if concat else Dsrc
    T_src = t_mul * T + t_add + (1 if concat else 0) + 1
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    p = dict(w_ih=0.4 * r(4 * H, Din), w_hh=0.4 * r(4 * H, H), b_ih=0.4 * r(4 * H),
             b_hh=0.4 * r(4 * H))
    lens = np.array([T, 5, 2, 1][:B], np.int32)
    pm = torch.randperm(B, generator=g).numpy() if perm else np.arange(B)
    return p, r(B, T_src, Dsrc), r(B, T, H), lens, pm, Din


def _torch_layer(p, x_src, dy, lens, pm, T, t_mul, t_add, concat, Din, mask=None):
    """The same op through torch's packed unidirectional module and autograd."""
    H = p['w_hh'].shape[1]
    mod = torch.nn.LSTM(Din, H, batch_first=True, bidirectional=False).double()
    assert not hasattr(mod, 'weight_ih_l0_reverse')
    with torch.no_grad():
        for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh'):
            name = k.replace('w_', 'weight_').replace('b_', 'bias_') + '_l0'
            getattr(mod, name).copy_(p[k])
    x = x_src.clone().requires_grad_(True)
    xm = x if mask is None else x * mask
    X = R.gather_rows(xm, pm, t_mul, t_add, T, concat)
    packed = torch.nn.utils.rnn.pack_padded_sequence(X, torch.as_tensor(lens.astype(np.int64)),
                                                     batch_first=True)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(mod(packed)[0], batch_first=True, total_length=T)
    (y * dy).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dW_ih=mod.weight_ih_l0.grad, dW_hh=mod.weight_hh_l0.grad,
                db_ih=mod.bias_ih_l0.grad, db_hh=mod.bias_hh_l0.grad)


ADDRESSING = {
    'identity': {},
    'perm': dict(perm=True),
    'perm_sub2': dict(perm=True, t_mul=2, t_add=1),
    'concat2': dict(concat=True, t_mul=2),
    'perm_concat_add': dict(perm=True, concat=True, t_mul=2, t_add=1),
}


@pytest.mark.parametrize('addr', sorted(ADDRESSING))
def test_reference_equals_torch_packed_autograd(addr):
    a = dict(perm=False, t_mul=1, t_add=0, concat=False)
    a.update(ADDRESSING[addr])
    T = 7
    p, x, dy, lens, pm, Din = _small(3 + len(addr), T=T, **a)
    got = U.layer(x, lens, T, pm, a['t_mul'], a['t_add'], a['concat'], p['w_ih'], p['w_hh'],
                  p['b_ih'], p['b_hh'], dy)
    want = _torch_layer(p, x, dy, lens, pm, T, a['t_mul'], a['t_add'], a['concat'], Din)
    for k in U.OUT_KEYS:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **TOL)
    for b, n in enumerate(lens):
        assert not got['y'][b, n:].any()
    live = R.mapped_mask(x.shape, lens, pm, a['t_mul'], a['t_add'], T, a['concat'])
    assert not got['dx'][torch.from_numpy(~live)].any()
    assert got['dx'][torch.from_numpy(live)].abs().min() > 0
    assert torch.equal(got['db_ih'], got['db_hh'])


def test_reference_single_frame_equals_torch():
    p, x, dy, lens, pm, Din = _small(17, B=3, T=1)
    lens = np.array([1, 1, 1], np.int32)
    got = U.layer(x, lens, 1, pm, 1, 0, False, p['w_ih'], p['w_hh'], p['b_ih'], p['b_hh'], dy)
    want = _torch_layer(p, x, dy, lens, pm, 1, 1, 0, False, Din)
    for k in U.OUT_KEYS:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **TOL)
    assert not got['dW_hh'].any()


def test_reference_dropout_equals_torch():
    T = 7
    p, x, dy, lens, pm, Din = _small(21, T=T, perm=True, t_mul=2, t_add=1)
    drop = (0.3, 0xABCDEF0123)
    mask = torch.from_numpy(rng.dropout_scale(drop[1], tuple(x.shape), drop[0])).double()
    assert 0 < int((mask == 0).sum()) < mask.numel()
    got = U.layer(x, lens, T, pm, 2, 1, False, p['w_ih'], p['w_hh'], p['b_ih'], p['b_hh'], dy, drop)
    want = _torch_layer(p, x, dy, lens, pm, T, 2, 1, False, Din, mask)
    for k in U.OUT_KEYS:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **TOL)
    assert not got['dx'][mask == 0].any()


def test_garbage_at_padded_frames_changes_nothing_and_none_is_zero():
    T = 7
    a = dict(perm=True, concat=True, t_mul=2, t_add=0)
    p, x, dy, lens, pm, Din = _small(9, T=T, **a)
    run = lambda xx, dd: U.layer(xx, lens, T, pm, 2, 0, True, p['w_ih'], p['w_hh'], p['b_ih'],  # noqa: E731
                                 p['b_hh'], dd)
    live = torch.from_numpy(R.mapped_mask(x.shape, lens, pm, 2, 0, T, True))
    x2, dy2 = x.clone(), dy.clone()
    x2[~live] = 1e3
    for b, n in enumerate(lens):
        dy2[b, n:] = -7e2
    base, other = run(x, dy), run(x2, dy2)
    for k in U.OUT_KEYS:
        np.testing.assert_array_equal(base[k].numpy(), other[k].numpy(), err_msg=k)
    none, zero = run(x, None), run(x, torch.zeros_like(dy))
    for k in U.OUT_KEYS:
        np.testing.assert_array_equal(none[k].numpy(), zero[k].numpy(), err_msg=k)
        assert k == 'y' or not none[k].any()


def test_bf16_emulation_rounds_only_the_documented_operands():
    """With every operand already a bf16 value and one frame (no recurrent
    product, dG read by the GEMMs only), the emulation differs from float32
    only through the rounding of dG."""
    p, x, dy, lens, pm, Din = _small(31, B=3, T=1)
    lens = np.array([1, 1, 1], np.int32)
    rb = lambda a: a.float().to(torch.bfloat16).float()      # noqa: E731
    args = (rb(x), lens, 1, pm, 1, 0, False, rb(p['w_ih']), rb(p['w_hh']), rb(p['b_ih']),
            rb(p['b_hh']), dy.float())
    f32, emu = U.layer(*args), U.layer(*args, bf16=True)
    assert torch.equal(f32['y'], emu['y'])
    assert torch.equal(f32['db_ih'], emu['db_ih'])
    assert not torch.equal(f32['dx'], emu['dx'])
    assert U.nerr(emu['dx'].numpy(), f32['dx'].numpy()) < 2.0 ** -7


@pytest.mark.parametrize('case', sorted(U.CASES))
def test_recorded_constants_are_reproduced_and_f32_has_room(case):
    """As tests/test_rnn_layer_ref_cpu.py holds its table: a bf16 constant to
    25 %, a float32 constant (set by the CPU's summation order) within 4 x both
    ways, and the float32 evaluation within a quarter of the fp32 bound."""
    ref = U.reference(case)
    got = U.measure_constants(case)
    cf, cb = U.case_constants(case)
    c = U.CASES[case]
    assert set(ref) == set(cf) == set(cb) == set(U.OUT_KEYS)
    print(case, ' '.join('%s %.1e/%.1e' % (k, cf[k], cb[k]) for k in sorted(cf)))
    for k in U.OUT_KEYS:
        zero = k == 'dW_hh' and c['T'] == 1
        assert np.isfinite(ref[k]).all() and (np.abs(ref[k]).max() > 0) != zero, k
        assert U.CONST_FLOOR <= cf[k] < 1e-4 and U.CONST_FLOOR <= cb[k] < 0.1, (k, cf[k], cb[k])
        assert cf[k] / 4 <= got['f32'][k] <= 4 * cf[k], (k, got['f32'][k], cf[k])
        assert abs(got['bf16'][k] - cb[k]) <= 0.25 * cb[k], (k, got['bf16'][k], cb[k])
        assert got['f32'][k] <= 0.25 * U.MARGIN * cf[k]
    assert np.array_equal(ref['db_ih'], ref['db_hh'])
    inp = U.case_inputs(case)
    for b, n in enumerate(inp['lens']):
        assert not ref['y'][b, n:].any()
    pm = np.arange(c['B']) if inp['perm'] is None else inp['perm']
    live = R.mapped_mask(inp['x'].shape, inp['lens'], pm, c['t_mul'], c['t_add'], c['T'], c['concat'])
    assert not ref['dx'][~live].any()


def test_case_table_covers_what_the_kernels_branch_on():
    C = U.CASES
    hs = {c['H'] for c in C.values()}
    assert min(hs) == 1 and any(h % 4 for h in hs) and any(h % 8 == 0 and h % 16 for h in hs)
    assert any(h > 128 for h in hs)                       # a second K slice per wave
    assert {1, 15, 17, 31, 33} <= {c['B'] for c in C.values()}
    assert any(c['T'] == 1 for c in C.values())
    assert list(U.case_inputs('h1_b3')['lens']) == [7, 4, 1]
    assert any(c['perm'] for c in C.values()) and any(c['concat'] for c in C.values())
    assert any(c['t_mul'] == 2 and c['t_add'] == 1 for c in C.values())
    assert all(c['Din'] == 9 for c in C.values() if not c['concat'])
    assert any(c['drop'] for c in C.values()) and any(c['garbage'] for c in C.values())
