"""tests/rnn_layer_ref.py (the float64 reference tests/test_rnn_layer_gpu.py
holds the BLSTM / BGRU layer passes to) is right: it equals torch.nn.LSTM /
torch.nn.GRU (bidirectional, double, pack_padded_sequence, autograd) on small
ragged cases with perm, t_mul = 2, t_add = 1, concat and dropout, its LSTM half
equals oracle.asr_ref.lstm_direction_bptt, garbage in x and dy at padded frames
changes nothing, the fp16 gate packing decodes as documented, the recorded
error constants are reproduced, the float32 evaluation of every case stays
within a quarter of its own bound, and the expected-path table is consistent
with the GPU table."""
import numpy as np
import pytest
import torch

import rnn_layer_ref as R
from oracle import asr_ref, rng

F64 = torch.float64
TOL = dict(rtol=1e-10, atol=1e-13)


def _small(kind, seed, B=4, T=7, H=5, Dsrc=3, perm=False, t_mul=1, t_add=0, concat=False):
    g = torch.Generator().manual_seed(seed)
    ng = 8 if kind == 'lstm' else 6
    Din = 2 * Dsrc if concat else Dsrc
    T_src = t_mul * T + t_add + (1 if concat else 0) + 1
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    p = dict(w_ih=0.4 * r(ng * H, Din), w_hh=0.4 * r(ng * H, H), b_ih=0.4 * r(ng * H),
             b_hh=0.4 * r(ng * H))
    lens = np.array([T, 5, 2, 1][:B], np.int32)
    pm = torch.randperm(B, generator=g).numpy() if perm else np.arange(B)
    return p, r(B, T_src, Dsrc), r(B, T, 2 * H), lens, pm, Din


def _torch_layer(kind, p, x_src, dy, lens, pm, T, t_mul, t_add, concat, Din, mask=None):
    """The same op through torch's packed bidirectional module and autograd."""
    H = p['w_hh'].shape[1]
    ng = 4 if kind == 'lstm' else 3
    mod = (torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU)(
        Din, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in enumerate(('', '_reverse')):
            sl = slice(d * ng * H, (d + 1) * ng * H)
            for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh'):
                name = k.replace('w_', 'weight_').replace('b_', 'bias_') + '_l0' + sfx
                getattr(mod, name).copy_(p[k][sl])
    x = x_src.clone().requires_grad_(True)
    xm = x if mask is None else x * mask
    X = R.gather_rows(xm, pm, t_mul, t_add, T, concat)
    packed = torch.nn.utils.rnn.pack_padded_sequence(X, torch.as_tensor(lens.astype(np.int64)),
                                                     batch_first=True)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(mod(packed)[0], batch_first=True, total_length=T)
    (y * dy).sum().backward()
    cat = lambda k: torch.cat([getattr(mod, k + '_l0').grad, getattr(mod, k + '_l0_reverse').grad])  # noqa: E731
    return dict(y=y.detach(), dx=x.grad, dW_ih=cat('weight_ih'), dW_hh=cat('weight_hh'),
                db_ih=cat('bias_ih'), db_hh=cat('bias_hh'))


ADDRESSING = {
    'identity': {},
    'perm': dict(perm=True),
    'perm_sub2': dict(perm=True, t_mul=2, t_add=1),
    'concat2': dict(concat=True, t_mul=2),
    'perm_concat_add': dict(perm=True, concat=True, t_mul=2, t_add=1),
}


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
@pytest.mark.parametrize('addr', sorted(ADDRESSING))
def test_reference_equals_torch_packed_autograd(kind, addr):
    a = dict(perm=False, t_mul=1, t_add=0, concat=False)
    a.update(ADDRESSING[addr])
    T = 7
    p, x, dy, lens, pm, Din = _small(kind, 3 + len(addr), T=T, **a)
    got = R.layer(kind, x, lens, T, pm, a['t_mul'], a['t_add'], a['concat'], p['w_ih'], p['w_hh'],
                  p['b_ih'], p['b_hh'], dy)
    want = _torch_layer(kind, p, x, dy, lens, pm, T, a['t_mul'], a['t_add'], a['concat'], Din)
    for k in R.OUT_KEYS:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **TOL)
    # exact zeros: padded frames of y, source frames no live row reads
    for b, n in enumerate(lens):
        assert not got['y'][b, n:].any()
    live = R.mapped_mask(x.shape, lens, pm, a['t_mul'], a['t_add'], T, a['concat'])
    assert not got['dx'][torch.from_numpy(~live)].any()
    assert got['dx'][torch.from_numpy(live)].abs().min() > 0
    if kind == 'lstm':
        assert torch.equal(got['db_ih'], got['db_hh'])


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_reference_dropout_equals_torch(kind):
    T = 7
    p, x, dy, lens, pm, Din = _small(kind, 21, T=T, perm=True, t_mul=2, t_add=1)
    drop = (0.3, 0xABCDEF0123)
    mask = torch.from_numpy(rng.dropout_scale(drop[1], tuple(x.shape), drop[0])).double()
    assert 0 < int((mask == 0).sum()) < mask.numel()
    got = R.layer(kind, x, lens, T, pm, 2, 1, False, p['w_ih'], p['w_hh'], p['b_ih'], p['b_hh'], dy,
                  drop)
    want = _torch_layer(kind, p, x, dy, lens, pm, T, 2, 1, False, Din, mask)
    for k in R.OUT_KEYS:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **TOL)
    assert not got['dx'][mask == 0].any()


def test_lstm_half_equals_bptt_oracle():
    T = 7
    p, x, dy, lens, pm, Din = _small('lstm', 5, T=T, perm=True, t_mul=2, t_add=1)
    H = p['w_hh'].shape[1]
    got = R.layer('lstm', x, lens, T, pm, 2, 1, False, p['w_ih'], p['w_hh'], p['b_ih'], p['b_hh'], dy)
    X = R.gather_rows(x, pm, 2, 1, T, False)
    dX = 0
    for d, rev in enumerate((False, True)):
        g, hs = slice(d * 4 * H, (d + 1) * 4 * H), slice(d * H, (d + 1) * H)
        y, dx, dwi, dwh, db = asr_ref.lstm_direction_bptt(X, lens, p['w_ih'][g], p['w_hh'][g],
                                                          p['b_ih'][g], p['b_hh'][g], rev, dy[:, :, hs])
        dX = dX + dx
        for a, b in ((got['y'][:, :, hs], y), (got['dW_ih'][g], dwi), (got['dW_hh'][g], dwh),
                     (got['db_ih'][g], db), (got['db_hh'][g], db)):
            np.testing.assert_allclose(a.numpy(), b.numpy(), **TOL)
    np.testing.assert_allclose(got['dx'].numpy(),
                               R.scatter_rows(dX, x.shape, pm, 2, 1, T, False).numpy(), **TOL)


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_garbage_at_padded_frames_changes_nothing(kind):
    T = 7
    a = dict(perm=True, concat=True, t_mul=2, t_add=0)
    p, x, dy, lens, pm, Din = _small(kind, 9, T=T, **a)
    run = lambda xx, dd: R.layer(kind, xx, lens, T, pm, 2, 0, True, p['w_ih'], p['w_hh'], p['b_ih'],  # noqa: E731
                                 p['b_hh'], dd)
    live = torch.from_numpy(R.mapped_mask(x.shape, lens, pm, 2, 0, T, True))
    x2, dy2 = x.clone(), dy.clone()
    x2[~live] = 1e3
    for b, n in enumerate(lens):
        dy2[b, n:] = -7e2
    base, other = run(x, dy), run(x2, dy2)
    for k in R.OUT_KEYS:
        np.testing.assert_array_equal(base[k].numpy(), other[k].numpy(), err_msg=k)


def test_fp16_gate_packing_keeps_the_small_factor():
    s = torch.tensor([0.0, 1e-4, 0.3, 0.4999, 0.5, 0.7, 0.9995, 1.0 - 2.0 ** -20, 1.0])
    v, om = R.pack_sigmoid(s)
    np.testing.assert_allclose(v.numpy(), s.numpy(), rtol=0, atol=2.0 ** -11)
    np.testing.assert_allclose(om.numpy(), (1 - s.double()).float().numpy(), rtol=2.0 ** -10, atol=0)
    g = torch.tensor([0.0, 0.2, -0.499, 0.4991, -0.8, 0.9999, -1.0 + 2.0 ** -18, 1.0, -1.0])
    v, om2 = R.pack_tanh(g)
    np.testing.assert_allclose(v.numpy(), g.numpy(), rtol=0, atol=2.0 ** -11)
    want = (1 - g.double() ** 2).float().numpy()
    # 1 - |g| is clamped to 2^-15 from below, so a saturated gate keeps 1 - g^2 ~ 2^-14
    want[-3:] = np.maximum(want[-3:], 2.0 ** -15 * (2 - 2.0 ** -15))
    np.testing.assert_allclose(om2.numpy(), want, rtol=2.0 ** -9, atol=0)
    assert (torch.sign(v) == torch.sign(g)).all()


def test_bf16_emulation_rounds_the_named_operands():
    """One step (T = 1, one utterance): dW_ih = rb(dG)^T rb(x), db = sum dG."""
    g = torch.Generator().manual_seed(4)
    rb = lambda a: a.to(torch.bfloat16).to(torch.float32)     # noqa: E731
    H, D = 3, 4
    x = torch.randn(1, 1, D, generator=g)
    w_ih, w_hh = torch.randn(8 * H, D, generator=g), torch.randn(8 * H, H, generator=g)
    b = torch.zeros(8 * H)
    dy = torch.randn(1, 1, 2 * H, generator=g)
    o = R.layer('lstm', x, np.array([1]), 1, None, 1, 0, False, w_ih, w_hh, b, b, dy, None,
                R._Emu(True))
    a = rb(x[0]) @ rb(w_ih).t()
    for d in range(2):
        ai, af, ag, ao = a[0, d * 4 * H:(d + 1) * 4 * H].split(H)
        i, gg, oo = torch.sigmoid(ai), torch.tanh(ag), torch.sigmoid(ao)
        tc = torch.tanh(i * gg)
        np.testing.assert_allclose(o['y'][0, 0, d * H:(d + 1) * H].numpy(), (oo * tc).numpy(),
                                   rtol=1e-6)
    dG = o['db_ih']
    np.testing.assert_array_equal(o['dW_ih'].numpy(), torch.outer(rb(dG), rb(x[0, 0])).numpy())
    np.testing.assert_allclose(o['dx'][0, 0].numpy(), (rb(dG) @ rb(w_ih)).numpy(), rtol=1e-5,
                               atol=1e-6)
    assert not o['dW_hh'].any()            # h_prev = 0 at the only step


# --------------------------------------------------------------------------
# cases, constants
# --------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(R.CASES))
def test_case_inputs_follow_the_contract(case):
    c, inp = R.CASES[case], R.case_inputs(case)
    lens = inp['lens']
    assert lens[0] == c['T'] and (np.diff(lens) <= 0).all() and lens[-1] == 1
    assert inp['dy'].abs().min() > 0                  # a cotangent at padded frames too
    assert float(inp['w_ih'].abs().max()) <= 0.1 and float(inp['b_hh'].abs().max()) <= 0.1
    pm = np.arange(c['B']) if inp['perm'] is None else inp['perm']
    assert sorted(pm) == list(range(c['B']))
    T_src, Dsrc = R.src_dims(c)
    assert tuple(inp['x'].shape) == (c['B'], T_src, Dsrc)
    full = R.mapped_mask(inp['x'].shape, np.full(c['B'], c['T']), pm, c['t_mul'], c['t_add'], c['T'],
                         c['concat'])
    live = R.mapped_mask(inp['x'].shape, lens, pm, c['t_mul'], c['t_add'], c['T'], c['concat'])
    pad = torch.from_numpy(full & ~live)
    if c['T'] > 1:
        assert pad.any()
        assert bool(inp['x'][pad].any()) == c['garbage']
    if c['perm'] or c['concat']:
        assert (~full).any() and inp['x'][torch.from_numpy(~full)].any()   # frames no row reads


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_recorded_constants_are_reproduced_and_f32_has_room(case):
    """The recorded table is what measure_constants gives, and a correct
    float32 implementation -- this reference in float32 -- stays within a
    quarter of every fp32 bound.  How closely a constant is reproduced: a bf16
    constant is set by the bf16 roundings, the same on every CPU, to 25 % (as
    test_aux_refs_cpu.py allows); a float32 constant is the largest of a few
    thousand float32 rounding errors of sums whose order the CPU's BLAS kernel
    picks (two CPU generations gave 3.0e-7 and 6.2e-7 for one tensor), so it is
    held to the quarter-of-the-margin both ways: the float32 evaluation here
    within 4 x the recorded constant (a quarter of the bound), and the recorded
    constant within 4 x this machine's, so no bound is inflated either."""
    ref = R.reference(case)
    got = R.measure_constants(case)
    lstm = R.CASES[case]['kind'] == 'lstm'
    keys = set(R.STACK_KEYS if R.CASES[case]['stack'] else R.OUT_KEYS)
    assert set(ref) == keys
    for packed in ((False, True) if lstm else (False,)):
        cf, cb = R.case_constants(case, packed)
        mb = got['bf16p' if packed else 'bf16']
        assert set(cf) == set(cb) == keys
        print(case, 'packed' if packed else '', ' '.join('%s %.1e/%.1e' % (k, cf[k], cb[k])
                                                         for k in sorted(cf)))
        for k in keys:
            # (a single frame has no previous state: dW_hh is exactly zero, on the GPU too)
            zero = k.startswith('dW_hh') and R.CASES[case]['T'] == 1
            assert np.isfinite(ref[k]).all() and (np.abs(ref[k]).max() > 0) != zero, k
            assert R.CONST_FLOOR <= cf[k] < 1e-4 and R.CONST_FLOOR <= cb[k] < 0.1, (k, cf[k], cb[k])
            assert cf[k] / 4 <= got['f32'][k] <= 4 * cf[k], (k, got['f32'][k], cf[k])
            assert abs(mb[k] - cb[k]) <= 0.25 * cb[k], (k, mb[k], cb[k])
    f32 = R.evaluate(case, torch.float32)
    cf, _ = R.case_constants(case)
    for k in keys:
        assert R.nerr(f32[k], ref[k]) <= 0.25 * R.MARGIN * cf[k], (k, R.nerr(f32[k], ref[k]), cf[k])
    if lstm:
        assert np.array_equal(ref['db_ih'], ref['db_hh'])
    inp, c = R.case_inputs(case), R.CASES[case]
    for b, n in enumerate(inp['lens']):
        assert not ref['y'][b, n:].any()
    pm = np.arange(c['B']) if inp['perm'] is None else inp['perm']
    live = R.mapped_mask(inp['x'].shape, inp['lens'], pm, c['t_mul'], c['t_add'], c['T'], c['concat'])
    assert not ref['dx'][~live].any()


# --------------------------------------------------------------------------
# dispatch
# --------------------------------------------------------------------------
def test_expected_paths_match_the_rows_purposes():
    ep = lambda case, prec, disp='default': R.expected_path(case, prec, R.DISPATCH[disp])   # noqa: E731
    fb = lambda e: (e['fwd'], e['bwd'])                                                     # noqa: E731
    for s in ('l_b9h64', 'l_b17h96', 'l_b8h128'):
        e = ep(s, 'bf16')
        assert fb(e) == (3, 1) and e['packed'], (s, e)
    e = ep('l_b9h64', 'bf16', 'act_f32')
    assert fb(e) == (3, 1) and not e['packed']
    for s in ('l_b9h64', 'l_b17h96'):
        assert fb(ep(s, 'bf16', 'gemm_first')) == (1, 1)
    assert ep('l_b9h64', 'bf16', 'colsum')['impl'] == ('fwd_xg', 'bwd_xg_colsum')
    for s in ('l_b9h64', 'l_b8h128'):
        assert 'bwd_xg_xu32' in ep(s, 'bf16', 'xu32')['impl']
    assert 'write_through' in ep('l_b9h64', 'bf16', 'write_through')['impl']
    for s in ('l_b9h64', 'l_b20h96'):
        assert fb(ep(s, 'bf16', 'counter')) == (4, 4)
    assert ep('l_b9h64', 'bf16', 'perstep')['impl'] == ('fwd_step_fast1', 'bwd_step_fast1')
    assert ep('l_b17h96', 'bf16', 'perstep')['impl'] == ('fwd_step_fast1', 'bwd_step_fast2')
    assert ep('l_b33h160', 'bf16', 'perstep')['impl'] == ('fwd_step_fast2', 'bwd_step_fast4')
    for s in ('l_b33h40', 'l_b17h72', 'l_b18h36_perm2'):
        want = ('fwd_step_vec1', 'bwd_step_vec1') if R.CASES[s]['H'] % 8 == 0 else \
            ('fwd_step_vec0', 'bwd_step_vec0')
        assert ep(s, 'bf16')['impl'] == want and fb(ep(s, 'bf16')) == (0, 0)
    for s in ('l_b5h6', 'l_b18h36', 'l_b5h6_t1'):
        assert ep(s, 'bf16')['impl'] == ('fwd_step_vec0', 'bwd_step_vec0')
    for s in ('l_b9h64', 'l_b7h128'):
        assert fb(ep(s, 'fp32')) == (2, 2)
    for s, d in (('l_b9h64', 'xg32_off'), ('l_b33h96', 'default'), ('l_b18h36', 'default'),
                 ('l_b17h40', 'default')):
        assert fb(ep(s, 'fp32', d)) == (0, 0)
    # the option rows at (9, 64) keep the default paths; Din = 13 is staged at 16 columns
    for o in R._OPTION_CASES + ('t64', 'stack'):
        assert fb(ep('l_b9h64_' + o, 'bf16')) == (3, 1), o
    assert R.staged_width(R.CASES['l_b9h64_din13'], 'bf16') == 16
    assert ep('g_b5h6', 'bf16') is None


def test_gpu_table_reaches_every_implementation():
    assert len(set(R.GPU_TABLE)) == len(R.GPU_TABLE)
    impl, fwd, bwd = set(), set(), set()
    for case, prec, disp in R.GPU_TABLE:
        assert case in R.CASES and prec in ('fp32', 'bf16') and disp in R.DISPATCH
        assert set(R.DISPATCH[disp]) <= set(R.ENV_KEYS)
        e = R.expected_path(case, prec, R.DISPATCH[disp])
        if e is None:
            continue
        impl.update(e['impl'])
        fwd.add(e['fwd'])
        bwd.add(e['bwd'])
        # a dispatch row names a path its shape is eligible for: the switch changes something
        if disp != 'default':
            assert e != R.expected_path(case, prec, {}), (case, prec, disp)
        assert set(R.bounds(case, prec, disp)) == set(R.reference(case))
    assert impl == set(R.IMPLEMENTATIONS), set(R.IMPLEMENTATIONS) ^ impl
    # asr_lstm_last_path: the backward has no fused-projection form (3)
    assert fwd == {0, 1, 2, 3, 4} and bwd == {0, 1, 2, 4}
    gru = {(c, p) for c, p, _ in R.GPU_TABLE if R.CASES[c]['kind'] == 'gru'}
    assert len(gru) == 2 * sum(c['kind'] == 'gru' for c in R.CASES.values())
    assert any(R.CASES[c]['B'] > 32 and R.CASES[c]['H'] % 4 for c, _ in gru)
