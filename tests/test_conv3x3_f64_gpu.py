"""Every 3x3 VGG convolution path (csrc/conv.hip, the conv entry points of
csrc/cnn.hip) against the float64 numpy references of tests/conv3x3_ref.py,
through the C entry points, on real-valued operands (randn, weights x 0.1).

Bounds are derived, not measured (tests/test_conv_taps_gpu.py's):
  * a result summed in f32 from K exact products (bf16 x bf16 operands):
    |err| <= sum_bound(K, sum |terms|) = 2 K 2^-24 sum |terms|, any order;
    K = 9 Cin (forward), 9 Cout (input gradient), P pixel rows (weight gradient);
  * the f32 kernels that multiply, then add (the direct kernels, the first
    layer's stencils and its weight gradient on unrounded features) round each
    product too: 2 K roundings, sum_bound(2 K, .); a bias or a prior value of an
    accumulated buffer joins sum |terms|;
  * a bf16 output adds one round-to-nearest: b + 2^-8 (|ref| + b), b the f32
    bound (truncation, up to 2^-7, fails);
  * bf16 mode: the reference sees the bf16-rounded operands;
  * packing, padding, halo and accumulate helpers are exact (array_equal; an
    accumulation's reference is the float32 sum).
Outputs are prefilled with NaN, so an unwritten element fails.  The
tap-resident kernels write all P padded rows and are compared on all of them
against the flat-row sums (rows outside [0, P) zero): the first and last
tile's out-of-range handling is part of the result.  Each case prints
max err / bound (the table of profiles/conv3x3_f64_gpu.txt)."""
import numpy as np
import pytest
import torch

import conv3x3_ref as R

pytestmark = pytest.mark.gpu

PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128)]
PAIR_IDS = ['%dto%d' % p for p in PAIRS]
NAN = float('nan')
F32, BF16 = 0, 1
ERR_ARG = -1   # include/asr_hip.h: ASR_ERR_ARG


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _t(a, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dt).contiguous()


def _np(t):
    return t.detach().float().cpu().double().numpy()


def _bf16_bound(ref, b):
    return b + 2.0 ** -8 * (np.abs(ref) + b)


def _report(case, what, got, ref, bound, fails):
    err = np.abs(got - ref)
    ok = bool(np.isfinite(got).all()) and bool(np.all(err <= bound))
    ratio = float(np.nanmax(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print('C3X3 %-40s %-12s max err %.3e  err/bound %.3f%s' %
          (case, what, float(np.nanmax(err)), ratio, '' if ok else '  FAIL'))
    if not ok:
        fails.append((case, what))


@pytest.fixture
def bf16_mode():
    ops = _ops()
    ops.set_compute_dtype('bf16')
    yield ops
    ops.set_compute_dtype('fp32')


@pytest.fixture
def env(monkeypatch):
    names = ('ASR_CONV_TR_GRID', 'ASR_CONV_TR_WRES', 'ASR_CONV_TR_SPLITS', 'ASR_VGG_TR',
             'ASR_VGG_WGRAD_SIDE')
    for n in names:
        monkeypatch.delenv(n, raising=False)

    def set_(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return set_


# ------------------------------------------------- tap-resident forward / dgrad
def _tr_check(dev, env, Cin, Cout, B, T, F, fails, grids=(None, '1'), nw=None):
    """asr_conv3x3_tr of kernel pair Cin -> Cout at [B][T+2][F+2]: sign +1 with
    bias and sign -1 without, f32 and bf16 out, every padded row."""
    N, ops = _N(), _ops()
    Fp, P = F + 2, B * (T + 2) * (F + 2)
    pl = N.conv3x3_tr_plan(Cin, Cout, Fp)
    assert pl is not None and (nw is None or pl[1] == nw), (Cin, Cout, Fp, pl)
    rng = np.random.RandomState(Cin + 3 * Cout + 1000 * Fp + P)
    x = R.bf16_round(rng.randn(P, Cin))
    wimg = R.bf16_round(rng.randn(Cout, 9 * Cin) * 0.1)
    bias = rng.randn(Cout).astype(np.float32)
    xd, wd, bd = _t(x, dev, torch.bfloat16), _t(wimg, dev, torch.bfloat16), _t(bias, dev)
    for sign, b_np, b_d in ((1, bias, bd), (-1, None, None)):
        ref, S = R.flat_conv(x, wimg, Fp, sign, b_np)
        bound = R.sum_bound(9 * Cin, S)
        for grid in grids:
            env('ASR_CONV_TR_GRID', grid)
            for odt in (torch.float32, torch.bfloat16):
                out = torch.full((P, Cout), NAN, dtype=odt, device=dev)
                ops.conv3x3_tr(xd, P, Cin, Fp, sign, wd, Cout, b_d, out)
                torch.cuda.synchronize()
                case = '%d->%d Fp %d P %d nw %d grid %s' % (Cin, Cout, Fp, P, pl[1], grid or '-')
                what = ('fwd' if sign == 1 else 'dgrad') + (' f32' if odt == torch.float32 else ' bf16')
                _report(case, what, _np(out), ref,
                        bound if odt == torch.float32 else _bf16_bound(ref, bound), fails)
    env('ASR_CONV_TR_GRID', None)


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_tr_every_pitch_residue(Cin, Cout, cuda_dev, env):
    """Fp 3..18 (every residue mod 16), P 192..1152: several tiles and a partial
    one; the full grid and one work-group chaining every tile."""
    fails = []
    for F in range(1, 17):
        _tr_check(cuda_dev, env, Cin, Cout, 2, 30, F, fails)
    assert not fails, fails


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_tr_tile_counts(Cin, Cout, cuda_dev, env):
    """P = 9 (less than a tile), 256 (whole tiles; 257 is prime, no grid has it)
    and 258 (two rows into the next tile)."""
    fails = []
    for B, T, F in ((1, 1, 1), (1, 14, 14), (1, 4, 41)):
        assert B * (T + 2) * (F + 2) in (9, 256, 258)
        _tr_check(cuda_dev, env, Cin, Cout, B, T, F, fails)
    assert not fails, fails


def test_tr_64_64_on_the_weight_ring(cuda_dev, env):
    env('ASR_CONV_TR_WRES', '0')
    fails = []
    for F in (3, 10):
        _tr_check(cuda_dev, env, 64, 64, 2, 30, F, fails, nw=4)
    assert not fails, fails


def _segments(Cin, Cout):
    """[(nw, first Fp, last Fp)] as the plan query reports them, Fp 3..700."""
    N = _N()
    segs = []
    for fp in range(3, 701):
        pl = N.conv3x3_tr_plan(Cin, Cout, fp)
        nw = None if pl is None else pl[1]
        if segs and segs[-1][0] == nw:
            segs[-1][2] = fp
        else:
            segs.append([nw, fp, fp])
    return segs


def _assert_tr_refused(dev, bf16_ops, Cin, Cout, Fp):
    N = _N()
    P = 3 * Fp
    assert N.query('asr_conv3x3_tr_supported', Cin, Cout, Fp) == 0
    assert not bf16_ops._conv_tr_ok(Cin, Cout, Fp, P, 4)
    x = torch.zeros(P, Cin, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(Cout, 9 * Cin, dtype=torch.bfloat16, device=dev)
    out = torch.full((P, Cout), NAN, device=dev)
    rc = N.lib().asr_conv3x3_tr(N.ptr(x), P, Cin, Fp, 1, N.ptr(w), Cout, None, N.ptr(out), F32,
                                N.stream_handle(dev))
    torch.cuda.synchronize()
    assert rc == N.ASR_ERR_UNSUPPORTED and N.lib().asr_last_error()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_tr_plan_boundaries(Cin, Cout, cuda_dev, env, bf16_mode):
    """B 1, T 1 (P = 3 Fp): the last pitch of every plan segment and the first of
    the next; where the plan refuses (the pitches past the last kernel: 249,
    249, 121, 89) VGGFn's switch is off and the launch returns
    ASR_ERR_UNSUPPORTED with nothing written; one pitch above a tile's rows."""
    segs = _segments(Cin, Cout)
    assert segs[-1][0] is None and segs[-1][2] == 700 and all(s[0] is not None for s in segs[:-1])
    fails, ran = [], []
    for nw, lo, hi in segs:
        for fp in sorted({lo, hi}):
            if nw is None:
                if fp == lo:
                    _assert_tr_refused(cuda_dev, bf16_mode, Cin, Cout, fp)
                continue
            if fp >= 19:      # (3..18: test_tr_every_pitch_residue)
                assert bf16_mode._conv_tr_ok(Cin, Cout, fp, 3 * fp, 4)
                _tr_check(cuda_dev, env, Cin, Cout, 1, 1, fp - 2, fails, nw=nw)
                ran.append((fp, nw))
    bm = 4 * _N().conv3x3_tr_plan(Cin, Cout, 3)[0]
    if segs[-1][1] - 1 > bm + 3:
        _tr_check(cuda_dev, env, Cin, Cout, 1, 1, bm + 3 - 2, fails)
        ran.append((bm + 3, None))
    want = {(64, 64): [(88, 0), (89, 4), (248, 4)], (64, 128): [(248, 4), (131, None)],
            (128, 64): [(120, 4)], (128, 128): [(56, 4), (57, 3), (88, 3)]}[(Cin, Cout)]
    assert ran == want, ran
    assert not fails, fails


# ------------------------------------------------ tap-resident weight gradient
def _trw_check(dev, env, ops, Cin, Cout, B, T, F, fails, splits=(None, '1', '3')):
    N = _N()
    Fp, P = F + 2, B * (T + 2) * (F + 2)
    assert N.conv3x3_tr_wgrad_plan(Cin, Cout, Fp) is not None
    rng = np.random.RandomState(5 * Cin + Cout + 1000 * Fp + P)
    x, dz = R.bf16_round(rng.randn(P, Cin)), R.bf16_round(rng.randn(P, Cout))
    dw0 = rng.randn(Cout, Cin, 3, 3).astype(np.float32)
    ref, S = R.flat_wgrad(x, dz, Fp)
    bound = R.sum_bound(P, S)
    xd, dzd = _t(x, dev, torch.bfloat16), _t(dz, dev, torch.bfloat16)
    for sp in splits:
        env('ASR_CONV_TR_SPLITS', sp)
        runs = []
        for _ in range(2):
            packed = torch.full((Cout, 9 * Cin), NAN, device=dev)
            assert ops.conv3x3_tr_wgrad(xd, dzd, P, Cin, Fp, Cout, packed)
            dw = _t(dw0, dev)
            N.call('asr_conv_weight_unpack_acc', N.ptr(packed), Cout, Cin, N.ptr(dw),
                   N.stream_handle(dev))
            torch.cuda.synchronize()
            runs.append((packed.cpu().numpy(), dw.cpu().numpy()))
        case = 'wgrad %d->%d Fp %d P %d splits %s' % (Cin, Cout, Fp, P, sp or '-')
        _report(case, 'image', runs[0][0].astype(np.float64), ref, bound, fails)
        if not (np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])):
            fails.append((case, 'two runs differ'))
        if np.isfinite(runs[0][0]).all():   # dw0 + image in float32, exactly
            np.testing.assert_array_equal(runs[0][1], dw0 + R.unpack_image(runs[0][0], Cin))
    env('ASR_CONV_TR_SPLITS', None)


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_trw_every_pitch_residue(Cin, Cout, cuda_dev, env, bf16_mode):
    """Fp 3..18, P up to 1872: the default split count, one chunk, and at most
    three (cuts at multiples of 8 that are no multiples of the 64-pixel k-tile)."""
    fails = []
    for F in range(1, 17):
        _trw_check(cuda_dev, env, bf16_mode, Cin, Cout, 2, 50, F, fails)
    assert not fails, fails


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_trw_short_chunks(Cin, Cout, cuda_dev, env, bf16_mode):
    """P = 9 (a chunk shorter than one k-tile, S = 1) and P = 64 exactly."""
    fails = []
    for B, T, F in ((1, 1, 1), (1, 6, 6)):
        assert B * (T + 2) * (F + 2) in (9, 64)
        _trw_check(cuda_dev, env, bf16_mode, Cin, Cout, B, T, F, fails, splits=(None,))
    assert not fails, fails


@pytest.mark.parametrize('Cin,Cout', PAIRS, ids=PAIR_IDS)
def test_trw_plan_limits(Cin, Cout, cuda_dev, env, bf16_mode):
    """The last pitch the LDS ring takes (Cin 64: 376, Cin 128: 120), and one
    beyond it: False, nothing written."""
    last = {64: 376, 128: 120}[Cin]
    fails = []
    _trw_check(cuda_dev, env, bf16_mode, Cin, Cout, 1, 1, last - 2, fails, splits=(None,))
    assert not fails, fails
    Fp = last + 1
    P = 3 * Fp
    assert _N().conv3x3_tr_wgrad_plan(Cin, Cout, Fp) is None
    x = torch.zeros(P, Cin, dtype=torch.bfloat16, device=cuda_dev)
    dz = torch.zeros(P, Cout, dtype=torch.bfloat16, device=cuda_dev)
    packed = torch.full((Cout, 9 * Cin), NAN, device=cuda_dev)
    assert bf16_mode.conv3x3_tr_wgrad(x, dz, P, Cin, Fp, Cout, packed) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(packed).all())


# --------------------------------------------------------- first-layer stencils
C1_T, C1_F = (1, 4, 5, 7), (1, 7, 33)


def _c1_inputs(Co, B, T, F):
    rng = np.random.RandomState(Co + 10 * T + F)
    xs = rng.randn(B, T, F).astype(np.float32)
    w = (rng.randn(Co, 1, 3, 3) * 0.1).astype(np.float32)
    bias = rng.randn(Co).astype(np.float32)
    return rng, xs, w, bias


def _nchw1(xs):   # [B][T][F] -> [B][1][F][T]
    return np.asarray(xs, np.float64).transpose(0, 2, 1)[:, None]


def _c1_ref(xs, w, bias):
    """(z [B][Co][F][T], bound): nine products and nine adds per element, all rounded."""
    z, S = R.conv_forward(_nchw1(xs), w, bias)
    return z, R.sum_bound(2 * 9, S + np.abs(np.asarray(bias, np.float64))[None, :, None, None])


def _z_buffer(B, T, F, Co, dt, dev):
    """[B][T+2][F+2][Co]: NaN inside, 7 on the halo (which no stencil may touch)."""
    z = torch.full((B, T + 2, F + 2, Co), 7.0, dtype=dt, device=dev)
    z[:, 1:T + 1, 1:F + 1] = NAN
    return z


def _halo_kept(z, B, T, F):
    return bool(np.all(_np(z)[R.halo_mask(B, T, F)] == 7.0))


def _c1_forward(dev, xs, w, bias, dt, cstride, rng):
    """asr_conv3x3_c1_forward on the padded operand (channel 0 = xs, the other
    cstride - 1 channels junk the kernel must not read into the sum)."""
    N = _N()
    B, T, F = xs.shape
    Co = w.shape[0]
    xp = rng.randn(B, T + 2, F + 2, cstride).astype(np.float32) * 100
    xp[..., 0] = R.pad_input(xs, 1)[..., 0]
    xpd = _t(xp, dev, dt)
    z = _z_buffer(B, T, F, Co, torch.float32, dev)
    wd, bd = _t(w, dev), _t(bias, dev)
    N.call('asr_conv3x3_c1_forward', N.ptr(xpd), BF16 if dt == torch.bfloat16 else F32, cstride,
           B, T, F, Co, N.ptr(wd), N.ptr(bd), N.ptr(z), N.stream_handle(dev))
    torch.cuda.synchronize()
    return z


@pytest.mark.parametrize('Co', [16, 64, 128])
def test_c1_forward(Co, cuda_dev):
    fails = []
    for T in C1_T:
        for F in C1_F:
            rng, xs, w, bias = _c1_inputs(Co, 2, T, F)
            for dt, cs in ((torch.float32, 1), (torch.bfloat16, 16)):
                xr = xs if dt == torch.float32 else R.bf16_round(xs)
                ref, bound = _c1_ref(xr, w, bias)
                z = _c1_forward(cuda_dev, xs, w, bias, dt, cs, rng)
                case = 'c1_forward Co %d T %d F %d %s' % (Co, T, F, 'f32' if cs == 1 else 'bf16x16')
                _report(case, 'z f32', R.from_haloed(_np(z)), ref, bound, fails)
                if not _halo_kept(z, 2, T, F):
                    fails.append((case, 'halo written'))
    assert not fails, fails


@pytest.mark.parametrize('Co', [16, 64, 128])
def test_c1_forward_xs(Co, cuda_dev):
    """From the raw features, C1_FT = 4 frames per work-group (T 1, 4, 5, 7);
    with rounding on and f32 z: the bits of asr_conv3x3_c1_forward on the
    padded bf16 operand."""
    N = _N()
    fails = []
    for T in C1_T:
        for F in C1_F:
            rng, xs, w, bias = _c1_inputs(Co, 2, T, F)
            xsd, wd, bd = _t(xs, cuda_dev), _t(w, cuda_dev), _t(bias, cuda_dev)
            for rb in (0, 1):
                ref, bound = _c1_ref(R.bf16_round(xs) if rb else xs, w, bias)
                for zdt in (torch.float32, torch.bfloat16):
                    z = _z_buffer(2, T, F, Co, zdt, cuda_dev)
                    N.call('asr_conv3x3_c1_forward_xs', N.ptr(xsd), rb, 2, T, F, Co, N.ptr(wd),
                           N.ptr(bd), N.ptr(z), BF16 if zdt == torch.bfloat16 else F32,
                           N.stream_handle(cuda_dev))
                    torch.cuda.synchronize()
                    f32 = zdt == torch.float32
                    case = 'c1_forward_xs Co %d T %d F %d round %d' % (Co, T, F, rb)
                    _report(case, 'z f32' if f32 else 'z bf16', R.from_haloed(_np(z)), ref,
                            bound if f32 else _bf16_bound(ref, bound), fails)
                    if not _halo_kept(z, 2, T, F):
                        fails.append((case, 'halo written'))
                    if rb and f32:
                        z1 = _c1_forward(cuda_dev, xs, w, bias, torch.bfloat16, 16, rng)
                        if not np.array_equal(R.from_haloed(_np(z)), R.from_haloed(_np(z1))):
                            fails.append((case, 'differs from c1_forward'))
    assert not fails, fails


def _c1_wgrad(dev, xs, dz, rb, Cip=16):
    N = _N()
    B, T, F = xs.shape
    Co = dz.shape[1]
    packed = torch.full((Co, 9 * Cip), NAN, device=dev)
    nb = N.query('asr_conv3x3_c1_wgrad_workspace_bytes', Co)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xsd, dzd = _t(xs, dev), _t(dz, dev, torch.bfloat16)
    rc = N.lib().asr_conv3x3_c1_wgrad_xs(N.ptr(xsd), rb, B, T, F, Co, N.ptr(dzd), Cip,
                                         N.ptr(packed), N.ptr(ws), nb, N.stream_handle(dev))
    torch.cuda.synchronize()
    return rc, packed.cpu().numpy()


@pytest.mark.parametrize('B,T,F', [(3, 40, 15), (1, 1, 1)])
def test_c1_wgrad_xs(B, T, F, cuda_dev):
    """P = 2142: two chunks, 256-pixel tiles crossing utterance boundaries; P = 9.
    Rounded features: exact products, P roundings; raw f32 features: 2 P."""
    Co, Cip, Fp = 64, 16, F + 2
    P = B * (T + 2) * Fp
    rng = np.random.RandomState(P)
    xs = rng.randn(B, T, F).astype(np.float32)
    dz = R.bf16_round(rng.randn(P, Co))
    fails = []
    for rb in (0, 1):
        xp = R.pad_input(R.bf16_round(xs) if rb else xs.astype(np.float64), 1).reshape(P, 1)
        ref, S = R.flat_wgrad(xp, dz, Fp)              # [Co][9]
        bound = R.sum_bound(P if rb else 2 * P, S)
        rc, packed = _c1_wgrad(cuda_dev, xs, dz, rb)
        assert rc == 0
        rc2, packed2 = _c1_wgrad(cuda_dev, xs, dz, rb)
        img = packed.reshape(Co, 9, Cip)
        case = 'c1_wgrad_xs P %d round %d' % (P, rb)
        _report(case, 'image', img[:, :, 0].astype(np.float64), ref, bound, fails)
        assert np.array_equal(img[:, :, 1:], np.zeros((Co, 9, Cip - 1), np.float32)), case
        assert np.array_equal(packed, packed2), case
    assert not fails, fails


def test_c1_wgrad_xs_refuses_a_row_beyond_its_lds(cuda_dev):
    """256 x 64 x 2 + (256 + 2 (F + 3)) x 4 <= 64 KB holds to F = 3965."""
    N = _N()
    for F, ok in ((3965, True), (3966, False)):
        rng = np.random.RandomState(F)
        P = 3 * (F + 2)
        rc, packed = _c1_wgrad(cuda_dev, rng.randn(1, 1, F).astype(np.float32),
                               R.bf16_round(rng.randn(P, 64)), 1)
        if ok:
            assert rc == 0 and np.isfinite(packed).all()
        else:
            assert rc == N.ASR_ERR_UNSUPPORTED and np.isnan(packed).all()


# ---------------------------------------------------------- direct fp32 kernels
@pytest.mark.parametrize('B,T,F', [(2, 6, 5), (1, 1, 1)])
@pytest.mark.parametrize('Ci,Co', [(1, 7), (3, 5), (5, 16)])
def test_direct_kernels(Ci, Co, B, T, F, cuda_dev):
    """asr_conv_direct_forward / _dgrad / _wgrad, f32 operands: K products and K
    adds per sum.  The outputs' halo rows stay as they were; the weight and
    bias gradients are ADDED to the buffers (asr_vgg_accumulate)."""
    N, dev = _N(), cuda_dev
    st = N.stream_handle(dev)
    rng = np.random.RandomState(100 * Ci + Co + T)
    x = rng.randn(B, Ci, F, T).astype(np.float32)
    w = (rng.randn(Co, Ci, 3, 3) * 0.1).astype(np.float32)
    bias = rng.randn(Co).astype(np.float32)
    dz = rng.randn(B, Co, F, T).astype(np.float32)
    xh, dzh, wd, bd = _t(R.to_haloed(x), dev), _t(R.to_haloed(dz), dev), _t(w, dev), _t(bias, dev)
    P = B * (T + 2) * (F + 2)
    fails = []
    case = 'direct %d->%d B %d T %d F %d' % (Ci, Co, B, T, F)
    for b_np in (bias, None):
        ref, S = R.conv_forward(x, w, b_np)
        if b_np is not None:
            S = S + np.abs(bias.astype(np.float64))[None, :, None, None]
        z = _z_buffer(B, T, F, Co, torch.float32, dev)
        N.call('asr_conv_direct_forward', N.ptr(xh), B, T, F, Ci, Co, N.ptr(wd),
               N.ptr(bd) if b_np is not None else None, N.ptr(z), st)
        torch.cuda.synchronize()
        _report(case, 'fwd' + (' +bias' if b_np is not None else ''), R.from_haloed(_np(z)), ref,
                R.sum_bound(2 * 9 * Ci, S), fails)
        assert _halo_kept(z, B, T, F), case
    ref, S = R.conv_dgrad(dz, w, F, T)
    dx = _z_buffer(B, T, F, Ci, torch.float32, dev)
    N.call('asr_conv_direct_dgrad', N.ptr(dzh), B, T, F, Ci, Co, N.ptr(wd), N.ptr(dx), st)
    torch.cuda.synchronize()
    _report(case, 'dgrad', R.from_haloed(_np(dx)), ref, R.sum_bound(2 * 9 * Co, S), fails)
    assert _halo_kept(dx, B, T, F), case
    # weight / bias gradient into non-zero buffers: dw0 + sum, db0 + sum dz
    dw0 = rng.randn(Co, Ci, 3, 3).astype(np.float32)
    db0 = rng.randn(Co).astype(np.float32)
    ref, S = R.conv_wgrad(x, dz, 3, 3)
    dw, db = _t(dw0, dev), _t(db0, dev)
    nb = N.query('asr_conv_direct_wgrad_workspace_bytes', B, T, F, Ci, Co)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    N.call('asr_conv_direct_wgrad', N.ptr(xh), N.ptr(dzh), B, T, F, Ci, Co, N.ptr(dw), N.ptr(db),
           N.ptr(ws), nb, st)
    torch.cuda.synchronize()
    _report(case, 'wgrad', _np(dw), dw0 + ref, R.sum_bound(2 * P, S + np.abs(dw0)), fails)
    _report(case, 'bias grad', _np(db), db0 + dz.astype(np.float64).sum((0, 2, 3)),
            R.sum_bound(2 * P, np.abs(dz.astype(np.float64)).sum((0, 2, 3)) + np.abs(db0)), fails)
    assert not fails, fails


# ------------------------------------------------------------------ helpers, exact
@pytest.mark.parametrize('B,T,F', [(2, 5, 7), (1, 1, 1), (3, 1, 4)])
def test_pad_input(B, T, F, cuda_dev):
    N, dev = _N(), cuda_dev
    xs = np.random.RandomState(T + F).randn(B, T, F).astype(np.float32)
    xsd = _t(xs, dev)
    out = torch.full((B, T + 2, F + 2, 1), NAN, device=dev)
    N.call('asr_vgg_pad_input', N.ptr(xsd), B, T, F, N.ptr(out), N.stream_handle(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), R.pad_input(xs, 1))
    for Cp in (1, 16):
        for dt, code in ((torch.float32, F32), (torch.bfloat16, BF16)):
            out = torch.full((B, T + 2, F + 2, Cp), NAN, dtype=dt, device=dev)
            N.call('asr_vgg_pad_input_ch', N.ptr(xsd), B, T, F, Cp, code, N.ptr(out),
                   N.stream_handle(dev))
            torch.cuda.synchronize()
            want = R.pad_input(xs if code == F32 else R.bf16_round(xs), Cp)
            np.testing.assert_array_equal(_np(out), want.astype(np.float64))


@pytest.mark.parametrize('dt,C', [(torch.float32, 4), (torch.bfloat16, 8), (torch.bfloat16, 64)],
                         ids=['f32_C4', 'bf16_C8', 'bf16_C64'])
def test_zero_halo(dt, C, cuda_dev):
    N, dev = _N(), cuda_dev
    for B, T, F in ((1, 1, 1), (2, 3, 5), (3, 1, 4), (2, 6, 1), (5, 9, 11)):
        buf = torch.full((B, T + 2, F + 2, C), 7.0, dtype=dt, device=dev)
        N.call('asr_vgg_zero_halo', N.ptr(buf), BF16 if dt == torch.bfloat16 else F32, B, T, F, C,
               N.stream_handle(dev))
        torch.cuda.synchronize()
        want = np.where(R.halo_mask(B, T, F)[..., None], 0.0, 7.0) * np.ones(C)
        np.testing.assert_array_equal(_np(buf), want)


def test_zero_halo_refuses_rows_that_are_not_16_bytes(cuda_dev):
    N = _N()
    for dt, code, C in ((torch.float32, F32, 2), (torch.bfloat16, BF16, 4), (torch.float32, F32, 5)):
        buf = torch.full((2, 5, 6, C), 7.0, dtype=dt, device=cuda_dev)
        rc = N.lib().asr_vgg_zero_halo(N.ptr(buf), code, 2, 3, 4, C, N.stream_handle(cuda_dev))
        torch.cuda.synchronize()
        assert rc == ERR_ARG and bool((buf == 7.0).all())


@pytest.mark.parametrize('Co,Ci,Cip', [(5, 3, 3), (64, 1, 16), (16, 7, 16), (128, 64, 64)])
def test_weight_pack(Co, Ci, Cip, cuda_dev):
    """Modes 0 and 1, f32 and bf16 images; padded channels (Cip > Ci, mode 0
    only) keep what the caller put there."""
    N, dev = _N(), cuda_dev
    st = N.stream_handle(dev)
    w = np.random.RandomState(Co + Ci).randn(Co, Ci, 3, 3).astype(np.float32)
    wd = _t(w, dev)
    for dt, code in ((torch.float32, F32), (torch.bfloat16, BF16)):
        wr = w.astype(np.float64) if code == F32 else R.bf16_round(w)
        out = torch.full((Co, 9 * Cip), 7.0, dtype=dt, device=dev)
        N.call('asr_conv_weight_pack_pad', N.ptr(wd), Co, Ci, Cip, 0, code, N.ptr(out), st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(out), R.pack_image(wr, Cip, 0, fill=7.0))
        out = torch.full((Ci, 9 * Co), NAN, dtype=dt, device=dev)
        if Cip == Ci:
            N.call('asr_conv_weight_pack_pad', N.ptr(wd), Co, Ci, Cip, 1, code, N.ptr(out), st)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_np(out), R.pack_image(wr, mode=1))
            for mode in (0, 1):
                o2 = torch.full((Co, 9 * Ci) if mode == 0 else (Ci, 9 * Co), NAN, dtype=dt,
                                device=dev)
                N.call('asr_conv_weight_pack', N.ptr(wd), Co, Ci, mode, code, N.ptr(o2), st)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(_np(o2), R.pack_image(wr, mode=mode))
        else:   # a padded transposed image does not exist
            rc = N.lib().asr_conv_weight_pack_pad(N.ptr(wd), Co, Ci, Cip, 1, code, N.ptr(out), st)
            torch.cuda.synchronize()
            assert rc == ERR_ARG and bool(torch.isnan(out).all())


@pytest.mark.parametrize('Co,Ci,Cip', [(5, 3, 3), (64, 1, 16), (16, 7, 16), (128, 64, 64)])
def test_weight_unpack_accumulate(Co, Ci, Cip, cuda_dev):
    """dw += image, for the three entry points, into a non-zero dw: the float32 sum."""
    N, dev = _N(), cuda_dev
    st = N.stream_handle(dev)
    rng = np.random.RandomState(Co * Ci + Cip)
    img = rng.randn(Co, 9 * Cip).astype(np.float32)
    dw0 = rng.randn(Co, Ci, 3, 3).astype(np.float32)
    want = dw0 + R.unpack_image(img, Ci)
    dw, imgd = _t(dw0, dev), _t(img, dev)
    N.call('asr_conv_weight_unpack_acc_pad', N.ptr(imgd), Co, Ci, Cip, N.ptr(dw), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dw.cpu().numpy(), want)
    dw = _t(dw0, dev)
    img_t = np.ascontiguousarray(img.T)
    imgtd = _t(img_t, dev)
    N.call('asr_conv_weight_unpack_acc_pad_t', N.ptr(imgtd), Co, Ci, Cip, N.ptr(dw), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dw.cpu().numpy(), dw0 + R.unpack_image_t(img_t, Ci))
    np.testing.assert_array_equal(dw.cpu().numpy(), want)
    if Cip == Ci:
        dw = _t(dw0, dev)
        N.call('asr_conv_weight_unpack_acc', N.ptr(imgd), Co, Ci, N.ptr(dw), st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dw.cpu().numpy(), want)


@pytest.mark.parametrize('n,n2', [(1000, 0), (257, 1), (1, 513)])
def test_vgg_accumulate(n, n2, cuda_dev):
    N, dev = _N(), cuda_dev
    rng = np.random.RandomState(n + n2)
    a, d = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    a2, d2 = rng.randn(max(n2, 1)).astype(np.float32), rng.randn(max(n2, 1)).astype(np.float32)
    dd, dd2, ad, a2d = _t(d, dev), _t(d2, dev), _t(a, dev), _t(a2, dev)
    N.call('asr_vgg_accumulate', N.ptr(ad), N.ptr(dd), n, N.ptr(a2d) if n2 else None,
           N.ptr(dd2) if n2 else None, n2, N.stream_handle(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dd.cpu().numpy(), d + a)
    want2 = d2.copy()
    want2[:n2] += a2[:n2]
    np.testing.assert_array_equal(dd2.cpu().numpy(), want2)


# ------------------------------------------------------------- the hole, end to end
@pytest.mark.parametrize('tr', [None, '0'], ids=['tr_default', 'tr0'])
def test_vgg_120_bins_unpooled_64_128_backward(tr, cuda_dev, env, bf16_mode):
    """VGGFn, bf16 mode, conv_channels [64, 128], no pooling, no batch norm, a
    120-bin plane (Fp = 122), B 1, T 3.  The input gradient of the 64 -> 128
    layer is the 128 -> 64 kernel at Fp 122, a pitch whose plan named a kernel
    that does not exist: the backward raised.  Now the plan refuses and VGGFn
    takes the tap GEMM; forward and backward complete, with ASR_VGG_TR=0 too.

    Checked per layer call on the run's own saved operands (no batch norm, so no
    cancellation): the second layer's weight gradient is the flat weight-
    gradient sum of its saved bf16 input and dz2 = dout where z2 > 0 (dout is
    bf16-exact), within sum_bound(P, .); the first layer's is the same sum over
    dz1 = dx1 where z1 > 0, dx1 the bf16 input gradient, whose reference error
    e = b + 2^-8 (|dx1| + b) is carried through the sum:
    sum_bound(P, S + E) + E, E = sum_p e |x|."""
    ops, dev = bf16_mode, cuda_dev
    env('ASR_VGG_TR', tr)
    # weight gradients on the compute stream: this test must not be the one that
    # creates the process's VGG side stream (streams share the hardware queues in
    # creation order, and the recurrence tests that run later in the same process
    # depend on which queues their own side streams get)
    env('ASR_VGG_WGRAD_SIDE', '0')
    assert not ops._conv_tr_ok(128, 64, 122, 610, 2)
    B, T, F = 1, 3, 120
    Fp, P = F + 2, B * (T + 2) * (F + 2)
    rng = np.random.RandomState(122)
    xs = rng.randn(B, T, F).astype(np.float32)
    ws = [(rng.randn(64, 1, 3, 3) * 0.1).astype(np.float32),
          (rng.randn(128, 64, 3, 3) * 0.1).astype(np.float32)]
    prm = [(torch.nn.Parameter(_t(w, dev)),
            torch.nn.Parameter(_t(rng.randn(w.shape[0]).astype(np.float32) * 0.1, dev))) for w in ws]
    specs = [dict(w=w, b=b, pt=0, pf=0, ceil=0, gamma=None, beta=None, run_mean=None,
                  run_var=None, momentum=0.1, eps=1e-5) for w, b in prm]
    out = ops.vgg_front(_t(xs, dev), specs, True, 0.0)
    assert tuple(out.shape) == (B, T, F * 128)
    dout = R.bf16_round(rng.randn(B, T, F, 128))
    saved = out.grad_fn.saved_tensors
    x2, z1, z2 = _np(saved[6]), _np(saved[1]), _np(saved[7])
    out.backward(_t(dout.reshape(B, T, F * 128), dev))
    torch.cuda.synchronize()
    g = [(_np(w.grad), _np(b.grad)) for w, b in prm]
    assert all(np.isfinite(a).all() for pair in g for a in pair) and np.isfinite(_np(out)).all()
    inner = ~R.halo_mask(B, T, F).reshape(P)
    fails = []
    # layer 2: weight gradient from its saved operands
    dz2 = np.zeros((P, 128))
    dz2[inner] = dout.reshape(-1, 128) * (z2[inner] > 0)
    ref, S = R.flat_wgrad(x2, dz2, Fp)
    case = 'vgg 64->128 F 120 TR %s' % (tr or '-')
    _report(case, 'dW layer 2', g[1][0], R.unpack_image(ref, 64),
            R.unpack_image(R.sum_bound(P, S), 64), fails)
    # layer 1: dx1 = bf16 input gradient of layer 2, masked by z1 > 0
    wt2 = R.bf16_round(R.pack_image(ws[1], mode=1))
    dx1, Sd = R.flat_conv(dz2, wt2, Fp, -1)
    e = _bf16_bound(dx1, R.sum_bound(9 * 128, Sd))
    m1 = inner[:, None] & (z1 > 0)
    xp = R.pad_input(R.bf16_round(xs), 1).reshape(P, 1)
    ref, S = R.flat_wgrad(xp, dx1 * m1, Fp)
    E, _ = R.flat_wgrad(np.abs(xp), e * m1, Fp)
    _report(case, 'dW layer 1', g[0][0], R.unpack_image(ref, 1),
            R.unpack_image(R.sum_bound(P, S + E) + E, 1), fails)
    assert not fails, fails
