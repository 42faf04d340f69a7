"""The kf x kt convolution kernels of csrc/conv_taps.hip (forward, input
gradient, weight-gradient image; kf, kt in {3, 5}) against the float64 numpy
reference tests/cnn_taps_ref.py, through the C entry points, in both precision
modes: bf16 mode against the reference evaluated on the bf16-rounded operands,
fp32 mode against the reference on the raw operands.

The bound is derived, not measured.  The products of bf16 (or f32-mode f32)
operands are exact in the f32 accumulator's inputs; only the f32 summation
differs from the reference, so every element must satisfy
    |err| <= 2 K 2^-24 sum |terms|
(the standard bound gamma_K sum |terms| for any summation order, with
gamma_K = K u / (1 - K u) <= 2 K u, u = 2^-24), K = the number of terms of one
sum: kf kt Cin for the forward, kf kt Cout for the input gradient (the same
convolution over dz, whose input channels are the layer's Cout), and the
number of output pixels B To Fo for the weight gradient.  The f32 mode forms
each term with a fused multiply-add, so its products are not rounded either.

Shapes: T = 11, F = 7 (output rows of 7, 5 or 3 pixels: a 64-pixel strip
crosses rows and ends in a partial strip, more than one strip per utterance),
every kernel shape, Cin / Cout of one and two 16-blocks; the recipe's 128 and
256 channels (several channel chunks, both 128-column groups) on a small grid;
T = 3 with kt = 5, a single output time row.
"""
import numpy as np
import pytest
import torch

import cnn_taps_ref as R

BF16, F32 = 1, 0

CASES = ([(2, 11, 7, kf, kt, ci, co) for (kf, kt) in ((3, 5), (5, 3), (5, 5), (3, 3))
          for (ci, co) in ((16, 32), (32, 16))] +
         [(2, 7, 4, 3, 5, 128, 256), (2, 7, 4, 3, 5, 256, 256), (2, 3, 7, 3, 5, 16, 32)])


def _N():
    from pytorch_end2end_speech_recognition_amd import _native as N
    return N


def _inputs(B, T, F, kf, kt, ci, co):
    rng = np.random.RandomState(1000 * kf + 100 * kt + ci + co + T)
    x = rng.randn(B, ci, F, T).astype(np.float32)
    w = (rng.randn(co, ci, kf, kt) * 0.2).astype(np.float32)
    dz = rng.randn(B, co, F + 3 - kf, T + 3 - kt).astype(np.float32)
    return x, w, dz


def _run(mode, dev, B, T, F, kf, kt, ci, co, x, w, dz, runs=1):
    """forward, input gradient and `runs` weight gradients of one layer through the
    C entry points; returns NCHW float64 arrays (z, dx, [dw ...]) and the raw z."""
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    N = _N()
    dt = torch.bfloat16 if mode == BF16 else torch.float32
    To, Fo = T + 3 - kt, F + 3 - kf
    xh = torch.from_numpy(R.to_haloed(x)).to(dev).to(dt).contiguous()
    dzh = torch.from_numpy(R.to_haloed(dz)).to(dev).to(dt).contiguous()
    wd = torch.from_numpy(w).to(dev)
    assert N.query('asr_conv_taps_supported', mode, B, T, F, ci, co, kf, kt) == 1, \
        N.lib().asr_last_error()
    wg = ops.conv_taps_weight_pack(wd, ci, 0, mode)
    wt = ops.conv_taps_weight_pack(wd, ci, 1, mode)
    z = torch.zeros(B, To + 2, Fo + 2, co, device=dev)
    z[:, 1:-1, 1:-1] = float('nan')
    ops.conv_taps_forward(xh, B, T, F, ci, wg, co, kf, kt, None, z, mode)
    dx = torch.zeros(B, T + 2, F + 2, ci, device=dev)
    dx[:, 1:-1, 1:-1] = float('nan')
    ops.conv_taps_dgrad(dzh, B, T, F, ci, wt, co, kf, kt, dx, mode)
    dws = []
    for _ in range(runs):
        packed = torch.full((co, kf * kt * ci), float('nan'), device=dev)
        ops.conv_taps_wgrad(xh, dzh, B, T, F, ci, co, kf, kt, packed, mode)
        dw = torch.zeros(co, ci, kf, kt, device=dev)
        N.call('asr_conv_taps_weight_unpack_acc', N.ptr(packed), co, ci, ci, kf, kt, N.ptr(dw),
               N.stream_handle(dev))
        dws.append(dw.cpu().double().numpy())
    torch.cuda.synchronize()
    zc, dxc = z.cpu().double().numpy(), dx.cpu().double().numpy()
    return zc, dxc, dws


def _halo_zero(a):
    a = a.copy()
    a[:, 1:-1, 1:-1] = 0
    return not np.any(a != 0)


def _within(what, got, ref, bound, fails):
    err = np.abs(got - ref)
    ok = np.isfinite(got).all() and bool(np.all(err <= bound))
    print('  %-10s max err %.3e, max err/bound %.3f' %
          (what, float(np.nanmax(err)), float(np.nanmax(err / np.maximum(bound, 1e-300)))))
    if not ok:
        fails.append(what)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('B,T,F,kf,kt,ci,co', CASES)
def test_conv_taps_vs_float64(B, T, F, kf, kt, ci, co, mode, cuda_dev):
    x, w, dz = _inputs(B, T, F, kf, kt, ci, co)
    if mode == BF16:   # the reference sees the operands the kernel sees
        xr, wr, dzr = R.bf16_round(x), R.bf16_round(w), R.bf16_round(dz)
    else:
        xr, wr, dzr = x, w, dz
    z, dx, dws = _run(mode, cuda_dev, B, T, F, kf, kt, ci, co, x, w, dz, runs=2)
    z_ref, z_S = R.conv_forward(xr, wr)
    dx_ref, dx_S = R.conv_dgrad(dzr, wr, F, T)
    dw_ref, dw_S = R.conv_wgrad(xr, dzr, kf, kt)
    To, Fo = T + 3 - kt, F + 3 - kf
    fails = []
    _within('forward', R.from_haloed(z), z_ref, R.sum_bound(kf * kt * ci, z_S), fails)
    _within('dgrad', R.from_haloed(dx), dx_ref, R.sum_bound(kf * kt * co, dx_S), fails)
    _within('wgrad', dws[0], dw_ref, R.sum_bound(B * To * Fo, dw_S), fails)
    assert not fails, fails
    assert _halo_zero(z) and _halo_zero(dx), 'a kernel wrote outside its output interior'
    assert np.array_equal(dws[0], dws[1]), 'two weight-gradient runs differ'


@pytest.mark.gpu
def test_conv_taps_3x3_agrees_with_conv3x3_tr(cuda_dev):
    """Where both kernels take the shape (bf16, 64 -> 64 channels, 3x3) the new
    kernel and asr_conv3x3_tr agree within the forward bound above: both sum the
    same exact products in f32, in different orders."""
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    N = _N()
    B, T, F, ci, co = 2, 11, 7, 64, 64
    x, w, dz = _inputs(B, T, F, 3, 3, ci, co)
    assert N.query('asr_conv3x3_tr_supported', ci, co, F + 2) == 1
    z, _, _ = _run(BF16, cuda_dev, B, T, F, 3, 3, ci, co, x, w, dz)
    xh = torch.from_numpy(R.to_haloed(x)).to(cuda_dev).to(torch.bfloat16).contiguous()
    wd = torch.from_numpy(w).to(cuda_dev)
    wg = torch.empty(co, 9 * ci, dtype=torch.bfloat16, device=cuda_dev)
    N.call('asr_conv_weight_pack', N.ptr(wd), co, ci, 0, BF16, N.ptr(wg),
           N.stream_handle(cuda_dev))
    npad = B * (T + 2) * (F + 2)
    z3 = torch.empty(npad, co, device=cuda_dev)
    ops.conv3x3_tr(xh, npad, ci, F + 2, 1, wg, co, None, z3)
    torch.cuda.synchronize()
    z3 = z3.cpu().double().numpy().reshape(B, T + 2, F + 2, co)
    _, S = R.conv_forward(R.bf16_round(x), R.bf16_round(w))
    err = np.abs(R.from_haloed(z) - R.from_haloed(z3))
    assert np.all(err <= R.sum_bound(9 * ci, S)), float(err.max())


@pytest.mark.gpu
def test_conv_taps_unsupported_shapes_are_refused(cuda_dev):
    """A shape the kernels do not take returns ASR_ERR_UNSUPPORTED with a reason,
    before any launch: a 7-tap axis, a channel count off the 16 grid (bf16), a grid
    smaller than the kernel."""
    N = _N()
    buf = torch.zeros(1 << 16, device=cuda_dev)
    for mode, T, F, ci, co, kf, kt in ((BF16, 11, 7, 16, 16, 7, 3), (BF16, 11, 7, 24, 16, 3, 5),
                                       (F32, 1, 7, 16, 16, 3, 5)):
        assert N.query('asr_conv_taps_supported', mode, 2, T, F, ci, co, kf, kt) == 0
        rc = N.lib().asr_conv_taps_forward(mode, N.ptr(buf), 2, T, F, ci, N.ptr(buf), co, kf, kt,
                                           None, N.ptr(buf), N.stream_handle(cuda_dev))
        assert rc == N.ASR_ERR_UNSUPPORTED and N.lib().asr_last_error()
