"""tests/conv3x3_ref.py checks itself, so the GPU tests do not trust an
unchecked reference: on zero-haloed operands the flat-row sums equal torch
float64 conv2d / conv_transpose2d / the weight gradient written as a
convolution on the interior (and tests/cnn_taps_ref.py's sums with kf = kt = 3),
and the weight-image index formulas round-trip."""
import numpy as np
import pytest
import torch

import conv3x3_ref as R

Fn = torch.nn.functional


def _case(B, T, F, Ci, Co, seed=0):
    rng = np.random.RandomState(seed + 7 * T + F)
    x = rng.randn(B, Ci, F, T)
    w = rng.randn(Co, Ci, 3, 3) * 0.3
    dz = rng.randn(B, Co, F, T)
    bias = rng.randn(Co)
    return x, w, dz, bias


def _flat(a):   # NCHW -> zero-haloed [P][C]
    return R.to_haloed(a).reshape(-1, a.shape[1])


def _interior(a, B, T, F):   # [P][C] -> NCHW interior
    return R.from_haloed(a.reshape(B, T + 2, F + 2, -1))


@pytest.mark.parametrize('B,T,F,Ci,Co', [(2, 5, 4, 3, 2), (1, 1, 1, 2, 3), (2, 1, 6, 1, 4),
                                         (1, 7, 1, 4, 1)])
def test_flat_sums_equal_torch_on_the_interior(B, T, F, Ci, Co):
    x, w, dz, bias = _case(B, T, F, Ci, Co)
    xt, wt, gt = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(dz)
    Fp = F + 2
    # forward: mode-0 image, sign +1
    z, S = R.flat_conv(_flat(x), R.pack_image(w), Fp, 1, bias)
    z_ref = Fn.conv2d(xt, wt, bias=torch.from_numpy(bias), padding=1).numpy()
    np.testing.assert_allclose(_interior(z, B, T, F), z_ref, rtol=0, atol=1e-12)
    z2, S2 = R.conv_forward(x, w, bias)
    np.testing.assert_allclose(z2, z_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(_interior(S, B, T, F), S2 + np.abs(bias)[None, :, None, None],
                               rtol=1e-12)
    assert np.all(np.abs(z) <= S * (1 + 1e-12))
    # input gradient: mode-1 image, sign -1
    dx, Sd = R.flat_conv(_flat(dz), R.pack_image(w, mode=1), Fp, -1)
    dx_ref = Fn.conv_transpose2d(gt, wt, padding=1).numpy()
    np.testing.assert_allclose(_interior(dx, B, T, F), dx_ref, rtol=0, atol=1e-12)
    dx2, Sd2 = R.conv_dgrad(dz, w, F, T)
    np.testing.assert_allclose(dx2, dx_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(_interior(Sd, B, T, F), Sd2, rtol=1e-12)
    # weight gradient: conv2d of x with dz as the kernel
    pk, Sw = R.flat_wgrad(_flat(x), _flat(dz), Fp)
    dw_ref = Fn.conv2d(xt.transpose(0, 1), gt.transpose(0, 1), padding=1).transpose(0, 1).numpy()
    np.testing.assert_allclose(R.unpack_image(pk, Ci), dw_ref, rtol=0, atol=1e-11)
    dw2, Sw2 = R.conv_wgrad(x, dz, 3, 3)
    np.testing.assert_allclose(dw2, dw_ref, rtol=0, atol=1e-11)
    np.testing.assert_allclose(R.unpack_image(Sw, Ci), Sw2, rtol=1e-12)


def test_flat_conv_reads_rows_outside_the_grid_as_zero():
    """Every row is a sum over the rows the shifts reach: a unit input row p0
    appears in out[p0 - sign shift(tap)] with that tap's weight, nowhere else."""
    P, Fp, Cin, N = 20, 5, 2, 3
    rng = np.random.RandomState(1)
    wimg = rng.randn(N, 9 * Cin)
    for sign in (1, -1):
        for p0 in (0, 7, P - 1):
            inp = np.zeros((P, Cin))
            inp[p0, 1] = 1.0
            out, _ = R.flat_conv(inp, wimg, Fp, sign)
            want = np.zeros((P, N))
            for tap in range(9):
                p = p0 - sign * R.tap_shift(tap, Fp)
                if 0 <= p < P:
                    want[p] += wimg[:, tap * Cin + 1]
            np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize('Co,Ci,cip', [(3, 2, 2), (4, 1, 16), (2, 5, 8)])
def test_weight_images_round_trip(Co, Ci, cip):
    rng = np.random.RandomState(Co + Ci)
    w = rng.randn(Co, Ci, 3, 3)
    img = R.pack_image(w, cip, 0, fill=np.nan)
    assert img.shape == (Co, 9 * cip)
    np.testing.assert_array_equal(R.unpack_image(img, Ci), w)
    np.testing.assert_array_equal(R.unpack_image_t(np.ascontiguousarray(img.T), Ci), w)
    # element by element, as include/asr_hip.h states the layout
    for co in range(Co):
        for ci in range(cip):
            for kh in range(3):
                for kw in range(3):
                    v = img[co, (kw * 3 + kh) * cip + ci]
                    assert (v == w[co, ci, kh, kw]) if ci < Ci else np.isnan(v)
    img1 = R.pack_image(w, mode=1)
    assert img1.shape == (Ci, 9 * Co)
    for co in range(Co):
        for ci in range(Ci):
            for kh in range(3):
                for kw in range(3):
                    assert img1[ci, (kw * 3 + kh) * Co + co] == w[co, ci, kh, kw]


def test_pad_input_and_halo_mask():
    xs = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4) + 1
    p = R.pad_input(xs, 3)
    assert p.shape == (2, 5, 6, 3)
    np.testing.assert_array_equal(p[:, 1:4, 1:5, 0], xs)
    assert not p[..., 1:].any() and not p[R.halo_mask(2, 3, 4)].any()
    assert R.halo_mask(2, 3, 4).sum() == 2 * (5 * 6 - 3 * 4)
