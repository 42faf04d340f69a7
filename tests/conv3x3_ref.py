"""float64 numpy references for the VGG front-end's 3x3 convolution kernels
(csrc/conv.hip, the conv / pack / pad entry points of csrc/cnn.hip), written
from the formulas in include/asr_hip.h and the header of conv.hip; none calls
a project kernel.  The NCHW convolutions, bf16_round, sum_bound and the haloed
layouts are tests/cnn_taps_ref.py's (kf = kt = 3); new here:

  flat_conv / flat_wgrad   the flat-row sums the tap-resident kernels implement
                           over ALL P padded pixel rows (halo rows included),
                           rows outside [0, P) reading as zero, each with the
                           sum of the magnitudes of its terms (sum_bound's unit)
  pack_image / unpack_image / unpack_image_t
                           the GEMM weight images of a Conv2d weight
                           [Co][Ci][3 (f)][3 (t)]: tap j = kw * 3 + kh has the
                           row shift (kw - 1) Fp + (kh - 1)
  pad_input / halo_mask    the padded input plane and the halo pixels of
                           [B][T+2][F+2]
"""
import numpy as np

from cnn_taps_ref import (bf16_round, conv_dgrad, conv_forward, conv_wgrad, from_haloed,  # noqa: F401
                          sum_bound, to_haloed)


def tap_shift(tap, Fp):
    return (tap // 3 - 1) * Fp + (tap % 3 - 1)


def _shifted(a, s):
    """rows r of the result = a[r + s], zero where r + s is outside [0, P)."""
    P = a.shape[0]
    out = np.zeros_like(a)
    lo, hi = max(0, -s), min(P, P - s)
    if lo < hi:
        out[lo:hi] = a[lo + s:hi + s]
    return out


def flat_conv(inp, wimg, Fp, sign, bias=None):
    """out[p][n] = bias[n] + sum_tap sum_c inp[p + sign shift(tap)][c] wimg[n][tap Cin + c]
    for every row p < P.  inp [P][Cin], wimg [N][9 Cin] -> (out [P][N], S [P][N])
    with S the sum of |terms| (|bias| included)."""
    inp, wimg = np.asarray(inp, np.float64), np.asarray(wimg, np.float64)
    P, Cin = inp.shape
    N = wimg.shape[0]
    out, S = np.zeros((P, N)), np.zeros((P, N))
    for tap in range(9):
        sh = _shifted(inp, sign * tap_shift(tap, Fp))
        wt = wimg[:, tap * Cin:(tap + 1) * Cin].T
        out += sh @ wt
        S += np.abs(sh) @ np.abs(wt)
    if bias is not None:
        b = np.asarray(bias, np.float64)
        out, S = out + b, S + np.abs(b)
    return out, S


def flat_wgrad(x, dz, Fp):
    """packed[n][tap Cin + c] = sum_p dz[p][n] x[p + shift(tap)][c].
    x [P][Cin], dz [P][N] -> (packed [N][9 Cin], S)."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    Cin, N = x.shape[1], dz.shape[1]
    out, S = np.zeros((N, 9 * Cin)), np.zeros((N, 9 * Cin))
    for tap in range(9):
        sh = _shifted(x, tap_shift(tap, Fp))
        out[:, tap * Cin:(tap + 1) * Cin] = dz.T @ sh
        S[:, tap * Cin:(tap + 1) * Cin] = np.abs(dz).T @ np.abs(sh)
    return out, S


# ------------------------------------------------------------ weight images
def pack_image(w, cip=None, mode=0, fill=0.0):
    """mode 0: out[co][j cip + ci] = w[co][ci][kh][kw]  ([Co][9 cip], channels
    ci >= Ci hold `fill`);  mode 1: out[ci][j Co + co] = w[co][ci][kh][kw]
    ([Ci][9 Co]);  j = kw * 3 + kh."""
    w = np.asarray(w)
    Co, Ci = w.shape[:2]
    if mode == 1:
        return np.ascontiguousarray(w.transpose(1, 3, 2, 0)).reshape(Ci, 9 * Co)
    cip = Ci if cip is None else cip
    out = np.full((Co, 3, 3, cip), fill, w.dtype)
    out[..., :Ci] = w.transpose(0, 3, 2, 1)          # [co][kw][kh][ci]
    return out.reshape(Co, 9 * cip)


def unpack_image(packed, Ci):
    """dw[co][ci][kh][kw] = packed[co][(kw * 3 + kh) cip + ci]  (packed [Co][9 cip])."""
    packed = np.asarray(packed)
    Co = packed.shape[0]
    cip = packed.shape[1] // 9
    return np.ascontiguousarray(packed.reshape(Co, 3, 3, cip)[..., :Ci].transpose(0, 3, 2, 1))


def unpack_image_t(packed_t, Ci):
    """dw[co][ci][kh][kw] = packed_t[(kw * 3 + kh) cip + ci][co]  (packed_t [9 cip][Co])."""
    packed_t = np.asarray(packed_t)
    Co = packed_t.shape[1]
    cip = packed_t.shape[0] // 9
    return np.ascontiguousarray(packed_t.reshape(3, 3, cip, Co)[:, :, :Ci].transpose(3, 2, 1, 0))


# ------------------------------------------------------------------ layouts
def pad_input(xs, Cp=1):
    """xs [B][T][F] -> [B][T+2][F+2][Cp]: channel 0 = xs, zero elsewhere."""
    xs = np.asarray(xs)
    B, T, F = xs.shape
    out = np.zeros((B, T + 2, F + 2, Cp), xs.dtype)
    out[:, 1:T + 1, 1:F + 1, 0] = xs
    return out


def halo_mask(B, T, F):
    """[B][T+2][F+2] bool: True on the one-pixel halo."""
    m = np.ones((B, T + 2, F + 2), bool)
    m[:, 1:T + 1, 1:F + 1] = False
    return m
