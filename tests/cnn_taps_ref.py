"""float64 references for the kf x kt convolution kernels (csrc/conv_taps.hip)
and the activation -> pool -> batch norm -> dropout block (csrc/cnn_act.hip),
written from the formulas in include/asr_hip.h; none calls a project kernel.

Convolution (numpy): NCHW with H = freq, W = time, as the reference's Conv2d
sees it (encoders/cnn.py:68-73: kernel (kf, kt), stride 1, padding 1); each
function also returns the sum of the magnitudes of its terms, the unit of the
summation bound the GPU test applies.  Layout helpers convert to and from the
kernels' channels-last haloed grids [B][T+2][F+2][C].

Block (torch, any dtype): float64 is the reference; the same formulas in
float32 give the error constants of the GPU bounds, as tests/vgg_block_ref.py
does for the ReLU block (case_constants; MARGIN x constant x scale_of).
"""
import numpy as np
import torch

import vgg_block_ref as R

ACT_RELU, ACT_PRELU, ACT_HARDTANH = 0, 1, 2


# ------------------------------------------------------------------ layouts
def to_haloed(a):
    """NCHW [B, C, F, T] -> [B, T+2, F+2, C] with a zero halo."""
    B, C, F, T = a.shape
    out = np.zeros((B, T + 2, F + 2, C), a.dtype)
    out[:, 1:T + 1, 1:F + 1] = a.transpose(0, 3, 2, 1)
    return out


def from_haloed(a):
    """[B, T+2, F+2, C] -> NCHW interior [B, C, F, T]."""
    return a[:, 1:-1, 1:-1].transpose(0, 3, 2, 1)


def bf16_round(a):
    """Round to the nearest bf16 value (ties to even), returned in float64."""
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


# -------------------------------------------------------------- convolution
def _windows(xp, kf, kt, Fo, To):
    """[B, C, kf, kt, Fo, To] view of the padded input."""
    return np.stack([np.stack([xp[:, :, df:df + Fo, dt:dt + To] for dt in range(kt)], 2)
                     for df in range(kf)], 2)


def conv_forward(x, w, bias=None):
    """x [B, Ci, F, T], w [Co, Ci, kf, kt] -> (z [B, Co, Fo, To], S = sum |x w|)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    kf, kt = w.shape[2:]
    B, Ci, F, T = x.shape
    Fo, To = F + 3 - kf, T + 3 - kt
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    win = _windows(xp, kf, kt, Fo, To)
    z = np.einsum('bcijft,ocij->boft', win, w)
    S = np.einsum('bcijft,ocij->boft', np.abs(win), np.abs(w))
    if bias is not None:
        z = z + np.asarray(bias, np.float64)[None, :, None, None]
    return z, S


def conv_dgrad(dz, w, F, T):
    """dz [B, Co, Fo, To] -> (dx [B, Ci, F, T], S): the adjoint of conv_forward."""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    Co, Ci, kf, kt = w.shape
    B = dz.shape[0]
    Fo, To = dz.shape[2:]
    dxp = np.zeros((B, Ci, F + 2, T + 2))
    Sp = np.zeros_like(dxp)
    for df in range(kf):
        for dt in range(kt):
            dxp[:, :, df:df + Fo, dt:dt + To] += np.einsum('boft,oc->bcft', dz, w[:, :, df, dt])
            Sp[:, :, df:df + Fo, dt:dt + To] += np.einsum('boft,oc->bcft', np.abs(dz),
                                                          np.abs(w[:, :, df, dt]))
    return dxp[:, :, 1:-1, 1:-1], Sp[:, :, 1:-1, 1:-1]


def conv_wgrad(x, dz, kf, kt):
    """(dw [Co, Ci, kf, kt], S) = sum over pixels of dz x."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    Fo, To = dz.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    win = _windows(xp, kf, kt, Fo, To)
    dw = np.einsum('bcijft,boft->ocij', win, dz)
    S = np.einsum('bcijft,boft->ocij', np.abs(win), np.abs(dz))
    return dw, S


def sum_bound(K, S):
    """|f32 sum of K exact products - exact sum| <= 2 K 2^-24 sum |terms| (any order)."""
    return 2.0 * K * 2.0 ** -24 * S


# -------------------------------------------------------------------- block
def pool_dims(T, F, pt, pf, ceil_mode):
    if not pt:
        return T, F
    if ceil_mode:
        return -(-T // pt), -(-F // pf)
    return T // pt, F // pf


def block(z, act, slope, pt, pf, ceil_mode, gamma, beta, run_mean, run_var, training, momentum,
          eps, mask, dnext, dtype=torch.float64):
    """The whole block on z [B, T, F, C] (valid pixels, channels last) in `dtype`:
    activation -> max pool (kernel = stride = (pf, pt) over (freq, time), the given
    rounding) -> batch norm (batch or running statistics) -> * mask (the dropout
    scale over [B, T', F', C], or None), and its gradients for d out = dnext.
    Returns a dict of float64 numpy arrays."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    zt = t(z).requires_grad_(True)
    sl = t(np.reshape(slope, (1,))).requires_grad_(True) if act == ACT_PRELU else None
    if act == ACT_PRELU:
        a = torch.where(zt > 0, zt, sl * zt)
    elif act == ACT_HARDTANH:
        a = torch.nn.functional.hardtanh(zt, 0.0, 20.0)   # gradient where 0 < z < 20
    else:
        a = torch.relu(zt)
    P = a
    if pt:
        # [B, T, F, C] -> [B, C, F, T]: torch's window scan order (freq outer, time inner)
        P = torch.nn.functional.max_pool2d(a.permute(0, 3, 2, 1), (pf, pt), (pf, pt),
                                           ceil_mode=bool(ceil_mode)).permute(0, 3, 2, 1)
    out = {'P': P}
    y = P
    g = be = None
    if gamma is not None:
        g, be = t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
        if training:
            n = P.numel() // P.shape[-1]
            mean = P.mean((0, 1, 2))
            var = ((P - mean) ** 2).mean((0, 1, 2))
            out['run_mean'] = (1 - momentum) * t(run_mean) + momentum * mean
            out['run_var'] = (1 - momentum) * t(run_var) + momentum * var * n / max(n - 1, 1)
        else:
            mean, var = t(run_mean), t(run_var)
        rstd = 1.0 / torch.sqrt(var + eps)
        out['mean'], out['rstd'] = mean, rstd
        y = (P - mean) * rstd * g + be
    if mask is not None:
        y = y * t(mask)
    out['out'] = y
    y.backward(t(dnext))
    out['dz'] = zt.grad
    if g is not None:
        out['dgamma'], out['dbeta'] = g.grad, be.grad
    out['dbias'] = zt.grad.sum((0, 1, 2))
    if sl is not None:
        out['dslope'] = sl.grad
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


def block_constants(args):
    """(float64 reference, {tensor: float32-vs-float64 error of the same formulas}),
    in vgg_block_ref.nerr units floored at CONST_FLOOR: the GPU bound on a
    tensor is vgg_block_ref.MARGIN x its constant x scale_of(reference)."""
    r64 = block(*args)
    r32 = block(*args, dtype=torch.float32)
    return r64, {k: max(R.nerr(r32[k], r64[k]), R.CONST_FLOOR) for k in r64}
