"""Float64 reference of one VGG block's element-wise half (csrc/cnn.hip behind
asr_vgg_block_forward* / asr_vgg_block_backward*): ReLU -> max-pool -> batch
norm -> dropout and its backward, restated in plain numpy.  Nothing here
imports the product package; oracle.rng supplies the dropout mask stream.

Layout: channels-last interiors, z [B, T, F, C] (time, then frequency), the
model's NCHW view being [B, C, F, T] (models/pytorch_v3/encoders/cnn.py:143-149).
pt / pf are the pool extents along time / frequency (0 = no pooling).

The same functions run in float32 (`dtype=np.float32`: every product and sum
rounded to float32, per-channel sums taken sequentially in row order) to
measure what float32 evaluation of these formulas costs against float64; the
GPU bounds are 16 x those figures (case_constants)."""
import functools

import numpy as np

from oracle import rng

F32_EPS = float(np.finfo(np.float32).eps)
# a tensor whose largest reference magnitude is below this is a cancellation
# residue of O(1) inputs (multiples of 1/8): errors are measured against the
# floor instead
SCALE_FLOOR = 2.0 ** -10
# no float32 result is expected to beat its own final rounding
CONST_FLOOR = F32_EPS / 2
MARGIN = 16.0


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def bf16_round(x):
    """float -> the nearest bf16 value (round to nearest, ties to even), as
    float32; done on the uint32 image of the float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits(x):
    """uint16 image of bf16-representable float32 values."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def pad(x):
    """[B, T, F, C] -> zero-haloed [B, T+2, F+2, C]."""
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def unpad(x):
    return x[:, 1:-1, 1:-1, :]


def pool_out(n, k, ceil_mode):
    """torch's pooling output size for kernel = stride = k, no padding."""
    if not ceil_mode:
        return (n - k) // k + 1
    o = -((n - k) // -k) + 1
    if (o - 1) * k >= n:      # the last window must start inside the input
        o -= 1
    return o


def pool_dims(T, F, pt, pf, ceil_mode):
    if not pt:
        return T, F
    return pool_out(T, pt, ceil_mode), pool_out(F, pf, ceil_mode)


def _colsum(x, dtype):
    """Per-channel sum over every leading axis; float32: sequential in row order."""
    x2 = x.reshape(-1, x.shape[-1])
    if dtype == np.float64:
        return x2.sum(axis=0, dtype=np.float64)
    return np.cumsum(x2, axis=0, dtype=np.float32)[-1]


# --------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------
def relu_pool(z, pt, pf, ceil_mode):
    """P = max over the window of relu(z), slot = df * pt + dt of the first
    maximum in the scan order frequency outer, time inner (post_fwd); windows
    are clipped at T and F.  Exact in any float type."""
    B, T, F, C = z.shape
    r = np.maximum(z, 0)
    if not pt:
        return r, None
    To, Fo = pool_dims(T, F, pt, pf, ceil_mode)
    assert To > 0 and Fo > 0
    full = np.full((B, To * pt, Fo * pf, C), -np.inf, dtype=z.dtype)
    tt, ff = min(T, To * pt), min(F, Fo * pf)
    full[:, :tt, :ff] = r[:, :tt, :ff]
    w = full.reshape(B, To, pt, Fo, pf, C)
    best = np.full((B, To, Fo, C), -np.inf, dtype=z.dtype)
    slot = np.zeros((B, To, Fo, C), dtype=np.uint8)
    for df in range(pf):
        for dt in range(pt):
            cand = w[:, :, dt, :, df, :]
            upd = cand > best            # strict: the first maximum wins
            best = np.where(upd, cand, best)
            slot = np.where(upd, np.uint8(df * pt + dt), slot)
    return best, slot


def bn_stats(P, run_mean, run_var, training, momentum, eps, dtype=np.float64, shifted=False):
    """(mean, rstd, new run_mean, new run_var).  Training: batch mean and
    biased variance over every (b, t', f') for the normalisation, the unbiased
    variance with momentum for the running update; eval: the running
    statistics, left untouched.  shifted: the variance as E[d^2] - E[d]^2 with
    d = P - run_mean, clamped at 0 (bn_finalize_shift), else two passes."""
    dt = dtype
    n = P.size // P.shape[-1]
    if not training:
        rm, rv = run_mean.astype(dt), run_var.astype(dt)
        return rm, (dt(1) / np.sqrt(rv + dt(eps))).astype(dt), run_mean, run_var
    inv_n = dt(1) / dt(n)
    Pd = P.astype(dt)
    if shifted:
        sh = run_mean.astype(dt)
        d = Pd - sh
        ed = _colsum(d, dt) * inv_n
        ed2 = _colsum(d * d, dt) * inv_n
        var = np.maximum(ed2 - ed * ed, dt(0))
        mean = sh + ed
    else:
        mean = _colsum(Pd, dt) * inv_n
        c = Pd - mean
        var = _colsum(c * c, dt) * inv_n
    rstd = (dt(1) / np.sqrt(var + dt(eps))).astype(dt)
    new_rm, new_rv = run_mean, run_var
    if run_mean is not None:
        unb = var * (dt(n) / dt(n - 1)) if n > 1 else var
        mom = dt(momentum)
        new_rm = (dt(1) - mom) * run_mean.astype(dt) + mom * mean
        new_rv = (dt(1) - mom) * run_var.astype(dt) + mom * unb
    return mean.astype(dt), rstd, new_rm, new_rv


def drop_mask(seed, shape, p):
    """The multiplicative dropout mask over [B][T'][F'][C] (0 or 1 / (1 - p) in
    float32, as the kernels form it); None when p == 0."""
    if not p:
        return None
    return rng.dropout_scale(seed, shape, p)


def apply_bn(P, gamma, beta, mean, rstd, mask, dtype=np.float64):
    dt = dtype
    y = P.astype(dt)
    if gamma is not None:
        y = (y - mean.astype(dt)) * rstd.astype(dt) * gamma.astype(dt) + beta.astype(dt)
    if mask is not None:
        y = y * mask.astype(dt)
    return y


def block_forward(z, pt, pf, ceil_mode, gamma, beta, run_mean, run_var, training, momentum, eps,
                  drop, seed, dtype=np.float64, shifted=False):
    """dict(P, slot, mean, rstd, run_mean, run_var, out, mask) of one block."""
    zz = np.asarray(z).astype(dtype)
    P, slot = relu_pool(zz, pt, pf, ceil_mode)
    mean = rstd = None
    rm, rv = run_mean, run_var
    if gamma is not None:
        mean, rstd, rm, rv = bn_stats(P, run_mean, run_var, training, momentum, eps, dtype, shifted)
    mask = drop_mask(seed, P.shape, drop)
    out = apply_bn(P, gamma, beta, mean, rstd, mask, dtype)
    return dict(P=P, slot=slot, mean=mean, rstd=rstd, run_mean=rm, run_var=rv, out=out, mask=mask)


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------
def block_backward(dnext, P, slot, T, F, pt, pf, gamma, mean, rstd, mask, training=True,
                   dtype=np.float64):
    """dict(dz [B, T, F, C], dgamma, dbeta, dbias) from dnext [B, T', F', C] and
    the forward's saved values.

    g = dnext * mask.  With gamma and training: the batch-statistics form
      dP = gamma rstd (g - sum(g) / n - xhat sum(g xhat) / n),  xhat = (P - mean) rstd,
    dgamma = sum(g xhat), dbeta = sum(g).  With gamma in eval mode the statistics
    are constants: dP = gamma rstd g (the plain affine form; dgamma / dbeta as
    above).  Without gamma dP = g.

    Which form the kernels apply: asr_vgg_block_backward* take no training
    flag; bn_bwd_moments / post_bwd (and their row-blocked forms) always apply
    the batch-statistics form to the mean / rstd they are handed, and the model
    never differentiates in eval mode.  The GPU tests therefore compare with
    training=True whatever statistics the forward used; training=False is
    here for the comparison with autograd only.

    dP goes to the window pixel slot names, if P > 0 (the ReLU: z > 0 at the
    argmax <=> P > 0); every other pixel, the ones no window covers included,
    gets 0.  dbias = per-channel sum of dz."""
    dt = dtype
    B, To, Fo, C = P.shape
    n = B * To * Fo
    g = np.asarray(dnext).astype(dt)
    if mask is not None:
        g = g * mask.astype(dt)
    Pd = P.astype(dt)
    dgamma = dbeta = None
    if gamma is not None:
        m, r, gm = mean.astype(dt), rstd.astype(dt), gamma.astype(dt)
        xh = (Pd - m) * r
        s1 = _colsum(g, dt)
        s2 = _colsum(g * xh, dt)
        dgamma, dbeta = s2, s1
        if training:
            inv_n = dt(1) / dt(n)
            dP = gm * r * (g - s1 * inv_n - xh * s2 * inv_n)
        else:
            dP = gm * r * g
    else:
        dP = g
    dP = np.where(Pd > 0, dP, dt(0)).astype(dt)
    dz = np.zeros((B, T, F, C), dtype=dt)
    if not pt:
        dz[...] = dP
    else:
        for df in range(pf):
            for dtm in range(pt):
                hit = np.where(slot == df * pt + dtm, dP, dt(0))
                # windows are clipped: a slot never names a pixel outside the input
                nt = len(range(dtm, min(T, To * pt), pt))
                nf = len(range(df, min(F, Fo * pf), pf))
                assert not hit[:, nt:].any() and not hit[:, :, nf:].any()
                dz[:, dtm:To * pt:pt, df:Fo * pf:pf][:, :nt, :nf] = hit[:, :nt, :nf]
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta, dbias=_colsum(dz, dt))


def covered(T, F, pt, pf, ceil_mode):
    """bool [T, F]: the pixel lies inside some pool window."""
    m = np.ones((T, F), dtype=bool)
    if pt:
        To, Fo = pool_dims(T, F, pt, pf, ceil_mode)
        m[To * pt:, :] = False
        m[:, Fo * pf:] = False
    return m


# --------------------------------------------------------------------------
# first layer: 3x3 stencil over one input channel
# --------------------------------------------------------------------------
def conv3x3_c1(xs, w, bias):
    """z[b, t, f, co] = bias[co] + sum_{kh, kw} w[co, 0, kh, kw] x[b, t + kw - 1, f + kh - 1]
    (torch Conv2d weight [Co, 1, 3 (freq), 3 (time)] on the [B, 1, F, T] view,
    zero padding) in float64, and S = |bias| + sum |w x| for error bounds."""
    x = np.pad(np.asarray(xs, dtype=np.float64), ((0, 0), (1, 1), (1, 1)))
    B, T, F = xs.shape
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3, 3)
    Co = w.shape[0]
    b = np.zeros(Co) if bias is None else np.asarray(bias, dtype=np.float64)
    z = np.broadcast_to(b, (B, T, F, Co)).copy()
    S = np.broadcast_to(np.abs(b), (B, T, F, Co)).copy()
    for kh in range(3):
        for kw in range(3):
            tap = x[:, kw:kw + T, kh:kh + F, None] * w[:, kh, kw]
            z += tap
            S += np.abs(tap)
    return z, S


def bf16_boundary_distance(v):
    """Distance of float64 v to the nearest bf16 rounding boundary (the midpoint
    of two adjacent bf16 values), for normal-range v."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -120)))
    ulp = 2.0 ** (e - 7)
    frac = a / ulp - np.floor(a / ulp)
    return np.abs(frac - 0.5) * ulp


# --------------------------------------------------------------------------
# cases and float32 error constants
# --------------------------------------------------------------------------
def make_case(B, T, F, C, pt=0, pf=0, ceil_mode=1, bn=True, training=True, run_stats=True,
              drop=0.0, seed=0, far=0.0, dead_channel=False, data_seed=0):
    """Inputs of one block case, bf16-representable by construction: z on the
    grid of multiples of 1/8 in [-2, 2] (ties and all-negative windows are
    common), dnext random normal rounded to bf16.  far: run_mean = batch mean
    +- far batch standard deviations (alternating sign per channel);
    dead_channel: every z of channel 0 <= 0."""
    r = np.random.RandomState(1000 + data_seed)
    z = (r.randint(-16, 17, size=(B, T, F, C)) / 8.0).astype(np.float32)
    if dead_channel:
        z[..., 0] = 0.0 - np.abs(z[..., 0])      # (no -0.0: P is compared bit for bit)
    To, Fo = pool_dims(T, F, pt, pf, ceil_mode)
    dnext = bf16_round(r.randn(B, To, Fo, C).astype(np.float32))
    c = dict(B=B, T=T, F=F, C=C, pt=pt, pf=pf, ceil_mode=ceil_mode, To=To, Fo=Fo, z=z, dnext=dnext,
             training=training, momentum=0.1, eps=1e-5, drop=drop, seed=seed,
             gamma=None, beta=None, run_mean=None, run_var=None)
    if bn:
        c['gamma'] = (r.rand(C) + 0.5).astype(np.float32)
        c['beta'] = (r.randn(C) * 0.1).astype(np.float32)
        if run_stats:
            c['run_mean'] = (r.randn(C) * 0.1).astype(np.float32)
            c['run_var'] = (r.rand(C) + 0.5).astype(np.float32)
            if far:
                P, _ = relu_pool(z.astype(np.float64), pt, pf, ceil_mode)
                m, sd = P.reshape(-1, C).mean(0), P.reshape(-1, C).std(0)
                sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
                c['run_mean'] = (m + sign * far * sd).astype(np.float32)
                if dead_channel:     # no spread to scale by: a plainly far centre
                    c['run_mean'][0] = 4.0
    return c


def reference(c, shifted=False, dtype=np.float64):
    """Forward and backward of case c in `dtype`; the backward consumes the
    float64 forward's mean / rstd rounded to float32 (what a kernel hands over)
    in either precision, so forward rounding stays out of the backward figures."""
    fw = block_forward(c['z'], c['pt'], c['pf'], c['ceil_mode'], c['gamma'], c['beta'],
                       c['run_mean'], c['run_var'], c['training'], c['momentum'], c['eps'],
                       c['drop'], c['seed'], dtype=dtype, shifted=shifted)
    f64 = fw if dtype == np.float64 else block_forward(
        c['z'], c['pt'], c['pf'], c['ceil_mode'], c['gamma'], c['beta'], c['run_mean'],
        c['run_var'], c['training'], c['momentum'], c['eps'], c['drop'], c['seed'])
    mean = rstd = None
    if c['gamma'] is not None:
        mean, rstd = f64['mean'].astype(np.float32), f64['rstd'].astype(np.float32)
    bw = block_backward(c['dnext'], fw['P'], fw['slot'], c['T'], c['F'], c['pt'], c['pf'],
                        c['gamma'], mean, rstd, fw['mask'], True, dtype=dtype)
    return fw, bw


def scale_of(ref):
    return max(float(np.max(np.abs(ref))) if np.size(ref) else 0.0, SCALE_FLOOR)


def nerr(got, ref):
    """max |got - ref| / max(max |ref|, floor): the unit of every bound here."""
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)))) / scale_of(ref)


STAT_KEYS = ('mean', 'rstd', 'run_mean', 'run_var')
FWD_KEYS = STAT_KEYS + ('out',)
BWD_KEYS = ('dgamma', 'dbeta', 'dbias', 'dz')


def case_constants(c, shifted):
    """{tensor: float32-versus-float64 error of the same formulas on case c},
    in nerr units, floored at half a float32 eps.  shifted: the variance in the
    E[d^2] - E[d]^2 form centred on run_mean, where the kernels use it.  The
    GPU bound on a tensor is MARGIN x its constant."""
    f64, b64 = reference(c, shifted=False)
    f32, b32 = reference(c, shifted=shifted, dtype=np.float32)
    out = {}
    for k in FWD_KEYS:
        if f64[k] is not None:
            out[k] = max(nerr(f32[k], f64[k]), CONST_FLOOR)
    for k in BWD_KEYS:
        if b64[k] is not None:
            out[k] = max(nerr(b32[k], b64[k]), CONST_FLOOR)
    return out


def fused_var_expected(c, env=None):
    """Whether asr_vgg_block_forward_* takes the shifted (fused) variance for
    case c: training-mode batch norm with running statistics, C % 4 == 0, and
    the fused pool pass's block count within the statistics' chunk count
    (vgg_block_forward_impl: fused_mean / fused_var), unless switched off."""
    env = env or {}
    if c['gamma'] is None or not c['training'] or c['run_mean'] is None or c['C'] % 4:
        return False
    if env.get('ASR_VGG_FUSED_MEAN') == '0' or env.get('ASR_VGG_FUSED_VAR') == '0':
        return False
    nr = c['B'] * c['To'] * c['Fo']
    per = -(-nr // (1 if nr < 1024 else 1024))
    vchunks = -(-nr // per)
    fgrid = min(max(-(-(nr * c['C'] // 4) // 256), 1), 8192, 1024)
    return fgrid <= vchunks


# The GPU cases' geometries (tests/test_vgg_block_gpu.py parametrises over
# these names; the CPU file computes and prints every constant).
GEOMS = {
    'u64':    dict(B=2, T=25, F=24, C=64),
    'u128':   dict(B=2, T=25, F=24, C=128),
    'ceil64': dict(B=3, T=41, F=39, C=64, pt=2, pf=2, ceil_mode=1),
    'floor64': dict(B=3, T=41, F=39, C=64, pt=2, pf=2, ceil_mode=0),
    'floor128s': dict(B=2, T=7, F=5, C=128, pt=2, pf=2, ceil_mode=0),
    'c4u':    dict(B=2, T=9, F=7, C=4),
    'c4p':    dict(B=2, T=9, F=7, C=4, pt=2, pf=2, ceil_mode=1),
    'np23':   dict(B=2, T=9, F=10, C=8, pt=2, pf=3, ceil_mode=1),
    'np32':   dict(B=2, T=9, F=10, C=8, pt=3, pf=2, ceil_mode=0),
    'f16p':   dict(B=2, T=9, F=7, C=16, pt=2, pf=2, ceil_mode=1),
    'f16u':   dict(B=2, T=9, F=7, C=16),
    'f2p':    dict(B=2, T=9, F=7, C=2, pt=2, pf=2, ceil_mode=0),
    'f2u':    dict(B=2, T=9, F=7, C=2),
}


# io defaults: the production types (bf16 z / P / padded out / dnext / dz)
IO = dict(z='bf16', p='bf16', out='bf16', flat=0, dn='bf16', dz='bf16')
F32IO = dict(z='f32', p='f32', out='f32', flat=0, dn='f32', dz='f32')
FLAT = dict(out='f32', flat=1, dn='f32')
ROWS0 = {'ASR_VGG_ROWS': '0'}
FULL0 = {'ASR_VGG_POST_FULL': '0'}
SEED = 0x1234567890


def _gpu_cases():
    cs = []

    def add(cid, geom, io=None, env=None, **kw):
        cs.append(dict(id=cid, geom=geom, io=dict(IO, **(io or {})), env=dict(env or {}), kw=kw))

    # 1: row-blocked, unpooled, fused mean and variance
    for g in ('u64', 'u128'):
        add('1-%s-dnbf16' % g, g)
        add('1-%s-dnf32' % g, g, dict(dn='f32'))
    # 2: row-blocked, 2 x 2 ceil-mode pool, odd extents; padded and flat
    add('2-ceil64-pad', 'ceil64')
    add('2-ceil64-flat', 'ceil64', FLAT)
    # 3: floor mode, odd T and F: uncovered last row and column
    add('3-floor64', 'floor64')
    add('3-floor128s', 'floor128s')
    add('3-floor128s-dnf32', 'floor128s', dict(dn='f32'))
    # 4: rw_bn_moments_nu
    for v in ('256x2', '512x1', '1024x2'):
        add('4-ceil64-bnm%s' % v, 'ceil64', env={'ASR_VGG_BNM': v})
    # 5: each statistics route
    for k in ('ASR_VGG_FUSED_VAR', 'ASR_VGG_FUSED_MEAN'):
        add('5-u64-%s0' % k[8:].lower(), 'u64', env={k: '0'})
        add('5-ceil64-%s0' % k[8:].lower(), 'ceil64', env={k: '0'})
    # 6: grid-stride passes at production types
    add('6-u64-rows0', 'u64', env=ROWS0)
    add('6-u128-rows0-dnf32', 'u128', dict(dn='f32'), env=ROWS0)
    add('6-ceil64-rows0', 'ceil64', env=ROWS0)
    add('6-ceil64-rows0-flat', 'ceil64', FLAT, env=ROWS0)
    add('6-floor64-rows0', 'floor64', env=ROWS0)
    add('6-floor64-rows0-dzf32', 'floor64', dict(dn='f32', dz='f32'), env=ROWS0)
    for g in ('u64', 'ceil64', 'floor64'):
        add('6-%s-rows0-full0' % g, g, dict(dn='f32'), env=dict(ROWS0, **FULL0))
    add('6-floor64-rows0-full0-dzf32', 'floor64', dict(dn='f32', dz='f32'), env=dict(ROWS0, **FULL0))
    # 7: C = 4, refused by the row kernels
    add('7-c4p-pbf16', 'c4p')
    add('7-c4p-pf32', 'c4p', dict(p='f32'))
    add('7-c4u-pbf16-dnf32', 'c4u', dict(dn='f32'))
    add('7-c4u-pf32-flat', 'c4u', dict(p='f32', **FLAT))
    # 8: non-square pools (poolings [freq, time] = [3, 2] and [2, 3] of the model)
    add('8-np23', 'np23')
    add('8-np32', 'np32')
    add('8-np32-pf32-dnf32', 'np32', dict(p='f32', dn='f32'))
    # 9: f32 z (asr_vgg_block_forward / _backward_ex), V = 4 and V = 1
    for g in ('f16p', 'f16u', 'f2p', 'f2u'):
        add('9-%s' % g, g, F32IO)
        add('9-%s-bf16' % g, g, dict(F32IO, out='bf16', dz='bf16'))
    add('9-f16p-full0', 'f16p', F32IO, env=FULL0)
    add('9-f16p-full0-bf16', 'f16p', dict(F32IO, dz='bf16'), env=FULL0)
    add('9-f16u-flat', 'f16u', dict(F32IO, flat=1))
    # 10: eval mode and no batch norm
    for g, io in (('f16p', F32IO), ('f16u', F32IO), ('f2p', F32IO), ('c4p', None), ('c4u', None),
                  ('u64', None), ('ceil64', None)):
        add('10-%s-eval' % g, g, io, training=False)
        add('10-%s-nobn' % g, g, io, bn=False)
    add('10-ceil64-nobn-rows0-full0', 'ceil64', dict(dn='f32'), env=dict(ROWS0, **FULL0), bn=False)
    # 11: dropout inside the block
    add('11-u64-drop', 'u64', drop=0.3, seed=SEED)
    add('11-ceil64-drop-flat', 'ceil64', FLAT, drop=0.3, seed=SEED + 1)
    add('11-c4p-drop', 'c4p', drop=0.3, seed=SEED + 2)
    add('11-c4p-drop-flat', 'c4p', FLAT, drop=0.3, seed=SEED + 3)
    add('11-f2p-drop', 'f2p', F32IO, drop=0.3, seed=SEED + 4)
    # 12: running mean 8 batch standard deviations off, one all-non-positive channel
    add('12-u64-far', 'u64', far=8.0, dead_channel=True)
    add('12-u128-far', 'u128', far=8.0, dead_channel=True)
    add('12-u64-far-rows0', 'u64', env=ROWS0, far=8.0, dead_channel=True)
    return cs


GPU_CASES = _gpu_cases()


def gpu_case(cc):
    """(inputs, constants, shifted) of one GPU_CASES entry."""
    kw = tuple(sorted(cc['kw'].items()))
    c = geom_case(cc['geom'], kw)
    shifted = fused_var_expected(c, cc['env'])
    return c, geom_constants(cc['geom'], shifted, kw), shifted


@functools.lru_cache(maxsize=None)
def geom_case(name, kw=()):
    return make_case(**dict(GEOMS[name], **dict(kw)))


@functools.lru_cache(maxsize=None)
def geom_constants(name, shifted, kw=()):
    return case_constants(geom_case(name, kw), shifted)
