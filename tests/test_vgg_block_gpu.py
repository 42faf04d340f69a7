"""The VGG block passes of csrc/cnn.hip (ReLU, max-pool, batch norm, dropout;
forward and backward) against the float64 reference tests/vgg_block_ref.py,
through the C entry points, on every dispatch path of vgg_block_forward_impl /
vgg_block_backward_impl / asr_vgg_block_forward_given_p ("VGG block
reference tests", lists case -> kernels).

Inputs are bf16-representable (z on the 1/8 grid in [-2, 2], dnext rounded to
bf16), so the reference sees exactly what a kernel sees in either type.  `out`
and `dz` are handed over as VGGFn does: interior uninitialised (NaN here), halo
zero -- except where VGGFn zero-fills dz because the pass writes only the
argmax pixels (C % 4 != 0 or ASR_VGG_POST_FULL=0).  dgamma / dbeta / dbias
accumulate, so they start non-zero.

Per case: P bit-equal, slot equal, no NaN left, halos zero, uncovered pixels'
dz exactly zero; statistics, dgamma, dbeta, dbias and f32 out / dz within
MARGIN (16) x the float32-evaluation constant of the same case
(vgg_block_ref.case_constants, in units of max |reference| of the tensor);
bf16 out / dz within that plus one bf16 ulp (2^-8 |ref|).  The backward is
given the kernel's own mean / rstd / P / slot, so forward rounding does not
enter its bound."""
import numpy as np
import pytest
import torch

import vgg_block_ref as R

BF16, F32 = 1, 0
DT = {'bf16': (torch.bfloat16, BF16), 'f32': (torch.float32, F32)}


def _N():
    from pytorch_end2end_speech_recognition_amd import _native as N
    return N


def _dev(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dtype).contiguous()


def _padded_nan(B, T, F, C, dtype, dev, fill=float('nan')):
    """[B, T+2, F+2, C]: interior `fill`, halo zero."""
    t = torch.zeros(B, T + 2, F + 2, C, dtype=dtype, device=dev)
    t[:, 1:-1, 1:-1] = fill
    return t


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _halo_zero(t):
    t = t.clone()
    t[:, 1:-1, 1:-1] = 0
    return not bool(t.ne(0).any())


def _check(what, got, ref, const, bf16=False, fails=None):
    """|got - ref| <= MARGIN const scale (+ one bf16 ulp of the reference)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = R.MARGIN * const * R.scale_of(ref) + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)
    err = np.abs(got - ref)
    worst = float(np.max(err / tol))
    print('  %-9s err/bound %.3f  (max err %.3e, const %.2e%s)'
          % (what, worst, float(err.max()), const, ', + bf16 ulp' if bf16 else ''))
    if not np.isfinite(worst) or worst > 1.0:
        fails.append((what, worst))


def _run_block(cc, c, dev, monkeypatch):
    """Forward then backward of GPU case cc on inputs c; returns the tensors."""
    N = _N()
    for k in ('ASR_VGG_ROWS', 'ASR_VGG_POST_FULL', 'ASR_VGG_FUSED_MEAN', 'ASR_VGG_FUSED_VAR',
              'ASR_VGG_BNM', 'ASR_VGG_POOL_WALK'):
        monkeypatch.delenv(k, raising=False)
    for k, v in cc['env'].items():
        monkeypatch.setenv(k, v)
    io = cc['io']
    B, T, F, C, pt, pf, cm = (c[k] for k in ('B', 'T', 'F', 'C', 'pt', 'pf', 'ceil_mode'))
    To, Fo = c['To'], c['Fo']
    zt, zd = DT[io['z']]
    ptt, pd = DT[io['p']]
    ot, od = DT[io['out']]
    dnt, dnd = DT[io['dn']]
    dzt, dzd = DT[io['dz']]
    flat = io['flat']
    bn = c['gamma'] is not None
    f32 = dict(dtype=torch.float32, device=dev)
    z = _dev(R.pad(c['z']), zt, dev)
    P = torch.full((B * To * Fo, C), float('nan'), dtype=ptt, device=dev)
    slot = torch.full((B * To * Fo * C,), 255, dtype=torch.uint8, device=dev) if pt else None
    out = (torch.full((B, To, Fo, C), float('nan'), **f32) if flat else
           _padded_nan(B, To, Fo, C, ot, dev))
    gamma = _dev(c['gamma'], torch.float32, dev) if bn else None
    beta = _dev(c['beta'], torch.float32, dev) if bn else None
    rm = _dev(c['run_mean'], torch.float32, dev) if c['run_mean'] is not None else None
    rv = _dev(c['run_var'], torch.float32, dev) if c['run_var'] is not None else None
    mean = torch.full((C,), float('nan'), **f32) if bn else None
    rstd = torch.full((C,), float('nan'), **f32) if bn else None
    nb = N.query('asr_vgg_block_workspace_bytes', B, To, Fo, C)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    st = N.stream_handle(dev)
    tail = (N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv), int(c['training']), c['momentum'],
            c['eps'], N.ptr(mean), N.ptr(rstd), float(c['drop']), int(c['seed']), N.ptr(out), od,
            int(flat), N.ptr(ws), nb, st)
    if io['z'] == 'f32':
        assert io['p'] == 'f32'
        N.call('asr_vgg_block_forward', N.ptr(z), B, T, F, C, pt, pf, cm, N.ptr(P), N.ptr(slot), *tail)
    elif io['p'] == 'f32' and pt:      # the f32-P entry point of a bf16 z
        N.call('asr_vgg_block_forward_z', N.ptr(z), zd, B, T, F, C, pt, pf, cm, N.ptr(P),
               N.ptr(slot), *tail)
    else:
        N.call('asr_vgg_block_forward_zp', N.ptr(z), zd, B, T, F, C, pt, pf, cm, N.ptr(P), pd,
               N.ptr(slot), *tail)
    torch.cuda.synchronize()
    # ---- backward, from the kernel's own saved values
    if flat:
        dn = _dev(c['dnext'], torch.float32, dev)
    else:
        dn = _dev(R.pad(c['dnext']), dnt, dev)
    writes_all = C % 4 == 0 and cc['env'].get('ASR_VGG_POST_FULL') != '0'
    dz = _padded_nan(B, T, F, C, dzt, dev, float('nan') if writes_all else 0.0)
    pre = {k: torch.linspace(-1.0, 2.0, C, **f32) * s for k, s in
           (('dgamma', 1.0), ('dbeta', -0.5), ('dbias', 3.0))}
    acc = {k: v.clone() for k, v in pre.items()}
    dg, db = (acc['dgamma'], acc['dbeta']) if bn else (None, None)
    btail = (N.ptr(slot), N.ptr(gamma), N.ptr(mean), N.ptr(rstd), N.ptr(dg), N.ptr(db),
             float(c['drop']), int(c['seed']), N.ptr(dz), dzd, N.ptr(acc['dbias']), N.ptr(ws), nb, st)
    if io['z'] == 'f32':
        assert io['dn'] == 'f32'
        N.call('asr_vgg_block_backward_ex', N.ptr(dn), int(flat), N.ptr(z), B, T, F, C, pt, pf, cm,
               N.ptr(P), *btail)
    elif io['p'] == 'f32' and pt:
        N.call('asr_vgg_block_backward_zd', N.ptr(dn), F32 if flat else dnd, int(flat), N.ptr(z), zd,
               B, T, F, C, pt, pf, cm, N.ptr(P), *btail)
    else:
        N.call('asr_vgg_block_backward_zdp', N.ptr(dn), F32 if flat else dnd, int(flat), N.ptr(z),
               zd, B, T, F, C, pt, pf, cm, N.ptr(P), pd, *btail)
    torch.cuda.synchronize()
    return dict(P=P, slot=slot, out=out, mean=mean, rstd=rstd, rm=rm, rv=rv, dz=dz,
                acc=acc, pre=pre)


def _assert_block(cc, c, k, g, dead=None):
    """Every assertion of one case: kernel results g against the reference."""
    io = cc['io']
    B, T, F, C, pt, pf, cm = (c[key] for key in ('B', 'T', 'F', 'C', 'pt', 'pf', 'ceil_mode'))
    To, Fo = c['To'], c['Fo']
    bn = c['gamma'] is not None
    fw = R.block_forward(c['z'], pt, pf, cm, c['gamma'], c['beta'], c['run_mean'], c['run_var'],
                         c['training'], c['momentum'], c['eps'], c['drop'], c['seed'])
    fails = []
    # ---- forward
    Pg = g['P'].float().cpu().numpy().reshape(B, To, Fo, C)
    Pref = fw['P'].astype(np.float32)
    assert np.array_equal(Pg.view(np.uint32), Pref.view(np.uint32)), 'P not bit-equal'
    if io['p'] == 'bf16':
        assert np.array_equal(g['P'].view(torch.int16).cpu().numpy().reshape(B, To, Fo, C).view(np.uint16),
                              R.bf16_bits(Pref)), 'bf16 P bits'
    if pt:
        assert np.array_equal(g['slot'].cpu().numpy().reshape(B, To, Fo, C), fw['slot']), 'slot'
    out = g['out']
    assert not bool(torch.isnan(out).any()), 'NaN left in out'
    if not io['flat']:
        assert _halo_zero(out), 'out halo touched'
        out = out[:, 1:-1, 1:-1]
    og = _np(out)
    obf = io['out'] == 'bf16' and not io['flat']
    _check('out', og, fw['out'], k['out'], obf, fails)
    if fw['mask'] is not None:
        dropped = fw['mask'] == 0
        assert 0 < dropped.sum() < dropped.size
        assert not og[dropped].any(), 'a dropped element is not exactly 0'
        # kept elements equal the scaled reference within the bound (above), and
        # none of those is 0: the zero pattern is the oracle's
        assert (fw['out'][~dropped] != 0).all()
        assert np.array_equal(og == 0, dropped), 'zero pattern differs from oracle.rng'
    if bn:
        _check('mean', _np(g['mean']), fw['mean'], k['mean'], fails=fails)
        _check('rstd', _np(g['rstd']), fw['rstd'], k['rstd'], fails=fails)
        if c['training'] and c['run_mean'] is not None:
            _check('run_mean', _np(g['rm']), fw['run_mean'], k['run_mean'], fails=fails)
            _check('run_var', _np(g['rv']), fw['run_var'], k['run_var'], fails=fails)
        elif c['run_mean'] is not None:      # eval: untouched, bit for bit
            assert np.array_equal(g['rm'].cpu().numpy(), c['run_mean'])
            assert np.array_equal(g['rv'].cpu().numpy(), c['run_var'])
    # ---- backward (batch-statistics form on the kernel's own mean / rstd)
    mean = g['mean'].cpu().numpy() if bn else None
    rstd = g['rstd'].cpu().numpy() if bn else None
    bw = R.block_backward(c['dnext'], fw['P'], fw['slot'], T, F, pt, pf, c['gamma'], mean, rstd,
                          fw['mask'], True)
    dz = g['dz']
    assert not bool(torch.isnan(dz).any()), 'NaN left in dz'
    assert bool(torch.isfinite(dz).all())
    assert _halo_zero(dz), 'dz halo touched'
    dzg = _np(dz[:, 1:-1, 1:-1])
    cov = R.covered(T, F, pt, pf, cm)
    if pt and not cm and (T % pt or F % pf):
        assert (~cov).any()
    assert not dzg[:, ~cov].any(), 'an uncovered pixel has dz != 0'
    _check('dz', dzg, bw['dz'], k['dz'], io['dz'] == 'bf16', fails)
    # (dropout: the reference's dz is built from the oracle's mask, so dz within
    # the bound means the backward drew the forward's mask)
    acc, pre = g['acc'], g['pre']
    _check('dbias', _np(acc['dbias'] - pre['dbias']), bw['dbias'], k['dbias'], fails=fails)
    if bn:
        _check('dgamma', _np(acc['dgamma'] - pre['dgamma']), bw['dgamma'], k['dgamma'], fails=fails)
        _check('dbeta', _np(acc['dbeta'] - pre['dbeta']), bw['dbeta'], k['dbeta'], fails=fails)
    else:
        for n in ('dgamma', 'dbeta'):
            assert torch.equal(acc[n], pre[n])
    if dead is not None:
        # a channel whose P is constant: variance 0, rstd = 1 / sqrt(eps), out = beta
        eps32 = float(np.float32(c['eps']))
        assert not Pg[..., dead].any()
        assert abs(float(g['rstd'][dead]) - eps32 ** -0.5) <= R.MARGIN * k['rstd'] * eps32 ** -0.5
        tol = R.MARGIN * k['out'] * R.scale_of(fw['out']) + 2.0 ** -8 * abs(float(c['beta'][dead]))
        assert float(np.abs(og[..., dead] - float(c['beta'][dead])).max()) <= tol
        assert np.isfinite(dzg[..., dead]).all()
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize('cc', R.GPU_CASES, ids=[cc['id'] for cc in R.GPU_CASES])
def test_block_matches_float64_reference(cc, cuda_dev, monkeypatch):
    c, k, shifted = R.gpu_case(cc)
    print('\n%s (%s variance)' % (cc['id'], 'shifted' if shifted else 'two-pass'))
    g = _run_block(cc, c, cuda_dev, monkeypatch)
    _assert_block(cc, c, k, g, dead=0 if cc['kw'].get('dead_channel') else None)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,F', [(2, 37, 40), (3, 18, 24)])
def test_first_layer_relu_p_given_p_and_aliased_backward(B, T, F, cuda_dev, monkeypatch):
    """asr_vgg_c1_forward_relu_p -> asr_vgg_block_forward_given_p ->
    asr_vgg_block_backward_zdp with z aliased to P, Co = 64 (T = 37 and 18
    leave the last 4-row block of an utterance part-filled).

    P: the float64 3 x 3 stencil over the bf16-rounded features, rounded to
    bf16, then ReLU.  The kernel accumulates in float32 (bias + 9 products, at
    most 18 roundings of magnitudes <= S = |bias| + sum |w x|), so its value may
    land on the other side of a bf16 rounding boundary only where the float64
    value lies within 18 x 2^-24 x S of one: every mismatch must be such an
    element and one bf16 step away; their number is bounded by the count of
    such elements, which the reference predicts (printed).  The batch norm and
    the backward are then held to the block reference on the kernel's own P."""
    N = _N()
    for kk in ('ASR_VGG_ROWS', 'ASR_VGG_POST_FULL', 'ASR_VGG_BNM', 'ASR_VGG_POOL_WALK'):
        monkeypatch.delenv(kk, raising=False)
    dev, Co = cuda_dev, 64
    f32 = dict(dtype=torch.float32, device=dev)
    r = np.random.RandomState(B * 100 + T)
    xs = R.bf16_round(r.randn(B, T, F).astype(np.float32))
    w = (r.randn(Co, 1, 3, 3) * 0.3).astype(np.float32)
    bias = (r.randn(Co) * 0.1).astype(np.float32)
    c = R.make_case(B, T, F, Co, data_seed=T)
    nblk = N.query('asr_vgg_c1_relu_p_blocks', B, T)
    assert nblk == B * ((T + 3) // 4) and T % 4
    P = torch.full((B * T * F, Co), float('nan'), dtype=torch.bfloat16, device=dev)
    mq = torch.full((2, nblk, Co), float('nan'), **f32)
    rm, rv = _dev(c['run_mean'], torch.float32, dev), _dev(c['run_var'], torch.float32, dev)
    xs_d, w_d, b_d = (_dev(a, torch.float32, dev) for a in (xs, w, bias))
    st = N.stream_handle(dev)
    N.call('asr_vgg_c1_forward_relu_p', N.ptr(xs_d), 1, B, T, F, Co, N.ptr(w_d), N.ptr(b_d),
           N.ptr(P), N.ptr(rm), N.ptr(mq[0]), N.ptr(mq[1]), st)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(mq).any())
    v, S = R.conv3x3_c1(xs, w, bias)
    Pref = np.maximum(R.bf16_round(v.astype(np.float32)), 0)
    Pg = P.float().cpu().numpy().reshape(B, T, F, Co)
    assert not np.isnan(Pg).any()
    near = R.bf16_boundary_distance(v) <= 18 * 2.0 ** -24 * S
    mis = R.bf16_bits(Pg) != R.bf16_bits(Pref)
    print('\nc1 P: %d elements, %d within the f32 stencil error of a bf16 boundary, %d differ'
          % (mis.size, int(near.sum()), int(mis.sum())))
    assert not (mis & ~near).any(), 'P differs away from a rounding boundary'
    assert int(mis.sum()) <= int(near.sum()) < mis.size // 100
    step = np.abs(R.bf16_bits(Pg)[mis].astype(np.int64) - R.bf16_bits(Pref)[mis].astype(np.int64))
    assert (step == 1).all(), 'a mismatch is more than one bf16 step'
    # ---- batch norm + apply on the kernel's P, then the aliased backward
    c = dict(c, z=Pg)
    k = R.case_constants(c, shifted=True)
    cc = dict(id='13', io=dict(R.IO), env={}, kw={})
    out = _padded_nan(B, T, F, Co, torch.bfloat16, dev)
    gamma, beta = _dev(c['gamma'], torch.float32, dev), _dev(c['beta'], torch.float32, dev)
    mean, rstd = torch.full((Co,), float('nan'), **f32), torch.full((Co,), float('nan'), **f32)
    nb = N.query('asr_vgg_block_workspace_bytes', B, T, F, Co)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    N.call('asr_vgg_block_forward_given_p', N.ptr(P), B, T, F, Co, N.ptr(gamma), N.ptr(beta),
           N.ptr(rm), N.ptr(rv), 1, c['momentum'], c['eps'], N.ptr(mean), N.ptr(rstd), 0.0, 0,
           N.ptr(out), BF16, 0, N.ptr(mq[0]), N.ptr(mq[1]), nblk, N.ptr(ws), nb, st)
    dn = _dev(R.pad(c['dnext']), torch.bfloat16, dev)
    dz = _padded_nan(B, T, F, Co, torch.bfloat16, dev)
    pre = {n: torch.linspace(-1.0, 2.0, Co, **f32) * s for n, s in
           (('dgamma', 1.0), ('dbeta', -0.5), ('dbias', 3.0))}
    acc = {n: t.clone() for n, t in pre.items()}
    N.call('asr_vgg_block_backward_zdp', N.ptr(dn), BF16, 0, N.ptr(P), BF16, B, T, F, Co, 0, 0, 0,
           N.ptr(P), BF16, None, N.ptr(gamma), N.ptr(mean), N.ptr(rstd), N.ptr(acc['dgamma']),
           N.ptr(acc['dbeta']), 0.0, 0, N.ptr(dz), BF16, N.ptr(acc['dbias']), N.ptr(ws), nb, st)
    torch.cuda.synchronize()
    _assert_block(cc, c, k, dict(P=P, slot=None, out=out, mean=mean, rstd=rstd, rm=rm, rv=rv,
                                 dz=dz, acc=acc, pre=pre))
