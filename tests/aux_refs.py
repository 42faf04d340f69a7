"""float64 references of the auxiliary kernels (losses, decoding, embedding,
cells, column sums, optimizer), the seeded inputs the GPU tests feed them,
and the float32-evaluation error measurements their tolerances come from.

Every reference is plain numpy / torch written from the formulas in
include/asr_hip.h and the kernels' header comments; none calls a project
kernel.  Each takes a torch dtype: float64 is the reference, float32 is "the
same formula evaluated in float32 on the CPU", whose distance from the float64
result is the unit of the transcendental tolerances (measure_f32_errors).
tests/test_aux_refs_cpu.py checks the references against independent torch
implementations; tests/test_aux_kernels_gpu.py compares the kernels with them.
"""
import functools

import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24          # float32 unit roundoff


def gamma(n):
    """Standard summation bound: |fl(sum x_i) - sum x_i| <= gamma_n sum |x_i|."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().to(F64).numpy()


# ----------------------------------------------------------------- xent
def ls_rows(R, T, lens, tgt):
    """LS mask: t < lens[b] for row b*T + t when lens is given, else tgt >= 0
    (all rows without targets)."""
    if lens is not None:
        r = np.arange(R)
        return (r % T) < np.asarray(lens)[r // T]
    if tgt is not None:
        return np.asarray(tgt) >= 0
    return np.ones(R, bool)


def xent(x, tgt, lens, T, ce, ls, g=1.0, dtype=F64):
    """loss = ce * sum_{tgt>=0} (lse - x[tgt]) + ls * sum_{LS rows} -(1/V) sum_v
    (x[v] - lse); a target >= V counts as V - 1.  Returns (loss, d(g*loss)/dx,
    S) with S = the sum of the magnitudes of the loss's terms."""
    xt = _t(x, dtype, True)
    R, V = xt.shape
    lp = torch.log_softmax(xt, -1)
    loss = torch.zeros((), dtype=dtype)
    S = 0.0
    if tgt is not None and ce != 0:
        t = torch.as_tensor(np.asarray(tgt, np.int64))
        nll = -lp.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
        loss = loss + ce * nll[t >= 0].sum()
        S += abs(ce) * float(nll[t >= 0].detach().abs().sum())
    if ls != 0:
        mask = torch.from_numpy(ls_rows(R, T, lens, tgt))
        per = -(lp[mask].sum(-1)) / V
        loss = loss + ls * per.sum()
        S += abs(ls) * float((lp[mask].detach().abs().sum(-1) / V).sum())
    if loss.requires_grad:
        (loss * g).backward()
        dx = _np(xt.grad)
    else:
        dx = np.zeros((R, V))
    return float(loss.detach()), dx, S


def softmax(x, dtype=F64):
    return _np(torch.softmax(_t(x, dtype), -1))


XENT_V = (1, 63, 64, 65, 129, 1000)
XENT_R = (1, 3, 4, 5, 9)
# R -> (T, lens) with R = B * T, a lens[b] of 0 and of T where R allows both
XENT_LENS = {1: (1, [1]), 3: (1, [0, 1, 1]), 4: (2, [0, 2]), 5: (1, [0, 1, 1, 0, 1]),
             9: (3, [0, 3, 2])}
XENT_VARIANTS = ('ce', 'ls_notgt', 'both', 'ignore', 'lens', 'g')


def xent_logits(rng, R, V):
    """Uniform in [-8, 8] (row range <= 16) on a 2^-10 grid, so that x +- 50 is
    exact in float32 and the shifted cases feed the kernel the same numbers."""
    return (np.round(rng.uniform(-8, 8, (R, V)) * 1024) / 1024).astype(np.float32)


@functools.lru_cache(None)
def xent_cases():
    rng = np.random.RandomState(1701)
    out = []
    for V in XENT_V:
        for R in XENT_R:
            x = xent_logits(rng, R, V)
            tgt = rng.randint(0, V, R).astype(np.int64)
            ign = tgt.copy()
            ign[::2] = -1                      # rows 0, 2, ... ignored
            T, lens = XENT_LENS[R]
            lens = np.asarray(lens, np.int32)
            tl = tgt.copy()
            tl[~ls_rows(R, T, lens, None)] = -1
            for var in XENT_VARIANTS:
                c = dict(name='%s-V%d-R%d' % (var, V, R), x=x, tgt=tgt, lens=None, T=0, ce=0.9,
                         ls=0.1, g=1.0)
                if var == 'ce':
                    c.update(ce=1.0, ls=0.0)
                elif var == 'ls_notgt':
                    c.update(tgt=None, ce=0.0, ls=0.25)
                elif var == 'ignore':
                    c.update(tgt=ign)
                elif var == 'lens':
                    c.update(tgt=tl, lens=lens, T=T)
                elif var == 'g':
                    c.update(g=0.37)
                out.append(c)
    return out


def xent_ref(c, dtype=F64):
    return xent(c['x'], c['tgt'], c['lens'], c['T'], c['ce'], c['ls'], c['g'], dtype)


# ---------------------------------------------------------------- cells
def lstm_cell(pre, c_prev, dh, dc, dtype=F64):
    """Gate order i, f, g, o: c = sig(f) c_prev + sig(i) tanh(g), h = sig(o)
    tanh(c).  Returns h, c, act, dpre, dc_prev (cotangents dh, dc; None = 0)."""
    p = _t(pre, dtype, True)
    B, D = p.shape[0], p.shape[1] // 4
    cp = _t(np.zeros((B, D)) if c_prev is None else c_prev, dtype, True)
    i, f, g, o = p.view(B, 4, D).unbind(1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * cp + i * g
    h = o * torch.tanh(c)
    L = torch.zeros((), dtype=dtype)
    if dh is not None:
        L = L + (h * _t(dh, dtype)).sum()
    if dc is not None:
        L = L + (c * _t(dc, dtype)).sum()
    L.backward()
    act = torch.stack([i, f, g, o], 1).reshape(B, 4 * D)
    return _np(h), _np(c), _np(act), _np(p.grad), _np(cp.grad)


def gru_cell(gi, gh, h, dh, dtype=F64):
    """Gate order r, z, n: r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n =
    tanh(gi_n + r gh_n), hout = (1 - z) n + z h.  Returns hout, act, dgi, dgh,
    dh_prev = dh z (the direct term only, as the header defines it)."""
    a, b = _t(gi, dtype, True), _t(gh, dtype, True)
    ht, dht = _t(h, dtype), _t(dh, dtype)
    B, D = ht.shape
    ar, az, an = a.view(B, 3, D).unbind(1)
    br, bz, bn = b.view(B, 3, D).unbind(1)
    r, z = torch.sigmoid(ar + br), torch.sigmoid(az + bz)
    n = torch.tanh(an + r * bn)
    hout = (1 - z) * n + z * ht
    (hout * dht).sum().backward()
    act = torch.stack([r, z, n], 1).reshape(B, 3 * D)
    return _np(hout), _np(act), _np(a.grad), _np(b.grad), _np(dht * z)


CELL_B = (1, 3)
CELL_D = (1, 5, 64, 257)
# (c_prev, dh, dc) given?
LSTM_NULLS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))


@functools.lru_cache(None)
def cell_cases():
    rng = np.random.RandomState(1702)
    out = []
    for B in CELL_B:
        for D in CELL_D:
            f = lambda *s: rng.randn(*s).astype(np.float32)
            u = lambda *s: rng.uniform(-4, 4, s).astype(np.float32)
            out.append(dict(B=B, D=D, pre=u(B, 4 * D), c_prev=f(B, D), dh=f(B, D), dc=f(B, D),
                            gi=u(B, 3 * D) / 2, gh=u(B, 3 * D) / 2, h=f(B, D)))
    return out


def lstm_ref(c, nulls, dtype=F64):
    cp, dh, dc = nulls
    return lstm_cell(c['pre'], c['c_prev'] if cp else None, c['dh'] if dh else None,
                     c['dc'] if dc else None, dtype)


def gru_ref(c, dtype=F64):
    return gru_cell(c['gi'], c['gh'], c['h'], c['dh'], dtype)


# -------------------------------------------------- tanh / add_tanh / add
ELEM_N = (1, 255, 256, 257, 4096 * 256 + 3)


@functools.lru_cache(None)
def elem_cases():
    rng = np.random.RandomState(1703)
    return [dict(n=n, a=rng.uniform(-4, 4, n).astype(np.float32),
                 b=rng.uniform(-2, 2, n).astype(np.float32),
                 dy=rng.randn(n).astype(np.float32)) for n in ELEM_N]


def tanh_fb(x, dy, dtype=F64):
    """y = tanh(x) and dx = dy (1 - y^2)."""
    xt = _t(x, dtype, True)
    y = torch.tanh(xt)
    (y * _t(dy, dtype)).sum().backward()
    return _np(y), _np(xt.grad)


def add_tanh_fb(a, b, dy, dtype=F64):
    at, bt = _t(a, dtype), _t(b, dtype)
    return tanh_fb((at + bt).numpy(), dy, dtype)


# ------------------------------------------------------------ embedding
def embedding_fwd(idx, w):
    """w [V, E]; an index outside [0, V) reads row clamp(idx, 0, V-1)."""
    return w[np.clip(idx, 0, w.shape[0] - 1)]


def embedding_bwd(idx, dout, V, pad, g0):
    """g0 [V, E] + index_add of dout over clamp(idx, 0, V-1), rows of the
    padding token skipped.  Returns (grad, sum of |addends| per element, number
    of addends per token)."""
    rows = np.clip(np.asarray(idx, np.int64).reshape(-1), 0, V - 1)
    keep = rows != (-1 if pad is None else pad)
    r = torch.from_numpy(rows[keep])
    d = torch.from_numpy(np.asarray(dout, np.float64).reshape(len(rows), -1)[keep])
    g = torch.from_numpy(np.asarray(g0, np.float64).copy())
    mag = g.abs().index_add(0, r, d.abs())
    g = g.index_add(0, r, d)
    cnt = np.bincount(rows[keep], minlength=V)
    return g.numpy(), mag.numpy(), cnt


# ------------------------------------------------------------ optimizer
def clip_coef(sqnorm, max_norm, dtype=F64):
    """torch.nn.utils.clip_grad_norm_: max_norm / (||g|| + 1e-6) when < 1."""
    if sqnorm is None or max_norm <= 0:
        return torch.ones((), dtype=dtype)
    c = max_norm / (torch.sqrt(torch.tensor(float(sqnorm), dtype=dtype)) + 1e-6)
    return torch.clamp(c, max=1.0)


def optim_step(kind, p, g, m, v, step, hp, sqnorm, dtype=F64):
    """One step of torch.optim.Adam (kind 0) / SGD (1) / SGD momentum with
    dampening (2) / SGD nesterov (3) on tensors of `dtype`; L2 weight decay is
    added to the (clipped) gradient.  Returns new (p, m, v)."""
    gr = g * clip_coef(sqnorm, hp['max_norm'], dtype) + hp['wd'] * p
    lr = hp['lr']
    if kind == 0:
        b1, b2 = hp['beta1'], hp['beta2']
        m = b1 * m + (1 - b1) * gr
        v = b2 * v + (1 - b2) * gr * gr
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        p = p - (lr / bc1) * m / (torch.sqrt(v) / bc2 ** 0.5 + hp['eps'])
    elif kind == 1:
        p = p - lr * gr
    else:
        m = gr.clone() if step == 1 else hp['momentum'] * m + (1 - hp['dampening']) * gr
        p = p - lr * (gr + hp['momentum'] * m if kind == 3 else m)
    return p, m, v


OPTIM_N = (1, 257, 8192 * 256 + 257)
OPTIM_CLIPS = ('off_zero', 'off_null', 'inactive', 'active')


def _f32(x):
    return float(np.float32(x))


def optim_hp(kind):
    """The hyper-parameters as the C ABI carries them: float32.  The kernel's
    beta2 IS float32(0.999) = 0.99900001287..., and its 1 - beta2 and bias
    corrections follow from that value; a reference run with the decimal 0.999
    is a different optimizer by 1.3e-5 relative in v."""
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, momentum=0.9,
              dampening=0.3 if kind == 2 else 0.0, max_norm=0.0)
    return {k: _f32(v) for k, v in hp.items()}


@functools.lru_cache(None)
def optim_cases():
    """kind x n x clip mode (every mode at the small sizes, 'active' at the
    grid-stride size), three gradients each."""
    rng = np.random.RandomState(1704)
    out = []
    for kind in range(4):
        for n in OPTIM_N:
            for clip in (OPTIM_CLIPS if n < 1000 else ('active',)):
                f = lambda: rng.randn(n).astype(np.float32)
                out.append(dict(kind=kind, n=n, clip=clip, p=f(), g=[f(), f(), f()]))
    return out


def optim_run(c, dtype=F64):
    """Three steps; yields (step, hp, sqnorm, p, m, v) with the state AFTER the
    step.  sqnorm is the float32 value handed to the kernel (None: no norm)."""
    p = _t(c['p'], dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3):
        g = c['g'][step - 1]
        hp = optim_hp(c['kind'])
        sq = np.float32((g.astype(np.float64) ** 2).sum())
        norm = float(np.sqrt(np.float64(sq)))
        hp['max_norm'] = _f32({'off_zero': 0.0, 'off_null': 1.0, 'inactive': 2.0 * norm,
                               'active': 0.5 * norm}[c['clip']])
        sqn = None if c['clip'] == 'off_null' else sq
        p, m, v = optim_step(c['kind'], p, _t(g, dtype), m, v, step, hp, sqn, dtype)
        yield step, hp, sqn, _np(p), _np(m), _np(v)


# ------------------------------------------- float32-evaluation errors
def _err(a32, a64, scale=1.0):
    a64 = np.asarray(a64, np.float64)
    if a64.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(a32, np.float64) - a64))) / scale


def measure_f32_errors():
    """Largest distance of the float32 CPU evaluation of each formula from its
    float64 reference over the inputs of the GPU tests, in the unit each test
    uses (see the constants at the top of test_aux_kernels_gpu.py)."""
    e = dict.fromkeys(('XENT_LOSS', 'XENT_DX', 'SOFTMAX_REL', 'LSTM_FWD', 'LSTM_BWD', 'GRU_FWD',
                       'GRU_BWD', 'TANH_FWD', 'TANH_BWD', 'OPTIM_P', 'OPTIM_M', 'OPTIM_V'), 0.0)

    def up(k, val):
        e[k] = max(e[k], val)

    for c in xent_cases():
        l64, d64, S = xent_ref(c)
        l32, d32, _ = xent_ref(c, F32)
        if S > 0:
            up('XENT_LOSS', abs(l32 - l64) / S)
        up('XENT_DX', _err(d32, d64, abs(c['g']) * (abs(c['ce']) + abs(c['ls']))))
        if c['name'].startswith('ce-'):
            y64 = softmax(c['x'])
            up('SOFTMAX_REL', float(np.max(np.abs(softmax(c['x'], F32) - y64) / y64)))
    for c in cell_cases():
        for nulls in LSTM_NULLS:
            r64, r32 = lstm_ref(c, nulls), lstm_ref(c, nulls, F32)
            up('LSTM_FWD', max(_err(r32[i], r64[i]) for i in range(3)))
            up('LSTM_BWD', max(_err(r32[i], r64[i]) for i in (3, 4)))
        r64, r32 = gru_ref(c), gru_ref(c, F32)
        up('GRU_FWD', max(_err(r32[i], r64[i]) for i in range(2)))
        up('GRU_BWD', max(_err(r32[i], r64[i]) for i in (2, 3, 4)))
    for c in elem_cases():
        for r64, r32 in ((tanh_fb(c['a'], c['dy']), tanh_fb(c['a'], c['dy'], F32)),
                         (add_tanh_fb(c['a'], c['b'], c['dy']),
                          add_tanh_fb(c['a'], c['b'], c['dy'], F32))):
            up('TANH_FWD', _err(r32[0], r64[0]))
            up('TANH_BWD', _err(r32[1], r64[1]))
    for c in optim_cases():
        for s64, s32 in zip(optim_run(c), optim_run(c, F32)):
            for k, i in (('OPTIM_P', 3), ('OPTIM_M', 4), ('OPTIM_V', 5)):
                up(k, _err(s32[i], s64[i]))
    return e
