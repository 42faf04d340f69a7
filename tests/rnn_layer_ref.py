"""Reference of one bidirectional recurrent encoder layer as native_ops defines
it (blstm_layer / bgru_layer: BLSTMLayerFn, BGRULayerFn over csrc/lstm*.hip,
gru.hip and the layer GEMMs), written from the equations in plain torch,
dtype-generic, with an explicit backward (no autograd, no kernel code read).
Nothing here imports the product package; oracle.rng supplies the dropout mask.

The op.  x_src [B, T_src, Dsrc]; row (b, t), t < T, of the layer input X is
x_src[perm[b], t * t_mul + t_add] (with concat followed by the next source
frame: Din = 2 Dsrc), times asr_dropout's mask of x_src (drop = (p, seed)).
Parameters are the combined [forward; reverse] tensors.  Packed-sequence
semantics: state and output are 0 for t >= lens[b]; the reverse direction
starts at each utterance's own last frame.
  LSTM (gate order i, f, g, o):  a = X W_ih^T + b_ih + b_hh + h W_hh^T,
      c' = sig(f) c + sig(i) tanh(g),  h' = sig(o) tanh(c')
  GRU (gate order r, z, n):  r = sig(gx_r + gh_r), z = sig(gx_z + gh_z),
      n = tanh(gx_n + r gh_n), h' = (1 - z) n + z h,
      gx = X W_ih^T + b_ih, gh = h W_hh^T + b_hh
Outputs for a cotangent dy [B, T, 2H] (any value at padded frames: it does not
enter): y, dx (x_src's shape, exactly zero at frames no row maps and at rows of
padded frames), dW_ih, dW_hh, db_ih, db_hh.

precision='bf16' rounds to bf16 (ties to even) the operands of every product
the bf16 paths feed from bf16, float32 elsewhere:
  LSTM: X (after dropout) and W_ih; h and W_hh in the recurrence; the gate
    gradients dG wherever a product reads them (dG W_hh, dG W_ih, dG^T X,
    dG^T h_prev) and h_prev = y in dW_hh; the bias gradients sum the unrounded
    dG.  packed=True (the fused forward's fp16 gate activations, lstm_xg.hip
    enc_sig / enc_tanh): the backward reads each sigmoid gate s as fp16(s)
    below 0.5 and as fp16(-(1 - s)) from there on, the tanh gate g as fp16(g)
    up to |g| = 0.499 and as fp16(sign(g) (1 - |g|) 2^14) beyond, and forms
    s, 1 - s, g, 1 - g^2 from the stored value.
  GRU: the recurrence is float32; the GEMMs round X, W_ih, dgx, dgh and
    h_prev = y.
(The one-bit step tag the tagged-granule hand-off keeps in the LSB of one bf16
in four is not modelled: it moves h by at most one bf16 ulp where rounding
already moves it by half.)

case_constants: max |eval - f64| / max |f64| per tensor of the float32 and of
the bf16-emulated evaluation of this reference, floored at half a float32 eps,
recorded in tests/golden/rnn_layer_constants.json (python tests/rnn_layer_ref.py
--record; tests/test_rnn_layer_ref_cpu.py recomputes them).  A GPU tensor may
be MARGIN x its constant off the float64 values (tests/test_rnn_layer_gpu.py)."""
import functools
import json
import os

import numpy as np
import torch

from oracle import rng

F32_EPS = float(np.finfo(np.float32).eps)
CONST_FLOOR = F32_EPS / 2
MARGIN = 16.0          # attdec_ref.MARGIN, the auxiliary-kernel tests
OUT_KEYS = ('y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh')
DROP_SEED = 0x5EED0123456
HANDOFF_SEED = 0x5EED0654321
CONSTANTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'rnn_layer_constants.json')


# --------------------------------------------------------------------------
# roundings
# --------------------------------------------------------------------------
class _Emu:
    """Where an evaluation rounds: nowhere (float64, float32) or as bf16 mode."""

    def __init__(self, bf16=False, packed=False):
        self.bf16, self.packed = bf16, bf16 and packed

    def rb(self, a):
        return a.to(torch.bfloat16).to(a.dtype) if self.bf16 else a


def _h16(a):
    return a.to(torch.float16).to(a.dtype)


def pack_sigmoid(s):
    """(s, 1 - s) as the backward decodes them from the packed fp16 gate."""
    e = _h16(torch.where(s < 0.5, s, -(1 - s)))
    neg = torch.signbit(e)                         # -0 (s == 1) included
    return torch.where(neg, 1 + e, e), torch.where(neg, -e, 1 - e)


def pack_tanh(g):
    """(g, 1 - g^2) as the backward decodes them from the packed fp16 gate."""
    a = g.abs()
    comp = torch.copysign(torch.clamp_min(1 - a, 2.0 ** -15) * 16384.0, g)
    e = _h16(torch.where(a <= 0.499, g, comp))
    c = e.abs() / 16384.0
    cm = e.abs() >= 0.5
    return torch.where(cm, torch.copysign(1 - c, e), e), torch.where(cm, c * (2 - c), 1 - e * e)


# --------------------------------------------------------------------------
# input addressing
# --------------------------------------------------------------------------
def source_frames(T, t_mul, t_add):
    return np.arange(T) * t_mul + t_add


def gather_rows(x_src, perm, t_mul, t_add, T, concat):
    """X [B, T, Din] from x_src [B, T_src, Dsrc]."""
    f = torch.as_tensor(source_frames(T, t_mul, t_add))
    xs = x_src[torch.as_tensor(np.asarray(perm), dtype=torch.long)]
    return torch.cat([xs[:, f], xs[:, f + 1]], dim=2) if concat else xs[:, f]


def scatter_rows(dX, shape, perm, t_mul, t_add, T, concat):
    """The adjoint of gather_rows: dX [B, T, Din] added into zeros(shape)."""
    out = dX.new_zeros(shape)
    Dsrc = shape[2]
    b = torch.as_tensor(np.asarray(perm), dtype=torch.long).unsqueeze(1)
    f = torch.as_tensor(source_frames(T, t_mul, t_add)).unsqueeze(0)
    out.index_put_((b, f), dX[..., :Dsrc], accumulate=True)
    if concat:
        out.index_put_((b, f + 1), dX[..., Dsrc:], accumulate=True)
    return out


def mapped_mask(shape, lens, perm, t_mul, t_add, T, concat):
    """bool [B, T_src]: source frames some row (b, t < lens[b]) reads."""
    m = np.zeros(shape[:2], bool)
    for b, n in enumerate(np.asarray(lens)):
        f = source_frames(int(n), t_mul, t_add)
        m[perm[b], f] = True
        if concat:
            m[perm[b], f + 1] = True
    return m


# --------------------------------------------------------------------------
# one direction, forward and backward through time
# --------------------------------------------------------------------------
def _steps(T, reverse):
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


def _live(lens, t, like):
    return (torch.as_tensor(np.asarray(lens), dtype=torch.long) > t).to(like.dtype).unsqueeze(1)


def lstm_direction(Xr, lens, w_ih_r, w_hh_r, b_ih, b_hh, reverse, dy, emu):
    """Xr, w_ih_r, w_hh_r: the operands as the products read them (rounded by
    the caller in bf16 mode).  Returns y, dX, dW_ih, dW_hh, db."""
    B, T, _ = Xr.shape
    H = w_hh_r.shape[1]
    gx = Xr @ w_ih_r.t() + (b_ih + b_hh)
    h = Xr.new_zeros(B, H)
    c = Xr.new_zeros(B, H)
    y = Xr.new_zeros(B, T, H)
    saved = [None] * T
    order = _steps(T, reverse)
    for t in order:
        a = gx[:, t] + emu.rb(h) @ w_hh_r.t()
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        g = torch.tanh(a[:, 2 * H:3 * H])
        c_new = f * c + i * g
        tc = torch.tanh(c_new)
        live = _live(lens, t, Xr)
        saved[t] = (h, c, i, f, g, o, tc, live)
        h = o * tc * live
        c = c_new * live
        y[:, t] = h
    dG = torch.zeros_like(gx)
    dGr = torch.zeros_like(gx)
    dw_hh = torch.zeros_like(w_hh_r)
    dh = Xr.new_zeros(B, H)
    dc = Xr.new_zeros(B, H)
    for t in reversed(order):
        h_prev, c_prev, i, f, g, o, tc, live = saved[t]
        if emu.packed:
            (i, omi), (f, omf), (o, omo) = pack_sigmoid(i), pack_sigmoid(f), pack_sigmoid(o)
            g, omg = pack_tanh(g)
        else:
            omi, omf, omo, omg = 1 - i, 1 - f, 1 - o, 1 - g * g
        dh_t = (dy[:, t] + dh) * live
        dc_t = dc * live + dh_t * o * (1 - tc * tc)
        d = torch.cat([dc_t * g * i * omi, dc_t * c_prev * f * omf, dc_t * i * omg,
                       dh_t * tc * o * omo], dim=1)
        dG[:, t] = d
        dr = emu.rb(d)
        dGr[:, t] = dr
        dw_hh += dr.t() @ emu.rb(h_prev)
        dh = dr @ w_hh_r
        dc = dc_t * f
    return (y, dGr @ w_ih_r, torch.einsum('btg,btd->gd', dGr, Xr), dw_hh, dG.sum(dim=(0, 1)))


def gru_direction(Xr, lens, w_ih_r, w_hh, b_ih, b_hh, reverse, dy, emu):
    """The recurrent products h W_hh^T and dgh W_hh are never rounded.
    Returns y, dX, dW_ih, dW_hh, db_ih, db_hh."""
    B, T, _ = Xr.shape
    H = w_hh.shape[1]
    gx = Xr @ w_ih_r.t() + b_ih
    h = Xr.new_zeros(B, H)
    y = Xr.new_zeros(B, T, H)
    saved = [None] * T
    order = _steps(T, reverse)
    for t in order:
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, t, H:2 * H] + gh[:, H:2 * H])
        ghn = gh[:, 2 * H:]
        n = torch.tanh(gx[:, t, 2 * H:] + r * ghn)
        live = _live(lens, t, Xr)
        saved[t] = (h, r, z, n, ghn, live)
        h = ((1 - z) * n + z * h) * live
        y[:, t] = h
    dgx = torch.zeros_like(gx)
    dgh = torch.zeros_like(gx)
    dw_hh = torch.zeros_like(w_hh)
    carry = Xr.new_zeros(B, H)
    for t in reversed(order):
        h_prev, r, z, n, ghn, live = saved[t]
        dh = (dy[:, t] + carry) * live
        dpn = dh * (1 - z) * (1 - n * n)
        dpz = dh * (h_prev - n) * z * (1 - z)
        dpr = dpn * ghn * r * (1 - r)
        dgx[:, t] = torch.cat([dpr, dpz, dpn], dim=1)
        dh_gates = torch.cat([dpr, dpz, dpn * r], dim=1)
        dgh[:, t] = dh_gates
        dw_hh += emu.rb(dh_gates).t() @ emu.rb(h_prev)
        carry = dh_gates @ w_hh + dh * z
    dgxr = emu.rb(dgx)
    return (y, dgxr @ w_ih_r, torch.einsum('btg,btd->gd', dgxr, Xr), dw_hh,
            dgx.sum(dim=(0, 1)), dgh.sum(dim=(0, 1)))


def layer(kind, x_src, lens, T, perm, t_mul, t_add, concat, w_ih, w_hh, b_ih, b_hh, dy, drop=None,
          emu=None):
    """One layer, both directions, in x_src's dtype: dict of OUT_KEYS (torch)."""
    emu = emu or _Emu()
    B = x_src.shape[0]
    perm = np.arange(B) if perm is None else np.asarray(perm)
    mask = None
    if drop is not None:
        mask = torch.from_numpy(rng.dropout_scale(drop[1], tuple(x_src.shape), drop[0])).to(x_src.dtype)
        x_src = x_src * mask
    Xr = emu.rb(gather_rows(x_src, perm, t_mul, t_add, T, concat))
    w_ih_r = emu.rb(w_ih)
    ng = 4 if kind == 'lstm' else 3
    H = w_hh.shape[1]
    outs = []
    for d, rev in enumerate((False, True)):
        g, hs = slice(d * ng * H, (d + 1) * ng * H), slice(d * H, (d + 1) * H)
        if kind == 'lstm':
            o = lstm_direction(Xr, lens, w_ih_r[g], emu.rb(w_hh[g]), b_ih[g], b_hh[g], rev,
                               dy[:, :, hs], emu)
            o = o + (o[4],)
        else:
            o = gru_direction(Xr, lens, w_ih_r[g], w_hh[g], b_ih[g], b_hh[g], rev, dy[:, :, hs], emu)
        outs.append(o)
    dx = scatter_rows(outs[0][1] + outs[1][1], x_src.shape, perm, t_mul, t_add, T, concat)
    if mask is not None:
        dx = dx * mask
    res = dict(y=torch.cat([outs[0][0], outs[1][0]], dim=2), dx=dx)
    for k, name in enumerate(OUT_KEYS[2:], start=2):
        res[name] = torch.cat([outs[0][k], outs[1][k]], dim=0)
    return res


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def _c(kind, B, H, T, Din=24, perm=False, t_mul=1, t_add=0, concat=False, drop=0.0, garbage=False,
       stack=False):
    return dict(kind=kind, B=B, H=H, T=T, Din=Din, perm=perm, t_mul=t_mul, t_add=t_add,
                concat=concat, drop=drop, garbage=garbage, stack=stack)


_PERM2 = dict(perm=True, t_mul=2, t_add=1)
_CONCAT2 = dict(concat=True, t_mul=2)
CASES = {}
for _B, _H in ((9, 64), (17, 96), (8, 128), (20, 96), (33, 160), (33, 40), (17, 72), (5, 6), (18, 36),
               (7, 128), (33, 96), (17, 40)):
    CASES['l_b%dh%d' % (_B, _H)] = _c('lstm', _B, _H, 13)
CASES.update({
    'l_b5h6_t1': _c('lstm', 5, 6, 1),
    'l_b9h64_perm2': _c('lstm', 9, 64, 13, **_PERM2),
    'l_b9h64_concat2': _c('lstm', 9, 64, 13, **_CONCAT2),
    'l_b9h64_din13': _c('lstm', 9, 64, 13, Din=13),
    'l_b9h64_drop': _c('lstm', 9, 64, 13, drop=0.3),
    'l_b9h64_t24': _c('lstm', 9, 64, 24),
    # beyond T = 24: the split input gradient's row bands (_dx_bands) start at T = 64
    'l_b9h64_t64': _c('lstm', 9, 64, 64),
    'l_b9h64_garbage': _c('lstm', 9, 64, 13, garbage=True),
    'l_b18h36_perm2': _c('lstm', 18, 36, 13, **_PERM2),
    'l_b9h64_stack': _c('lstm', 9, 64, 13, stack=True),
})
for _B, _H in ((5, 6), (17, 20), (33, 50), (20, 96)):
    CASES['g_b%dh%d' % (_B, _H)] = _c('gru', _B, _H, 9)
CASES.update({
    'g_b5h6_t1': _c('gru', 5, 6, 1),
    'g_b33h50_perm2': _c('gru', 33, 50, 9, **_PERM2),
    'g_b33h50_concat2': _c('gru', 33, 50, 9, **_CONCAT2),
})
STACK_KEYS = ('y', 'dx') + tuple(k + s for s in ('', '2') for k in OUT_KEYS[2:])


def make_lens(B, T):
    """Descending, lens[0] = T, the last utterance one frame long."""
    return np.linspace(T, 1, B).astype(np.int32) if B > 1 else np.array([T], np.int32)


def src_dims(c):
    """(T_src, Dsrc): a non-identity map leaves source frames no row reads."""
    Dsrc = c['Din'] // 2 if c['concat'] else c['Din']
    ident = not c['perm'] and not c['concat'] and c['t_mul'] == 1 and c['t_add'] == 0
    return (c['T'] if ident else c['t_mul'] * c['T'] + 1), Dsrc


def _params(g, kind, H, Din):
    ng = 8 if kind == 'lstm' else 6
    u = lambda *s: torch.rand(*s, generator=g) * 0.2 - 0.1     # noqa: E731
    return dict(w_ih=u(ng * H, Din), w_hh=u(ng * H, H), b_ih=u(ng * H), b_hh=u(ng * H))


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """CPU float32 inputs of a case (never modified): parameters U(+-0.1),
    x = 0.5 N(0, 1) -- zero at the source frames of padded rows unless the case
    keeps garbage there -- and a cotangent N(0, 1) at every frame."""
    c = CASES[case]
    B, T, H, Din = c['B'], c['T'], c['H'], c['Din']
    g = torch.Generator().manual_seed(sum(map(ord, case)) * 7919 + 11)
    T_src, Dsrc = src_dims(c)
    lens = make_lens(B, T)
    perm = torch.randperm(B, generator=g).numpy().astype(np.int32) if c['perm'] else None
    t = _params(g, c['kind'], H, Din)
    x = 0.5 * torch.randn(B, T_src, Dsrc, generator=g)
    live = mapped_mask(x.shape, lens, np.arange(B) if perm is None else perm, c['t_mul'],
                       c['t_add'], T, c['concat'])
    full = mapped_mask(x.shape, np.full(B, T), np.arange(B) if perm is None else perm, c['t_mul'],
                       c['t_add'], T, c['concat'])
    pad = torch.from_numpy(full & ~live)
    x[pad] = 100.0 * torch.randn(int(pad.sum()), Dsrc, generator=g) if c['garbage'] else 0.0
    t.update(x=x, dy=torch.randn(B, T, 2 * H, generator=g), lens=lens, perm=perm)
    if c['stack']:
        t.update({k + '2': v for k, v in _params(g, c['kind'], H, 2 * H).items()})
    return t


def _drop(c):
    return (c['drop'], DROP_SEED) if c['drop'] else None


def evaluate(case, dtype=torch.float64, precision=None, packed=False):
    """{tensor name: float64 numpy array} of a case evaluated in `dtype`
    (precision='bf16': float32 with the bf16 paths' roundings; packed: and the
    fp16 gate activations).  A stack case composes the layer twice: layer 2
    reads dropout(y1) (HANDOFF_SEED, p = 0.2) and its dx is layer 1's dy."""
    c = CASES[case]
    inp = case_inputs(case)
    emu = _Emu(precision == 'bf16', packed)
    t = {k: v.to(dtype) for k, v in inp.items() if torch.is_tensor(v)}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)          # one summation order whatever the machine
    try:
        args = (c['kind'], t['x'], inp['lens'], c['T'], inp['perm'], c['t_mul'], c['t_add'], c['concat'],
                t['w_ih'], t['w_hh'], t['b_ih'], t['b_hh'])
        if not c['stack']:
            out = layer(*args, t['dy'], _drop(c), emu)
        else:
            y1 = layer(*args, torch.zeros_like(t['dy']), _drop(c), emu)['y']
            o2 = layer(c['kind'], y1, inp['lens'], c['T'], None, 1, 0, False, t['w_ih2'], t['w_hh2'],
                       t['b_ih2'], t['b_hh2'], t['dy'], (0.2, HANDOFF_SEED), emu)
            out = layer(*args, o2['dx'], _drop(c), emu)
            out['y'] = o2['y']
            out.update({k + '2': o2[k] for k in OUT_KEYS[2:]})
    finally:
        torch.set_num_threads(nt)
    return {k: v.double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 tensors of a case, computed once."""
    return evaluate(case)


def nerr(got, ref):
    """max |got - ref| / max |ref|: the unit of every bound here."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


def measure_constants(case):
    """{'f32' | 'bf16' | 'bf16p': {tensor: constant}} recomputed from the
    reference ('bf16p', packed activations: BLSTM cases only)."""
    ref = reference(case)
    evs = {'f32': evaluate(case, torch.float32), 'bf16': evaluate(case, torch.float32, 'bf16')}
    if CASES[case]['kind'] == 'lstm':
        evs['bf16p'] = evaluate(case, torch.float32, 'bf16', packed=True)
    return {m: {k: max(nerr(e[k], ref[k]), CONST_FLOOR) for k in ref} for m, e in evs.items()}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(CONSTANTS_JSON) as f:
        return json.load(f)


def case_constants(case, packed=False):
    """({tensor: f32 constant}, {tensor: bf16-emulated constant}) in nerr units,
    floored at half a float32 eps: the recorded table.  The GPU bound on a
    tensor is MARGIN x the f32 constant in fp32 mode, MARGIN x the larger of
    the two in bf16 mode."""
    rec = _recorded()[case]
    return dict(rec['f32']), dict(rec['bf16p' if packed else 'bf16'])


# --------------------------------------------------------------------------
# which implementation a BLSTM call takes (lstm.hip asr_lstm_forward /
# lstm_backward_impl, lstm_xg.hip xg_rows / xg32_shape_ok / lstm_fwd_xgx_launch
# behind asr_lstm_forward_x_ok, lstm_persist.hip) on a device of 256 CUs whose
# occupancy queries admit every instantiation, as the MI355X's do
# --------------------------------------------------------------------------
NCU = 256
ENV_KEYS = ('ASR_LSTM_XG', 'ASR_LSTM_PERSIST', 'ASR_LSTM_XG32', 'ASR_XG_LOCAL', 'ASR_FUSE_XPROJ',
            'ASR_XG_ACT_H', 'ASR_BIAS_FUSED', 'ASR_XG_BWD_XU')
IMPLEMENTATIONS = ('fwd_xgx_packed', 'fwd_xgx_f32act', 'fwd_xg', 'fwd_counter', 'fwd_step_fast1',
                   'fwd_step_fast2', 'fwd_step_vec1', 'fwd_step_vec0', 'fwd_xg32', 'fwd_step_f32',
                   'bwd_xg_packed', 'bwd_xg', 'bwd_xg_xu32', 'bwd_xg_colsum', 'bwd_counter',
                   'bwd_step_fast1', 'bwd_step_fast2', 'bwd_step_fast4', 'bwd_step_vec1',
                   'bwd_step_vec0', 'bwd_xg32', 'bwd_step_f32', 'write_through')


def _cd(a, b):
    return -(-a // b)


def xg_rows(B, H):
    if H % 32 or H // 16 > 64:
        return 0
    for R in (8, 16):
        if 2 * _cd(B, R) * (H // 16) <= NCU:
            return R
    return 0


def staged_width(c, precision):
    """Columns of the staged bf16 input (zero-padded to a multiple of 8 unless
    the dropout is fused into the staging)."""
    Din = c['Din']
    fused_drop = bool(c['drop']) and not c['concat']
    return _cd(Din, 8) * 8 if precision == 'bf16' and Din % 8 and not fused_drop else Din


def expected_path(case, precision, env):
    """dict(fwd, bwd: asr_lstm_last_path's values -- 0 per-step, 1 tagged-granule
    bf16, 2 tagged-granule f32, 3 tagged-granule bf16 with the fused projection,
    4 counter form; packed: fp16 gate activations; impl: the IMPLEMENTATIONS the
    call reaches).  None for a GRU case (one implementation)."""
    c = CASES[case]
    if c['kind'] != 'lstm':
        return None
    B, H = c['B'], c['H']
    on = lambda k: env.get(k, '1') != '0'      # noqa: E731
    xg = on('ASR_LSTM_XG') and on('ASR_LSTM_PERSIST')
    R = xg_rows(B, H)
    impl = []
    packed = False
    if precision == 'bf16':
        Dp = staged_width(c, precision)
        fused = (xg and on('ASR_FUSE_XPROJ') and R == 8 and Dp % 8 == 0 and Dp <= 1024
                 and _cd(_cd(Dp, 32), 6) <= 6 and _cd(H // 32, 4) <= 4)
        if fused:
            fwd, packed = 3, on('ASR_XG_ACT_H')
            impl.append('fwd_xgx_packed' if packed else 'fwd_xgx_f32act')
        elif xg and R and _cd(H // 32, 4) <= 8:
            fwd = 1
            impl.append('fwd_xg')
        elif (on('ASR_LSTM_PERSIST') and H % 32 == 0 and (H // 8) * 2 * _cd(B, 16) <= NCU
              and _cd(H // 32, 4) <= 8):
            fwd = 4
            impl.append('fwd_counter')
        else:
            fwd = 0
            nks = H // 32
            impl.append('fwd_step_fast%d' % (1 if nks <= 4 else 2 if nks <= 8 else 4)
                        if H % 32 == 0 else 'fwd_step_vec%d' % (H % 8 == 0))
        xu = 32 if env.get('ASR_XG_BWD_XU') == '32' and R == 8 and _cd(H // 16, 4) <= 8 else 16
        if xg and R and _cd(H // 16, xu // 4) <= 16:
            bwd = 1
            impl.append('bwd_xg_packed' if packed else
                        'bwd_xg' if on('ASR_BIAS_FUSED') else 'bwd_xg_colsum')
            if xu == 32:
                impl.append('bwd_xg_xu32')
        elif (on('ASR_LSTM_PERSIST') and H % 32 == 0 and (H // 16) * 2 * _cd(B, 16) <= NCU
              and _cd(H // 8, 8) <= 16):
            bwd = 4
            impl.append('bwd_counter')
        else:
            bwd = 0
            nks = H // 8
            impl.append('bwd_step_fast%d' % (1 if nks <= 8 else 2 if nks <= 16 else 4)
                        if H % 32 == 0 else 'bwd_step_vec%d' % (H % 8 == 0))
        if (fwd in (1, 3) or bwd == 1) and not on('ASR_XG_LOCAL'):
            impl.append('write_through')
    else:
        xg32 = xg and on('ASR_LSTM_XG32') and R and H % 64 == 0
        fwd = 2 if xg32 and H <= 512 else 0
        bwd = 2 if xg32 and H <= 384 else 0
        impl += ['fwd_xg32' if fwd else 'fwd_step_f32', 'bwd_xg32' if bwd else 'bwd_step_f32']
    return dict(fwd=fwd, bwd=bwd, packed=packed, impl=tuple(impl))


# --------------------------------------------------------------------------
# the GPU table: (case, precision, dispatch)
# --------------------------------------------------------------------------
DISPATCH = {
    'default': {},
    'act_f32': {'ASR_XG_ACT_H': '0'},
    'gemm_first': {'ASR_FUSE_XPROJ': '0'},
    'colsum': {'ASR_FUSE_XPROJ': '0', 'ASR_BIAS_FUSED': '0'},
    'xu32': {'ASR_XG_BWD_XU': '32'},
    'write_through': {'ASR_XG_LOCAL': '0'},
    'counter': {'ASR_LSTM_XG': '0'},
    'perstep': {'ASR_LSTM_PERSIST': '0'},
    'xg32_off': {'ASR_LSTM_XG32': '0'},
}
_L = 'l_b%dh%d'
_OPTION_CASES = ('perm2', 'concat2', 'din13', 'drop', 't24', 'garbage')


def _gpu_table():
    rows = []
    add = lambda shapes, prec, disp: rows.extend((_L % s, prec, disp) for s in shapes)   # noqa: E731
    add([(9, 64), (17, 96), (8, 128)], 'bf16', 'default')
    add([(9, 64)], 'bf16', 'act_f32')
    add([(9, 64), (17, 96)], 'bf16', 'gemm_first')
    add([(9, 64)], 'bf16', 'colsum')
    add([(9, 64), (8, 128)], 'bf16', 'xu32')
    add([(9, 64)], 'bf16', 'write_through')
    add([(9, 64), (20, 96)], 'bf16', 'counter')
    # (17, 96): the backward's fast_ks = 2 template (H = 96, 128), which the
    # shapes (9, 64) and (33, 160) leave out
    add([(9, 64), (17, 96), (33, 160)], 'bf16', 'perstep')
    add([(33, 40), (17, 72), (5, 6), (18, 36)], 'bf16', 'default')
    rows.append(('l_b5h6_t1', 'bf16', 'default'))
    add([(9, 64), (7, 128)], 'fp32', 'default')
    add([(9, 64)], 'fp32', 'xg32_off')
    add([(33, 96), (18, 36), (17, 40)], 'fp32', 'default')
    for o in _OPTION_CASES:
        rows += [('l_b9h64_' + o, 'bf16', 'default'), ('l_b9h64_' + o, 'fp32', 'default')]
    rows += [('l_b9h64_t64', 'bf16', 'default'), ('l_b18h36_perm2', 'bf16', 'default'),
             ('l_b9h64_stack', 'bf16', 'default')]
    for case in CASES:
        if CASES[case]['kind'] == 'gru':
            rows += [(case, 'fp32', 'default'), (case, 'bf16', 'default')]
    return rows


GPU_TABLE = _gpu_table()


def bounds(case, precision, dispatch):
    """{tensor: largest nerr a GPU tensor of this row may have}."""
    path = expected_path(case, precision, DISPATCH[dispatch])
    cf, cb = case_constants(case, bool(path and path['packed']))
    if precision == 'fp32':
        return {k: MARGIN * cf[k] for k in cf}
    return {k: MARGIN * max(cf[k], cb[k]) for k in cf}


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['--record']:
        table = {case: measure_constants(case) for case in CASES}
        with open(CONSTANTS_JSON, 'w') as f:
            json.dump(table, f, indent=0, sort_keys=True)
            f.write('\n')
        print('recorded', len(table), 'cases in', CONSTANTS_JSON)
