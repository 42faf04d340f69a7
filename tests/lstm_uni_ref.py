"""Reference of one unidirectional LSTM encoder layer as native_ops.lstm_layer
defines it (LSTMLayerFn over csrc/lstm_uni.hip and the layer GEMMs), written
from the equations in plain torch, dtype-generic, with an explicit backward (no
autograd, no kernel code read).  Nothing here imports the product package;
oracle.rng supplies the dropout mask and tests/rnn_layer_ref.py the input
addressing (gather_rows / scatter_rows / mapped_mask) and the error unit.

The op.  x_src [B, T_src, Dsrc]; row (b, t), t < T, of the layer input X is
x_src[perm[b], t * t_mul + t_add] (with concat followed by the next source
frame: Din = 2 Dsrc), times asr_dropout's mask of x_src (drop = (p, seed)).
nn.LSTM(bidirectional=False) over a packed sequence: gate order i, f, g, o,
h0 = c0 = 0, state and output 0 for t >= lens[b]:
    a = X W_ih^T + b_ih + b_hh + h W_hh^T,
    c' = sig(f) c + sig(i) tanh(g),  h' = sig(o) tanh(c')
Outputs for a cotangent dy [B, T, H] (any value at padded frames: it does not
enter; None: zero): y, dx (x_src's shape, exactly zero at frames no row maps
and at rows of padded frames), dW_ih, dW_hh, db_ih, db_hh (= db_ih).

precision='bf16' is float32 with bf16 mode's roundings (ties to even):
  the recurrence kernels (include/asr_hip.h, asr_lstm_uni_*): h and W_hh in
    h W_hh^T, the gate gradients dG and W_hh in dG W_hh; state, accumulation
    and the cell math stay float32;
  the layer GEMMs, which in bf16 mode round both operands as they load them
    (as for every other layer op): X (after dropout) and W_ih in the input
    projection, dG and W_ih in dX, dG and X in dW_ih, dG and h_prev = y in
    dW_hh.  The bias gradients sum the unrounded dG.

case_constants: max |eval - f64| / max |f64| per tensor of the float32 and of
the bf16-emulated evaluation of this reference, floored at half a float32 eps,
recorded in tests/golden/lstm_uni_constants.json (python tests/lstm_uni_ref.py
--record; tests/test_lstm_uni_ref_cpu.py recomputes them).  A GPU tensor may be
MARGIN x its constant off the float64 values (tests/test_lstm_uni_gpu.py):
MARGIN x the f32 constant in fp32 mode, MARGIN x the larger of the two in bf16
mode -- rnn_layer_ref.py's rule."""
import functools
import json
import os

import numpy as np
import torch

import rnn_layer_ref as R
from oracle import rng

MARGIN = R.MARGIN
CONST_FLOOR = R.CONST_FLOOR
OUT_KEYS = R.OUT_KEYS
DROP_SEED = 0x5EED0777123
CONSTANTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'lstm_uni_constants.json')
nerr = R.nerr


def _rb(a, on):
    return a.to(torch.bfloat16).to(a.dtype) if on else a


def layer(x_src, lens, T, perm, t_mul, t_add, concat, w_ih, w_hh, b_ih, b_hh, dy, drop=None,
          bf16=False):
    """One layer in x_src's dtype: dict of OUT_KEYS (torch).  dy None: zero."""
    B = x_src.shape[0]
    H = w_hh.shape[1]
    perm = np.arange(B) if perm is None else np.asarray(perm)
    lens_t = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    mask = None
    if drop is not None:
        mask = torch.from_numpy(rng.dropout_scale(drop[1], tuple(x_src.shape), drop[0])).to(x_src.dtype)
        x_src = x_src * mask
    X = _rb(R.gather_rows(x_src, perm, t_mul, t_add, T, concat), bf16)
    w_ih_r, w_hh_r = _rb(w_ih, bf16), _rb(w_hh, bf16)
    dy = X.new_zeros(B, T, H) if dy is None else dy
    gx = X @ w_ih_r.t() + (b_ih + b_hh)
    h = X.new_zeros(B, H)
    c = X.new_zeros(B, H)
    y = X.new_zeros(B, T, H)
    saved = []
    for t in range(T):
        a = gx[:, t] + _rb(h, bf16) @ w_hh_r.t()
        i, f = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H])
        g, o = torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c_new = f * c + i * g
        tc = torch.tanh(c_new)
        live = (lens_t > t).to(X.dtype).unsqueeze(1)
        saved.append((h, c, i, f, g, o, tc, live))
        h = o * tc * live
        c = c_new * live
        y[:, t] = h
    dG = torch.zeros_like(gx)      # as the bias sums read it
    dGr = torch.zeros_like(gx)     # as every product reads it
    dw_hh = torch.zeros_like(w_hh)
    dh = X.new_zeros(B, H)
    dc = X.new_zeros(B, H)
    for t in range(T - 1, -1, -1):
        h_prev, c_prev, i, f, g, o, tc, live = saved[t]
        dh_t = (dy[:, t] + dh) * live
        dc_t = dc * live + dh_t * o * (1 - tc * tc)
        d = torch.cat([dc_t * g * i * (1 - i), dc_t * c_prev * f * (1 - f), dc_t * i * (1 - g * g),
                       dh_t * tc * o * (1 - o)], dim=1)
        dG[:, t] = d
        dr = _rb(d, bf16)
        dGr[:, t] = dr
        dw_hh += dr.t() @ _rb(h_prev, bf16)
        dh = dr @ w_hh_r
        dc = dc_t * f
    dx = R.scatter_rows(dGr @ w_ih_r, x_src.shape, perm, t_mul, t_add, T, concat)
    if mask is not None:
        dx = dx * mask
    db = dG.sum(dim=(0, 1))
    return dict(y=y, dx=dx, dW_ih=torch.einsum('btg,btd->gd', dGr, X), dW_hh=dw_hh, db_ih=db,
                db_hh=db.clone())


# --------------------------------------------------------------------------
# cases: the smallest at which the kernels can go wrong.  Forward work-group:
# 4 units x 32 utterances, 4 waves over K = H in slices of 32 (bf16) / 4 (f32);
# backward: 16 units x 16 utterances, 8 waves over K = 4H; H % 8 == 0 takes
# vector fragment loads, any other H guarded scalar ones.
# --------------------------------------------------------------------------
def _c(B, H, T, Din=9, perm=False, t_mul=1, t_add=0, concat=False, drop=0.0, garbage=False):
    return dict(B=B, H=H, T=T, Din=Din, perm=perm, t_mul=t_mul, t_add=t_add, concat=concat,
                drop=drop, garbage=garbage)


CASES = {
    'h1_b3': _c(3, 1, 7),                  # the smallest width; lens [7, 4, 1]
    'h6_b3': _c(3, 6, 7),                  # no multiple of either unit tile, scalar loads
    'h24_b1': _c(1, 24, 7),                # vector loads, not a multiple of the backward's 16
    'h24_b15': _c(15, 24, 7),              # one short of / one past the backward's row tile
    'h24_b17': _c(17, 24, 7),
    'h8_b31': _c(31, 8, 5),                # ... and the forward's
    'h8_b33': _c(33, 8, 5),
    'h40_b3_t1': _c(3, 40, 1),             # T = 1: no recurrent product at all
    'h136_b5': _c(5, 136, 7),              # every wave's K loop runs more than once
    'h24_perm': _c(5, 24, 7, perm=True),
    'h24_sub2': _c(5, 24, 7, perm=True, t_mul=2, t_add=1),
    'h24_concat': _c(5, 24, 7, Din=18, concat=True, t_mul=2),
    'h24_drop': _c(5, 24, 7, drop=0.3),
    'h24_garbage': _c(5, 24, 7, garbage=True),
}


def src_dims(c):
    return R.src_dims(c)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """CPU float32 inputs of a case (never modified): parameters U(+-0.3),
    x = 0.5 N(0, 1), zero at the source frames of padded rows, and a cotangent
    N(0, 1) at every frame, padded ones included; a garbage case has 100 N(0, 1)
    in x and dy at the padded frames."""
    c = CASES[case]
    B, T, H, Din = c['B'], c['T'], c['H'], c['Din']
    g = torch.Generator().manual_seed(sum(map(ord, case)) * 7919 + 29)
    T_src, Dsrc = src_dims(c)
    lens = R.make_lens(B, T)
    perm = torch.randperm(B, generator=g).numpy().astype(np.int32) if c['perm'] else None
    if perm is not None and np.array_equal(perm, np.arange(B)):
        perm = np.roll(perm, 1)                               # never the identity
    u = lambda *s: torch.rand(*s, generator=g) * 0.6 - 0.3     # noqa: E731
    t = dict(w_ih=u(4 * H, Din), w_hh=u(4 * H, H), b_ih=u(4 * H), b_hh=u(4 * H))
    x = 0.5 * torch.randn(B, T_src, Dsrc, generator=g)
    pm = np.arange(B) if perm is None else perm
    live = R.mapped_mask(x.shape, lens, pm, c['t_mul'], c['t_add'], T, c['concat'])
    full = R.mapped_mask(x.shape, np.full(B, T), pm, c['t_mul'], c['t_add'], T, c['concat'])
    pad = torch.from_numpy(full & ~live)
    x[pad] = 100.0 * torch.randn(int(pad.sum()), Dsrc, generator=g) if c['garbage'] else 0.0
    dy = torch.randn(B, T, H, generator=g)
    if c['garbage']:
        for b, n in enumerate(lens):
            dy[b, n:] *= 100.0
    t.update(x=x, dy=dy, lens=lens, perm=perm)
    return t


def drop_of(c):
    return (c['drop'], DROP_SEED) if c['drop'] else None


def evaluate(case, dtype=torch.float64, precision=None):
    """{tensor name: float64 numpy array} of a case evaluated in `dtype`
    (precision='bf16': float32 with bf16 mode's roundings)."""
    c = CASES[case]
    inp = case_inputs(case)
    t = {k: v.to(dtype) for k, v in inp.items() if torch.is_tensor(v)}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)          # one summation order whatever the machine
    try:
        out = layer(t['x'], inp['lens'], c['T'], inp['perm'], c['t_mul'], c['t_add'], c['concat'],
                    t['w_ih'], t['w_hh'], t['b_ih'], t['b_hh'], t['dy'], drop_of(c),
                    bf16=precision == 'bf16')
    finally:
        torch.set_num_threads(nt)
    return {k: v.double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 tensors of a case, computed once."""
    return evaluate(case)


def measure_constants(case):
    """{'f32' | 'bf16': {tensor: constant}} recomputed from the reference."""
    ref = reference(case)
    evs = {'f32': evaluate(case, torch.float32), 'bf16': evaluate(case, torch.float32, 'bf16')}
    return {m: {k: max(nerr(e[k], ref[k]), CONST_FLOOR) for k in ref} for m, e in evs.items()}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(CONSTANTS_JSON) as f:
        return json.load(f)


def case_constants(case):
    """({tensor: f32 constant}, {tensor: bf16-emulated constant}) in nerr
    units, floored at half a float32 eps: the recorded table."""
    rec = _recorded()[case]
    return dict(rec['f32']), dict(rec['bf16'])


def bounds(case, precision):
    """{tensor: largest nerr a GPU tensor of this case may have}."""
    cf, cb = case_constants(case)
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
