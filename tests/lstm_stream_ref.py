"""Reference of the stateful (streaming) unidirectional LSTM recurrence,
asr_lstm_stream_forward (include/asr_hip.h, csrc/lstm_stream.hip), written from
the equations in plain torch, dtype-generic; no kernel code read, nothing here
imports the product package.

One chunk.  gx [B, Tc, 4H] = x W_ih^T + b_ih + b_hh (gate order i, f, g, o),
lens [B] the chunk's valid frames per row, (h, c) [B, H] the state before it:
    a = gx[:, t] + h W_hh^T,  c' = sig(f) c + sig(i) tanh(g),  h' = sig(o) tanh(c')
for t < lens[b]; for t >= lens[b] the output is 0 and the state is FROZEN (the
whole-utterance layer of tests/lstm_uni_ref.py zeroes it), so the state after
the chunk is the one after frame lens[b] - 1, and the input state itself where
lens[b] == 0.  run_schedule feeds an utterance of T frames as chunks of the
given sizes (a size 0: a chunk of one padded frame in which no row has a
frame) and concatenates the outputs.

precision='bf16' is float32 with bf16 mode's roundings (ties to even), the rule
of tests/lstm_uni_ref.py for the recurrence: h and W_hh in h W_hh^T; state,
sums and the cell math stay float32.

case_constants: max |eval - f64| / max |f64| per tensor (y, h, c) of the
float32 and of the bf16-emulated evaluation of the single-chunk schedule,
floored at half a float32 eps, recorded in tests/golden/lstm_stream_constants.json
(python tests/lstm_stream_ref.py --record; tests/test_lstm_stream_ref_cpu.py
recomputes them).  A GPU tensor may be MARGIN x its constant off the float64
values: MARGIN x the f32 constant in fp32 mode, MARGIN x the larger of the two
in bf16 mode -- rnn_layer_ref.py's rule."""
import functools
import json
import os

import numpy as np
import torch

import rnn_layer_ref as R

MARGIN = R.MARGIN
CONST_FLOOR = R.CONST_FLOOR
OUT_KEYS = ('y', 'h', 'c')
CONSTANTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'lstm_stream_constants.json')
nerr = R.nerr
T = 7
SCHEDULES = {'whole': [7], 'ones': [1] * 7, 'three_four': [3, 4], 'two_zero_five': [2, 0, 5]}


def _rb(a, on):
    return a.to(torch.bfloat16).to(a.dtype) if on else a


def run_chunk(gx, w_hh, lens, h, c, bf16=False):
    """One chunk in gx's dtype: (y [B, Tc, H], h, c)."""
    B, Tc = gx.shape[:2]
    H = w_hh.shape[1]
    lens_t = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    w = _rb(w_hh, bf16)
    y = gx.new_zeros(B, Tc, H)
    for t in range(Tc):
        a = gx[:, t] + _rb(h, bf16) @ w.t()
        i, f = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H])
        g, o = torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c_new = f * c + i * g
        h_new = o * torch.tanh(c_new)
        live = (lens_t > t).unsqueeze(1)
        h = torch.where(live, h_new, h)
        c = torch.where(live, c_new, c)
        y[:, t] = torch.where(live, h_new, torch.zeros_like(h_new))
    return y, h, c


def chunk_lens(totals, sizes):
    """[(start, size, lens [B])] of an utterance batch fed as chunks of `sizes`."""
    totals = np.asarray(totals, np.int64)
    out, s = [], 0
    for n in sizes:
        out.append((s, n, np.clip(totals - s, 0, n).astype(np.int32)))
        s += n
    return out


def run_schedule(gx, w_hh, totals, h, c, sizes, bf16=False):
    """(y [B, sum sizes, H], h, c) of feeding gx [B, T, 4H] chunk by chunk."""
    ys = []
    for s, n, lens in chunk_lens(totals, sizes):
        if n == 0:     # one padded frame (any values): no row has a frame in it
            _, h, c = run_chunk(torch.full_like(gx[:, :1], 3.0), w_hh, lens, h, c, bf16)
            continue
        y, h, c = run_chunk(gx[:, s:s + n], w_hh, lens, h, c, bf16)
        ys.append(y)
    return torch.cat(ys, dim=1), h, c


# --------------------------------------------------------------------------
# cases: the smallest at which the step kernel can go wrong.  Work-group: 4
# units x 32 utterances, 4 waves over K = H in slices of 32 (bf16) / 4 (f32);
# H % 8 == 0 takes vector fragment loads, any other H guarded scalar ones.
# H = 4: one unit tile; 20: scalar tail loads; 24: vector loads off the 16-unit
# tile.  B = 1, one short of and one past the row tile, and 3 with the totals
# [7, 4, 1]: rows that finish mid-chunk and then sit at lens = 0.
# --------------------------------------------------------------------------
CASES = {'h%d_b%d' % (H, B): dict(H=H, B=B) for H in (4, 20, 24) for B in (1, 31, 33)}
CASES['h20_b3'] = dict(H=20, B=3)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """CPU float32 inputs of a case (never modified): gx N(0, 1) with 100 N(0, 1)
    garbage at padded frames, W_hh U(+-0.3), a non-zero initial state (h U(+-0.8),
    c N(0, 1)) and the per-row totals make_lens(B, T) ([7, 4, 1] at B = 3)."""
    c = CASES[case]
    B, H = c['B'], c['H']
    g = torch.Generator().manual_seed(sum(map(ord, case)) * 7919 + 31)
    totals = R.make_lens(B, T)
    gx = torch.randn(B, T, 4 * H, generator=g)
    for b, n in enumerate(totals):
        gx[b, n:] *= 100.0
    return dict(gx=gx, w_hh=torch.rand(4 * H, H, generator=g) * 0.6 - 0.3,
                h0=torch.rand(B, H, generator=g) * 1.6 - 0.8, c0=torch.randn(B, H, generator=g),
                totals=totals)


def evaluate(case, dtype=torch.float64, precision=None, schedule='whole'):
    """{tensor name: float64 numpy array} of a case fed as `schedule`, evaluated
    in `dtype` (precision='bf16': float32 with bf16 mode's roundings)."""
    inp = case_inputs(case)
    t = {k: v.to(dtype) for k, v in inp.items() if torch.is_tensor(v)}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)          # one summation order whatever the machine
    try:
        out = run_schedule(t['gx'], t['w_hh'], inp['totals'], t['h0'], t['c0'],
                           SCHEDULES[schedule], bf16=precision == 'bf16')
    finally:
        torch.set_num_threads(nt)
    return {k: v.double().numpy() for k, v in zip(OUT_KEYS, out)}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 tensors of a case (single chunk), computed once."""
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


def layer_constant(precision):
    """The largest recorded constant of y over the cases: the error unit of one
    recurrent layer in `precision` ('fp32' | 'bf16'), for bounds on a stack of
    layers (tests/test_ctc_stream_gpu.py)."""
    cs = [case_constants(k) for k in CASES]
    if precision == 'fp32':
        return max(cf['y'] for cf, _ in cs)
    return max(max(cf['y'], cb['y']) for cf, cb in cs)


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['--record']:
        table = {case: measure_constants(case) for case in CASES}
        with open(CONSTANTS_JSON, 'w') as f:
            json.dump(table, f, indent=0, sort_keys=True)
            f.write('\n')
        print('recorded', len(table), 'cases in', CONSTANTS_JSON)
