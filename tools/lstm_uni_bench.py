"""Timing of one unidirectional LSTM layer (native_ops.lstm_layer: the per-step
recurrence of csrc/lstm_uni.hip and the layer GEMMs), forward and backward,
with the same-shape bidirectional layer (native_ops.blstm_layer) for scale.

Each round times the forward and the backward with torch events; every other
round also turns the library's HIP-event hooks on (asr_prof_begin(1): every
step launch timed), which gives the launch count and the mean in-kernel time
of a step.  The launch-gap share of the layer is 1 - (steps x mean step time +
the GEMMs' time) / layer time, the layer time taken from the rounds without
the hooks (they add two event records per launch).  Medians over the rounds
after one warm-up round.

usage: python tools/lstm_uni_bench.py [--rounds 7] [--B 32] [--T 1000] [--H 512]
       [--Din 512] [--dtype bf16]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_end2end_speech_recognition_amd import _native as N  # noqa: E402
from pytorch_end2end_speech_recognition_amd import native_ops as ops  # noqa: E402


def _round(fn, x, lens, T, ws, R, hooks):
    torch.cuda.synchronize()
    if hooks:
        N.call('asr_prof_begin', 1)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    y = fn(x, lens, T, *ws)
    ev[1].record()
    y.backward(R)
    ev[2].record()
    torch.cuda.synchronize()
    out = dict(fwd=ev[0].elapsed_time(ev[1]) * 1e3, bwd=ev[1].elapsed_time(ev[2]) * 1e3)
    if hooks:
        mean_us = (ctypes.c_double * 9)()
        launches = (ctypes.c_longlong * 9)()
        N.call('asr_prof_end', ctypes.cast(mean_us, ctypes.c_void_p),
               ctypes.cast(launches, ctypes.c_void_p), None, 9)
        out.update(step_fwd=mean_us[0], n_fwd=launches[0], step_bwd=mean_us[1], n_bwd=launches[1],
                   seq_fwd=mean_us[2], seq_bwd=mean_us[3], n_seq=launches[2] + launches[3],
                   gemm=mean_us[4] * launches[4], n_gemm=launches[4])
    for w in ws:
        w.grad = None
    x.grad = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--H', type=int, default=512)
    ap.add_argument('--Din', type=int, default=512)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    ops.set_compute_dtype(args.dtype)
    B, T, H, Din = args.B, args.T, args.H, args.Din
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.randn(B, T, Din).astype(np.float32)).to(dev).requires_grad_(True)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    print('shape B %d T %d H %d Din %d, %s, %s' % (B, T, H, Din, args.dtype,
                                                  torch.cuda.get_device_name(0)))
    for name, fn, nd in (('lstm_layer (unidirectional)', ops.lstm_layer, 1),
                         ('blstm_layer (bidirectional)', ops.blstm_layer, 2)):
        ws = [torch.from_numpy(rng.uniform(-0.1, 0.1, s).astype(np.float32)).to(dev)
              .requires_grad_(True)
              for s in ((4 * nd * H, Din), (4 * nd * H, H), (4 * nd * H,), (4 * nd * H,))]
        R = torch.randn(B, T, nd * H, device=dev)
        plain, hooked = [], []
        for rnd in range(2 * args.rounds + 2):
            r = _round(fn, x, lens, T, ws, R, hooks=rnd % 2 == 1)
            if rnd >= 2:      # one warm-up round of each kind
                (hooked if rnd % 2 else plain).append(r)
        med = lambda rs, k: float(np.median([r[k] for r in rs]))      # noqa: E731
        fwd, bwd = med(plain, 'fwd'), med(plain, 'bwd')
        print('%s: forward %.1f us, backward %.1f us, layer %.1f us (medians of %d rounds)'
              % (name, fwd, bwd, fwd + bwd, len(plain)))
        h = hooked[-1]
        if h['n_fwd'] or h['n_bwd']:
            sf, sb = med(hooked, 'step_fwd'), med(hooked, 'step_bwd')
            print('  step launches: forward %d x %.2f us in-kernel, backward %d x %.2f us in-kernel'
                  % (h['n_fwd'], sf, h['n_bwd'], sb))
            gemm = med(hooked, 'gemm')
            busy = h['n_fwd'] * sf + h['n_bwd'] * sb + gemm
            print('  in-kernel time: forward steps %.1f us, backward steps %.1f us, %d GEMM '
                  'launches %.1f us; launch gaps and the small passes: %.0f %% of the layer'
                  % (h['n_fwd'] * sf, h['n_bwd'] * sb, h['n_gemm'], gemm,
                     100 * (1 - busy / (fwd + bwd))))
        if h['n_seq']:
            print('  persistent passes: %d launches, forward %.1f us, backward %.1f us'
                  % (h['n_seq'], med(hooked, 'seq_fwd'), med(hooked, 'seq_bwd')))
    ops.set_compute_dtype('fp32')


if __name__ == '__main__':
    main()
