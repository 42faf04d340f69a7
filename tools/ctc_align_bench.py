#!/usr/bin/env python
"""Time CTC forced alignment (asr_ctc_align) beside the CTC forward
(asr_ctc_forward: the alpha / beta lattices) at the same shape, and beside the
numpy host path (ctc_align_host), on an MI355X.  Not part of bench.py.

Shape: the default config's head -- B 32, T 1000, V 29 (28 labels + blank),
input lengths U[800, 1000], label lengths U[60, 125] as bench.py draws them.
asr_ctc_align and asr_ctc_forward are both called through the raw C ABI on
preallocated buffers (one more line times the native_ops wrapper, which
allocates its outputs).  A window is `inner` back-to-back calls between two
stream events (about 0.3 s); every round times one window of each line in
turn, so the lines alternate; us per call is the median (min .. max) over the
rounds.  The host path is timed once with a host clock.  No pass threshold:
the figures are recorded.

Writes profiles/ctc_align_bench.txt (or --out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, inner):
    """us per call of `inner` back-to-back calls between two stream events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def _mmm(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_align_bench.txt'))
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ctc_align_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dev = torch.device('cuda:0')
    B, T, V = 32, 1000, 29
    rng = np.random.RandomState(0)
    x = (3 * rng.randn(B, T, V)).astype(np.float32)
    x_lens = np.sort(rng.randint(800, T + 1, B))[::-1].astype(np.int32)
    y_lens = rng.randint(60, 126, B).astype(np.int32)
    flat = np.concatenate([rng.randint(1, V, n) for n in y_lens]).astype(np.int32)
    M = int(y_lens.max())
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(x_lens.copy()).to(dev)
    fd, yd = torch.from_numpy(flat).to(dev), torch.from_numpy(y_lens).to(dev)
    lines = ['# asr_ctc_align beside asr_ctc_forward and ctc_align_host, MI355X; B %d, T %d, V %d, '
             'x_lens U[800, %d], y_lens U[60, 125] (max %d); both entry points called through the '
             'raw C ABI on preallocated buffers; a window = %d back-to-back calls between two '
             'stream events; %d rounds, every round one window of each line in turn, after %d '
             'warm-up calls of each; us per call, median (min .. max) over the rounds'
             % (B, T, V, T, M, args.inner, args.repeats, args.warmup)]
    st = N.stream_handle(dev)
    ali = torch.empty(B, T, dtype=torch.int32, device=dev)
    starts = torch.empty(B, M, dtype=torch.int32, device=dev)
    ends = torch.empty(B, M, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    nba = N.query('asr_ctc_align_ws_bytes', T, B, V, M)
    wsa = torch.empty(nba, dtype=torch.uint8, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    nbf = N.query('asr_ctc_workspace_bytes', T, B, V, M)
    wsf = torch.empty(nbf, dtype=torch.uint8, device=dev)

    def align(normalize, spans):
        return lambda: N.call(
            'asr_ctc_align', N.ptr(xd), V, T * V, T, B, V, N.ptr(fd), N.ptr(yd), N.ptr(ld), M, 0,
            normalize, N.ptr(ali), N.ptr(starts) if spans else None,
            N.ptr(ends) if spans else None, N.ptr(scores), N.ptr(wsa), nba, st)

    jobs = [
        ('asr_ctc_align normalize=1 spans=1', align(1, True)),
        ('asr_ctc_forward (alpha and beta lattices, costs)',
         lambda: N.call('asr_ctc_forward', N.ptr(xd), V, T * V, T, B, V, N.ptr(fd), N.ptr(yd),
                        N.ptr(ld), M, 0, 1, N.ptr(costs), None, 1.0, N.ptr(wsf), nbf, st)),
        ('asr_ctc_align normalize=0 spans=1', align(0, True)),
        ('asr_ctc_align normalize=1 spans=0', align(1, False)),
        ('native_ops.ctc_align (the Python wrapper: allocates its outputs), normalize=1 spans=1',
         lambda: ops.ctc_align(xd, ld, fd, yd, M, 0, True, True)),
    ]
    for _, fn in jobs:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in jobs]
    for _ in range(args.repeats):
        for i, (_, fn) in enumerate(jobs):
            times[i].append(_window(fn, args.inner))
    for (name, _), t in zip(jobs, times):
        lines.append('%s: %.1f us (%.1f .. %.1f)' % ((name,) + _mmm(t)))
    assert ops.last_ctc_align_path() == 'device'
    t0 = time.perf_counter()
    host = ops.ctc_align_host(x, x_lens, flat, y_lens, M, 0, True, True)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = ops.ctc_align(xd, ld, fd, yd, M, 0, True, True)
    same = all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got[:3], host[:3]))
    lines.append('ctc_align_host (numpy float32, one host clock): %.0f ms; device ali / starts / '
                 'ends equal the host path: %s' % (host_ms, same))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
