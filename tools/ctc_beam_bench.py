#!/usr/bin/env python
"""Time the device CTC prefix beam search (native_ops.ctc_beam_search) beside
the best path on the same logits, on an MI355X.  Not part of bench.py.

Shapes: beam width 10, B 32, V 29 / T 1000 (character head) and V 10001 /
T 250 (word head).  Per shape: warm-up, then device events around each call,
median (min .. max) of the repeats.  The row pre-pass is also timed alone
(asr_ctc_beam_rows) and its rate is given as logits bytes / time: what the
pass must read once, whatever it re-reads from cache.

Writes profiles/ctc_beam_bench.txt (or --out).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_beam_bench.txt'))
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=11)
    ap.add_argument('--beam_width', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ctc_beam_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dev = torch.device('cuda:0')
    W, B = args.beam_width, 32
    lines = ['# CTC prefix beam search beside the best path, MI355X; beam width %d, B %d; device '
             'events, median (min .. max) of %d calls after %d warm-up calls'
             % (W, B, args.repeats, args.warmup)]
    for V, T in ((29, 1000), (10001, 250)):
        g = torch.Generator(device='cpu').manual_seed(V)
        logits = (torch.randn(B, T, V, generator=g) * 3).to(dev)
        logits[:, :, 0] += 3
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        nb = N.query('asr_ctc_beam_ws_bytes', T, B, V, W)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def rows():
            N.call('asr_ctc_beam_rows', N.ptr(logits), V, T * V, T, B, V, N.ptr(lens), 0, W, 1,
                   N.ptr(ws), nb, N.stream_handle(dev))

        beam = _time_ms(lambda: ops.ctc_beam_search(logits, lens, W), args.warmup, args.repeats)
        greedy = _time_ms(lambda: ops.ctc_best_path(logits, lens), args.warmup, args.repeats)
        pre = _time_ms(rows, args.warmup, args.repeats)
        nbytes = B * T * V * 4
        _, hl, _ = ops.ctc_beam_search(logits, lens, W)
        lines.append('V %5d T %4d: beam search %.3f ms (%.3f .. %.3f), best path %.3f ms '
                     '(%.3f .. %.3f), ratio %.1fx; mean hypothesis length %.1f'
                     % ((V, T) + beam + greedy + (beam[0] / greedy[0], float(hl.float().mean()))))
        lines.append('    row pre-pass alone %.3f ms (%.3f .. %.3f): %.1f MB of logits, %.1f GB/s'
                     % (pre + (nbytes / 1e6, nbytes / pre[0] / 1e6)))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
