#!/usr/bin/env python
"""Time the device CTC prefix beam search with a language model
(native_ops.ctc_beam_search(lm=...), asr_ctc_beam_search_lm) beside the search
without one on the same logits, on an MI355X.  Not part of bench.py.

Shapes: B 32, T 1000, beam width 20, V 29 and V 1000; a 2 x 512 LSTM LM
(embedding 512); alpha 0.3 against alpha = beta = 0.  Inputs resident, warm-up,
then device events around each call, median (min .. max) of the repeats.

--no-lm-only: one line with the no-LM search alone, for runs of two builds of
the library side by side (ASR_LIB_PATH selects the other build).

Appends to profiles/ctc_beam_lm_bench.txt (or --out).
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


def _lm(V, layers, H, Y, dev, weight):
    g = torch.Generator(device='cpu').manual_seed(V + 1)
    u = lambda *s: ((torch.rand(*s, generator=g) - 0.5) * 0.2).to(dev)   # noqa: E731
    return dict(cell='lstm', weight=weight, emb=u(V, Y),
                w_ih=[u(4 * H, Y if l == 0 else H) for l in range(layers)],
                w_hh=[u(4 * H, H) for l in range(layers)],
                b_ih=[u(4 * H) for l in range(layers)], b_hh=[u(4 * H) for l in range(layers)],
                w_out=u(V, H), b_out=u(V))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_beam_lm_bench.txt'))
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--beam_width', type=int, default=20)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--no-lm-only', action='store_true')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ctc_beam_lm_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dev = torch.device('cuda:0')
    W, B, T = args.beam_width, 32, args.frames
    lines = []
    if not args.no_lm_only:
        lines.append('# CTC prefix beam search with a 2 x 512 LSTM LM (alpha 0.3) beside the search '
                     'without one, MI355X; B %d, T %d, beam width %d; device events, median '
                     '(min .. max) of %d calls after %d warm-up calls'
                     % (B, T, W, args.repeats, args.warmup))
    for V in (29, 1000):
        g = torch.Generator(device='cpu').manual_seed(V)
        logits = (torch.randn(B, T, V, generator=g) * 3).to(dev)
        logits[:, :, 0] += 3
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        plain = _time_ms(lambda: ops.ctc_beam_search(logits, lens, W), args.warmup, args.repeats)
        if args.no_lm_only:
            lines.append('no-LM search %s: V %4d T %d W %d: %.3f ms (%.3f .. %.3f)'
                         % ((args.label, V, T, W) + plain))
            continue
        lm = _lm(V, 2, 512, 512, dev, 0.3)
        fused = _time_ms(lambda: ops.ctc_beam_search(logits, lens, W, lm=lm), args.warmup,
                         args.repeats)
        bonus = _time_ms(lambda: ops.ctc_beam_search(logits, lens, W, beta=0.5), args.warmup,
                         args.repeats)
        _, hl, _ = ops.ctc_beam_search(logits, lens, W, lm=lm)
        lines.append('V %4d: alpha 0.3 %.3f ms (%.3f .. %.3f) = %.1f us / frame at 3 launches a '
                     'frame; beta 0.5 without an LM %.3f ms (%.3f .. %.3f), 2 launches a frame; '
                     'alpha = beta = 0 %.3f ms (%.3f .. %.3f); mean hypothesis length %.1f'
                     % ((V,) + fused + (fused[0] * 1e3 / T,) + bonus + plain +
                        (float(hl.float().mean()),)))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
