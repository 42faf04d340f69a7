#!/usr/bin/env python
"""Time one feed of the streaming CTC prefix beam search
(native_ops.ctc_beam_stream_feed, asr_ctc_beam_stream_feed) beside the
whole-utterance search's time for the same number of frames, on an MI355X.
Not part of bench.py.

Shapes: V 29, beam width 16, B 1 and 8, chunks of 16, 32 and 64 frames, without
a language model and with a 2 x 256 LSTM LM (embedding 256, alpha 0.3).  One
utterance of T = 1024 frames per row is fed chunk by chunk after a warm-up
utterance; device events around each feed, median (min .. max) over the
utterance's feeds; with the stable-prefix step (stable_lens) and without it.
The yardstick: native_ops.ctc_beam_search on the T = 1024 logits, median of the
repeats, scaled by chunk / T.

Appends to profiles/ctc_beam_stream_bench.txt (or --out).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ctc_beam_lm_bench import _lm, _time_ms   # noqa: E402


def _feed_times(ops, logits, lens_c, chunk, W, lm, stable, warmup):
    """Per-feed milliseconds of one utterance fed in chunks of `chunk`."""
    B, T, V = logits.shape
    st = ops.ctc_beam_stream_state(B, V, W, T, logits.device, lm=lm)
    chunks = [logits[:, s:s + chunk].contiguous() for s in range(0, T, chunk)]
    times = []
    for rep in range(warmup + 1):
        ops.ctc_beam_stream_reset(st)
        torch.cuda.synchronize()
        times = []
        for x in chunks:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.ctc_beam_stream_feed(st, x, lens_c, None, stable=stable)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_beam_stream_bench.txt'))
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--beam_width', type=int, default=16)
    ap.add_argument('--frames', type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ctc_beam_stream_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dev = torch.device('cuda:0')
    V, W, T = 29, args.beam_width, args.frames
    lines = ['# one feed of the streaming CTC prefix beam search beside the whole-utterance '
             'search scaled to the chunk, MI355X; V %d, beam width %d, T %d; LM: 2 x 256 LSTM, '
             'alpha 0.3; device events, median (min .. max) over the %d / chunk feeds of one '
             'utterance after %d warm-up utterance(s); offline: median of %d calls'
             % (V, W, T, T, args.warmup, args.repeats)]
    for B in (1, 8):
        g = torch.Generator(device='cpu').manual_seed(V + B)
        logits = (torch.randn(B, T, V, generator=g) * 3).to(dev)
        logits[:, :, 0] += 3
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        for lm in (None, _lm(V, 2, 256, 256, dev, 0.3)):
            off = _time_ms(lambda: ops.ctc_beam_search(logits, lens, W, lm=lm), args.warmup,
                           args.repeats)
            _, hl, _ = ops.ctc_beam_search(logits, lens, W, lm=lm)
            for chunk in (16, 32, 64):
                lens_c = torch.full((B,), chunk, dtype=torch.int32, device=dev)
                with_s = _feed_times(ops, logits, lens_c, chunk, W, lm, True, args.warmup)
                no_s = _feed_times(ops, logits, lens_c, chunk, W, lm, False, args.warmup)
                scaled = off[0] * chunk / T
                lines.append('B %d %s chunk %2d: feed %.3f ms (%.3f .. %.3f) = %.1f us / frame; '
                             'without the stable prefix %.3f ms (%.3f .. %.3f); offline %.3f ms '
                             'for T %d = %.3f ms per chunk (%.1f us / frame); feed / offline %.2f; '
                             'mean hypothesis length %.1f'
                             % ((B, 'LM   ' if lm else 'no LM', chunk) + with_s +
                                (with_s[0] * 1e3 / chunk,) + no_s + (off[0], T, scaled,
                                                                     off[0] * 1e3 / T,
                                                                     with_s[0] / scaled,
                                                                     float(hl.float().mean()))))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
