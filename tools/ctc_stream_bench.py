#!/usr/bin/env python
"""Time chunk-by-chunk recognition (CTC.stream) beside what a user had before
it: decode() on the growing prefix at every chunk boundary, and one
whole-utterance decode(), on an MI355X.  Not part of bench.py.

Model: 5 x 512 unidirectional LSTM CTC (input 120, 28 classes), eval mode, B =
1 and B = 8, a 1000-frame utterance fed in chunks of 16, 32 and 64 frames.
Every timed call ends in its own host read of the hypotheses, i.e. in a device
synchronise, so a host clock around it measures the call.  Per configuration:
warm-up passes over the whole utterance (every chunk shape, the last shorter
one included), then timed passes; ms per feed is the median (min .. max) over
all feeds of all timed passes, the totals are medians (min .. max) over the
passes.  No pass threshold: the figures are recorded.

Writes profiles/ctc_stream_bench.txt (or --out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _mmm(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_stream_bench.txt'))
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--prefix_repeats', type=int, default=3)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--precision', default='bf16', choices=['fp32', 'bf16'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ctc_stream_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    from pytorch_end2end_speech_recognition_amd.models.pytorch_v3.ctc.ctc import CTC
    ops.set_compute_dtype(args.precision)
    torch.manual_seed(1623)
    model = CTC(input_size=120, encoder_type='lstm', encoder_bidirectional=False,
                encoder_num_units=512, encoder_num_proj=0, encoder_num_layers=5, fc_list=[],
                dropout_input=0, dropout_encoder=0, num_classes=28, parameter_init=0.1,
                subsample_list=[], subsample_type='drop')
    model.set_cuda()
    model.eval()
    T = args.frames
    lines = ['# CTC.stream beside decode() on the growing prefix and one whole-utterance decode(), '
             'MI355X; 5 x 512 unidirectional LSTM CTC, %s, %d frames; host clock around calls '
             'that end in a host read, median (min .. max); %d timed passes (%d of the prefix '
             're-decode) after %d warm-up'
             % (args.precision, T, args.repeats, args.prefix_repeats, args.warmup)]
    for B in (1, 8):
        xs = torch.from_numpy(np.random.RandomState(B).randn(B, T, 120).astype(np.float32))
        xs = xs.to(model.device)
        full = np.full(B, T, np.int32)
        whole = []
        for i in range(args.warmup + args.repeats):
            ms, ref = _clock(lambda: model.decode(xs, full, beam_width=1))
            if i >= args.warmup:
                whole.append(ms)
        lines.append('B %d: whole-utterance decode() %.2f ms (%.2f .. %.2f)' % ((B,) + _mmm(whole)))
        for C in (16, 32, 64):
            cuts = list(range(0, T, C)) + [T]
            st = model.stream(B)
            feeds, totals = [], []
            for i in range(args.warmup + args.repeats):
                st.reset()
                per = []
                for s, e in zip(cuts[:-1], cuts[1:]):
                    ms, _ = _clock(lambda: st.feed(xs[:, s:e], np.full(B, e - s, np.int32)))
                    per.append(ms)
                if i >= args.warmup:
                    feeds += per[:-1] if (T % C) else per     # full-size chunks only
                    totals.append(sum(per))
            same = all(np.array_equal(a, b) for a, b in zip(st.hyps(), ref[0]))
            prefix, last = [], []     # per pass: all prefix calls, the last (longest) one
            for i in range(args.warmup + args.prefix_repeats):
                per = []
                for e in cuts[1:]:
                    ms, _ = _clock(lambda: model.decode(xs[:, :e], np.full(B, e, np.int32),
                                                        beam_width=1))
                    per.append(ms)
                if i >= args.warmup:
                    prefix.append(sum(per))
                    last.append(per[-1])
            f, t, p = _mmm(feeds), _mmm(totals), _mmm(prefix)
            lines.append('  chunk %2d (%3d feeds): %.3f ms per feed (%.3f .. %.3f), streamed '
                         'total %.1f ms (%.1f .. %.1f); decode() on each prefix, total %.1f ms '
                         '(%.1f .. %.1f), %.1fx the stream; last prefix call alone %.2f ms (median); '
                         'labels equal decode(): %s'
                         % ((C, len(cuts) - 1) + f + t + p + (p[0] / t[0], float(np.median(last)), same)))
    ops.set_compute_dtype('fp32')
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
