#!/usr/bin/env python
"""Time the device scorer (native_ops.edit_distance) beside the host
restatement (native_ops.edit_distance_host, the reference's per-utterance
Python table) on the same pairs, on an MI355X.  Not part of bench.py; the
numbers are reported and gate nothing.

Shapes, B 32: character transcripts of about 200 tokens (vocabulary 28 with a
separator; token units and word units) and 40 phones (vocabulary 39).  The
hypotheses are the transcripts with 10 % of the tokens dropped and 10 %
replaced.  Kernel: warm-up, then device events around groups of --inner calls,
per-call median (min .. max) over --repeats groups.  Host: wall time of one
pass over the batch (median of 3).

Writes profiles/edit_distance_bench.txt (or --out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def _pairs(rng, B, n, V, space):
    refs, hyps = [], []
    for _ in range(B):
        r = rng.randint(0, V, rng.randint(int(n * 0.8), int(n * 1.2) + 1))
        if space is not None:
            r[rng.rand(len(r)) < 0.18] = space
        h = r[rng.rand(len(r)) > 0.1].copy()
        flip = rng.rand(len(h)) < 0.1
        h[flip] = rng.randint(0, V, int(flip.sum()))
        refs.append(r)
        hyps.append(h)
    return refs, hyps


def _pad(rows):
    out = np.full((len(rows), max(len(r) for r in rows)), -1, np.int32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edit_distance_bench.txt'))
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=11)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('edit_distance_bench: needs an MI355X; a CPU run gives no time')
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dev = torch.device('cuda:0')
    B = 32
    rng = np.random.RandomState(0)
    lines = ['# device edit distance beside the host restatement, MI355X; B %d; kernel: device '
             'events, per-call median (min .. max) of %d groups of %d calls after %d warm-up '
             'calls; host: wall time of one pass over the batch, median of 3'
             % (B, args.repeats, args.inner, args.warmup)]
    for name, n, V, space, unit in (('characters ~200, token units', 200, 28, 27, 'token'),
                                    ('characters ~200, word units', 200, 28, 27, 'word'),
                                    ('phones 40', 40, 39, None, 'token')):
        refs, hyps = _pairs(rng, B, n, V, space)
        rl, hl = [len(r) for r in refs], [len(h) for h in hyps]
        ref_h, hyp_h = _pad(refs), _pad(hyps)
        ref_d, hyp_d = torch.from_numpy(ref_h).to(dev), torch.from_numpy(hyp_h).to(dev)
        rl_d = torch.tensor(rl, dtype=torch.int32, device=dev)
        hl_d = torch.tensor(hl, dtype=torch.int32, device=dev)
        kw = dict(unit=unit, space=space)
        kern = _time_ms(lambda: ops.edit_distance(hyp_d, hl_d, ref_d, rl_d, **kw), args.warmup,
                        args.repeats, args.inner)
        got = ops.edit_distance(hyp_d, hl_d, ref_d, rl_d, **kw).cpu().numpy()
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = ops.edit_distance_host(hyp_h, hl, ref_h, rl, **kw)
            host.append((time.perf_counter() - t0) * 1e3)
        assert ops.last_edit_distance_path() == 'device' and np.array_equal(got, want)
        lines.append('%-30s kernel %.4f ms (%.4f .. %.4f), host %.1f ms, ratio %.0fx; '
                     'mean units %.1f, error rate %.3f'
                     % ((name + ':',) + kern + (float(np.median(host)),
                                                float(np.median(host)) / kern[0],
                                                got[:, 4].mean(), got[:, 0].sum() / got[:, 4].sum())))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
