#!/usr/bin/env python
"""Record tests/golden/edit_distance.npz from the REFERENCE's compute_wer.

Runs only in the build container (it imports the read-only reference
checkout, as make_golden.py does); its Levenshtein import, which compute_wer
does not use, is stubbed out.  Only numbers are stored.

Per vocabulary size in VOCABS random (ref, hyp) pairs with lengths 1..40 are
drawn until KEEP of them are kept.  A pair is kept iff the reference returns a
value: its backtrace has no border rule, its indices wrap to the far side of
the table, and it raises IndexError for part of the pairs (or trips its own
assertions).  The numbers drawn and dropped are stored with the pairs.

Condition (asserted): at least 64 kept pairs per vocabulary size.

Usage (from the repo root, in the build container):
    python tests/golden/make_golden_edit_distance.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get('ASR_REFERENCE_ROOT', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))

VOCABS = (2, 3, 30)
KEEP = 96
MAX_LEN = 40


def _reference_compute_wer():
    sys.modules.setdefault('Levenshtein', types.ModuleType('Levenshtein'))
    path = os.path.join(REF, 'utils', 'evaluation', 'edit_distance.py')
    spec = importlib.util.spec_from_file_location('ref_edit_distance', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.compute_wer


def main():
    compute_wer = _reference_compute_wer()
    rng = np.random.RandomState(20261020)
    refs, hyps, rl, hl, res, vocab = [], [], [], [], [], []
    drawn, dropped = [], []
    for V in VOCABS:
        n_draw = n_drop = kept = 0
        while kept < KEEP:
            n_draw += 1
            nr, nh = rng.randint(1, MAX_LEN + 1), rng.randint(1, MAX_LEN + 1)
            r, h = rng.randint(0, V, nr), rng.randint(0, V, nh)
            if rng.rand() < 0.5:        # a hypothesis that is an edited reference
                h = np.array([t for t in r if rng.rand() > 0.15] or [0])[:MAX_LEN]
                flip = rng.rand(len(h)) < 0.2
                h = np.where(flip, rng.randint(0, V, len(h)), h)
                nh = len(h)
            try:
                wer, sub, ins, dele = compute_wer(list(r), list(h))
            except (IndexError, AssertionError):
                n_drop += 1
                continue
            kept += 1
            row_r, row_h = np.full(MAX_LEN, -1, np.int32), np.full(MAX_LEN, -1, np.int32)
            row_r[:nr], row_h[:nh] = r, h
            refs.append(row_r)
            hyps.append(row_h)
            rl.append(nr)
            hl.append(nh)
            res.append([int(wer), sub, ins, dele])
            vocab.append(V)
        assert kept >= 64
        drawn.append(n_draw)
        dropped.append(n_drop)
        print('V = %d: drew %d, dropped %d, kept %d' % (V, n_draw, n_drop, kept))
    np.savez_compressed(os.path.join(OUT, 'edit_distance.npz'),
                        ref=np.array(refs), hyp=np.array(hyps), ref_lens=np.array(rl, np.int32),
                        hyp_lens=np.array(hl, np.int32), result=np.array(res, np.int32),
                        vocab=np.array(vocab, np.int32), vocabs=np.array(VOCABS, np.int32),
                        drawn=np.array(drawn, np.int32), dropped=np.array(dropped, np.int32))


if __name__ == '__main__':
    main()
