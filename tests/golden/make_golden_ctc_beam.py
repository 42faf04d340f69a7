#!/usr/bin/env python
"""Generate tests/golden/ctc_beam.npz from the REFERENCE's BeamSearchDecoder.

Runs only in the build container (it imports the read-only reference checkout,
as make_golden.py does).  Only numbers are stored: logits, lengths, widths, the
reference's hypotheses, and the float64 scores and gaps of the restatement in
tests/ctc_beam_ref.py.

Every recorded utterance meets this condition (asserted, never loosened):
  * the reference (float32 log-probabilities) and the float64 restatement give
    the same hypothesis;
  * the final gap between best and second best is >= 1e-3;
  * at every frame the gap between the last kept and the first dropped
    candidate is >= 1e-3.
Seeds are searched (200 at most per case) until a draw meets it.

score_tol = 8 x the largest |float32 restatement score - float64 score| over
the recorded utterances (8: the device's exp / log1p differ from numpy's).

Usage (from the repo root, in the build container):
    python tests/golden/make_golden_ctc_beam.py
"""
import importlib.util
import os
import sys

import numpy as np

REF = os.environ.get('ASR_REFERENCE_ROOT', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import ctc_beam_ref as R  # noqa: E402

GAP = 1e-3
MAX_SEEDS = 200

# name, V, T, W, blank
CASES = [('v6', 6, 24, 4, 0), ('v29', 29, 48, 10, 0), ('v41', 41, 40, 10, 0),
         ('v300', 300, 20, 8, 0), ('v10001', 10001, 8, 10, 0), ('v29_blank_last', 29, 32, 10, 28)]
RAGGED = dict(V=29, T=40, W=10, blank=0, lens=[0, 1, 17, 40, 45])
IDENTITY = dict(V=4, T=16, W=3, blank=0)


def _reference_decoder():
    path = os.path.join(REF, 'models', 'pytorch_v3', 'ctc', 'decoders', 'beam_search_decoder.py')
    spec = importlib.util.spec_from_file_location('ref_beam_search_decoder', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BeamSearchDecoder


def draw(rng, V, T, blank, runs):
    """Gaussian x (2..4); runs: +3 on the blank and frames repeated in runs of
    1..4, so that repeats and blanks occur."""
    scale = rng.uniform(2.0, 4.0)
    x = (rng.randn(T, V) * scale).astype(np.float32)
    if runs:
        x[:, blank] += 3.0
        t = 0
        while t < T:
            n = rng.randint(1, 5)
            x[t:t + n] = x[t]
            t += n
    return x


def check(dec_cls, logits, W, blank):
    """One utterance [T, V]: the record if it meets the condition, else None."""
    with np.errstate(all='ignore'):
        lp32 = R.log_softmax(logits, np.float32)
        ref = dec_cls(blank_index=blank)(lp32[None], np.array([len(logits)]), beam_width=W)[0]
        r64 = R.beam_search(R.log_softmax(logits, np.float64), W, blank)
    if not np.array_equal(np.asarray(ref, np.int64), r64['hyp']):
        return None
    if r64['final_gap'] < GAP or r64['prune_gap'] < GAP:
        return None
    with np.errstate(all='ignore'):
        r32 = R.beam_search(lp32, W, blank, np.float32)
    r64['ref_hyp'] = np.asarray(ref, np.int64)
    r64['f32_err'] = abs(r32['score'] - r64['score'])
    return r64


def main():
    dec_cls = _reference_decoder()
    out, names, errs = {}, [], []

    def record(name, logits, lens, W, blank, recs):
        names.append(name)
        out[name + '/logits'] = logits
        out[name + '/lens'] = np.asarray(lens, np.int32)
        out[name + '/W'] = np.int32(W)
        out[name + '/blank'] = np.int32(blank)
        out[name + '/score'] = np.array([r['score'] for r in recs], np.float64)
        out[name + '/final_gap'] = np.array([r['final_gap'] for r in recs], np.float64)
        out[name + '/prune_gap'] = np.array([r['prune_gap'] for r in recs], np.float64)
        for b, r in enumerate(recs):
            out['%s/hyp%d' % (name, b)] = r['ref_hyp']
            assert r['final_gap'] >= GAP and r['prune_gap'] >= GAP
            errs.append(r['f32_err'])

    for ci, (name, V, T, W, blank) in enumerate(CASES):
        for runs in (False, True):
            for seed in range(MAX_SEEDS):
                rng = np.random.RandomState(1000 * ci + 500 * runs + seed)
                x = draw(rng, V, T, blank, runs)
                r = check(dec_cls, x, W, blank)
                if r is not None:
                    break
            assert r is not None, (name, runs)
            record(name + ('_runs' if runs else ''), x[None], [T], W, blank, [r])
            print(name, runs, 'seed', seed, 'hyp len', len(r['ref_hyp']), 'gaps', r['final_gap'],
                  r['prune_gap'])

    # the ragged batch: every row meets the condition; NaN beyond each length
    g = RAGGED
    for seed in range(MAX_SEEDS):
        rng = np.random.RandomState(7000 + seed)
        xs = np.stack([draw(rng, g['V'], g['T'], g['blank'], b % 2 == 1) for b in range(5)])
        recs = []
        for b, n in enumerate(g['lens']):
            n = min(n, g['T'])
            if n == 0:
                recs.append(dict(ref_hyp=np.zeros(0, np.int64), score=0.0, final_gap=np.inf,
                                 prune_gap=np.inf, f32_err=0.0))
                continue
            recs.append(check(dec_cls, xs[b, :n], g['W'], g['blank']))
        if all(r is not None for r in recs):
            break
    assert all(r is not None for r in recs)
    for b, n in enumerate(g['lens']):
        xs[b, min(n, g['T']):] = np.nan
    record('ragged', xs, g['lens'], g['W'], g['blank'], recs)
    print('ragged seed', seed, [len(r['ref_hyp']) for r in recs])

    # identity under re-creation: a prefix comes back into the beam while a
    # child of its earlier self stayed, and a search that identifies prefixes
    # by node id then returns something else
    g = IDENTITY
    found = None
    for seed in range(20000):
        rng = np.random.RandomState(9000 + seed)
        x = draw(rng, g['V'], g['T'], g['blank'], seed % 2 == 1)
        lp = R.log_softmax(x, np.float64)
        r64 = R.beam_search(lp, g['W'], g['blank'])
        if not r64['recreated'] or r64['final_gap'] < GAP or r64['prune_gap'] < GAP:
            continue
        good = R.restricted_search(lp, g['W'], g['blank'], True)
        bad = R.restricted_search(lp, g['W'], g['blank'], False)
        assert np.array_equal(good[0], r64['hyp']) and abs(good[1] - r64['score']) < 1e-9
        if np.array_equal(bad[0], r64['hyp']) and abs(bad[1] - r64['score']) < 1e-2:
            continue
        r = check(dec_cls, x, g['W'], g['blank'])
        if r is not None:
            found = (x, r)
            break
    assert found is not None
    record('identity', found[0][None], [g['T']], g['W'], g['blank'], [found[1]])
    out['identity/recreated'] = np.bool_(found[1]['recreated'])
    print('identity seed', seed, found[1]['ref_hyp'])

    out['names'] = np.array(names)
    out['score_tol'] = np.float64(8.0 * max(errs))
    print('score_tol', out['score_tol'])
    np.savez_compressed(os.path.join(OUT, 'ctc_beam.npz'), **out)


if __name__ == '__main__':
    main()
