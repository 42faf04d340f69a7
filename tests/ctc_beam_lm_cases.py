"""The cases tests/test_ctc_beam_lm_gpu.py runs on the device and
tests/test_ctc_beam_lm_cpu.py qualifies without one: seeds and shapes, the
inputs they draw, and the restatement (tests/ctc_beam_lm_ref.py) of each case,
computed once per process and shared.

Every case is B = 3 utterances of unequal lengths.  The seeds are picked so
that on the f64 restatement every utterance's final gap and every pruning gap
is >= GAP (test_ctc_beam_lm_cpu.py asserts it for ALL cases; the GPU tests skip
none).  A case's score_tol is 8 x the largest deviation of the restatement's
f32 evaluation from its f64 one over the case's utterances."""
import functools

import numpy as np

import ctc_beam_lm_ref as R

GAP = 1e-3
MAX_LAYERS = 4          # ASR_ATT_BEAM_LM_MAX_LAYERS

# name -> V, W, T, lens, blank, lm (layers, H, Y) or None, alpha, beta, seed
CASES = {
    # V 2: blank plus one label; widths 1 and 2
    'v2_w1': dict(V=2, W=1, T=8, lens=[8, 0, 1], blank=0, lm=(1, 8, 4), alpha=0.5, beta=0.0),
    'v2_w2_b1': dict(V=2, W=2, T=8, lens=[1, 8, 5], blank=1, lm=(1, 8, 4), alpha=0.3, beta=0.2),
    'v3_w2': dict(V=3, W=2, T=12, lens=[12, 1, 0], blank=0, lm=(2, 32, 16), alpha=0.5, beta=-0.3),
    'v3_w64': dict(V=3, W=64, T=5, lens=[5, 3, 1], blank=2, lm=(1, 8, 4), alpha=0.4, beta=0.1),
    # wave mode
    'v29_w1': dict(V=29, W=1, T=12, lens=[12, 7, 1], blank=0, lm=(1, 8, 4), alpha=0.5, beta=0.0),
    'v29_w20': dict(V=29, W=20, T=12, lens=[12, 7, 1], blank=0, lm=(2, 32, 16), alpha=0.3,
                    beta=0.0),
    'v29_w20_b5': dict(V=29, W=20, T=10, lens=[0, 10, 6], blank=5, lm=(2, 32, 16), alpha=0.7,
                       beta=0.5),
    'v29_w64': dict(V=29, W=64, T=6, lens=[6, 1, 4], blank=0, lm=(1, 8, 4), alpha=0.3, beta=-0.2),
    # the insertion bonus alone: no LM
    'v29_beta_pos': dict(V=29, W=20, T=12, lens=[12, 0, 5], blank=0, lm=None, alpha=0.0, beta=0.8),
    'v29_beta_neg': dict(V=29, W=20, T=12, lens=[1, 12, 9], blank=28, lm=None, alpha=0.0,
                         beta=-0.8),
    # either side of kWaveModeMaxV; the maximum layer count
    'v128_w20_l4': dict(V=128, W=20, T=8, lens=[8, 1, 5], blank=0, lm=(MAX_LAYERS, 16, 8),
                        alpha=0.5, beta=0.0),
    'v129_w20': dict(V=129, W=20, T=8, lens=[5, 8, 0], blank=128, lm=(2, 32, 16), alpha=0.3,
                     beta=0.3),
    'v129_w2': dict(V=129, W=2, T=8, lens=[8, 2, 1], blank=0, lm=(1, 8, 4), alpha=0.6, beta=0.0),
    # several passes of the work-group over a row
    'v1000_w20': dict(V=1000, W=20, T=6, lens=[6, 1, 3], blank=0, lm=(2, 32, 16), alpha=0.3,
                      beta=0.1),
}
SEEDS = {'v2_w1': 0, 'v2_w2_b1': 0, 'v3_w2': 0, 'v3_w64': 0, 'v29_w1': 0, 'v29_w20': 2,
         'v29_w20_b5': 0, 'v29_w64': 0, 'v29_beta_pos': 0, 'v29_beta_neg': 0, 'v128_w20_l4': 2,
         'v129_w20': 0, 'v129_w2': 0, 'v1000_w20': 0}

# identity under recreation with an LM (the construction of make_golden_ctc_beam.py's
# IDENTITY case): seed picked so that the f64 restatement reports `recreated`
IDENTITY = dict(V=4, W=3, T=16, lens=[16], blank=0, lm=(1, 8, 4), alpha=0.4, beta=0.0)
IDENTITY_SEED = 64


def draw(case, seed):
    """(logits f32 [B, T, V], lens int32 [B], LM parameters or None)."""
    rng = np.random.RandomState(7000 + seed)
    B = len(case['lens'])
    x = (rng.randn(B, case['T'], case['V']) * rng.uniform(2.0, 4.0)).astype(np.float32)
    lm = None
    if case['lm'] is not None:
        layers, H, Y = case['lm']
        lm = R.make_lm(8000 + seed, case['V'], layers, H, Y)
    return x, np.asarray(case['lens'], np.int32), lm


def restate(case, seed, dtype):
    """The restatement's result dict per utterance."""
    x, lens, lm = draw(case, seed)
    return [R.search(x[b, :lens[b]], case['W'], case['blank'], lm, case['alpha'], case['beta'],
                     dtype) for b in range(len(lens))]


@functools.lru_cache(maxsize=None)
def ref(name, f64=True):
    """The restatement of a case, computed once and shared."""
    if name == 'identity':
        return restate(IDENTITY, IDENTITY_SEED, np.float64 if f64 else np.float32)
    return restate(CASES[name], SEEDS[name], np.float64 if f64 else np.float32)


@functools.lru_cache(maxsize=None)
def score_tol(name):
    """8 x the largest |f32 - f64| score of the restatement over the case's
    utterances."""
    dev = max(abs(a['score'] - r['score']) for a, r in zip(ref(name, False), ref(name, True)))
    return 8.0 * dev


@functools.lru_cache(maxsize=None)
def score_tol_all():
    """The largest score_tol of the case list: the bound of the tests whose
    inputs are not a case of the list."""
    return max(score_tol(n) for n in CASES)
