"""Reference, cases and bound of the CTC forced alignment (csrc/ctc_align.hip,
asr_ctc_align).  Nothing here imports the product package.

align_f32: the recurrence of include/asr_hip.h in numpy float32 -- raw logits,
one rounding per add, the first predecessor in the order s, s-1, s-2 on ties --
so ali / starts / ends (and with normalize == 0 the score) are compared BIT FOR
BIT.  score_f64: the float64 log-softmax summed along a given path.
enumerate_alignments: every alignment of a tiny case, ranked.

Normalised scores follow the cost rule of ctc_paths_ref:

    |got - score_f64(path)| <= MARGIN (16) x max(K_score, 2^-24 x A_b)

A_b = sum over t of |log-softmax| along the path; K_score = the error of
score_f32 (the same sum with every value held in numpy float32, frames added
in order) against score_f64, measured on the CPU per case and recorded in
tests/golden/ctc_align_constants.json (python tests/ctc_align_ref.py --record);
the CPU test recomputes it.  The kernel uses __expf / __logf and a lane tree,
so the margin is over another float32 evaluation, not over itself.
"""
import itertools
import json
import os

import numpy as np

MARGIN = 16
F32_U = 2.0 ** -24
NEG = np.float32(-np.inf)
CONSTS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                           'ctc_align_constants.json')


def states(lab, blank):
    cls = np.full(2 * len(lab) + 1, blank, np.int64)
    cls[1::2] = lab
    return cls


def align_f32(x, Tb, lab, blank):
    """One utterance: x float32 [T, V] raw logits, Tb frames, lab its labels.
    Returns (path of classes int32 [Tb], starts, ends int32 [L], end value
    float32) or None for an infeasible row."""
    x = np.asarray(x, np.float32)
    lab = np.asarray(lab, np.int64).reshape(-1)
    L, V = len(lab), x.shape[1]
    if ((lab < 0) | (lab >= V) | (lab == blank)).any():
        return None
    if Tb <= 0:
        return (np.zeros(0, np.int32),) * 3 + (np.float32(0),) if L == 0 else None
    cls = states(lab, blank)
    S = len(cls)
    v = np.full(S, NEG, np.float32)
    v[0] = x[0, blank]
    if L:
        v[1] = x[0, lab[0]]
    back = np.zeros((Tb, S), np.int64)
    skip = np.zeros(S, bool)          # s odd, s >= 3, c(s) != c(s-2)
    skip[3::2] = lab[1:] != lab[:-1]
    with np.errstate(invalid='ignore'):
        for t in range(1, Tb):        # every state at once: the same float32 operations
            m, d = v.copy(), back[t]
            p1 = np.concatenate(([NEG], v[:-1]))
            k = p1 > m                                    # strictly greater: s wins ties
            m[k], d[k] = p1[k], 1
            p2 = np.concatenate(([NEG, NEG], v[:-2]))[:S]
            k = skip & (p2 > m)                           # s and s-1 win ties
            m[k], d[k] = p2[k], 2
            v = m + x[t, cls]                             # float32 + float32: one rounding
            assert v.dtype == np.float32
    s = S - 1 if L == 0 or v[S - 1] >= v[S - 2] else S - 2
    if not v[s] > NEG:
        return None
    endv = v[s]
    st = np.empty(Tb, np.int64)
    for t in range(Tb - 1, -1, -1):
        st[t] = s
        s -= back[t, s]
    starts = np.array([np.nonzero(st == 2 * j + 1)[0][0] for j in range(L)], np.int32)
    ends = np.array([np.nonzero(st == 2 * j + 1)[0][-1] for j in range(L)], np.int32)
    return cls[st].astype(np.int32), starts.reshape(-1), ends.reshape(-1), endv


def align_batch(x, lens, labs, blank, max_label_len):
    """[B, T, V] logits -> (ali [B, T], starts, ends [B, M], end values [B],
    feasible [B]) in asr_ctc_align's output layout."""
    B, T, _ = x.shape
    ali = np.full((B, T), -1, np.int32)
    starts = np.full((B, max_label_len), -1, np.int32)
    ends = np.full((B, max_label_len), -1, np.int32)
    endv = np.full(B, NEG, np.float32)
    feas = np.zeros(B, bool)
    for b in range(B):
        Tb = max(min(int(lens[b]), T), 0)
        r = align_f32(x[b], Tb, labs[b], blank)
        if r is None:
            continue
        feas[b] = True
        L = len(labs[b])
        ali[b, :Tb], starts[b, :L], ends[b, :L], endv[b] = r
    return ali, starts, ends, endv, feas


def _log_softmax(x, dtype):
    x = np.asarray(x, dtype)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide='ignore'):
        return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype))


def score_f64(x, path):
    """(log-probability of `path`, A = sum |log-softmax| along it), float64."""
    n = len(path)
    if n == 0:
        return 0.0, 0.0
    lp = _log_softmax(np.asarray(x[:n], np.float64), np.float64)[np.arange(n), path]
    return float(lp.sum()), float(np.abs(lp).sum())


def score_f32(x, path):
    """The same sum with every value held in float32, frames added in order."""
    n = len(path)
    acc = np.float32(0)
    if n:
        lp = _log_softmax(np.asarray(x[:n], np.float32), np.float32)[np.arange(n), path]
        for v in lp:
            acc = np.float32(acc + v)
    return acc


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def enumerate_alignments(x, Tb, lab, blank):
    """Every state path of a tiny case as (score float64 on raw logits, state
    tuple), best first; among equal scores the path the backtrace's tie rule
    picks comes first: at the end the higher state, then going back in time
    the smaller step (stay before s-1 before s-2), i.e. the lexicographically
    LARGEST state sequence read from the last frame to the first."""
    cls = states(lab, blank)
    S = len(cls)
    out = []
    for st in itertools.product(range(S), repeat=Tb):
        if st[0] > 1 or st[-1] < S - 2:
            continue
        ok = True
        for a, b in zip(st, st[1:]):
            d = b - a
            if d < 0 or d > 2 or (d == 2 and not ((b & 1) and cls[b] != cls[a])):
                ok = False
                break
        if ok:
            out.append((float(sum(np.float64(x[t, cls[s]]) for t, s in enumerate(st))), st))
    out.sort(key=lambda r: (-r[0], tuple(-s for s in reversed(r[1]))))
    return out


# --------------------------------------------------------------------- cases
def _rand_labels(rng, L, V, blank, repeats):
    cl = [c for c in range(V) if c != blank]
    lab = rng.choice(cl, L) if L else np.zeros(0, np.int64)
    if len(cl) > 1:
        for j in range(1, L):       # no accidental repeats ...
            while lab[j] == lab[j - 1]:
                lab[j] = rng.choice(cl)
    for j in rng.permutation(np.arange(1, L))[:repeats] if L > 1 else []:
        lab[j] = lab[j - 1]         # ... then `repeats` places where one is made
    return np.asarray(lab, np.int64)


def n_repeats(lab):
    lab = np.asarray(lab)
    return int((lab[1:] == lab[:-1]).sum())


def make_case(seed, T, V, Ls, lens=None, blank=0, repeats=0, kind='randn', pad_nan=False):
    """dict(x [B, T, V] float32, lens, labs, blank, M)."""
    rng = np.random.RandomState(seed)
    B = len(Ls)
    if kind == 'randn':
        x = (3 * rng.randn(B, T, V)).astype(np.float32)
    elif kind == 'quarter':     # multiples of 1/4 in [-2, 2]: every sum is exact
        x = (rng.randint(-8, 9, (B, T, V)) / 4.0).astype(np.float32)
    else:
        x = np.zeros((B, T, V), np.float32)
    labs = [_rand_labels(rng, L, V, blank, repeats) for L in Ls]
    lens = np.full(B, T, np.int32) if lens is None else np.asarray(lens, np.int32)
    if pad_nan:
        for b in range(B):
            x[b, max(int(lens[b]), 0):] = np.nan
    return dict(x=x, lens=lens, labs=labs, blank=blank, M=max(list(Ls) + [0]))


def flat_labels(case):
    labs = case['labs']
    flat = np.concatenate([np.asarray(l, np.int32) for l in labs] + [np.zeros(0, np.int32)])
    return flat.astype(np.int32), np.array([len(l) for l in labs], np.int32)


def tight(seed, V, L, repeats, short=0, blank=0):
    """One utterance of L labels with T = L + repeats - short frames."""
    rng = np.random.RandomState(seed)
    lab = _rand_labels(rng, L, V, blank, repeats)
    T = L + n_repeats(lab) - short
    x = (3 * rng.randn(1, T, V)).astype(np.float32)
    return dict(x=x, lens=np.array([T], np.int32), labs=[lab], blank=blank, M=L)


def tier_case(L):
    """Both sides of a lane-ownership tier: T = L + 3, a sprinkling of repeats
    (feasible while repeats <= 3)."""
    return make_case(100 + L, L + 3, 37, [L], repeats=2)


def chunk_cases(chunk, lds):
    """T one short of, equal to and one past the backtrace's chunk size and its
    LDS-resident limit, and one T of at least three chunks beyond the limit."""
    Ts = sorted({chunk - 1, chunk, chunk + 1, lds - 1, lds, lds + 1, lds + 3 * chunk + 5})
    return {('T%d' % T): make_case(200 + T, T, 7, [5, 0, 9], lens=[T, T - 1, max(T - chunk, 1)],
                                   repeats=1) for T in Ts}


WIDTHS = (2, 5, 29, 257, 1025, 4099)


def width_case(V, blank):
    n = min(V - 1, 6)
    return make_case(300 + V + blank, 14, V, [n, min(n, 3), 1], lens=[14, 11, 6], blank=blank,
                     repeats=1 if V > 2 else 0)


def _fixed_cases():
    c = {}
    c['L0'] = make_case(1, 5, 5, [0])
    c['L1_T1'] = make_case(2, 1, 5, [1])
    c['T_eq_L'] = tight(3, 5, 6, 0)
    c['repeats_tight'] = tight(4, 5, 6, 2)
    c['repeats_short'] = tight(4, 5, 6, 2, short=1)          # infeasible
    c['len0'] = make_case(5, 4, 5, [0, 3, 2], lens=[0, 0, 4])   # L 0 and L > 0 with no frames
    for V in WIDTHS:
        c['V%d' % V] = width_case(V, 0)
        c['V%d_blank%d' % (V, V - 1)] = width_case(V, V - 1)
    c['B300'] = make_case(6, 3, 5, list(np.random.RandomState(6).randint(0, 3, 300)))
    c['ragged_nan'] = make_case(7, 20, 29, [4, 6, 2, 0], lens=[20, 13, 7, 1], repeats=1,
                                pad_nan=True)
    return c


CASES = _fixed_cases()
TIER_LS = (31, 32, 63, 64, 127, 128, 255, 256, 511)
# asr_ctc_align_limits as the constants were recorded (the GPU test asks the
# library and fails if they moved: record again)
CHUNK_FRAMES, LDS_FRAMES = 64, 256
EXACT = {'quarter': make_case(8, 40, 6, [7, 3, 12], lens=[40, 25, 31], repeats=2, kind='quarter'),
         'zeros': make_case(9, 17, 4, [5, 0, 2], lens=[17, 9, 3], repeats=1, kind='zeros')}


def score_cases():
    """The cases whose normalised scores are held to the bound."""
    c = {k: v for k, v in CASES.items() if k != 'B300'}
    c.update(('tier%d' % L, tier_case(L)) for L in TIER_LS)
    c.update(chunk_cases(CHUNK_FRAMES, LDS_FRAMES))
    return c


def k_score(case):
    """max over the case's feasible utterances of |score_f32 - score_f64|."""
    k = 0.0
    for b, lab in enumerate(case['labs']):
        Tb = max(min(int(case['lens'][b]), case['x'].shape[1]), 0)
        r = align_f32(case['x'][b], Tb, lab, case['blank'])
        if r is not None and Tb:
            k = max(k, abs(float(score_f32(case['x'][b], r[0])) - score_f64(case['x'][b], r[0])[0]))
    return k


def consts():
    with open(CONSTS_PATH) as f:
        return json.load(f)


def bound(kc, A):
    return MARGIN * max(kc, F32_U * A)


if __name__ == '__main__':
    import sys
    vals = {k: k_score(c) for k, c in sorted(score_cases().items())}
    for k, v in vals.items():
        print('%-24s K_score %.3g' % (k, v))
    if '--record' in sys.argv:
        with open(CONSTS_PATH, 'w') as f:
            json.dump(vals, f, indent=1, sort_keys=True)
            f.write('\n')
