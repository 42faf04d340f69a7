"""Plain-Python restatement of asr_edit_distance (csrc/edit_distance.hip) for
the tests: the token-level clean-up, compute_wer's table (reference
utils/evaluation/edit_distance.py:53-126) and its backtrace with this
project's border rule.  Written from the specification in include/asr_hip.h,
apart from the host path in native_ops.py.
"""
import numpy as np


def clean(seq, n=None, is_hyp=False, eos=None, space=None, token_map=None):
    """Steps 1-3: the surviving tokens of seq[:n]."""
    seq = [int(t) for t in seq]
    seq = seq if n is None else seq[:max(0, int(n))]
    seq = [t for t in seq if t >= 0]                       # padding
    if is_hyp and eos is not None and eos in seq:          # 1. cut before the first eos
        seq = seq[:seq.index(eos)]
    if token_map is not None:                              # 2. rename / delete
        m = [int(v) for v in token_map]
        seq = [m[t] if t < len(m) else t for t in seq]
        seq = [t for t in seq if t >= 0]
    if space is not None and space >= 0:                   # 3. separator runs, both ends
        seq = [t for k, t in enumerate(seq) if not (t == space and k > 0 and seq[k - 1] == space)]
        if seq and seq[0] == space:
            seq = seq[1:]
        if seq and seq[-1] == space:
            seq = seq[:-1]
    return seq


def units(tokens, unit='token', space=None):
    """Steps 4-5.  Words are tuples of tokens; no tokens, no words (Python's
    ''.split('_') would give one empty word: deliberately not followed)."""
    if unit == 'token':
        return list(tokens)
    assert unit == 'word' and space is not None and space >= 0
    words, cur = [], []
    for t in tokens:
        if t == space:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    if cur:
        words.append(tuple(cur))
    return words


def table(ref, hyp):
    d = np.zeros((len(ref) + 1, len(hyp) + 1), np.int64)
    d[:, 0] = np.arange(len(ref) + 1)
    d[0, :] = np.arange(len(hyp) + 1)
    for i in range(1, len(ref) + 1):
        for j in range(1, len(hyp) + 1):
            if ref[i - 1] == hyp[j - 1]:
                d[i, j] = d[i - 1, j - 1]
            else:
                d[i, j] = 1 + min(d[i - 1, j - 1], d[i, j - 1], d[i - 1, j])
    return d


def counts(ref, hyp):
    """(distance, sub, ins, dele): the reference's backtrace; on the borders
    insertion at x == 0 and deletion at y == 0, where it has no rule."""
    d = table(ref, hyp)
    x, y = len(ref), len(hyp)
    sub = ins = dele = 0
    while not (x == 0 and y == 0):
        if x == 0:
            ins += 1
            y -= 1
        elif y == 0:
            dele += 1
            x -= 1
        elif d[x, y] == d[x - 1, y - 1] and ref[x - 1] == hyp[y - 1]:
            x -= 1
            y -= 1
        elif d[x, y] == d[x, y - 1] + 1:
            ins += 1
            y -= 1
        elif d[x, y] == d[x - 1, y - 1] + 1:
            sub += 1
            x -= 1
            y -= 1
        else:
            dele += 1
            x -= 1
    return int(d[len(ref), len(hyp)]), sub, ins, dele


def score(hyp, hyp_lens, ref, ref_lens, unit='token', eos=None, space=None, token_map=None):
    """Rows of (distance, sub, ins, dele, ref units) for padded or ragged
    batches, as asr_edit_distance's out."""
    out = np.zeros((len(hyp), 5), np.int64)
    for b in range(len(hyp)):
        r = units(clean(ref[b], ref_lens[b], False, eos, space, token_map), unit, space)
        h = units(clean(hyp[b], hyp_lens[b], True, eos, space, token_map), unit, space)
        out[b, :4] = counts(r, h)
        out[b, 4] = len(r)
    return out
