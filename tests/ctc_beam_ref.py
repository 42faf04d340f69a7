"""References for the CTC prefix beam search (asr_ctc_beam_search).

* beam_search: a restatement of the reference decoder
  (models/pytorch_v3/ctc/decoders/beam_search_decoder.py:22-124, alpha = beta =
  0) as a plain dictionary search over ALL W x V candidates, in the same loop
  order, in float64 (the reference) or float32 (the unit of the score
  tolerance).  Besides the best hypothesis and its score it reports how close
  the search came to a different answer: the final gap between the best and
  the second best prefix, and the smallest gap between the last kept and the
  first dropped candidate over all frames.  A case whose gaps are far above
  float32 rounding has one right answer for any float32 implementation.
* prefix_prob_bruteforce: log-probability of a prefix as the sum over all V^T
  alignments (tiny shapes only).
* restricted_search: a float64 model of the device algorithm (stay entries
  with merged extensions + pure extensions by the W + 1 best non-blank
  classes, prefixes as (parent, label) nodes).  With exact_identity=False it
  compares node ids instead of prefixes, which is the mistake the kernel's
  chain walk exists to avoid; the golden generator uses it to pick a case that
  tells the two apart.

None of these calls a project kernel.
"""
import itertools
import math

import numpy as np

NEG_INF = -float('inf')


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    m = x.max(axis=-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))).astype(dtype)


def _lae64(a, b):
    if a < b:
        a, b = b, a
    if b == NEG_INF:
        return a
    return a + math.log1p(math.exp(b - a))


def _lae32(a, b):
    return np.logaddexp(a, b)       # float32 operands -> float32


def beam_search(lp, beam_width, blank=0, dtype=np.float64):
    """lp [T, V] log-probabilities of one utterance.  Returns a dict: hyp (int64
    array), score, final_gap, prune_gap (inf when nothing was ever dropped),
    recreated (a prefix came back into the beam while a child of its earlier
    self had stayed there)."""
    f32 = np.dtype(dtype) == np.float32
    lae = _lae32 if f32 else _lae64
    conv = np.float32 if f32 else float
    ninf = conv(NEG_INF)
    lp = np.asarray(lp).astype(dtype)
    T, V = lp.shape
    beam = [((), (conv(0.0), ninf))]
    ever, prev_set = {()}, {()}
    prune_gap = float('inf')
    recreated = False
    for t in range(T):
        row = [conv(v) for v in lp[t]]
        nxt = {}
        for c in range(V):
            p_t = row[c]
            for prefix, (p_b, p_nb) in beam:
                if c == blank:
                    nb, nnb = nxt.get(prefix, (ninf, ninf))
                    nxt[prefix] = (lae(nb, lae(p_b + p_t, p_nb + p_t)), nnb)
                    continue
                end = prefix[-1] if prefix else None
                new = prefix + (c,)
                nb, nnb = nxt.get(new, (ninf, ninf))
                if c != end:
                    nnb = lae(nnb, lae(p_b + p_t, p_nb + p_t))
                else:
                    nnb = lae(nnb, p_b + p_t)
                nxt[new] = (nb, nnb)
                if c == end:
                    nb, nnb = nxt.get(prefix, (ninf, ninf))
                    nxt[prefix] = (nb, lae(nnb, p_nb + p_t))
        ranked = sorted(nxt.items(), key=lambda kv: lae(*kv[1]), reverse=True)
        if len(ranked) > beam_width:
            prune_gap = min(prune_gap, float(lae(*ranked[beam_width - 1][1])) -
                            float(lae(*ranked[beam_width][1])))
        beam = ranked[:beam_width]
        cur = set(p for p, _ in beam)
        for p in cur - prev_set:
            if p in ever and any(len(q) == len(p) + 1 and q[:len(p)] == p and q in prev_set
                                 for q in cur):
                recreated = True
        ever |= cur
        prev_set = cur
    score = float(lae(*beam[0][1]))
    final_gap = score - float(lae(*beam[1][1])) if len(beam) > 1 else float('inf')
    return dict(hyp=np.array(beam[0][0], np.int64), score=score, final_gap=final_gap,
                prune_gap=prune_gap, recreated=recreated)


def prefix_prob_bruteforce(lp, prefix, blank=0):
    """log sum over every alignment in V^T that collapses to `prefix`."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    prefix = tuple(int(c) for c in prefix)
    total = NEG_INF
    for path in itertools.product(range(V), repeat=T):
        col, last = [], None
        for c in path:
            if c != last and c != blank:
                col.append(c)
            last = c
        if tuple(col) == prefix:
            total = _lae64(total, float(sum(lp[t, c] for t, c in enumerate(path))))
    return total


def restricted_search(lp, beam_width, blank=0, exact_identity=True):
    """The device algorithm in float64 (csrc/ctc_beam.hip header).  Returns
    (hyp, score)."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    W, K = beam_width, beam_width + 1
    nodes = [(0, -1)]                            # (parent, label)

    def prefix(n):
        out = []
        while n != 0:
            out.append(nodes[n][1])
            n = nodes[n][0]
        return tuple(out[::-1])

    def same(a, b):
        return prefix(a) == prefix(b) if exact_identity else a == b

    beam = [dict(node=0, pb=0.0, pnb=NEG_INF, depth=0)]
    for t in range(T):
        row = [float(v) for v in lp[t]]
        top = sorted((c for c in range(V) if c != blank), key=lambda c: (-row[c], c))[:K]
        cands, merged = [], set()
        for i, e in enumerate(beam):
            tot = _lae64(e['pb'], e['pnb'])
            last = nodes[e['node']][1]
            npb, npnb = tot + row[blank], NEG_INF
            if last >= 0:
                npnb = e['pnb'] + row[last]
                for j, q in enumerate(beam):
                    if q['depth'] == e['depth'] - 1 and same(q['node'], nodes[e['node']][0]):
                        base = q['pb'] if nodes[q['node']][1] == last else _lae64(q['pb'], q['pnb'])
                        npnb = _lae64(npnb, row[last] + base)
                        merged.add((j, last))
                        break
            cands.append((-_lae64(npb, npnb), i, dict(node=e['node'], pb=npb, pnb=npnb,
                                                        depth=e['depth'])))
        for j, q in enumerate(beam):
            tot = _lae64(q['pb'], q['pnb'])
            for k, c in enumerate(top):
                if (j, c) in merged:
                    continue
                base = q['pb'] if nodes[q['node']][1] == c else tot
                cands.append((-(row[c] + base), 64 + j * K + k,
                              dict(parent=q['node'], label=c, depth=q['depth'] + 1)))
        cands.sort(key=lambda x: (x[0], x[1]))
        beam = []
        for s, _, e in cands[:W]:
            if 'label' in e:
                nodes.append((e['parent'], e['label']))
                e = dict(node=len(nodes) - 1, pb=NEG_INF, pnb=-s, depth=e['depth'])
            beam.append(e)
    return np.array(prefix(beam[0]['node']), np.int64), _lae64(beam[0]['pb'], beam[0]['pnb'])
