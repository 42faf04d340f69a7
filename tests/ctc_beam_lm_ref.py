"""Float64 restatement of the CTC prefix beam search with shallow fusion of an
RNN language model and an insertion bonus (the contract at the top of
csrc/ctc_beam.hip; asr_ctc_beam_search_lm).

    S_t(l) = log P_ctc,t(l) + alpha sum_i log p_lm(l_i | <eos>, l_<i) + beta |l|

* search: the beam is a dict keyed by label tuples, so prefix identity is
  trivial; ALL V - 1 classes are proposed for every entry (no pruning by
  class), the LM and bonus terms are added on the extension edge, the beam is
  the W best distinct prefixes by S_t, and the final ranking adds alpha log
  p_lm(<eos> | l).  dtype float64 is the reference; float32 (the acoustic
  log-softmax, the LM, its log-softmax and every sum in f32 -- the device's
  arithmetic) is the unit of the score tolerance.  Besides the best hypothesis
  and its score it reports the final gap (best against second best final score),
  the smallest pruning gap (last kept against first dropped S_t over all
  frames), and whether a prefix came back into the beam while a child of its
  earlier self had stayed there.
* the LM is att_beam_lm_ref.lm_step, the float64 / float32 torch restatement of
  the stacked LSTM LM, over a parameter dict with RNNLM's state_dict keys.
  CTC class c != blank is LM class c - (c > blank); <eos> = V - 1 is also the
  start token.
* score_bruteforce: the final score of a prefix with the CTC term summed over
  all V^T alignments (tiny shapes only).

None of these calls a project kernel.
"""
import math

import numpy as np
import torch

import ctc_beam_ref as R0
from att_beam_lm_ref import lm_layers, lm_step

NEG_INF = -float('inf')


def make_lm(seed, V, layers, H, Y, scale=0.6):
    """A random LSTM LM over V classes with RNNLM's state_dict keys (f32)."""
    rng = np.random.RandomState(seed)
    u = lambda *s: torch.from_numpy(rng.uniform(-scale, scale, s).astype(np.float32))  # noqa: E731
    p = {'embed.embed.weight': u(V, Y)}
    for l in range(layers):
        p['lstm.weight_ih_l%d' % l] = u(4 * H, Y if l == 0 else H)
        p['lstm.weight_hh_l%d' % l] = u(4 * H, H)
        p['lstm.bias_ih_l%d' % l] = u(4 * H)
        p['lstm.bias_hh_l%d' % l] = u(4 * H)
    p['output.fc.weight'] = u(V, H)
    p['output.fc.bias'] = u(V)
    return p


def device_lm(p, dev, weight, cell='lstm'):
    """The dict native_ops.ctc_beam_search(lm=...) takes."""
    n = len([k for k in p if '.weight_ih_l' in k])
    pre = 'gru' if cell == 'gru' else 'lstm'
    d = lambda k: p[k].to(dev)  # noqa: E731
    return dict(cell=cell, weight=float(weight), emb=d('embed.embed.weight'),
                w_ih=[d('%s.weight_ih_l%d' % (pre, l)) for l in range(n)],
                w_hh=[d('%s.weight_hh_l%d' % (pre, l)) for l in range(n)],
                b_ih=[d('%s.bias_ih_l%d' % (pre, l)) for l in range(n)],
                b_hh=[d('%s.bias_hh_l%d' % (pre, l)) for l in range(n)],
                w_out=d('output.fc.weight'), b_out=d('output.fc.bias'))


class LM(object):
    """log p_lm(. | <eos>, prefix) rows in dtype, cached by prefix (LM classes)."""

    def __init__(self, params, dtype=np.float64):
        self.np_dtype = np.dtype(dtype)
        td = torch.float64 if self.np_dtype == np.float64 else torch.float32
        self.p = {k: v.detach().cpu().to(td) for k, v in params.items()}
        self.V = self.p['output.fc.weight'].shape[0]
        self.eos = self.V - 1
        n, H = lm_layers(self.p), self.p['lstm.weight_hh_l0'].shape[1]
        zero = torch.zeros(1, n, H, dtype=td)
        self._cache = {}
        self._put((), self.eos, zero, zero)

    def _put(self, key, tok, h, c):
        with torch.no_grad():
            lg, h, c = lm_step(self.p, torch.tensor([tok]), h, c)
        lg = lg.numpy()[0]
        mx = lg.max()
        row = (lg - mx) - np.log(np.exp(lg - mx).sum(dtype=self.np_dtype))
        self._cache[key] = (row.astype(self.np_dtype), h, c)

    def row(self, prefix):
        """prefix: a tuple of LM classes."""
        prefix = tuple(int(c) for c in prefix)
        if prefix not in self._cache:
            self.row(prefix[:-1])
            _, h, c = self._cache[prefix[:-1]]
            self._put(prefix, prefix[-1], h, c)
        return self._cache[prefix][0]


def lm_class(c, blank):
    return c - (1 if c > blank else 0)


def search(x, beam_width, blank=0, lm_params=None, alpha=0.0, beta=0.0, dtype=np.float64,
           normalize=True):
    """x [T, V]: raw logits (normalize) or log-probabilities of one utterance.
    Returns a dict: hyp (int64 CTC classes), score, final_gap, prune_gap (inf when
    nothing was ever dropped), recreated."""
    f32 = np.dtype(dtype) == np.float32
    conv = np.float32 if f32 else float
    lae = R0._lae32 if f32 else R0._lae64
    ninf = conv(NEG_INF)
    x = np.asarray(x)
    lp = R0.log_softmax(x, dtype) if normalize else x.astype(dtype)
    T, V = lp.shape
    use_lm = lm_params is not None and alpha > 0
    lm = LM(lm_params, dtype) if use_lm else None
    alpha, beta = conv(alpha), conv(beta)

    def lmrow(prefix):
        return lm.row(tuple(lm_class(c, blank) for c in prefix))

    beam = [((), (conv(0.0), ninf))]
    ever, prev_set = {()}, {()}
    prune_gap = float('inf')
    recreated = False
    for t in range(T):
        row = [conv(v) for v in lp[t]]
        nxt = {}
        for prefix, _ in beam:                       # stays first, by rank
            nxt[prefix] = [ninf, ninf]
        for prefix, (p_b, p_nb) in beam:
            e = nxt[prefix]
            e[0] = lae(e[0], lae(p_b, p_nb) + row[blank])
            if prefix:
                e[1] = lae(e[1], p_nb + row[prefix[-1]])
        for prefix, (p_b, p_nb) in beam:             # extensions by parent rank
            tot = lae(p_b, p_nb)
            last = prefix[-1] if prefix else -1
            q = lmrow(prefix) if use_lm else None
            edge = {}
            for c in range(V):
                if c == blank:
                    continue
                edge[c] = row[c] + alpha * conv(q[lm_class(c, blank)]) if use_lm else row[c]
            for c in sorted(edge, key=lambda c: (-edge[c], c)):
                e = nxt.setdefault(prefix + (c,), [ninf, ninf])
                e[1] = lae(e[1], edge[c] + beta + (p_b if c == last else tot))
        ranked = sorted(nxt.items(), key=lambda kv: -float(lae(kv[1][0], kv[1][1])))   # stable
        if len(ranked) > beam_width:
            prune_gap = min(prune_gap, float(lae(*ranked[beam_width - 1][1])) -
                            float(lae(*ranked[beam_width][1])))
        beam = [(p, (v[0], v[1])) for p, v in ranked[:beam_width]]
        cur = set(p for p, _ in beam)
        for p in cur - prev_set:
            if p in ever and any(len(q_) == len(p) + 1 and q_[:len(p)] == p and q_ in prev_set
                                 for q_ in cur):
                recreated = True
        ever |= cur
        prev_set = cur
    final = []
    for prefix, (p_b, p_nb) in beam:
        s = lae(p_b, p_nb)
        if use_lm:
            s = s + alpha * conv(lmrow(prefix)[lm.eos])
        final.append((float(s), prefix))
    order = sorted(range(len(final)), key=lambda i: -final[i][0])                      # stable
    best = final[order[0]]
    final_gap = best[0] - final[order[1]][0] if len(final) > 1 else float('inf')
    return dict(hyp=np.array(best[1], np.int64), score=best[0], final_gap=final_gap,
                prune_gap=prune_gap, recreated=recreated)


def score_bruteforce(lp, lm_params, prefix, alpha, beta, blank=0):
    """log P_ctc(prefix) over all V^T alignments + alpha (sum_i log p_lm(l_i |
    <eos>, l_<i) + log p_lm(<eos> | l)) + beta |l|, in float64.  lp [T, V]
    log-probabilities."""
    prefix = tuple(int(c) for c in prefix)
    s = R0.prefix_prob_bruteforce(lp, prefix, blank)
    if lm_params is not None and alpha > 0:
        lm = LM(lm_params, np.float64)
        lmp = tuple(lm_class(c, blank) for c in prefix)
        for i, c in enumerate(lmp):
            s += alpha * float(lm.row(lmp[:i])[c])
        s += alpha * float(lm.row(lmp)[lm.eos])
    return s + beta * len(prefix)
