"""CTC prefix beam search decoder (reference beam_search_decoder.py:22-124).

The reference walks T x V x beam in Python; here the search runs on the
device (native_ops.ctc_beam_search, csrc/ctc_beam.hip) and only the compact
hypotheses cross PCIe.  numpy inputs (decode_from_probs) are uploaded to the
current device first: there is no host implementation without an LM.  Returns
an object array of int arrays (ragged; the reference's ``np.array(best_hyps)``
of ragged lists fails on numpy >= 1.24).

alpha (LM weight) and beta (insertion bonus per label) -- arguments the
reference takes and ignores -- fuse an RNNLM into the search (the contract at
the top of csrc/ctc_beam.hip):

    S_t(l) = log P_ctc,t(l) + alpha sum_i log p_lm(l_i | <eos>, l_<i) + beta |l|

with the LM and bonus terms added on the extension edge, the beam the W best
distinct prefixes by S_t, and the final ranking by S_T(l) + alpha log
p_lm(<eos> | l).  CTC class c != blank is LM class c - (c > blank); the LM has
exactly as many classes as the CTC head, <eos> = the last one, which is also its
start token.  alpha == 0 and beta == 0 is the search without these terms, by
the launches it always had.

``host_search`` states the same contract in numpy doubles over the f32
log-softmax of one utterance's logits, with the LM stepped through
``rnnlm.step`` (f32 on the device ops): it serves what the kernels refuse (a
GRU LM, an LM deeper than ASR_ATT_BEAM_LM_MAX_LAYERS) and ``ASR_CTC_BEAM=host``,
and is the model-level oracle of the device path.  It proposes all V - 1
classes for every entry (no pruning), so it is for small jobs.
"""
import math
import os

import numpy as np
import torch

from ..... import native_ops as ops

NEG_INF = -float('inf')


def _lae(a, b):
    if a < b:
        a, b = b, a
    if b == NEG_INF:
        return a
    return a + math.log1p(math.exp(b - a))


def _log_softmax_f32(x):
    x = np.asarray(x, np.float32)
    m = x.max(axis=-1, keepdims=True)
    return ((x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32)))


class _HostLM(object):
    """The LM's f32 log-softmax row and state after each prefix of the beam."""

    def __init__(self, rnnlm):
        self.lm = rnnlm
        self.eos = rnnlm.num_classes - 1
        logits, state = rnnlm.step(np.array([self.eos], np.int64))
        self.rows = {(): self._row(logits)[0]}
        self.state = {(): state}

    @staticmethod
    def _row(logits):
        return _log_softmax_f32(logits.float().cpu().numpy()).astype(np.float64)

    def advance(self, prefixes, blank):
        """Keep the rows of `prefixes`; a new one steps from its parent's state
        (the parent was in the previous beam, so its state is here)."""
        new = [p for p in prefixes if p not in self.rows]
        if new:
            toks = np.array([p[-1] - (1 if p[-1] > blank else 0) for p in new], np.int64)
            par = [self.state[p[:-1]] for p in new]
            nl = len(par[0][0])
            hs = [torch.cat([s[0][l] for s in par], dim=0) for l in range(nl)]
            cs = [torch.cat([s[1][l] for s in par], dim=0) for l in range(nl)]
            logits, (hs, cs) = self.lm.step(toks, (hs, cs))
            rows = self._row(logits)
        keep_r, keep_s = {}, {}
        for p in prefixes:
            if p in self.rows:
                keep_r[p], keep_s[p] = self.rows[p], self.state[p]
        for i, p in enumerate(new):
            keep_r[p] = rows[i]
            keep_s[p] = ([h[i:i + 1] for h in hs], [c[i:i + 1] for c in cs])
        self.rows, self.state = keep_r, keep_s


def host_search(lp, beam_width, blank, alpha=0.0, beta=0.0, rnnlm=None):
    """One utterance: lp [T, V] log-probabilities (f32 values).  Returns (hyp
    int64 array, score float)."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    alpha = float(alpha) if rnnlm is not None else 0.0
    lm = _HostLM(rnnlm) if alpha > 0 else None
    beam = [((), (0.0, NEG_INF))]
    for t in range(T):
        row = lp[t]
        nxt = {}
        for prefix, (pb, pnb) in beam:          # stays first, by rank
            nxt[prefix] = [NEG_INF, NEG_INF]
        for prefix, (pb, pnb) in beam:
            tot = _lae(pb, pnb)
            e = nxt[prefix]
            e[0] = _lae(e[0], tot + row[blank])
            if prefix:
                e[1] = _lae(e[1], pnb + row[prefix[-1]])
        for prefix, (pb, pnb) in beam:          # extensions by parent rank, then by the list
            tot = _lae(pb, pnb)
            last = prefix[-1] if prefix else -1
            edge = {}
            for c in range(V):
                if c == blank:
                    continue
                v = row[c]
                if lm is not None:
                    v = v + alpha * lm.rows[prefix][c - (1 if c > blank else 0)]
                edge[c] = v
            for c in sorted(edge, key=lambda c: (-edge[c], c)):
                e = nxt.setdefault(prefix + (c,), [NEG_INF, NEG_INF])
                e[1] = _lae(e[1], edge[c] + beta + (pb if c == last else tot))
        ranked = sorted(nxt.items(), key=lambda kv: -_lae(kv[1][0], kv[1][1]))   # stable
        beam = [(p, (v[0], v[1])) for p, v in ranked[:beam_width]]
        if lm is not None:
            lm.advance([p for p, _ in beam], blank)
    best, best_s = None, NEG_INF
    for prefix, (pb, pnb) in beam:
        s = _lae(pb, pnb)
        if lm is not None:
            s += alpha * lm.rows[prefix][lm.eos]
        if best is None or s > best_s:
            best, best_s = prefix, s
    return np.array(best, np.int64), float(best_s)


class LanguageModelRequired(ValueError, NotImplementedError):
    """alpha > 0 without an LM.  A ValueError; also the NotImplementedError this
    call raised before the decoder took an LM, so callers that caught that still
    do."""


class BeamSearchDecoder(object):
    """Args as the reference: blank_index, space_index (unused there too)."""

    def __init__(self, blank_index, space_index=-1):
        self._blank = blank_index
        self._space = space_index

    @staticmethod
    def check_lm(alpha, beta, rnnlm, num_classes):
        """The LM search's preconditions (ValueError), checked before anything
        runs.  num_classes: the CTC head's width, blank included."""
        if alpha < 0:
            raise ValueError('CTC beam search: LM weight alpha = %r is negative' % (alpha,))
        if not np.isfinite(beta):
            raise ValueError('CTC beam search: insertion bonus beta = %r is not finite' % (beta,))
        if alpha > 0 and rnnlm is None:
            raise LanguageModelRequired('CTC beam search: alpha = %r > 0 needs a language model '
                                        '(rnnlm=)' % (alpha,))
        if alpha > 0 and rnnlm.num_classes != num_classes:
            raise ValueError('rnnlm.num_classes = %d (<eos> included), the CTC head has %d classes '
                             '(blank included): the LM must have exactly as many, <eos> in the '
                             "blank's place" % (rnnlm.num_classes, num_classes))

    def search(self, log_probs, x_lens, beam_width=1, alpha=0., beta=0., normalize=False,
               rnnlm=None):
        """The search, its result left on the device: (hyps int32 [B, T],
        hyp_lens int32 [B], scores float32 [B])."""
        if not torch.is_tensor(log_probs):
            log_probs = torch.from_numpy(np.ascontiguousarray(log_probs, dtype=np.float32))
        self.check_lm(alpha, beta, rnnlm, int(log_probs.shape[-1]))
        if not log_probs.is_cuda:
            log_probs = log_probs.to(torch.device('cuda', torch.cuda.current_device()))
        if not torch.is_tensor(x_lens):
            x_lens = torch.as_tensor(np.asarray(x_lens).astype(np.int32))
        lens = x_lens.to(log_probs.device).int()
        if alpha == 0 and beta == 0:
            return ops.ctc_beam_search(log_probs, lens, int(beam_width), self._blank,
                                       normalize=normalize)
        if not 1 <= int(beam_width) <= 64:
            raise ValueError('CTC beam search: beam_width = %r outside [1, 64]' % (beam_width,))
        res = None
        if os.environ.get('ASR_CTC_BEAM', '') != 'host':
            lm = None
            if alpha > 0:
                lm = dict(rnnlm.device_weights(), weight=float(alpha))
            res = ops.ctc_beam_search(log_probs, lens, int(beam_width), self._blank,
                                      normalize=normalize, lm=lm, beta=float(beta))
        if res is None:
            res = self._search_host(log_probs, lens, int(beam_width), alpha, beta, normalize,
                                    rnnlm)
        return res

    def _search_host(self, log_probs, lens, beam_width, alpha, beta, normalize, rnnlm):
        B, T, _ = log_probs.shape
        lens_np = np.clip(lens.cpu().numpy(), 0, T)
        hyps = np.zeros((B, T), np.int32)
        hl = np.zeros(B, np.int32)
        scores = np.zeros(B, np.float32)
        for b in range(B):
            lp = log_probs[b, :int(lens_np[b])].float().cpu().numpy()
            if normalize:
                lp = _log_softmax_f32(lp)
            h, s = host_search(lp, beam_width, self._blank, alpha, beta, rnnlm)
            hyps[b, :len(h)] = h
            hl[b] = len(h)
            scores[b] = s
        ops._ctc_beam['path'] = 'host'
        dev = log_probs.device
        return (torch.from_numpy(hyps).to(dev), torch.from_numpy(hl).to(dev),
                torch.from_numpy(scores).to(dev))

    def __call__(self, log_probs, x_lens, beam_width=1, alpha=0., beta=0., normalize=False,
                 rnnlm=None):
        """log_probs [B, T, num_classes] (numpy or device tensor), x_lens [B].
        normalize=True: ``log_probs`` holds raw logits and the log-softmax is
        fused into the kernel.  alpha: the weight of ``rnnlm`` (an RNNLM with
        num_classes classes, <eos> included); beta: the insertion bonus."""
        hyps, hl, _ = self.search(log_probs, x_lens, beam_width, alpha, beta, normalize, rnnlm)
        hyps, hl = hyps.cpu().numpy(), hl.cpu().numpy()
        out = np.empty(len(hl), dtype=object)
        for b in range(len(hl)):
            out[b] = hyps[b, :hl[b]].astype(np.int64)
        return out
