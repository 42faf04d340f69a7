"""CTC prefix scoring for the joint CTC/attention beam search of the host path
(AttentionSeq2seq._decode_infer_beam_host with ctc_weight > 0), in numpy
doubles.  The contract is the one csrc/att_beam.hip states: attention class c
is CTC class c + 1, blank is class 0, LOGZERO = -1.0e10 stands for log 0.

A hypothesis carries (phi, gb, psi): phi_t = logaddexp(gn_t, gb_t) and gb_t
over the utterance's frames, and its prefix score.  The two recurrences

    gn_t = logaddexp(gn_{t-1}, a_t) + lp_t(c)        a_t = phi'_{t-1} of the parent
    gb_t = logaddexp(gn_{t-1}, gb_{t-1}) + lp_t(blank)

are first-order in log space, x_t = logaddexp(x_{t-1}, a_t) + b_t, so with
S_t = b_1 + .. + b_t each is x_t = S_t + logcumsumexp(x_0, a_1 - S_0, a_2 - S_1,
..)_t: two np.logaddexp.accumulate calls per kept row instead of a Python loop
over the frames."""
import numpy as np

LOGZERO = -1.0e10


def log_softmax_f32(lg):
    """The search's f32 log-softmax, (lg - max) - log(sum(exp(lg - max)))."""
    lg = np.asarray(lg, np.float32)
    mx = lg.max(axis=-1, keepdims=True)
    return lg - mx - np.log(np.exp(lg - mx).sum(axis=-1, keepdims=True))


def _scan(x0, a, b):
    """x_0 = x0, x_t = logaddexp(x_{t-1}, a[t]) + b[t] for t >= 1 (a[0], b[0] unused)."""
    s = np.concatenate([[0.0], np.cumsum(b[1:])])
    y = np.concatenate([[x0], a[1:] - s[:-1]])
    return np.logaddexp.accumulate(y) + s


class CtcPrefixScorer(object):
    """lp: [L, Vc] log-probabilities of one utterance's own frames."""

    def __init__(self, lp):
        self.lp = np.asarray(lp, np.float64)
        self.L = self.lp.shape[0]

    def empty(self):
        gb = np.cumsum(self.lp[:, 0])
        return dict(phi=np.logaddexp(LOGZERO, gb), gb=gb, psi=0.0)

    def _prev(self, st, hyp, c):
        """phi'_{t-1} at index t (index 0 unused): gb alone when c repeats the last token."""
        src = st['gb'] if (len(hyp) > 0 and hyp[-1] == c) else st['phi']
        return np.concatenate([[LOGZERO], src[:-1]])

    def psi(self, st, hyp, c):
        """psi(hyp . c) for a class c != <eos>; hyp: the tokens after <sos>."""
        x = self._prev(st, hyp, c) + self.lp[:, c + 1]
        x[0] = self.lp[0, c + 1] if len(hyp) == 0 else LOGZERO
        return float(np.logaddexp.reduce(x))

    def eos(self, st):
        return float(st['phi'][self.L - 1])

    def advance(self, st, hyp, c, psi):
        a = self._prev(st, hyp, c)
        gn0 = self.lp[0, c + 1] if len(hyp) == 0 else LOGZERO
        gn = _scan(gn0, a, self.lp[:, c + 1])
        gb = _scan(LOGZERO, np.concatenate([[LOGZERO], gn[:-1]]), self.lp[:, 0])
        return dict(phi=np.logaddexp(gn, gb), gb=gb, psi=psi)
