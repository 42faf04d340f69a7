"""Restatement of the joint CTC/attention beam search (the contract in the
header of csrc/att_beam.hip) on the CPU, from the encoder output on, written
from the equations with plain loops over the frames:

    PrefixScorer        the CTC prefix state (gn_t, gb_t), psi(g.c), the <eos>
                        term and the state of g.c, in float64
    beam_decode_joint   att_beam_ref.beam_decode's search with the candidate
                        score (1 - lam) lp_att(c) + lam delta_ctc(g, c)

dtype = torch.float32: the attention part and the CTC head's log-softmax run in
f32 and the prefix recursion in double -- the device's arithmetic; torch.float64:
everything in f64.  The f32-against-f64 score error of this restatement sets the
score bound of tests/test_att_beam_ctc_gpu.py."""
import math

import numpy as np
import torch

from att_beam_ref import _attend
from oracle import asr_ref

LOGZERO = -1.0e10


def logaddexp(a, b):
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


class PrefixScorer(object):
    """lp [L][Vc]: log-probabilities of one utterance's frames, class 0 blank;
    attention class c is CTC class c + 1.  A state is (gn [L], gb [L], psi)."""

    def __init__(self, lp):
        self.lp = [[float(v) for v in row] for row in np.asarray(lp, np.float64)]
        self.L = len(self.lp)

    def empty(self):
        gb, s = [], 0.0
        for t in range(self.L):
            s += self.lp[t][0]
            gb.append(s)
        return [LOGZERO] * self.L, gb, 0.0

    def _phi(self, st, g, c):
        gn, gb, _ = st
        if len(g) > 0 and g[-1] == c:
            return list(gb)
        return [logaddexp(gn[t], gb[t]) for t in range(self.L)]

    def psi(self, st, g, c):
        """psi(g.c), c != <eos>: the parent's state only."""
        phi = self._phi(st, g, c)
        acc = self.lp[0][c + 1] if len(g) == 0 else LOGZERO      # r_n[0]
        for t in range(1, self.L):
            acc = logaddexp(acc, phi[t - 1] + self.lp[t][c + 1])
        return acc

    def eos_term(self, st):
        gn, gb, _ = st
        return logaddexp(gn[self.L - 1], gb[self.L - 1])

    def delta(self, st, g, c, eos):
        if c == eos:
            return self.eos_term(st) - st[2]
        return self.psi(st, g, c) - st[2]

    def advance(self, st, g, c):
        phi = self._phi(st, g, c)
        gn = [self.lp[0][c + 1] if len(g) == 0 else LOGZERO]
        gb = [LOGZERO]
        for t in range(1, self.L):
            gn.append(logaddexp(gn[t - 1], phi[t - 1]) + self.lp[t][c + 1])
            gb.append(logaddexp(gn[t - 1], gb[t - 1]) + self.lp[t][0])
        return gn, gb, self.psi(st, g, c)


def ctc_log_probs(sd, head, enc, dtype):
    """[L, Vc] log-softmax of the CTC head over enc [L, E], in dtype; (lg - max) -
    log(sum(exp(lg - max)))."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if k.startswith(head + '.')}
    lg = asr_ref.linear_nd(p, head, enc.to(dtype)).numpy()
    mx = lg.max(axis=1, keepdims=True)
    return lg - mx - np.log(np.exp(lg - mx).sum(axis=1, keepdims=True))


@torch.no_grad()
def beam_decode_joint(sd, cfg, enc_out, lens, beam_width, max_len, min_len=0, penalty=0,
                      dtype=torch.float64, gaps=None, ctc_weight=0.0, task=0, num_classes=None,
                      num_units=None):
    """att_beam_ref.beam_decode with the joint score.  Returns (hyps, scores, aws);
    gaps receives per utterance the smallest positive margin at a decision
    boundary (the last kept candidate against the first dropped one on the JOINT
    score; per row the last class of the top-k against the next one on the
    attention log-probability).  task / num_classes / num_units: the sub-task of a
    hierarchical model (its parameter names end in _1).  The decoder is a plain
    stack of cfg['decoder_num_layers'] LSTMCell layers (att_beam_ref has one)."""
    lam = float(ctc_weight)
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if v.is_floating_point()}
    enc_all = torch.as_tensor(np.asarray(enc_out)).to(dtype)
    eos = cfg['num_classes'] if num_classes is None else num_classes
    D = cfg['decoder_num_units'] if num_units is None else num_units
    pre = 'attend_%d_fwd.' % task
    nl = cfg.get('decoder_num_layers', 1) if task == 0 else 1
    emb_w = p['embed_%d.embed.weight' % task]
    hyps, scores, aws = [], [], []
    for b in range(enc_all.shape[0]):
        L = int(lens[b])
        enc = enc_all[b:b + 1, :L]
        enc_a = asr_ref.linear_nd(p, pre + 'W_enc_head0', enc)
        if cfg.get('init_dec_state', 'first') == 'zero':
            h = enc.new_zeros(1, D)
        else:
            h = torch.tanh(asr_ref.linear_nd(p, 'W_dec_init_%d_fwd' % task, enc[:, 0]))
        st = dict(dec=h, ctx=enc.new_zeros(1, enc.shape[2]), aw=enc.new_zeros(1, L))
        for l in range(nl):
            st['h%d' % l], st['c%d' % l] = h, enc.new_zeros(1, D)
        beam = [dict(hyp=[eos], score=0.0, row=0, hist=[])]
        if lam > 0:
            scorer = PrefixScorer(ctc_log_probs(sd, 'fc_ctc_%d' % task, enc[0], dtype))
            beam[0]['ctc'] = scorer.empty()
        complete, step_aw = [], []
        gap = float('inf')
        for t in range(max_len):
            n = len(beam)
            if n == 0:
                break
            rows = torch.tensor([c['row'] for c in beam])
            cur = {k: v[rows] for k, v in st.items()}
            if t > 0:
                tok = torch.tensor([c['hyp'][-1] for c in beam])
                x = torch.cat([emb_w[tok], cur['ctx']], dim=-1)
                for l in range(nl):          # a plain stack: no residual connections
                    x, cc = asr_ref.lstm_cell(p, 'decoder_%d_fwd.lstm_l%d' % (task, l), x,
                                              cur['h%d' % l], cur['c%d' % l])
                    cur['h%d' % l], cur['c%d' % l] = x, cc
                cur['dec'] = x
            ctx, aw = _attend(p, pre, enc.expand(n, L, -1), enc_a.expand(n, L, -1), cur['dec'],
                              cur['aw'], cfg.get('sharpening_factor', 1),
                              cfg.get('sigmoid_smoothing', False))
            cur.update(ctx=ctx, aw=aw)
            st = cur
            z = torch.tanh(asr_ref.linear_nd(p, 'W_d_%d_fwd' % task, cur['dec']) +
                           asr_ref.linear_nd(p, 'W_c_%d_fwd' % task, ctx))
            lg = asr_ref.linear_nd(p, 'fc_%d_fwd' % task, z).numpy()
            mx = lg.max(axis=1, keepdims=True)
            lp = lg - mx - np.log(np.exp(lg - mx).sum(axis=1, keepdims=True))
            k_top = min(beam_width, lp.shape[1])
            order = np.argsort(-lp, axis=1, kind='stable')[:, :k_top]
            step_aw.append(aw)
            new = []
            for i in range(n):
                for k in range(k_top):
                    tk = int(order[i, k])
                    if tk == eos and len(beam[i]['hyp']) < min_len:
                        continue
                    if lam > 0:
                        d = scorer.delta(beam[i]['ctc'], beam[i]['hyp'][1:], tk, eos)
                        score = beam[i]['score'] + (1.0 - lam) * float(lp[i, tk]) + lam * d + penalty
                    else:
                        score = beam[i]['score'] + float(lp[i, tk]) + penalty
                    new.append(dict(hyp=beam[i]['hyp'] + [tk], score=score, row=i,
                                    hist=beam[i]['hist'] + [(t, i)]))
            new.sort(key=lambda c: c['score'], reverse=True)
            ds = []
            if len(new) > beam_width:
                ds.append(new[beam_width - 1]['score'] - new[beam_width]['score'])
            if k_top < lp.shape[1]:
                nxt = np.argsort(-lp, axis=1, kind='stable')[:, k_top]
                ds += [float(lp[i, order[i, k_top - 1]]) - float(lp[i, nxt[i]]) for i in range(n)]
            gap = min([gap] + [d for d in ds if d > 0])
            not_complete = []
            for cand in new[:beam_width]:
                (complete if cand['hyp'][-1] == eos else not_complete).append(cand)
            if len(complete) >= beam_width:
                complete = complete[:beam_width]
                break
            if lam > 0:
                for cand in not_complete[:beam_width]:
                    par = beam[cand['row']]
                    cand['ctc'] = scorer.advance(par['ctc'], par['hyp'][1:], cand['hyp'][-1])
            beam = not_complete[:beam_width]
        if len(complete) == 0:
            complete = beam
        if gaps is not None:
            gaps.append(gap)
        complete.sort(key=lambda c: c['score'], reverse=True)
        top = complete[0]
        hyps.append(np.array(top['hyp'][1:], dtype=np.int64))
        scores.append(float(top['score']))
        aws.append(torch.stack([step_aw[t][i] for t, i in top['hist']]).numpy())
    return hyps, scores, aws
