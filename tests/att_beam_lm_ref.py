"""Restatement of attention beam search with shallow fusion of an RNN language
model (the contract in the header of csrc/att_beam.hip) on the CPU, from the
encoder output on:

    lm_step            one step of the LM's stacked LSTM (torch's gate rows i, f,
                       g, o) and its output layer, in a chosen dtype; checked
                       against torch.nn.LSTM in f64 (tests/test_att_beam_lm_cpu.py)
    beam_decode_lm     att_beam_ctc_ref.beam_decode_joint, statement for statement,
                       with the LM's state carried per row and gamma * lp_lm(c | g)
                       added to every candidate's score; gamma == 0 runs no LM
                       statement and is beam_decode_joint bit for bit

The candidates stay the min(W, V) best ATTENTION classes of each row; the LM
steps at every t >= 0 (<sos> at t = 0) from the parent's LM state; LM class c is
attention class c.  dtype = torch.float32: the attention part, the LM and both
log-softmaxes run in f32 and the scores add up in double -- the device's
arithmetic; torch.float64: everything in f64.  The f32-against-f64 score error of
this restatement sets the score bound of tests/test_att_beam_lm_gpu.py.

A GRU decoder: run beam_decode_lm under att_beam_gru_ref._gru_for_lstm(), which
rebinds the one name the decoder cell is stepped through (the LM's cell is
stated here and is not affected)."""
import numpy as np
import torch

from att_beam_ctc_ref import PrefixScorer, ctc_log_probs
from att_beam_ref import _attend
from oracle import asr_ref


def lm_params(lm_sd, dtype):
    """The LM's state_dict (RNNLM / the reference's keys) in dtype."""
    return {k: v.detach().cpu().to(dtype) for k, v in lm_sd.items()}


def lm_layers(lp):
    return len([k for k in lp if k.startswith('lstm.weight_ih_l')])


def lm_step(lp, tok, h, c):
    """tok int64 [n]; h, c [n, layers, H].  Returns (logits [n, V], h, c)."""
    x = lp['embed.embed.weight'][tok]
    hs, cs = [], []
    for l in range(lm_layers(lp)):
        g = (x @ lp['lstm.weight_ih_l%d' % l].t() + lp['lstm.bias_ih_l%d' % l] +
             h[:, l] @ lp['lstm.weight_hh_l%d' % l].t() + lp['lstm.bias_hh_l%d' % l])
        i, f, gg, o = g.chunk(4, dim=1)
        cn = torch.sigmoid(f) * c[:, l] + torch.sigmoid(i) * torch.tanh(gg)
        x = torch.sigmoid(o) * torch.tanh(cn)
        hs.append(x)
        cs.append(cn)
    logits = x @ lp['output.fc.weight'].t() + lp['output.fc.bias']
    return logits, torch.stack(hs, dim=1), torch.stack(cs, dim=1)


def log_softmax_np(lg):
    mx = lg.max(axis=1, keepdims=True)
    return lg - mx - np.log(np.exp(lg - mx).sum(axis=1, keepdims=True))


@torch.no_grad()
def beam_decode_lm(sd, cfg, enc_out, lens, beam_width, max_len, min_len=0, penalty=0,
                   dtype=torch.float64, gaps=None, ctc_weight=0.0, task=0, num_classes=None,
                   num_units=None, lm_sd=None, lm_weight=0.0):
    """beam_decode_joint with the LM term.  Returns (hyps, scores, aws); gaps as
    beam_decode_joint's (the kept / dropped margin on the FUSED score)."""
    lam = float(ctc_weight)
    gam = float(lm_weight) if lm_sd is not None else 0.0
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if v.is_floating_point()}
    enc_all = torch.as_tensor(np.asarray(enc_out)).to(dtype)
    eos = cfg['num_classes'] if num_classes is None else num_classes
    D = cfg['decoder_num_units'] if num_units is None else num_units
    pre = 'attend_%d_fwd.' % task
    nl = cfg.get('decoder_num_layers', 1) if task == 0 else 1
    emb_w = p['embed_%d.embed.weight' % task]
    if gam > 0:
        lmp = lm_params(lm_sd, dtype)
        lm_H = lmp['lstm.weight_hh_l0'].shape[1]
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
        if gam > 0:
            lm_h = enc.new_zeros(1, lm_layers(lmp), lm_H)
            lm_c = enc.new_zeros(1, lm_layers(lmp), lm_H)
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
            if gam > 0:      # every t, <sos> at t = 0: the last token from the parent's state
                lm_lg, lm_h, lm_c = lm_step(lmp, torch.tensor([c['hyp'][-1] for c in beam]),
                                            lm_h[rows], lm_c[rows])
                lm_lp = log_softmax_np(lm_lg.numpy())
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
                        if gam > 0:
                            score = (beam[i]['score'] + (1.0 - lam) * float(lp[i, tk]) + lam * d +
                                     gam * float(lm_lp[i, tk]) + penalty)
                        else:
                            score = beam[i]['score'] + (1.0 - lam) * float(lp[i, tk]) + lam * d + penalty
                    elif gam > 0:
                        score = (beam[i]['score'] + float(lp[i, tk]) + gam * float(lm_lp[i, tk]) +
                                 penalty)
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
