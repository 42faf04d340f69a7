"""Restatement of AttentionSeq2seq._decode_infer_beam (bahdanau order, one
LSTMCell layer, location or content attention) on CPU torch in a chosen float
dtype, from the encoder output on: the f32-against-f64 score error of this
restatement sets the score bound of tests/test_att_beam_gpu.py."""
import numpy as np
import torch

from oracle import asr_ref


def _attend(p, pre, enc, enc_a, dec, aw_prev, sharpen, sigmoid):
    """One attention step over all frames of `enc` [n, L, E] (no padding)."""
    q = enc_a + (dec @ p[pre + 'W_dec_head0.fc.weight'].t()).unsqueeze(1)
    if pre + 'conv_head0.weight' in p:
        w = p[pre + 'conv_head0.weight']
        C, K = w.shape[0], w.shape[3]
        f = torch.nn.functional.conv1d(aw_prev.unsqueeze(1), w.view(C, 1, K), padding=K // 2)
        q = q + f.transpose(1, 2) @ p[pre + 'W_conv_head0.fc.weight'].t()
    e = (torch.tanh(q) @ p[pre + 'V_head0.fc.weight'].t()).squeeze(2) * sharpen
    aw = torch.sigmoid(e) if sigmoid else torch.softmax(e, dim=-1)
    return (enc * aw.unsqueeze(2)).sum(1), aw


@torch.no_grad()
def beam_decode(sd, cfg, enc_out, lens, beam_width, max_len, min_len=0, penalty=0,
                dtype=torch.float64, gaps=None):
    """Returns (hyps list of int64 arrays, scores list of float, aws list of [len, L]).
    gaps: a list that receives, per utterance, the smallest positive margin at a
    decision boundary, as the model's host path defines it (_gaps)."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if v.is_floating_point()}
    enc_all = torch.as_tensor(np.asarray(enc_out)).to(dtype)
    eos = cfg['num_classes']
    D = cfg['decoder_num_units']
    pre = 'attend_0_fwd.'
    emb_w = p['embed_0.embed.weight']
    hyps, scores, aws = [], [], []
    for b in range(enc_all.shape[0]):
        L = int(lens[b])
        enc = enc_all[b:b + 1, :L]
        enc_a = asr_ref.linear_nd(p, pre + 'W_enc_head0', enc)
        if cfg.get('init_dec_state', 'first') == 'zero':
            h = enc.new_zeros(1, D)
        else:
            h = torch.tanh(asr_ref.linear_nd(p, 'W_dec_init_0_fwd', enc[:, 0]))
        st = dict(h=h, c=enc.new_zeros(1, D), dec=h, ctx=enc.new_zeros(1, enc.shape[2]),
                  aw=enc.new_zeros(1, L))
        beam = [dict(hyp=[eos], score=0.0, row=0, hist=[])]
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
                hh, cc = asr_ref.lstm_cell(p, 'decoder_0_fwd.lstm_l0', x, cur['h'], cur['c'])
                cur.update(h=hh, c=cc, dec=hh)
            ctx, aw = _attend(p, pre, enc.expand(n, L, -1), enc_a.expand(n, L, -1), cur['dec'],
                              cur['aw'], cfg.get('sharpening_factor', 1),
                              cfg.get('sigmoid_smoothing', False))
            cur.update(ctx=ctx, aw=aw)
            st = cur
            z = torch.tanh(asr_ref.linear_nd(p, 'W_d_0_fwd', cur['dec']) +
                           asr_ref.linear_nd(p, 'W_c_0_fwd', ctx))
            lg = asr_ref.linear_nd(p, 'fc_0_fwd', z).numpy()
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
                    new.append(dict(hyp=beam[i]['hyp'] + [tk],
                                    score=beam[i]['score'] + float(lp[i, tk]) + penalty,
                                    row=i, hist=beam[i]['hist'] + [(t, i)]))
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
