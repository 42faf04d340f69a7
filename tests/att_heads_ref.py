"""Reference of one attention step over H heads (csrc/att_heads.hip behind
asr_att_heads_forward / asr_att_heads_backward; the contract is
include/asr_hip.h, "multi-head attention step") in plain torch, dtype-generic,
with autograd for every gradient.  Nothing here imports the product package.

Per head h (attention_layer.py:141-251):
  additive: f_h = conv1d(aw_prev[:, :, h]) (C channels, K taps, zero padding
            K // 2; absent for content attention),
            e_h = V_h . tanh(enc_a[:, :, :, h] + W_dec_h dec + W_conv_h f_h)
  dot:      e_h = enc_a[:, :, :, h] . dec
  e_h *= (frame < len) (multiplicative: a padded frame keeps energy 0, hence a
  weight, and enters the context), e_h *= sharpening, aw_h = softmax over all T
  frames or element-wise sigmoid, ctx_h = sum_frames aw_h enc.
Outputs: ctx [B, H*E] (head-major concatenation), aw [B, T, H].

nerr, CONST_FLOOR and MARGIN are attdec_ref's: a GPU tensor may be MARGIN x the
error of this reference's own float32 evaluation off its float64 values (the op
is f32 in both compute modes, so there is no bf16-emulated constant)."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from attdec_ref import CONST_FLOOR, MARGIN, frame_mask, nerr  # noqa: F401

# name -> kind, H, B, T, lens, E, A, D, C, K, sigmoid, sharpening
CASES = {
    'loc3':     ('location', 3, 3, 70, (70, 41, 1), 24, 20, 12, 3, 5, False, 1.0),
    'loc2_sig': ('location', 2, 2, 5, (5, 3), 8, 16, 8, 10, 11, True, 2.0),
    'con2':     ('content', 2, 3, 33, (33, 32, 7), 20, 12, 12, 0, 0, False, 1.0),
    'dot1':     ('dot_product', 1, 3, 70, (70, 64, 2), 24, 12, 12, 0, 0, False, 1.0),
    'dot3_sig': ('dot_product', 3, 2, 37, (37, 9), 16, 20, 20, 0, 0, True, 2.0),
}
FIELDS = 'kind H B T lens E A D C K sigmoid sharpen'.split()
ACT_KEYS = ('enc', 'enc_a', 'dec_out', 'aw_prev')
WEIGHT_KEYS = {'location': ('w_dec', 'w_conv', 'conv_w', 'v'), 'content': ('w_dec', 'v'),
               'dot_product': ()}


def dims_of(case):
    return dict(zip(FIELDS, CASES[case]))


def heads_step(enc, enc_a, mask, dec, aw_prev, heads, kind, sharpen, sigmoid):
    """(ctx [B, H*E], aw [B, T, H]).  enc [B,T,E], enc_a [B,T,A,H], mask [B,T],
    dec [B,D], aw_prev [B,T,H]; heads: per head a dict of w_dec [A,D], v [1,A]
    and, for location attention, w_conv [A,C], conv_w [C,1,1,K] (empty for
    dot_product)."""
    ctxs, aws = [], []
    for h, hd in enumerate(heads):
        ea = enc_a[..., h]
        if kind == 'dot_product':
            e = torch.einsum('bta,ba->bt', ea, dec)
        else:
            pre = ea + (dec @ hd['w_dec'].t()).unsqueeze(1)
            if kind == 'location':
                cw = hd['conv_w']
                C, K = cw.shape[0], cw.shape[-1]
                f = Fn.conv1d(aw_prev[..., h].unsqueeze(1), cw.reshape(C, 1, K), padding=K // 2)
                pre = pre + f.transpose(1, 2) @ hd['w_conv'].t()
            e = torch.tanh(pre) @ hd['v'].reshape(-1)
        e = e * mask * sharpen
        aw = torch.sigmoid(e) if sigmoid else torch.softmax(e, dim=-1)
        ctxs.append(torch.einsum('bt,bte->be', aw, enc))
        aws.append(aw)
    return torch.cat(ctxs, dim=-1), torch.stack(aws, dim=-1)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """CPU float32 inputs of a case (never modified): O(1) activations so tanh
    is neither linear nor saturated, non-zero enc / enc_a beyond lens, a random
    positive previous-weights row per (utterance, head), random cotangents."""
    p = dims_of(case)
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(case))
    r = lambda *s, sc=1.0: (torch.rand(*s, generator=g) * 2 - 1) * sc   # noqa: E731
    B, T, E, A, D, C, K, H = (p[k] for k in 'B T E A D C K H'.split())
    t = dict(enc=r(B, T, E), enc_a=r(B, T, A, H), dec_out=r(B, D))
    aw = torch.rand(B, T, H, generator=g) + 0.05
    t['aw_prev'] = aw / aw.sum(1, keepdim=True)
    heads = []
    for _ in range(H):
        hd = {}
        if p['kind'] != 'dot_product':
            hd['w_dec'] = r(A, D, sc=0.5)
            if p['kind'] == 'location':
                hd['w_conv'] = r(A, C, sc=0.5)
                hd['conv_w'] = r(C, 1, 1, K, sc=0.5)
            hd['v'] = r(1, A, sc=0.5)
        heads.append(hd)
    t['heads'] = heads
    t['cot_ctx'] = torch.randn(B, H * E, generator=g)
    t['cot_aw'] = torch.randn(B, T, H, generator=g)
    t['lens'] = np.asarray(p['lens'], np.int32)
    return t


def tensor_names(case):
    p = dims_of(case)
    names = ['ctx', 'aw'] + ['d_' + k for k in ACT_KEYS]
    for h in range(p['H']):
        names += ['d_%s%d' % (k, h) for k in WEIGHT_KEYS[p['kind']]]
    return names


def evaluate(case, dtype=torch.float64):
    """{name: float64 numpy array}: ctx, aw and the gradients of
    sum(ctx cot_ctx) + sum(aw cot_aw) w.r.t. enc, enc_a, dec_out, aw_prev and
    every head's weights ('d_w_dec0', ...), evaluated in `dtype`."""
    p = dims_of(case)
    inp = case_inputs(case)
    mk = lambda x: x.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731
    t = {k: mk(inp[k]) for k in ACT_KEYS}
    heads = [{k: mk(v) for k, v in hd.items()} for hd in inp['heads']]
    mask = frame_mask(inp['lens'], p['T'], dtype)
    ctx, aw = heads_step(t['enc'], t['enc_a'], mask, t['dec_out'], t['aw_prev'], heads,
                         p['kind'], p['sharpen'], p['sigmoid'])
    loss = (ctx * inp['cot_ctx'].to(dtype)).sum() + (aw * inp['cot_aw'].to(dtype)).sum()
    leaves = [('d_' + k, t[k]) for k in ACT_KEYS]
    for h, hd in enumerate(heads):
        leaves += [('d_%s%d' % (k, h), hd[k]) for k in WEIGHT_KEYS[p['kind']]]
    grads = torch.autograd.grad(loss, [v for _, v in leaves], allow_unused=True)
    res = dict(ctx=ctx.detach().double().numpy(), aw=aw.detach().double().numpy())
    for (k, v), gr in zip(leaves, grads):
        res[k] = (torch.zeros_like(v) if gr is None else gr).double().numpy()
    return res


@functools.lru_cache(maxsize=None)
def _reference(case):
    f64 = evaluate(case)
    f32 = evaluate(case, torch.float32)
    return f64, {k: max(nerr(f32[k], f64[k]), CONST_FLOOR) for k in f64}


def reference(case):
    """The float64 tensors of a case, computed once."""
    return _reference(case)[0]


def case_constants(case):
    """{tensor: constant}: nerr of this reference's float32 evaluation against
    its float64 one, floored at half a float32 eps.  The GPU bound on a tensor
    is MARGIN x its constant."""
    return _reference(case)[1]
