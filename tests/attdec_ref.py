"""Reference of the teacher-forced location-attention decoder pass
(csrc/decoder.hip behind asr_attdec_forward_ex / asr_attdec_backward_ex; the
contract is include/asr_hip.h, "attention decoder") in plain torch, dtype-generic,
with autograd for every gradient.  Nothing here imports the product package;
oracle.rng supplies the dropout mask stream.

One pass over S steps (bahdanau order):
  t = 0   : no cell step; dec_0 = h0 (zeros when h0 is None), c_0 = 0,
            gates_0 = 0, x_0 = 0
  t >= 1  : x_t = [ctx_{t-1}; h_{t-1}]
            pre = pre_emb[:, t] + x_t Wcat^T,  Wcat = [W_ih[:, Y:] | W_hh]
            i, f, o = sigmoid, g = tanh (gate order i, f, g, o; saved activated)
            c_t = f c_{t-1} + i g,  h_t = o tanh(c_t) (* dropout scale [:, t])
  every t : f = conv1d(aw_{t-1}) (C channels, K taps, zero padding K // 2,
            aw_{-1} = 0), e = V . tanh(enc_a + W_dec h_t + W_conv f),
            e *= (frame < len) (multiplicative mask: a padded frame keeps
            energy 0, hence a weight, and enters the context), e *= sharpening,
            aw_t = softmax over all T frames, or element-wise sigmoid,
            ctx_t = sum_frames aw_t enc.

precision='bf16' places round_bf16 where the kernels round operands to bf16
(bf16 compute mode; everything else there is float32):
  cell product (cell_fwd<true>, the persistent forward's MFMA tiles): x_t and
    Wcat rounded, float32 accumulation;
  r = dgates_{t+1} Wcat (rgemm<true>, the persistent backward's r role): the
    gradient entering the cell product is rounded, Wcat rounded;
  dW_ih[:, Y:], dW_hh = dgates^T x (native_ops run_gemm): both rounded -- the
    same rounded dgates and the forward's rounded x;
  dW_dec = dwd^T dec and d enc = aw^T dctx_tot (run_gemm): both operands
    rounded; the forward products W_dec h_t and aw_t . enc, and d h_t / d aw_t
    through them, stay float32 (att_energy, att_context, att_bwd_*).
The gradient of pre_emb is the unrounded dgates; dV, dW_conv, the conv kernel's
gradient, d enc_a and d h0 are float32 sums.

case_constants: max |eval - f64| / max |f64| per tensor of the float32 and of
the bf16-emulated evaluation of this same reference; a GPU tensor may be
MARGIN x its constant off the float64 values (tests/test_attdec_gpu.py)."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import rng

F32_EPS = float(np.finfo(np.float32).eps)
# no float32 result is expected to beat its own final rounding
CONST_FLOOR = F32_EPS / 2
MARGIN = 16.0

FWD_KEYS = ('dec', 'c', 'gates', 'x', 'ctx', 'aw')
IN_KEYS = ('enc', 'enc_a', 'pre_emb', 'h0', 'w_ih', 'w_hh', 'w_dec', 'w_conv', 'conv_w', 'v')
GRAD_KEYS = tuple('d_' + k for k in IN_KEYS)


# --------------------------------------------------------------------------
# bf16 rounding with a straight-through gradient
# --------------------------------------------------------------------------
def _rb(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class _RoundBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _rb(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_rb(g) if ctx.bwd else g), None, None


def round_bf16(x, fwd=True, bwd=True):
    """Forward: x rounded to the nearest bf16 (ties to even); backward: the
    incoming gradient rounded likewise and passed straight through.  fwd / bwd
    = False leave that direction untouched (an operand only one pass rounds)."""
    return _RoundBF16.apply(x, fwd, bwd)


def _cell_product(x, wcat, bf16):
    """x Wcat^T.  bf16: both operands rounded; the gradient arriving at the
    product (dgates) is rounded once and feeds both r = dgates Wcat and
    dWcat = dgates^T x."""
    if not bf16:
        return x @ wcat.t()
    return round_bf16(round_bf16(x, bwd=False) @ round_bf16(wcat, bwd=False).t(), fwd=False)


def _wgrad_rounded(prod, a, w, bf16):
    """prod(a, w), bilinear.  bf16: value and d a in float32; d w formed from
    the rounded cotangent and the rounded a (a weight-gradient GEMM of
    native_ops).  The second term is zero in value and carries only d w."""
    if not bf16:
        return prod(a, w)
    y = prod(a, w.detach())
    p = round_bf16(prod(_rb(a.detach()), w), fwd=False)
    return y + (p - p.detach())


# --------------------------------------------------------------------------
# one attention step, one cell step
# --------------------------------------------------------------------------
def attention_step(enc, enc_a, mask, h, aw_prev, w_dec, w_conv, conv_w, v, sharpen, sigmoid,
                   bf16=False):
    """(ctx [B, E], aw [B, T]) from dec_out h [B, D] and aw_prev [B, T];
    mask [B, T] = (frame < len) in enc's dtype; conv_w [C, 1, 1, K], v [1, A]."""
    C, K = conv_w.shape[0], conv_w.shape[-1]
    f = Fn.conv1d(aw_prev.unsqueeze(1), conv_w.reshape(C, 1, K), padding=K // 2)   # [B, C, T]
    wd = _wgrad_rounded(lambda a, w: a @ w.t(), h, w_dec, bf16)                    # [B, A]
    pre = enc_a + wd.unsqueeze(1) + f.transpose(1, 2) @ w_conv.t()
    e = torch.tanh(pre) @ v.reshape(-1)                                            # [B, T]
    e = e * mask * sharpen
    aw = torch.sigmoid(e) if sigmoid else torch.softmax(e, dim=-1)
    ctx = _wgrad_rounded(lambda a, w: torch.einsum('bt,bte->be', a, w), aw, enc, bf16)
    return ctx, aw


def cell_step(pre_emb_t, x_t, c_prev, wcat, bf16=False):
    """(h, c, gates [B, 4D] activated) of one LSTMCell step on gate
    pre-activations pre_emb_t + x_t Wcat^T."""
    D = c_prev.shape[1]
    pre = pre_emb_t + _cell_product(x_t, wcat, bf16)
    i, f, g, o = pre.split(D, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], dim=1)


def frame_mask(lens, T, dtype):
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    return (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).to(dtype)


def decoder_pass(enc, enc_a, lens, pre_emb, h0, w_ih, w_hh, w_dec, w_conv, conv_w, v, sharpen=1.0,
                 sigmoid=False, drop=None, precision=None):
    """dict(dec [B,S,D], c [B,S,D], gates [B,S,4D], x [B,S,E+D], ctx [B,S,E],
    aw [B,S,T]) as the forward saves them.  w_ih [4D, Y+E]: only the columns
    from Y = w_ih.shape[1] - E on are used.  drop: [B,S,D] dropout scale or
    None.  precision: None (the tensors' dtype throughout) or 'bf16'."""
    bf16 = precision == 'bf16'
    B, T, E = enc.shape
    S = pre_emb.shape[1]
    D = w_hh.shape[1]
    Y = w_ih.shape[1] - E
    wcat = torch.cat([w_ih[:, Y:], w_hh], dim=1)
    mask = frame_mask(lens, T, enc.dtype)
    h = h0 if h0 is not None else enc.new_zeros(B, D)
    c = enc.new_zeros(B, D)
    gates = enc.new_zeros(B, 4 * D)
    x = enc.new_zeros(B, E + D)
    ctx = enc.new_zeros(B, E)
    aw = enc.new_zeros(B, T)
    out = {k: [] for k in FWD_KEYS}
    for t in range(S):
        if t > 0:
            x = torch.cat([ctx, h], dim=1)
            h, c, gates = cell_step(pre_emb[:, t], x, c, wcat, bf16)
            if drop is not None:
                h = h * drop[:, t]
        ctx, aw = attention_step(enc, enc_a, mask, h, aw, w_dec, w_conv, conv_w, v, sharpen,
                                 sigmoid, bf16)
        for k, val in zip(FWD_KEYS, (h, c, gates, x, ctx, aw)):
            out[k].append(val)
    return {k: torch.stack(val, dim=1) for k, val in out.items()}


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
# name -> B, T, E, A, C, K, D, S, Y (the issue's table; check_dims accepts all)
CASES = {
    'generic3':  (5, 61, 52, 24, 3, 11, 20, 7, 6),
    'generic4':  (32, 40, 64, 256, 4, 5, 64, 4, 8),
    'ten_rt':    (9, 100, 96, 64, 10, 21, 40, 9, 8),
    'prod_geom': (3, 70, 640, 128, 10, 201, 320, 3, 32),
    'ten_wideA': (4, 50, 48, 160, 10, 9, 32, 4, 8),
    'c16':       (3, 45, 40, 16, 16, 3, 24, 4, 8),
    'odd_ed':    (4, 37, 51, 20, 2, 7, 22, 5, 5),
    't_edge505': (2, 505, 16, 8, 1, 201, 8, 3, 4),
    't_edge513': (2, 513, 16, 8, 1, 201, 8, 3, 4),
    'k_wide':    (2, 300, 16, 8, 2, 257, 8, 3, 4),
    'tiny':      (1, 5, 8, 8, 1, 1, 8, 2, 4),
}
EXTRA_CASES = ('generic3', 'ten_rt', 'prod_geom', 'odd_ed')
DROP_SEED = 0x5EED0123456

# name -> dict(sigmoid, sharpen, h0, drop, env)
OPTIONS = {
    'softmax':  dict(sigmoid=False, sharpen=1.0, h0=True, drop=0.0),
    'sigmoid':  dict(sigmoid=True, sharpen=1.0, h0=True, drop=0.0),
    'sharp':    dict(sigmoid=False, sharpen=1.7, h0=True, drop=0.0),
    'sigsharp': dict(sigmoid=True, sharpen=1.7, h0=True, drop=0.0),
    'noh0':     dict(sigmoid=False, sharpen=1.0, h0=False, drop=0.0),
    'drop':     dict(sigmoid=False, sharpen=1.0, h0=True, drop=0.2),
    # the persistent backward recomputes the conv features instead of reading
    # the forward's (same mathematics: the reference of 'softmax')
    'nofeat':   dict(sigmoid=False, sharpen=1.0, h0=True, drop=0.0, env={'ASR_ATT_CONV_FEAT': '0'}),
}


def dims_of(case):
    return dict(zip('B T E A C K D S Y'.split(), CASES[case]))


def make_lens(B, T, K):
    """Descending, lens[0] = T; the last utterance has one frame and, from three
    utterances on, the one before it fewer frames than half the conv width."""
    if B == 1:
        return np.array([T], np.int32)
    lens = np.linspace(T, 1, B).astype(np.int32)
    if B >= 3:
        lens[-2] = max(1, min(int(lens[-2]), K // 2 - 1))
    return lens


@functools.lru_cache(maxsize=None)
def case_inputs(case, seed=0):
    """CPU float32 inputs of a case (shared by every option set; never
    modified): weights U(+-0.1), non-zero enc / enc_a beyond lens, random
    cotangents on dec and ctx."""
    p = dims_of(case)
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s, sc=0.1: (torch.rand(*s, generator=g) * 2 - 1) * sc   # noqa: E731
    B, T, E, A, C, K, D, S, Y = (p[k] for k in 'B T E A C K D S Y'.split())
    t = dict(enc=r(B, T, E, sc=1.0), enc_a=r(B, T, A, sc=1.0), pre_emb=r(B, S, 4 * D, sc=0.5),
             h0=r(B, D, sc=0.5), w_ih=r(4 * D, Y + E), w_hh=r(4 * D, D), w_dec=r(A, D),
             w_conv=r(A, C), conv_w=r(C, 1, 1, K), v=r(1, A))
    t['cot_dec'] = torch.randn(B, S, D, generator=g)
    t['cot_ctx'] = torch.randn(B, S, E, generator=g)
    t['lens'] = make_lens(B, T, K)
    return t


def drop_scale(case, opt):
    p = dims_of(case)
    if not opt['drop']:
        return None
    return rng.dropout_scale(DROP_SEED, (p['B'], p['S'], p['D']), opt['drop'])


def evaluate(case, optname, dtype=torch.float64, precision=None):
    """{tensor name: float64 numpy array}: the forward's saved tensors and the
    gradients of sum(dec cot_dec) + sum(ctx cot_ctx), evaluated in `dtype`
    (precision='bf16': float32 with the kernels' bf16 roundings)."""
    opt = OPTIONS[optname]
    inp = case_inputs(case)
    t = {k: inp[k].detach().to(dtype).clone().requires_grad_(True) for k in IN_KEYS}
    if not opt['h0']:
        t['h0'] = None
    ds = drop_scale(case, opt)
    drop = None if ds is None else torch.from_numpy(ds).to(dtype)
    out = decoder_pass(t['enc'], t['enc_a'], inp['lens'], t['pre_emb'], t['h0'], t['w_ih'],
                       t['w_hh'], t['w_dec'], t['w_conv'], t['conv_w'], t['v'], opt['sharpen'],
                       opt['sigmoid'], drop, precision)
    loss = (out['dec'] * inp['cot_dec'].to(dtype)).sum() + (out['ctx'] * inp['cot_ctx'].to(dtype)).sum()
    keys = [k for k in IN_KEYS if t[k] is not None]
    grads = torch.autograd.grad(loss, [t[k] for k in keys])
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    res.update({'d_' + k: g.double().numpy() for k, g in zip(keys, grads)})
    return res


def nerr(got, ref):
    """max |got - ref| / max |ref|: the unit of every bound here."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)


def _ref_key(optname):
    """Option sets that differ only in environment share a reference."""
    o = OPTIONS[optname]
    for k, v in OPTIONS.items():
        if all(v[f] == o[f] for f in ('sigmoid', 'sharpen', 'h0', 'drop')):
            return k
    return optname


@functools.lru_cache(maxsize=None)
def _reference(case, optname):
    f64 = evaluate(case, optname)
    f32 = evaluate(case, optname, torch.float32)
    b16 = evaluate(case, optname, torch.float32, 'bf16')
    cf = {k: max(nerr(f32[k], f64[k]), CONST_FLOOR) for k in f64}
    cb = {k: max(nerr(b16[k], f64[k]), CONST_FLOOR) for k in f64}
    return f64, cf, cb


def reference(case, optname):
    """The float64 tensors of (case, option set), computed once."""
    return _reference(case, _ref_key(optname))[0]


def case_constants(case, optname='softmax'):
    """({tensor: f32 constant}, {tensor: bf16-emulated constant}) in nerr units,
    floored at half a float32 eps.  The GPU bound on a tensor is MARGIN x the
    f32 constant in fp32 mode, MARGIN x the larger of the two in bf16 mode."""
    _, cf, cb = _reference(case, _ref_key(optname))
    return cf, cb


# --------------------------------------------------------------------------
# one standalone attention step (asr_att_step_forward / _backward)
# --------------------------------------------------------------------------
STEP_CASE, STEP_SHARPEN, STEP_SIGMOID = 'generic3', 2.0, True
STEP_IN_KEYS = ('enc', 'enc_a', 'dec_out', 'aw_prev', 'w_dec', 'w_conv', 'conv_w', 'v')


@functools.lru_cache(maxsize=None)
def step_inputs():
    """The decoder case's tensors plus a previous alignment (a softmax row per
    utterance, non-zero beyond lens as a decoder step leaves it) and a
    cotangent on the new weights."""
    inp = case_inputs(STEP_CASE)
    p = dims_of(STEP_CASE)
    g = torch.Generator().manual_seed(77)
    t = {k: inp[k] for k in ('enc', 'enc_a', 'w_dec', 'w_conv', 'conv_w', 'v', 'lens')}
    t['dec_out'] = inp['h0']
    t['aw_prev'] = torch.softmax(torch.randn(p['B'], p['T'], generator=g), dim=-1)
    t['cot_ctx'] = inp['cot_ctx'][:, 0].contiguous()
    t['cot_aw'] = torch.randn(p['B'], p['T'], generator=g)
    return t


def evaluate_step(dtype=torch.float64, precision=None):
    inp = step_inputs()
    t = {k: inp[k].detach().to(dtype).clone().requires_grad_(True) for k in STEP_IN_KEYS}
    mask = frame_mask(inp['lens'], inp['enc'].shape[1], dtype)
    ctx, aw = attention_step(t['enc'], t['enc_a'], mask, t['dec_out'], t['aw_prev'], t['w_dec'],
                             t['w_conv'], t['conv_w'], t['v'], STEP_SHARPEN, STEP_SIGMOID,
                             precision == 'bf16')
    loss = (ctx * inp['cot_ctx'].to(dtype)).sum() + (aw * inp['cot_aw'].to(dtype)).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in STEP_IN_KEYS])
    res = dict(ctx=ctx.detach().double().numpy(), aw=aw.detach().double().numpy())
    res.update({'d_' + k: g.double().numpy() for k, g in zip(STEP_IN_KEYS, grads)})
    return res


@functools.lru_cache(maxsize=None)
def step_reference():
    """(float64 tensors, f32 constants, bf16-emulated constants) of the step."""
    f64 = evaluate_step()
    f32 = evaluate_step(torch.float32)
    b16 = evaluate_step(torch.float32, 'bf16')
    return (f64, {k: max(nerr(f32[k], f64[k]), CONST_FLOOR) for k in f64},
            {k: max(nerr(b16[k], f64[k]), CONST_FLOOR) for k in f64})


# --------------------------------------------------------------------------
# which path a call takes (decoder.hip pd_eligible / pb_eligible / pd_kind)
# --------------------------------------------------------------------------
_GROUPS, _MEMBERS, _SLOTS, _CHUNKS, _THREADS = 8, 32, 4, 8, 512
_UMAX, _KMAX, _FPW, _CM, _KQ = 12, 16, 8, 4, 12
_LDS = 160 * 1024


def _cd(a, b):
    return -(-a // b)


def _a4(n):
    return (n + 3) & ~3


def pd_kind(p):
    if (p['C'], p['A'], p['E'], p['D'], p['K']) == (10, 128, 640, 320, 201):
        return 2
    return 1 if p['C'] == 10 and p['A'] <= 128 else 0


def _pd_lds_floats(p):
    B, T, E, A, C, K, D = (p[k] for k in 'B T E A C K D'.split())
    UPW, FCH, ECW, ED = _cd(D, _MEMBERS), _cd(T, _CHUNKS), _cd(E, _CHUNKS), E + D
    o = _SLOTS * ED + A * UPW + C * K + A * C + A + (T + 2 * (K // 2) + 16) + A + 4 * A
    o = _a4(o) + FCH * _a4(C) + _SLOTS * _UMAX + 6 * _SLOTS * 16 + 64 + _THREADS + 2048 + T * ECW
    return _a4(o)


def _pb_lds_floats(p, f32):
    B, T, E, A, C, K, D = (p[k] for k in 'B T E A C K D'.split())
    UPW, FCH, G4 = _cd(D, _MEMBERS), _cd(T, _CHUNKS), 4 * D
    W = FCH + K - 1
    o = _a4(FCH * E + FCH * A)
    o = _a4(o + C * 16 * _cd(K, 16) + A * C + A + E + W)
    o = _a4(o + FCH * _a4(C) + 4 * FCH + A)
    un = _SLOTS * G4 + 4 if f32 else _SLOTS * G4 // 2 + 4
    un = max(un, FCH * (A + 1), (8 + W) * C + _SLOTS * UPW * 8, 2048)
    o += un + 8 * _SLOTS * 16 + _SLOTS * A + A * UPW
    o += max(8 * A, _THREADS, 4 * _cd(FCH, 4) * 4 * C,
             (1 if FCH <= 16 else 2 if FCH <= 32 else 4) * 256) + 64
    return _a4(o)


def expected_path(case, precision, env):
    """dict(fwd, bwd: 1 = one persistent launch; fwd_tmpl, bwd_tmpl: the conv
    channel template asr_attdec_last_launch reports; chunks: 32-frame chunks)
    for a call without scheduled sampling on a device of at least 256 CUs."""
    p = dims_of(case)
    B, T, E, A, C, K, D, S = (p[k] for k in 'B T E A C K D S'.split())
    f32 = precision == 'fp32'
    ED, G4 = E + D, 4 * D
    ten = pd_kind(p) > 0
    common = (B <= _GROUPS * _SLOTS and _cd(D, _MEMBERS) <= _UMAX and _cd(T, _CHUNKS) <= 8 * _FPW
              and A <= 256 and (ten or C <= _CM) and env.get('ASR_ATT_PERSIST') != '0'
              and not (f32 and env.get('ASR_ATT_PERSIST32') == '0'))
    fwd = (common and ED % 8 == 0 and _cd(ED, 32) <= 2 * _KMAX and _cd(E, _CHUNKS) <= _THREADS
           and _pd_lds_floats(p) * 4 <= _LDS and B * S * ED * 4 < 2 ** 31 and B * T * 4 < 2 ** 31)
    bwd = (common and env.get('ASR_ATT_PERSIST_BWD') != '0' and _cd(ED, _MEMBERS) <= 32
           and G4 % 8 == 0 and _cd(_cd(G4, 32), 4) <= _KQ and K <= 256
           and not (f32 and _cd(_cd(G4, 4), 4) > 8 * _KQ)
           and _pb_lds_floats(p, f32) * 4 <= _LDS and B * S * G4 * 4 < 2 ** 31
           and B * T * C * 4 < 2 ** 31)
    step_tmpl = C if C in (10, 3) else 0
    pers_tmpl = 10 if ten else 0
    return dict(fwd=int(fwd), bwd=int(bwd), fwd_tmpl=pers_tmpl if fwd else step_tmpl,
                bwd_tmpl=pers_tmpl if bwd else step_tmpl, chunks=_cd(T, 32))


# --------------------------------------------------------------------------
# the GPU table: (case, option set, precision, dispatch)
# --------------------------------------------------------------------------
DISPATCH = {
    'default': {},
    'perstep': {'ASR_ATT_PERSIST': '0'},
    'pbwd0': {'ASR_ATT_PERSIST_BWD': '0'},
}


def _gpu_table():
    rows = []
    for case in CASES:
        opts = ['softmax', 'sigmoid']
        if case in EXTRA_CASES:
            opts += ['sharp', 'sigsharp', 'noh0', 'drop', 'nofeat']
        for o in opts:
            for prec in ('fp32', 'bf16'):
                for disp in DISPATCH:
                    if o == 'nofeat' and disp != 'default':
                        continue
                    if disp == 'pbwd0' and not expected_path(case, prec, {})['bwd']:
                        continue
                    rows.append((case, o, prec, disp))
    return rows


GPU_TABLE = _gpu_table()
