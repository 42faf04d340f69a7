"""Cases, float64 reference and error bounds of the CTC forward and its float32
gradient (csrc/ctc.hip: ctc_prep, ctc_emit, ctc_emit_wide, ctc_lse_from_parts,
ctc_emit_gather, the lattice's cost, ctc_loss_reduce, ctc_grad<true> /
ctc_grad<false>) at every width and layout those kernels branch on;
tests/test_ctc_paths_gpu.py holds the kernels to them, and
tests/test_ctc_paths_ref_cpu.py checks this module with the reference alone.
Nothing here imports the product package.

Reference: oracle.ctc_ref.ctc_batch in float64 -- costs [B] and the unscaled
gradient [B, T, V]; the GPU file multiplies the gradient by scale x grad_scale.
eval_f32: the same formulas with every value held in numpy float32
(ctc_width_ref.ctc_single_dtype); it only sizes the bounds.

Bounds (the convention of ctc_width_ref.bound / vgg_block_ref):

    gradient  |got - ref| <= MARGIN (16) x K_grad x max |ref|
              (and never above test_ctc_gpu.py's atol 2e-4 + rtol 1e-3 |ref|)
              K_grad = max |eval_f32 - ref| / max |ref| of the case, floored at
              half a float32 eps (vgg_block_ref.CONST_FLOOR)
    cost_b    |got - ref| <= MARGIN x max(K_cost, 2^-24 x A_b)
              K_cost = max_b |cost_f32 - cost_f64| of the case
              A_b = sum over t of |log-softmax| along the best (Viterbi)
              alignment of utterance b = viterbi_cost: what one float32
              rounding of each of the T terms of a path's log-probability costs

K_grad and K_cost are written into CONSTS below per case (measured with
measure(); the CPU test recomputes them and fails on a drift beyond 2x).  The
kernels use __expf / __logf and a base-2 lattice, so the margin of 16 is over a
different float32 evaluation, not over themselves.  The two multiplications by
scale and *grad_scale add two roundings of 2^-24 relative each, inside the
margin (the floor alone gives 16 x 2^-24); K_grad is measured on the unscaled
gradient.

Inputs: the boosted-alignment recipe of ctc_width_ref.case -- 3 x randn logits,
BOOST on an even alignment of every utterance -- which keeps the costs between
a fraction of a nat (V 2) and 95 nats (V 4099: ~6.7 nats per frame) and gives
every label class an occupancy >= 0.5 at some frame (label_occupancy; the CPU
test checks it).  Base shape B 3 x T 14, lengths
(14, 11, 6); utterance 0 holds an adjacent repeat, two classes of one 4-column
quad and the last class (small V: as many of these as V allows).

Input sets (case()):
    base            every width of WIDTHS, blank 0; V 5 / 1025 with blank V - 1
                    and a middle class
    shift           V 257 / 1025, the logits + 80 and - 80
    mask 'lead'     V 257 / 4099, blank V - 1: -inf on columns [0, 12) and
                    [1024 k, 1024 k + 12): for any row phase (0..3 floats before
                    the first 16-B boundary) the first two quads of the row and,
                    at V 4099, all sixteen values of threads 0 and 1's first
                    unrolled round of ctc_emit_wide, besides the row head
    mask 'slab'     V 1025: columns [192, 256) -inf -- one whole 64-column slab
                    of the head GEMM's partials is empty, (-inf, 0)
    infeasible      V 5 / 257: utterance 1 has 3 frames for 3 labels with an
                    adjacent repeat (needs 4)
    batch300        B 300 x T 3, V 5, label lengths in {0, 1, 2}

Findings on the GPU (an MI355X), in units of the bound: see the docstring of
tests/test_ctc_paths_gpu.py.
"""
import functools

import numpy as np

import ctc_width_ref as W
import vgg_block_ref as VR
from oracle import ctc_ref

MARGIN = VR.MARGIN
F32_U = 2.0 ** -24
BOOST = W.BOOST
NEG = -np.inf

TABLE_WIDTHS = (2, 3, 5, 64, 255, 256)        # ctc_emit, ctc_grad<true>
COMPACT_WIDTHS = (257, 773, 1023, 1024)       # ctc_emit, ctc_grad<false>
WIDE_WIDTHS = (1025, 3077, 4099)              # ctc_emit_wide, ctc_grad<false>
WIDTHS = TABLE_WIDTHS + COMPACT_WIDTHS + WIDE_WIDTHS
LAYOUT_WIDTHS = (5, 257, 1025, 3077)
LSE_WIDTHS = (64, 1024, 1025, 2051)           # nslab 1, 16, 17, 33
SHIFTS = (80.0, -80.0)

# id -> (K_grad, K_cost): measure() of every case, as printed by
# test_constants_are_current (K_grad in units of max |ref|, K_cost in nats).
CONSTS = {
    'V2':                          (1.44e-06, 1.19e-06),
    'V3':                          (6.6e-07, 1.18e-06),
    'V5':                          (8.25e-07, 7.51e-07),
    'V64':                         (4.09e-06, 1.77e-06),
    'V255':                        (1.1e-05, 6.71e-06),
    'V256':                        (6.63e-06, 3.35e-06),
    'V257':                        (6.6e-06, 2.47e-06),
    'V773':                        (8.88e-06, 4.93e-06),
    'V1023':                       (8.93e-06, 3.3e-06),
    'V1024':                       (1.41e-05, 5.48e-06),
    'V1025':                       (1.55e-05, 4.49e-06),
    'V3077':                       (1.62e-05, 8.97e-06),
    'V4099':                       (1.19e-05, 5.89e-06),
    'V5_blank4':                   (7.55e-07, 9.79e-07),
    'V5_blank2':                   (1.22e-06, 1.71e-06),
    'V1025_blank1024':             (5.19e-06, 1.62e-06),
    'V1025_blank512':              (9.39e-06, 8.32e-06),
    'V257_shift+80':               (5.38e-06, 1.01e-05),
    'V257_shift-80':               (8.37e-06, 2.89e-06),
    'V1025_shift+80':              (1.28e-05, 1.76e-05),
    'V1025_shift-80':              (6.13e-06, 8.02e-06),
    'V257_blank256_mask_lead':     (9.61e-06, 3.29e-06),
    'V4099_blank4098_mask_lead':   (1.79e-05, 8.12e-06),
    'V2051':                       (9.44e-06, 3.29e-06),
    'V1025_mask_slab':             (1.09e-05, 9e-06),
    'V5_infeasible':               (1.35e-06, 1.84e-06),
    'V257_infeasible':             (1.99e-05, 9.21e-06),
    'V5_batch300':                 (9.73e-07, 1.14e-06),
}


def mid_blank(V):
    return V // 2


def _labels(V, blank):
    """Utterance 0: an adjacent repeat, two classes of one 4-column quad and
    the last class; 1 and 2: classes elsewhere.  Below V = 64: the same from
    the few classes there are."""
    if V < 64:
        cl = [v for v in range(V) if v != blank]
        n = len(cl)
        labs = [[cl[0], cl[0]] + ([cl[1], cl[2]] if n >= 4 else []) + [cl[-1]],
                [cl[n // 2], cl[0]] if n >= 2 else [cl[0]],
                [cl[min(1, n - 1)]]]
        return labs
    last = V - 1 if blank != V - 1 else V - 2
    a = V // 3
    c = 4 * (V // 8) + 18
    labs = [[a, a, c, c + 1, last], [V // 2 - 7, 16, 3 * V // 4 - 20], [V - 9]]
    flat = [x for u in labs for x in u]
    assert blank not in flat and len(set(flat)) == len(flat) - 1 and c // 4 == (c + 1) // 4, (V, blank)
    assert all(0 <= x < V for x in flat)
    return labs


def _align(labels, Tb, blank):
    if not len(labels):
        return [blank] * Tb
    return W._align(labels, Tb, blank)


def mask_columns(V, mask):
    if mask == 'lead':
        return [v for k in range(0, min(V - 12, 3073), 1024) for v in range(k, k + 12)]
    if mask == 'slab':
        return list(range(192, 256))
    assert mask is None
    return []


@functools.lru_cache(maxsize=None)
def case(V, blank=0, shift=0.0, mask=None, kind='base'):
    """One input set, shared by every layout / entry point / scaling that runs
    it.  Arrays are read-only."""
    rng = np.random.RandomState(7000 + V + 31 * blank + (0 if kind == 'base' else 5) +
                                (int(shift) % 997))
    if kind == 'batch300':
        B, T = 300, 3
        label_lens = rng.randint(0, 3, B).astype(np.int32)
        labs = [[int(x) for x in rng.randint(1, V, L)] for L in label_lens]
        need = [len(u) + sum(a == b for a, b in zip(u, u[1:])) for u in labs]
        act_lens = np.array([rng.randint(max(n, 1), T + 1) for n in need], np.int32)
    else:
        B, T = 3, 14
        act_lens = np.array([14, 11, 6], np.int32)
        labs = _labels(V, blank)
        if kind == 'infeasible':
            act_lens = np.array([14, 3, 6], np.int32)
            cl = [v for v in range(V) if v != blank]
            labs[1] = [cl[1], cl[1], cl[2]]          # 3 labels + 1 repeat > 3 frames
        else:
            assert kind == 'base'
    label_lens = np.array([len(u) for u in labs], np.int32)
    labels = np.array([x for u in labs for x in u], np.int32)
    logits = (3.0 * rng.randn(B, T, V)).astype(np.float32)
    for b in range(B):
        for t, c in enumerate(_align(labs[b], int(act_lens[b]), blank)):
            logits[b, t, c] += np.float32(BOOST)
    if shift:
        logits = (logits + np.float32(shift)).astype(np.float32)
    cols = mask_columns(V, mask)
    if cols:
        assert blank not in cols and not set(cols) & set(int(x) for x in labels), (V, blank, mask)
        logits[:, :, cols] = -np.inf
    logits.setflags(write=False)
    feasible = np.array([len(u) + sum(a == b for a, b in zip(u, u[1:])) <= int(n)
                         for u, n in zip(labs, act_lens)])
    cid = 'V%d' % V
    if blank:
        cid += '_blank%d' % blank
    if shift:
        cid += '_shift%+d' % int(shift)
    if mask:
        cid += '_mask_' + mask
    if kind != 'base':
        cid += '_' + kind
    return dict(id=cid, key=(V, blank, shift, mask, kind), V=V, B=B, T=T, blank=blank,
                max_label_len=max(int(label_lens.max()), 1), act_lens=act_lens,
                label_lens=label_lens, labels=labels, labs=labs, logits=logits,
                feasible=feasible, mask_cols=cols)


def blank_cases():
    return [case(V, blank=b) for V in (5, 1025) for b in (0, V - 1, mid_blank(V))]


def shift_cases():
    return [case(V, shift=s) for V in (257, 1025) for s in SHIFTS]


def mask_cases():
    return [case(257, blank=256, mask='lead'), case(4099, blank=4098, mask='lead')]


def lse_cases():
    return [case(V) for V in LSE_WIDTHS] + [case(1025, mask='slab')]


def infeasible_cases():
    return [case(5, kind='infeasible'), case(257, kind='infeasible')]


def batch300_case():
    return case(5, kind='batch300')


def cases():
    """Every input set the GPU file runs, once."""
    out, seen = [], set()
    for c in ([case(V) for V in WIDTHS] + blank_cases() + shift_cases() + mask_cases() +
              lse_cases() + infeasible_cases() + [batch300_case()]):
        if c['id'] not in seen:
            seen.add(c['id'])
            out.append(c)
    return out


# --------------------------------------------------------------------------
# reference, float32 evaluation, Viterbi cost
# --------------------------------------------------------------------------
def _per_utterance(c, fn, dt=np.float64, logits=None):
    """fn(acts [T_b, V], labels, blank) -> (cost, grad [T_b, V]) over the batch."""
    x = c['logits'] if logits is None else logits
    B, T, V = x.shape
    costs = np.zeros(B, dt)
    grads = np.zeros((B, T, V), dt)
    off = 0
    for b in range(B):
        L, Tb = int(c['label_lens'][b]), int(c['act_lens'][b])
        costs[b], grads[b, :Tb] = fn(x[b, :Tb], c['labels'][off:off + L], c['blank'])
        off += L
    return costs, grads


@functools.lru_cache(maxsize=None)
def _ref(key):
    c = case(*key)
    costs, g = ctc_ref.ctc_batch(c['logits'], c['labels'], c['label_lens'], c['act_lens'],
                                 blank=c['blank'], time_major=False)
    costs.setflags(write=False)
    g.setflags(write=False)
    return costs, g


def costs_ref(c):
    """float64 costs [B] (0 for an infeasible utterance: zero_infinity)."""
    return _ref(c['key'])[0]


def grad_ref(c):
    """The unscaled float64 gradient [B, T, V] (softmax - occupancy)."""
    return _ref(c['key'])[1]


@functools.lru_cache(maxsize=None)
def _f32(key):
    c = case(*key)
    costs, g = _per_utterance(
        c, lambda a, l, bl: W.ctc_single_dtype(a, l, bl, np.float32), np.float32)
    assert costs.dtype == np.float32 and g.dtype == np.float32
    return costs, g


def eval_f32(c):
    """(costs, gradient) of the same formulas in numpy float32."""
    return _f32(c['key'])


def _lattice_parts(acts, labels, blank):
    acts = np.asarray(acts, np.float64)
    S = 2 * len(labels) + 1
    path = np.full(S, blank, np.int64)
    path[1::2] = labels
    return acts, S, path


def _shift(a, n, S):
    return np.concatenate([np.full(n, NEG), a])[:S]


def viterbi_cost_single(acts, labels, blank):
    """- log-probability of the best single alignment (max in place of the sum
    over alignments) = the sum of its T |log-softmax| terms; inf if infeasible."""
    acts, S, path = _lattice_parts(acts, labels, blank)
    m = acts.max(axis=1, keepdims=True)
    logp = acts - (m + np.log(np.exp(acts - m).sum(axis=1, keepdims=True)))
    emit = logp[:, path]
    skip = np.zeros(S, bool)
    skip[2:] = path[2:] != path[:-2]
    a = np.full(S, NEG)
    a[:2] = emit[0, :2]
    for t in range(1, acts.shape[0]):
        a = np.maximum(np.maximum(a, _shift(a, 1, S)), np.where(skip, _shift(a, 2, S), NEG)) + emit[t]
    return float(-np.max(a[-2:]))


@functools.lru_cache(maxsize=None)
def _viterbi(key):
    c = case(*key)
    out = np.zeros(c['B'])
    off = 0
    for b in range(c['B']):
        L, Tb = int(c['label_lens'][b]), int(c['act_lens'][b])
        out[b] = viterbi_cost_single(c['logits'][b, :Tb], c['labels'][off:off + L], c['blank'])
        off += L
    out.setflags(write=False)
    return out


def viterbi_cost(c):
    return _viterbi(c['key'])


def measure(c):
    """(K_grad, K_cost) of a case: the float32 evaluation's distance from
    float64 (module docstring)."""
    c64, g64 = costs_ref(c), grad_ref(c)
    c32, g32 = eval_f32(c)
    return (max(VR.nerr(g32, g64), VR.CONST_FLOOR),
            float(np.max(np.abs(c32.astype(np.float64) - c64))))


def cost_tol_of(c, k_cost):
    """[B]: MARGIN x max(K_cost, 2^-24 x A_b); 0 for an infeasible utterance
    (its cost is exact: 0 or +inf)."""
    a = np.where(c['feasible'], viterbi_cost(c), 0.0)
    return np.where(c['feasible'], MARGIN * np.maximum(k_cost, F32_U * a), 0.0)


def bound(c, scale=1.0, consts=None):
    """(tol_grad [B, T, V], tol_cost [B]) for the gradient x scale and the
    costs.  The gradient's bound is capped at what tests/test_ctc_gpu.py asserts
    (atol 2e-4 + rtol 1e-3, here on the scaled gradient): nothing in this file
    is ever looser than that."""
    k_grad, k_cost = CONSTS[c['id']] if consts is None else consts
    g = grad_ref(c) * scale
    tol_grad = np.minimum(MARGIN * k_grad * VR.scale_of(g),
                          2e-4 * abs(scale) + 1e-3 * np.abs(g))
    return tol_grad, cost_tol_of(c, k_cost)


def sum_bound(costs, loss_scale):
    """ctc_loss_reduce against the float64 sum of the same float32 costs: any
    summation order of B terms errs by at most gamma_B x sum |cost| (the kernel's
    tree is far shallower), the product with the scale by one rounding more."""
    n = len(costs) + 1
    gamma = n * F32_U / (1 - n * F32_U)
    return gamma * float(np.sum(np.abs(costs))) * abs(loss_scale)


def label_occupancy(c):
    """[(b, class, occupancy [T_b])] of every label class of every feasible
    utterance: softmax - gradient of the float64 reference on that column."""
    x = c['logits'].astype(np.float64)
    p = np.exp(x - x.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    g = grad_ref(c)
    out = []
    for b, labs in enumerate(c['labs']):
        if not c['feasible'][b]:
            continue
        Tb = int(c['act_lens'][b])
        for cl in sorted(set(int(x) for x in labs)):
            out.append((b, cl, p[b, :Tb, cl] - g[b, :Tb, cl]))
    return out


# --------------------------------------------------------------------------
# the head GEMM epilogue's log-sum-exp partials, built on the host
# --------------------------------------------------------------------------
def nslab_of(V):
    return (V + 63) // 64


def slab_partials(c):
    """f32 [nslab, B T, 2]: (max, sum exp(x - max)) of each 64-column slab of
    each row b T + t, in float64 from the logits, rounded to float32 -- the
    layout ctc_lse_from_parts documents, part[2 (q M + row)].  A slab that is
    all -inf is (-inf, 0); rows t >= act_lens[b] hold NaN (never read)."""
    B, T, V = c['logits'].shape
    x = c['logits'].astype(np.float64).reshape(B * T, V)
    ns = nslab_of(V)
    part = np.zeros((ns, B * T, 2), np.float32)
    for q in range(ns):
        xs = x[:, 64 * q:min(64 * q + 64, V)]
        m = xs.max(axis=1)
        with np.errstate(invalid='ignore'):
            s = np.where(np.isneginf(m), 0.0, np.exp(xs - m[:, None]).sum(axis=1))
        part[q, :, 0] = m
        part[q, :, 1] = s
    for b in range(B):
        part[:, b * T + int(c['act_lens'][b]):(b + 1) * T] = np.nan
    return part


def lse_from_partials(part):
    """float64 log-sum-exp [M] of the partials (what ctc_lse_from_parts forms)."""
    m = part[:, :, 0].astype(np.float64)
    s = part[:, :, 1].astype(np.float64)
    M = m.max(axis=0)
    with np.errstate(invalid='ignore'):
        w = np.where(np.isneginf(m), 0.0, s * np.exp(m - M))
    return M + np.log(w.sum(axis=0))


# --------------------------------------------------------------------------
# mutations of the reference (the CPU test: each exceeds the bound 4x somewhere)
# --------------------------------------------------------------------------
MUTATIONS = ('skip_across_repeat', 'last_class_not_normalised', 'slab_left_out',
             'blank_states_not_folded', 'row_head_left_out')


def ctc_mutant(acts, labels, blank, mut):
    """ctc_ref.ctc_single's formulas with one mistake a kernel could make:
      skip_across_repeat          the s-2 -> s transition also between equal labels
      last_class_not_normalised   class V - 1 missing from the log-sum-exp
      slab_left_out               columns [64, 128) missing from the log-sum-exp
      blank_states_not_folded     only the first blank state's occupancy is
                                  subtracted from the blank column
      row_head_left_out           columns [0, 3) (a row's floats before its first
                                  16-B boundary) missing from the log-sum-exp
    mut None: the oracle itself."""
    assert mut is None or mut in MUTATIONS
    acts, S, path = _lattice_parts(acts, labels, blank)
    T, V = acts.shape
    keep = np.ones(V, bool)
    if mut == 'last_class_not_normalised':
        keep[V - 1] = False
    elif mut == 'slab_left_out':
        keep[64:128] = False
    elif mut == 'row_head_left_out':
        keep[:3] = False
    xs = np.where(keep, acts, NEG)
    m = xs.max(axis=1, keepdims=True)
    logp = acts - (m + np.log(np.exp(xs - m).sum(axis=1, keepdims=True)))
    emit = logp[:, path]
    skip = np.zeros(S, bool)
    skip[2:] = path[2:] != path[:-2]
    if mut == 'skip_across_repeat':
        skip[2:] = path[2:] != blank
    alpha = np.full((T, S), NEG)
    alpha[0, :2] = emit[0, :2]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = ctc_ref._lse(a, _shift(a, 1, S), np.where(skip, _shift(a, 2, S), NEG)) + emit[t]
    beta = np.full((T, S), NEG)
    beta[T - 1, max(S - 2, 0):] = emit[T - 1, max(S - 2, 0):]
    skip_fwd = np.zeros(S, bool)
    skip_fwd[:-2] = skip[2:]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        b1 = np.concatenate([b[1:], [NEG]])
        b2 = np.concatenate([b[2:], [NEG, NEG]])[:S]
        beta[t] = ctc_ref._lse(b, b1, np.where(skip_fwd, b2, NEG)) + emit[t]
    logP = ctc_ref._lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, 0]
    if not np.isfinite(logP):
        return 0.0, np.zeros((T, V))
    with np.errstate(invalid='ignore'):
        occ = np.exp(alpha + beta - emit - logP)
    occ = np.where(np.isnan(occ), 0.0, occ)     # (-inf) - (-inf) of an unreachable masked state
    grad = np.exp(logp)
    for s in range(S):
        if mut == 'blank_states_not_folded' and s % 2 == 0 and s > 0:
            continue
        grad[:, path[s]] -= occ[:, s]
    return float(-logP), grad


def mutant(c, mut):
    """(costs, gradient) of the batch under ctc_mutant."""
    return _per_utterance(c, lambda a, l, bl: ctc_mutant(a, l, bl, mut))


def excess(c, costs, grad, consts=None):
    """max over the case of |error| / bound, gradient and feasible costs."""
    tol_g, tol_c = bound(c, consts=consts)
    r = float(np.max(np.abs(grad - grad_ref(c)) / tol_g))
    f = c['feasible']
    if f.any():
        r = max(r, float(np.max(np.abs(costs - costs_ref(c))[f] / tol_c[f])))
    return r
