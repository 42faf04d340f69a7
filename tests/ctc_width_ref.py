"""Float64 reference and error bounds of the CTC gradient pass at the
vocabulary widths where csrc/ctc.hip changes its gradient kernel or the
kernel's chunks-per-thread template argument (tests/test_ctc_widths_gpu.py
holds asr_ctc_backward_bf16 / asr_ctc_backward_bf16_db to them).  Nothing here
imports the product package.

dy_ref: oracle.ctc_ref.ctc_batch in float64, times the gradient scale
(loss_scale x the upstream gradient): dY [B, T, V] and db [V] = its sum over
(b, t).  dy_f32: the same formulas (ctc_single's, restated over a dtype) with
every value held in numpy float32; it only sizes the bound.  bound: the
convention of tests/test_vgg_block_gpu.py (_check) --

    |got - ref| <= MARGIN (16) x const x max |ref|  (+ 2^-8 |ref| for bf16 dY)

with const = max |dy_f32 - dy_ref| / max |dy_ref| of the same case, floored at
half a float32 eps (vgg_block_ref.nerr / scale_of / CONST_FLOOR).  db gets no
bf16 term: the kernels sum it in f32 before the rounding.

Inputs: logits 3 x randn with BOOST added to the label classes along an even
alignment of every utterance (the 608-frame utterance: see LONG_LEVEL), so
label columns carry occupancies far above their bound
(test_ctc_width_ref_cpu.py checks that with the reference alone).
"""
import functools

import numpy as np

import vgg_block_ref as VR
from oracle import ctc_ref

MARGIN = VR.MARGIN
LOSS_SCALE = 1.0 / 3.0          # the C entry points' `scale`
GRAD_SCALE = 2.0                # the device scalar *grad_scale
BOOST = 6.0
# The 608-frame utterance: the float32 lattice's rounding grows with the cost
# (alpha + beta - log P at the cost's magnitude, summed over T steps), so its
# constant is ~1e-3 of max |ref| at a cost of thousands of nats.  Its inputs
# keep the cost near T ln 3 and the alignment sharp instead: unit-variance
# logits (log Z ~ ln V + 1/2 = 8.8) and the aligned class set to 8 + 0.3 randn,
# ~e^5 above any other class of the lattice at that frame, softmax ~0.3 -- every
# occupancy is near 0 or near 1, and where it is near 1, |ref| ~ 0.7 x scale.
LONG_LEVEL = 8.0

# (V, logits pitch P): the widths of the dispatch table in
# tests/test_ctc_widths_gpu.py.  gld = V rounded up to 8.
WIDTHS = ((2051, 2052), (2051, 2051), (4099, 4100), (6151, 6152), (10243, 10244),
          (14339, 14340), (16389, 16392))


def gld_of(V):
    return (V + 7) // 8 * 8


def _labels(V, blank):
    """Utterance 0: an adjacent repeat, two classes of one 8-column chunk and
    the last class; 1 and 2: classes spread over other chunks."""
    last = V - 1 if blank != V - 1 else V - 2
    a = V // 3
    c = 8 * (V // 16) + 2
    first = 1 if blank == 0 else 0
    labs = [[a, a, c, c + 1, last], [V // 2 + 5, first, 777], [V - 9]]
    flat = [x for u in labs for x in u]
    assert blank not in flat and len(set(flat)) == len(flat) - 1 and c // 8 == (c + 1) // 8
    return labs


def _align(labels, Tb, blank):
    """The class each frame of an even alignment sits on (a blank between
    adjacent repeats only)."""
    seq = []
    for i, l in enumerate(labels):
        if i and labels[i - 1] == l:
            seq.append(blank)
        seq.append(int(l))
    return [seq[t * len(seq) // Tb] for t in range(Tb)]


@functools.lru_cache(maxsize=None)
def case(V, blank=0, long_labels=False):
    """One input set (shared by every pitch / path / bias-block setting of a
    width).  long_labels: B = 2, max_label_len 300 (1024 padded lattice
    states), T = 608 for that utterance only."""
    rng = np.random.RandomState(1000 + V + (7 if blank else 0) + (13 if long_labels else 0))
    if long_labels:
        B, T, mll = 2, 2 * 300 + 8, 300
        act_lens = np.array([T, 9], np.int32)
        lab0 = rng.randint(1, V, 300)
        lab0[lab0 == blank] = 1
        lab0[10] = lab0[11]                      # an adjacent repeat
        lab0[20], lab0[21] = 2402, 2403          # one 8-column chunk
        lab0[299] = V - 1 if blank != V - 1 else V - 2
        labs = [list(lab0), [V // 2 + 5, 1, 777]]
    else:
        B, T, mll = 3, 14, 5
        act_lens = np.array([14, 11, 6], np.int32)
        labs = _labels(V, blank)
    label_lens = np.array([len(u) for u in labs], np.int32)
    labels = np.array([x for u in labs for x in u], np.int32)
    logits = ((1.0 if long_labels else 3.0) * rng.randn(B, T, V)).astype(np.float32)
    for b in range(B):
        for t, c in enumerate(_align(labs[b], int(act_lens[b]), blank)):
            if long_labels and b == 0:
                logits[b, t, c] = np.float32(LONG_LEVEL + 0.3 * rng.randn())
            else:
                logits[b, t, c] += np.float32(BOOST)
    logits.setflags(write=False)
    return dict(id='V%d%s%s' % (V, '_blank_last' if blank else '', '_long' if long_labels else ''),
                V=V, B=B, T=T, blank=blank, max_label_len=mll, act_lens=act_lens,
                label_lens=label_lens, labels=labels, labs=labs, logits=logits,
                loss_scale=LOSS_SCALE, grad_scale=GRAD_SCALE)


def cases():
    """Every input set the GPU file runs."""
    seen, out = set(), []
    for V, _ in WIDTHS:
        if V not in seen:
            seen.add(V)
            out.append(case(V))
    out.append(case(4099, blank=4098))
    out.append(case(4099, long_labels=True))
    return out


# --------------------------------------------------------------------------
# the formulas of oracle.ctc_ref.ctc_single over a dtype
# --------------------------------------------------------------------------
def _lse(dt, *xs):
    m = np.max(np.stack(xs), axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.zeros_like(m)
        for x in xs:
            s = s + np.exp(x - m)
        out = m + np.log(s)
    return np.where(np.isneginf(m), dt(-np.inf), out).astype(dt)


def ctc_single_dtype(acts, labels, blank, dt):
    """ctc_ref.ctc_single with every array and scalar of type dt."""
    acts = np.asarray(acts, dt)
    NEG = dt(-np.inf)
    T, V = acts.shape
    L = len(labels)
    S = 2 * L + 1
    path = np.full(S, blank, np.int64)
    path[1::2] = labels
    m = acts.max(axis=1, keepdims=True)
    logz = m + np.log(np.exp(acts - m).sum(axis=1, keepdims=True, dtype=dt))
    logp = acts - logz
    emit = logp[:, path]
    skip = np.zeros(S, bool)
    skip[2:] = path[2:] != path[:-2]
    neg1, neg2 = np.full(1, NEG, dt), np.full(2, NEG, dt)
    alpha = np.full((T, S), NEG, dt)
    alpha[0, 0] = emit[0, 0]
    if S > 1:
        alpha[0, 1] = emit[0, 1]
    for t in range(1, T):
        a = alpha[t - 1]
        a1 = np.concatenate([neg1, a[:-1]])
        a2 = np.where(skip, np.concatenate([neg2, a[:-2]])[:S], NEG)
        alpha[t] = _lse(dt, a, a1, a2) + emit[t]
    beta = np.full((T, S), NEG, dt)
    beta[T - 1, S - 1] = emit[T - 1, S - 1]
    if S > 1:
        beta[T - 1, S - 2] = emit[T - 1, S - 2]
    skip_fwd = np.zeros(S, bool)
    skip_fwd[:-2] = path[:-2] != path[2:]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        b1 = np.concatenate([b[1:], neg1])
        b2 = np.where(skip_fwd, np.concatenate([b[2:], neg2])[:S], NEG)
        beta[t] = _lse(dt, b, b1, b2) + emit[t]
    logP = (_lse(dt, alpha[T - 1, S - 1:S], alpha[T - 1, S - 2:S - 1])[0] if S > 1
            else alpha[T - 1, 0])
    if not np.isfinite(logP):
        return dt(0), np.zeros((T, V), dt)
    occ = np.exp(alpha + beta - emit - logP)
    grad = np.exp(logp)
    for s in range(S):
        grad[:, path[s]] -= occ[:, s]
    assert grad.dtype == dt and occ.dtype == dt
    return dt(-logP), grad


def _batch(c, dt):
    B, T, V = c['logits'].shape
    costs = np.zeros(B, dt)
    grads = np.zeros((B, T, V), dt)
    off = 0
    for b in range(B):
        L, Tb = int(c['label_lens'][b]), int(c['act_lens'][b])
        costs[b], grads[b, :Tb] = ctc_single_dtype(c['logits'][b, :Tb], c['labels'][off:off + L],
                                                   c['blank'], dt)
        off += L
    return costs, grads


def _key(c):
    return c['V'], c['blank'], c['max_label_len'] > 5


@functools.lru_cache(maxsize=None)
def _ref(key):
    c = case(*key)
    costs, g = ctc_ref.ctc_batch(c['logits'], c['labels'], c['label_lens'], c['act_lens'],
                                 blank=c['blank'], time_major=False)
    dy = g * (c['loss_scale'] * c['grad_scale'])
    db = dy.sum(axis=(0, 1))
    for a in (costs, g, dy, db):
        a.setflags(write=False)
    return costs, g, dy, db


def costs_ref(c):
    return _ref(_key(c))[0]


def grad_ref(c):
    """The unscaled float64 gradient (softmax - occupancy)."""
    return _ref(_key(c))[1]


def dy_ref(c):
    """(dY [B, T, V], db [V]) in float64."""
    return _ref(_key(c))[2:]


@functools.lru_cache(maxsize=None)
def _f32(key):
    c = case(*key)
    costs, g = _batch(c, np.float32)
    dy = g * (np.float32(c['loss_scale']) * np.float32(c['grad_scale']))
    db = np.zeros(c['V'], np.float32)
    for row in dy.reshape(-1, c['V']):        # sequential float32 row sums
        db = db + row
    assert dy.dtype == np.float32 and db.dtype == np.float32
    return costs, dy, db


def dy_f32(c):
    """(dY, db) of the same formulas in numpy float32."""
    return _f32(_key(c))[1:]


def constants(c):
    """{'dy', 'db'}: the float32 evaluation's distance from float64 in units of
    max |ref| (vgg_block_ref.nerr), floored at half a float32 eps."""
    (dy64, db64), (dy32, db32) = dy_ref(c), dy_f32(c)
    return dict(dy=max(VR.nerr(dy32, dy64), VR.CONST_FLOOR),
                db=max(VR.nerr(db32, db64), VR.CONST_FLOOR))


def bound(c):
    """(tol_dY [B, T, V], tol_db scalar, constants): what a bf16 dY and an f32
    db may differ from dy_ref by."""
    k = constants(c)
    dy64, db64 = dy_ref(c)
    tol_dy = MARGIN * k['dy'] * VR.scale_of(dy64) + 2.0 ** -8 * np.abs(dy64)
    tol_db = MARGIN * k['db'] * VR.scale_of(db64)
    return tol_dy, tol_db, k


def label_occupancy(c):
    """[(b, class, occupancy [T_b])] of every label class of every utterance:
    softmax - gradient of the float64 reference on that column."""
    x = c['logits'].astype(np.float64)
    p = np.exp(x - x.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    g = grad_ref(c)
    out = []
    for b, labs in enumerate(c['labs']):
        Tb = int(c['act_lens'][b])
        for cl in sorted(set(int(x) for x in labs)):
            out.append((b, cl, p[b, :Tb, cl] - g[b, :Tb, cl]))
    return out
