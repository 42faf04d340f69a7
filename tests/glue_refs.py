"""float64 numpy references, forward and backward, of the autograd functions
that join the GEMM kernels into the attention models (native_ops.py:
linear_ex, linear2, mean_time, add_batch_sum, dropout), with the case tables
and operand generators that tests/test_glue_refs_cpu.py (references against
torch.autograd in float64) and tests/test_glue_ops_gpu.py (HIP ops against the
references) share.  numpy only; the dropout mask is oracle/rng.py's.

Weight and bias gradients are returned as the ops leave them: accumulated onto
the initial contents of the gradient buffer (gw0, gb0, ...), and for a column
window only inside the window.

Operands are small integers (inputs, weights, dy in [-3, 3]; biases and the
prefilled gradient buffers in [-8, 8]), so every product and sum below is
exact in f32 and in bf16 with f32 accumulation."""
import numpy as np

from oracle import rng as _rng

F64 = np.float64


def _f(a):
    return None if a is None else np.asarray(a, F64)


def linear_ex(x, w, b, b2, c0, K, t_index, dy, gw0, gb0=None, gb20=None):
    """y = x2d @ w[:, c0:c0+K].T + b + b2, x2d = x[:, t_index, :] of x [B, T, K]
    when t_index is given, else x over its leading dims.  Returns dict(y, dx,
    gw, gb, gb2): dx has x's shape (zero at every other time index), gw = gw0
    with dy^T x2d added into columns [c0, c0+K), gb / gb2 = gb0 / gb20 + column
    sums of dy (None without that bias)."""
    x, w, dy, gw0 = _f(x), _f(w), _f(dy), _f(gw0)
    Nout = w.shape[0]
    x2 = x[:, t_index, :] if t_index is not None else x.reshape(-1, K)
    win = w[:, c0:c0 + K]
    y = x2 @ win.T
    for bb in (b, b2):
        if bb is not None:
            y = y + _f(bb)
    dy2 = dy.reshape(-1, Nout)
    d2 = dy2 @ win
    if t_index is not None:
        dx = np.zeros_like(x)
        dx[:, t_index, :] = d2
        yshape = (x.shape[0], Nout)
    else:
        dx = d2.reshape(x.shape)
        yshape = x.shape[:-1] + (Nout,)
    gw = gw0.copy()
    gw[:, c0:c0 + K] += dy2.T @ x2
    db = dy2.sum(0)
    return dict(y=y.reshape(yshape), dx=dx, gw=gw,
                gb=None if b is None else _f(gb0) + db,
                gb2=None if b2 is None else _f(gb20) + db)


def linear2(x1, w1, b1, x2, w2, b2, dy, gw10, gw20, gb10=None, gb20=None):
    """y = x1 w1^T + b1 + x2 w2^T + b2 on the last dim.  Returns dict(y, dx1,
    dx2, gw1, gw2, gb1, gb2), the weight / bias gradients accumulated onto
    gw10, gw20, gb10, gb20."""
    x1, w1, x2, w2, dy = _f(x1), _f(w1), _f(x2), _f(w2), _f(dy)
    Nout = w1.shape[0]
    a1, a2 = x1.reshape(-1, x1.shape[-1]), x2.reshape(-1, x2.shape[-1])
    y = a1 @ w1.T + a2 @ w2.T
    for bb in (b1, b2):
        if bb is not None:
            y = y + _f(bb)
    dy2 = dy.reshape(-1, Nout)
    db = dy2.sum(0)
    return dict(y=y.reshape(x1.shape[:-1] + (Nout,)),
                dx1=(dy2 @ w1).reshape(x1.shape), dx2=(dy2 @ w2).reshape(x2.shape),
                gw1=_f(gw10) + dy2.T @ a1, gw2=_f(gw20) + dy2.T @ a2,
                gb1=None if b1 is None else _f(gb10) + db,
                gb2=None if b2 is None else _f(gb20) + db)


def mean_time(x, dout):
    """out[b] = mean_t x[b, t, :]; dx[b, t] = dout[b] / T.  dict(out, dx)."""
    x, dout = _f(x), _f(dout)
    T = x.shape[1]
    dx = np.broadcast_to(dout[:, None, :] / T, x.shape).copy()
    return dict(out=x.sum(1) / T, dx=dx)


def add_batch_sum(h, lower, dy):
    """y[b] = h[b] + sum_b' lower[b']; dh = dy; dlower[b] = sum_b' dy[b']."""
    h, lower, dy = _f(h), _f(lower), _f(dy)
    dl = np.broadcast_to(dy.sum(0, keepdims=True), lower.shape).copy()
    return dict(y=h + lower.sum(0, keepdims=True), dh=dy.copy(), dlower=dl)


def dropout_keep(n, p, seed):
    """Element i of a dropped tensor of n elements is kept iff u01(seed, i) >= p
    (p as the float32 the kernel receives)."""
    return _rng.u01(seed, n) >= np.float32(p)


def dropout(x, p, seed, dy):
    """y = x * keep / (1 - p), dx = dy * keep / (1 - p) with the same mask;
    1 - p formed in float32 as the kernel forms it, the division in float64.
    dict(y, dx, keep)."""
    x, dy = _f(x), _f(dy)
    keep = dropout_keep(x.size, p, seed).reshape(x.shape)
    q = F64(np.float32(1.0) - np.float32(p))
    return dict(y=x * keep / q, dx=dy * keep / q, keep=keep)


# ---------------------------------------------------------------------------
# Cases.  The kernel families (asr_gemm_last_family() // 4, csrc/prof.h
# ASR_PTAG_GEMM_*) the GPU test expects of a forward that is one GEMM launch
# are derived from the dispatch predicates of csrc/gemm.hip, not observed.
# ---------------------------------------------------------------------------
FAM_8R, FAM_FAST2, FAM_GEN_BF16, FAM_GEN_F32, FAM_F32F = 1, 5, 7, 8, 12
FAMILY_NAMES = {1: '8R', 5: 'FAST2', 7: 'GEN_BF16', 8: 'GEN_F32', 12: 'F32F'}

# linear_ex over all steps: x [B, S, K] (M = B S rows), weight [Nout, ldw],
# window [c0, c0 + K).  biases: which of (bias, bias2) are given.
#   fp32 mode: gemm_f32_fast (F32F) when both operands have a 16-B aligned
#   pointer and a row pitch % 4 == 0 (fast32_operand_ok), else gemm_kernel<false>.
#   bf16 mode: both f32 operands are staged to bf16 when 2 M N K >= 3.2e7,
#   K % 8 == 0 and (K % 8 == 0 columns) pointer 16-B aligned, pitch % 4 == 0
#   (plan_stage); the staged M >= 256, N >= 256 product takes the 8-wave ring
#   kernel (big8_ok).  Anything else keeps f32 operands: gemm_kernel<true>.
# name: (B, S, K, c0, ldw, Nout, biases, family fp32, family bf16)
LINEAR_EX_ALL = {
    # x pitch 5: neither fast path
    'tiny':            (3, 5, 5, 3, 11, 12, 'both', FAM_GEN_F32, FAM_GEN_BF16),
    'tiny_bias_only':  (3, 5, 5, 3, 11, 12, 'first', FAM_GEN_F32, FAM_GEN_BF16),
    'tiny_bias2_only': (3, 5, 5, 3, 11, 12, 'second', FAM_GEN_F32, FAM_GEN_BF16),
    'tiny_no_bias':    (3, 5, 5, 3, 11, 12, 'none', FAM_GEN_F32, FAM_GEN_BF16),
    # 2 * 2048 * 256 * 32 = 3.36e7 >= 3.2e7, every pointer and pitch aligned
    'staged_c0_0':     (8, 256, 32, 0, 48, 256, 'both', FAM_F32F, FAM_8R),
    # window base 16 B into the row: still a 16-B aligned f32 pointer
    'staged_c0_4':     (8, 256, 32, 4, 48, 256, 'both', FAM_F32F, FAM_8R),
    # window base 8 B into the row: staging and the f32 fast kernel decline
    'misaligned_c0_2': (8, 256, 32, 2, 48, 256, 'both', FAM_GEN_F32, FAM_GEN_BF16),
    # K % 8 != 0 (no staging) and weight pitch 50 % 4 != 0 (no f32 fast kernel)
    'ragged_k36_ld50': (8, 256, 36, 4, 50, 256, 'both', FAM_GEN_F32, FAM_GEN_BF16),
}

# linear_ex at a fixed time index: x [B, T, K], weight [Nout, K], one bias;
# the A rows have pitch T K and base offset t_index K.  All far below the
# staging threshold (bf16 mode: gemm_kernel<true>); fp32 mode takes the fast
# kernel iff T K % 4 == 0, t_index K % 4 == 0 and K % 4 == 0.
# (B, T, K, Nout, family fp32, family bf16)
LINEAR_EX_T = [
    (3, 7, 10, 7, FAM_GEN_F32, FAM_GEN_BF16),      # pitch 70
    (20, 5, 64, 64, FAM_F32F, FAM_GEN_BF16),
    (33, 2, 36, 130, FAM_F32F, FAM_GEN_BF16),      # pitch 72, offsets 0 / 36
]

# (M, K1, K2, Nout); the last: both products >= 3.2e7 flops (staged in bf16
# mode), its two dW products (reduction length 1024, 2 tiles each) take split-K
LINEAR2 = [(7, 5, 9, 3), (35, 24, 40, 16), (1024, 64, 128, 256)]
LINEAR2_BIASES = ['both', 'first', 'second', 'none']

# mean_time (B, T, E): a batched M = 1 product, A = ones(T) with pitch T and
# batch stride 0, B = x[b] K-major with pitch E and batch stride T E.
#   fp32 mode: F32F iff T % 4 == 0, E % 4 == 0 (and so T E % 4 == 0).
#   bf16 mode: staged iff 2 B T E >= 3.2e7, T % 8 == 0, E % 8 == 0; the staged
#   M = 1 product with a K-major B is neither 8-wave nor 256 x 64: the 128 x
#   128 fast kernel, two stages.
# (B, T, E, family fp32, family bf16)
MEAN_TIME = [
    (3, 7, 5, FAM_GEN_F32, FAM_GEN_BF16),
    (2, 1, 8, FAM_GEN_F32, FAM_GEN_BF16),          # ones pitch 1
    (4, 64, 32, FAM_F32F, FAM_GEN_BF16),
    (5, 33, 36, FAM_GEN_F32, FAM_GEN_BF16),        # ones pitch 33
    (3, 16, 6, FAM_GEN_F32, FAM_GEN_BF16),         # batch strides 96 / 6, x pitch 6
    (16, 2048, 512, FAM_F32F, FAM_FAST2),          # 2 B T E = 3.36e7: stage_map, A stride 0
]

ADD_BATCH_SUM = [(B, D) for B in (1, 3, 32, 33) for D in (5, 320, 1024)]

DROPOUT_N = [1, 5, 1023, 4097]
DROPOUT_P = [0.5, 0.2, 13107.0 / 65536.0]
DROPOUT_SEED = 0xDEADBEEFCAFEBABE


def ints(rs, shape, lim=3):
    return rs.randint(-lim, lim + 1, shape).astype(np.float32)


def nonzero_ints(rs, shape, lim=3):
    a = rs.randint(1, lim + 1, shape) * (2 * rs.randint(0, 2, shape) - 1)
    return a.astype(np.float32)


def _bias_pair(rs, Nout, which):
    b = ints(rs, (Nout,), 8) if which in ('both', 'first') else None
    b2 = ints(rs, (Nout,), 8) if which in ('both', 'second') else None
    return b, b2


def linear_ex_all_inputs(name):
    B, S, K, c0, ldw, Nout, biases = LINEAR_EX_ALL[name][:7]
    rs = np.random.RandomState(1000 + B * S + 7 * K + 13 * c0 + ldw)
    b, b2 = _bias_pair(rs, Nout, biases)
    return dict(x=ints(rs, (B, S, K)), w=ints(rs, (Nout, ldw)), b=b, b2=b2, c0=c0, K=K,
                t_index=None, dy=ints(rs, (B, S, Nout)), gw0=ints(rs, (Nout, ldw), 8),
                gb0=ints(rs, (Nout,), 8), gb20=ints(rs, (Nout,), 8))


def linear_ex_t_inputs(B, T, K, Nout, t_index):
    rs = np.random.RandomState(2000 + B + 3 * T + 5 * K + 11 * Nout + t_index)
    return dict(x=ints(rs, (B, T, K)), w=ints(rs, (Nout, K)), b=ints(rs, (Nout,), 8), b2=None,
                c0=0, K=K, t_index=t_index, dy=ints(rs, (B, Nout)),
                gw0=ints(rs, (Nout, K), 8), gb0=ints(rs, (Nout,), 8), gb20=None)


def linear2_inputs(M, K1, K2, Nout, biases):
    rs = np.random.RandomState(3000 + M + 3 * K1 + 5 * K2 + Nout)
    b1, b2 = _bias_pair(rs, Nout, biases)
    return dict(x1=ints(rs, (M, K1)), w1=ints(rs, (Nout, K1)), b1=b1, x2=ints(rs, (M, K2)),
                w2=ints(rs, (Nout, K2)), b2=b2, dy=ints(rs, (M, Nout)),
                gw10=ints(rs, (Nout, K1), 8), gw20=ints(rs, (Nout, K2), 8),
                gb10=ints(rs, (Nout,), 8), gb20=ints(rs, (Nout,), 8))


def mean_time_inputs(B, T, E):
    rs = np.random.RandomState(4000 + B + 3 * T + 5 * E)
    return dict(x=ints(rs, (B, T, E)), dout=ints(rs, (B, E)))


def add_batch_sum_inputs(B, D):
    rs = np.random.RandomState(5000 + B + 3 * D)
    return dict(h=ints(rs, (B, D)), lower=ints(rs, (B, D)), dy=ints(rs, (B, D)))


def dropout_inputs(n):
    """Nonzero x and dy, so the zeros of y and dx are the mask's."""
    rs = np.random.RandomState(6000 + n)
    return dict(x=nonzero_ints(rs, (n,)), dy=nonzero_ints(rs, (n,)))
