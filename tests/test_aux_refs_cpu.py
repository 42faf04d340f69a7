"""The float64 references of tests/aux_refs.py against independent torch
implementations (so a wrong reference cannot bless a wrong kernel), and the
float32-evaluation error constants of test_aux_kernels_gpu.py recomputed.
Runs on the CPU; no project kernel is involved."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_refs as R
import test_aux_kernels_gpu as G
from oracle import asr_ref, ctc_ref

D = torch.float64


def _same(a, b, tol=1e-12):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=tol,
                               atol=tol)


@pytest.mark.parametrize('V,Rr', [(1, 3), (65, 9), (1000, 5)])
def test_xent_reference_matches_torch(V, Rr):
    rng = np.random.RandomState(3)
    x = R.xent_logits(rng, Rr, V)
    tgt = rng.randint(0, V, Rr)
    tgt[::2] = -1
    # CE: F.cross_entropy(ignore_index=-1, reduction='sum'), loss and gradient
    xt = torch.tensor(x, dtype=D, requires_grad=True)
    ce = F.cross_entropy(xt, torch.from_numpy(tgt), ignore_index=-1, reduction='sum')
    (ce * 0.37).backward()
    loss, dx, S = R.xent(x, tgt, None, 0, 1.0, 0.0, 0.37)
    _same(loss, ce.item())
    _same(dx, xt.grad.numpy())
    _same(S, abs(ce.item()))
    # LS with lens: the oracle's cross_entropy_label_smoothing
    T, lens = R.XENT_LENS[Rr]
    xt = torch.tensor(x, dtype=D, requires_grad=True)
    ls = asr_ref.ls_xent(xt.view(len(lens), T, V), lens, 0.1, size_average=False)
    ls.backward()
    loss, dx, _ = R.xent(x, None, np.asarray(lens), T, 0.0, 0.1)
    _same(loss, float(ls.detach()))
    _same(dx, xt.grad.numpy())
    # both, LS rows from targets >= 0; a target of V is V - 1
    both = R.xent(x, tgt, None, 0, 0.9, 0.1)
    xt = torch.tensor(x, dtype=D)
    lp = torch.log_softmax(xt, -1)[torch.from_numpy(tgt >= 0)]
    _same(both[0], 0.9 * ce.item() + 0.1 * float(-lp.sum() / V))
    hi = np.where(tgt == V - 1, V, tgt)
    hi[1] = V
    last = np.where(hi == V, V - 1, hi)
    _same(R.xent(x, hi, None, 0, 0.9, 0.1)[0], R.xent(x, last, None, 0, 0.9, 0.1)[0], 0)


def test_cell_references_match_torch_cells():
    torch.manual_seed(4)
    B, Din, H = 3, 6, 5
    x, h0, c0 = (torch.randn(B, n, dtype=D, requires_grad=True) for n in (Din, H, H))
    dh, dc = torch.randn(B, H, dtype=D), torch.randn(B, H, dtype=D)
    cell = torch.nn.LSTMCell(Din, H).double()
    h, c = cell(x, (h0, c0))
    ((h * dh).sum() + (c * dc).sum()).backward()
    pre = (x @ cell.weight_ih.T + cell.bias_ih + h0 @ cell.weight_hh.T + cell.bias_hh).detach()
    rh, rc, act, dpre, dcp = R.lstm_cell(pre.numpy(), c0.detach().numpy(), dh.numpy(), dc.numpy())
    _same(rh, h.detach())
    _same(rc, c.detach())
    _same(dcp, c0.grad)
    _same(dpre @ cell.weight_ih.detach().numpy(), x.grad)
    _same(dpre @ cell.weight_hh.detach().numpy(), h0.grad)
    _same(act[:, 2 * H:3 * H], np.tanh(pre.numpy()[:, 2 * H:3 * H]))
    # null c_prev / cotangents are zeros
    z = np.zeros((B, H))
    for a, b in ((R.lstm_cell(pre.numpy(), None, dh.numpy(), None),
                  R.lstm_cell(pre.numpy(), z, dh.numpy(), z)),):
        for p, q in zip(a, b):
            _same(p, q, 0)

    x, h0 = (torch.randn(B, n, dtype=D, requires_grad=True) for n in (Din, H))
    cell = torch.nn.GRUCell(Din, H).double()
    h = cell(x, h0)
    (h * dh).sum().backward()
    gi = (x @ cell.weight_ih.T + cell.bias_ih).detach().numpy()
    gh = (h0 @ cell.weight_hh.T + cell.bias_hh).detach().numpy()
    hout, act, dgi, dgh, dhp = R.gru_cell(gi, gh, h0.detach().numpy(), dh.numpy())
    _same(hout, h.detach())
    _same(dgi @ cell.weight_ih.detach().numpy(), x.grad)
    _same(dhp + dgh @ cell.weight_hh.detach().numpy(), h0.grad)   # direct term + dgh W_hh
    _same(dhp, dh.numpy() * act[:, H:2 * H])
    _same(dgi[:, :2 * H], dgh[:, :2 * H], 0)                      # r and z share the gradient
    _same(dgh[:, 2 * H:], dgi[:, 2 * H:] * act[:, :H])            # dgh_n = dp_n r


@pytest.mark.parametrize('pad', [None, 2])
def test_embedding_reference_matches_torch(pad):
    rng = np.random.RandomState(5)
    V, E, n = 7, 5, 60
    idx = rng.randint(0, V, n)
    w = torch.tensor(rng.randn(V, E), requires_grad=True)
    dout = rng.randn(n, E)
    g0 = rng.randn(V, E)
    out = F.embedding(torch.from_numpy(idx), w, padding_idx=pad)
    out.backward(torch.from_numpy(dout))
    _same(out.detach(), R.embedding_fwd(idx, w.detach().numpy()), 0)
    g, mag, cnt = R.embedding_bwd(idx, dout, V, pad, g0)
    _same(g, g0 + w.grad.numpy())
    assert (mag >= np.abs(g) - 1e-12).all()
    want = np.bincount(idx, minlength=V)
    if pad is not None:
        want[pad] = 0
    np.testing.assert_array_equal(cnt, want)
    # out of range: the row the forward reads
    oor = idx.copy()
    oor[:3], oor[3:5] = -1, V + 2
    _same(R.embedding_fwd(oor, w.detach().numpy()),
          w.detach().numpy()[np.clip(oor, 0, V - 1)], 0)
    _same(R.embedding_bwd(oor, dout, V, pad, g0)[0],
          R.embedding_bwd(np.clip(oor, 0, V - 1), dout, V, pad, g0)[0], 0)


@pytest.mark.parametrize('kind', [0, 1, 2, 3])
@pytest.mark.parametrize('clip', ['off_zero', 'active'])
def test_optimizer_reference_matches_torch_optim(kind, clip):
    rng = np.random.RandomState(6)
    n = 37
    c = dict(kind=kind, n=n, clip=clip, p=rng.randn(n).astype(np.float32),
             g=[rng.randn(n).astype(np.float32) for _ in range(3)])
    hp = R.optim_hp(kind)
    w = torch.tensor(c['p'], dtype=D, requires_grad=True)
    if kind == 0:
        opt = torch.optim.Adam([w], lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'],
                               weight_decay=hp['wd'])
    else:
        opt = torch.optim.SGD([w], lr=hp['lr'], momentum=hp['momentum'] if kind > 1 else 0.0,
                              dampening=hp['dampening'], nesterov=kind == 3,
                              weight_decay=hp['wd'])
    for step, hp_s, sqn, p64, m64, v64 in R.optim_run(c):
        w.grad = torch.tensor(c['g'][step - 1], dtype=D)
        if clip == 'active':
            # the reference clips by the float32 norm the kernel is handed; torch
            # by the float64 norm of the same gradient: equal to float32 rounding
            norm = torch.nn.utils.clip_grad_norm_([w], hp_s['max_norm'])
            assert abs(float(norm) - np.sqrt(float(sqn))) <= 1e-6 * float(norm)
            assert float(norm) > hp_s['max_norm']
        opt.step()
        tol = 1e-12 if clip == 'off_zero' else 1e-7
        _same(p64, w.detach(), tol)
        st = opt.state[w]
        if kind == 0:
            _same(m64, st['exp_avg'], tol)
            _same(v64, st['exp_avg_sq'], tol)
        elif kind > 1:
            _same(m64, st['momentum_buffer'], tol)


def test_clip_coefficient_matches_clip_grad_norm():
    rng = np.random.RandomState(7)
    g = rng.randn(50)
    for max_norm in (0.5, 100.0):
        w = torch.zeros(50, dtype=D, requires_grad=True)
        w.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([w], max_norm)
        _same(w.grad, g * float(R.clip_coef((g ** 2).sum(), max_norm)))
    assert float(R.clip_coef(None, 1.0)) == 1.0 and float(R.clip_coef(4.0, 0.0)) == 1.0


def test_best_path_oracle_on_hand_made_frames():
    """The collapse rules the GPU test's constructed cases rely on."""
    V = 5
    x = G._one_hot_frames(np.array([3, 3, 0, 3, 1, 1, 0, 0, 2]), V)
    np.testing.assert_array_equal(ctc_ref.greedy_best_path(x, [9], 0)[0], [3, 3, 1, 2])
    np.testing.assert_array_equal(ctc_ref.greedy_best_path(x, [9], 3)[0], [0, 1, 0, 2])
    np.testing.assert_array_equal(ctc_ref.greedy_best_path(x, [2], 0)[0], [3])
    assert len(ctc_ref.greedy_best_path(x, [0], 0)[0]) == 0
    x[0, 0, [1, 4]] = 5.0                       # a three-way tie: the first index wins
    assert ctc_ref.greedy_best_path(x, [1], 0)[0][0] == 1


def test_summation_bound():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    rng = np.random.RandomState(8)
    x = rng.randn(5000).astype(np.float32)
    s = np.float32(0)
    for v in x:                                  # the worst order a kernel may use
        s = np.float32(s + v)
    assert abs(float(s) - x.astype(np.float64).sum()) <= R.gamma(len(x)) * np.abs(x).sum()


def test_f32_reference_error_constants_are_reproduced():
    """The constants at the top of test_aux_kernels_gpu.py are what
    measure_f32_errors() gives (to the rounding of vectorised float32 libm
    kernels across CPUs: 25 %)."""
    got = R.measure_f32_errors()
    assert set(got) == set(G.F32_REF_ERR)
    for k, v in got.items():
        assert abs(v - G.F32_REF_ERR[k]) <= 0.25 * G.F32_REF_ERR[k], (k, v, G.F32_REF_ERR[k])
