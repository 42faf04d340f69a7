"""Per-step recurrence workspace arena (round 6, native_ops.rec_arena_begin).

The encoder forward clears one buffer holding a granule workspace for every
BLSTM layer pass of the step, and those launches skip their own memset.  The
recurrences must compute bitwise what they compute with a fresh, memset
workspace per launch (ASR_REC_ARENA=0), also when a second forward clears the
arena again before the first one's backward ran (its reservations are then
stale and its backward takes a private workspace).
"""
import numpy as np
import pytest
import torch

from test_grad_buckets_gpu import _batch, _kw
from test_model_ctc import _build


def _loss_grad(m, batch):
    m.zero_grad()
    loss = m(batch['xs'], batch['ys'], batch['x_lens'], batch['y_lens'])
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), m._flat_grad.clone()


@pytest.fixture
def bf16_mode():
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.set_compute_dtype('bf16')
    yield
    native_ops.set_compute_dtype('fp32')


@pytest.mark.gpu
def test_arena_bitwise_equals_per_launch_memset(cuda_dev, monkeypatch, bf16_mode):
    from pytorch_end2end_speech_recognition_amd import native_ops
    H, L = 256, 3
    torch.manual_seed(1623)
    sd = {k: v.clone() for k, v in _build(_kw(H, L)).state_dict().items()}
    b1, b2 = _batch(T=160, seed=1), _batch(T=200, seed=2)

    def fresh():
        m = _build(_kw(H, L))
        m.load_state_dict(sd)
        m.set_cuda()
        return m

    monkeypatch.setenv('ASR_REC_ARENA', '0')
    m = fresh()
    ref = [_loss_grad(m, b1), _loss_grad(m, b2)]

    monkeypatch.setenv('ASR_REC_ARENA', '1')
    m = fresh()
    got = [_loss_grad(m, b1), _loss_grad(m, b2), _loss_grad(m, b1)]
    for (l0, g0), (l1, g1) in zip(ref + ref[:1], got):
        assert l0 == l1
        assert torch.equal(g0, g1), int((g0 != g1).sum())

    # two forwards, then the two backwards: the first forward's backward
    # reservations are stale once the second forward cleared the arena
    m.zero_grad()
    la = m(b1['xs'], b1['ys'], b1['x_lens'], b1['y_lens'])
    gen_a = native_ops._arena['gen']
    lb = m(b2['xs'], b2['ys'], b2['x_lens'], b2['y_lens'])
    assert native_ops._arena['gen'] == gen_a + 1
    la.backward()
    torch.cuda.synchronize()
    ga = m._flat_grad.clone()
    m.zero_grad()
    lb.backward()
    torch.cuda.synchronize()
    gb = m._flat_grad.clone()
    assert la.item() == ref[0][0] and lb.item() == ref[1][0]
    assert torch.equal(ga, ref[0][1]), int((ga != ref[0][1]).sum())
    assert torch.equal(gb, ref[1][1]), int((gb != ref[1][1]).sum())


@pytest.mark.gpu
def test_arena_hands_out_only_cleared_slots(cuda_dev, bf16_mode):
    """A generation that reuses a longer buffer of an earlier, larger arena
    clears only its own slots: nothing past them is handed out (a layer op
    called outside a model would otherwise skip its memset on a workspace that
    still holds an earlier launch's granules)."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops
    native_ops.rec_arena_begin(cuda_dev, 32, 512, 10)
    big = native_ops._arena['buf']
    big.fill_(0xff)
    native_ops.rec_arena_begin(cuda_dev, 16, 256, 2)
    assert native_ops._arena['buf'] is big
    nb = N.query('asr_lstm_workspace_bytes', 16, 256, native_ops.BF16, 0)
    zb = int(N.query('asr_lstm_ws_zero_bytes', 16, 256))
    taken = []
    while True:
        res = native_ops._arena_take(nb, cuda_dev, zb)
        if res is None:
            break
        taken.append(res)
        assert len(taken) <= 2
    assert len(taken) == 2
    for t, gen in taken:
        assert gen == native_ops._arena['gen']
        assert int(t[:zb].max()) == 0


_BS = (1, 4, 15, 16, 17, 32, 33, 48, 64)
_HS = (64, 128, 256, 320, 384, 512)


@pytest.mark.gpu
def test_arena_slot_granted_only_where_its_zeroed_prefix_suffices(cuda_dev):
    """rec_arena_begin clears asr_lstm_ws_zero_bytes(B0, H0) leading bytes of
    each slot; the recurrence's row grouping makes neither that nor the slot
    size monotone in B.  For every arena shape / dtype and every launch shape
    / dtype / pass whose workspace fits the slot: the launch is granted the
    slot only if the prefix it would clear itself is no longer than the
    arena's (it is told `prezeroed` and skips its memset).  The arena's own
    shape is always granted (the model's path).  (The size queries ask the
    device for its CU count, hence a GPU test; no kernel but the fills runs.)"""
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    dts = (('bf16', ops.BF16), ('fp32', ops.F32))
    shapes = [(b, h) for b in _BS for h in _HS]
    zbs = {s: int(N.query('asr_lstm_ws_zero_bytes', *s)) for s in shapes}
    nbs = {(s, cd, k): int(N.query('asr_lstm_workspace_bytes', s[0], s[1], cd, k))
           for s in shapes for _, cd in dts for k in (0, 1, 2)}
    assert min(zbs.values()) > 0 and min(nbs.values()) > 0
    fit = need_refusal = need_refusal_same_dtype = granted = 0
    try:
        for name0, cd0 in dts:
            for s0 in shapes:
                ops.set_compute_dtype(name0)
                ops.rec_arena_begin(cuda_dev, s0[0], s0[1], 1)
                slot = ops._arena['slot']
                assert slot >= max(nbs[(s0, cd0, k)] for k in (0, 1, 2))
                for name1, cd1 in dts:
                    ops.set_compute_dtype(name1)
                    for s1 in shapes:
                        for k in (0, 1, 2):
                            nb = nbs[(s1, cd1, k)]
                            if nb > slot:
                                continue
                            fit += 1
                            ops._arena['off'] = 0          # the one slot, again
                            res = ops._arena_take(nb, cuda_dev, zbs[s1])
                            granted += res is not None
                            if zbs[s1] > zbs[s0]:
                                need_refusal += 1
                                need_refusal_same_dtype += cd1 == cd0
                                assert res is None, (name0, s0, name1, s1, k, nb, slot,
                                                     zbs[s1], zbs[s0])
                            if s1 == s0 and cd1 == cd0:
                                assert res is not None, (name0, s0, k)
    finally:
        ops.set_compute_dtype('fp32')
    print('\narena slots: %d (arena, launch) pairs fit; %d of them need a longer zeroed prefix '
          'than the arena cleared and had to be refused (%d in the arena\'s own compute dtype); '
          '%d granted' % (fit, need_refusal, need_refusal_same_dtype, granted))


def _layer_case(Bs, Ts, Hs, Ds, seed):
    rng = np.random.RandomState(seed)
    lens = np.sort(rng.randint(Ts // 2, Ts + 1, Bs))[::-1].astype(np.int32)
    lens[0] = Ts
    x = (rng.randn(Bs, Ts, Ds) * 0.5).astype(np.float32)
    dy = rng.randn(Bs, Ts, 2 * Hs).astype(np.float32)
    for b in range(Bs):
        x[b, lens[b]:] = 0
        dy[b, lens[b]:] = 0
    g = torch.Generator().manual_seed(seed + 1)
    w_ih = torch.rand(8 * Hs, Ds, generator=g) * 0.2 - 0.1
    w_hh = (torch.rand(8 * Hs, Hs, generator=g) * 2 - 1) * 0.03      # contracting
    b_ih = torch.rand(8 * Hs, generator=g) * 0.2 - 0.1
    b_hh = torch.rand(8 * Hs, generator=g) * 0.2 - 0.1
    return lens, torch.from_numpy(x), w_ih, w_hh, b_ih, b_hh, torch.from_numpy(dy)


_ORACLE = {}


def _layer_oracle(Bs, Ts, Hs, Ds):
    """(case, float64 BPTT y, dx, dW_ih, dW_hh, db) of both directions, once per shape."""
    key = (Bs, Ts, Hs, Ds)
    if key not in _ORACLE:
        from oracle import asr_ref
        case = _layer_case(Bs, Ts, Hs, Ds, seed=Bs + Hs)
        lens, x, w_ih, w_hh, b_ih, b_hh, dy = case
        d = torch.float64
        o = [asr_ref.lstm_direction_bptt(x.to(d), lens, w_ih[sl].to(d), w_hh[sl].to(d),
                                         b_ih[sl].to(d), b_hh[sl].to(d), r, dy[:, :, hs].to(d))
             for r, sl, hs in ((False, slice(0, 4 * Hs), slice(0, Hs)),
                               (True, slice(4 * Hs, 8 * Hs), slice(Hs, 2 * Hs)))]
        _ORACLE[key] = (case, [torch.cat([o[0][0], o[1][0]], dim=2), o[0][1] + o[1][1]] +
                        [torch.cat([o[0][i], o[1][i]]) for i in (2, 3, 4)])
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize('prec,bound', [('bf16', 2e-2), ('fp32', 1e-4)])
@pytest.mark.parametrize('B0,B1', [(16, 32), (32, 16)])
def test_layer_of_another_shape_inside_a_model_generation(B0, B1, prec, bound, cuda_dev):
    """An encoder step at (B0, 256), then -- in one arena generation with spare
    slots, the buffer holding 0xff past every cleared prefix -- a standalone
    BLSTM layer at (B1, 256).  (16 -> 32: the layer would clear a longer
    prefix than the arena did and must get a private workspace; 32 -> 16: it
    may take a slot.)  Either way its outputs and gradients match the float64
    BPTT oracle (max error / max |reference|: bf16 2e-2, fp32 1e-4) and no
    recurrence gives up.  The encoder step itself takes every workspace from
    the arena."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    H, L, Ts, Ds = 256, 2, 48, 64
    (lens, x, w_ih, w_hh, b_ih, b_hh, dy), ref = _layer_oracle(B1, Ts, H, Ds)
    ops.set_compute_dtype(prec)
    try:
        m = _build(_kw(H, L))
        m.set_cuda()
        ops.recurrence_status(cuda_dev)                      # clear
        ops.ARENA_STATS.update(granted=0, private=0)
        loss, _ = _loss_grad(m, _batch(B=B0, T=96, seed=3))
        assert np.isfinite(loss)
        # every BLSTM forward (and every tagged-granule backward) from the arena
        assert ops.ARENA_STATS['private'] == 0 and ops.ARENA_STATS['granted'] >= L, \
            ops.ARENA_STATS
        ops._arena['buf'].fill_(0xff)
        ops.rec_arena_begin(cuda_dev, B0, H, 4)
        zb0, zb1 = (int(N.query('asr_lstm_ws_zero_bytes', b, H)) for b in (B0, B1))
        ops.ARENA_STATS.update(granted=0, private=0)
        ws = [t.clone().to(cuda_dev).requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh)]
        for w in ws:
            w.grad = torch.zeros_like(w)
        xd = x.to(cuda_dev).requires_grad_(True)
        y = ops.blstm_layer(xd, torch.from_numpy(lens).to(cuda_dev), Ts, *ws)
        y.backward(dy.to(cuda_dev))
        torch.cuda.synchronize()
        st = ops.recurrence_status(cuda_dev)
        assert int(st.max()) == 0, st.tolist()
        stats = dict(ops.ARENA_STATS)
        got = [t.double().cpu() for t in (y.detach(), xd.grad, ws[0].grad, ws[1].grad,
                                          ws[2].grad, ws[3].grad)]
    finally:
        ops.set_compute_dtype('fp32')
    assert stats['granted'] + stats['private'] >= 1, stats
    if zb1 > zb0:
        assert stats['granted'] == 0, (stats, zb1, zb0)
    names = ['y', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']
    errs = {n: float((g - r).abs().max() / r.abs().max())
            for n, g, r in zip(names, got, ref + [ref[4]])}
    print('\n%s arena (%d, %d) zero %d B -> layer (%d, %d) zero %d B: %s; max error / max|ref| %s'
          % (prec, B0, H, zb0, B1, H, zb1, stats, ', '.join('%s %.2e' % kv for kv in errs.items())))
    for n, e in errs.items():
        assert e <= bound, (prec, n, e, bound)
