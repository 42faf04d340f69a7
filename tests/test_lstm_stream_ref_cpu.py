"""tests/lstm_stream_ref.py (the float64 reference tests/test_lstm_stream_gpu.py
holds asr_lstm_stream_forward to) is right: on float64 every chunk schedule of a
case gives the whole-utterance y and final state to 1e-12; from a zero state
its y equals the whole-utterance layer reference tests/lstm_uni_ref.py (which
differs only in zeroing the state at padded frames); a row without frames in a
chunk keeps its state bit for bit; garbage at padded frames changes nothing;
and the recorded error constants are reproduced."""
import numpy as np
import pytest
import torch

import lstm_stream_ref as S
import lstm_uni_ref as U

F64 = torch.float64


@pytest.mark.parametrize('case', sorted(S.CASES))
def test_every_schedule_gives_the_whole_utterance_result_on_float64(case):
    ref = S.reference(case)
    totals = S.case_inputs(case)['totals']
    for b, n in enumerate(totals):
        assert not ref['y'][b, n:].any()
        assert np.abs(ref['y'][b, :n]).min() > 0
    for name in S.SCHEDULES:
        got = S.evaluate(case, schedule=name)
        for k in S.OUT_KEYS:
            assert got[k].shape == ref[k].shape
            np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-12, err_msg=name + ' ' + k)


def test_from_a_zero_state_y_equals_the_whole_utterance_layer_reference():
    g = torch.Generator().manual_seed(11)
    B, T, H, Din = 4, 7, 5, 3
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    w_ih, w_hh, b_ih, b_hh = 0.4 * r(4 * H, Din), 0.4 * r(4 * H, H), 0.4 * r(4 * H), 0.4 * r(4 * H)
    x = r(B, T, Din)
    lens = np.array([T, T, 4, 1], np.int32)
    want = U.layer(x, lens, T, None, 1, 0, False, w_ih, w_hh, b_ih, b_hh, None)['y']
    gx = x @ w_ih.t() + (b_ih + b_hh)
    zero = torch.zeros(B, H, dtype=F64)
    for sizes in S.SCHEDULES.values():
        y, h, c = S.run_schedule(gx, w_hh, lens, zero, zero, sizes)
        np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=0, atol=1e-12)
        for b, n in enumerate(lens):          # the frozen state: that of the last valid frame
            np.testing.assert_allclose(h[b].numpy(), want[b, n - 1].numpy(), rtol=0, atol=1e-12)
    assert (lens == T).sum() >= 2 and (lens < T).any()


def test_a_row_without_frames_keeps_its_state_and_garbage_does_not_enter():
    inp = S.case_inputs('h20_b3')
    assert list(inp['totals']) == [7, 4, 1]
    gx, w = inp['gx'].double(), inp['w_hh'].double()
    h0, c0 = inp['h0'].double(), inp['c0'].double()
    lens = np.array([2, 0, 1], np.int32)
    y, h, c = S.run_chunk(gx[:, :2], w, lens, h0, c0)
    assert torch.equal(h[1], h0[1]) and torch.equal(c[1], c0[1])
    assert not torch.equal(h[0], h0[0]) and not torch.equal(c[2], c0[2])
    assert not y[1].any() and not y[2, 1:].any() and bool(y[2, 0].all())
    g2 = gx.clone()
    for b, n in enumerate(inp['totals']):
        g2[b, n:] = -7e2
    a = S.run_schedule(gx, w, inp['totals'], h0, c0, [3, 4])
    b_ = S.run_schedule(g2, w, inp['totals'], h0, c0, [3, 4])
    for p, q in zip(a, b_):
        assert torch.equal(p, q)


def test_chunk_lens_of_the_schedules():
    cl = S.chunk_lens([7, 4, 1], [2, 0, 5])
    assert [(s, n, l.tolist()) for s, n, l in cl] == [(0, 2, [2, 2, 1]), (2, 0, [0, 0, 0]),
                                                      (2, 5, [5, 2, 0])]
    for sizes in S.SCHEDULES.values():
        assert sum(sizes) == S.T
        assert sum(l for _, _, l in S.chunk_lens([7, 4, 1], sizes)).tolist() == [7, 4, 1]


def test_bf16_emulation_rounds_only_h_and_w_hh():
    """One frame from a state and weights that are bf16 values already: the
    emulation is the float32 evaluation."""
    inp = S.case_inputs('h24_b1')
    rb = lambda a: a.to(torch.bfloat16).float()      # noqa: E731
    args = (inp['gx'][:, :1], rb(inp['w_hh']), [1], rb(inp['h0']), inp['c0'])
    for p, q in zip(S.run_chunk(*args), S.run_chunk(*args, bf16=True)):
        assert torch.equal(p, q)
    args = (inp['gx'][:, :2], inp['w_hh'], [2], inp['h0'], inp['c0'])
    assert not torch.equal(S.run_chunk(*args)[0], S.run_chunk(*args, bf16=True)[0])


@pytest.mark.parametrize('case', sorted(S.CASES))
def test_recorded_constants_are_reproduced_and_f32_has_room(case):
    """As tests/test_lstm_uni_ref_cpu.py holds its table: a bf16 constant to
    25 %, a float32 constant (set by the CPU's summation order) within 4 x both
    ways, and the float32 evaluation within a quarter of the fp32 bound."""
    ref = S.reference(case)
    got = S.measure_constants(case)
    cf, cb = S.case_constants(case)
    assert set(ref) == set(cf) == set(cb) == set(S.OUT_KEYS)
    print(case, ' '.join('%s %.1e/%.1e' % (k, cf[k], cb[k]) for k in sorted(cf)))
    for k in S.OUT_KEYS:
        assert np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, k
        assert S.CONST_FLOOR <= cf[k] < 1e-4 and S.CONST_FLOOR <= cb[k] < 0.1, (k, cf[k], cb[k])
        assert cf[k] / 4 <= got['f32'][k] <= 4 * cf[k], (k, got['f32'][k], cf[k])
        assert abs(got['bf16'][k] - cb[k]) <= 0.25 * cb[k], (k, got['bf16'][k], cb[k])
        assert got['f32'][k] <= 0.25 * S.MARGIN * cf[k]


def test_case_table_covers_what_the_kernel_branches_on():
    C = S.CASES
    assert {c['H'] for c in C.values()} == {4, 20, 24}
    assert {1, 3, 31, 33} == {c['B'] for c in C.values()}
    assert list(S.case_inputs('h20_b3')['totals']) == [7, 4, 1]
    assert sorted(S.SCHEDULES.values()) == sorted([[7], [1] * 7, [3, 4], [2, 0, 5]])
    assert all(S.case_inputs(k)['h0'].abs().min() > 0 for k in C)
