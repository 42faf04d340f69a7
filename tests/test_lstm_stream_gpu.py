"""asr_lstm_stream_forward (csrc/lstm_stream.hip, the stateful recurrence of
streaming inference) at the C ABI, against the float64 reference
tests/lstm_stream_ref.py, in both compute types, on lstm_stream_ref.CASES: H =
4 (one unit tile), 20 (scalar tail loads) and 24 (vector loads off the 16-unit
tile); B = 1, 31 and 33 (one short of / one past the row tile) and 3 with the
per-row totals [7, 4, 1]; T = 7 fed as [7], [1] * 7, [3, 4] and [2, 0, 5], so
rows finish mid-chunk and then sit at lens = 0; a non-zero random initial
state; 100 N(0, 1) garbage in gx at padded frames.

Every case: on the same gx, each schedule's concatenated y and final (h, c)
equal the single-chunk call's bit for bit; y is exactly 0 at padded frames;
and per tensor max |got - f64| / max |f64| <= MARGIN x the recorded constant
(the f32 one in fp32 mode, the larger of the f32 and the bf16 one in bf16
mode).  err/bound is printed per tensor.  Also: from a zero state a single
chunk gives the bits of asr_lstm_uni_forward, two identical calls agree bit
for bit, rows with lens == 0 return their state bit-identical, c_out may be
c_in, a bf16 W_hh gives the bits of the converted f32 one, aliased h_in / h_out
are ASR_ERR_ARG and H = 1032 is ASR_ERR_UNSUPPORTED with nothing written."""
import numpy as np
import pytest
import torch

import lstm_stream_ref as S
from test_rnn_layer_gpu import _compare

pytestmark = pytest.mark.gpu

ASR_ERR_ARG = -1
CD = {'fp32': 0, 'bf16': 1}


def _call(dev, gx, whh, lens, cd, h_in, c_in, h_out=None, c_out=None, y=None):
    """(rc, y, h_out, c_out) of one asr_lstm_stream_forward call (device tensors)."""
    from pytorch_end2end_speech_recognition_amd import _native as N
    B, Tc, H4 = gx.shape
    H = H4 // 4
    h_out = torch.empty_like(h_in) if h_out is None else h_out
    c_out = torch.empty_like(c_in) if c_out is None else c_out
    y = torch.empty(B, Tc, H, device=dev) if y is None else y
    w_dt = N.ASR_DT_BF16 if whh.dtype == torch.bfloat16 else N.ASR_DT_F32
    nb = max(int(N.query('asr_lstm_stream_workspace_bytes', B, H, cd)), 256)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    lens_d = torch.as_tensor(np.asarray(lens, np.int32)).to(dev)
    rc = N.query('asr_lstm_stream_forward', N.ptr(gx), N.ptr(whh), w_dt, N.ptr(lens_d), B, Tc, H,
                 cd, N.ptr(h_in), N.ptr(c_in), N.ptr(h_out), N.ptr(c_out), N.ptr(y), N.ptr(ws), nb,
                 N.stream_handle(dev))
    torch.cuda.synchronize()
    return rc, y, h_out, c_out


def _feed(dev, case, cd, sizes, whh=None, alias_c=False):
    """A case fed as chunks of `sizes`: (y [B, T, H], h, c) on the device."""
    inp = S.case_inputs(case)
    gx = inp['gx'].to(dev)
    whh = inp['w_hh'].to(dev) if whh is None else whh
    h, c = inp['h0'].to(dev), inp['c0'].to(dev)
    ys = []
    for s, n, lens in S.chunk_lens(inp['totals'], sizes):
        # a size 0: a chunk of one padded frame in which no row has a frame
        g = gx[:, s:s + n].contiguous() if n else torch.full_like(gx[:, :1], 3.0)
        rc, y, h, c = _call(dev, g, whh, lens, cd, h, c, c_out=c if alias_c else None)
        assert rc == 0
        if n:
            ys.append(y)
    return torch.cat(ys, dim=1), h, c


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', sorted(S.CASES))
def test_chunked_equals_whole_bitwise_and_matches_f64(case, precision, cuda_dev):
    cd = CD[precision]
    ref = S.reference(case)
    totals = S.case_inputs(case)['totals']
    whole = _feed(cuda_dev, case, cd, S.SCHEDULES['whole'])
    got = dict(zip(S.OUT_KEYS, whole))
    bad = _compare(case + '-' + precision, got, ref, S.bounds(case, precision))
    assert not bad, (case, precision, bad)
    yh = whole[0].cpu().numpy()
    for b, n in enumerate(totals):
        assert not yh[b, n:].any(), ('y at padded frames of row', b)
    for name, sizes in S.SCHEDULES.items():
        other = _feed(cuda_dev, case, cd, sizes)
        for k, a, b in zip(S.OUT_KEYS, whole, other):
            assert torch.equal(a, b), (name, k, 'differs from the single-chunk call')


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', ['h20_b3', 'h24_b33'])
def test_zero_state_single_chunk_equals_the_offline_recurrence_bitwise(case, precision, cuda_dev):
    """From h = c = 0 and in one chunk, asr_lstm_stream_forward gives the bits
    asr_lstm_uni_forward writes on a copy of the same gx: y everywhere, and
    h_out[b] is y[b, lens[b] - 1].  (The offline step skips the recurrent
    product at t = 0; the stream's product of zeros sums to the same zeros.)"""
    from pytorch_end2end_speech_recognition_amd import _native as N
    dev, cd = cuda_dev, CD[precision]
    inp = S.case_inputs(case)
    gx, whh, lens = inp['gx'].to(dev), inp['w_hh'].to(dev), inp['totals']
    B, T, H = gx.shape[0], gx.shape[1], whh.shape[1]
    zero = torch.zeros(B, H, device=dev)
    rc, y, h, c = _call(dev, gx.clone(), whh, lens, cd, zero, zero.clone())
    assert rc == 0
    act = gx.clone()                           # the offline forward overwrites its gx
    y_off, cst = torch.empty(B, T, H, device=dev), torch.empty(B, T, H, device=dev)
    nb = max(int(N.query('asr_lstm_uni_workspace_bytes', B, H, cd, 0)), 256)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    lens_d = torch.as_tensor(np.asarray(lens, np.int32)).to(dev)
    rc = N.query('asr_lstm_uni_forward', N.ptr(act), N.ptr(whh), N.ASR_DT_F32, N.ptr(lens_d), B, T,
                 H, cd, N.ptr(y_off), N.ptr(cst), None, N.ptr(ws), nb, N.stream_handle(dev))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(y, y_off)
    for b, n in enumerate(lens):
        assert torch.equal(h[b], y_off[b, n - 1]), ('h_out of row', b)
        assert torch.equal(c[b], cst[b, n - 1]), ('c_out of row', b)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_two_identical_calls_agree_bit_for_bit(precision, cuda_dev):
    a, b = (_feed(cuda_dev, 'h24_b33', CD[precision], [3, 4]) for _ in range(2))
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_rows_without_frames_return_their_state_bit_identical(precision, cuda_dev):
    inp = S.case_inputs('h20_b3')
    dev = cuda_dev
    gx, whh = inp['gx'][:, :2].contiguous().to(dev), inp['w_hh'].to(dev)
    h0, c0 = inp['h0'].to(dev), inp['c0'].to(dev)
    rc, y, h, c = _call(dev, gx, whh, [2, 0, 1], CD[precision], h0, c0)
    assert rc == 0
    assert torch.equal(h[1], h0[1]) and torch.equal(c[1], c0[1])
    assert not torch.equal(h[0], h0[0]) and not torch.equal(c[2], c0[2])
    assert not y[1].any() and not y[2, 1:].any() and bool(y[2, 0].all())


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_c_out_may_be_c_in(precision, cuda_dev):
    a = _feed(cuda_dev, 'h24_b33', CD[precision], [2, 0, 5])
    b = _feed(cuda_dev, 'h24_b33', CD[precision], [2, 0, 5], alias_c=True)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize('case', ['h20_b3', 'h24_b33'])
def test_a_bf16_w_hh_gives_the_bits_of_the_converted_f32_one(case, cuda_dev):
    whh = S.case_inputs(case)['w_hh'].to(torch.bfloat16).to(cuda_dev)
    a = _feed(cuda_dev, case, 1, [3, 4])
    b = _feed(cuda_dev, case, 1, [3, 4], whh=whh)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_aliased_h_buffers_are_refused(cuda_dev):
    from pytorch_end2end_speech_recognition_amd import _native as N
    inp = S.case_inputs('h20_b3')
    dev = cuda_dev
    gx, whh = inp['gx'].to(dev), inp['w_hh'].to(dev)
    h0, c0 = inp['h0'].to(dev), inp['c0'].to(dev)
    keep = h0.clone()
    y = torch.full((3, S.T, 20), 7.0, device=dev)
    rc, y, h, c = _call(dev, gx, whh, [7, 4, 1], 0, h0, c0, h_out=h0, y=y)
    assert rc == ASR_ERR_ARG and b'alias' in N.lib().asr_last_error()
    assert torch.equal(h0, keep) and bool((y == 7.0).all())       # nothing was launched


def test_other_overlaps_of_an_output_are_refused(cuda_dev):
    """y, h_out, c_out against each other and against gx, h_in, c_in (only
    c_out == c_in is allowed): ASR_ERR_ARG, nothing launched."""
    inp = S.case_inputs('h20_b3')
    dev = cuda_dev
    whh = inp['w_hh'].to(dev)
    B, H = 3, 20

    def fresh():
        return dict(gx=inp['gx'].to(dev), h_in=inp['h0'].to(dev), c_in=inp['c0'].to(dev),
                    h_out=torch.full((B, H), 7.0, device=dev),
                    c_out=torch.full((B, H), 7.0, device=dev),
                    y=torch.full((B, S.T, H), 7.0, device=dev))

    def alias(t, like):          # a view of t's memory with like's shape
        return t.reshape(-1)[:like.numel()].view(like.shape)

    for out, other in (('h_out', 'c_out'), ('c_out', 'y'), ('h_out', 'y'), ('h_out', 'c_in'),
                       ('c_out', 'h_in'), ('c_out', 'gx'), ('h_out', 'gx')):
        a = fresh()
        before = {k: v.clone() for k, v in a.items()}
        a[out] = alias(a[other], a[out])
        rc, _, _, _ = _call(dev, a['gx'], whh, [7, 4, 1], 0, a['h_in'], a['c_in'], h_out=a['h_out'],
                            c_out=a['c_out'], y=a['y'])
        assert rc == ASR_ERR_ARG, (out, other, rc)
        for k in before:
            if k != out:
                assert torch.equal(a[k], before[k]), (out, other, k)
    # y against gx / the input state (y is the larger: alias the other way round)
    for other in ('gx', 'h_in', 'c_in'):
        a = fresh()
        big = torch.full((B, S.T, 4 * H), 7.0, device=dev)
        y = alias(big, a['y'])
        a[other] = alias(big, a[other]) if other != 'gx' else big
        rc, _, _, _ = _call(dev, a['gx'], whh, [7, 4, 1], 0, a['h_in'], a['c_in'], h_out=a['h_out'],
                            c_out=a['c_out'], y=y)
        assert rc == ASR_ERR_ARG, (other, rc)
        assert bool((big == 7.0).all())


@pytest.mark.parametrize('cd', [0, 1], ids=['fp32', 'bf16'])
def test_a_shape_outside_the_accepted_set_is_refused_before_any_launch(cd, cuda_dev):
    from pytorch_end2end_speech_recognition_amd import _native as N
    dev = cuda_dev
    B, Tc, H = 3, 2, 1032                      # above the widest accepted H
    assert N.query('asr_lstm_uni_shape_ok', B, Tc, H) == 0
    gx = torch.zeros(B, Tc, 4 * H, device=dev)
    whh = torch.zeros(4 * H, H, device=dev)
    h0, c0 = torch.zeros(B, H, device=dev), torch.zeros(B, H, device=dev)
    sent = [torch.full((B, H), 7.0, device=dev), torch.full((B, H), 7.0, device=dev),
            torch.full((B, Tc, H), 7.0, device=dev)]
    rc, y, h, c = _call(dev, gx, whh, [2, 2, 1], cd, h0, c0, h_out=sent[0], c_out=sent[1],
                        y=sent[2])
    assert rc == N.ASR_ERR_UNSUPPORTED
    assert all(bool((t == 7.0).all()) for t in sent)
