"""The tagged-granule recurrence's launch settings travel with the call
(asr_lstm_opts_t, include/asr_hip.h): direct C-API calls of asr_lstm_forward_xh
and asr_lstm_backward_dgbf_h at B = 9, H = 64, T = 4, Din = 16 in bf16 -- two
row groups, ragged lens, the last utterance one frame long.

  a setting dies with its call: NULL opts, 32 units per work-group, NULL opts
      again -- the third result is the first bit for bit;
  a dirty workspace is cleared unless the call says it is zero already;
  a ws_prezeroed given to a call that takes the per-step kernels is not seen by
      the next call;
  the progress report and the dy flags arrive by the struct;
  a value out of range is ASR_ERR_ARG.

Every test first asserts asr_lstm_last_path == [3, 1].  The 32-unit result is
held to the float64 layer reference tests/rnn_layer_ref.py: db_ih and db_hh as
written, dx = dG W_ih and dW_ih = dG^T X formed on the host in float64 from the
bf16 dG the call wrote, each within rnn_layer_ref.MARGIN x the constant that
tests/golden/bwd_publish_constants.json records for the single-layer case of
this B, H and dtype (pub_b9h64_t2, packed activations)."""
import ctypes
import json
import os

import pytest
import torch

import rnn_layer_ref as R

pytestmark = pytest.mark.gpu

CONSTANTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'bwd_publish_constants.json')
CASE = 'opts_b9h64_t4'
B, H, T, DIN = 9, 64, 4, 16
RECORDED = 'pub_b9h64_t2'
PERSTEP = (5, 6, 2)         # B, H, T of rnn_layer_ref's l_b5h6: the per-step kernels
ASR_ERR_ARG = -1


@pytest.fixture(scope='module', autouse=True)
def _case():
    """rnn_layer_ref's case table holds this module's shape while its tests run."""
    R.CASES[CASE] = R._c('lstm', B, H, T, Din=DIN)
    try:
        yield
    finally:
        R.CASES.pop(CASE, None)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in R.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


def _N():
    from pytorch_end2end_speech_recognition_amd import _native as N
    return N


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _last_path():
    out = (ctypes.c_int * 2)()
    _N().call('asr_lstm_last_path', ctypes.cast(out, ctypes.c_void_p))
    return [int(v) for v in out]


def _opts(**fields):
    return ctypes.byref(_N().LstmOpts(**fields)) if fields else None


def _workspace(dev, kind, dirty):
    N = _N()
    nb = int(N.query('asr_lstm_workspace_bytes', B, H, N.ASR_DT_BF16, kind))
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    if dirty:
        ws.fill_(0xFF)
    return ws, nb


def _inputs(dev):
    inp = R.case_inputs(CASE)
    t = {k: inp[k].to(dev) for k in ('w_hh', 'b_ih', 'b_hh', 'dy')}
    t['x'] = inp['x'].to(dev).to(torch.bfloat16).view(B * T, DIN)
    t['w_ih'] = inp['w_ih'].to(dev).to(torch.bfloat16)
    t['lens'] = torch.from_numpy(inp['lens']).to(dev)
    t['whh_r'] = ctypes.c_void_p(t['w_hh'].data_ptr() + 4 * H * H * 4)
    return t


def _forward(dev, t, dirty=False, **fields):
    """asr_lstm_forward_xh: (rc, dict(act_h, y, cst, ybf))."""
    N = _N()
    o = dict(act_h=torch.zeros(B, T, 2, H, 4, dtype=torch.float16, device=dev),
             y=torch.zeros(B, T, 2 * H, device=dev), cst=torch.zeros(B, T, 2 * H, device=dev),
             ybf=torch.zeros(B, T, 2 * H, dtype=torch.bfloat16, device=dev))
    ws, nb = _workspace(dev, 0, dirty)
    rc = N.query('asr_lstm_forward_xh', N.ptr(t['x']), DIN, N.ptr(t['w_ih']), N.ptr(t['b_ih']),
                 N.ptr(t['b_hh']), N.ptr(t['w_hh']), t['whh_r'], N.ptr(t['lens']), B, T, H,
                 N.ptr(o['act_h']), N.ptr(o['y']), N.ptr(o['cst']), N.ptr(o['ybf']), N.ptr(ws), nb,
                 N.stream_handle(dev), _opts(**fields))
    torch.cuda.synchronize()
    return rc, o


def _backward(dev, t, fwd, dirty=False, **fields):
    """asr_lstm_backward_dgbf_h on the forward's activations:
    (rc, dict(dg, db_ih, db_hh)); the bias gradients accumulate onto zeros."""
    N = _N()
    o = dict(dg=torch.zeros(B, T, 8 * H, dtype=torch.bfloat16, device=dev),
             db_ih=torch.zeros(8 * H, device=dev), db_hh=torch.zeros(8 * H, device=dev))
    ws, nb = _workspace(dev, 2, dirty)
    rc = N.query('asr_lstm_backward_dgbf_h', N.ptr(t['dy']), N.ptr(t['w_hh']), t['whh_r'],
                 N.ASR_DT_F32, N.ptr(t['lens']), B, T, H, N.ASR_DT_BF16, N.ptr(fwd['act_h']),
                 N.ptr(fwd['cst']), N.ptr(o['dg']), N.ptr(o['db_ih']), N.ptr(o['db_hh']), N.ptr(ws),
                 nb, N.stream_handle(dev), _opts(**fields))
    torch.cuda.synchronize()
    return rc, o


def _base(dev):
    """(inputs, forward outputs, backward outputs) with NULL opts and clean
    private workspaces: how every test starts, so none passes on another path."""
    _ops().recurrence_status(dev)
    t = _inputs(dev)
    rc, fwd = _forward(dev, t)
    assert rc == 0, rc
    rc, bwd = _backward(dev, t, fwd)
    assert rc == 0, rc
    assert _last_path() == [3, 1], _last_path()
    assert int(_ops().recurrence_status(dev).max()) == 0
    return t, fwd, bwd


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_settings_die_with_their_call(cuda_dev):
    N = _N()
    t, fwd, first = _base(cuda_dev)
    grid16, grid32 = (N.query('asr_lstm_backward_grid', B, H, xu) for xu in (16, 32))
    assert grid16 == 2 * 2 * (H // 16) and 2 * grid32 == grid16, (grid16, grid32)
    rc, second = _backward(cuda_dev, t, fwd, bwd_units=32)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    rc, third = _backward(cuda_dev, t, fwd)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    assert int(_ops().recurrence_status(cuda_dev).max()) == 0
    _same(first, third)

    with open(CONSTANTS_JSON) as f:
        rec = json.load(f)[RECORDED]
    bound = {k: R.MARGIN * max(rec['f32'][k], rec['bf16p'][k]) for k in rec['f32']}
    ref, inp = R.reference(CASE), R.case_inputs(CASE)
    dg = second['dg'].double().cpu()
    got = dict(db_ih=second['db_ih'].double().cpu(), db_hh=second['db_hh'].double().cpu(),
               dx=dg @ inp['w_ih'].double(),
               dW_ih=torch.einsum('btg,btd->gd', dg, inp['x'].double()))
    line, bad = [], []
    for k, g in got.items():
        ratio = R.nerr(g.numpy(), ref[k]) / bound[k]
        line.append('%s %.3f' % (k, ratio))
        if not ratio <= 1.0:
            bad.append((k, ratio))
    print('xu32 err/bound:', ' '.join(line))
    assert not bad, bad
    assert torch.equal(second['db_ih'], second['db_hh'])


def test_dirty_workspace_is_cleared_unless_prezeroed(cuda_dev):
    t, fwd0, bwd0 = _base(cuda_dev)
    rc, fwd = _forward(cuda_dev, t, dirty=True)
    assert rc == 0, rc
    rc, bwd = _backward(cuda_dev, t, fwd, dirty=True)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    assert int(_ops().recurrence_status(cuda_dev).max()) == 0
    rc, fwd_z = _forward(cuda_dev, t, ws_prezeroed=1)          # (a torch.zeros workspace)
    assert rc == 0, rc
    rc, bwd_z = _backward(cuda_dev, t, fwd_z, ws_prezeroed=1)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    assert int(_ops().recurrence_status(cuda_dev).max()) == 0
    _same(fwd, fwd_z)
    _same(bwd, bwd_z)
    _same(fwd, fwd0)
    _same(bwd, bwd0)


def test_prezeroed_on_another_path_does_not_reach_the_next_call(cuda_dev):
    N = _N()
    t, fwd0, _ = _base(cuda_dev)
    b, h, n = PERSTEP
    gen = torch.Generator().manual_seed(5)
    gx = torch.randn(b, n, 8 * h, generator=gen).to(cuda_dev)
    whh = (torch.rand(8 * h, h, generator=gen) * 0.2 - 0.1).to(cuda_dev)
    lens = torch.from_numpy(R.make_lens(b, n)).to(cuda_dev)
    y, cst = (torch.zeros(b, n, 2 * h, device=cuda_dev) for _ in range(2))
    nb = int(N.query('asr_lstm_workspace_bytes', b, h, N.ASR_DT_BF16, 0))
    ws = torch.zeros(nb, dtype=torch.uint8, device=cuda_dev)
    N.call('asr_lstm_forward', N.ptr(gx), N.ptr(whh), ctypes.c_void_p(whh.data_ptr() + 4 * h * h * 4),
           N.ASR_DT_F32, N.ptr(lens), b, n, h, N.ASR_DT_BF16, N.ptr(y), N.ptr(cst), None, N.ptr(ws),
           nb, N.stream_handle(cuda_dev), _opts(ws_prezeroed=1))
    torch.cuda.synchronize()
    assert _last_path()[0] == 0, _last_path()
    rc, fwd = _forward(cuda_dev, t, dirty=True)
    assert rc == 0 and _last_path()[0] == 3, (rc, _last_path())
    assert int(_ops().recurrence_status(cuda_dev).max()) == 0
    _same(fwd, fwd0)


def test_progress_and_dy_flags_by_struct(cuda_dev):
    N = _N()
    t, fwd, first = _base(cuda_dev)
    counter = torch.zeros(1, dtype=torch.int64, device=cuda_dev)
    rc, bwd = _backward(cuda_dev, t, fwd, progress=counter.data_ptr(), progress_q1=1,
                        progress_q2=2)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    arrivals = int(N.query('asr_lstm_bwd_progress_arrivals', B, H, 0))
    assert arrivals > 0 and int(counter.item()) == 2 * arrivals, (counter.item(), arrivals)
    _same(bwd, first)
    # every flag already holds the epoch when the launch is enqueued: no wait
    epoch = 7
    flags = torch.full((16,), epoch, dtype=torch.int32, device=cuda_dev)
    torch.cuda.synchronize()
    rc, bwd = _backward(cuda_dev, t, fwd, dy_flags=flags.data_ptr(), dy_c0=1, dy_epoch=epoch)
    assert rc == 0 and _last_path() == [3, 1], (rc, _last_path())
    assert int(_ops().recurrence_status(cuda_dev).max()) == 0
    _same(bwd, first)


@pytest.mark.parametrize('fields', [dict(bwd_units=24), dict(bwd_pin_kb=50),
                                    dict(progress_q1=-1, progress_q2=-1),
                                    dict(progress_q1=2, progress_q2=1)],
                         ids=['units24', 'pin50', 'q1neg', 'q2_not_above_q1'])
def test_argument_checks(fields, cuda_dev):
    t, fwd, first = _base(cuda_dev)
    if 'progress_q1' in fields:
        counter = torch.zeros(1, dtype=torch.int64, device=cuda_dev)
        fields = dict(fields, progress=counter.data_ptr())
    rc, bwd = _backward(cuda_dev, t, fwd, **fields)
    assert rc == ASR_ERR_ARG, rc
    # returned before any launch: nothing written, nothing counted
    assert not bwd['dg'].any() and not bwd['db_ih'].any() and not bwd['db_hh'].any()
    if 'progress' in fields:
        assert int(counter.item()) == 0
