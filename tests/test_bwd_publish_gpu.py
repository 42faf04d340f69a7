"""The backward recurrence's partial-dh publish (csrc/lstm_xg.hip lstm_bwd_xg,
bf16: every MFMA wave owns adjacent M block pairs with permuted rows and stores
a lane's eight consecutive units -- two tagged granules -- as one 16-B store)
against the float64 layer reference tests/rnn_layer_ref.py, at the shapes where
the pairing, the permutation and the tag can go wrong:

  H = 32             one block pair; with 32 units per work-group one producer
  H = 64, 96         4 and 6 blocks: fewer pairs than MFMA waves, an odd pair
                     count, the clamped fragment of the waves without a pair
  H = 160            5 pairs: the waves' second pair slot half filled
  H = 512, T = 3     the flagship's width (16 pairs, 2 or 4 per wave)
  B = 5, 9           rows past B in the last group; a second group
  T = 1, 2, 3        both parity buffers and each tag value on first use
  lens               ragged, the last utterance one frame long
each with 16 and with 32 units per backward work-group, and the f32
instantiation (whose 16-B store was already one consumer load) at one shape.

Every row: a cotangent at every frame, recurrence_status == 0, the
tagged-granule backward ran (asr_lstm_last_path) on the expected grid, and per
tensor max |got - f64| / max |f64| <= rnn_layer_ref.MARGIN (16) x the recorded
constant of the shape (tests/golden/bwd_publish_constants.json, written by
`PYTHONPATH=. python tests/test_bwd_publish_gpu.py --record` with rnn_layer_ref.
measure_constants and reproduced by the CPU test below the way
tests/test_rnn_layer_ref_cpu.py reproduces the layer table).  A two-layer stack
run twice in one process gives the same bits both times: a tag left over from
the first run would be taken for a published granule in the second."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rnn_layer_ref as R

gpu = pytest.mark.gpu

CONSTANTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'bwd_publish_constants.json')
# name: (B, H, T)
SHAPES = {
    'pub_b5h32_t3': (5, 32, 3),
    'pub_b9h64_t2': (9, 64, 2),
    'pub_b5h64_t1': (5, 64, 1),
    'pub_b9h96_t3': (9, 96, 3),
    'pub_b5h160_t3': (5, 160, 3),
    'pub_b9h512_t3': (9, 512, 3),
}
STACK = 'pub_b9h64_t3_stack'
ALL = dict({k: R._c('lstm', *v) for k, v in SHAPES.items()})
ALL[STACK] = R._c('lstm', 9, 64, 3, stack=True)
F32_SHAPE = 'pub_b9h64_t2'
PARAMS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')
GRADS = dict(zip(PARAMS, R.OUT_KEYS[2:]))


@pytest.fixture(scope='module', autouse=True)
def _cases():
    """rnn_layer_ref's case table holds this module's shapes while its tests run."""
    R.CASES.update(ALL)
    try:
        yield
    finally:
        for k in ALL:
            R.CASES.pop(k, None)


def _recorded():
    with open(CONSTANTS_JSON) as f:
        return json.load(f)


def _bounds(case, precision):
    rec = _recorded()[case]
    if precision == 'fp32':
        return {k: R.MARGIN * v for k, v in rec['f32'].items()}
    # bf16 mode takes the fused forward here: packed fp16 gate activations
    return {k: R.MARGIN * max(rec['f32'][k], rec['bf16p'][k]) for k in rec['f32']}


def test_recorded_constants_are_reproduced():
    """As tests/test_rnn_layer_ref_cpu.py holds the layer table: a bf16 constant
    to 25 %, a float32 constant within 4 x both ways."""
    rec = _recorded()
    assert set(rec) == set(ALL)
    for case in sorted(ALL):
        got = R.measure_constants(case)
        for k, cf in rec[case]['f32'].items():
            assert R.CONST_FLOOR <= cf < 1e-4, (case, k, cf)
            assert cf / 4 <= got['f32'][k] <= 4 * cf, (case, k, got['f32'][k], cf)
            cb = rec[case]['bf16p'][k]
            assert R.CONST_FLOOR <= cb < 0.1, (case, k, cb)
            assert abs(got['bf16p'][k] - cb) <= 0.25 * cb, (case, k, got['bf16p'][k], cb)
        for b, n in enumerate(R.case_inputs(case)['lens']):
            assert not R.reference(case)['y'][b, n:].any()
        assert R.case_inputs(case)['lens'][-1] == 1


def _native():
    from pytorch_end2end_speech_recognition_amd import _native as N
    return N


def _last_path():
    out = (ctypes.c_int * 2)()
    _native().call('asr_lstm_last_path', ctypes.cast(out, ctypes.c_void_p))
    return [int(v) for v in out]


def _layer_params(inp, ref, sfx, dev, gen):
    """Device parameters with .grad filled with random values (compared:
    grad - fill; one fill for both bias gradients)."""
    ps, fills = [], {}
    for k in PARAMS:
        p = inp[k + sfx].to(dev).requires_grad_(True)
        scale = 0.25 * float(np.abs(ref[GRADS[k] + sfx]).max())
        fill = ((torch.rand(p.shape, generator=gen) * 2 - 1) * scale).to(dev)
        if k == 'b_hh':
            fill = fills['db_ih' + sfx]
        p.grad = fill.clone()
        ps.append(p)
        fills[GRADS[k] + sfx] = fill
    return ps, fills


def _run(case, precision, dev):
    """One forward + backward of the case on the device: ({tensor: torch}, paths)."""
    from pytorch_end2end_speech_recognition_amd import native_ops as ops
    c, inp, ref = R.CASES[case], R.case_inputs(case), R.reference(case)
    gen = torch.Generator().manual_seed(len(case))
    ps, fills = _layer_params(inp, ref, '', dev, gen)
    x = inp['x'].to(dev).requires_grad_(True)
    lens = torch.from_numpy(inp['lens']).to(dev)
    ops.set_compute_dtype(precision)
    try:
        ops.recurrence_status(dev)
        if c['stack']:
            hand = (0.2, R.HANDOFF_SEED)
            ps2, fills2 = _layer_params(inp, ref, '2', dev, gen)
            fills.update(fills2)
            y1 = ops.blstm_layer(x, lens, c['T'], *ps, bf16_handoff=True, out_drop=hand)
            y = ops.blstm_layer(y1, lens, c['T'], *ps2, drop=hand, next_rec=True)
            ps = ps + ps2
        else:
            y = ops.blstm_layer(x, lens, c['T'], *ps)
        y.backward(inp['dy'].to(dev))
        torch.cuda.synchronize()
        path = _last_path()
        st = ops.recurrence_status(dev)
        assert int(st.max()) == 0, ('a persistent recurrence gave up', st.tolist())
    finally:
        ops.set_compute_dtype('fp32')
    names = [GRADS[k] + s for s in (('', '2') if c['stack'] else ('',)) for k in PARAMS]
    got = dict(y=y.detach(), dx=x.grad)
    got.update({n: p.grad - fills[n] for n, p in zip(names, ps)})
    return got, path


def _check(tag, got, case, precision):
    ref, bound = R.reference(case), _bounds(case, precision)
    bad, line = [], []
    for k, g in got.items():
        g = g.double().cpu().numpy()
        assert g.shape == ref[k].shape and np.isfinite(g).all(), (tag, k)
        err = R.nerr(g, ref[k])
        # (dW_hh of a single frame is exactly zero)
        ratio = err / bound[k] if np.abs(ref[k]).max() > 0 else (np.inf if g.any() else 0.0)
        line.append('%s %.3f' % (k, ratio))
        if not ratio <= 1.0:
            bad.append((k, 'err/bound %.3f' % ratio, 'bound %.2e' % bound[k]))
    print(tag, 'err/bound:', ' '.join(line))
    assert not bad, (tag, bad)
    yh = got['y'].cpu().numpy()
    for b, n in enumerate(R.case_inputs(case)['lens']):
        assert not yh[b, n:].any(), ('y at padded frames of utterance', b)
    assert torch.equal(got['db_ih'], got['db_hh'])


def _set_env(monkeypatch, xu):
    for k in R.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if xu == 32:
        monkeypatch.setenv('ASR_XG_BWD_XU', '32')


@gpu
@pytest.mark.parametrize('xu', [16, 32])
@pytest.mark.parametrize('case', sorted(SHAPES))
def test_publish_matches_f64(case, xu, cuda_dev, monkeypatch):
    _set_env(monkeypatch, xu)
    B, H, _ = SHAPES[case]
    # work-groups of the tagged-granule backward under this setting: 8 rows per
    # group, two directions, H / xu producers each
    grid = _native().query('asr_lstm_backward_grid', B, H, 0)
    assert grid == 2 * -(-B // 8) * (H // xu), (grid, B, H, xu)
    got, path = _run(case, 'bf16', cuda_dev)
    assert path == [3, 1], ('fused forward, tagged-granule bf16 backward', path)
    _check('%s-xu%d' % (case, xu), got, case, 'bf16')


@gpu
def test_publish_f32_matches_f64(cuda_dev, monkeypatch):
    _set_env(monkeypatch, 16)
    got, path = _run(F32_SHAPE, 'fp32', cuda_dev)
    assert path == [2, 2], ('tagged-granule f32 forward and backward', path)
    _check(F32_SHAPE + '-fp32', got, F32_SHAPE, 'fp32')


@gpu
@pytest.mark.parametrize('xu', [16, 32])
def test_stack_twice_is_bitwise_equal(xu, cuda_dev, monkeypatch):
    _set_env(monkeypatch, xu)
    first, path = _run(STACK, 'bf16', cuda_dev)
    assert path[1] == 1, path
    _check('%s-xu%d' % (STACK, xu), first, STACK, 'bf16')
    again, path = _run(STACK, 'bf16', cuda_dev)
    assert path[1] == 1, path
    for k in first:
        assert torch.equal(first[k], again[k]), ('second run differs', k)


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['--record']:
        R.CASES.update(ALL)
        table = {}
        for case in sorted(ALL):
            m = R.measure_constants(case)
            table[case] = {'f32': m['f32'], 'bf16p': m['bf16p']}
        with open(CONSTANTS_JSON, 'w') as f:
            json.dump(table, f, indent=0, sort_keys=True)
            f.write('\n')
        print('recorded', len(table), 'cases in', CONSTANTS_JSON)
