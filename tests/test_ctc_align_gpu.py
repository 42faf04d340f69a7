"""asr_ctc_align on the device against ctc_align_ref.align_f32: ali, starts and
ends bit for bit on every case; scores bitwise where the sums are exact
(normalize = 0 on quarter-valued and all-zero logits), otherwise within
ctc_align_ref's bound (err / bound printed per case).
"""
import functools

import numpy as np
import pytest
import torch

import ctc_align_ref as R

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _limits():
    return _ops().ctc_align_limits()


_REF = {}


def _ref(key, case):
    """align_batch of a case, computed once per id."""
    if key not in _REF:
        _REF[key] = R.align_batch(case['x'], case['lens'], case['labs'], case['blank'], case['M'])
    return _REF[key]


def _abi(dev, case, normalize=1, time_major=False, spans=True, ws_fill=None, ws_short=0,
         prefill=None, M=None):
    """One raw asr_ctc_align call; returns (rc, ali, starts, ends, scores) as numpy."""
    N = _N()
    x = case['x']
    B, T, V = x.shape
    M = case['M'] if M is None else M
    flat, ll = R.flat_labels(case)
    if time_major:
        xd = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev)
        st, sb = B * V, V
    else:
        xd = torch.from_numpy(x).to(dev)
        st, sb = V, T * V
    fl = torch.from_numpy(flat if len(flat) else np.zeros(1, np.int32)).to(dev)
    lld = torch.from_numpy(ll).to(dev)
    al = torch.from_numpy(np.asarray(case['lens'], np.int32)).to(dev)
    fill = -7 if prefill is None else prefill
    ali = torch.full((B, T), fill, dtype=torch.int32, device=dev)
    starts = torch.full((B, max(M, 1)), fill, dtype=torch.int32, device=dev)
    ends = torch.full((B, max(M, 1)), fill, dtype=torch.int32, device=dev)
    scores = torch.full((B,), 123.0, dtype=torch.float32, device=dev)
    nb = N.query('asr_ctc_align_ws_bytes', T, B, V, M)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    rc = N.lib().asr_ctc_align(
        N.ptr(xd), st, sb, T, B, V, N.ptr(fl), N.ptr(lld), N.ptr(al), M, case['blank'], normalize,
        N.ptr(ali), N.ptr(starts) if spans else None, N.ptr(ends) if spans else None,
        N.ptr(scores), N.ptr(ws), max(nb - ws_short, 0), N.stream_handle(dev))
    torch.cuda.synchronize()
    return (rc, ali.cpu().numpy(), starts.cpu().numpy()[:, :M], ends.cpu().numpy()[:, :M],
            scores.cpu().numpy())


def _check_paths(key, case, got):
    rc, ali, starts, ends, _ = got
    want = _ref(key, case)
    assert rc == 0
    np.testing.assert_array_equal(ali, want[0], err_msg=key)
    np.testing.assert_array_equal(starts, want[1], err_msg=key)
    np.testing.assert_array_equal(ends, want[2], err_msg=key)
    return want


def _check_scores(key, case, scores, want, kc):
    """The normalised scores against score_f64 of the reference's path."""
    for b in range(len(scores)):
        if not want[4][b]:
            assert scores[b] == -np.inf, (key, b)
            continue
        Tb = max(min(int(case['lens'][b]), case['x'].shape[1]), 0)
        ref, A = R.score_f64(case['x'][b], want[0][b, :Tb])
        err, bd = abs(float(scores[b]) - ref), R.bound(kc, A)
        print('%-22s b %d  score %.6f  err %.3g  bound %.3g  err/bound %.3f'
              % (key, b, ref, err, bd, err / bd if bd else 0.0))
        assert err <= bd, (key, b, err, bd)


def _check_exact_scores(key, scores, want):
    """normalize = 0: the end value, bitwise."""
    np.testing.assert_array_equal(scores.view(np.int32), want[3].view(np.int32), err_msg=key)


@pytest.mark.parametrize('key', sorted(R.CASES))
def test_cases(cuda_dev, key):
    """Label lengths 0 / 1 / T, tight and infeasible repeats, rows without
    frames, every width with blank 0 and V - 1, B 300, ragged lengths with NaN
    padding: paths bit for bit, normalised scores within the bound, raw scores
    (normalize = 0) bitwise the end value."""
    case = R.CASES[key]
    got = _abi(cuda_dev, case)
    want = _check_paths(key, case, got)
    if key in R.consts():
        _check_scores(key, case, got[4], want, R.consts()[key])
    else:
        assert (got[4][~want[4]] == -np.inf).all()
    raw = _abi(cuda_dev, case, normalize=0)
    _check_paths(key, case, raw)
    _check_exact_scores(key, raw[4], want)


def test_infeasible_cases_are_infeasible():
    """The cases meant to be infeasible are, by the reference."""
    assert not _ref('repeats_short', R.CASES['repeats_short'])[4][0]
    assert _ref('repeats_tight', R.CASES['repeats_tight'])[4][0]
    np.testing.assert_array_equal(_ref('len0', R.CASES['len0'])[4], [True, False, True])


@pytest.mark.parametrize('L', R.TIER_LS)
def test_lane_ownership_tiers(cuda_dev, L):
    """L on both sides of every states-per-lane tier (K 1 .. 16), T = L + 3."""
    key, case = 'tier%d' % L, R.tier_case(L)
    got = _abi(cuda_dev, case)
    want = _check_paths(key, case, got)
    assert want[4][0], 'the tier case must be feasible'
    _check_scores(key, case, got[4], want, R.consts()[key])
    raw = _abi(cuda_dev, case, normalize=0)
    _check_paths(key, case, raw)
    _check_exact_scores(key, raw[4], want)


def test_backtrace_chunks(cuda_dev):
    """T around the backtrace's chunk size and its LDS-resident limit (both
    asked of the library), and one T of more than three chunks past the limit."""
    chunk, lds = _limits()
    assert chunk > 0 and lds % chunk == 0
    # the recorded K_score constants are of the cases at these limits
    assert (chunk, lds) == (R.CHUNK_FRAMES, R.LDS_FRAMES)
    for key, case in R.chunk_cases(chunk, lds).items():
        got = _abi(cuda_dev, case)
        want = _check_paths(key, case, got)
        _check_scores(key, case, got[4], want, R.consts()[key])
        _check_exact_scores(key, _abi(cuda_dev, case, normalize=0)[4], want)


@pytest.mark.parametrize('key', ['V5', 'V1025_blank1024', 'ragged_nan'])
def test_time_major(cuda_dev, key):
    case = R.CASES[key]
    _check_paths(key, case, _abi(cuda_dev, case, time_major=True))


@pytest.mark.parametrize('key', sorted(R.EXACT))
def test_ties_exact(cuda_dev, key):
    """Quarter-valued logits and the all-zero tensor: every sum is exact and
    (zeros) every decision a tie; scores bitwise the reference's."""
    case = R.EXACT[key]
    got = _abi(cuda_dev, case, normalize=0)
    want = _check_paths(key, case, got)
    _check_exact_scores(key, got[4], want)
    _check_paths(key, case, _abi(cuda_dev, case, normalize=1))


def test_masked_classes(cuda_dev):
    """-inf on classes the labels do not use changes no path and the lse
    ignores them; -inf on a needed column makes the row infeasible."""
    base = R.CASES['V29']
    used = set([base['blank']] + [int(c) for l in base['labs'] for c in l])
    free = [c for c in range(29) if c not in used]
    m = dict(base, x=base['x'].copy())
    m['x'][:, :, free[:9]] = -np.inf
    got = _abi(cuda_dev, m)
    want = _check_paths('V29', base, got)       # the unmasked case's paths
    _check_scores('V29_masked', m, got[4], want, R.consts()['V29'])
    n = dict(base, x=base['x'].copy())
    n['x'][1, 2, :] = -np.inf                    # frame 2 of utterance 1: nothing is reachable
    n['x'][0, :, int(base['labs'][0][0])] = -np.inf   # a label column of utterance 0
    got = _abi(cuda_dev, n)
    want = _check_paths('V29_needed', n, got)
    np.testing.assert_array_equal(want[4], [False, False, True])
    assert (got[1][:2] == -1).all() and (got[4][:2] == -np.inf).all()


def test_bad_rows(cuda_dev):
    """A label >= V, a label equal to blank, a negative label and a label_len
    beyond max_label_len, each beside good rows: that row alone is infeasible
    (all -1, -inf), the others equal the reference and the whole the host path."""
    N, ops = _N(), _ops()
    base = R.CASES['V29']
    flat, ll = R.flat_labels(base)
    B, T, V = base['x'].shape
    M = base['M']
    want = _ref('V29', base)
    dev = cuda_dev

    def run(f, l):
        xd = torch.from_numpy(base['x']).to(dev)
        ali = torch.full((B, T), -7, dtype=torch.int32, device=dev)
        st = torch.full((B, M), -7, dtype=torch.int32, device=dev)
        en = torch.full((B, M), -7, dtype=torch.int32, device=dev)
        sc = torch.full((B,), 123.0, dtype=torch.float32, device=dev)
        nb = N.query('asr_ctc_align_ws_bytes', T, B, V, M)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        fd, ld = torch.from_numpy(f).to(dev), torch.from_numpy(l).to(dev)
        al = torch.from_numpy(np.asarray(base['lens'], np.int32)).to(dev)
        rc = N.lib().asr_ctc_align(
            N.ptr(xd), V, T * V, T, B, V, N.ptr(fd), N.ptr(ld), N.ptr(al), M, base['blank'],
            1, N.ptr(ali), N.ptr(st), N.ptr(en), N.ptr(sc), N.ptr(ws), nb, N.stream_handle(dev))
        torch.cuda.synchronize()
        assert rc == 0
        return ali.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy(), sc.cpu().numpy()

    good = run(flat, ll)
    for g, w in zip(good[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    for row, bad in ((1, V), (1, base['blank']), (0, -3), (2, V + 1000)):
        f = flat.copy()
        f[int(ll[:row].sum())] = bad            # the row's first label
        got = run(f, ll)
        host = ops.ctc_align_host(base['x'], base['lens'], f, ll, M, base['blank'])
        for g, h in zip(got[:3], host[:3]):
            np.testing.assert_array_equal(g, h)
        assert (got[0][row] == -1).all() and (got[1][row] == -1).all() and (got[2][row] == -1).all()
        assert got[3][row] == -np.inf
        for b in range(B):
            if b != row:
                np.testing.assert_array_equal(got[0][b], want[0][b])
                assert got[3][b] == good[3][b]
    # label_len beyond max_label_len (row 1), and a negative one (row 2): the
    # flat labels keep their layout (a negative length takes no labels)
    for row, val in ((1, M + 1), (2, -1)):
        l = ll.copy()
        l[row] = val
        f = flat if val < 0 and row == B - 1 else np.concatenate(
            [flat[:int(ll[:row].sum())], np.full(max(val, 0), 1 if base['blank'] != 1 else 2, np.int32),
             flat[int(ll[:row + 1].sum()):]]).astype(np.int32)
        got = run(f, l)
        host = ops.ctc_align_host(base['x'], base['lens'], f, l, M, base['blank'])
        for g, h in zip(got[:3], host[:3]):
            np.testing.assert_array_equal(g, h)
        assert (got[0][row] == -1).all() and got[3][row] == -np.inf
        for b in range(B):
            if b != row:
                np.testing.assert_array_equal(got[0][b], want[0][b])
                np.testing.assert_array_equal(got[1][b], want[1][b])


def test_null_spans(cuda_dev):
    case = R.CASES['V29']
    got = _abi(cuda_dev, case, spans=False)
    want = _ref('V29', case)
    np.testing.assert_array_equal(got[1], want[0])
    assert (got[2] == -7).all() and (got[3] == -7).all()      # untouched


def test_workspace(cuda_dev):
    """One byte short: ASR_ERR_WORKSPACE and nothing written; a workspace of
    0xFF bytes: the same results."""
    N = _N()
    chunk, lds = _limits()
    case = R.chunk_cases(chunk, lds)['T%d' % (lds + 1)]
    got = _abi(cuda_dev, case, ws_short=1)
    assert got[0] == N.ASR_ERR_WORKSPACE
    assert (got[1] == -7).all() and (got[4] == 123.0).all()
    a = _abi(cuda_dev, case, ws_fill=0xFF)
    b = _abi(cuda_dev, case, ws_fill=0)
    _check_paths('T%d' % (lds + 1), case, a)
    for u, v in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(u.view(np.int32), v.view(np.int32))


def test_refusal_and_host_path(cuda_dev):
    """max_label_len 512: refused with the outputs untouched; native_ops then
    answers through the host path with the reference's values."""
    N, ops = _N(), _ops()
    case = R.make_case(77, 520, 5, [512, 3])
    got = _abi(cuda_dev, case)
    assert got[0] == N.ASR_ERR_UNSUPPORTED
    assert (got[1] == -7).all() and (got[2] == -7).all() and (got[4] == 123.0).all()
    assert N.query('asr_ctc_align_ws_bytes', 520, 2, 5, 512) == 0
    flat, ll = R.flat_labels(case)
    dev = cuda_dev
    for normalize in (True, False):
        res = ops.ctc_align(torch.from_numpy(case['x']).to(dev),
                            torch.from_numpy(case['lens']).to(dev), torch.from_numpy(flat).to(dev),
                            torch.from_numpy(ll).to(dev), 512, blank=0, normalize=normalize)
        assert ops.last_ctc_align_path() == 'host'
        assert all(r.is_cuda for r in res)
        want = _ref('refused', case)
        for g, w in zip(res[:3], want[:3]):
            np.testing.assert_array_equal(g.cpu().numpy(), w)
        if not normalize:
            _check_exact_scores('refused', res[3].cpu().numpy(), want)
    # the same call one label shorter runs on the device
    case = R.tier_case(511)
    flat, ll = R.flat_labels(case)
    res = ops.ctc_align(torch.from_numpy(case['x']).to(dev), torch.from_numpy(case['lens']).to(dev),
                        torch.from_numpy(flat).to(dev), torch.from_numpy(ll).to(dev), 511)
    assert ops.last_ctc_align_path() == 'device'
    np.testing.assert_array_equal(res[0].cpu().numpy(), _ref('tier511', case)[0])


def test_native_ops_layouts(cuda_dev):
    """native_ops.ctc_align reads a transposed time-major tensor in place and
    returns what the raw call returns; spans=False gives None."""
    ops = _ops()
    case = R.CASES['ragged_nan']
    flat, ll = R.flat_labels(case)
    dev = cuda_dev
    tm = torch.from_numpy(np.ascontiguousarray(case['x'].transpose(1, 0, 2))).to(dev)
    args = (torch.from_numpy(case['lens']).to(dev), torch.from_numpy(flat).to(dev),
            torch.from_numpy(ll).to(dev), case['M'])
    a = ops.ctc_align(tm.transpose(0, 1), *args)
    b = ops.ctc_align(torch.from_numpy(case['x']).to(dev), *args, spans=False)
    want = _ref('ragged_nan', case)
    for g, w in zip(a[:3], want[:3]):
        assert g.dtype == torch.int32
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    assert b[1] is None and b[2] is None
    np.testing.assert_array_equal(b[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(a[3].cpu().numpy().view(np.int32),
                                  b[3].cpu().numpy().view(np.int32))


def test_deterministic(cuda_dev):
    chunk, lds = _limits()
    case = R.chunk_cases(chunk, lds)['T%d' % (lds + 3 * chunk + 5)]
    a, b = _abi(cuda_dev, case), _abi(cuda_dev, case)
    for u, v in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(u.view(np.int32), v.view(np.int32))
