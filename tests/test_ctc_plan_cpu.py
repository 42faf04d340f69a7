"""The bf16 CTC gradient's plan (csrc/ctc.hip, ctc_grad_plan) through the
host-only query asr_ctc_grad_plan: which kernel runs, with which template
arguments, on which grid and with how much LDS -- no GPU (the CU count is
given: 256) and a 16-B aligned dummy address for the activations.

The shapes are those of tests/test_ctc_widths_gpu.py, B 3 x T 14 (42 rows),
max_label_len 5 (64 padded lattice states), with bias sums.  path is
asr_ctc_last_path()[1]'s number (1 ctc_grad_bf16, 2 _narrow, 3 _pipe,
4 _stream), NCH the kernel's 8-column chunks per thread:

    V      pitch  gld    default         ASR_CTC_GRAD_STREAM=0  + ASR_CTC_GRAD_PIPE=0
    2051   2052   2056   4, NCH 1        3, NCH 2               1, NCH 2, aligned
    2051   2051   2056   1, NCH 2, not aligned (every setting)
    4099   4100   4104   4, NCH 2        3, NCH 4               1, NCH 4
    6151   6152   6152   4, NCH 2        3, NCH 4               1, NCH 4
    10243  10244  10248  4, NCH 3        3, NCH 8               1, NCH 8
    14339  14340  14344  3, NCH 8        3, NCH 8               1, NCH 8
    16389  16392  16392  no bias: 1, NCH 0; with bias: ASR_ERR_UNSUPPORTED

The literals restate the dispatch as it stood before the plan function
existed (the five-kernel choice inside ctc_backward_bf16_impl)."""
import itertools

import pytest

import ctc_width_ref as R

B, T, MLL, SPAD, CUS, ADDR = 3, 14, 5, 64, 256, 4096
ENVS = ('ASR_CTC_GRAD_STREAM', 'ASR_CTC_GRAD_PIPE', 'ASR_CTC_GRAD_NARROW', 'ASR_CTC_BIAS_BLOCKS',
        'ASR_CTC_ORDER')
DEFAULT, NO_STREAM, PLAIN = {}, {'ASR_CTC_GRAD_STREAM': '0'}, {'ASR_CTC_GRAD_STREAM': '0',
                                                               'ASR_CTC_GRAD_PIPE': '0'}
# (V, pitch): ((path, NCH) under DEFAULT, NO_STREAM, PLAIN)
TABLE = {
    (2051, 2052): ((4, 1), (3, 2), (1, 2)),
    (2051, 2051): ((1, 2), (1, 2), (1, 2)),
    (4099, 4100): ((4, 2), (3, 4), (1, 4)),
    (6151, 6152): ((4, 2), (3, 4), (1, 4)),
    (10243, 10244): ((4, 3), (3, 8), (1, 8)),
    (14339, 14340): ((3, 8), (3, 8), (1, 8)),
}
assert set(TABLE) | {(16389, 16392)} == set(R.WIDTHS)


def _N():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


@pytest.fixture
def env(monkeypatch):
    """Sets exactly the given switches (the others unset)."""
    def set_(**kv):
        for e in ENVS:
            monkeypatch.delenv(e, raising=False)
        for k, v in kv.items():
            monkeypatch.setenv(k, v)
    set_()
    return set_


def _plan(V, P, bias=True, t=T, b=B, mll=MLL, gld=None, cus=CUS):
    return _N().ctc_grad_plan(t, b, V, gld or R.gld_of(V), mll, ADDR, P, t * P, bias, cus)


def _lds(p, V, bias):
    """The LDS bytes the kernels of each path index (Spad 64)."""
    n8 = R.gld_of(V) // 8
    if p.path == 2:
        return (4 * V + (4 * R.gld_of(V) if bias else 0)) * 4
    if p.path == 4:
        return (5 * SPAD + n8 + 8) * 4
    return (V if V <= 256 else 2 * SPAD + (V if bias else 0)) * 4


@pytest.mark.parametrize('bias_blocks', [None, '2'], ids=['bb_default', 'bb2'])
@pytest.mark.parametrize('V,P', sorted(TABLE), ids=['V%d_P%d' % vp for vp in sorted(TABLE)])
def test_width_table(V, P, bias_blocks, env):
    for switches, (path, nch) in zip((DEFAULT, NO_STREAM, PLAIN), TABLE[(V, P)]):
        env(**switches, **({'ASR_CTC_BIAS_BLOCKS': bias_blocks} if bias_blocks else {}))
        p = _plan(V, P)
        what = (V, P, switches, bias_blocks)
        assert (p.path, p.nch) == (path, nch), what
        assert p.aligned == (P % 4 == 0), what
        assert p.threads == (512 if path == 4 else 256), what
        assert (p.rpb, p.nblk) == ((21, 2) if bias_blocks else (1, 42)), what
        assert p.lds_bytes == _lds(p, V, True), what
        assert p.acts_bytes == 4 * ((B * T - 1) * P + V), what
        assert p.part_bytes == (p.nblk * R.gld_of(V) * 4 + 255) // 256 * 256, what
    if (V, P) == (14339, 14340):
        env(ASR_CTC_GRAD_PIPE='0')            # too wide for the streamed pass: PIPE=0 alone
        assert _plan(V, P).path == 1


def test_literals_of_the_first_row(env):
    p = _plan(2051, 2052)
    assert (p.path, p.nch, p.threads, p.lds_bytes) == (4, 1, 512, 2340)
    env(**NO_STREAM)
    p = _plan(2051, 2052)
    assert (p.path, p.nch, p.threads, p.lds_bytes) == (3, 2, 256, 8716)
    env(**PLAIN)
    p = _plan(2051, 2052)
    assert (p.path, p.nch, p.aligned, p.lds_bytes) == (1, 2, 1, 8716)


def test_v16389_refused_with_bias_only(env):
    N = _N()
    p = _plan(16389, 16392, bias=False)
    assert (p.path, p.nch, p.aligned, p.part_bytes) == (1, 0, 1, 0)
    assert (p.rpb, p.nblk, p.lds_bytes) == (1, 42, 2 * SPAD * 4)
    with pytest.raises(N.NativeError) as ei:
        _plan(16389, 16392, bias=True)
    assert 'rc=%d' % N.ASR_ERR_UNSUPPORTED in str(ei.value) and 'too wide' in str(ei.value)


def test_pipe_needs_bias_sums(env):
    """Without bias sums the chunk count stays 0: the pipelined form is never
    chosen, while the streamed one takes its own NCH either way."""
    p = _plan(4099, 4100, bias=False)
    assert (p.path, p.nch, p.rpb, p.nblk) == (4, 2, 1, 42)
    env(**NO_STREAM)
    p = _plan(4099, 4100, bias=False)
    assert (p.path, p.nch, p.aligned, p.lds_bytes) == (1, 0, 1, 2 * SPAD * 4)


def test_narrow_head(env):
    V, gld = 29, 32
    p = _plan(V, V)
    assert (p.path, p.threads, p.rpb, p.nblk) == (2, 256, 3, 14)
    assert p.lds_bytes == (4 * 29 + 4 * 32) * 4
    p = _plan(V, V, bias=False)
    assert (p.path, p.threads, p.rpb, p.nblk) == (2, 256, 4, 11)
    assert p.lds_bytes == 4 * 29 * 4
    env(ASR_CTC_GRAD_NARROW='0')
    for bias, nch in ((True, 1), (False, 0)):
        p = _plan(V, V, bias=bias)
        assert (p.path, p.threads, p.nch, p.aligned) == (1, 64, nch, 0)
        assert p.lds_bytes == V * 4
    # the one-wave table form is built with NCH 1 only, whatever the pitch of dY
    assert _plan(200, 200, gld=1024).nch == 1
    assert gld == R.gld_of(V)


def test_refusals_agree_with_bias_supported(env):
    N = _N()
    points = [(V, mll) for V in (29, 2051, 14336, 14337, 15360, 15361, 16256, 16257, 16384, 16389)
              for mll in (5, 255, 300)] + [(4099, 512)]
    refused = []
    for V, mll in points:
        gld = R.gld_of(V)
        try:
            _plan(V, gld, mll=mll)
            ok = 1
        except N.NativeError as e:
            assert 'rc=%d' % N.ASR_ERR_UNSUPPORTED in str(e) and 'ctc_grad_plan:' in str(e), str(e)
            # "too wide" names the two width reasons only, not labels beyond the lattice
            assert ('too wide' in str(e)) == (mll <= 511) and ('labels' in str(e)) == (mll > 511)
            ok = 0
            refused.append((V, mll))
        assert N.query('asr_ctc_bias_supported', V, gld, mll) == ok, (V, mll)
    assert (16257, 5) in refused and (14337, 300) in refused and (15361, 255) in refused
    assert (4099, 512) in refused and (16256, 5) not in refused


SWEEP = [(t, b, V, mll) for (t, b) in ((14, 3), (1, 1), (1000, 32), (37, 5))
         for V, mll in ((29, 5), (29, 125), (256, 31), (257, 31), (1000, 60), (4099, 300),
                        (10001, 40), (12288, 5), (12289, 5), (14339, 5))]


@pytest.mark.parametrize('bias_blocks,cus', [(None, 256), ('2', 256), ('5000', 8), (None, 1),
                                             ('64', 304)])
def test_sweep_grid_covers_rows_and_fits(bias_blocks, cus, env):
    """Production heads (V = 29, 1000, 10001 at B 32 x T 1000) among them:
    the grid covers every row, LDS within a work-group's 64 KiB, and the
    partial rows within what asr_ctc_bias_workspace_bytes sizes."""
    N = _N()
    for switches, (t, b, V, mll) in itertools.product((DEFAULT, NO_STREAM, PLAIN), SWEEP):
        env(**switches, **({'ASR_CTC_BIAS_BLOCKS': bias_blocks} if bias_blocks else {}))
        P = (V + 3) // 4 * 4 if V > 1024 else V
        gld = R.gld_of(V)
        for bias in (True, False):
            p = _plan(V, P, bias=bias, t=t, b=b, mll=mll, cus=cus)
            what = (switches, t, b, V, mll, bias, p.path, p.rpb, p.nblk)
            assert 1 <= p.path <= 4 and p.rpb >= 1 and p.nblk >= 1, what
            assert p.nblk * p.rpb >= t * b, what
            assert (p.nblk - 1) * p.rpb < t * b, what     # no block without a row
            assert p.lds_bytes <= 64 * 1024, what
            if bias:
                assert p.part_bytes >= p.nblk * gld * 4, what
                assert p.part_bytes <= N.query('asr_ctc_bias_workspace_bytes', t, b, V, gld), what


def test_production_heads(env):
    """B 32 x T 1000 as the benchmark's configurations run them."""
    p = _plan(29, 29, t=1000, b=32, mll=125)
    assert (p.path, p.rpb, p.nblk) == (2, 4, 8000)
    p = _plan(1000, 1000, t=1000, b=32, mll=60)
    assert (p.path, p.nch, p.threads, p.rpb, p.nblk) == (4, 1, 512, 63, 508)
    env(**NO_STREAM)
    p = _plan(1000, 1000, t=1000, b=32, mll=60)
    assert (p.path, p.nch, p.aligned, p.rpb, p.nblk) == (3, 1, 1, 31, 1033)
    env()
    p = _plan(10001, 10004, t=1000, b=32, mll=40)
    assert (p.path, p.nch, p.threads, p.rpb, p.nblk) == (4, 3, 512, 63, 508)


def test_row_order_is_read_per_call(env):
    env(ASR_CTC_ORDER='0')
    assert _plan(4099, 4100).rev == 0
    env(ASR_CTC_ORDER='2')
    assert _plan(4099, 4100).rev == 1
    env()
    assert _plan(4099, 4100).rev == 1           # the default: the gradient pass descending
