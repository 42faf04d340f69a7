"""Every kernel family of csrc/gemm.hip on real-valued operands against the
float64 reference and derived bound of tests/gemm_ref.py.  Each test asserts
the family the launch took (asr_gemm_last_family() // 4), that every written
element is finite, and the bound per element.  Stored operands hold NaN in
their padding columns and in every row their row map skips; C starts as a NaN
bit pattern that must survive wherever the product does not write (so beta = 0
over a NaN C is every case without a beta).  Each case prints its largest
err / bound."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_end2end_speech_recognition_amd import native_ops
    return native_ops


def _NL():
    from pytorch_end2end_speech_recognition_amd import _native
    return _native


def _rowmap(ops, spec, ld, perm, dev, keep):
    pt = None
    if perm is not None:
        pt = torch.from_numpy(perm).to(dev)
        keep.append(pt)
    return ops.rowmap(ld, spec['T'] * ld if spec['rpb'] > 0 else 0, spec['rpb'], spec['t_mul'],
                      spec['t_add'], spec['t_limit'], perm=pt)


def _operand(ops, op, trans, dev, keep, off=0, bytes0=False):
    """The operand on the device: NaN wherever no logical element reads, and
    in the spare elements around a misaligned base."""
    store = np.where(op['read'], op['shadow'], np.float32(np.nan)).astype(np.float32)
    tdt = torch.bfloat16 if op['dt'] == 'bf16' else torch.float32
    n = store.size
    buf = torch.full((n + 8,), float('nan'), dtype=tdt, device=dev)
    buf[off:off + n] = torch.from_numpy(store).to(tdt).to(dev)
    view = buf[off:off + n]
    keep.append(buf)
    assert view.data_ptr() % 16 == (off * view.element_size()) % 16
    o = ops.operand(view, trans, _rowmap(ops, op['spec'], op['ld'], op['perm'], dev, keep))
    if bytes0:
        o.bytes = 0
    return o


def prepare(d, dev):
    """(asr_gemm_t, C's bits on the device [int32 / int16 view], keep-alive)."""
    ops, cs, keep = _ops(), d.cs, []
    a = _operand(ops, d.A, cs['at'], dev, keep, off=cs['a_off'], bytes0=cs['a_bytes0'])
    b = _operand(ops, d.B, cs['bt'], dev, keep)
    bf16c = cs['c'] == 'bf16'
    init = np.full(d.c_total + 4, R.SENT_BF16 if bf16c else R.SENT_F32,
                   np.int16 if bf16c else np.int32)
    if cs['beta'] != 0.0:
        init[cs['c_off']:].view(np.float32)[d.cidx] = d.c0[d.cidx]
    cbits = torch.from_numpy(init).to(dev)
    cview = cbits.view(torch.bfloat16 if bf16c else torch.float32)
    bias = [torch.from_numpy(x).to(dev) for x in d.bias] + [None, None]
    keep += bias
    p = ops.gemm_problem(a, b, cview, _rowmap(ops, d.cspec, d.ldc, d.cperm, dev, keep), cs['M'],
                         cs['N'], cs['K'], alpha=cs['alpha'], beta=cs['beta'], bias=bias[0],
                         bias2=bias[1], c_offset=cs['c_off'], batch=cs['batch'],
                         batch_strides=(d.A['sb'], d.B['sb'], d.sC))
    return p, cbits, keep


def run(d, dev, monkeypatch, lse=None):
    """One run_gemm of the case: (C's bits from c_off on, family)."""
    ops, NL, cs = _ops(), _NL(), d.cs
    for k, v in cs['env'].items():
        monkeypatch.setenv(k, v)
    p, cbits, keep = prepare(d, dev)
    ops.set_compute_dtype(cs['cd'])
    try:
        ops.run_gemm([p], dev, lse=lse, opts=NL.GemmOpts(**cs['opts']) if cs['opts'] else None)
        torch.cuda.synchronize()
        fam = NL.query('asr_gemm_last_family') // 4
    finally:
        ops.set_compute_dtype('fp32')
    return cbits.cpu().numpy()[cs['c_off']:][:d.c_total], fam


def _values(bits):
    if bits.dtype == np.int16:
        return (bits.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float32)


def check(d, bits, fam, ref=None, bound=None):
    """Family, finiteness, the bound per element (bit for bit in the integer
    bf16-C cases), and the sentinel wherever the product does not write."""
    cs = d.cs
    ref = d.ref if ref is None else ref
    bound = d.bound if bound is None else bound
    assert fam == cs['fam'], (cs['name'], R.FAM_NAMES.get(fam, fam))
    got = _values(bits)[d.cidx].astype(np.float64)
    assert np.isfinite(got).all(), (cs['name'], int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    print('gemm_real %-34s %-8s %s' % (cs['name'], R.FAM_NAMES[fam],
                                       'bit for bit' if cs['ints'] else 'err/bound %.4f' % ratio))
    if cs['ints']:
        want = torch.from_numpy(ref.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy()
        np.testing.assert_array_equal(bits[d.cidx], want)
    else:
        bad = err > bound
        assert not bad.any(), (cs['name'], int(bad.sum()), ratio)
    untouched = np.ones(bits.size, bool)
    untouched[d.cidx] = False
    sent = R.SENT_BF16 if bits.dtype == np.int16 else R.SENT_F32
    assert (bits[untouched] == sent).all(), cs['name']
    return ratio


@pytest.mark.parametrize('name', R.names('8w', 'kk256', 'n64', 'fast2', 'gen_bf16', 'f32f', 'gen_f32',
                                         'batch', 'epi', 'cmap', 'bf16c', 'bf16c_ties'))
def test_family_within_bound(name, cuda_dev, monkeypatch):
    """The table's cases: one launch each (see gemm_ref._table for what each
    group is there for).  'cmap': the rows whose frame falls outside C's limit
    and the frames between the written ones keep the sentinel; 'batch': so
    does the gap between C's batches; 'bf16c': so do the columns between N and
    C's pitch -- the bf16 store of store_acc writes columns n < N only."""
    d = R.build(R.CASES[name])
    if d.cs['group'] == 'cmap':
        assert not d.crow_ok.all() and d.crow_ok.any()
    bits, fam = run(d, cuda_dev, monkeypatch)
    check(d, bits, fam)


@pytest.mark.parametrize('name', R.names('stage'))
def test_in_library_staging(name, cuda_dev, monkeypatch):
    """f32 operands of a product of at least STAGE_FLOPS are converted to bf16
    copies in run_gemm's workspace (through their row maps and batches) and the
    product takes the LDS-DMA kernels: within the bound of the round-to-
    nearest-even operands; the one-launch conversion (ASR_GEMM_STAGE_MULTI=1)
    and the per-operand one give the same C bit for bit."""
    d = R.build(R.CASES[name])
    cs = d.cs
    assert 2.0 * cs['M'] * cs['N'] * cs['K'] * cs['batch'] >= 3.2e7
    if cs['batch'] > 1:
        bits, fam = run(d, cuda_dev, monkeypatch)
        check(d, bits, fam)
        return
    outs = []
    for multi in ('1', '0'):
        monkeypatch.setenv('ASR_GEMM_STAGE_MULTI', multi)
        bits, fam = run(d, cuda_dev, monkeypatch)
        check(d, bits, fam)
        outs.append(bits)
    np.testing.assert_array_equal(outs[0], outs[1])


def test_split_k_reduce_kernels_agree(cuda_dev, monkeypatch):
    """The same split-K product finished by splitk_reduce4 (N % 4 == 0, C
    16-B aligned) and by the scalar splitk_reduce (C one element off): equal
    bit for bit, both within the bound."""
    base = R.CASES['epi_splitk4']
    outs = []
    for c_off in (0, 1):
        d = R.build(dict(base, name='%s_coff%d' % (base['name'], c_off), c_off=c_off))
        assert d.ksplit > 1 and d.cs['N'] % 4 == 0 and d.ldc % 4 == 0
        bits, fam = run(d, cuda_dev, monkeypatch)
        check(d, bits, fam)
        outs.append(bits)
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize('name', R.names('lse'))
def test_lse_ws_writes_the_plain_c(name, cuda_dev, monkeypatch):
    """asr_gemm_lse_ws: the same family and, bit for bit, the C of a plain
    run_gemm of the same problem."""
    d = R.build(R.CASES[name])
    plain, fam = run(d, cuda_dev, monkeypatch)
    check(d, plain, fam)
    nq = (d.cs['N'] + 63) // 64
    lse = torch.full((nq, d.cs['M'], 2), float('nan'), device=cuda_dev)
    bits, fam2 = run(d, cuda_dev, monkeypatch, lse=lse)
    assert fam2 == fam
    np.testing.assert_array_equal(bits, plain)
    assert bool(torch.isfinite(lse).all())


def _raw_call(p, cd, dev, lse=None):
    NL = _NL()
    parr = ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)
    if lse is not None:
        rc = NL.lib().asr_gemm_lse_ws(parr, cd, NL.ptr(lse), None, 0, NL.stream_handle(dev), None)
    else:
        rc = NL.lib().asr_gemm_ws(parr, 1, cd, None, 0, NL.stream_handle(dev), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('why', ['beta', 'f32_compute', 'lse_ws'])
def test_bf16_c_refusals(why, cuda_dev):
    """A bf16 C with beta != 0, in f32 compute, or through asr_gemm_lse_ws:
    ASR_ERR_ARG (-1), and C is left as it was."""
    NL = _NL()
    d = R.build(R.CASES['bf16c_real_fast2'])
    p, cbits, keep = prepare(d, cuda_dev)
    before = cbits.clone()
    lse = None
    if why == 'beta':
        p.beta = 0.5
    if why == 'lse_ws':
        lse = torch.zeros((d.cs['N'] + 63) // 64, d.cs['M'], 2, device=cuda_dev)
    rc = _raw_call(p, NL.ASR_DT_F32 if why == 'f32_compute' else NL.ASR_DT_BF16, cuda_dev, lse)
    assert rc == -1, rc
    assert torch.equal(cbits, before)


@pytest.mark.parametrize('name', ['epi_fast2', 'epi_f32f'])
@pytest.mark.parametrize('M,N', [(0, None), (None, 0)])
def test_empty_output_extent_writes_nothing(name, M, N, cuda_dev):
    """M = 0 or N = 0: ASR_OK and no store."""
    NL = _NL()
    d = R.build(R.CASES[name])
    p, cbits, keep = prepare(d, cuda_dev)
    before = cbits.clone()
    if M == 0:
        p.M = 0
    if N == 0:
        p.N = 0
    rc = _raw_call(p, NL.ASR_DT_BF16 if d.cs['cd'] == 'bf16' else NL.ASR_DT_F32, cuda_dev)
    assert rc == NL.ASR_OK
    assert torch.equal(cbits, before)


@pytest.mark.parametrize('name', ['epi_8r', 'epi_fast2', 'epi_n64', 'epi_genbf16', 'epi_f32f'])
def test_empty_k_is_the_epilogue_alone(name, cuda_dev):
    """K = 0: the host routes an empty sum to the generic kernel, whose k loop
    runs zero tiles, and C = beta C + bias + bias2 (three roundings)."""
    NL = _NL()
    d = R.build(R.CASES[name])
    cs = d.cs
    p, cbits, keep = prepare(d, cuda_dev)
    p.K = 0
    bf = cs['cd'] == 'bf16'
    rc = _raw_call(p, NL.ASR_DT_BF16 if bf else NL.ASR_DT_F32, cuda_dev)
    assert rc == NL.ASR_OK
    fam = NL.query('asr_gemm_last_family') // 4
    c0 = d.c0[d.cidx].astype(np.float64)
    b1, b2 = (x.astype(np.float64) for x in d.bias)
    ref = cs['beta'] * c0 + b1 + b2
    S = abs(cs['beta']) * np.abs(c0) + np.abs(b1) + np.abs(b2)
    want = dict(cs, fam=R.FAM_GEN_BF16 if bf else R.FAM_GEN_F32)
    d2 = R.Data()
    d2.__dict__.update(d.__dict__)
    d2.cs = want
    check(d2, cbits.cpu().numpy()[:d.c_total], fam, ref=ref, bound=(0 + 1 + 6) * R.U_ACC * S)
