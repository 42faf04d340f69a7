"""The GEMM reference and bound of tests/gemm_ref.py are right and sharp, with
no GPU: for every case of the table two float32 evaluations of the product
stay inside the bound (soundness), and each wrong kernel the case can express
leaves it for at least one element (sharpness).  The row-map reader agrees
with test_gemm_gpu._mapped_rows, and the integer bf16-C cases contain the
roundings they are there for."""
import numpy as np
import pytest
import torch

import gemm_ref as R

ALL = list(R.CASES)


def test_table_covers_every_family_and_mutation():
    fams = {cs['fam'] for cs in R.CASES.values()}
    assert fams == {R.FAM_8R, R.FAM_8W, R.FAM_KK256, R.FAM_N64, R.FAM_FAST2, R.FAM_GEN_BF16,
                    R.FAM_GEN_F32, R.FAM_F32F}
    cases = list(R.CASES.values())
    assert any(c['cd'] == 'bf16' and c['a'] == 'f32' for c in cases)        # mutation (a)
    assert any(c['cd'] == 'fp32' for c in cases)                            # (b)
    assert any(c['amap'] or c['bmap'] for c in cases)                       # (d)
    assert any(c['nbias'] == 2 for c in cases)                              # (e)
    for cs in cases:       # every operand has padding columns to poison
        assert R._ld(cs['K'], cs['a']) > cs['K'] and R._ld(cs['N'], cs['b']) > cs['N']


@pytest.mark.parametrize('name', ALL)
def test_float32_evaluations_stay_inside_the_bound(name):
    d = R.build(R.CASES[name])
    if d.cs['ints']:
        assert np.array_equal(d.ref, np.round(d.ref))      # compared bit for bit on the GPU
        return
    base = d.bound - (2.0 ** -8 * np.abs(d.ref) if d.cs['c'] == 'bf16' else 0.0)
    assert np.isfinite(d.ref).all() and (d.S >= np.abs(d.ref) * (1 - 1e-12)).all()
    for how, got in (('tiles', R.evaluate_f32_tiles(d, d.A_log, d.B_log)),
                     ('matmul', R.evaluate(d, d.A_log, d.B_log, dtype=np.float32)[0])):
        err = np.abs(got.astype(np.float64) - d.ref)
        assert (err <= base).all(), (how, float((err / np.maximum(base, 1e-300)).max()))


@pytest.mark.parametrize('name', ALL)
def test_wrong_kernels_leave_the_bound(name):
    d = R.build(R.CASES[name])
    if d.cs['ints']:
        return
    muts = R.mutations(d)
    assert 'c_last_k_dropped' in muts
    if d.cs['cd'] == 'bf16' and 'f32' in (d.cs['a'], d.cs['b']):
        assert 'a_truncated' in muts
    if d.cs['cd'] == 'fp32':
        assert 'b_bf16_operands' in muts
    if d.cs['amap'] or d.cs['bmap'] or (d.cs['at'], d.cs['bt']) == (0, 0):
        assert 'd_masked_read' in muts
    if d.cs['nbias'] == 2:
        assert 'e_bias2_dropped' in muts
    for how, got in muts.items():
        assert (np.abs(got - d.ref) > d.bound).any(), how


def test_k_eff_and_ksplit():
    d = R.build(R.CASES['n64long_s2_256x17x65560_10'])
    assert d.K_eff == 440 and d.ksplit > 1
    assert R.build(R.CASES['fast2_sf1_kmap'])
    assert R.build(R.CASES['fast2_sf1_kmap']).K_eff == 5 * 35
    assert R.build(R.CASES['fast2_sf1_kmap_prev']).K_eff == 5 * 36
    assert R.ksplit(R.CASES['8r_256x256x64_00']) == 1
    assert R.ksplit(R.CASES['8r_256x257x1104_00']) > 1
    assert R.ksplit(R.CASES['epi_splitk1']) > 1 and R.ksplit(R.CASES['cmap_splitk']) > 1
    assert R.ksplit(R.CASES['f32f_s2_192x160x1100_00']) > 1
    assert R.ksplit(R.CASES['batch3_fast2_dense']) == 1


def test_row_map_reader_agrees_with_test_gemm_gpu():
    import test_gemm_gpu as G
    rng = np.random.RandomState(0)
    # the maps of test_fast_kernel_mapped_k_rows_exact / test_f32_fast_kernel_mapped_rows_exact
    rpb, T, t_mul, t_add, t_limit, nb = 37, 80, 2, 1, 60, 9
    for cols, ld in ((320, 328), (200, 208), (64, 324)):
        store = rng.standard_normal((nb * T, ld))
        for fn in (G._mapped_rows,):
            want = fn(store, rpb, T * ld, ld, t_mul, t_add, t_limit, nb * rpb, cols)
            got = R.mapped_rows(store, rpb, T * ld, ld, t_mul, t_add, t_limit, nb * rpb, cols)
            np.testing.assert_array_equal(got, want)
    # shifted maps (t_add = -1 / +1 with a limit) and a plain one
    store = rng.standard_normal((4 * 50, 24))
    for t_add in (-1, 1):
        np.testing.assert_array_equal(
            R.mapped_rows(store, 50, 50 * 24, 24, 1, t_add, 50, 200, 16),
            G._mapped_rows(store, 50, 50 * 24, 24, 1, t_add, 50, 200, 16))
    np.testing.assert_array_equal(R.mapped_rows(store, 0, 0, 24, 1, 0, 0, 200, 24), store)
    # perm: utterance b reads utterance perm[b]
    perm = np.array([2, 0, 3, 1])
    got = R.mapped_rows(store, 50, 50 * 24, 24, 1, 0, 0, 200, 24, perm=perm)
    np.testing.assert_array_equal(got, store.reshape(4, 50, 24)[perm].reshape(200, 24))


@pytest.mark.parametrize('name', R.names('bf16c_ties'))
def test_bf16_c_integer_cases_contain_the_roundings(name):
    d = R.build(R.CASES[name])
    ref = d.ref
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2048
    want = torch.from_numpy(ref.astype(np.float32)).to(torch.bfloat16).double().numpy()
    inexact = want != ref
    assert ((np.abs(ref) > 256) & inexact).any()           # low bits above 256
    # exact ties: the two bf16 neighbours are equally far
    a = np.abs(ref)
    ulp = np.exp2(np.floor(np.log2(np.maximum(a, 1))) - 7)
    tie = inexact & (np.abs(np.abs(want) - a) * 2 == ulp)
    assert (tie & (np.abs(want) > a)).any()                # tie rounding up to even
    assert (tie & (np.abs(want) < a)).any()                # tie rounding down to even
    assert (tie & ((np.abs(want) / ulp) % 2 != 0)).sum() == 0
    assert (ref < -256).any()


def test_empty_extents_are_host_only():
    """M = 0 or N = 0: ASR_OK before anything is launched (wg == 0), so the
    call needs no GPU; the pointers are never dereferenced."""
    import ctypes
    from pytorch_end2end_speech_recognition_amd import _native as NL
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    for M, N in ((0, 40), (70, 0), (0, 0)):
        for cd in (NL.ASR_DT_BF16, NL.ASR_DT_F32):
            g = NL.Gemm()
            g.M, g.N, g.K, g.batch, g.alpha = M, N, 64, 1, 1.0
            for op in (g.a, g.b):
                op.ptr, op.dtype, op.map.stride_t, op.bytes = addr, NL.ASR_DT_F32, 64, 256
            g.c, g.c_map.stride_t, g.c_dtype = addr, max(N, 1), NL.ASR_DT_F32
            rc = NL.lib().asr_gemm_ws(ctypes.cast(ctypes.pointer(g), ctypes.c_void_p), 1, cd, None,
                                      0, None, None)
            assert rc == NL.ASR_OK, (M, N, cd)
