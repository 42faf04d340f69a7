"""Real-valued cases of csrc/gemm.hip, their float64 reference and the derived
per-element bound.  tests/test_gemm_ref_cpu.py shows that the bound is sound
(two float32 evaluations stay inside it) and sharp (five wrong kernels leave
it); tests/test_gemm_real_gpu.py holds every kernel family to it.

A case is a dict (see `case`): shapes and layouts, operand dtypes in memory,
row maps, batch, alpha / beta / biases, compute dtype, the environment and
GemmOpts that select the kernel family, and the family expected from
asr_gemm_last_family() // 4 (ASR_PTAG_GEMM_* of csrc/prof.h).

Reference: float64 of the logical operands, read through `mapped_rows` (a
numpy asr_rowmap_t); in bf16 compute every f32-in-memory operand is first
rounded with torch's CPU .to(bfloat16) (round to nearest even).

Bound, per element:   |got - ref| <= (K_eff + ksplit + 6) * 2^-23 * S
  S[m, n] = |alpha| sum_k |a||b| + |beta||c0| + |bias| + |bias2|
  K_eff   = the k terms that neither operand's row map masks
  ksplit  = split-K slabs of the workspace plan (1 without a split)
bf16 x bf16 products are exact in f32 and f32 products round once; a sum of n
terms in any order errs by at most gamma_n S for unit roundoff u, and 2^-23 is
u of a truncating accumulator (twice round-to-nearest's), so the bound holds
however the MFMA unit rounds inside.  The 6 covers alpha, the two biases, the
beta term, the slab sum's alpha and one spare.  A real-valued bf16 C adds
2^-8 |ref| (one rounding of the stored value).

Largest observed err / bound per family on an MI355X (test_gemm_real_gpu.py
prints one line per case):

  family     f32 C   (real-valued bf16 C, where 2^-8 |ref| is the bound's
  ---------  -----    larger part and round-to-nearest can reach 1.0)
  8R         0.013
  8W         0.013
  KK256      0.004
  N64        0.003   (0.95)
  FAST2      0.006   (0.97)
  GEN_BF16   0.013   (0.98)
  GEN_F32    0.031
  F32F       0.036
  K = 0 (the epilogue alone, bound 7 * 2^-23 S): 0.14 on either generic kernel.
  (FAST4 is off by default and ASR_GEMM_STAGES is read once per process: not
  reachable from a suite that also runs FAST2, so it has no cases.)
"""
import ctypes
import functools

import numpy as np
import torch

# asr_gemm_last_family() // 4 (csrc/prof.h, ASR_PTAG_GEMM_*)
FAM_8R, FAM_8W, FAM_KK256, FAM_N64, FAM_FAST2, FAM_FAST4 = 1, 2, 3, 4, 5, 6
FAM_GEN_BF16, FAM_GEN_F32, FAM_F32F = 7, 8, 12
FAM_NAMES = {1: '8R', 2: '8W', 3: 'KK256', 4: 'N64', 5: 'FAST2', 6: 'FAST4', 7: 'GEN_BF16',
             8: 'GEN_F32', 12: 'F32F'}

U_ACC = 2.0 ** -23           # unit roundoff of a truncating f32 accumulator
SENT_F32 = 0x7fc12345        # NaN bit patterns no kernel produces: unwritten C
SENT_BF16 = 0x7fc1
L4 = [(0, 0), (0, 1), (1, 0), (1, 1)]


def rne_bf16(x):
    """float values rounded to bf16 by torch's CPU conversion, as float64."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16).double().numpy()


def trunc_bf16(x):
    """float32 values with the low 16 bits cleared (the wrong conversion)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return b.view(np.float32).astype(np.float64)


# --------------------------------------------------------------- asr_rowmap_t
def row_offsets(nrows, stride_t, stride_b=0, rpb=0, t_mul=1, t_add=0, t_limit=0, perm=None):
    """(offset of logical row r, or -1 where the map masks it; the unmasked
    offset), as row_off of gemm.hip computes them."""
    r = np.arange(nrows, dtype=np.int64)
    b, t = (r // rpb, r % rpb) if rpb > 0 else (np.zeros_like(r), r)
    tp = t * (t_mul if t_mul else 1) + t_add
    ok = (tp >= 0) & (tp < (t_limit if t_limit > 0 else 1 << 30))
    bp = np.asarray(perm, np.int64)[b] if perm is not None else b
    raw = bp * stride_b + tp * stride_t
    return np.where(ok, raw, -1), raw


def mapped_rows(store, rpb, stride_b, stride_t, t_mul, t_add, t_limit, nrows, ncols, perm=None):
    """Rows 0..nrows-1 of an operand read through asr_rowmap_t, zero where the
    mapped frame falls outside [0, t_limit) (test_gemm_gpu._mapped_rows with
    the batch permutation)."""
    off, _ = row_offsets(nrows, stride_t, stride_b, rpb, t_mul, t_add, t_limit, perm)
    flat = np.asarray(store).reshape(-1)
    out = np.zeros((nrows, ncols), np.float64)
    ok = off >= 0
    out[ok] = flat[off[ok][:, None] + np.arange(ncols)]
    return out


def gmap(rpb, T, t_mul=1, t_add=0, t_limit=0, perm=False):
    """A grouped row map over storage of T frames per utterance."""
    return dict(rpb=rpb, T=T, t_mul=t_mul, t_add=t_add, t_limit=t_limit, perm=perm)


# ---------------------------------------------------------------------- cases
def case(name, group, fam, M, N, K, at=0, bt=0, cd='bf16', a='bf16', b='bf16', c='f32',
         amap=None, bmap=None, cmap=None, batch=1, bkind='dense', cgap=0, cpad=4, alpha=1.0,
         beta=0.0, nbias=2, env=None, opts=None, a_off=0, c_off=0, a_bytes0=False, scale=False,
         ints=0, seed=0):
    """bkind: 'dense' | 'bcast_a' (batch_stride_a = 0) | 'odd' (operand batch
    strides that are no multiple of 4) | 'mul4' (a multiple of 4, not of 8).
    a_off: A's base that many elements past a 16-B boundary.  a_bytes0: A's
    readable extent passed as unknown.  scale: |a| spans 2^-10 .. 2^10.
    ints: operands are integers in [-ints, ints] (the bf16 tie case).  cgap:
    elements between the batches of C; cpad: columns between N and C's pitch."""
    d = dict(locals())
    d['env'] = dict(env or {})
    d['opts'] = dict(opts or {})
    return d


def _ld(cols, dt):
    q = 8 if dt == 'bf16' else 4
    return (cols + q - 1) // q * q + q      # always at least one padding column


def _values(rng, n, dt, scale, ints):
    if ints:
        return rng.randint(-ints, ints + 1, n).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    if scale:
        v = v * np.exp2(rng.randint(-10, 11, n)).astype(np.float32)
    if dt == 'bf16':
        v = rne_bf16(v).astype(np.float32)
    return v


def _operand(rng, rows, cols, dt, spec, batch, bstride_extra, bcast, scale, ints):
    """One operand's storage.  shadow: finite values everywhere; read: the
    elements some logical (row, column) reads -- the GPU copy holds NaN
    everywhere else."""
    ld = _ld(cols, dt)
    spec = spec or dict(rpb=0, T=rows, t_mul=1, t_add=0, t_limit=0, perm=False)
    nb = -(-rows // spec['rpb']) if spec['rpb'] > 0 else 1
    size1 = nb * spec['T'] * ld
    sb = 0 if bcast else size1 + bstride_extra
    total = sb * (batch - 1) + size1
    shadow = _values(rng, total, dt, scale, ints)
    perm = rng.permutation(nb).astype(np.int32) if spec['perm'] else None
    off, raw = row_offsets(rows, ld, spec['T'] * ld, spec['rpb'], spec['t_mul'], spec['t_add'],
                           spec['t_limit'], perm)
    ok = off >= 0
    read = np.zeros(total, bool)
    logical = np.zeros((batch, rows, cols), np.float64)
    unmasked = np.zeros((batch, rows, ld), np.float64)     # what ignoring mask and pitch reads
    inside = (raw >= 0) & (raw + ld <= size1)
    for z in range(batch):
        idx = z * sb + off[ok][:, None] + np.arange(cols)
        read[idx] = True
        logical[z][ok] = shadow[idx]
        unmasked[z][inside] = shadow[z * sb + raw[inside][:, None] + np.arange(ld)]
    return dict(shadow=shadow, read=read, ld=ld, sb=sb, spec=spec, perm=perm, valid=ok,
                logical=logical, unmasked=unmasked, dt=dt)


class Data(object):
    pass


@functools.lru_cache(maxsize=4)      # consecutive tests share a case; the long-K ones are large
def _build_cached(name):
    return _build(CASES[name])


def build(cs):
    """The case's operands, float64 reference, S and bound (cached by name)."""
    return _build_cached(cs['name']) if CASES.get(cs['name']) is cs else _build(cs)


def _build(cs):
    rng = np.random.RandomState(cs['seed'] + 7919 * (2 * cs['at'] + cs['bt']) + cs['M'] + 3 * cs['N']
                                + 5 * cs['K'])
    M, N, K, at, bt, nz = cs['M'], cs['N'], cs['K'], cs['at'], cs['bt'], cs['batch']
    extra = {'dense': 0, 'bcast_a': 0, 'odd': 3, 'mul4': 4}[cs['bkind']]
    d = Data()
    d.cs = cs
    d.A = _operand(rng, K if at else M, M if at else K, cs['a'], cs['amap'], nz, extra,
                   cs['bkind'] == 'bcast_a', cs['scale'], cs['ints'])
    d.B = _operand(rng, K if bt else N, N if bt else K, cs['b'], cs['bmap'], nz, extra, False,
                   False, cs['ints'])
    # C: [rows through its map][N + cpad], batches cgap elements apart
    ldc = N + cs['cpad']
    cspec = cs['cmap'] or dict(rpb=0, T=M, t_mul=1, t_add=0, t_limit=0, perm=False)
    nbc = -(-M // cspec['rpb']) if cspec['rpb'] > 0 else 1
    csize = nbc * cspec['T'] * ldc
    d.ldc, d.sC, d.cspec = ldc, csize + cs['cgap'], cspec
    d.cperm = rng.permutation(nbc).astype(np.int32) if cspec['perm'] else None
    coff, _ = row_offsets(M, ldc, cspec['T'] * ldc, cspec['rpb'], cspec['t_mul'], cspec['t_add'],
                          cspec['t_limit'], d.cperm)
    d.crow_ok = coff >= 0
    d.c_total = d.sC * (nz - 1) + csize
    d.c0 = rng.standard_normal(d.c_total).astype(np.float32)
    # flat C offsets of the written elements, [batch][stored rows][N]
    d.cidx = (np.arange(nz)[:, None, None] * d.sC + coff[d.crow_ok][None, :, None]
              + np.arange(N)[None, None, :])
    if cs['ints']:
        d.bias = [rng.randint(-8, 9, N).astype(np.float32) for _ in range(cs['nbias'])]
    else:
        # (beside operands scaled up to 2^10 a bias of order 1 would vanish in the bound)
        bscale = np.float32(256.0 if cs['scale'] else 1.0)
        d.bias = [bscale * rng.standard_normal(N).astype(np.float32) for _ in range(cs['nbias'])]

    def logical(op, trans, field='logical'):
        x = op[field]
        return np.swapaxes(x, 1, 2) if trans else x
    bf = cs['cd'] == 'bf16'
    d.A_raw, d.B_raw = logical(d.A, at), logical(d.B, bt)            # [batch][M][K], [batch][N][K]
    d.A_log = rne_bf16(d.A_raw) if bf else d.A_raw
    d.B_log = rne_bf16(d.B_raw) if bf else d.B_raw
    ka = d.A['valid'] if at else np.ones(K, bool)
    kb = d.B['valid'] if bt else np.ones(K, bool)
    d.kvalid = ka & kb
    d.K_eff = int(d.kvalid.sum())
    d.ksplit = ksplit(cs)
    d.ref, d.S = evaluate(d, d.A_log, d.B_log)
    d.bound = (d.K_eff + d.ksplit + 6) * U_ACC * d.S
    if cs['c'] == 'bf16' and not cs['ints']:
        d.bound = d.bound + 2.0 ** -8 * np.abs(d.ref)
    return d


def evaluate(d, A, B, nbias=None, dtype=np.float64):
    """(alpha A B^T + beta c0 + biases, S) over the rows C's map stores, in
    `dtype` ([batch][stored rows][N])."""
    cs = d.cs
    A = A[:, d.crow_ok].astype(dtype)
    B = B.astype(dtype)
    al, be = dtype(cs['alpha']), dtype(cs['beta'])
    v = al * np.matmul(A, np.swapaxes(B, 1, 2))
    S = abs(cs['alpha']) * np.matmul(np.abs(A), np.swapaxes(np.abs(B), 1, 2)).astype(np.float64)
    for bias in d.bias[:len(d.bias) if nbias is None else nbias]:
        v = v + bias.astype(dtype)
        S = S + np.abs(bias.astype(np.float64))
    if cs['beta'] != 0.0:
        c0 = d.c0[d.cidx]
        v = v + be * c0.astype(dtype)
        S = S + abs(cs['beta']) * np.abs(c0.astype(np.float64))
    return v, S


def evaluate_f32_tiles(d, A, B):
    """The product in float32 by a plain k-ordered loop over 32-deep tiles,
    then the epilogue in float32, each step rounded."""
    cs = d.cs
    A = A[:, d.crow_ok].astype(np.float32)
    B = B.astype(np.float32)
    acc = np.zeros((A.shape[0], A.shape[1], B.shape[1]), np.float32)
    for k0 in range(0, cs['K'], 32):
        if d.kvalid[k0:k0 + 32].any():
            acc += np.matmul(A[:, :, k0:k0 + 32], np.swapaxes(B[:, :, k0:k0 + 32], 1, 2))
    v = np.float32(cs['alpha']) * acc
    for bias in d.bias:
        v = v + bias
    if cs['beta'] != 0.0:
        v = v + np.float32(cs['beta']) * d.c0[d.cidx]
    return v


def ksplit(cs):
    """Split-K slabs of the library's workspace plan for the case's shape:
    asr_gemm_workspace_bytes of the same product with bf16 operands (no staging
    copies), over the 4 M N bytes of one slab."""
    from pytorch_end2end_speech_recognition_amd import _native as NL
    g = NL.Gemm()
    g.M, g.N, g.K, g.batch = cs['M'], cs['N'], cs['K'], cs['batch']
    g.a.dtype = g.b.dtype = NL.ASR_DT_BF16
    g.c_dtype = NL.ASR_DT_BF16 if cs['c'] == 'bf16' else NL.ASR_DT_F32
    opts = NL.GemmOpts(**cs['opts']) if cs['opts'] else None
    nb = NL.query('asr_gemm_workspace_bytes', ctypes.cast(ctypes.pointer(g), ctypes.c_void_p), 1,
                  NL.ptr_struct(opts))
    one = 4 * cs['M'] * cs['N']
    return max(1, int(nb) // one) if one else 1


# -------------------------------------------- the wrong kernels of the CPU test
def mutations(d):
    """name -> wrong result on the rows C stores, for every mutation the case
    can express: (a) f32 operands truncated to bf16 in bf16 compute, (b) f32
    compute on bf16-rounded operands, (c) the last k term dropped, (d) masked
    rows and padding read as stored, (e) bias2 dropped."""
    cs = d.cs
    out = {}
    if cs['cd'] == 'bf16' and 'f32' in (cs['a'], cs['b']):
        A = trunc_bf16(d.A_raw) if cs['a'] == 'f32' else d.A_log
        B = trunc_bf16(d.B_raw) if cs['b'] == 'f32' else d.B_log
        out['a_truncated'] = evaluate(d, A, B)[0]
    if cs['cd'] == 'fp32':
        out['b_bf16_operands'] = evaluate(d, rne_bf16(d.A_raw), rne_bf16(d.B_raw))[0]
    if d.K_eff > 0:
        A = d.A_log.copy()
        A[:, :, np.nonzero(d.kvalid)[0][-1]] = 0.0
        out['c_last_k_dropped'] = evaluate(d, A, d.B_log)[0]
    rnd = rne_bf16 if cs['cd'] == 'bf16' else (lambda x: x)
    ua, ub = d.A['unmasked'], d.B['unmasked']
    Au = rnd(np.swapaxes(ua[:, :, :cs['M']], 1, 2) if cs['at'] else ua[:, :, :cs['K']])
    Bu = rnd(np.swapaxes(ub[:, :, :cs['N']], 1, 2) if cs['bt'] else ub[:, :, :cs['K']])
    if not cs['at'] and not cs['bt']:      # both k-contiguous: the first padding column is a term
        Au = np.concatenate([Au, rnd(ua[:, :, cs['K']:cs['K'] + 1])], axis=2)
        Bu = np.concatenate([Bu, rnd(ub[:, :, cs['K']:cs['K'] + 1])], axis=2)
    if Au.shape[2] != cs['K'] or not (np.array_equal(Au, d.A_log) and np.array_equal(Bu, d.B_log)):
        out['d_masked_read'] = evaluate(d, Au, Bu)[0]
    if len(d.bias) == 2:
        out['e_bias2_dropped'] = evaluate(d, d.A_log, d.B_log, nbias=1)[0]
    return out


# ---------------------------------------------------------------- the table
CASES = {}


def _add(*args, **kw):
    cs = case(*args, **kw)
    assert cs['name'] not in CASES, cs['name']
    CASES[cs['name']] = cs


def _layouts(prefix, group, fam, M, N, K, layouts=L4, **kw):
    for at, bt in layouts:
        _add('%s_%dx%dx%d_%d%d' % (prefix, M, N, K, at, bt), group, fam, M, N, K, at=at, bt=bt, **kw)


def _table():
    # --- bf16 compute, bf16 operands: the 8-wave kernels.  K = 1100 is no
    # multiple of 8, which the LDS-DMA kernels need of a k-contiguous operand,
    # so (257, 256, 1100) exists K-major x K-major only (and reduces through
    # splitk_reduce4: N % 4 == 0); (256, 257, 1104) is the split-K product with
    # an odd N in every layout (the scalar splitk_reduce)
    for ring, fam in (('1', FAM_8R), ('0', FAM_8W)):
        env = {'ASR_GEMM_8W': '1', 'ASR_GEMM_8R': ring}
        p = '8r' if ring == '1' else '8w'
        _layouts(p, '8w', fam, 256, 256, 64, env=env)
        _layouts(p, '8w', fam, 300, 260, 200, env=env)
        _layouts(p, '8w', fam, 257, 256, 1100, layouts=[(1, 1)], env=env)
        _layouts(p, '8w', fam, 256, 257, 1104, env=env)
    env = {'ASR_GEMM_KK256': '1', 'ASR_GEMM_8W': '0'}
    _layouts('kk256', 'kk256', FAM_KK256, 300, 260, 200, layouts=[(1, 1)], env=env)
    _layouts('kk256', 'kk256', FAM_KK256, 256, 256, 1100, layouts=[(1, 1)], env=env)
    # --- the 256 x 64 kernel: B k-contiguous; B K-major by n64_kmode; the
    # long-K entry (M < 4096, K >= 65536) with all but 440 of A's k rows masked
    # by t_limit, so that K_eff keeps the bound sharp
    for st in ('2', '3'):
        env = {'ASR_GEMM_N64_STAGES': st}
        _layouts('n64_s' + st, 'n64', FAM_N64, 4100, 48, 264, layouts=[(0, 0), (1, 0)], env=env)
        _layouts('n64k_s' + st, 'n64', FAM_N64, 4100, 48, 264, layouts=[(0, 1), (1, 1)], env=env,
                 opts={'n64_kmode': 1})
        _layouts('n64long_s' + st, 'n64', FAM_N64, 256, 17, 65560, layouts=[(1, 0)], env=env,
                 amap=gmap(0, 448, t_limit=440))
    # --- the 128 x 128 kernel, with the division-free staging and without
    for sf in ('1', '0'):
        env = {'ASR_GEMM_STAGEF': sf}
        _layouts('fast2_sf' + sf, 'fast2', FAM_FAST2, 130, 257, 520, env=env)
        _layouts('fast2_sf' + sf, 'fast2', FAM_FAST2, 37, 300, 136, env=env)
        # K rows through grouped maps: 5 utterances x 37 rows, frame stride 2,
        # offset 1, limit 70 (rows 35, 36 masked); and t_add = -1 (row 0 masked)
        _add('fast2_sf%s_kmap' % sf, 'fast2', FAM_FAST2, 130, 200, 185, at=1, bt=1, env=env,
             amap=gmap(37, 80, 2, 1, 70), bmap=gmap(37, 80, 2, 1, 70))
        _add('fast2_sf%s_kmap_prev' % sf, 'fast2', FAM_FAST2, 130, 200, 185, at=1, bt=1, env=env,
             amap=gmap(37, 40), bmap=gmap(37, 40, 1, -1, 40))
    # --- bf16 compute, f32 operands below the staging threshold: the generic
    # kernel converts inside its loads
    _layouts('gen_f32ops', 'gen_bf16', FAM_GEN_BF16, 70, 40, 64, a='f32', b='f32')
    _layouts('gen_mixed', 'gen_bf16', FAM_GEN_BF16, 70, 40, 64, layouts=[(0, 0), (1, 1)], b='f32')
    _layouts('gen_f32ops', 'gen_bf16', FAM_GEN_BF16, 70, 40, 203, a='f32', b='f32')
    # ... and reached by its fall-backs from bf16 operands
    _layouts('gen_bytes0', 'gen_bf16', FAM_GEN_BF16, 70, 40, 64, a_bytes0=True)
    _layouts('gen_misaligned', 'gen_bf16', FAM_GEN_BF16, 70, 40, 64, a_off=1)
    # --- in-library staging of f32 operands (2 M N K >= 3.2e7)
    _add('stage_plain', 'stage', FAM_8R, 256, 256, 256, a='f32', b='f32')
    _add('stage_rowmap_perm', 'stage', FAM_FAST2, 300, 200, 272, a='f32', b='f32',
         amap=gmap(60, 130, 2, 1, 119, perm=True))
    _add('stage_kk_ragged_k', 'stage', FAM_8R, 256, 256, 260, at=1, bt=1, a='f32', b='f32')
    _add('stage_batched', 'stage', FAM_FAST2, 128, 128, 328, a='f32', b='f32', batch=3,
         bkind='mul4')
    # --- f32 compute: the fast kernel's three tiles, split-K, mapped operands
    for st in ('2', '3'):
        kw = dict(cd='fp32', a='f32', b='f32', scale=True, env={'ASR_GEMM_F32_STAGES': st})
        for M, N, K in ((130, 140, 203), (300, 40, 198), (37, 300, 401), (192, 160, 1100)):
            _layouts('f32f_s' + st, 'f32f', FAM_F32F, M, N, K, **kw)
        _add('f32f_s%s_rmap_perm' % st, 'f32f', FAM_F32F, 135, 140, 132, amap=gmap(45, 90, 2, 1, 88, perm=True),
             **kw)
        _add('f32f_s%s_kmap_perm' % st, 'f32f', FAM_F32F, 140, 132, 135, at=1, bt=1,
             bmap=gmap(45, 90, 2, 1, 88, perm=True), **kw)
    kw = dict(cd='fp32', a='f32', b='f32', scale=True)
    _layouts('genf32_off', 'gen_f32', FAM_GEN_F32, 130, 140, 203, env={'ASR_GEMM_F32FAST': '0'}, **kw)
    _layouts('genf32_misaligned', 'gen_f32', FAM_GEN_F32, 130, 140, 203, a_off=1, **kw)
    # --- batched products.  Strides that are no multiple of 8 (bf16) / 4 (f32)
    # keep a product off the LDS-DMA kernels: the generic kernel, vec_ok cleared
    fams = (('fast2', dict(), (130, 257, 136), FAM_FAST2, FAM_GEN_BF16),
            ('genbf16', dict(a='f32', b='f32'), (70, 40, 64), FAM_GEN_BF16, FAM_GEN_BF16),
            ('f32f', dict(cd='fp32', a='f32', b='f32', scale=True), (130, 140, 203), FAM_F32F,
             FAM_GEN_F32))
    for i, (p, kw, (M, N, K), fam, fam_odd) in enumerate(fams):
        for nz in (3, 5):
            for j, (bkind, cgap) in enumerate((('dense', 0), ('bcast_a', 0), ('odd', 0), ('dense', 37))):
                at, bt = L4[(i + j + nz) % 4]
                _add('batch%d_%s_%s%s' % (nz, p, bkind, '_cgap' if cgap else ''), 'batch',
                     fam_odd if bkind == 'odd' else fam, M, N, K, at=at, bt=bt, batch=nz,
                     bkind=bkind, cgap=cgap, **kw)
    # --- epilogue: alpha, beta and both biases on one family per epilogue
    # (beta = 0 over a NaN C is every other case of this table)
    kw = dict(alpha=-1.25, beta=0.5)
    _add('epi_8r', 'epi', FAM_8R, 300, 260, 200, at=0, bt=1, **kw)
    _add('epi_fast2', 'epi', FAM_FAST2, 130, 257, 520, at=1, bt=0, **kw)
    _add('epi_n64', 'epi', FAM_N64, 4100, 48, 264, **kw)
    _add('epi_genbf16', 'epi', FAM_GEN_BF16, 70, 40, 64, a='f32', b='f32', at=1, bt=1, **kw)
    _add('epi_f32f', 'epi', FAM_F32F, 130, 140, 203, cd='fp32', a='f32', b='f32', scale=True, **kw)
    _add('epi_splitk4', 'epi', FAM_FAST2, 130, 140, 1104, cpad=0, **kw)      # splitk_reduce4
    _add('epi_splitk1', 'epi', FAM_FAST2, 130, 141, 1104, **kw)              # splitk_reduce
    _add('epi_f32f_splitk', 'epi', FAM_F32F, 192, 160, 1100, cd='fp32', a='f32', b='f32',
         scale=True, at=1, bt=0, **kw)
    # --- a row-mapped C: 4 utterances x 35 rows to frames 2 t + 1 < 66 of 70
    # (rows 33, 34 of each utterance are not stored)
    cm = gmap(35, 70, 2, 1, 66)
    _add('cmap_fast2', 'cmap', FAM_FAST2, 140, 200, 136, cmap=cm)
    _add('cmap_fast2_beta', 'cmap', FAM_FAST2, 140, 200, 136, cmap=cm, alpha=-1.25, beta=0.5)
    _add('cmap_f32f_perm', 'cmap', FAM_F32F, 140, 200, 203, cd='fp32', a='f32', b='f32',
         scale=True, cmap=gmap(35, 70, 2, 1, 66, perm=True))
    _add('cmap_splitk', 'cmap', FAM_FAST2, 140, 200, 1104, at=1, bt=1, cmap=cm)
    _add('cmap_fast2_bf16c', 'cmap', FAM_FAST2, 140, 200, 136, c='bf16', cmap=cm)
    _add('cmap_genbf16_bf16c_perm', 'cmap', FAM_GEN_BF16, 140, 40, 64, a='f32', b='f32', c='bf16',
         cmap=gmap(35, 70, 2, 1, 66, perm=True))
    # --- asr_gemm_lse_ws writes the C a plain call writes
    _add('lse_bf16', 'lse', FAM_FAST2, 300, 200, 256, nbias=1)
    _add('lse_f32', 'lse', FAM_F32F, 300, 200, 256, cd='fp32', a='f32', b='f32', scale=True, nbias=1)
    # --- bf16 C: integers whose exact results reach several hundred (ties to
    # even both ways), and real values; C's pitch is wider than N
    for p, fam, (M, N, K), r, kw in (('fast2', FAM_FAST2, (130, 257, 520), 4, {}),
                                     ('n64', FAM_N64, (4100, 48, 264), 4, {}),
                                     ('genbf16', FAM_GEN_BF16, (70, 40, 64), 8, dict(a='f32', b='f32'))):
        _add('bf16c_ties_' + p, 'bf16c_ties', fam, M, N, K, c='bf16', ints=r, cpad=8, nbias=1, **kw)
        _add('bf16c_real_' + p, 'bf16c', fam, M, N, K, c='bf16', cpad=8, **kw)


_table()


def names(*groups):
    return [n for n, cs in CASES.items() if cs['group'] in groups]
