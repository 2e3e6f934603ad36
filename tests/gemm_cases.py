"""The table of products tests/test_gpu_gemm.py runs through ek_hip_debug_gemm_desc, one launch per Case, and the layout of
their operands in memory: plain data and arithmetic, no fixtures, no GPU.  tests/test_gemm_host.py confirms on the CPU
(ek_hip_debug_gemm_plan) that every Case reaches the variant it states, and that the table as a whole reaches every one.

A variant is (kernel, ta, tb, vec, mode): kernel 0 gemm_small_kernel, 1 gemm_kernel (4 waves), 2 gemm_kernel_w8 (8 waves),
3 gemm_rankk_kernel; vec 1 the 16-byte instantiation; mode lower_only as launched (0, 1 whole grid, 2 compact grid).

Layout.  An operand stored as rows x cols lies strictly inside an allocation of its own: `front` doubles in front of its
base, leading dimension ld > rows, `back` doubles behind its last column; a batch by strides has a gap between the
entries.  Everything that is not an entry of the operand is NaN.  front is at least two columns, back at least 33 columns
for A and B: a K walk that runs past K by less than a slab (16, or 32 in the 64-tiling), or a row past M, reads NaN and
poisons the result, it never leaves the allocation."""
from collections import namedtuple

import numpy as np

SMALL, W4, W8, RANKK = 0, 1, 2, 3
KERNEL_NAMES = ("small", "4-wave", "8-wave", "rank-k")
ALPHAS = (1.0, -1.0, 2.0, -0.5)
BETAS = (0.0, 1.0, -2.0, 0.5)
TRANS = ((0, 0), (0, 1), (1, 0), (1, 1))
SCALAR_WAYS = ("lda", "ldb", "base")          # how a scalar (non-VEC) instantiation is forced
# per-entry {M, N, K} of the table-driven batches (the D&C and ORMTR forms); host M, N, K = 128, 130, 129
TABLE_ENTRIES = ((0, 0, 0), (70, 1, 129), (128, 128, 16), (1, 130, 5), (97, 64, 0), (127, 129, 31))

_FIELDS = ("key ta tb m n k alpha beta batch lower staged small_tiles scalar tables entries data share_ab gram expect")
Case = namedtuple("Case", _FIELDS)
Case.__doc__ = """key: the pytest case it runs in; scalar: '' (VEC) or how VEC is switched off ('lda', 'ldb': odd leading
dimension; 'base': a base 8 mod 16; 'stride': odd batch stride); tables: '' / 'even' (even offsets and even_offs) / 'odd'
(odd offsets, no promise); entries: per-entry (M, N, K) with tables; data: 'int' (exact), 'uniform', 'identity' (A = I,
B = arange); share_ab: A and B with stride 0; gram: B is A's pointer and offsets; expect: (kernel, vec, mode)."""


def case(key, ta, tb, m, n, k, alpha, beta, expect, batch=1, lower=0, staged=0, small_tiles=0, scalar="", tables="",
         entries=(), data="int", share_ab=False, gram=False):
    return Case(key, ta, tb, m, n, k, alpha, beta, batch, lower, staged, small_tiles, scalar, tables, tuple(entries), data,
                share_ab, gram, tuple(expect))


def variant_of(c):
    return (c.expect[0], c.ta, c.tb, c.expect[1], c.expect[2])


def all_variants():
    """Every kernel gemm() can launch x the lower_only modes: 3 templates x 4 transposes x {VEC, scalar} = 24
    instantiations and the rank-k kernel (NT only; its VEC is a run-time branch, counted as two here)."""
    out = set()
    for kern in (SMALL, W4, W8):
        for ta, tb in TRANS:
            for vec in (0, 1):
                for mode in (0, 1, 2):
                    out.add((kern, ta, tb, vec, mode))
    for vec in (0, 1):
        for mode in (0, 1, 2):
            out.add((RANKK, 0, 1, vec, mode))
    return out


# ------------------------------------------------------------------------------------------------------ the table
def _ab(i):
    """alpha and beta of the i-th launch of a group: every pair comes up."""
    return ALPHAS[i % 4], BETAS[(i // 4 + i) % 4]


def _nonzero_beta(i):
    return BETAS[1 + i % 3]


def _ways(i, full):
    """'' (VEC) and the scalar ways: all three, or one in rotation."""
    return ("",) + (SCALAR_WAYS if full else (SCALAR_WAYS[i % 3],))


def build():
    T = []
    i = 0
    # --- gemm_small_kernel: fewer than 256 tiles of 128 x 128
    for (m, n, k) in ((1, 1, 1), (63, 65, 31), (64, 64, 32), (129, 70, 33), (300, 5, 129), (70, 33, 0)):
        for ta, tb in TRANS:
            for way in _ways(i, True):
                alpha, beta = _ab(i)
                if k == 0:
                    beta = _nonzero_beta(i)          # C <- beta C
                T.append(case("small-%dx%dx%d" % (m, n, k), ta, tb, m, n, k, alpha, beta, (SMALL, int(not way), 0),
                              scalar=way))
                i += 1
    # --- gemm_kernel (4 waves): 256 tiles or more with beta = 0, or K > 512
    for (m, n, k) in ((1921, 1921, 37), (2047, 1930, 16)):
        for ta, tb in TRANS:
            for way in _ways(i, True):
                T.append(case("w4-%dx%dx%d-%d%d" % (m, n, k, ta, tb), ta, tb, m, n, k, ALPHAS[i % 4], 0.0,
                              (W4, int(not way), 0), scalar=way))
                i += 1
    for ta, tb in TRANS:
        for way in _ways(i, True):
            T.append(case("w4-257x130x520-lower", ta, tb, 257, 130, 520, ALPHAS[i % 4], 1.0, (W4, int(not way), 2),
                          lower=1, scalar=way))
            i += 1
    for ta, tb in TRANS:
        for way in _ways(i, True):
            T.append(case("w4-batch64-129x256x40-%d%d" % (ta, tb), ta, tb, 129, 256, 40, ALPHAS[i % 4], 0.0,
                          (W4, int(not way), 0), batch=64, scalar=way))
            i += 1
    # --- gemm_kernel_w8 (8 waves): K <= 512 and beta != 0
    for k in (1, 15, 16, 17, 512):
        for (m, n) in ((1921, 1921), (2047, 1930)):
            for ta, tb in TRANS:
                for way in _ways(i, False):
                    T.append(case("w8-%dx%dx%d-%d%d" % (m, n, k, ta, tb), ta, tb, m, n, k, ALPHAS[i % 4], _nonzero_beta(i),
                                  (W8, int(not way), 0), scalar=way))
                    i += 1
        for ta, tb in TRANS:
            for way in _ways(i, True):
                T.append(case("w8-257x130x%d-lower" % k, ta, tb, 257, 130, k, ALPHAS[i % 4], _nonzero_beta(i),
                              (W8, int(not way), 2), lower=1, scalar=way))
                i += 1
        for ta, tb in TRANS:
            for way in _ways(i, False):
                T.append(case("w8-batch64-129x256x%d" % k, ta, tb, 129, 256, k, ALPHAS[i % 4], _nonzero_beta(i),
                              (W8, int(not way), 0), batch=64, scalar=way))
                i += 1
    # --- gemm_rankk_kernel: staged_rank_k, NT, 32 <= K <= 256; lower_only on the compact grid; beta = 1 and beta = 0
    for mn in (128, 300, 641):
        for k in (32, 33, 64, 100, 128, 256):
            for beta in (1.0, 0.0):
                for way in ("", "lda" if (i // 2) % 2 == 0 else "ldb"):
                    T.append(case("rankk-%d" % mn, 0, 1, mn, mn, k, ALPHAS[i % 4], beta, (RANKK, int(not way), 2), lower=1,
                                  staged=1, scalar=way))
                    i += 1
    # --- lower_only: the contract and the three grids, beta = 1 (a tile visited twice shows)
    for ta, tb in ((0, 1), (0, 0)):
        for mn in (300, 1000):
            T.append(case("lower-square", ta, tb, mn, mn, 24, -1.0, 1.0, (W8, 1, 2), lower=1))
        T.append(case("lower-square-2100-small-tiles-%d%d" % (ta, tb), ta, tb, 2100, 2100, 24, -1.0, 1.0, (SMALL, 1, 2),
                      lower=1, small_tiles=1))
        for (m, n) in ((700, 64), (1000, 200)):
            T.append(case("lower-tall", ta, tb, m, n, 24, -1.0, 1.0, (W8, 1, 2), lower=1))
            T.append(case("lower-tall", ta, tb, m, n, 24, -1.0, 1.0, (SMALL, 1, 2), lower=1, small_tiles=1))
        T.append(case("lower-wide-and-batched", ta, tb, 200, 500, 24, -1.0, 1.0, (W8, 1, 1), lower=1))
        T.append(case("lower-wide-and-batched", ta, tb, 200, 500, 24, -1.0, 1.0, (SMALL, 1, 1), lower=1, small_tiles=1))
        T.append(case("lower-wide-and-batched", ta, tb, 300, 300, 24, -1.0, 1.0, (W8, 1, 1), lower=1, batch=3))
        T.append(case("lower-wide-and-batched", ta, tb, 300, 300, 24, -1.0, 1.0, (SMALL, 1, 1), lower=1, small_tiles=1, batch=3))
    # --- every instantiation in the lower_only modes 1 (batch of 2) and 2 (one product)
    for kern, (mn, k, st) in ((SMALL, (200, 40, 1)), (W4, (300, 520, 0)), (W8, (300, 20, 0))):
        for ta, tb in TRANS:
            for way in _ways(i, False):
                for mode in (1, 2):
                    T.append(case("modes-%s" % KERNEL_NAMES[kern], ta, tb, mn, mn, k, ALPHAS[i % 4], 1.0,
                                  (kern, int(not way), mode), lower=1, small_tiles=st, batch=1 if mode == 2 else 2, scalar=way))
                    i += 1
    for way in ("", "lda"):
        # the rank-k kernel without lower_only needs 256 tiles, and with lower_only on the whole grid a batch
        T.append(case("modes-rank-k", 0, 1, 128, 128, 40, 2.0, 1.0, (RANKK, int(not way), 0), staged=1, batch=256, scalar=way))
        T.append(case("modes-rank-k", 0, 1, 300, 300, 64, -0.5, 1.0, (RANKK, int(not way), 1), staged=1, lower=1, batch=3,
                      scalar=way))
    # --- batches by tables in device memory: offsets into shared buffers, strides 0, per-entry dims
    for reps in (1, 22):                 # 6 entries x 2 tiles, and 132 x 2 = 264 >= 256 tiles
        for ta, tb in ((0, 0), (1, 0)):
            for tables in ("even", "odd"):
                for beta in (0.0, 1.0):
                    kern = SMALL if reps == 1 else (W4 if beta == 0.0 else W8)
                    T.append(case("tables-x%d" % reps, ta, tb, 128, 130, 129, ALPHAS[i % 4], beta,
                                  (kern, int(tables == "even"), 0), batch=6 * reps, tables=tables, entries=TABLE_ENTRIES * reps))
                    i += 1
    # the Gram products of the block reflectors: V^T V, A and B the same pointer, K the column height
    for batch in (8, 256):
        for tables in ("even", "odd"):
            T.append(case("tables-gram", 1, 0, 32, 32, 200, 1.0, 0.0, (SMALL if batch == 8 else W4, int(tables == "even"), 0),
                          batch=batch, tables=tables, entries=((32, 32, 200),) * batch, gram=True))
    # --- A = I, B = arange: a transposed store layout shows as such (256 entries of one tile reach the 128-tiling)
    T.append(case("asymmetry", 0, 0, 128, 128, 128, 1.0, 0.0, (W4, 1, 0), batch=256, data="identity", share_ab=True))
    T.append(case("asymmetry", 0, 1, 128, 128, 128, 1.0, 0.0, (W4, 1, 0), batch=256, data="identity", share_ab=True))
    T.append(case("asymmetry", 0, 0, 128, 128, 128, 1.0, 1.0, (W8, 1, 0), batch=256, data="identity", share_ab=True))
    T.append(case("asymmetry", 0, 1, 128, 128, 128, 1.0, 1.0, (W8, 1, 0), batch=256, data="identity", share_ab=True))
    T.append(case("asymmetry", 0, 1, 128, 128, 128, 1.0, 1.0, (RANKK, 1, 0), batch=256, staged=1, data="identity", share_ab=True))
    # --- uniform(-1, 1) against a long double product, one per kernel: accumulation precision
    T.append(case("uniform", 0, 0, 129, 70, 33, 0.75, -0.5, (SMALL, 1, 0), data="uniform"))
    T.append(case("uniform", 0, 1, 257, 130, 520, 0.75, -0.5, (W4, 1, 2), lower=1, data="uniform"))
    T.append(case("uniform", 1, 0, 257, 130, 100, 0.75, -0.5, (W8, 1, 2), lower=1, data="uniform"))
    T.append(case("uniform", 0, 1, 300, 300, 100, 0.75, -0.5, (RANKK, 1, 2), lower=1, staged=1, data="uniform"))
    return T


CASES = build()
KEYS = tuple(dict.fromkeys(c.key for c in CASES))


# ------------------------------------------------------------------------------------------------------ the layout
Operand = namedtuple("Operand", "rows cols ld stride front total offs")
Operand.__doc__ = """Stored rows x cols (of the host M, N, K), leading dimension, element stride between batch entries
(0 with tables), doubles in front of the base, doubles allocated, per-entry element offsets from the base (tables)."""


def _ld(rows, odd):
    ld = rows + 1
    return ld if (ld & 1) == int(odd) else ld + 1


def _operand(rows, cols, odd_ld, odd_base, batch, tables, back_cols, shared, odd_stride=False):
    ld = _ld(rows, odd_ld)
    front = 2 * ld + 64                            # even: the base is 16-byte aligned in an aligned allocation
    if odd_base:
        front += 1
    slot = ld * (cols + back_cols)
    slot += slot & 1                               # even
    offs = ()
    if tables:
        stride = 0
        offs = tuple(e * slot + (1 if tables == "odd" and e % 3 != 2 else 0) for e in range(batch))
        total = front + batch * slot + ld + 64
    elif shared:
        stride = 0
        total = front + slot + 64
    else:
        stride = slot + (1 if odd_stride else 0)
        total = front + batch * stride + 64
    return Operand(rows, cols, ld, stride, front, total, offs)


def layout(c):
    """(A, B, C) of a case.  With c.gram B is A (the caller passes A's pointer and offsets for both)."""
    ra, ca = (c.k, c.m) if c.ta else (c.m, c.k)
    rb, cb = (c.n, c.k) if c.tb else (c.k, c.n)
    base_a = c.scalar == "base" and (c.ta ^ c.tb) == 0
    base_b = c.scalar == "base" and (c.ta ^ c.tb) == 1
    A = _operand(ra, ca, c.scalar == "lda", base_a, c.batch, c.tables, 33, c.share_ab, c.scalar == "stride")
    B = _operand(rb, cb, c.scalar == "ldb", base_b, c.batch, c.tables, 33, c.share_ab, c.scalar == "stride")
    C = _operand(c.m, c.n, False, False, c.batch, c.tables, 2, False)
    if c.gram:
        B = A
    return A, B, C


def entry_dims(c, e):
    return c.entries[e] if c.tables else (c.m, c.n, c.k)


def entry_offset(op, e):
    """Element offset of batch entry e from the start of the allocation."""
    return op.front + (op.offs[e] if op.offs else e * op.stride)


def host_tables(c, A, B, C):
    """offs (3 * batch int64) and dims (3 * batch int32), or (None, None)."""
    if not c.tables:
        return None, None
    offs = np.array([[A.offs[e], B.offs[e], C.offs[e]] for e in range(c.batch)], dtype=np.int64).ravel()
    dims = np.array(c.entries, dtype=np.int32).ravel()
    return offs, dims


def call(lib, launch, c, pA, pB, pC):
    """ek_hip_debug_gemm_desc (launch) or _plan on the allocations at the addresses pA, pB, pC; returns (rc, variant[8])."""
    import ctypes
    A, B, C = layout(c)
    offs, dims = host_tables(c, A, B, C)
    v = np.full(8, -7, dtype=np.int32)
    fn = lib.ek_hip_debug_gemm_desc if launch else lib.ek_hip_debug_gemm_plan
    rc = fn(c.ta, c.tb, c.m, c.n, c.k, c.alpha, c.beta, ctypes.c_void_p(pA + 8 * A.front), A.ld, A.stride,
            ctypes.c_void_p(pB + 8 * B.front), B.ld, B.stride, ctypes.c_void_p(pC + 8 * C.front), C.ld, C.stride, c.batch,
            c.lower, c.staged, c.small_tiles, int(c.tables == "even"),
            None if offs is None else offs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
            None if dims is None else dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            v.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return rc, v
