"""The host side of the fp64 GEMM (ek_gemm.hip) without a GPU: the compact grid's map workgroup -> tile (the kernels' own
tile_of, compiled for the host), the dispatch of gemm() (gemm_plan, what gemm() itself launches by) and the argument checks
of the launch hook.  Also confirms that every product of tests/gemm_cases.py reaches the variant it states and that the
table reaches all of them, so tests/test_gpu_gemm.py cannot lose a kernel to a later change of a threshold."""
import ctypes

import numpy as np
import pytest

import gemm_cases as gc
from eigenkernel_amd import solver

_ip = ctypes.POINTER(ctypes.c_int)
BASE = 1 << 30            # an address that is never dereferenced: the plan looks at its alignment only


@pytest.fixture(scope="module")
def lib():
    return solver.load_library()


def _plan(lib, m, n, k, ta=0, tb=0, alpha=1.0, beta=0.0, a=BASE, lda=None, sa=0, b=2 * BASE, ldb=None, sb=0, c=3 * BASE,
          ldc=None, sc=0, batch=1, lower=0, staged=0, small_tiles=0, even_offs=0, offs=None, dims=None, launch=False,
          variant=True):
    """ek_hip_debug_gemm_plan (or, launch=True, _gemm_desc: only for calls its argument checks refuse) -> (rc, variant)."""
    even = lambda rows: max(2, rows + (rows & 1))          # the default leading dimensions are even
    lda = even(k if ta else m) if lda is None else lda
    ldb = even(n if tb else k) if ldb is None else ldb
    ldc = even(m) if ldc is None else ldc
    v = np.full(8, -7, dtype=np.int32)
    o = None if offs is None else np.asarray(offs, dtype=np.int64)
    d = None if dims is None else np.asarray(dims, dtype=np.int32)
    fn = lib.ek_hip_debug_gemm_desc if launch else lib.ek_hip_debug_gemm_plan
    rc = fn(ta, tb, m, n, k, alpha, beta, ctypes.c_void_p(a), lda, sa, ctypes.c_void_p(b), ldb, sb, ctypes.c_void_p(c), ldc,
            sc, batch, lower, staged, small_tiles, even_offs,
            None if o is None else o.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
            None if d is None else d.ctypes.data_as(_ip), v.ctypes.data_as(_ip) if variant else None)
    return rc, v


def _kvm(lib, *args, **kw):
    """(kernel, vec, mode) of a plan."""
    rc, v = _plan(lib, *args, **kw)
    assert rc == 0, rc
    return int(v[0]), int(v[1]), int(v[2])


# ------------------------------------------------------------------------------------------------ the compact map
def _count(T, n):
    return n * T - n * (n - 1) // 2


def _column_by_column(T):
    """The tiles on and below the diagonal of a T x T tiling, column by column: (tm, tn) as two int32 arrays."""
    tn = np.repeat(np.arange(T, dtype=np.int32), np.arange(T, 0, -1))
    start = np.arange(T, dtype=np.int64) * T - np.arange(T, dtype=np.int64) * (np.arange(T, dtype=np.int64) - 1) // 2
    tm = (np.arange(_count(T, T), dtype=np.int64) - start[tn] + tn).astype(np.int32)
    return tm, tn


@pytest.mark.parametrize("lo,hi", [(1, 120), (121, 180), (181, 220), (221, 250), (251, 275), (276, 300)])
def test_compact_map_is_one_to_one_and_column_by_column(lib, lo, hi):
    """Every tiles_m in lo..hi, every tiles_n <= tiles_m: workgroup c of the grid gemm() computes (count workgroups) is
    the c-th tile of {(tm, tn): tn <= tm < tiles_m, tn < tiles_n} taken column by column -- equality with that sequence is
    one-to-one, onto and the order at once."""
    cap = _count(hi, hi)
    tm, tn, ok = (np.empty(cap, dtype=np.int32) for _ in range(3))
    for T in range(lo, hi + 1):
        em, en = _column_by_column(T)
        assert em.min() >= 0 and em.max() == T - 1 and np.all(em >= en)
        for n in range(1, T + 1):
            cnt = _count(T, n)
            # the first cnt tiles of the column-by-column order are exactly those with tn < n
            assert en[cnt - 1] == n - 1 and (cnt == len(en) or en[cnt] == n)
            got = lib.ek_hip_debug_gemm_compact_map(T, n, 0, cnt, tm.ctypes.data_as(_ip), tn.ctypes.data_as(_ip),
                                                    ok.ctypes.data_as(_ip))
            assert got == cnt, (T, n, got)
            assert ok[:cnt].all(), (T, n)
            assert np.array_equal(tm[:cnt], em[:cnt]) and np.array_equal(tn[:cnt], en[:cnt]), (T, n)


@pytest.mark.parametrize("tile,small_tiles", [(128, 0), (64, 1)])
def test_compact_grid_size_is_the_number_of_tiles(lib, tile, small_tiles):
    """gemm()'s grid for a lower_only product of tiles_m x tiles_n tiles, tiles_n <= tiles_m <= 300, in both tilings."""
    for T in range(1, 301):
        for n in range(1, T + 1):
            rc, v = _plan(lib, tile * T - (T % 3), tile * n - (n % 5), 24, tb=1, beta=1.0, lower=1, small_tiles=small_tiles)
            assert rc == 0 and v[2] == 2 and v[3] == tile and (v[4], v[5]) == (T, n), (T, n, v)
            assert v[6] == _count(T, n) and v[7] == 1, (T, n, v)


@pytest.mark.parametrize("T", [2048, 32768])
def test_compact_map_rows_at_the_largest_orders(lib, T):
    """Whole columns at the ends and in the middle of the tilings of orders 262144 (128-tiling) and 2^21 / 2^22: the
    square root there works on numbers near 2^32 and the tile index near 2^29."""
    assert _count(T, T) < 2 ** 31
    for n in (T, T - 1, T // 3, 1):
        cnt = _count(T, n)
        for j in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
            first, rows = _count(T, j), T - j
            # the last tile of the column before, the column, the first tile of the next (where there is one)
            lo = first - (1 if j else 0)
            num = rows + (1 if j else 0) + (1 if first + rows < cnt else 0)
            tm, tn, ok = (np.empty(num, dtype=np.int32) for _ in range(3))
            got = lib.ek_hip_debug_gemm_compact_map(T, n, lo, num, tm.ctypes.data_as(_ip), tn.ctypes.data_as(_ip),
                                                    ok.ctypes.data_as(_ip))
            assert got == num and ok.all(), (T, n, j)
            c = np.arange(lo, lo + num, dtype=np.int64)
            en = np.where(c < first, j - 1, np.where(c < first + rows, j, j + 1))
            start = en * T - en * (en - 1) // 2
            assert np.array_equal(tn, en) and np.array_equal(tm, c - start + en), (T, n, j)


def test_compact_map_refuses_what_is_not_a_compact_grid(lib):
    one = np.zeros(1, dtype=np.int32)
    p = one.ctypes.data_as(_ip)
    assert lib.ek_hip_debug_gemm_compact_map(0, 1, 0, 1, p, p, p) == -1
    assert lib.ek_hip_debug_gemm_compact_map(3, 0, 0, 1, p, p, p) == -2
    assert lib.ek_hip_debug_gemm_compact_map(3, 4, 0, 1, p, p, p) == -2        # tiles_n > tiles_m: gemm() keeps mode 1
    assert lib.ek_hip_debug_gemm_compact_map(3, 3, -1, 1, p, p, p) == -3
    assert lib.ek_hip_debug_gemm_compact_map(3, 3, 0, -1, p, p, p) == -4
    assert lib.ek_hip_debug_gemm_compact_map(3, 3, 2 ** 31 - 1, 1, p, p, p) == -4
    assert lib.ek_hip_debug_gemm_compact_map(3, 3, 0, 1, None, p, p) == -5
    assert lib.ek_hip_debug_gemm_compact_map(3, 3, 0, 1, p, p, None) == 1      # valid is optional


# ------------------------------------------------------------------------------------------------ the dispatch table
S, W4, W8, RK = gc.SMALL, gc.W4, gc.W8, gc.RANKK


def test_fewer_than_256_tiles_is_the_small_kernel_and_256_is_not(lib):
    assert _kvm(lib, 1, 1, 1) == (S, 1, 0)
    assert _kvm(lib, 513, 384, 200, beta=-0.5) == (S, 1, 0)                  # the largest shape of test_dgemm_matches_numpy
    assert _kvm(lib, 1920, 2048, 37) == (S, 1, 0)                            # 15 x 16 = 240
    assert _kvm(lib, 128 * 17, 128 * 15, 37) == (S, 1, 0)                    # 255
    assert _kvm(lib, 2048, 2048, 37) == (W4, 1, 0)                           # 256
    assert _kvm(lib, 1921, 1921, 37) == (W4, 1, 0)                           # ragged: 16 x 16
    assert _kvm(lib, 2047, 1930, 16) == (W4, 1, 0)
    # the batch counts: 64 entries of 2 x 2 tiles
    assert _kvm(lib, 129, 256, 40, batch=63, sa=2 ** 20, sb=2 ** 20, sc=2 ** 20) == (S, 1, 0)
    assert _kvm(lib, 129, 256, 40, batch=64, sa=2 ** 20, sb=2 ** 20, sc=2 ** 20) == (W4, 1, 0)
    rc, v = _plan(lib, 129, 256, 40, batch=64, sa=2 ** 20, sb=2 ** 20, sc=2 ** 20)
    assert list(v[3:]) == [128, 2, 2, 4, 64]
    rc, v = _plan(lib, 129, 256, 40, batch=63, sa=2 ** 20, sb=2 ** 20, sc=2 ** 20)
    assert list(v[3:]) == [64, 3, 4, 12, 63]


def test_an_empty_product_launches_nothing(lib):
    for kw in ({"m": 0, "n": 5, "k": 5}, {"m": 5, "n": 0, "k": 5}, {"m": 5, "n": 5, "k": 5, "batch": 0}):
        rc, v = _plan(lib, **kw)
        assert rc == 0 and v[0] == -1 and v[6] == 0 and v[7] == 0
    assert _kvm(lib, 5, 5, 0, beta=1.0) == (S, 1, 0)                         # K = 0 is C <- beta C, a launch


@pytest.mark.parametrize("ta,tb", gc.TRANS)
def test_four_waves_for_beta_zero_or_long_k_eight_for_short_k_updates(lib, ta, tb):
    big = dict(ta=ta, tb=tb)
    for k in (1, 16, 512, 513, 640, 4096):
        assert _kvm(lib, 2048, 2048, k, beta=0.0, **big) == (W4, 1, 0)
    for k in (1, 15, 16, 17, 511, 512):
        for beta in (1.0, -2.0, 0.5, -0.0 + 1e-300):
            assert _kvm(lib, 2048, 2048, k, beta=beta, **big) == (W8, 1, 0)
    for k in (513, 520, 640, 8192):
        assert _kvm(lib, 2048, 2048, k, beta=1.0, **big) == (W4, 1, 0)
    assert _kvm(lib, 2048, 2048, 512, beta=-0.0, **big) == (W4, 1, 0)        # -0.0 is beta = 0


def test_rank_k_needs_the_flag_nt_and_k_from_32_to_256(lib):
    kw = dict(beta=1.0, lower=1, staged=1)
    for k in (32, 33, 64, 100, 128, 255, 256):
        assert _kvm(lib, 641, 641, k, tb=1, **kw) == (RK, 1, 2)
        assert _kvm(lib, 641, 641, k, tb=1, beta=0.0, lower=1, staged=1) == (RK, 1, 2)
    for k in (1, 31):
        assert _kvm(lib, 641, 641, k, tb=1, **kw) == (W8, 1, 2)
    assert _kvm(lib, 641, 641, 257, tb=1, **kw) == (W8, 1, 2)
    assert _kvm(lib, 641, 641, 600, tb=1, **kw) == (W4, 1, 2)
    assert _kvm(lib, 641, 641, 64, tb=1, beta=1.0, lower=1) == (W8, 1, 2)    # no flag
    for ta, tb in ((0, 0), (1, 0), (1, 1)):
        assert _kvm(lib, 641, 641, 64, ta=ta, tb=tb, **kw) == (W8, 1, 2)
    # without lower_only the small kernel comes first below 256 tiles
    assert _kvm(lib, 641, 641, 64, tb=1, beta=1.0, staged=1) == (S, 1, 0)
    assert _kvm(lib, 2048, 2048, 64, tb=1, beta=1.0, staged=1) == (RK, 1, 0)
    # its VEC is the kernel's own run-time test; the plan reports the same for one product
    assert _kvm(lib, 641, 641, 64, tb=1, lda=643, **kw) == (RK, 0, 2)
    assert _kvm(lib, 641, 641, 64, tb=1, ldb=643, **kw) == (RK, 0, 2)


def test_lower_only_keeps_the_128_tiling_unless_small_tiles_allows_the_64(lib):
    for (m, n) in ((1, 1), (64, 64), (300, 300), (700, 64), (1000, 200), (200, 500), (2100, 2100)):
        for k, beta, kern in ((24, 1.0, W8), (24, 0.0, W4), (520, 1.0, W4)):
            rc, v = _plan(lib, m, n, k, tb=1, beta=beta, lower=1)
            assert rc == 0 and v[0] == kern and v[3] == 128, (m, n, k, v)
            rc, v = _plan(lib, m, n, k, tb=1, beta=beta, lower=1, small_tiles=1)
            assert rc == 0 and v[0] == S and v[3] == 64, (m, n, k, v)
    # small_tiles means nothing without lower_only
    assert _plan(lib, 2048, 2048, 24, beta=1.0, small_tiles=1)[1][0] == W8


def test_compact_grid_only_for_one_product_without_tables_and_n_not_wider_than_m(lib):
    kw = dict(tb=1, beta=1.0, lower=1)
    z3 = [0, 0, 0]
    for st in (0, 1):
        t = 64 if st else 128
        assert _kvm(lib, 300, 300, 24, small_tiles=st, **kw)[2] == 2
        assert _kvm(lib, 700, 64, 24, small_tiles=st, **kw)[2] == 2
        assert _kvm(lib, 3 * t, 3 * t + 1, 24, small_tiles=st, **kw)[2] == 1          # 3 x 4 tiles
        assert _kvm(lib, 3 * t + 1, 4 * t, 24, small_tiles=st, **kw)[2] == 2          # 4 x 4
        assert _kvm(lib, 200, 500, 24, small_tiles=st, **kw)[2] == 1
        assert _kvm(lib, 300, 300, 24, small_tiles=st, batch=3, sa=10 ** 6, sb=10 ** 6, sc=10 ** 6, **kw)[2] == 1
        assert _kvm(lib, 300, 300, 24, small_tiles=st, offs=z3, **kw)[2] == 1
        assert _kvm(lib, 300, 300, 24, small_tiles=st, dims=[300, 300, 24], **kw)[2] == 1
        assert _kvm(lib, 300, 300, 24, small_tiles=st, tb=1, beta=1.0)[2] == 0
    rc, v = _plan(lib, 200, 500, 24, **kw)
    assert list(v[4:]) == [2, 4, 8, 1]                                                # mode 1: the whole grid


def test_vec_needs_even_leading_dimensions_aligned_bases_even_strides_and_promised_offsets(lib):
    for m, n, k, beta, kern in ((300, 200, 40, 1.0, S), (2048, 2048, 40, 0.0, W4), (2048, 2048, 40, 1.0, W8)):
        kw = dict(beta=beta)
        assert _kvm(lib, m, n, k, **kw) == (kern, 1, 0)
        assert _kvm(lib, m, n, k, lda=m + 2, ldb=k + 2, **kw) == (kern, 1, 0)
        assert _kvm(lib, m, n, k, lda=m + 1, **kw) == (kern, 0, 0)
        assert _kvm(lib, m, n, k, ldb=k + 1, **kw) == (kern, 0, 0)
        assert _kvm(lib, m, n, k, ldc=m + 1, **kw) == (kern, 1, 0)                    # C is stored by elements
        assert _kvm(lib, m, n, k, a=BASE + 8, **kw) == (kern, 0, 0)
        assert _kvm(lib, m, n, k, b=2 * BASE + 8, **kw) == (kern, 0, 0)
        assert _kvm(lib, m, n, k, c=3 * BASE + 8, **kw) == (kern, 1, 0)
        assert _kvm(lib, m, n, k, a=BASE + 16, b=2 * BASE + 48, **kw) == (kern, 1, 0)
    big = 2 ** 24
    for sa, sb, vec in ((big, big, 1), (big + 1, big, 0), (big, big + 1, 0), (0, 0, 1), (big + 2, big + 6, 1)):
        assert _kvm(lib, 129, 256, 40, batch=64, sa=sa, sb=sb, sc=big + 1) == (W4, vec, 0)
    assert _kvm(lib, 129, 256, 40, batch=1, sa=big + 1, sb=big + 1, sc=big) == (S, 1, 0)   # one entry: strides unused
    offs = [0, 2, 1, 4, 6, 3]
    assert _kvm(lib, 128, 130, 129, batch=2, offs=offs) == (S, 0, 0)
    assert _kvm(lib, 128, 130, 129, batch=2, offs=offs, even_offs=1) == (S, 1, 0)
    assert _kvm(lib, 128, 130, 129, batch=2, dims=[1, 1, 1, 2, 2, 2]) == (S, 1, 0)       # dims alone do not move operands
    assert _kvm(lib, 128, 130, 129, batch=132, offs=[0] * 396) == (W4, 0, 0)
    assert _kvm(lib, 128, 130, 129, batch=132, offs=[0] * 396, even_offs=1, beta=1.0) == (W8, 1, 0)


# ------------------------------------------------------------------------------------------------ the GPU module's table
def test_every_case_of_the_gpu_table_reaches_the_variant_it_states(lib):
    for c in gc.CASES:
        rc, v = gc.call(lib, False, c, BASE, BASE if c.gram else 2 * BASE, 3 * BASE)
        assert rc == 0, (c, rc)
        assert (int(v[0]), int(v[1]), int(v[2])) == c.expect, (c, v)
        assert v[7] == c.batch


def test_the_gpu_table_reaches_every_instantiation_in_every_lower_only_mode(lib):
    reached = {gc.variant_of(c) for c in gc.CASES}
    missing = gc.all_variants() - reached
    assert not missing, sorted(missing)
    assert reached == gc.all_variants()
    kernels = {v[:4] for v in reached if v[0] != gc.RANKK} | {(gc.RANKK,)}
    assert len(kernels) == 3 * 4 * 2 + 1       # the instantiations in ek_gemm.hip: 8 + 8 + 8 templates and the rank-k kernel


def test_the_gpu_table_keeps_to_exact_arithmetic_and_to_its_allocations():
    """|operand| <= 7, |C| <= 1000, K <= 640, |alpha|, |beta| <= 2: every partial sum is an integer or a half integer
    below 2^16, whatever the order of summation.  Every entry of a batch lies strictly inside its allocation."""
    assert 2 * 7 * 7 * 640 + 2 * 1000 < 2 ** 16
    assert set(gc.ALPHAS) == {1.0, -1.0, 2.0, -0.5} and set(gc.BETAS) == {0.0, 1.0, -2.0, 0.5}
    for c in gc.CASES:
        assert 0 <= c.k <= 640
        if c.data == "int":
            assert c.alpha in gc.ALPHAS and c.beta in gc.BETAS
        else:
            assert abs(c.alpha) <= 1 and abs(c.beta) <= 1
        A, B, C = gc.layout(c)
        for op, back in ((A, 33), (B, 33), (C, 2)):
            assert op.ld > op.rows and op.front >= 2 * op.ld
            spans = []
            for e in range(c.batch):
                lo = gc.entry_offset(op, e)
                hi = lo + op.ld * op.cols
                assert lo >= 2 * op.ld and hi + back * op.ld <= op.total, (c, e)
                spans.append((lo, hi))
            if op is C:                                   # no two entries of C overlap
                spans.sort()
                assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)), c
        if c.tables == "even":
            assert all(o % 2 == 0 for o in A.offs + B.offs)
        if c.tables == "odd":
            assert any(o % 2 for o in A.offs) and any(o % 2 for o in B.offs)
        if not c.scalar and not c.tables:
            assert A.ld % 2 == 0 and B.ld % 2 == 0 and A.front % 2 == 0 and B.front % 2 == 0
            assert A.stride % 2 == 0 and B.stride % 2 == 0


# ------------------------------------------------------------------------------------------------ argument errors
def test_launch_hook_refuses_bad_arguments_before_any_device_work(lib):
    """ek_hip_debug_gemm_desc: info = -k for the k-th argument, decided on the host (this process has no GPU context);
    the plan entry answers the same."""
    for launch in (True, False):
        bad = lambda *a, **kw: _plan(lib, *a, launch=launch, **kw)[0]
        assert bad(4, 4, 4, ta=2) == -1
        assert bad(4, 4, 4, tb=-1) == -2
        assert bad(-1, 4, 4) == -3
        assert bad(4, -1, 4) == -4
        assert bad(4, 4, -1) == -5
        assert bad(4, 4, 4, a=0) == -8
        assert bad(5, 4, 3, lda=4) == -9
        assert bad(5, 4, 3, ta=1, lda=2) == -9
        assert bad(5, 4, 3, lda=0) == -9
        assert bad(4, 4, 4, b=0) == -11
        assert bad(5, 4, 3, ldb=2) == -12
        assert bad(5, 4, 3, tb=1, ldb=3) == -12
        assert bad(4, 4, 4, c=0) == -14
        assert bad(5, 4, 3, ldc=4) == -15
        assert bad(4, 4, 4, batch=-1) == -17
        assert bad(4, 4, 4, lower=2) == -18
        assert bad(4, 4, 4, staged=2) == -19
        assert bad(4, 4, 4, small_tiles=-1) == -20
        assert bad(4, 4, 4, even_offs=3) == -21
        assert bad(4, 4, 4, batch=2, offs=[0, 0, 0, 2, 1, 0], even_offs=1) == -21   # a broken promise
        assert bad(4, 4, 4, batch=2, offs=[0, 0, 0, 2, -2, 0]) == -22
        assert bad(4, 4, 4, batch=2, dims=[4, 4, 4, 5, 4, 4]) == -23
        assert bad(4, 4, 4, batch=2, dims=[4, 4, 4, 4, 4, -1]) == -23
        assert bad(4, 4, 4, variant=False) == -24
    # legal: an odd offset of C under even_offs, and null operands where nothing reads them
    assert _plan(lib, 4, 4, 4, batch=2, offs=[0, 0, 1, 2, 2, 3], even_offs=1)[0] == 0
    assert _plan(lib, 4, 4, 0, a=0, b=0, beta=1.0)[0] == 0
    assert _plan(lib, 0, 4, 4, a=0, b=0, c=0)[0] == 0
