"""The divide & conquer stage (ek_stedc.hip) on hard tridiagonals, in every storage form, through ek_hip_debug_stedc.

Inputs: the 17 classes of tests/stedc_cases.py.  Bounds: those of test_gpu_path.py::test_stedc_matches_oracle, with
scale = max|T|:
    |w - w_oracle| <= 4 n eps scale      max|T Z - Z w| <= 32 n eps scale      max|Z^T Z - I| <= 32 n eps
w ascending, info == 0.  w_oracle is oracle.stedc's, run here up to order 515 and read from tests/golden/ at 1100 and 2100
(tests/test_stedc_cases_host.py holds that file to the oracle); the same host file shows the oracle alone a factor of 17
inside each bound.  Every merge's record {off, n1, n, k, nrot, k1} comes back with the result, so a test can tell which
branch of the deflation it ran.  Every test prints its figures before it asserts (pytest -s shows them).

Measured on an MI355X.  Top merge (deflated, nrot, k), next to the numpy replay on the oracle's halves where they differ:
    class             n = 1100                                n = 2100
    graded_down/up    477, 1, 623                             928, 6, 1172
    clement           550, 550, 550                           1050, 1050, 1050
    legendre          0, 0, 1100                              0, 0, 2100
    laguerre          160, 0, 940                             332, 0, 1768
    wilkinson_glued   615, 196, 485 (replay 618, 186, 482)    1586, 767, 514 (replay 1585, 758, 515)
    cluster_eps, zero_at_splits, tiny_at_splits: everything deflates (k = 0)
    negative_e        959, 1, 141                             1951, 3, 149
    mixed_sign_e      951, 2, 149                             1953, 1, 147
    huge              954, 2, 146                             1952, 1, 148
    tiny              953, 4, 147                             1944, 3, 156
    large_e           253, 5, 847                             773, 7, 1327
    repeated_blocks   1084, 0, 16                             2084, 0, 16
    localized         1096, 0, 4                              2096, 0, 4
    one_big           597, 226, 503 (replay 596, 225, 504)    1242, 530, 858 (replay 1242, 529, 858)
Worst ratios (eigenvalues, residual, orthogonality; units of n eps): full form 0.55, 0.55, 0.50 (all at order 2; from
order 259 on 0.08, 0.06, 0.12); windows 0.23 and 0.38 (select), 0.14 and 0.17 (compact); a cell's share and the
assembled basis 0.02 and 0.05.  Every selected column and every eigenvalue had the full form's bits.
"""
import numpy as np
import pytest

import stedc_cases as sc

pytestmark = pytest.mark.gpu
EPS = sc.EPS

FULL_ORDERS = (2, 33, 65, 66, 130, 259, 515, 1100, 2100)
WINDOW_ORDERS = (20, 66, 259, 1100)
WINDOW_CLASSES = ("wilkinson_glued", "clement", "cluster_eps", "laguerre", "mixed_sign_e", "tiny_at_splits")
GRIDS = ((259, 16, 3), (1100, 64, 4), (1100, 128, 2))
GRID_CLASSES = ("wilkinson_glued", "clement", "one_big")

_ORACLE_W = {}
_FULL = {}


def _oracle_w(oracle, name, n):
    """the reference eigenvalues, computed (or read) once per case"""
    if (name, n) not in _ORACLE_W:
        if n in sc.RECORDED_ORDERS:
            w = sc.recorded_spectrum(name, n)
        else:
            w = oracle.stedc(*sc.tridiagonal(name, n))[0]
        w.setflags(write=False)
        _ORACLE_W[(name, n)] = w
    return _ORACLE_W[(name, n)]


def _full(hip, name, n):
    """the full form's (w, Z, info, merges) of a case the selecting forms are compared with: one GPU call per case"""
    if (name, n) not in _FULL:
        w, Z, info, merges = hip.stedc_select(*sc.tridiagonal(name, n))
        for a in (w, Z, merges):
            a.setflags(write=False)
        _FULL[(name, n)] = (w, Z, info, merges)
    return _FULL[(name, n)]


def _plan(n):
    """the merges of order n as (off, n1, n), height by height, the top merge last (Plan::height of ek_stedc.hip)"""
    levels = []

    def height(off, m):
        if m <= sc.LEAF:
            return 0
        m1 = m // 2
        h = max(height(off, m1), height(off + m1, m - m1)) + 1
        while len(levels) < h:
            levels.append([])
        levels[h - 1].append((off, m1, m))
        return h

    height(0, n)
    return [m for lv in levels for m in lv]


def _check_records(n, merges):
    plan = _plan(n)
    assert merges.shape == (len(plan), 6)
    for (off, n1, m), rec in zip(plan, merges):
        assert tuple(rec[:3]) == (off, n1, m)
        k, nrot, k1 = int(rec[3]), int(rec[4]), int(rec[5])
        assert 0 <= k <= m and 0 <= nrot <= m - k, rec
        assert (k1 == -1) if nrot > 0 else (0 <= k1 <= min(k, n1)), rec
    if plan:
        assert tuple(merges[-1][:3]) == (0, n // 2, n)


def _ratios(d, e, w_cols, Z):
    """(residual, orthogonality) of the columns Z with eigenvalues w_cols, in units of n eps scale and n eps"""
    n = len(d)
    scale = sc.scale_of(d, e)
    res = np.abs(sc.apply_tridiagonal(d, e, Z) - Z * w_cols).max() / (n * EPS * scale) if Z.shape[1] else 0.0
    orth = np.abs(Z.T @ Z - np.eye(Z.shape[1])).max() / (n * EPS) if Z.shape[1] else 0.0
    return float(res), float(orth)


def _same_bits(tag, got, want):
    """np.array_equal with a report of how far apart the arrays are when they are not"""
    same = np.array_equal(got, want)
    if not same:
        diff = np.abs(got - want)
        bad = np.flatnonzero(diff.reshape(diff.shape[0], -1).max(axis=0) > 0) if diff.ndim == 2 else np.flatnonzero(diff)
        print("stedc bits DIFFER %s: %d columns/entries, first %s, max|diff| %.3e" % (tag, bad.size, bad[:8], diff.max()))
    return same


# ------------------------------------------------------------------------------------------------ the full form
@pytest.mark.parametrize("n", FULL_ORDERS)
@pytest.mark.parametrize("name", sc.CLASSES)
def test_full_form_every_class(hip, oracle, name, n):
    """orders: a single leaf pair (2), odd n1 and odd off (33, 65, 259, 515), tree heights 1 to 7, and top merges of more
    than one and more than two 1024-pole chunks of the sequential scan (1100, 2100)"""
    d, e = sc.tridiagonal(name, n)
    w_or = _oracle_w(oracle, name, n)
    if n <= 1100:
        w, Z, info, merges = _full(hip, name, n)
    else:
        w, Z, info, merges = hip.stedc_select(d, e)
    scale = sc.scale_of(d, e)
    r_w = float(np.abs(w - w_or).max() / (n * EPS * scale))
    r_res, r_orth = _ratios(d, e, w, Z)
    top = tuple(int(v) for v in merges[-1]) if len(merges) else None
    print("stedc full %s n=%d: w %.3f res %.3f orth %.3f (n eps); top merge (deflated, nrot, k) = %s"
          % (name, n, r_w, r_res, r_orth, (n - top[3], top[4], top[3]) if top else None))
    assert info == 0
    assert Z.shape == (n, n) and np.all(np.diff(w) >= 0)
    assert r_w <= sc.BOUND_W
    assert r_res <= sc.BOUND_RES
    assert r_orth <= sc.BOUND_ORTH
    _check_records(n, merges)
    if name == "clement":
        assert np.abs(w - sc.exact_spectrum(name, n)).max() <= 4 * n * EPS * (n - 1)
    if name == "repeated_blocks":
        assert np.abs(w - sc.exact_spectrum(name, n)).max() <= 4 * n * EPS * 4
    if n <= 515:
        # the entry's full form is the stage entry's: same kernels, same launches, same bits
        w0, Z0, info0 = hip.stedc(d, e)
        assert info0 == 0 and np.array_equal(w0, w) and np.array_equal(Z0, Z)


@pytest.mark.parametrize("n", [1100, 2100])
def test_top_merge_takes_the_intended_path(hip, n):
    """what keeps the tests above from passing on the wrong branch: the top merge's record"""
    top = {}
    for name in ("clement", "wilkinson_glued", "one_big", "legendre", "laguerre", "cluster_eps", "zero_at_splits"):
        merges = _full(hip, name, n)[3] if n <= 1100 else hip.stedc_select(*sc.tridiagonal(name, n))[3]
        top[name] = tuple(int(v) for v in merges[-1][3:])
        print("stedc path %s n=%d: k %d nrot %d k1 %d" % ((name, n) + top[name]))
    assert top["clement"][1] >= 0.4 * n                              # the sequential scan, every pole rotated
    for name in ("wilkinson_glued", "one_big"):                      # the sequential scan, mixed
        assert top[name][1] >= 50 and top[name][0] >= 100, name
    assert top["legendre"][1] == 0 and top["legendre"][0] >= 0.9 * n  # the fast path, full-size secular equation + GEMM
    assert top["laguerre"][1] == 0                                   # the fast path with tiny-z deflation
    assert 0 < top["laguerre"][0] < n
    for name in ("cluster_eps", "zero_at_splits"):                   # the all-deflate branch
        assert top[name][0] == 0 and top[name][1] == 0, name


# ------------------------------------------------------------------------------------------------ the selecting forms
def _window_pairs(n):
    h2 = n - n // 2
    return ((1, 0), (1, n - 1), (h2, 0), (h2, n - h2), (h2 + 1, 0), (n - 1, 1), (7, n // 2 - 3))


def _check_selection(hip, name, n, nsel, first, nb, npcol, mycol, tag):
    """one selecting call against the full form of the same case; returns (ranks, Z, bits held)"""
    d, e = sc.tridiagonal(name, n)
    wf, Zf, _, mf = _full(hip, name, n)
    w, Z, info, merges = hip.stedc_select(d, e, nsel=nsel, first=first, nb=nb, npcol=npcol, mycol=mycol)
    ranks = sc.sel_rank(np.arange(nsel), first, nb, npcol, mycol)
    r_res, r_orth = _ratios(d, e, w[ranks], Z)
    compact = hip.stedc_zcols(n, nsel) != n
    print("stedc %s %s n=%d nsel=%d first=%d %s: res %.3f orth %.3f (n eps)"
          % (tag, name, n, nsel, first, "compact" if compact else "select", r_res, r_orth))
    assert info == 0
    assert Z.shape == (n, nsel) and w.shape == (n,)
    assert compact == (n > 32 and nsel <= n - n // 2) == sc.is_compact(n, nsel)
    assert r_res <= sc.BOUND_RES
    assert r_orth <= sc.BOUND_ORTH
    # the deflation does not know about the selection: the same records
    assert np.array_equal(merges, mf)
    bits = _same_bits("%s %s n=%d nsel=%d first=%d w" % (tag, name, n, nsel, first), w, wf)
    bits = _same_bits("%s %s n=%d nsel=%d first=%d Z" % (tag, name, n, nsel, first), Z, Zf[:, ranks]) and bits
    return ranks, Z, bits


@pytest.mark.parametrize("n", WINDOW_ORDERS)
@pytest.mark.parametrize("name", WINDOW_CLASSES)
def test_window_on_a_1x1_grid(hip, name, n):
    """nb = n, npcol = 1: the lowest and the highest pair, both compact halves, the first non-compact selection, all but
    one, and seven pairs across the middle (inside clement's rotated pairs and wilkinson_glued's clusters); order 20 is
    a single leaf (the gather path)"""
    held = True
    for nsel, first in _window_pairs(n):
        held = _check_selection(hip, name, n, nsel, first, n, 1, 0, "window")[2] and held
    assert held, "a selected column or an eigenvalue differs from the full form's in some bit"


@pytest.mark.parametrize("name", GRID_CLASSES)
@pytest.mark.parametrize("n,nb,npcol", GRIDS)
def test_grid_cells_share_one_basis(hip, name, n, nb, npcol):
    """every cell of a process row solves on its own and forms its block-cyclic share of the columns; scattered back by
    rank the shares must be ONE orthogonal basis that diagonalises T -- inside clusters and rotated pairs too"""
    d, e = sc.tridiagonal(name, n)
    wf = _full(hip, name, n)[0]
    Zs = np.full((n, n), np.nan)
    held = True
    for mycol in range(npcol):
        nsel = sc.numroc(n, nb, mycol, npcol)
        ranks, Z, bits = _check_selection(hip, name, n, nsel, 0, nb, npcol, mycol, "cell %d/%d" % (mycol, npcol))
        assert np.isnan(Zs[:, ranks]).all()
        Zs[:, ranks] = Z
        held = held and bits
    assert np.isfinite(Zs).all()
    r_res, r_orth = _ratios(d, e, wf, Zs)
    print("stedc grid %s n=%d nb=%d npcol=%d assembled: res %.3f orth %.3f (n eps)" % (name, n, nb, npcol, r_res, r_orth))
    assert r_res <= sc.BOUND_RES
    assert r_orth <= sc.BOUND_ORTH
    assert held, "a cell's column or an eigenvalue differs from the full form's in some bit"


@pytest.mark.parametrize("name,n", [("repeated_blocks", 259), ("localized", 260), ("graded_down", 260),
                                    ("graded_down", 516)])
def test_odd_count_of_top_only_survivors(hip, oracle, name, n):
    """the second product of a merge starts on an even column: with an odd number k1 of top-only survivors it takes the
    last of them along (k1e = k1 & ~1 != k1).  The top merge of these cases has an odd k1 -- predicted by the replay of
    the scan on the oracle's halves, read back from the stage's record -- at n1 odd (259) and even (260, 516: the
    aligned loads of the product); all three forms must stay correct and agree"""
    d, e = sc.tridiagonal(name, n)
    (d1, e1), (d2, e2) = sc.split_halves(d, e)
    (_, nrot_cpu, k_cpu), (k1_cpu, _, _) = sc.top_merge_counts(d, e, (oracle.stedc(d1, e1), oracle.stedc(d2, e2)), types=True)
    w, Z, info, merges = _full(hip, name, n)
    k, nrot, k1 = (int(v) for v in merges[-1][3:])
    odd_below = sum(1 for r in merges[:-1] if r[5] >= 0 and r[5] % 2 == 1 and r[0] % 2 == 0 and r[1] % 2 == 0)
    print("stedc odd-k1 %s n=%d: top merge k %d nrot %d k1 %d (replay: k %d nrot %d k1 %d); %d lower merges with odd k1 "
          "at even off and n1" % (name, n, k, nrot, k1, k_cpu, nrot_cpu, k1_cpu, odd_below))
    assert info == 0
    assert nrot_cpu == 0 and k1_cpu % 2 == 1
    assert nrot == 0 and k1 % 2 == 1 and (k1 & ~1) != k1
    r_w = np.abs(w - _oracle_w(oracle, name, n)).max() / (n * EPS * sc.scale_of(d, e))
    r_res, r_orth = _ratios(d, e, w, Z)
    assert r_w <= sc.BOUND_W and r_res <= sc.BOUND_RES and r_orth <= sc.BOUND_ORTH
    h2 = n - n // 2
    held = True
    for nsel, first in ((h2, 0), (h2 + 1, n - h2 - 1), (7, n // 2 - 3)):
        held = _check_selection(hip, name, n, nsel, first, n, 1, 0, "odd-k1")[2] and held
    assert held, "a selected column or an eigenvalue differs from the full form's in some bit"


def test_repeat_calls_leak_nothing(hip):
    """the cached plan and the workspace are reused from call to call: 1100, then 66, then 1100 again, every call in
    another form, must give the bits of the first calls"""
    name = "wilkinson_glued"
    big, small = sc.tridiagonal(name, 1100), sc.tridiagonal(name, 66)
    h2 = 550
    a1 = hip.stedc_select(*big)
    s1 = hip.stedc_select(*small, nsel=20, first=5)                   # compact
    b = hip.stedc_select(*big, nsel=h2 + 1, first=3)                  # select: Z doubles as the scratch
    s2 = hip.stedc_select(*small)                                     # full
    c = hip.stedc_select(*big, nsel=300, first=400)                   # compact
    s3 = hip.stedc_select(*small, nsel=40, first=26)                  # select
    a2 = hip.stedc_select(*big)
    b2 = hip.stedc_select(*big, nsel=h2 + 1, first=3)
    c2 = hip.stedc_select(*big, nsel=300, first=400)
    for r in (a1, s1, b, s2, c, s3, a2, b2, c2):
        assert r[2] == 0
    # like with like: the same call before and after the others
    for x, y in ((a1, a2), (b, b2), (c, c2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[3], y[3])
    for r in (b, c, a2):
        assert np.array_equal(r[0], a1[0]) and np.array_equal(r[3], a1[3])
    for r in (s1, s3):
        assert np.array_equal(r[0], s2[0]) and np.array_equal(r[3], s2[3])
    # ... and across the forms
    held = _same_bits("repeat 1100 select", b[1], a1[1][:, 3:3 + h2 + 1])
    held = _same_bits("repeat 1100 compact", c[1], a1[1][:, 400:700]) and held
    held = _same_bits("repeat 66 compact", s1[1], s2[1][:, 5:25]) and held
    held = _same_bits("repeat 66 select", s3[1], s2[1][:, 26:66]) and held
    assert held
