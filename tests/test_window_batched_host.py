"""Host-side checks of the batched window entries (ek_hip_eigenpairs_window_batched*), no GPU needed: declared in the
boundary header, exported and bound; every argument error decided before any device work; the old batched entries accept
what they accepted; and the table of tests/window_batched_cases.py pinned against LAPACK's own windowed drivers
(scipy.linalg.eigh with driver evx / gvx): they stay inside HALF of the eigenvalue bound and a QUARTER of the residual and
orthogonality bounds (measured when the table was drawn up: 0.198, 0.021, 0.021 at most), so that the bounds the GPU test
holds the kernel to are bounds that inverse iteration can meet on these inputs; the cond_b pencils under the rule for a
stated cond(B) with LAPACK's full driver as "its own".  Every 'V' bound of the table keeps the stated gap from every
reference eigenvalue."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import window_batched_cases as wc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_eigenpairs_window_batched_device", "ek_hip_eigenpairs_window_batched")
HOOK = "ek_hip_debug_window_batched_chunk"
ORDERS = (3, 17, 30, 33, 64, 100, 128)


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return hdr, dbg, set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_window_entries_declared_exported_and_bound():
    """Fails on a tree without the feature: the symbols are the signal, ek_hip_version stays 3."""
    _, _, declared, hooks = _headers()
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in NAMES:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 23
        assert fn.argtypes[5] is ctypes.c_double and fn.argtypes[6] is ctypes.c_double
        for k in (11, 14, 20):
            assert fn.argtypes[k] is ctypes.c_longlong
    assert callable(solver.eigenpairs_window_batched)
    assert lib.ek_hip_version() == 3


def test_chunk_hook_is_a_debug_entry():
    _, _, declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    default = solver.window_batched_chunk(7)
    try:
        assert default == 1024
        assert solver.window_batched_chunk(3) == 7
    finally:
        assert solver.window_batched_chunk(0) == 3
    assert solver.window_batched_chunk(0) == 1024


@pytest.mark.parametrize("name", NAMES)
def test_window_argument_errors_without_gpu(name):
    """-k for argument k of the prototype, before any device work: pointers are never dereferenced here (the device form
    gets host addresses, and there may be no GPU at all)."""
    fn = getattr(solver.load_library(), name)
    n, batch = 4, 3
    buf = np.zeros(batch * n * n)
    info = np.zeros(batch, dtype=np.int32)
    mm = np.zeros(batch, dtype=np.int32)
    if name.endswith("_device"):
        p = ctypes.c_void_p(buf.ctypes.data)
    else:
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    mp = mm.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    nan, inf = float("nan"), float("inf")

    def call(problem=1, jobz=1, rng=0, n=n, batch=batch, vl=0.0, vu=1.0, il=1, iu=2, A=p, lda=None, sA=None, B=p,
             ldb=None, sB=None, m=mp, w=p, Z=p, ldz=None, zcap=None, sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        zcap = ld if zcap is None else zcap
        sA, sB = (ld * ld if x is None else x for x in (sA, sB))
        sZ = ld * max(zcap, 1) if sZ is None else sZ
        return fn(problem, jobz, rng, n, batch, vl, vu, il, iu, A, lda, sA, B, ldb, sB, m, w, Z, ldz, zcap, sZ, info, None)

    assert call(problem=2) == -1 and call(problem=-1) == -1
    assert call(jobz=2) == -2
    assert call(rng=2) == -3 and call(rng=-1) == -3
    assert call(n=-1) == -4 and call(n=129) == -4
    assert call(batch=-1) == -5
    # 'V': vl, vu; il and iu are not looked at
    assert call(rng=1, vl=nan) == -6
    assert call(rng=1, vu=nan) == -7
    assert call(rng=1, vl=1.0, vu=1.0) == -7 and call(rng=1, vl=2.0, vu=1.0) == -7
    assert call(rng=1, vl=-inf, vu=inf, il=0, iu=99, A=None) == -10
    assert call(rng=1, vl=inf, vu=inf) == -7
    # 'I': il, iu; vl and vu are not looked at
    assert call(il=0) == -8 and call(il=n + 1, iu=n + 1) == -8
    assert call(il=3, iu=2) == -9 and call(iu=n + 1) == -9
    assert call(vl=nan, vu=nan, A=None) == -10
    assert call(A=None) == -10
    assert call(lda=n - 1) == -11
    assert call(sA=n * n - 1) == -12 and call(sA=0) == -12
    assert call(lda=n + 2, sA=n * n) == -12
    assert call(B=None) == -13
    assert call(ldb=n - 1) == -14
    assert call(sB=n * n - 1) == -15 and call(sB=0) == -15
    assert call(m=None) == -16
    assert call(w=None) == -17
    assert call(Z=None) == -18
    assert call(ldz=n - 1) == -19
    assert call(zcap=-1) == -20
    assert call(il=1, iu=3, zcap=2) == -20          # 'I' needs room for the window
    assert call(rng=1, zcap=0, info=None) == -22    # 'V' may be given none: -20 is then a problem's info
    assert call(zcap=3, sZ=3 * n - 1) == -21
    assert call(rng=1, zcap=0, sZ=n - 1) == -21     # strideZ >= ldz max(1, zcap)
    assert call(info=None) == -22
    # the first offending argument decides
    assert call(problem=2, jobz=2, rng=5) == -1
    assert call(rng=5, n=-1) == -3
    assert call(n=129, batch=-1) == -4
    assert call(rng=1, vl=nan, vu=nan) == -6
    assert call(il=0, iu=0, A=None) == -8
    assert call(m=None, w=None) == -16
    # nothing to do: success without a device and without touching any pointer or the window
    assert call(batch=0, il=0, iu=0, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    assert call(n=0, il=0, iu=0, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    assert call(n=0, rng=1, vl=nan, vu=nan, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    # what is not referenced is not checked
    assert call(problem=0, B=None, ldb=0, sB=0, m=None) == -16
    assert call(jobz=0, Z=None, ldz=0, sZ=0, info=None) == -22
    assert call(jobz=0, Z=None, ldz=0, zcap=-1, sZ=0) == -20       # zcap is checked with and without vectors
    assert call(jobz=0, il=1, iu=3, zcap=2) == -20
    assert not info.any() and not buf.any() and not mm.any()


def test_the_old_entries_still_accept_what_they_accepted():
    """The 16-argument entries keep their argument numbers, their order limit and their empty calls."""
    lib = solver.load_library()
    info = np.zeros(1, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for name in ("ek_hip_eigenpairs_batched", "ek_hip_eigenpairs_batched_device"):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 16
        assert fn(0, 0, 129, 1, None, 129, 129 * 129, None, 129, 129 * 129, None, None, 129, 129 * 129, ip, None) == -3
        assert fn(0, 0, 128, 1, None, 128, 128 * 128, None, 128, 128 * 128, None, None, 128, 128 * 128, ip, None) == -5
        assert fn(1, 1, 4, 0, None, 4, 16, None, 4, 16, None, None, 4, 16, None, None) == 0
        assert fn(1, 1, 0, 3, None, 1, 1, None, 1, 1, None, None, 1, 1, None, None) == 0
    w, Z, info = solver.eigenpairs_batched(np.zeros((0, 5, 5)))
    assert w.shape == (0, 5) and Z.shape == (0, 5, 5) and info.shape == (0,)


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_window_batched(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        solver.eigenpairs_window_batched(np.zeros((2, 4, 4)), np.zeros((2, 3, 3)))
    with pytest.raises(ValueError):
        solver.eigenpairs_window_batched(np.zeros((2, 4, 4)), il=1, vu=0.0)
    w, Z, m, info = solver.eigenpairs_window_batched(np.zeros((0, 9, 9)), il=2, iu=4)
    assert w.shape == (0, 9) and Z.shape == (0, 9, 3) and m.shape == (0,) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_batched(np.zeros((1, 129, 129)))
    assert ei.value.info == -4
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_batched(np.zeros((1, 8, 8)), il=5, iu=4)
    assert ei.value.info == -9


def test_window_table_and_cluster_cuts():
    for n in (1, 2, 3, 17, 128):
        tab = wc.windows(n)
        assert tab[0] == ("whole", 1, n)
        assert len({(il, iu) for _, il, iu in tab}) == len(tab)
        assert all(1 <= il <= iu <= n for _, il, iu in tab)
    assert {name for name, _, _ in wc.windows(128)} == {"whole", "first", "last", "quarter", "middle3"}
    assert ("quarter", 33, 64) in wc.windows(128) and ("middle3", 63, 65) in wc.windows(128)
    for n in (17, 64, 128):
        for name in wc.CLUSTERED:
            if name == "glued:1e-14" and n <= 21:   # a single Wilkinson block: nothing is glued yet
                continue
            w_ref = sl.eigh(bc.make(name, n).A, lower=True)[0]
            cut = wc.cluster_cut(w_ref)
            assert cut is not None, (name, n)
            il, iu = cut
            lim = 1e-10 * np.abs(w_ref).max()
            assert il >= 2 and w_ref[il - 1] - w_ref[il - 2] <= lim, (name, n, "the lower edge cuts no cluster")
            assert iu <= n - 1 and w_ref[iu] - w_ref[iu - 1] <= lim, (name, n, "the upper edge cuts no cluster")


def _reference(base):
    return sl.eigh(base.A, base.B, lower=True) if base.B is not None else sl.eigh(base.A, lower=True)


@pytest.mark.parametrize("n", ORDERS)
def test_lapack_windowed_drivers_stay_inside_part_of_the_bounds(n):
    """DSYEVX / DSYGVX on every unscaled case of the table, every window of the table and the cluster cuts: half of the
    eigenvalue bound, a quarter of the residual and orthogonality bounds.  A window for which LAPACK returns fewer values
    than asked (all_equal has one) is judged on what it returned, against the same slice of the full reference.
    The cond_b pencils are held to the rule for a stated cond(B), LAPACK's full driver on the whole pencil as "its own";
    at order 3 their eigenvalues only: DSYGVX leaves the smallest of the three, a 1e-6 part of |T|, with the absolute
    accuracy 2 ulp |T| of DSTEBZ's default tolerance (SciPy passes no ABSTOL), and the residual of its vector in the
    window (1, 1), 20983 n eps, misses that rule's 562 (cond_b:1e6; the full driver's own: 140.6).  The kernel refines
    such an eigenvalue to DSTEBZ's relative criterion, and tests/test_gpu_window_batched.py holds it to the whole rule
    at order 3 too."""
    worst, fails = [0.0, 0.0, 0.0], []
    names = list(bc.STANDARD) + [p for p in bc.PENCILS if not (p == "hilbert_b" and n >= 4)]
    for name in names:
        base = bc.make(name, n)
        w_ref, Z_ref = _reference(base)
        if base.exact is not None:
            w_ref = base.exact
        table = wc.windows(n)
        if name in wc.CLUSTERED and wc.cluster_cut(w_ref) is not None:
            table = table + [("cluster_cut",) + wc.cluster_cut(w_ref)]
        for wname, il, iu in table:
            w, Z = sl.eigh(base.A, base.B, lower=True, subset_by_index=(il - 1, iu - 1),
                           driver="evx" if base.B is None else "gvx")
            if len(w) == 0:
                continue
            what = "n=%d %s %s %d..%d" % (n, name, wname, il, iu)
            vectors = Z if (base.cond_b is None or n > 3) else None
            s, f = wc.judge(base.A, base.B, base.cond_b, w_ref, Z_ref, il - 1, w, vectors, what, ev_part=0.5,
                            vec_part=0.25)
            fails += f
            if s is not None and base.cond_b is None:
                worst = [max(a, b * part) for a, b, part in zip(worst, s, (0.5, 0.25, 0.25))]
    print("n=%d LAPACK's windowed drivers, largest share of the full bounds: %.3f %.3f %.3f" % ((n,) + tuple(worst)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", ORDERS)
def test_value_bounds_keep_the_gap(n):
    """Every 'V' bound of the table lies at least half the stated gap (its midpoint) from every reference eigenvalue, and
    the window it makes holds the index window it was made for."""
    for name in list(bc.STANDARD) + ["band5_band5", "a_equals_b"]:
        base = bc.make(name, n)
        w_ref = _reference(base)[0]
        for wname, il, iu in wc.windows(n):
            vl, vu, span = wc.value_bounds([w_ref], il, iu)
            first, m = span[0]
            assert vl < vu and first <= il - 1 and first + m >= iu, (name, wname)
            for x in (vl, vu):
                if np.isfinite(x):
                    assert np.abs(w_ref - x).min() >= 0.5 * wc.gap_limit(w_ref), (name, wname, x)
            assert m == int(((w_ref > vl) & (w_ref <= vu)).sum())
