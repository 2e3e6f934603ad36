"""Host-side checks of the window entries for DSYGV's problem types (ek_hip_sygv_window_batched*,
ek_hip_sygv_window_xbatched*), no GPU needed: declared in the boundary header, exported and bound with 23 arguments; every
argument error decided before any device work, with NULL, host and garbage pointers (none is dereferenced) -- itype 0 and
4 are -1 before anything else, B = NULL is -13 for every type; n = 129 is -4 for the batched pair and legal for the
xbatched pair, 257 is -4 for both; the eigenpairs window entries are still type 1 only (problem = 2 is -1 there).

And LAPACK as the yardstick of the GPU tests' own yardstick: scipy.linalg.eigh(A, B, type=itype, subset_by_index=...,
driver='gvx') (DSYGVX) against SciPy's full driver, sliced, with the judge of tests/sygv_window_cases.py -- on the seeded
random pairs, the hard pencils and the planted-cluster pencils, every window of window_batched_cases.windows, types 2 and
3, orders 2, 3, 17, 33, 64, 128, 129, 193, 256.  LAPACK is held to half of the eigenvalue bound and a quarter of the
vector bounds on the random and the planted-cluster pencils and on the two well-conditioned hard pencils, and to the whole
rule (4 max(LAPACK's full driver's own, 16 n eps)) on the cond_b pencils.  The planted pencils reproduce eigvalsh(C) and
its cluster cut, so that the GPU tests' cluster-cut windows cut clusters; every 'V' bound keeps its gap to every
reference spectrum it is used with."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import sygv_window_cases as sw
import window_batched_cases as wc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHED = ("ek_hip_sygv_window_batched_device", "ek_hip_sygv_window_batched")
XBATCHED = ("ek_hip_sygv_window_xbatched_device", "ek_hip_sygv_window_xbatched")
NAMES = BATCHED + XBATCHED
ORDERS = (2, 3, 17, 33, 64, 128, 129, 193, 256)
EPS = sw.EPS


def test_sygv_window_entries_declared_exported_and_bound():
    """Fails on a tree without the feature: the symbols are the signal, ek_hip_version stays 3."""
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in NAMES:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 23
        assert fn.argtypes == getattr(lib, name.replace("sygv_window", "eigenpairs_window")).argtypes
    assert callable(solver.sygv_window_batched) and callable(solver.sygv_window_xbatched)
    assert lib.ek_hip_version() == 3


@pytest.mark.parametrize("pointers", ["null", "host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_sygv_window_argument_errors_without_gpu(name, pointers):
    """-k for argument k of the prototype, before any device work: a pointer is compared with NULL and never followed
    (host addresses to the device form, an address that belongs to nobody, and NULL for everything that is not the
    argument under test)."""
    fn = getattr(solver.load_library(), name)
    nmax = 256 if "xbatched" in name else 128
    n, batch = (200, 3) if nmax == 256 else (100, 3)
    buf = np.zeros(8)
    info = np.zeros(batch, dtype=np.int32)
    mm = np.zeros(batch, dtype=np.int32)
    if pointers == "null":
        p = ip = mp = None
    else:
        addr = buf.ctypes.data if pointers == "host" else 0x10
        p = ctypes.c_void_p(addr) if name.endswith("_device") else ctypes.cast(ctypes.c_void_p(addr),
                                                                               ctypes.POINTER(ctypes.c_double))
        if pointers == "host":
            ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
            mp = mm.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        else:
            ip = mp = ctypes.cast(ctypes.c_void_p(0x10), ctypes.POINTER(ctypes.c_int))
    nan, inf = float("nan"), float("inf")

    def call(itype=2, jobz=1, rng=0, n=n, batch=batch, vl=0.0, vu=1.0, il=1, iu=2, A=p, lda=None, sA=None, B=p,
             ldb=None, sB=None, m=mp, w=p, Z=p, ldz=None, zcap=None, sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        zcap = ld if zcap is None else zcap
        sA, sB = (ld * ld if x is None else x for x in (sA, sB))
        sZ = ld * max(zcap, 1) if sZ is None else sZ
        return fn(itype, jobz, rng, n, batch, vl, vu, il, iu, A, lda, sA, B, ldb, sB, m, w, Z, ldz, zcap, sZ, info, None)

    # itype first, whatever else is wrong
    for bad in (0, 4, -1):
        assert call(itype=bad) == -1
        assert call(itype=bad, jobz=2, rng=5, n=-1, batch=-1, A=None, B=None, m=None, w=None, Z=None, info=None) == -1
    assert call(jobz=2) == -2
    assert call(rng=2) == -3 and call(rng=-1) == -3
    assert call(n=-1) == -4 and call(n=257) == -4 and call(n=1 << 20) == -4
    assert call(n=nmax + 1) == -4
    assert call(n=129, batch=-1) == (-5 if nmax == 256 else -4)
    assert call(n=nmax, batch=-1) == -5
    assert call(batch=-1) == -5
    assert call(rng=1, vl=nan) == -6
    assert call(rng=1, vu=nan) == -7
    assert call(rng=1, vl=1.0, vu=1.0) == -7 and call(rng=1, vl=2.0, vu=1.0) == -7
    assert call(rng=1, vl=inf, vu=inf) == -7
    assert call(il=0) == -8 and call(il=n + 1, iu=n + 1) == -8
    assert call(il=3, iu=2) == -9 and call(iu=n + 1) == -9
    if pointers == "null":
        for itype in (1, 2, 3):                     # every pointer is NULL: A decides, whatever the type
            assert call(itype=itype) == -10
        assert call(batch=0) == 0 and call(n=0, il=0, iu=0) == 0
        assert call(n=0, rng=1, vl=nan, vu=nan) == 0
        return
    assert call(rng=1, vl=-inf, vu=inf, il=0, iu=999, A=None) == -10
    assert call(vl=nan, vu=nan, A=None) == -10
    assert call(A=None) == -10
    assert call(lda=n - 1) == -11
    assert call(sA=n * n - 1) == -12 and call(sA=0) == -12
    assert call(lda=n + 2, sA=n * n) == -12
    for itype in (1, 2, 3):                         # B is always required
        assert call(itype=itype, B=None) == -13
        assert call(itype=itype, ldb=n - 1) == -14
        assert call(itype=itype, sB=n * n - 1) == -15 and call(itype=itype, sB=0) == -15
    assert call(m=None) == -16
    assert call(w=None) == -17
    assert call(Z=None) == -18
    assert call(ldz=n - 1) == -19
    assert call(zcap=-1) == -20
    assert call(il=1, iu=3, zcap=2) == -20
    assert call(rng=1, zcap=0, info=None) == -22
    assert call(zcap=3, sZ=3 * n - 1) == -21
    assert call(rng=1, zcap=0, sZ=n - 1) == -21
    assert call(info=None) == -22
    # the first offending argument decides
    assert call(rng=5, n=-1) == -3
    assert call(n=257, batch=-1) == -4
    assert call(rng=1, vl=nan, vu=nan) == -6
    assert call(il=0, iu=0, A=None) == -8
    assert call(B=None, ldb=0, m=None) == -13
    assert call(m=None, w=None) == -16
    # nothing to do: success without a device and without touching any pointer or the window
    assert call(batch=0) == 0 and call(n=0, il=0, iu=0) == 0
    assert call(batch=0, il=0, iu=0, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    assert call(n=0, rng=1, vl=nan, vu=nan, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    # what is not referenced is not checked
    assert call(jobz=0, Z=None, ldz=0, sZ=0, info=None) == -22
    assert call(jobz=0, Z=None, ldz=0, zcap=-1, sZ=0) == -20
    assert call(jobz=0, il=1, iu=3, zcap=2) == -20
    assert not info.any() and not buf.any() and not mm.any()


@pytest.mark.parametrize("name", ["ek_hip_eigenpairs_window_batched_device", "ek_hip_eigenpairs_window_batched",
                                  "ek_hip_eigenpairs_window_xbatched_device", "ek_hip_eigenpairs_window_xbatched"])
def test_the_eigenpairs_window_entries_are_still_type_1_only(name):
    fn = getattr(solver.load_library(), name)
    for problem in (2, 3):
        assert fn(problem, 0, 0, 8, 1, 0.0, 0.0, 1, 1, None, 8, 64, None, 8, 64, None, None, None, 8, 1, 8, None,
                  None) == -1
    assert fn(1, 0, 0, 8, 1, 0.0, 0.0, 1, 1, None, 8, 64, None, 8, 64, None, None, None, 8, 1, 8, None, None) == -10


def test_python_mirrors_reject_bad_input_before_the_library():
    for fn, nmax in ((solver.sygv_window_batched, 128), (solver.sygv_window_xbatched, 256)):
        with pytest.raises(ValueError):
            fn(np.zeros((3, 20)), np.zeros((3, 20)))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 20, 20)), None)
        with pytest.raises(ValueError):
            fn(np.zeros((2, 20, 20)), np.zeros((2, 19, 19)))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 20, 20)), np.zeros((2, 20, 20)), il=1, vu=0.0)
        w, Z, m, info = fn(np.zeros((0, 20, 20)), np.zeros((0, 20, 20)), itype=3, il=2, iu=4)
        assert w.shape == (0, 20) and Z.shape == (0, 20, 3) and m.shape == (0,) and info.shape == (0,)
        for bad in (0, 4):
            with pytest.raises(solver.SolverError) as ei:
                fn(np.zeros((1, 20, 20)), np.zeros((1, 20, 20)), itype=bad)
            assert ei.value.info == -1
        with pytest.raises(solver.SolverError) as ei:
            fn(np.zeros((1, nmax + 1, nmax + 1)), np.zeros((1, nmax + 1, nmax + 1)), itype=2)
        assert ei.value.info == -4
        with pytest.raises(solver.SolverError) as ei:
            fn(np.zeros((1, 20, 20)), np.zeros((1, 20, 20)), itype=2, il=5, iu=4)
        assert ei.value.info == -9


# ------------------------------------------------------------------------------------ LAPACK against the same judge
def _gvx(itype, A, B, il, iu):
    return sl.eigh(A, B, type=itype, lower=True, subset_by_index=(il - 1, iu - 1), driver="gvx")


def _pencils(n):
    """[(key, A, B, kind)] of an order: kind 'random', 'planted', 'hard' (well-conditioned) or 'ill' (cond_b)."""
    A, B = sw.pairs(n)
    out = [(("pairs", n, b), A[b], B[b], "random") for b in range(A.shape[0])]
    for name in sw.HARD:
        Ah, Bh = sw.hard(name, n)
        out.append((("hard", name, n), Ah, Bh, "ill" if name in sw.ILL else "hard"))
    for name in wc.CLUSTERED:
        Ap, Bp, _ = sw.planted(name, n)
        out.append((("planted", name, n), Ap, Bp, "planted"))
    return out


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", ORDERS)
def test_lapack_windowed_driver_stays_inside_part_of_the_bounds(n, itype):
    worst = {"random": [0.0] * 3, "planted": [0.0] * 3, "hard": [0.0] * 3, "ill": [0.0] * 3}
    fails = []
    for key, A, B, kind in _pencils(n):
        w_ref, Z_ref = sw.reference(key, itype, A, B)
        rule = None if kind in ("random", "planted") else sw.quantities(itype, A, B, w_ref, Z_ref)
        ev, vec = (1.0, 1.0) if kind == "ill" else (0.5, 0.25)
        for wname, il, iu in wc.windows(n):
            w, Z = _gvx(itype, A, B, il, iu)
            if len(w) != iu - il + 1:
                fails.append("n=%d itype=%d %s %s: LAPACK returned %d values" % (n, itype, key[1:], wname, len(w)))
                continue
            s, f = sw.judge(itype, A, B, w_ref, il - 1, w, Z, "n=%d itype=%d %s %s" % (n, itype, key[1:], wname), ev, vec,
                            rule)
            fails += f
            if s:                                   # shares of the WHOLE bound
                worst[kind] = sw.worse(worst[kind], [s[0] * ev, s[1] * vec, s[2] * vec])
    for kind in sorted(worst):
        print("n=%d itype=%d %-8s LAPACK's DSYGVX uses of the bounds: eigenvalues %.3f residual %.4f orthogonality %.4f"
              % ((n, itype, kind) + tuple(worst[kind])))
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("n", [33, 64, 128, 129, 193, 256])
def test_planted_pencils_have_the_spectrum_and_the_clusters_of_c(n):
    """SciPy's spectrum of types 2 and 3 of a planted pencil is eigvalsh(C) within 0.045 of the eigenvalue bound, and its
    cluster cut is C's: the GPU tests' cluster-cut windows cut clusters."""
    for name in wc.CLUSTERED:
        A, B, C = sw.planted(name, n)
        assert 4.0 <= np.linalg.cond(B) <= 5.5, (name, n, np.linalg.cond(B))
        wC = sl.eigvalsh(C)
        cut = wc.cluster_cut(wC)
        assert cut is not None, (name, n)
        for itype in (2, 3):
            w_ref = sw.reference(("planted", name, n), itype, A, B)[0]
            tol = 4 * max(n, 8) * EPS * np.abs(wC).max()
            assert np.abs(w_ref - wC).max() <= 0.045 * tol, (name, n, itype, np.abs(w_ref - wC).max() / tol)
            if n in (33, 128, 129, 256):
                assert wc.cluster_cut(w_ref) == cut, (name, n, itype, wc.cluster_cut(w_ref), cut)


@pytest.mark.parametrize("n", ORDERS)
def test_value_bounds_keep_the_gap_to_every_reference_spectrum(n):
    """Every 'V' bound the GPU tests take from value_bounds for the random pairs lies at least half of gap_limit away
    from every reference spectrum it is used with (types 2 and 3 share the spectrum to rounding: both are checked), and
    the counts it states are the counts of those spectra."""
    A, B = sw.pairs(n)
    for itype in (2, 3):
        refs = [sw.reference(("pairs", n, b), itype, A[b], B[b])[0] for b in range(A.shape[0])]
        both = refs + [sw.reference(("pairs", n, b), 5 - itype, A[b], B[b])[0] for b in range(A.shape[0])]
        for wname, il, iu in wc.windows(n):
            vl, vu, span = wc.value_bounds(both, il, iu)
            assert vl < vu
            for w, (first, m) in zip(both, span):
                for x in (vl, vu):
                    if np.isfinite(x):
                        assert np.abs(w - x).min() >= 0.5 * wc.gap_limit(w), (n, itype, wname, x)
                assert m == int(((w > vl) & (w <= vu)).sum()) and first == int((w <= vl).sum())
            first0, m0 = span[0]
            assert first0 <= il - 1 and first0 + m0 >= iu, (n, itype, wname)
