"""Host side of the divide & conquer's stage tests (no GPU needed): the inputs of tests/test_gpu_stedc.py are what they
claim to be, the CPU oracle alone stays far inside every bound the GPU file uses, the classes land in the branch of the
top merge's deflation they were chosen for, the recorded spectra are the oracle's, and the stage entry is declared,
exported, bound and refuses bad arguments before any device work.

Measured over every class at orders 33, 66, 259, 1100 and 2100, the oracle's worst figures are 0.23 n eps scale for the
eigenvalues against DSTEBZ, 0.22 n eps scale for the residual and 0.38 n eps for the orthogonality (all three at order 33;
from 259 on: 0.05, 0.05, 0.06), against bounds of 4, 32 and 32: a factor of 17 or more inside."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import stedc_cases as sc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (33, 66, 259, 1100)
HOOKS = ("ek_hip_debug_stedc", "ek_hip_debug_stedc_zcols")


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    """(d, e, w, Z) of the oracle's D&C, computed once per case and left unchanged"""
    from oracle import ek_oracle
    d, e = sc.tridiagonal(name, n)
    w, Z = ek_oracle.stedc(d, e)
    for a in (d, e, w, Z):
        a.setflags(write=False)
    return d, e, w, Z


@functools.lru_cache(maxsize=None)
def _top_counts(name, n):
    from oracle import ek_oracle
    d, e = sc.tridiagonal(name, n)
    (d1, e1), (d2, e2) = sc.split_halves(d, e)
    return sc.top_merge_counts(d, e, (ek_oracle.stedc(d1, e1), ek_oracle.stedc(d2, e2)), types=True)


def test_hooks_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in HOOKS:
        assert name in hooks and name not in declared
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
    assert lib.ek_hip_debug_stedc.restype is ctypes.c_int and len(lib.ek_hip_debug_stedc.argtypes) == 14
    assert callable(solver.stedc_select) and callable(solver.stedc_zcols)


def test_entry_refuses_bad_arguments_before_any_device_work():
    """-k for the k-th argument, as ek_hip_stedc; none of these calls initialises a device"""
    lib = solver.load_library()
    n = 40
    d, e, w = np.ones(n), np.ones(n), np.zeros(n)
    Z = np.zeros((n, n), order="F")
    rec = np.zeros((8, 6), dtype=np.int32)
    info = ctypes.c_int(7)
    P, I = solver._P, solver._I

    def call(n=n, d=P(d), e=P(e), nsel=-1, first=0, nb=n, npcol=1, mycol=0, w=P(w), Z=P(Z), ldz=n, merges=I(rec), cap=8):
        return lib.ek_hip_debug_stedc(n, d, e, nsel, first, nb, npcol, mycol, w, Z, ldz, merges, cap, ctypes.byref(info))

    assert call(n=-1) == -1
    assert call(d=None) == -2
    assert call(e=None) == -3
    assert call(nsel=n + 1) == -4
    assert call(nsel=5, first=n - 4) == -4               # ranks n-4 .. n: one beyond the last
    assert call(nsel=14, nb=8, npcol=3, mycol=2) == -4   # the cell's second block would start at rank 40
    assert call(nsel=5, first=-1) == -5
    assert call(nsel=5, first=1, nb=8, npcol=2) == -5    # a window on a grid
    assert call(nsel=5, nb=0) == -6
    assert call(nsel=5, npcol=0) == -7
    assert call(nsel=5, npcol=2, mycol=2) == -8
    assert call(w=None) == -9
    assert call(Z=None) == -10
    assert call(ldz=n - 1) == -11
    assert call(merges=None) == -12
    assert call(cap=-1) == -13
    assert call(n=130, ldz=130, cap=4) == -13            # 130 -> 65 + 65 -> (32 + 33) x 2 -> (16 + 17) x 2: five merges
    assert lib.ek_hip_debug_stedc(n, P(d), P(e), -1, 0, n, 1, 0, P(w), P(Z), n, I(rec), 8, None) == -14
    assert call(n=0) == 0 and info.value == 0


@pytest.mark.parametrize("n", [2, 20, 32, 33, 66, 259, 1100, 2100])
def test_storage_form_follows_the_selection(n):
    """compact bases (an n x nsel array) exactly when n > 32 and nsel <= n - n/2; the full form is never compact"""
    h2 = n - n // 2
    assert solver.stedc_zcols(n, -1) == n
    for nsel in sorted({1, 2, h2 - 1, h2, h2 + 1, n - 1, n} & set(range(1, n + 1))):
        want = nsel if (n > 32 and nsel <= h2 and nsel < n) else n
        assert solver.stedc_zcols(n, nsel) == want, (n, nsel)
        assert sc.is_compact(n, nsel) == (want != n), (n, nsel)
    assert solver.stedc_zcols(n, n + 1) == -1


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("name", sc.CLASSES)
def test_oracle_meets_the_bounds_of_the_gpu_tests(name, n):
    d, e, w, Z = _reference(name, n)
    scale = sc.scale_of(d, e)
    w2 = sl.eigvalsh_tridiagonal(d, e, lapack_driver="stebz")
    r_w = np.abs(w - w2).max() / (n * sc.EPS * scale)
    r_res = np.abs(sc.apply_tridiagonal(d, e, Z) - Z * w).max() / (n * sc.EPS * scale)
    r_orth = np.abs(Z.T @ Z - np.eye(n)).max() / (n * sc.EPS)
    print("stedc oracle %s n=%d: w %.3f res %.3f orth %.3f (n eps)" % (name, n, r_w, r_res, r_orth))
    assert np.all(np.diff(w) >= 0)
    # a tenth of each bound: the reference's own error leaves the GPU stage nine tenths
    assert r_w <= sc.BOUND_W / 10 and r_res <= sc.BOUND_RES / 10 and r_orth <= sc.BOUND_ORTH / 10


@pytest.mark.parametrize("n", ORDERS)
def test_generators_with_a_closed_form(n):
    for name, width in (("clement", n - 1), ("repeated_blocks", 4.0)):
        d, e, w, _ = _reference(name, n)
        exact = sc.exact_spectrum(name, n)
        assert exact.shape == (n,) and np.all(np.diff(exact) >= 0)
        assert np.abs(w - exact).max() <= sc.BOUND_W / 10 * n * sc.EPS * width, name
    d, e = sc.tridiagonal("clement", n)
    assert not d.any() and np.allclose(e * e, np.arange(1.0, n) * np.arange(n - 1.0, 0, -1), rtol=4 * sc.EPS, atol=0)
    d, e = sc.tridiagonal("repeated_blocks", n)
    assert np.all(d == 2.0) and set(np.flatnonzero(e == 0.0)) == set(range(15, n - 1, 16)) and np.all(np.abs(e) <= 1.0)


@pytest.mark.parametrize("n", [2, 3, 33, 1100])
def test_generators_are_seeded_and_shaped(n):
    for name in sc.CLASSES:
        d, e = sc.tridiagonal(name, n)
        d2, e2 = sc.tridiagonal(name, n)
        assert d.shape == (n,) and e.shape == (n - 1,) and d.dtype == e.dtype == np.float64
        assert np.array_equal(d, d2) and np.array_equal(e, e2) and d is not d2
        assert np.isfinite(d).all() and np.isfinite(e).all()
    h = n // 2
    d, e = sc.tridiagonal("zero_at_splits", n)
    assert e[h - 1] == 0.0 and (h // 2 < 1 or e[h // 2 - 1] == 0.0)
    d, e = sc.tridiagonal("tiny_at_splits", n)
    assert e[h - 1] == 1e-18 and (n < 3 or e[h + (n - h) // 2 - 1] == -1e-15)
    assert (sc.tridiagonal("negative_e", n)[1] < 0).all()
    e = sc.tridiagonal("mixed_sign_e", n)[1]
    assert np.array_equal(e < 0, np.arange(n - 1) % 3 == 2)
    assert np.abs(sc.tridiagonal("huge", n)[0]).max() > 1e148 and np.abs(sc.tridiagonal("tiny", n)[0]).max() < 1e-149


def test_classes_take_the_intended_branch_of_the_top_merge():
    """counts of the numpy replay of the top merge's scan on the oracle's halves, at order 1100"""
    n = 1100
    counts = {name: _top_counts(name, n) for name in sc.CLASSES}
    for name in sc.CLASSES:
        print("stedc replay %s n=%d: (deflated, rotations, k) = %s, (k1, k2, k3) = %s" % ((name, n) + counts[name]))
    (ndf, nrot, k), _ = counts["clement"]
    assert nrot >= 0.4 * n and ndf + k == n
    assert counts["legendre"][0] == (0, 0, n)
    (ndf, nrot, k), _ = counts["laguerre"]
    assert nrot == 0 and 1 <= ndf <= n // 2
    for name in ("cluster_eps", "zero_at_splits", "tiny_at_splits"):
        assert counts[name][0] == (n, 0, 0), name
    for name in ("wilkinson_glued", "one_big"):
        (ndf, nrot, k), _ = counts[name]
        assert nrot >= 50 and k >= 100, name
    for name in ("repeated_blocks", "localized"):
        (ndf, nrot, k), _ = counts[name]
        assert nrot == 0 and 1 <= k <= 16, name
    for name in sc.CLASSES:
        (ndf, nrot, k), (k1, k2, k3) = counts[name]
        assert ndf + k == n and k1 + k2 + k3 == k and k2 <= nrot <= ndf


def test_replay_of_a_merge_that_is_known_exactly():
    """two identical halves coupled weakly: every pole of the first half meets its twin, so every pair is rotated (the
    dense type) unless its weight is tiny; a diagonal matrix deflates everything"""
    n = 8
    d = np.array([1.0, 2.0, 3.0, 4.0, 1.0, 2.0, 3.0, 4.0])
    e = np.array([0.5, 0.5, 0.5, 0.25, 0.5, 0.5, 0.5])
    (d1, e1), (d2, e2) = sc.split_halves(d, e)
    assert d1[-1] == (4.0 - 0.25) / 4.0 and d2[0] == (1.0 - 0.25) / 4.0 and len(e1) == len(e2) == 3
    T1 = np.diag(d1) + np.diag(e1, 1) + np.diag(e1, -1)
    h = np.linalg.eigh(T1)
    (ndf, nrot, k), (k1, k2, k3) = sc.top_merge_counts(d, e, (h, h), types=True)   # the SAME spectrum twice
    assert (ndf, nrot, k) == (4, 4, 4) and (k1, k2, k3) == (0, 4, 0)
    d0, e0 = np.arange(8.0), np.zeros(7)
    (a1, b1), (a2, b2) = sc.split_halves(d0, e0)
    halves = ((a1, np.eye(4)), (a2, np.eye(4)))
    assert sc.top_merge_counts(d0, e0, halves) == (8, 0, 0)


def test_recorded_spectra_are_the_oracles():
    """the file tests/test_gpu_stedc.py reads at orders 1100 and 2100: every class, the right length, ascending, equal to a
    fresh run of the oracle at 1100 (to 0.05 n eps scale, a quarter of what the oracle differs from DSTEBZ by: the same
    arithmetic, another libm at most) and within
    a tenth of the eigenvalue bound of DSTEBZ at both orders"""
    for n in sc.RECORDED_ORDERS:
        for name in sc.CLASSES:
            w = sc.recorded_spectrum(name, n)
            d, e = sc.tridiagonal(name, n)
            scale = sc.scale_of(d, e)
            assert w.shape == (n,) and np.all(np.diff(w) >= 0)
            w2 = sl.eigvalsh_tridiagonal(d, e, lapack_driver="stebz")
            assert np.abs(w - w2).max() <= sc.BOUND_W / 10 * n * sc.EPS * scale, (name, n)
            if n == 1100:
                assert np.abs(w - _reference(name, n)[2]).max() <= 0.05 * n * sc.EPS * scale, name


def test_selection_ranks_tile_the_spectrum():
    """numroc and sel_rank as the grid tests use them: the cells' ranks are a partition of 0 .. n-1"""
    for n, nb, npcol in ((259, 16, 3), (1100, 64, 4), (1100, 128, 2), (20, 20, 1), (7, 2, 5)):
        seen = []
        for mycol in range(npcol):
            m = sc.numroc(n, nb, mycol, npcol)
            seen.extend(sc.sel_rank(np.arange(m), 0, nb, npcol, mycol).tolist())
        assert sorted(seen) == list(range(n)), (n, nb, npcol)
    assert sc.sel_rank(np.arange(3), 5, 100, 1, 0).tolist() == [5, 6, 7]
