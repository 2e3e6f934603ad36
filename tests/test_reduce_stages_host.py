"""Host side of the stage tests of the generalized path's first three stages (no GPU needed): the two test hooks of
ek_hip_sygst / ek_hip_trtrs are declared, exported, bound and clamp as documented; the scratch of the reduction covers
both recursions at every order with the direct order at its lowest; and the inputs of tests/test_gpu_reduce_stages.py are
what they claim to be -- the integer pencil is exact, and SciPy alone stays inside every bound the GPU file uses."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import reduce_cases as rc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ek_hip_debug_stage_leaves256", "ek_hip_debug_set_sygst_direct", "ek_hip_debug_sygst_scratch")


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
    for name in HOOKS[:2]:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_int]
    assert lib.ek_hip_debug_sygst_scratch.restype is ctypes.c_ulonglong
    assert callable(solver.stage_leaves256) and callable(solver.set_sygst_direct) and callable(solver.sygst_scratch)
    # the boundary header points at the hook that selects the production form of the solves
    assert "ek_hip_debug_stage_leaves256" in hdr


def test_stage_leaves_hook_returns_the_previous_mode():
    before = solver.stage_leaves256(1)
    try:
        assert before == 0                           # the default: today's behaviour
        assert solver.stage_leaves256(1) == 1
        assert solver.stage_leaves256(0) == 1
        assert solver.stage_leaves256(7) == 0        # only 1 switches the leaves on
        assert solver.stage_leaves256(-1) == 0
        assert solver.stage_leaves256(1) == 0
    finally:
        assert solver.stage_leaves256(0) == 1
    assert solver.stage_leaves256(0) == 0


def test_sygst_direct_hook_returns_the_previous_order_and_clamps():
    before = solver.set_sygst_direct(300)
    try:
        assert before == 4096
        assert solver.set_sygst_direct(100) == 300   # below 256: raised to 256
        assert solver.set_sygst_direct(1) == 256
        assert solver.set_sygst_direct(256) == 256
        assert solver.set_sygst_direct(8192) == 256
        assert solver.set_sygst_direct(0) == 8192    # <= 0 restores 4096
        assert solver.set_sygst_direct(-5) == 4096
        assert solver.set_sygst_direct(257) == 4096
    finally:
        assert solver.set_sygst_direct(0) == 257
    assert solver.set_sygst_direct(0) == 4096


def _need(n, direct):
    """what the two recursions take from the scratch: (n1^2 + n1 n2, max(n1, n2) n), the largest over all levels"""
    if n <= direct:
        return 0, 0
    n1 = rc.split_t(n)
    n2 = n - n1
    a, b = _need(n1, direct)
    c, d = _need(n2, direct)
    return max(n1 * n1 + n1 * n2, a, c), max(max(n1, n2) * n, b, d)


def test_scratch_covers_both_recursions_with_the_direct_order_at_256():
    """sygst_scratch_doubles(n) = 2 (n / 2 + 128)^2 against what sygst_rec (C11 in full and L21 C11: n1^2 + n1 n2) and
    sygst2_rec (T and the larger of A22 and the SYR2K's product: max(n1, n2) n) take under split_t, for every order up
    to beyond the largest the suite and the benchmark run, at the lowest direct order the hook allows and at the default."""
    try:
        for direct in (256, 4096):
            solver.set_sygst_direct(direct)
            for n in range(1, 40001):
                have, need1, need2 = solver.sygst_scratch(n)
                assert have == max(2 * (n // 2 + 128) ** 2, 2 * 128 * 128)
                assert need1 <= have and need2 <= have, (direct, n, have, need1, need2)
                if n > direct:
                    n1 = rc.split_t(n)
                    n2 = n - n1
                    assert 0 < n1 < n and n1 % 256 == 0
                    # the top level is the largest, and it is the quantity the header names
                    assert need1 == n1 * n1 + n1 * n2 and need2 == max(n1, n2) * n, (direct, n)
                else:
                    assert need1 == need2 == 0
            for n in list(range(257, 3000)) + [4097, 5000, 8191, 16384, 32768, 39999]:   # the library's own walk of the levels
                assert solver.sygst_scratch(n)[1:] == _need(n, direct), (direct, n)
    finally:
        solver.set_sygst_direct(0)
    assert solver.sygst_scratch(5000)[1:] == _need(5000, 4096)


@pytest.mark.parametrize("n", [2, 257, 640, 1300])
def test_integer_pencil_is_exact(n):
    """L L^T = B, L C L^T = A and L^T Y = Z hold exactly (the float64 BLAS products against int64 arithmetic at the small orders, through the exact inverse at all), L has the
    structure that makes its inverse dyadic, and SciPy's Cholesky factor, reduction and recovery -- the operations of the
    GPU stages -- reproduce L, C and Y inside every bound of tests/test_gpu_reduce_stages.py (in fact exactly)."""
    p = rc.pencil("integer", n)
    A, B, L, C, Z, Y, D, E = (p[k] for k in "A B L C Z X D E".split())
    Li, Ci, Yi = (np.rint(M).astype(np.int64) for M in (L, C, Y))
    for M in (A, B, L, C, Z, Y):
        assert np.array_equal(M, np.rint(M))
    if n <= 300:                                                # (int64 products are slow: the identities below serve above)
        assert np.array_equal(np.rint(B).astype(np.int64), Li @ Li.T)
        assert np.array_equal(np.rint(A).astype(np.int64), Li @ Ci @ Li.T)
        assert np.array_equal(np.rint(Z).astype(np.int64), Li.T @ Yi)
    assert np.array_equal(C, C.T) and np.abs(C).max() <= 3 and np.abs(Y).max() <= 3
    # the structure: D in {1, 2, 4}; E strictly lower, entries in -2 .. 2, at (odd row, even column) only
    assert set(np.unique(D)) <= {1.0, 2.0, 4.0} and np.array_equal(np.diag(L), D)
    assert np.array_equal(np.triu(E), np.zeros((n, n))) and np.abs(E).max() <= 2
    r, c = np.nonzero(E)
    assert (r % 2 == 1).all() and (c % 2 == 0).all()
    assert len(r) >= n // 2                                     # no odd row of E is empty
    DE = E / D[:, None]
    assert not (DE @ DE).any()
    Linv = rc.integer_inverse(D, E)
    assert np.array_equal(L @ Linv, np.eye(n)) and np.array_equal(Linv @ L, np.eye(n))
    assert np.array_equal(Linv * 16, np.rint(Linv * 16))        # dyadic
    assert np.array_equal(Linv @ A @ Linv.T, C) and np.array_equal(Linv @ B @ Linv.T, np.eye(n))
    assert np.array_equal(Linv.T @ Z, Y)
    # SciPy on the exact pencil, under the GPU file's bounds
    Ls = sl.cholesky(B, lower=True)
    assert np.abs(Ls - L).max() <= rc.bound_potrf(n, L)
    assert np.abs(Ls @ Ls.T - B).max() <= rc.bound_potrf(n, L)
    Cs = rc.reduce_scipy(A, L)
    assert np.abs(Cs - C).max() <= rc.bound_sygst_forward(n, C)
    assert np.abs(L @ Cs @ L.T - A).max() <= rc.bound_sygst_backward(n, A)
    Xs = rc.recover_scipy(L, Z)
    assert np.abs(Xs - Y).max() <= rc.bound_trtrs(n, Y)
    assert np.array_equal(Ls, L) and np.array_equal(Cs, C) and np.array_equal(Xs, Y)


@pytest.mark.parametrize("cls", ["random", "ill"])
def test_scipy_reference_is_well_inside_the_bounds(cls):
    """The reference of the random and of the ill-conditioned class against substitution in numpy.longdouble at n = 257
    (the class's own factor L taken as given): the reference spends at most a quarter of each bound, so a GPU result
    that is as good as SciPy's passes."""
    n = 257
    p = rc.pencil(cls, n)
    A, B, L, C, Z, X, cond = (p[k] for k in "A B L C Z X cond".split())
    if cls == "random":
        assert cond == 1.0 and np.linalg.cond(B) < 10.0
    else:
        assert 1e7 < cond < 1e9
    Cq = rc.substitute_longdouble(L, rc.substitute_longdouble(L, A).T)
    Xq = rc.substitute_longdouble(L, Z, trans=True)
    err_c = float(np.abs(C - Cq).max())
    err_x = float(np.abs(X - Xq).max())
    print("%s n=%d: |C - C_ld| = %.3e (bound %.3e), |X - X_ld| = %.3e (bound %.3e)"
          % (cls, n, err_c, rc.bound_sygst_forward(n, C, cond), err_x, rc.bound_trtrs(n, X, cond)))
    assert err_c <= rc.bound_sygst_forward(n, C, cond) / 4
    assert err_x <= rc.bound_trtrs(n, X, cond) / 4
    assert np.abs(L @ C @ L.T - A).max() <= rc.bound_sygst_backward(n, A, cond) / 4
    assert np.abs(L @ L.T - B).max() <= rc.bound_potrf(n, L) / 4
