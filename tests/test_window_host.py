"""CPU suite of the eigenpair-window interface (ek_hip_eigenpairs*, ek_hip_stebz_range): the symbols are declared,
exported and bound, the window plans are the ones the header promises, and every argument check answers without a GPU
(the checks run before the library touches a device).  No torch in this process (see tests/test_host_logic.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ek_hip_eigenpairs_device", "ek_hip_eigenpairs", "ek_hip_stebz_range")
HOOK = "ek_hip_debug_window_workspace_bytes"
INF = math.inf


def test_window_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    assert set(NEW) <= set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    assert HOOK in set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    assert set(NEW) | {HOOK} <= set(solver.EXPORTED_SYMBOLS)
    lib = solver.load_library()
    for name in NEW + (HOOK,):
        assert getattr(lib, name).argtypes is not None, name
    assert callable(solver.eigenpairs) and callable(solver.stebz_range)


SIZES = [256, 640, 1000, 2048, 4096, 8192, 16384, 32768]


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_index_window_plan_is_the_select_arms(problem, n):
    for m in sorted({1, 64, 1024 if 1024 <= n - n // 2 else 1, n // 4, n - n // 2}):
        got = solver.window_workspace_bytes(problem, n, vectors=True, by_value=False, m=m)
        assert got == solver.workspace_bytes(problem, n, n_vec=m)[0], (n, m)


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_value_window_plan_is_the_full_plan(problem, n):
    full = solver.workspace_bytes(problem, n, n_vec=n)[0]
    for m in (0, 1, n // 2, n):            # (m is not known when a value window plans: it is not referenced)
        assert solver.window_workspace_bytes(problem, n, vectors=True, by_value=True, m=m) == full


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_values_only_window_plan_is_the_values_plan(problem, n):
    vals = solver.values_workspace_bytes(problem, n)
    for by_value in (False, True):
        assert solver.window_workspace_bytes(problem, n, vectors=False, by_value=by_value, m=n // 3) == vals


@pytest.mark.parametrize("n", [33, 99, 255, 257, 1001, 4097])
def test_value_window_plan_holds_any_window_on_odd_orders(n):
    # the full plan, grown where a compact D&C or Q1 on m columns could want more: never below the full plan
    full = solver.workspace_bytes(1, n, n_vec=n)[0]
    got = solver.window_workspace_bytes(1, n, vectors=True, by_value=True)
    assert full <= got <= full + 64 * 1024 + 64 * n


def test_window_hook_rejects_bad_arguments():
    lib = solver.load_library()
    assert lib.ek_hip_debug_window_workspace_bytes(2, 100, 1, 0, 10) == 0
    assert lib.ek_hip_debug_window_workspace_bytes(0, 0, 1, 0, 0) == 0
    assert lib.ek_hip_debug_window_workspace_bytes(0, 100, 2, 0, 10) == 0
    assert lib.ek_hip_debug_window_workspace_bytes(0, 100, 1, 2, 10) == 0
    assert lib.ek_hip_debug_window_workspace_bytes(0, 100, 1, 0, 101) == 0


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_eigenpairs_argument_checks_without_gpu():
    lib = solver.load_library()
    n = 4
    a = np.eye(n, order="F"); b = np.eye(n, order="F"); w = np.zeros(n); z = np.zeros((n, n), order="F")
    m, f = ctypes.c_int(-7), ctypes.c_int(-7)
    M, F = ctypes.byref(m), ctypes.byref(f)

    def call(problem=0, jobz=1, rng=0, nn=n, vl=0.0, vu=1.0, il=1, iu=n, A=_dp(a), lda=n, B=None, ldb=1,
             mp=M, fp=F, W=_dp(w), Z=_dp(z), ldz=n, zcap=n):
        return lib.ek_hip_eigenpairs(problem, jobz, rng, nn, vl, vu, il, iu, A, lda, B, ldb, mp, fp, W, Z, ldz, zcap,
                                     None, 0)
    assert call(problem=2) == -1
    assert call(jobz=2) == -2 and call(jobz=-1) == -2
    assert call(rng=2) == -3 and call(rng=-1) == -3
    assert call(nn=-1) == -4
    assert call(rng=1, vl=math.nan) == -5
    assert call(rng=1, vu=math.nan) == -6
    assert call(rng=1, vl=1.0, vu=1.0) == -6 and call(rng=1, vl=2.0, vu=1.0) == -6
    assert call(rng=1, vl=INF, vu=INF) == -6 and call(rng=1, vl=-INF, vu=-INF) == -6
    assert call(il=0) == -7 and call(il=n + 1, iu=n + 1) == -7
    assert call(il=3, iu=2) == -8 and call(iu=n + 1) == -8
    assert call(A=None) == -9
    assert call(lda=n - 1) == -10
    assert call(problem=1, B=None, ldb=n) == -11
    assert call(problem=1, B=_dp(b), ldb=n - 1) == -12
    assert call(mp=None) == -13
    assert call(fp=None) == -14
    assert call(W=None) == -15
    assert call(Z=None) == -16
    assert call(ldz=n - 1) == -17
    assert call(zcap=-1) == -18
    # an index window wider than zcap: its m comes back, before any device work
    m.value = -7
    assert call(il=2, iu=4, zcap=2) == -18 and m.value == 3
    # the checks a value window or a values-only call does not make
    assert call(jobz=0, Z=None, ldz=0, zcap=-1, nn=-1) == -4       # (Z, ldz, zcap: not referenced without vectors)
    assert call(rng=1, il=0, iu=-5, A=None) == -9                  # (il, iu: not referenced by a value window)
    assert call(rng=0, vl=math.nan, vu=math.nan, A=None) == -9     # (vl, vu: not referenced by an index window)
    # the device form answers the same
    dummy = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks first

    def dcall(problem=0, jobz=1, rng=0, nn=n, vl=0.0, vu=1.0, il=1, iu=n, A=dummy, lda=n, B=None, ldb=1,
              mp=M, fp=F, W=dummy, Z=dummy, ldz=n, zcap=n):
        return lib.ek_hip_eigenpairs_device(problem, jobz, rng, nn, vl, vu, il, iu, A, lda, B, ldb, mp, fp, W, Z, ldz,
                                            zcap, None, 0)
    assert dcall(problem=-1) == -1
    assert dcall(jobz=3) == -2
    assert dcall(rng=5) == -3
    assert dcall(nn=-2) == -4
    assert dcall(rng=1, vl=math.nan) == -5
    assert dcall(rng=1, vl=0.5, vu=0.5) == -6
    assert dcall(il=0) == -7
    assert dcall(il=2, iu=1) == -8
    assert dcall(A=None) == -9
    assert dcall(lda=1) == -10
    assert dcall(problem=1, B=None, ldb=n) == -11
    assert dcall(problem=1, B=dummy, ldb=2) == -12
    assert dcall(mp=None) == -13
    assert dcall(fp=None) == -14
    assert dcall(W=None) == -15
    assert dcall(Z=None) == -16
    assert dcall(ldz=0) == -17
    assert dcall(zcap=-3) == -18
    m.value = -7
    assert dcall(il=1, iu=4, zcap=3) == -18 and m.value == 4


def test_stebz_range_argument_checks_without_gpu():
    lib = solver.load_library()
    d = np.ones(5); e = np.ones(5); w = np.zeros(5)
    il, m = ctypes.c_int(0), ctypes.c_int(0)
    IL, M = ctypes.byref(il), ctypes.byref(m)
    call = lib.ek_hip_stebz_range
    assert call(-1, _dp(d), _dp(e), 0.0, 1.0, IL, M, _dp(w)) == -1
    assert call(5, None, _dp(e), 0.0, 1.0, IL, M, _dp(w)) == -2
    assert call(5, _dp(d), None, 0.0, 1.0, IL, M, _dp(w)) == -3
    assert call(5, _dp(d), _dp(e), math.nan, 1.0, IL, M, _dp(w)) == -4
    assert call(5, _dp(d), _dp(e), 0.0, math.nan, IL, M, _dp(w)) == -5
    assert call(5, _dp(d), _dp(e), 1.0, 1.0, IL, M, _dp(w)) == -5
    assert call(5, _dp(d), _dp(e), 0.0, 1.0, None, M, _dp(w)) == -6
    assert call(5, _dp(d), _dp(e), 0.0, 1.0, IL, None, _dp(w)) == -7
    assert call(5, _dp(d), _dp(e), 0.0, 1.0, IL, M, None) == -8
    dn = d.copy(); dn[2] = np.nan
    assert call(5, _dp(dn), _dp(e), 0.0, 1.0, IL, M, _dp(w)) == -2
    en = e.copy(); en[1] = -np.inf
    assert call(5, _dp(d), _dp(en), -INF, INF, IL, M, _dp(w)) == -3


def test_python_eigenpairs_rejects_mixed_ranges():
    with pytest.raises(ValueError):
        solver.eigenpairs(np.eye(3), il=1, vl=0.0)
