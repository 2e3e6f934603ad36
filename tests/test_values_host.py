"""CPU suite of the eigenvalues-only interface (ek_hip_eigenvalues*, ek_hip_stebz): the symbols are exported and
bound, the values-only plan leaves out at least the eigenvector array, and the argument checks answer without a GPU
(they run before the library touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ek_hip_eigenvalues_device", "ek_hip_eigenvalues", "ek_hip_stebz")


def test_new_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    boundary = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    assert set(NEW) <= boundary
    assert "ek_hip_debug_values_workspace_bytes" in hooks
    assert set(NEW) | {"ek_hip_debug_values_workspace_bytes"} <= set(solver.EXPORTED_SYMBOLS)
    lib = solver.load_library()
    for name in NEW + ("ek_hip_debug_values_workspace_bytes", "ek_hip_debug_set_stebz"):
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ek_hip_version() == 3


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [256, 4096, 16384, 32768])
def test_values_plan_reserves_no_eigenvector_array(problem, n):
    full, _ = solver.workspace_bytes(problem, n, n_vec=n, nranks=1)
    vals = solver.values_workspace_bytes(problem, n)
    ld = (n + 127) // 128 * 128
    assert 0 < vals <= full - ld * ld * 8, (vals, full)


def test_values_workspace_bytes_rejects_bad_arguments():
    lib = solver.load_library()
    assert lib.ek_hip_debug_values_workspace_bytes(2, 100) == 0
    assert lib.ek_hip_debug_values_workspace_bytes(0, 0) == 0


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_eigenvalues_argument_checks_without_gpu():
    lib = solver.load_library()
    a = np.eye(4, order="F"); b = np.eye(4, order="F"); w = np.zeros(4)
    call = lambda *args: lib.ek_hip_eigenvalues(*args, None, 0)
    assert call(2, 4, 1, 4, _dp(a), 4, _dp(b), 4, _dp(w)) == -1
    assert call(0, -1, 1, 1, _dp(a), 4, None, 1, _dp(w)) == -2
    assert call(0, 4, 0, 4, _dp(a), 4, None, 1, _dp(w)) == -3
    assert call(0, 4, 5, 5, _dp(a), 4, None, 1, _dp(w)) == -3
    assert call(0, 4, 3, 2, _dp(a), 4, None, 1, _dp(w)) == -4
    assert call(0, 4, 1, 5, _dp(a), 4, None, 1, _dp(w)) == -4
    assert call(0, 4, 1, 4, None, 4, None, 1, _dp(w)) == -5
    assert call(0, 4, 1, 4, _dp(a), 3, None, 1, _dp(w)) == -6
    assert call(1, 4, 1, 4, _dp(a), 4, None, 4, _dp(w)) == -7
    assert call(1, 4, 1, 4, _dp(a), 4, _dp(b), 2, _dp(w)) == -8
    assert call(0, 4, 1, 4, _dp(a), 4, None, 1, None) == -9
    dcall = lambda *args: lib.ek_hip_eigenvalues_device(*args, None, 0)
    dummy = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks first
    assert dcall(2, 4, 1, 4, dummy, 4, dummy, 4, dummy) == -1
    assert dcall(0, -3, 1, 1, dummy, 4, None, 1, dummy) == -2
    assert dcall(0, 4, 0, 4, dummy, 4, None, 1, dummy) == -3
    assert dcall(0, 4, 2, 1, dummy, 4, None, 1, dummy) == -4
    assert dcall(0, 4, 1, 4, None, 4, None, 1, dummy) == -5
    assert dcall(0, 4, 1, 4, dummy, 2, None, 1, dummy) == -6
    assert dcall(1, 4, 1, 4, dummy, 4, None, 4, dummy) == -7
    assert dcall(1, 4, 1, 4, dummy, 4, dummy, 3, dummy) == -8
    assert dcall(0, 4, 1, 4, dummy, 4, None, 1, None) == -9


def test_stebz_argument_checks_without_gpu():
    lib = solver.load_library()
    d = np.ones(5); e = np.ones(5); w = np.zeros(5)
    assert lib.ek_hip_stebz(-1, _dp(d), _dp(e), 1, 1, _dp(w)) == -1
    assert lib.ek_hip_stebz(5, None, _dp(e), 1, 5, _dp(w)) == -2
    assert lib.ek_hip_stebz(5, _dp(d), None, 1, 5, _dp(w)) == -3
    assert lib.ek_hip_stebz(5, _dp(d), _dp(e), 0, 5, _dp(w)) == -4
    assert lib.ek_hip_stebz(5, _dp(d), _dp(e), 6, 6, _dp(w)) == -4
    assert lib.ek_hip_stebz(5, _dp(d), _dp(e), 3, 2, _dp(w)) == -5
    assert lib.ek_hip_stebz(5, _dp(d), _dp(e), 1, 6, _dp(w)) == -5
    assert lib.ek_hip_stebz(5, _dp(d), _dp(e), 1, 5, None) == -6
    dn = d.copy(); dn[2] = np.nan
    assert lib.ek_hip_stebz(5, _dp(dn), _dp(e), 1, 5, _dp(w)) == -2
    en = e.copy(); en[1] = np.inf
    assert lib.ek_hip_stebz(5, _dp(d), _dp(en), 1, 5, _dp(w)) == -3
