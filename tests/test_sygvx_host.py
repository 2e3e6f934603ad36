"""CPU suite of the DSYGVX-style entries (ek_hip_sygvx*, ek_hip_sygst_ibtype, ek_hip_trmm): the symbols are declared,
exported and bound, types 2 and 3 plan exactly as type 1, and every argument check answers without a GPU (the checks
run before the library touches a device).  No torch in this process (see tests/test_host_logic.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import descriptor as dsc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ek_hip_sygvx_device", "ek_hip_sygvx", "ek_hip_sygst_ibtype", "ek_hip_trmm")
HOOK = "ek_hip_debug_sygvx_workspace_bytes"
INF = math.inf


def test_sygvx_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    assert set(NEW) <= set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    assert HOOK in set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    assert set(NEW) | {HOOK} <= set(solver.EXPORTED_SYMBOLS)
    lib = solver.load_library()
    for name in NEW + (HOOK,):
        assert getattr(lib, name).argtypes is not None, name
    for fn in ("sygvx", "sygst_ibtype", "trmm", "sygvx_workspace_bytes"):
        assert callable(getattr(solver, fn)), fn
    assert lib.ek_hip_version() == 3


SIZES = [256, 1000, 4096, 16384, 32768]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("vectors", [False, True])
@pytest.mark.parametrize("by_value", [False, True])
def test_types_2_and_3_plan_as_type_1(n, vectors, by_value):
    lib = solver.load_library()
    for m in sorted({0, 1, 64, n // 4, n - n // 2, n}):
        if not by_value and vectors and m == 0:
            continue                       # (an index window holds at least one pair)
        ref = lib.ek_hip_debug_window_workspace_bytes(1, n, int(vectors), int(by_value), m)
        assert ref > 0
        for itype in (1, 2, 3):
            got = solver.sygvx_workspace_bytes(itype, n, vectors=vectors, by_value=by_value, m=m)
            assert got == ref, (itype, n, vectors, by_value, m)


def test_sygvx_hook_rejects_bad_arguments():
    lib = solver.load_library()
    for itype in (0, 4, -1):
        assert lib.ek_hip_debug_sygvx_workspace_bytes(itype, 100, 1, 0, 10) == 0
    assert lib.ek_hip_debug_sygvx_workspace_bytes(2, 0, 1, 0, 0) == 0
    assert lib.ek_hip_debug_sygvx_workspace_bytes(3, 100, 2, 0, 10) == 0
    assert lib.ek_hip_debug_sygvx_workspace_bytes(2, 100, 1, 2, 10) == 0
    assert lib.ek_hip_debug_sygvx_workspace_bytes(3, 100, 1, 0, 101) == 0


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_sygvx_argument_checks_without_gpu():
    lib = solver.load_library()
    n = 4
    a = np.eye(n, order="F"); b = np.eye(n, order="F"); w = np.zeros(n); z = np.zeros((n, n), order="F")
    m, f = ctypes.c_int(-7), ctypes.c_int(-7)
    M, F = ctypes.byref(m), ctypes.byref(f)

    def call(itype=2, jobz=1, rng=0, nn=n, vl=0.0, vu=1.0, il=1, iu=n, A=_dp(a), lda=n, B=_dp(b), ldb=n,
             mp=M, fp=F, W=_dp(w), Z=_dp(z), ldz=n, zcap=n):
        return lib.ek_hip_sygvx(itype, jobz, rng, nn, vl, vu, il, iu, A, lda, B, ldb, mp, fp, W, Z, ldz, zcap, None, 0)
    for bad in (0, 4, -1, 99):
        assert call(itype=bad) == -1
        assert call(itype=bad, nn=-1, A=None) == -1                # (itype is argument 1: checked first)
    for itype in (1, 2, 3):
        assert call(itype=itype, jobz=2) == -2
        assert call(itype=itype, rng=2) == -3
        assert call(itype=itype, nn=-1) == -4
        assert call(itype=itype, rng=1, vl=math.nan) == -5
        assert call(itype=itype, rng=1, vl=1.0, vu=1.0) == -6
        assert call(itype=itype, rng=1, vl=INF, vu=INF) == -6
        assert call(itype=itype, il=0) == -7
        assert call(itype=itype, il=3, iu=2) == -8
        assert call(itype=itype, A=None) == -9
        assert call(itype=itype, lda=n - 1) == -10
        assert call(itype=itype, B=None) == -11                    # (B is always referenced)
        assert call(itype=itype, ldb=n - 1) == -12
        assert call(itype=itype, mp=None) == -13
        assert call(itype=itype, fp=None) == -14
        assert call(itype=itype, W=None) == -15
        assert call(itype=itype, Z=None) == -16
        assert call(itype=itype, ldz=n - 1) == -17
        assert call(itype=itype, zcap=-1) == -18
        m.value = -7
        assert call(itype=itype, il=2, iu=4, zcap=2) == -18 and m.value == 3
    # what a call without vectors or with a value window does not reference
    assert call(itype=3, jobz=0, Z=None, ldz=0, zcap=-1, A=None) == -9
    assert call(itype=2, rng=1, il=0, iu=-5, A=None) == -9
    dummy = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks first

    def dcall(itype=3, jobz=1, rng=0, nn=n, vl=0.0, vu=1.0, il=1, iu=n, A=dummy, lda=n, B=dummy, ldb=n,
              mp=M, fp=F, W=dummy, Z=dummy, ldz=n, zcap=n):
        return lib.ek_hip_sygvx_device(itype, jobz, rng, nn, vl, vu, il, iu, A, lda, B, ldb, mp, fp, W, Z, ldz,
                                       zcap, None, 0)
    assert dcall(itype=0) == -1 and dcall(itype=4) == -1
    assert dcall(jobz=3) == -2
    assert dcall(rng=5) == -3
    assert dcall(nn=-2) == -4
    assert dcall(rng=1, vl=math.nan) == -5
    assert dcall(rng=1, vl=0.5, vu=0.5) == -6
    assert dcall(il=0) == -7
    assert dcall(il=2, iu=1) == -8
    assert dcall(A=None) == -9
    assert dcall(lda=1) == -10
    assert dcall(B=None) == -11
    assert dcall(ldb=2) == -12
    assert dcall(mp=None) == -13
    assert dcall(fp=None) == -14
    assert dcall(W=None) == -15
    assert dcall(Z=None) == -16
    assert dcall(ldz=0) == -17
    assert dcall(zcap=-3) == -18
    m.value = -7
    assert dcall(itype=2, il=1, iu=4, zcap=3) == -18 and m.value == 4


def test_the_existing_entries_still_refuse_problem_2():
    lib = solver.load_library()
    n = 4
    a = np.eye(n, order="F"); w = np.zeros(n); z = np.zeros((n, n), order="F")
    m, f = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ek_hip_eigenpairs(2, 1, 0, n, 0.0, 1.0, 1, n, _dp(a), n, _dp(a), n, ctypes.byref(m), ctypes.byref(f),
                                 _dp(w), _dp(z), n, n, None, 0) == -1


def test_stage_entries_argument_checks_without_gpu():
    lib = solver.load_library()
    desc = dsc.descinit(4, 4, 4, 4, 0, 0, 0, 4)
    a = np.zeros((4, 4), order="F")
    ip, dp = _ip(desc), _dp(a)
    bad = desc.copy(); bad[2] = 5
    bp = _ip(bad)
    s = ctypes.c_double(0.0)
    S = ctypes.byref(s)
    sy = lib.ek_hip_sygst_ibtype
    assert sy(0, 4, dp, ip, dp, ip, S) == -1 and sy(4, 4, dp, ip, dp, ip, S) == -1
    assert sy(2, -1, dp, ip, dp, ip, S) == -2
    assert sy(2, 4, None, ip, dp, ip, S) == -3
    assert sy(3, 4, dp, None, dp, ip, S) == -4
    assert sy(3, 4, dp, bp, dp, ip, S) == -403
    assert sy(2, 4, dp, ip, None, ip, S) == -5
    assert sy(2, 4, dp, ip, dp, None, S) == -6
    assert sy(1, 4, dp, ip, dp, bp, S) == -603
    tr = lib.ek_hip_trmm
    assert tr(-1, 4, dp, ip, dp, ip) == -1
    assert tr(4, -1, dp, ip, dp, ip) == -2
    assert tr(4, 4, None, ip, dp, ip) == -3
    assert tr(4, 4, dp, bp, dp, ip) == -403
    assert tr(4, 4, dp, ip, None, ip) == -5
    assert tr(4, 4, dp, ip, dp, None) == -6
    assert tr(4, 4, dp, ip, dp, bp) == -603
    narrow = dsc.descinit(4, 2, 4, 4, 0, 0, 0, 4)
    assert tr(4, 3, dp, ip, dp, _ip(narrow)) == -604


def test_python_sygvx_rejects_mixed_ranges():
    with pytest.raises(ValueError):
        solver.sygvx(np.eye(3), np.eye(3), itype=2, il=1, vl=0.0)
