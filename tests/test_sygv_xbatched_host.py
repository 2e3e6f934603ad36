"""Host-side checks of DSYGV's three problem types at orders up to 256 (ek_hip_sygv_xbatched*): declared in the boundary
header, exported, bound by the Python mirror, and every argument error decided before any device work (no GPU needed).
Modelled on tests/test_xbatched_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_sygv_xbatched_device", "ek_hip_sygv_xbatched")


def test_sygv_xbatched_entries_declared_exported_and_bound():
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
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
        assert fn.argtypes[6] is ctypes.c_longlong and fn.argtypes[9] is ctypes.c_longlong
        assert fn.argtypes[13] is ctypes.c_longlong
    assert callable(solver.sygv_xbatched)
    assert lib.ek_hip_version() == 3              # the symbols are the signal


def test_python_mirror_rejects_before_the_library():
    A = np.zeros((2, 130, 130))
    for itype in (0, 4):
        with pytest.raises(ValueError):
            solver.sygv_xbatched(A, A, itype=itype)
    with pytest.raises(ValueError):
        solver.sygv_xbatched(A, None)
    with pytest.raises(ValueError):
        solver.sygv_xbatched(A, None, itype=2)
    with pytest.raises(ValueError):
        solver.sygv_xbatched(np.zeros((3, 4)), np.zeros((3, 4)), itype=2)
    w, Z, info = solver.sygv_xbatched(np.zeros((0, 200, 200)), np.zeros((0, 200, 200)), itype=3)
    assert w.shape == (0, 200) and Z.shape == (0, 200, 200) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.sygv_xbatched(np.zeros((1, 257, 257)), np.zeros((1, 257, 257)), itype=2)
    assert ei.value.info == -3


@pytest.mark.parametrize("name", NAMES)
def test_sygv_xbatched_argument_errors_without_gpu(name):
    """-k for argument k, before any device work: pointers are never dereferenced here (the device form gets host
    addresses, and there may be no GPU at all)."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    n, batch = 4, 3
    buf = np.zeros(batch * n * n)
    info = np.zeros(batch, dtype=np.int32)
    if name.endswith("_device"):
        p = ctypes.c_void_p(buf.ctypes.data)
    else:
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def call(itype=2, jobz=1, n=n, batch=batch, A=p, lda=None, sA=None, B=p, ldb=None, sB=None, w=p, Z=p, ldz=None,
             sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        sA, sB, sZ = (ld * ld if x is None else x for x in (sA, sB, sZ))
        return fn(itype, jobz, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, None)

    assert call(itype=0) == -1
    assert call(itype=4) == -1
    assert call(itype=0, n=200) == -1
    for itype in (1, 2, 3):
        assert call(itype=itype, jobz=2) == -2
        assert call(itype=itype, n=-1) == -3
        assert call(itype=itype, n=257) == -3
        assert call(itype=itype, batch=-1) == -4
        assert call(itype=itype, A=None) == -5
        assert call(itype=itype, lda=n - 1) == -6
        assert call(itype=itype, sA=n * n - 1) == -7
        # B is always required, for itype 1 too
        assert call(itype=itype, B=None) == -8
        assert call(itype=itype, ldb=n - 1) == -9
        assert call(itype=itype, sB=0) == -10
        assert call(itype=itype, sB=n * n - 1) == -10
        assert call(itype=itype, ldb=n + 2, sB=n * n) == -10
        assert call(itype=itype, w=None) == -11
        assert call(itype=itype, Z=None) == -12
        assert call(itype=itype, ldz=n - 1) == -13
        assert call(itype=itype, sZ=n * n - 1) == -14
        assert call(itype=itype, info=None) == -15
        # orders 129 .. 256 are legal: the next argument decides, and no device is touched
        for big in (129, 200, 256):
            assert call(itype=itype, n=big, info=None) == -15
            assert call(itype=itype, n=big, jobz=0, Z=None, ldz=0, sZ=0, info=None) == -15
            assert call(itype=itype, n=big, B=None) == -8
            assert call(itype=itype, n=big, ldb=big - 1) == -9
            assert call(itype=itype, n=big, sB=0) == -10
            assert call(itype=itype, n=big, sB=big * big - 1) == -10
        # nothing to do: success without a device and without touching any pointer
        assert call(itype=itype, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
        assert call(itype=itype, n=0, A=None, B=None, w=None, Z=None, info=None) == 0
        assert call(itype=itype, n=200, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
    # the first offending argument decides
    assert call(itype=4, jobz=2, n=-1) == -1
    assert call(jobz=3, n=257) == -2
    assert call(n=257, batch=-1) == -3
    assert call(n=129, batch=-1) == -4
    assert call(A=None, B=None) == -5
    assert not info.any() and not buf.any()


def test_the_old_sygv_entries_still_stop_at_128():
    lib = solver.load_library()
    info = np.zeros(1, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for itype in (1, 2, 3):
        for fn in (lib.ek_hip_sygv_batched, lib.ek_hip_sygv_batched_device):
            assert fn(itype, 0, 129, 1, None, 129, 129 * 129, None, 129, 129 * 129, None, None, 129, 129 * 129, ip,
                      None) == -3
    assert not info.any()
