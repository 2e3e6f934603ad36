"""Host-side checks of the entries for orders up to 256 (ek_hip_eigenpairs_xbatched*): declared in the boundary header,
exported, bound by the Python mirror, and every argument error decided before any device work (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_eigenpairs_xbatched_device", "ek_hip_eigenpairs_xbatched")
HOOK = "ek_hip_debug_xbatched_chunk"


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return hdr, dbg, set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_xbatched_entries_declared_exported_and_bound():
    hdr, _, declared, hooks = _headers()
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
    m = re.search(r"#define\s+EK_HIP_XBATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 256 == solver.XBATCH_NMAX
    m = re.search(r"#define\s+EK_HIP_BATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 128 == solver.BATCH_NMAX
    assert callable(solver.eigenpairs_xbatched)
    assert lib.ek_hip_version() == 3


def test_chunk_hook_is_a_debug_entry():
    _, _, declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    fn = getattr(solver.load_library(), HOOK)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_int]
    # host state only: the previous value comes back, 0 restores the default
    default = solver.xbatched_chunk(7)
    try:
        assert default == 1024
        assert solver.xbatched_chunk(3) == 7
    finally:
        assert solver.xbatched_chunk(0) == 3
    assert solver.xbatched_chunk(0) == 1024


@pytest.mark.parametrize("name", NAMES)
def test_xbatched_argument_errors_without_gpu(name):
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

    def call(problem=1, jobz=1, n=n, batch=batch, A=p, lda=None, sA=None, B=p, ldb=None, sB=None, w=p, Z=p, ldz=None,
             sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        sA, sB, sZ = (ld * ld if x is None else x for x in (sA, sB, sZ))
        return fn(problem, jobz, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, None)

    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(jobz=2) == -2
    assert call(n=-1) == -3
    assert call(n=257) == -3
    assert call(batch=-1) == -4
    assert call(A=None) == -5
    # orders 129 .. 256 are legal: the next argument decides, and no device is touched
    for big in (129, 200, 256):
        assert call(n=big, A=None) == -5
        assert call(n=big, lda=big - 1) == -6
        assert call(n=big, sA=big * big - 1) == -7
        assert call(n=big, info=None) == -15
    assert call(lda=n - 1) == -6
    assert call(sA=n * n - 1) == -7
    assert call(sA=0) == -7                       # no broadcast
    assert call(lda=n + 2, sA=n * n) == -7        # the stride follows the leading dimension
    assert call(B=None) == -8
    assert call(ldb=n - 1) == -9
    assert call(sB=n * n - 1) == -10
    assert call(w=None) == -11
    assert call(Z=None) == -12
    assert call(ldz=n - 1) == -13
    assert call(sZ=n * n - 1) == -14
    assert call(info=None) == -15
    # the first offending argument decides
    assert call(problem=2, jobz=2, n=-1) == -1
    assert call(n=257, batch=-1) == -3
    assert call(n=129, batch=-1) == -4
    assert call(jobz=3, n=257) == -2
    # nothing to do: success without a device and without touching any pointer
    assert call(batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
    assert call(n=0, A=None, B=None, w=None, Z=None, info=None) == 0
    assert call(n=200, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
    # what is not referenced is not checked
    assert call(problem=0, B=None, ldb=0, sB=0, A=None) == -5
    assert call(jobz=0, Z=None, ldz=0, sZ=0, A=None) == -5
    assert call(n=130, problem=0, B=None, ldb=0, sB=0, A=None) == -5
    assert not info.any() and not buf.any()


def test_the_old_entries_still_stop_at_128():
    lib = solver.load_library()
    info = np.zeros(1, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.ek_hip_eigenpairs_batched(0, 0, 129, 1, None, 129, 129 * 129, None, 129, 129 * 129, None, None, 129,
                                         129 * 129, ip, None) == -3
    assert lib.ek_hip_sygv_batched(1, 0, 129, 1, None, 129, 129 * 129, None, 129, 129 * 129, None, None, 129,
                                   129 * 129, ip, None) == -3


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_xbatched(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        solver.eigenpairs_xbatched(np.zeros((2, 4, 4)), np.zeros((2, 3, 3)))
    w, Z, info = solver.eigenpairs_xbatched(np.zeros((0, 200, 200)))
    assert w.shape == (0, 200) and Z.shape == (0, 200, 200) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_xbatched(np.zeros((1, 257, 257)))
    assert ei.value.info == -3
