"""Host-side checks of the batched entries (ek_hip_eigenpairs_batched*): declared in the boundary header, exported,
bound by the Python mirror, and every argument error decided before any device work (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_eigenpairs_batched_device", "ek_hip_eigenpairs_batched")


def test_batched_entries_declared_exported_and_bound():
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
    m = re.search(r"#define\s+EK_HIP_BATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 128 == solver.BATCH_NMAX
    assert callable(solver.eigenpairs_batched)
    assert lib.ek_hip_version() == 3


@pytest.mark.parametrize("name", NAMES)
def test_batched_argument_errors_without_gpu(name):
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

    def call(problem=1, jobz=1, n=n, batch=batch, A=p, lda=n, sA=n * n, B=p, ldb=n, sB=n * n, w=p, Z=p, ldz=n,
             sZ=n * n, info=ip):
        return fn(problem, jobz, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, None)

    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(jobz=2) == -2
    assert call(n=-1) == -3
    assert call(n=129, lda=129, ldb=129, ldz=129, sA=129 * 129, sB=129 * 129, sZ=129 * 129) == -3
    assert call(batch=-1) == -4
    assert call(A=None) == -5
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
    assert call(n=129, batch=-1) == -3
    # nothing to do: success without a device and without touching any pointer
    assert call(batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
    assert call(n=0, A=None, B=None, w=None, Z=None, info=None) == 0
    # what is not referenced is not checked
    assert call(problem=0, B=None, ldb=0, sB=0, A=None) == -5
    assert call(jobz=0, Z=None, ldz=0, sZ=0, A=None) == -5
    assert not info.any() and not buf.any()


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_batched(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        solver.eigenpairs_batched(np.zeros((2, 4, 4)), np.zeros((2, 3, 3)))
    w, Z, info = solver.eigenpairs_batched(np.zeros((0, 4, 4)))
    assert w.shape == (0, 4) and Z.shape == (0, 4, 4) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_batched(np.zeros((1, 129, 129)))
    assert ei.value.info == -3
