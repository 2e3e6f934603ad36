"""Host-side checks of the variable-order batched entries (ek_hip_eigenpairs_vbatched*): declared in the boundary
header, exported, bound by the Python mirror, and every argument error decided before any device work and without
dereferencing a data pointer (no GPU needed: both forms get host addresses in their pointer arrays)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_eigenpairs_vbatched_device", "ek_hip_eigenpairs_vbatched")
_ip = ctypes.POINTER(ctypes.c_int)


def test_vbatched_entries_declared_exported_and_bound():
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
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert callable(solver.eigenpairs_vbatched)
    assert lib.ek_hip_version() == 3


@pytest.mark.parametrize("name", NAMES)
def test_vbatched_argument_errors_without_gpu(name):
    """-k for argument k of the prototype, the first offender deciding.  The data pointers are host addresses of
    buffers whose contents must come back untouched; for the device form they would fault if they were used."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    orders = np.array([4, 0, 3], dtype=np.int32)
    batch = len(orders)
    bufs = [np.full(16, 3.5) for _ in range(batch)]
    info = np.full(batch, 777, dtype=np.int32)

    def ptrs(null_at=None):
        return (ctypes.c_void_p * batch)(*[None if b == null_at else bufs[b].ctypes.data for b in range(batch)])

    def ints(v):
        return np.array(v, dtype=np.int32)

    ld_ok = ints([4, 1, 3])
    keep = []

    def call(problem=1, jobz=1, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok",
             ldz=ld_ok, info=info):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(_ip)
        return fn(problem, jobz, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info), None)

    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(jobz=2) == -2
    assert call(jobz=-1) == -2
    assert call(batch=-1) == -3
    assert call(n=None) == -4
    assert call(n=ints([4, -1, 3])) == -4
    assert call(n=ints([4, 0, 129]), lda=ints([4, 1, 129]), ldb=ints([4, 1, 129]), ldz=ints([4, 1, 129])) == -4
    assert call(A=None) == -5
    assert call(A=ptrs(null_at=2)) == -5
    assert call(lda=None) == -6
    assert call(lda=ints([3, 1, 3])) == -6
    assert call(lda=ints([4, 0, 3])) == -6           # lda[b] >= max(1, n[b]) also for an empty problem
    assert call(B=None) == -7
    assert call(B=ptrs(null_at=0)) == -7
    assert call(ldb=None) == -8
    assert call(ldb=ints([4, 1, 2])) == -8
    assert call(w=None) == -9
    assert call(w=ptrs(null_at=2)) == -9
    assert call(Z=None) == -10
    assert call(Z=ptrs(null_at=0)) == -10
    assert call(ldz=None) == -11
    assert call(ldz=ints([4, 1, 2])) == -11
    assert call(info=None) == -12
    # a NULL entry is legal where the problem is empty: the next offender decides
    assert call(A=ptrs(null_at=1), B=ptrs(null_at=1), w=ptrs(null_at=1), Z=ptrs(null_at=1), info=None) == -12
    # the first offending argument decides
    assert call(problem=2, jobz=2, batch=-1) == -1
    assert call(jobz=3, n=None) == -2
    assert call(batch=-1, n=None, A=None) == -3
    assert call(n=ints([4, 0, 200]), A=None) == -4
    assert call(A=ptrs(null_at=0), lda=ints([1, 1, 1]), info=None) == -5
    assert call(lda=ints([1, 1, 1]), B=None, info=None) == -6
    assert call(B=None, ldb=None, w=None) == -7
    assert call(w=None, Z=None, info=None) == -9
    # what is not referenced is not looked at
    assert call(problem=0, B=None, ldb=None, info=None) == -12
    assert call(jobz=0, Z=None, ldz=None, info=None) == -12
    assert call(problem=0, B=None, ldb=ints([0, 0, 0]), w=None) == -9
    # nothing to do: success without a device and without touching any pointer
    assert call(batch=0, n=None, A=None, lda=None, B=None, ldb=None, w=None, Z=None, ldz=None, info=None) == 0
    assert np.all(info == 777)
    for b in bufs:
        assert np.all(b == 3.5)


@pytest.mark.parametrize("name", NAMES)
def test_vbatched_all_orders_zero_needs_no_device(name):
    """Every problem empty: info[b] = 0, success, no pointer looked at (NULL entries everywhere)."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    batch = 3
    n = np.zeros(batch, dtype=np.int32)
    ld = np.ones(batch, dtype=np.int32)
    info = np.full(batch, 777, dtype=np.int32)
    null = (ctypes.c_void_p * batch)()
    sec = ctypes.c_double(-1.0)
    rc = fn(1, 1, batch, n.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null, null,
            ld.ctypes.data_as(_ip), info.ctypes.data_as(_ip), ctypes.byref(sec))
    assert rc == 0 and not info.any() and sec.value == 0.0


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_vbatched([np.zeros((3, 4))])
    with pytest.raises(ValueError):
        solver.eigenpairs_vbatched([np.zeros((2, 4, 4))])
    with pytest.raises(ValueError):
        solver.eigenpairs_vbatched([np.zeros(4)])
    with pytest.raises(ValueError):
        solver.eigenpairs_vbatched([np.zeros((4, 4)), np.zeros((3, 3))], [np.zeros((4, 4)), np.zeros((4, 4))])
    with pytest.raises(ValueError):
        solver.eigenpairs_vbatched([np.zeros((4, 4)), np.zeros((3, 3))], [np.zeros((4, 4))])
    w, Z, info = solver.eigenpairs_vbatched([])
    assert w == [] and Z == [] and info.shape == (0,)
    w, Z, info = solver.eigenpairs_vbatched([], [], vectors=False)
    assert w == [] and Z is None and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_vbatched([np.zeros((4, 4)), np.zeros((129, 129))])
    assert ei.value.info == -4
    # every problem empty: decided on the host
    w, Z, info = solver.eigenpairs_vbatched([np.zeros((0, 0))] * 2)
    assert [x.shape for x in w] == [(0,)] * 2 and [x.shape for x in Z] == [(0, 0)] * 2 and not info.any()
