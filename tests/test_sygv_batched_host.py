"""Host-side checks of the batched entries for DSYGV's three problem types (ek_hip_sygv_batched*, ek_hip_sygv_vbatched*):
declared in the boundary header with the prototypes of the eigenpairs forms (itype in the place of problem), exported,
bound by the Python mirror, and every argument error decided before any device work and without dereferencing a data
pointer (no GPU needed: the device forms get host addresses)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIFORM = ("ek_hip_sygv_batched_device", "ek_hip_sygv_batched")
VARIABLE = ("ek_hip_sygv_vbatched_device", "ek_hip_sygv_vbatched")
_ip = ctypes.POINTER(ctypes.c_int)


def _prototype(hdr, name):
    """The argument list of `name` in the header: types and names, white space and the `d` of device names dropped."""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return [re.sub(r"\bd([ABwZ])\b", r"\1", a) for a in args]


def test_sygv_batched_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in UNIFORM + VARIABLE:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        twin = name.replace("ek_hip_sygv_", "ek_hip_eigenpairs_")
        fn, fn_twin = getattr(lib, name), getattr(lib, twin)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(fn_twin.argtypes)
        assert len(fn.argtypes) == (16 if name in UNIFORM else 13)
        # argument for argument the prototype of the eigenpairs form, with itype in the place of problem
        mine, theirs = _prototype(hdr, name), _prototype(hdr, twin)
        assert mine[0] == "int itype" and theirs[0] == "int problem"
        assert mine[1:] == theirs[1:], (name, mine, theirs)
    assert callable(solver.sygv_batched) and callable(solver.sygv_vbatched)
    assert lib.ek_hip_version() == 3
    m = re.search(r"#define\s+EK_HIP_BATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == solver.BATCH_NMAX


@pytest.mark.parametrize("name", UNIFORM)
def test_sygv_batched_argument_errors_without_gpu(name):
    """-k for argument k in argument order, the first offender deciding; B is required for every itype."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    n, batch = 4, 3
    buf = np.zeros(batch * n * n)
    info = np.zeros(batch, dtype=np.int32)
    if name.endswith("_device"):
        p = ctypes.c_void_p(buf.ctypes.data)
    else:
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = info.ctypes.data_as(_ip)

    def call(itype=2, jobz=1, n=n, batch=batch, A=p, lda=n, sA=n * n, B=p, ldb=n, sB=n * n, w=p, Z=p, ldz=n,
             sZ=n * n, info=ip):
        return fn(itype, jobz, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, None)

    for bad in (0, 4, -1):
        assert call(itype=bad) == -1
    for itype in (1, 2, 3):
        assert call(itype=itype, jobz=2) == -2
        assert call(itype=itype, jobz=-1) == -2
        assert call(itype=itype, n=-1) == -3
        assert call(itype=itype, n=129, lda=129, ldb=129, ldz=129, sA=129 * 129, sB=129 * 129, sZ=129 * 129) == -3
        assert call(itype=itype, batch=-1) == -4
        assert call(itype=itype, A=None) == -5
        assert call(itype=itype, lda=n - 1) == -6
        assert call(itype=itype, sA=n * n - 1) == -7
        assert call(itype=itype, sA=0) == -7
        assert call(itype=itype, lda=n + 2, sA=n * n) == -7
        assert call(itype=itype, B=None) == -8
        assert call(itype=itype, ldb=n - 1) == -9
        assert call(itype=itype, sB=n * n - 1) == -10
        assert call(itype=itype, sB=0) == -10
        assert call(itype=itype, w=None) == -11
        assert call(itype=itype, Z=None) == -12
        assert call(itype=itype, ldz=n - 1) == -13
        assert call(itype=itype, sZ=n * n - 1) == -14
        assert call(itype=itype, info=None) == -15
        # the first offending argument decides
        assert call(itype=itype, jobz=2, n=-1) == -2
        assert call(itype=itype, n=129, batch=-1) == -3
        assert call(itype=itype, A=None, B=None) == -5
        assert call(itype=itype, B=None, ldb=0, sB=0, w=None) == -8
        assert call(itype=itype, ldb=0, sB=0) == -9
        # values only: Z is not looked at, B still is
        assert call(itype=itype, jobz=0, Z=None, ldz=0, sZ=0, info=None) == -15
        assert call(itype=itype, jobz=0, Z=None, ldz=0, sZ=0, B=None) == -8
        # nothing to do: success without a device and without touching any pointer
        assert call(itype=itype, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
        assert call(itype=itype, n=0, A=None, B=None, w=None, Z=None, info=None) == 0
    assert call(itype=0, jobz=2, n=-1, B=None) == -1
    assert call(itype=4, batch=0) == -1             # a bad itype is an error even where there is nothing to do
    assert not info.any() and not buf.any()


@pytest.mark.parametrize("name", VARIABLE)
def test_sygv_vbatched_argument_errors_without_gpu(name):
    """-k for argument k of the variable prototype; the data pointers are host addresses of buffers that must come back
    untouched."""
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

    def call(itype=3, jobz=1, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok",
             ldz=ld_ok, info=info):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(_ip)
        return fn(itype, jobz, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info), None)

    for bad in (0, 4, -1):
        assert call(itype=bad) == -1
    for itype in (1, 2, 3):
        assert call(itype=itype, jobz=2) == -2
        assert call(itype=itype, batch=-1) == -3
        assert call(itype=itype, n=None) == -4
        assert call(itype=itype, n=ints([4, -1, 3])) == -4
        assert call(itype=itype, n=ints([4, 0, 129]), lda=ints([4, 1, 129]), ldb=ints([4, 1, 129]),
                    ldz=ints([4, 1, 129])) == -4
        assert call(itype=itype, A=None) == -5
        assert call(itype=itype, A=ptrs(null_at=2)) == -5
        assert call(itype=itype, lda=None) == -6
        assert call(itype=itype, lda=ints([3, 1, 3])) == -6
        assert call(itype=itype, B=None) == -7
        assert call(itype=itype, B=ptrs(null_at=0)) == -7
        assert call(itype=itype, ldb=None) == -8
        assert call(itype=itype, ldb=ints([4, 1, 2])) == -8
        assert call(itype=itype, w=None) == -9
        assert call(itype=itype, w=ptrs(null_at=2)) == -9
        assert call(itype=itype, Z=None) == -10
        assert call(itype=itype, Z=ptrs(null_at=0)) == -10
        assert call(itype=itype, ldz=None) == -11
        assert call(itype=itype, ldz=ints([4, 1, 2])) == -11
        assert call(itype=itype, info=None) == -12
        # a NULL entry is legal where the problem is empty
        assert call(itype=itype, A=ptrs(null_at=1), B=ptrs(null_at=1), w=ptrs(null_at=1), Z=ptrs(null_at=1),
                    info=None) == -12
        # the first offending argument decides
        assert call(itype=itype, jobz=3, n=None) == -2
        assert call(itype=itype, batch=-1, n=None, A=None) == -3
        assert call(itype=itype, n=ints([4, 0, 200]), A=None) == -4
        assert call(itype=itype, lda=ints([1, 1, 1]), B=None, info=None) == -6
        assert call(itype=itype, B=None, ldb=None, w=None) == -7
        assert call(itype=itype, jobz=0, Z=None, ldz=None, B=None) == -7
        assert call(itype=itype, jobz=0, Z=None, ldz=None, info=None) == -12
        # nothing to do
        assert call(itype=itype, batch=0, n=None, A=None, lda=None, B=None, ldb=None, w=None, Z=None, ldz=None,
                    info=None) == 0
    assert call(itype=0, jobz=2, batch=-1) == -1
    assert np.all(info == 777)
    for b in bufs:
        assert np.all(b == 3.5)


@pytest.mark.parametrize("name", VARIABLE)
def test_sygv_vbatched_all_orders_zero_needs_no_device(name):
    lib = solver.load_library()
    fn = getattr(lib, name)
    batch = 3
    n = np.zeros(batch, dtype=np.int32)
    ld = np.ones(batch, dtype=np.int32)
    null = (ctypes.c_void_p * batch)()
    for itype in (1, 2, 3):
        info = np.full(batch, 777, dtype=np.int32)
        sec = ctypes.c_double(-1.0)
        rc = fn(itype, 1, batch, n.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null,
                null, ld.ctypes.data_as(_ip), info.ctypes.data_as(_ip), ctypes.byref(sec))
        assert rc == 0 and not info.any() and sec.value == 0.0


def test_python_mirrors_reject_bad_arguments_before_the_library():
    A, B = np.zeros((2, 4, 4)), np.zeros((2, 4, 4))
    for itype in (0, 4, None, 2.5):
        with pytest.raises(ValueError):
            solver.sygv_batched(A, B, itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_vbatched(list(A), list(B), itype=itype)
    for itype in (1, 2, 3):
        with pytest.raises(ValueError):
            solver.sygv_batched(A, None, itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_vbatched(list(A), None, itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_batched(np.zeros((3, 4)), np.zeros((3, 4)), itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_batched(A, np.zeros((2, 3, 3)), itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_vbatched([np.zeros((4, 4)), np.zeros((3, 3))], [np.zeros((4, 4))], itype=itype)
        with pytest.raises(ValueError):
            solver.sygv_vbatched([np.zeros((3, 4))], [np.zeros((3, 4))], itype=itype)
        # nothing to do: decided on the host
        w, Z, info = solver.sygv_batched(np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), itype=itype)
        assert w.shape == (0, 4) and Z.shape == (0, 4, 4) and info.shape == (0,)
        w, Z, info = solver.sygv_batched(np.zeros((3, 0, 0)), np.zeros((3, 0, 0)), itype=itype, vectors=False)
        assert w.shape == (3, 0) and Z is None and not info.any()
        w, Z, info = solver.sygv_vbatched([], [], itype=itype)
        assert w == [] and Z == [] and info.shape == (0,)
        w, Z, info = solver.sygv_vbatched([np.zeros((0, 0))] * 2, [np.zeros((0, 0))] * 2, itype=itype)
        assert [x.shape for x in w] == [(0,)] * 2 and [x.shape for x in Z] == [(0, 0)] * 2 and not info.any()
        with pytest.raises(solver.SolverError) as ei:
            solver.sygv_batched(np.zeros((1, 129, 129)), np.zeros((1, 129, 129)), itype=itype)
        assert ei.value.info == -3
        with pytest.raises(solver.SolverError) as ei:
            solver.sygv_vbatched([np.zeros((129, 129))], [np.zeros((129, 129))], itype=itype)
        assert ei.value.info == -4
