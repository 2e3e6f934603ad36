"""Host-side checks of the variable-order batched entries for orders up to EK_HIP_XBATCH_NMAX (ek_hip_eigenpairs_xvbatched*,
ek_hip_sygv_xvbatched*): declared in the boundary header, exported, bound by the Python mirror, and every argument error
decided before any device work and without dereferencing a data pointer, with an order above EK_HIP_BATCH_NMAX present
(no GPU needed: both forms get host addresses in their pointer arrays).  The pattern is test_vbatched_host.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG = ("ek_hip_eigenpairs_xvbatched_device", "ek_hip_eigenpairs_xvbatched")
SYGV = ("ek_hip_sygv_xvbatched_device", "ek_hip_sygv_xvbatched")
OLD = ("ek_hip_eigenpairs_vbatched_device", "ek_hip_eigenpairs_vbatched", "ek_hip_sygv_vbatched_device",
       "ek_hip_sygv_vbatched")
HOOK = "ek_hip_debug_xvbatched_last"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
NB = 200                                                # the order above EK_HIP_BATCH_NMAX every batch here holds


def test_xvbatched_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in EIG + SYGV:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        twin = getattr(lib, name.replace("xvbatched", "vbatched"))
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
        assert list(fn.argtypes) == list(twin.argtypes)
    assert HOOK in hooks and HOOK not in declared and HOOK in solver.EXPORTED_SYMBOLS and hasattr(raw, HOOK)
    hook = getattr(lib, HOOK)
    assert hook.restype is ctypes.c_int and list(hook.argtypes) == [_dp, _ip]
    assert callable(solver.eigenpairs_xvbatched) and callable(solver.sygv_xvbatched)
    assert lib.ek_hip_version() == 3
    assert solver.BATCH_NMAX == 128 and solver.XBATCH_NMAX == 256


def test_last_call_hook_answers_without_a_device():
    """Host state only: four seconds and four counts (classes of 256, 128, 64, 32), either pointer may be NULL; the old
    hook keeps its three."""
    lib = solver.load_library()
    sec, cnt = np.full(5, -1.0), np.full(5, -1, dtype=np.int32)
    assert lib.ek_hip_debug_xvbatched_last(sec.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip)) == 0
    assert np.all(sec[:4] >= 0.0) and np.all(cnt[:4] >= 0) and sec[4] == -1.0 and cnt[4] == -1
    assert lib.ek_hip_debug_xvbatched_last(None, None) == 0
    sec3, cnt3 = np.full(4, -1.0), np.full(4, -1, dtype=np.int32)
    assert lib.ek_hip_debug_vbatched_last(sec3.ctypes.data_as(_dp), cnt3.ctypes.data_as(_ip)) == 0
    assert sec3[3] == -1.0 and cnt3[3] == -1
    assert np.array_equal(sec3[:3], sec[1:4]) and np.array_equal(cnt3[:3], cnt[1:4])


@pytest.mark.parametrize("name", EIG + SYGV)
def test_xvbatched_argument_errors_without_gpu(name):
    """-k for argument k of the prototype, the first offender deciding.  The data pointers are host addresses of small
    buffers whose contents must come back untouched; they would fault if the order-200 problem were touched."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    sygv = name in SYGV
    orders = np.array([4, 0, NB], dtype=np.int32)
    batch = len(orders)
    bufs = [np.full(16, 3.5) for _ in range(batch)]
    info = np.full(batch, 777, dtype=np.int32)

    def ptrs(null_at=None):
        return (ctypes.c_void_p * batch)(*[None if b == null_at else bufs[b].ctypes.data for b in range(batch)])

    def ints(v):
        return np.array(v, dtype=np.int32)

    ld_ok = ints([4, 1, NB])
    keep = []

    def call(first=1, jobz=1, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok",
             ldz=ld_ok, info=info):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(_ip)
        return fn(first, jobz, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info), None)

    if sygv:
        assert call(first=0) == -1
        assert call(first=4) == -1
        for itype in (1, 2, 3):
            assert call(first=itype, info=None) == -12
    else:
        assert call(first=2) == -1
        assert call(first=-1) == -1
    assert call(jobz=2) == -2
    assert call(jobz=-1) == -2
    assert call(batch=-1) == -3
    assert call(n=None) == -4
    assert call(n=ints([4, -1, NB])) == -4
    assert call(n=ints([4, 0, 257]), lda=ints([4, 1, 257]), ldb=ints([4, 1, 257]), ldz=ints([4, 1, 257])) == -4
    for edge in (129, 256):                             # legal orders: the next offender decides
        ld = ints([4, 1, edge])
        assert call(n=ints([4, 0, edge]), lda=ld, ldb=ld, ldz=ld, info=None) == -12
    assert call(A=None) == -5
    assert call(A=ptrs(null_at=2)) == -5
    assert call(lda=None) == -6
    assert call(lda=ints([4, 1, NB - 1])) == -6
    assert call(lda=ints([4, 0, NB])) == -6          # lda[b] >= max(1, n[b]) also for an empty problem
    assert call(B=None) == -7
    assert call(B=ptrs(null_at=2)) == -7
    assert call(ldb=None) == -8
    assert call(ldb=ints([4, 1, NB - 1])) == -8
    assert call(w=None) == -9
    assert call(w=ptrs(null_at=2)) == -9
    assert call(Z=None) == -10
    assert call(Z=ptrs(null_at=2)) == -10
    assert call(ldz=None) == -11
    assert call(ldz=ints([4, 1, NB - 1])) == -11
    assert call(info=None) == -12
    # a NULL entry is legal where the problem is empty: the next offender decides
    assert call(A=ptrs(null_at=1), B=ptrs(null_at=1), w=ptrs(null_at=1), Z=ptrs(null_at=1), info=None) == -12
    # the first offending argument decides
    assert call(first=7, jobz=2, batch=-1) == -1
    assert call(jobz=3, n=None) == -2
    assert call(batch=-1, n=None, A=None) == -3
    assert call(n=ints([4, 0, 300]), A=None) == -4
    assert call(A=ptrs(null_at=2), lda=ints([1, 1, 1]), info=None) == -5
    assert call(lda=ints([1, 1, 1]), B=None, info=None) == -6
    assert call(B=None, ldb=None, w=None) == -7
    assert call(w=None, Z=None, info=None) == -9
    # what is not referenced is not looked at -- but the sygv forms always require B
    assert call(jobz=0, Z=None, ldz=None, info=None) == -12
    if sygv:
        for itype in (1, 2, 3):
            assert call(first=itype, B=None, ldb=None, info=None) == -7
            assert call(first=itype, ldb=ints([0, 0, 0]), w=None) == -8
    else:
        assert call(first=0, B=None, ldb=None, info=None) == -12
        assert call(first=0, B=None, ldb=ints([0, 0, 0]), w=None) == -9
    # nothing to do: success without a device and without touching any pointer
    assert call(batch=0, n=None, A=None, lda=None, B=None, ldb=None, w=None, Z=None, ldz=None, info=None) == 0
    assert np.all(info == 777)
    for b in bufs:
        assert np.all(b == 3.5)


@pytest.mark.parametrize("name", EIG + SYGV)
def test_xvbatched_all_orders_zero_needs_no_device(name):
    """Every problem empty: info[b] = 0, success, no pointer looked at (NULL entries everywhere)."""
    fn = getattr(solver.load_library(), name)
    batch = 3
    n = np.zeros(batch, dtype=np.int32)
    ld = np.ones(batch, dtype=np.int32)
    info = np.full(batch, 777, dtype=np.int32)
    null = (ctypes.c_void_p * batch)()
    sec = ctypes.c_double(-1.0)
    rc = fn(1, 1, batch, n.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null, ld.ctypes.data_as(_ip), null, null,
            ld.ctypes.data_as(_ip), info.ctypes.data_as(_ip), ctypes.byref(sec))
    assert rc == 0 and not info.any() and sec.value == 0.0


@pytest.mark.parametrize("name", OLD)
def test_old_variable_entries_keep_their_limit(name):
    """ek_hip_*_vbatched* still answer -4 at order EK_HIP_BATCH_NMAX + 1 (and take EK_HIP_BATCH_NMAX)."""
    fn = getattr(solver.load_library(), name)
    bufs = [np.full(16, 3.5) for _ in range(2)]
    tab = (ctypes.c_void_p * 2)(*[b.ctypes.data for b in bufs])
    info = np.full(2, 777, dtype=np.int32)

    def call(top, info_ptr):
        n = np.array([4, top], dtype=np.int32)
        return fn(1, 1, 2, n.ctypes.data_as(_ip), tab, n.ctypes.data_as(_ip), tab, n.ctypes.data_as(_ip), tab, tab,
                  n.ctypes.data_as(_ip), info_ptr, None)

    assert call(129, info.ctypes.data_as(_ip)) == -4
    assert call(256, info.ctypes.data_as(_ip)) == -4
    assert call(128, None) == -12
    assert np.all(info == 777) and all(np.all(b == 3.5) for b in bufs)


def test_python_mirror_errors_and_empty_batches():
    for fn in (solver.eigenpairs_xvbatched, lambda As, Bs=None, **kw: solver.sygv_xvbatched(As, Bs, **kw)):
        with pytest.raises(ValueError):
            fn([np.zeros((3, 4))], [np.zeros((3, 4))])
        with pytest.raises(ValueError):
            fn([np.zeros((4, 4)), np.zeros((3, 3))], [np.zeros((4, 4))])
        w, Z, info = fn([], [])
        assert w == [] and Z == [] and info.shape == (0,)
        w, Z, info = fn([], [], vectors=False)
        assert w == [] and Z is None and info.shape == (0,)
        # SolverError.info carries the library's code: order 257 is argument 4
        with pytest.raises(solver.SolverError) as ei:
            fn([np.zeros((4, 4)), np.zeros((257, 257))], [np.zeros((4, 4)), np.zeros((257, 257))])
        assert ei.value.info == -4
        # every problem empty: decided on the host
        w, Z, info = fn([np.zeros((0, 0))] * 2, [np.zeros((0, 0))] * 2)
        assert [x.shape for x in w] == [(0,)] * 2 and [x.shape for x in Z] == [(0, 0)] * 2 and not info.any()
    with pytest.raises(ValueError):
        solver.sygv_xvbatched([np.zeros((4, 4))], None)
    with pytest.raises(ValueError):
        solver.sygv_xvbatched([np.zeros((4, 4))], [np.zeros((4, 4))], itype=4)
    with pytest.raises(ValueError):
        solver.sygv_xvbatched([np.zeros((4, 4))], [np.zeros((4, 4))], itype=0)
    # the old wrapper still refuses order 129
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_vbatched([np.zeros((4, 4)), np.zeros((129, 129))])
    assert ei.value.info == -4
