"""Host-side checks of the window entries for orders up to 256 (ek_hip_eigenpairs_window_xbatched*), no GPU needed:
declared in the boundary header, exported and bound with 23 arguments; the chunk hook a debug entry; every argument error
decided before any device work, with NULL, host and garbage pointers (none is dereferenced); n = 129, 200 and 256 legal,
257 is -4, and the old window entries still answer -4 at 129; and the table of tests/window_batched_cases.py pinned
against LAPACK's DSYEVX / DSYGVX at orders 129, 193 and 256 by the logic of tests/test_window_batched_host.py, called as
it stands: half of the eigenvalue bound, a quarter of the residual and orthogonality bounds, every 'V' bound with its gap."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_window_batched_host as base
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_eigenpairs_window_xbatched_device", "ek_hip_eigenpairs_window_xbatched")
OLD = ("ek_hip_eigenpairs_window_batched_device", "ek_hip_eigenpairs_window_batched")
HOOK = "ek_hip_debug_window_xbatched_chunk"
ORDERS = (129, 193, 256)


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_xwindow_entries_declared_exported_and_bound():
    """Fails on a tree without the feature: the symbols are the signal, ek_hip_version stays 3."""
    declared, hooks = _headers()
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in NAMES:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 23
        assert fn.argtypes == getattr(lib, name.replace("xbatched", "batched")).argtypes
    assert callable(solver.eigenpairs_window_xbatched)
    assert solver.XBATCH_NMAX == 256
    assert lib.ek_hip_version() == 3


def test_xwindow_chunk_hook_is_a_debug_entry():
    declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    default = solver.window_xbatched_chunk(7)
    try:
        assert default == 1024
        assert solver.window_xbatched_chunk(3) == 7
        assert solver.window_batched_chunk(0) == 1024      # the other class's hook is another word
    finally:
        assert solver.window_xbatched_chunk(0) == 3
    assert solver.window_xbatched_chunk(0) == 1024


@pytest.mark.parametrize("pointers", ["host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_xwindow_argument_errors_without_gpu(name, pointers):
    """-k for argument k of the prototype, before any device work: a pointer is compared with NULL and never followed
    (host addresses to the device form, and an address that belongs to nobody)."""
    fn = getattr(solver.load_library(), name)
    n, batch = 200, 3
    buf = np.zeros(8)
    info = np.zeros(batch, dtype=np.int32)
    mm = np.zeros(batch, dtype=np.int32)
    addr = buf.ctypes.data if pointers == "host" else 0x10
    if name.endswith("_device"):
        p = ctypes.c_void_p(addr)
    else:
        p = ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_double))
    if pointers == "host":
        ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        mp = mm.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    else:
        ip = mp = ctypes.cast(ctypes.c_void_p(0x10), ctypes.POINTER(ctypes.c_int))
    nan, inf = float("nan"), float("inf")

    def call(problem=1, jobz=1, rng=0, n=n, batch=batch, vl=0.0, vu=1.0, il=1, iu=2, A=p, lda=None, sA=None, B=p,
             ldb=None, sB=None, m=mp, w=p, Z=p, ldz=None, zcap=None, sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        zcap = ld if zcap is None else zcap
        sA, sB = (ld * ld if x is None else x for x in (sA, sB))
        sZ = ld * max(zcap, 1) if sZ is None else sZ
        return fn(problem, jobz, rng, n, batch, vl, vu, il, iu, A, lda, sA, B, ldb, sB, m, w, Z, ldz, zcap, sZ, info, None)

    assert call(problem=2) == -1 and call(problem=-1) == -1
    assert call(jobz=2) == -2
    assert call(rng=2) == -3 and call(rng=-1) == -3
    assert call(n=-1) == -4 and call(n=257) == -4 and call(n=1 << 20) == -4
    for legal in (129, 200, 256):                   # the order is accepted: the next argument decides
        assert call(n=legal, batch=-1) == -5
        assert call(n=legal, A=None) == -10
    assert call(batch=-1) == -5
    assert call(rng=1, vl=nan) == -6
    assert call(rng=1, vu=nan) == -7
    assert call(rng=1, vl=1.0, vu=1.0) == -7 and call(rng=1, vl=2.0, vu=1.0) == -7
    assert call(rng=1, vl=-inf, vu=inf, il=0, iu=999, A=None) == -10
    assert call(rng=1, vl=inf, vu=inf) == -7
    assert call(il=0) == -8 and call(il=n + 1, iu=n + 1) == -8
    assert call(il=3, iu=2) == -9 and call(iu=n + 1) == -9
    assert call(vl=nan, vu=nan, A=None) == -10
    assert call(A=None) == -10
    assert call(lda=n - 1) == -11
    assert call(sA=n * n - 1) == -12 and call(sA=0) == -12
    assert call(lda=n + 2, sA=n * n) == -12
    assert call(B=None) == -13
    assert call(ldb=n - 1) == -14
    assert call(sB=n * n - 1) == -15 and call(sB=0) == -15
    assert call(m=None) == -16
    assert call(w=None) == -17
    assert call(Z=None) == -18
    assert call(ldz=n - 1) == -19
    assert call(zcap=-1) == -20
    assert call(il=1, iu=3, zcap=2) == -20
    assert call(rng=1, zcap=0, info=None) == -22
    assert call(zcap=3, sZ=3 * n - 1) == -21
    assert call(rng=1, zcap=0, sZ=n - 1) == -21
    assert call(info=None) == -22
    # the first offending argument decides
    assert call(problem=2, jobz=2, rng=5) == -1
    assert call(rng=5, n=-1) == -3
    assert call(n=257, batch=-1) == -4
    assert call(rng=1, vl=nan, vu=nan) == -6
    assert call(il=0, iu=0, A=None) == -8
    assert call(m=None, w=None) == -16
    # nothing to do: success without a device and without touching any pointer or the window
    assert call(batch=0) == 0 and call(n=0, il=0, iu=0) == 0
    assert call(batch=0, il=0, iu=0, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    assert call(n=0, rng=1, vl=nan, vu=nan, A=None, B=None, m=None, w=None, Z=None, info=None) == 0
    # what is not referenced is not checked
    assert call(problem=0, B=None, ldb=0, sB=0, m=None) == -16
    assert call(jobz=0, Z=None, ldz=0, sZ=0, info=None) == -22
    assert call(jobz=0, Z=None, ldz=0, zcap=-1, sZ=0) == -20
    assert call(jobz=0, il=1, iu=3, zcap=2) == -20
    assert not info.any() and not buf.any() and not mm.any()


@pytest.mark.parametrize("name", OLD)
def test_the_old_window_entries_still_stop_at_128(name):
    fn = getattr(solver.load_library(), name)
    none = [None] * 2
    assert fn(0, 0, 0, 129, 1, 0.0, 0.0, 1, 1, None, 129, 129 * 129, None, 129, 129 * 129, *none, None, 129, 1, 129,
              None, None) == -4
    assert fn(0, 0, 0, 128, 1, 0.0, 0.0, 1, 1, None, 128, 128 * 128, None, 128, 128 * 128, *none, None, 128, 1, 128,
              None, None) == -10


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xbatched(np.zeros((3, 200)))
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xbatched(np.zeros((2, 200, 200)), np.zeros((2, 199, 199)))
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xbatched(np.zeros((2, 200, 200)), il=1, vu=0.0)
    w, Z, m, info = solver.eigenpairs_window_xbatched(np.zeros((0, 200, 200)), il=2, iu=4)
    assert w.shape == (0, 200) and Z.shape == (0, 200, 3) and m.shape == (0,) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_xbatched(np.zeros((1, 257, 257)))
    assert ei.value.info == -4
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_xbatched(np.zeros((1, 200, 200)), il=5, iu=4)
    assert ei.value.info == -9
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_batched(np.zeros((1, 129, 129)))
    assert ei.value.info == -4


@pytest.mark.parametrize("n", ORDERS)
def test_lapack_windowed_drivers_stay_inside_part_of_the_bounds_at_the_new_orders(n):
    """tests/test_window_batched_host.py's check as it stands (every unscaled case but hilbert_b, every window and the
    cluster cuts; half / a quarter / a quarter of the bounds), and every clustered class has a cluster cut here too."""
    base.test_lapack_windowed_drivers_stay_inside_part_of_the_bounds(n)
    for name in base.wc.CLUSTERED:
        w_ref = base.sl.eigh(base.bc.make(name, n).A, lower=True)[0]
        assert base.wc.cluster_cut(w_ref) is not None, (name, n)


@pytest.mark.parametrize("n", ORDERS)
def test_value_bounds_keep_the_gap_at_the_new_orders(n):
    base.test_value_bounds_keep_the_gap(n)
