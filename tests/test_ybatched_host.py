"""Host-side checks of the entries for orders up to 512 (ek_hip_eigenpairs_ybatched*, ek_hip_sygv_ybatched*): declared in
the boundary header, exported, bound by the Python mirror, and every argument error decided before any device work (no GPU
needed).  Modelled on tests/test_xbatched_host.py and tests/test_sygv_xbatched_host.py.

The last two tests hold LAPACK alone, on this machine's CPU, to HALF of every bound the GPU suites of these entries use
(tests/test_gpu_ybatched.py, tests/test_gpu_sygv_ybatched.py) at the new orders: if a second LAPACK driver needed more than
half of a bound against SciPy's default one, the bound would say little about the kernel.  Measured: see each test."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import test_gpu_batched_hard as hard
from eigenkernel_amd import solver
from test_gpu_batched import EPS, _check_problem, _pairs
from test_gpu_sygv_batched import _quantities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG = ("ek_hip_eigenpairs_ybatched_device", "ek_hip_eigenpairs_ybatched")
SYGV = ("ek_hip_sygv_ybatched_device", "ek_hip_sygv_ybatched")
HOOK = "ek_hip_debug_ybatched_chunk"
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return hdr, dbg, set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def _prototype(hdr, name):
    """the argument types of a prototype of the header, in order, without the names"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_ybatched_entries_declared_exported_and_bound():
    hdr, _, declared, hooks = _headers()
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in EIG + SYGV:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
        # argument for argument the xbatched entry: in the header and in the binding
        twin = name.replace("ybatched", "xbatched")
        assert _prototype(hdr, name) == _prototype(hdr, twin), name
        assert list(fn.argtypes) == list(getattr(lib, twin).argtypes), name
        assert fn.argtypes[6] is ctypes.c_longlong and fn.argtypes[9] is ctypes.c_longlong
        assert fn.argtypes[13] is ctypes.c_longlong
    m = re.search(r"#define\s+EK_HIP_YBATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 512 == solver.YBATCH_NMAX
    m = re.search(r"#define\s+EK_HIP_XBATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 256 == solver.XBATCH_NMAX
    assert callable(solver.eigenpairs_ybatched) and callable(solver.sygv_ybatched) and callable(solver.ybatched_chunk)
    assert lib.ek_hip_version() == 3              # the symbols are the signal


def test_ybatched_chunk_hook_is_a_debug_entry():
    _, _, declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    fn = getattr(solver.load_library(), HOOK)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_int]
    # host state only: the previous value comes back, 0 restores the default; the x class's hook is another variable
    default = solver.ybatched_chunk(7)
    try:
        assert default == 256
        assert solver.ybatched_chunk(3) == 7
        assert solver.xbatched_chunk(0) == 1024
    finally:
        assert solver.ybatched_chunk(0) == 3
    assert solver.ybatched_chunk(0) == 256


def _pointers(name, kind, buf):
    """the data pointer of a call: `host` a real host array (the device form gets a host address too), `garbage` an
    address that must never be dereferenced"""
    address = buf.ctypes.data if kind == "host" else 0x10
    if name.endswith("_device"):
        return ctypes.c_void_p(address)
    return ctypes.cast(ctypes.c_void_p(address), _dp)


@pytest.mark.parametrize("kind", ["host", "garbage"])
@pytest.mark.parametrize("name", EIG + SYGV)
def test_ybatched_argument_errors_without_gpu(name, kind):
    """-k for argument k in prototype order, before any device work: a data pointer is never dereferenced here (host
    addresses in the device form, garbage addresses in both, and there may be no GPU at all).  Every call below is
    refused -- or has nothing to do -- so none reaches the device."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    sygv = name in SYGV
    n, batch = 4, 3
    buf = np.zeros(batch * n * n)
    info = np.zeros(batch, dtype=np.int32)
    p = _pointers(name, kind, buf)
    ip = info.ctypes.data_as(_ip) if kind == "host" else ctypes.cast(ctypes.c_void_p(0x10), _ip)

    def call(first=(2 if sygv else 1), jobz=1, n=n, batch=batch, A=p, lda=None, sA=None, B=p, ldb=None, sB=None, w=p, Z=p,
             ldz=None, sZ=None, info=ip):
        ld = max(n, 1)
        lda, ldb, ldz = (ld if x is None else x for x in (lda, ldb, ldz))
        sA, sB, sZ = (ld * ld if x is None else x for x in (sA, sB, sZ))
        return fn(first, jobz, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, None)

    firsts = (1, 2, 3) if sygv else (0, 1)
    if sygv:                                       # itype 0 and 4 before everything
        for bad in (0, 4, -1):
            assert call(first=bad) == -1
            assert call(first=bad, jobz=2, n=-1, batch=-1, A=None, info=None) == -1
            assert call(first=bad, n=513) == -1
            assert call(first=bad, n=400) == -1
    else:
        assert call(first=2) == -1
        assert call(first=-1) == -1
        assert call(first=2, jobz=2, n=-1) == -1
    for first in firsts:
        needs_b = sygv or first == 1
        assert call(first=first, jobz=2) == -2
        assert call(first=first, jobz=-1) == -2
        assert call(first=first, n=-1) == -3
        assert call(first=first, n=513) == -3
        assert call(first=first, n=1024) == -3
        assert call(first=first, batch=-1) == -4
        assert call(first=first, A=None) == -5
        assert call(first=first, lda=n - 1) == -6
        assert call(first=first, sA=n * n - 1) == -7
        assert call(first=first, sA=0) == -7                       # no broadcast
        assert call(first=first, lda=n + 2, sA=n * n) == -7        # the stride follows the leading dimension
        if needs_b:                                # B is always required in the sygv form, for itype 1 too
            assert call(first=first, B=None) == -8
            assert call(first=first, ldb=n - 1) == -9
            assert call(first=first, sB=n * n - 1) == -10
            assert call(first=first, sB=0) == -10
            assert call(first=first, ldb=n + 2, sB=n * n) == -10
        else:                                      # what is not referenced is not checked
            assert call(first=first, B=None, ldb=0, sB=0, w=None) == -11
        assert call(first=first, w=None) == -11
        assert call(first=first, Z=None) == -12
        assert call(first=first, ldz=n - 1) == -13
        assert call(first=first, sZ=n * n - 1) == -14
        assert call(first=first, jobz=0, Z=None, ldz=0, sZ=0, info=None) == -15
        assert call(first=first, info=None) == -15
        # 257, 400 and 512 are legal: the next argument decides, and no device is touched
        for big in (257, 400, 512):
            assert call(first=first, n=big, batch=-1) == -4
            assert call(first=first, n=big, A=None) == -5
            assert call(first=first, n=big, lda=big - 1) == -6
            assert call(first=first, n=big, sA=big * big - 1) == -7
            if needs_b:
                assert call(first=first, n=big, B=None) == -8
                assert call(first=first, n=big, ldb=big - 1) == -9
                assert call(first=first, n=big, sB=big * big - 1) == -10
            assert call(first=first, n=big, w=None) == -11
            assert call(first=first, n=big, Z=None) == -12
            assert call(first=first, n=big, ldz=big - 1) == -13
            assert call(first=first, n=big, sZ=big * big - 1) == -14
            assert call(first=first, n=big, info=None) == -15
            assert call(first=first, n=big, jobz=0, Z=None, ldz=0, sZ=0, info=None) == -15
            assert call(first=first, n=big, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
        # nothing to do: success without a device and without touching any pointer
        assert call(first=first, batch=0, A=None, B=None, w=None, Z=None, info=None) == 0
        assert call(first=first, n=0, A=None, B=None, w=None, Z=None, info=None) == 0
        assert call(first=first, n=0) == 0 and call(first=first, batch=0) == 0
        # the first offending argument decides
        assert call(first=first, jobz=3, n=513) == -2
        assert call(first=first, n=513, batch=-1) == -3
        assert call(first=first, n=512, batch=-1, A=None) == -4
        assert call(first=first, A=None, B=None, w=None) == -5
        assert call(first=first, lda=0, sA=0, info=None) == -6
    assert not info.any() and not buf.any()


def test_the_old_entries_still_stop_where_they_did():
    lib = solver.load_library()
    info = np.zeros(1, dtype=np.int32)
    ip = info.ctypes.data_as(_ip)

    def refuses(fn, first, n):
        return fn(first, 0, n, 1, None, n, n * n, None, n, n * n, None, None, n, n * n, ip, None) == -3

    for first in (0, 1):
        for form in ("", "_device"):
            assert refuses(getattr(lib, "ek_hip_eigenpairs_xbatched" + form), first, 257)
            assert refuses(getattr(lib, "ek_hip_eigenpairs_batched" + form), first, 129)
            assert refuses(getattr(lib, "ek_hip_eigenpairs_batched" + form), first, 257)
    for itype in (1, 2, 3):
        for form in ("", "_device"):
            assert refuses(getattr(lib, "ek_hip_sygv_xbatched" + form), itype, 257)
            assert refuses(getattr(lib, "ek_hip_sygv_batched" + form), itype, 129)
            assert refuses(getattr(lib, "ek_hip_sygv_batched" + form), itype, 257)
    assert not info.any()


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_ybatched(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        solver.eigenpairs_ybatched(np.zeros((2, 4, 4)), np.zeros((2, 3, 3)))
    A = np.zeros((2, 300, 300))
    for itype in (0, 4):
        with pytest.raises(ValueError):
            solver.sygv_ybatched(A, A, itype=itype)
    with pytest.raises(ValueError):
        solver.sygv_ybatched(A, None, itype=2)
    w, Z, info = solver.eigenpairs_ybatched(np.zeros((0, 400, 400)))
    assert w.shape == (0, 400) and Z.shape == (0, 400, 400) and info.shape == (0,)
    w, Z, info = solver.sygv_ybatched(np.zeros((0, 400, 400)), np.zeros((0, 400, 400)), itype=3)
    assert w.shape == (0, 400) and Z.shape == (0, 400, 400) and info.shape == (0,)
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_ybatched(np.zeros((1, 513, 513)))
    assert ei.value.info == -3
    with pytest.raises(solver.SolverError) as ei:
        solver.sygv_ybatched(np.zeros((1, 513, 513)), np.zeros((1, 513, 513)), itype=2)
    assert ei.value.info == -3


# ------------------------------------------------------------------------------------------------- LAPACK inside the bounds
@pytest.mark.parametrize("kind,n", [("standard", 257), ("type1", 384), ("type2", 263), ("type3", 512)])
def test_lapack_alone_uses_under_half_of_the_bounds(kind, n):
    """A second LAPACK route against SciPy's default driver on _pairs(1000 + n, ...), the GPU suites' inputs: the QR
    drivers ev / gv for the standard problem and type 1, and for types 2 and 3 DSYEV on an explicit C = L^T A L with
    x = L^-T y / x = L y.  Each uses at most half of 4 max(n, 8) eps max|lambda| and of 64 / 256 n eps (measured on one
    x86 host at the four (kind, order) pairs below: 0.034 / 0.002 / 0.002 at most)."""
    A, B = _pairs(1000 + n, 1, n)
    A, B = A[0], B[0]
    if kind == "standard":
        w_ref = sl.eigh(A, lower=True, eigvals_only=True)
        w, Z = sl.eigh(A, lower=True, driver="ev")
        shares = _check_problem(A, None, w, Z, w_ref, (kind, n))
    elif kind == "type1":
        w_ref = sl.eigh(A, B, lower=True, eigvals_only=True)
        w, Z = sl.eigh(A, B, lower=True, driver="gv")
        shares = _check_problem(A, B, w, Z, w_ref, (kind, n))
    else:
        itype = 2 if kind == "type2" else 3
        w_ref = sl.eigh(A, B, type=itype, lower=True, eigvals_only=True)
        L = np.linalg.cholesky(B)
        C = L.T @ A @ L
        w, Y = sl.eigh((C + C.T) / 2, lower=True, driver="ev")
        Z = sl.solve_triangular(L, Y, lower=True, trans="T") if itype == 2 else L @ Y
        res, orth = _quantities(itype, A, B, w, Z)
        shares = (np.abs(w - w_ref).max() / (4 * max(n, 8) * EPS * np.abs(w_ref).max()), res / (256 * n * EPS),
                  orth / (256 * n * EPS))
    print("%s n=%d: LAPACK's share of the bounds: eigenvalues %.3f residual %.3f orthogonality %.3f" % ((kind, n) + shares))
    assert max(shares) <= 0.5, shares


def test_lapack_alone_passes_the_hard_table_at_257_with_half_of_the_bounds():
    """A seeded subset of the hard table at order 257 (12 standard cases, 8 pencils, the scaled ones among them) solved by
    the QR drivers ev / gv and judged by test_gpu_batched_hard._judge as the GPU suite's results are: no failure, and no
    share above one half (measured on the whole table at 257 and 512: 0.024 / 0.006 / 0.004 on standard cases,
    0.014 / 0.278 / 0.334 on pencils).  A B that is not numerically SPD, and A 2^600 with B 2^-600 (eigenvalues beyond
    the range of a double), have no LAPACK result and are left to the GPU suite."""
    n = 257
    rng = np.random.default_rng(257257)
    std = bc.standard_batch(n)
    pen = [cb for cb in bc.pencil_batch(n) if cb[0].spd and not (cb[0].ka == 600 and cb[0].kb == -600)]
    picked = [std[i] for i in sorted(rng.choice(len(std), 12, replace=False))]
    picked += [pen[i] for i in sorted(rng.choice(len(pen), 8, replace=False))]
    worst, fails = np.zeros(3), []
    for c, base in picked:
        with np.errstate(all="ignore"):
            if c.B is None:
                w, Z = sl.eigh(c.A, lower=True, driver="ev")
            else:
                w, Z = sl.eigh(c.A, c.B, lower=True, driver="gv")
        shares, f = hard._judge(None, c, base, 0, w, Z, "n=%d %s" % (n, c.name))
        fails += f
        if shares is not None:
            worst = np.maximum(worst, [s or 0.0 for s in shares])
    print("hard table, %d cases at n=%d: LAPACK's share of the bounds: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((len(picked), n) + tuple(worst)))
    assert not fails, "\n".join(fails)
    assert worst.max() <= 0.5, worst
