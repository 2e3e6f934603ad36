"""Host-side checks of the batched acceptance checks of DSYGV's three types for orders up to 256
(ek_hip_check_sygv_xbatched*): declared in the boundary header, exported, bound by the Python mirror with the right argument
types, and every argument error decided before any device work and without dereferencing a data pointer (no GPU needed:
the device forms get host addresses or garbage, and there may be no GPU at all)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_check_sygv_xbatched_device", "ek_hip_check_sygv_xbatched")
HOOK = "ek_hip_debug_check_xbatched_chunk"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced


def test_entries_declared_exported_and_bound():
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
        at = fn.argtypes
        assert fn.restype is ctypes.c_int and len(at) == 17
        assert at[5] is ctypes.c_longlong and at[8] is ctypes.c_longlong and at[12] is ctypes.c_longlong
        assert at[13] is _ip and at[14] is _dp and at[15] is _dp and at[16] is _dp      # info, out, ipr: host arrays
        old = getattr(lib, name.replace("xbatched", "batched"))
        assert list(at) == list(old.argtypes)                                            # argument for argument
    assert callable(solver.check_sygv_xbatched)
    assert lib.ek_hip_version() == 3
    # the header no longer says that these checks are missing
    assert "the checks of types 2 and 3. */" not in hdr
    assert "at a time is checked by ek_hip_check_sygvx*" not in hdr


def test_the_chunk_hook_keeps_its_behaviour():
    default = solver.check_xbatched_chunk(7)
    try:
        assert default == 1024
        assert solver.check_xbatched_chunk(3) == 7
    finally:
        assert solver.check_xbatched_chunk(0) == 3
    assert solver.check_xbatched_chunk(-5) == 1024
    assert solver.check_xbatched_chunk(0) == 1024


@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_without_gpu(name, data):
    """-k for argument k of the prototype, the first offender deciding; no data pointer is dereferenced."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    n, batch = 4, 3
    buf = np.full(batch * n * n, 3.5)
    out = np.full(batch * 4, 777.0)
    ipr = np.full(batch * n, 777.0)
    info = np.zeros(batch, dtype=np.int32)
    if data == "garbage":
        p = ctypes.c_void_p(GARBAGE) if name.endswith("_device") else ctypes.cast(GARBAGE, _dp)
    else:
        p = ctypes.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(_dp)
    ip, op, qp = info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), ipr.ctypes.data_as(_dp)

    def call(itype=2, n=n, batch=batch, A=p, lda=None, sA=None, B=p, ldb=None, sB=None, w=p, Z=p, ldz=None, sZ=None,
             info=ip, out=op, ipr=qp, seconds=None):
        lda, ldb, ldz = (n if x is None else x for x in (lda, ldb, ldz))
        sA, sB, sZ = (n * n if x is None else x for x in (sA, sB, sZ))
        return fn(itype, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, out, ipr, seconds)

    assert call(itype=0) == -1
    assert call(itype=4) == -1
    for itype in (1, 2, 3):
        assert call(itype=itype, n=-1) == -2
        assert call(itype=itype, n=257) == -2
        assert call(itype=itype, batch=-1) == -3
        assert call(itype=itype, A=None) == -4
        assert call(itype=itype, lda=n - 1) == -5
        assert call(itype=itype, sA=n * n - 1) == -6
        assert call(itype=itype, sA=0) == -6
        assert call(itype=itype, B=None) == -7      # B is always required
        assert call(itype=itype, ldb=n - 1) == -8
        assert call(itype=itype, sB=n * n - 1) == -9
        assert call(itype=itype, sB=0) == -9
        assert call(itype=itype, w=None) == -10
        assert call(itype=itype, Z=None) == -11
        assert call(itype=itype, ldz=n - 1) == -12
        assert call(itype=itype, sZ=n * n - 1) == -13
        assert call(itype=itype, out=None) == -15
        assert call(itype=itype, info=None, ipr=None, out=None) == -15      # info = NULL and ipr = NULL are legal
        assert call(itype=itype, info=None, ipr=None, Z=None) == -11
        # orders 129 .. 256 are legal: the next offender decides, and no device is touched
        for big in (129, 200, 256):
            assert call(itype=itype, n=big, A=None) == -4
            assert call(itype=itype, n=big, lda=big - 1) == -5
            assert call(itype=itype, n=big, sA=big * big - 1) == -6
            assert call(itype=itype, n=big, B=None) == -7
            assert call(itype=itype, n=big, ldb=big - 1) == -8
            assert call(itype=itype, n=big, sB=big * big - 1) == -9
            assert call(itype=itype, n=big, w=None) == -10
            assert call(itype=itype, n=big, Z=None) == -11
            assert call(itype=itype, n=big, ldz=big - 1) == -12
            assert call(itype=itype, n=big, sZ=big * big - 1) == -13
            assert call(itype=itype, n=big, out=None) == -15
            assert call(itype=itype, n=big, info=None, ipr=None, out=None) == -15
            sec = ctypes.c_double(-1.0)
            assert call(itype=itype, n=big, batch=0, seconds=ctypes.byref(sec)) == 0 and sec.value == 0.0
            assert call(itype=itype, n=big, batch=0, A=None, B=None, w=None, Z=None, info=None, out=None, ipr=None) == 0
        assert call(itype=itype, n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0, A=None, B=None, w=None, Z=None, info=None,
                    out=None, ipr=None) == 0
    # the first offending argument decides
    assert call(itype=0, n=-1, batch=-1) == -1
    assert call(itype=4, n=257, A=None) == -1
    assert call(n=257, batch=-1, A=None) == -2
    assert call(n=200, batch=-1, A=None) == -3
    assert call(A=None, lda=0, sA=0) == -4
    assert call(lda=0, sA=0, B=None) == -5
    assert call(sA=0, B=None, w=None) == -6
    assert call(B=None, ldb=0, sB=0, out=None) == -7
    assert call(ldb=0, sB=0, w=None) == -8
    assert call(sB=0, w=None, Z=None) == -9
    assert call(w=None, Z=None, out=None) == -10
    assert call(Z=None, ldz=0, out=None) == -11
    assert call(ldz=0, sZ=0, out=None) == -12
    assert call(sZ=0, out=None) == -13
    assert call(n=200, sZ=0, out=None) == -13
    assert np.all(buf == 3.5) and np.all(out == 777.0) and np.all(ipr == 777.0) and not info.any()


def test_the_old_entries_still_stop_at_128():
    lib = solver.load_library()
    out = np.full(4, 777.0)
    op = out.ctypes.data_as(_dp)
    k = 129
    for name in ("ek_hip_check_batched_device", "ek_hip_check_batched"):
        assert getattr(lib, name)(0, k, 1, None, k, k * k, None, k, k * k, None, None, k, k * k, None, op, None, None) == -2
    for name in ("ek_hip_check_sygv_batched_device", "ek_hip_check_sygv_batched"):
        for itype in (1, 2, 3):
            assert getattr(lib, name)(itype, k, 1, None, k, k * k, None, k, k * k, None, None, k, k * k, None, op, None,
                                      None) == -2
    assert np.all(out == 777.0)


def test_python_mirror_rejects_bad_arguments_before_the_library():
    z3, z4 = np.zeros((2, 3, 3)), np.zeros((2, 4, 4))
    w3 = np.zeros((2, 3))
    for itype in (0, 4):
        with pytest.raises(ValueError):
            solver.check_sygv_xbatched(z3, z3, w3, z3, itype=itype)
    with pytest.raises(ValueError):
        solver.check_sygv_xbatched(z3, None, w3, z3, itype=2)
    for bad in (dict(A=np.zeros((2, 3, 4))), dict(B=z4), dict(Z=z4), dict(w=np.zeros((2, 4))),
                dict(info=np.zeros(3, dtype=np.int32))):
        kw = dict(A=z3, B=z3, w=w3, Z=z3, info=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            solver.check_sygv_xbatched(kw["A"], kw["B"], kw["w"], kw["Z"], itype=3, info=kw["info"])
    # decided without a device: nothing to check, an order beyond the last
    z = np.zeros((0, 200, 200))
    out, q = solver.check_sygv_xbatched(z, z, np.zeros((0, 200)), z, itype=3)
    assert out.shape == (0, 4) and q.shape == (0, 200)
    big = np.zeros((1, 257, 257))
    with pytest.raises(solver.SolverError) as ei:
        solver.check_sygv_xbatched(big, big, np.zeros((1, 257)), big, itype=2)
    assert ei.value.info == -2
