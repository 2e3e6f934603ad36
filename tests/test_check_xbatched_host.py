"""Host-side checks of the batched acceptance checks for orders up to 256 (ek_hip_check_xbatched*): declared in the boundary
header, exported, bound by the Python mirror with the right argument types, the chunk hook a debug entry, and every
argument error decided before any device work and without dereferencing a data pointer (no GPU needed: the device forms
get host addresses or garbage, and there may be no GPU at all)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_check_xbatched_device", "ek_hip_check_xbatched")
OLD = ("ek_hip_check_batched_device", "ek_hip_check_batched")
HOOK = "ek_hip_debug_check_xbatched_chunk"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return hdr, dbg, set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_check_xbatched_entries_declared_exported_and_bound():
    hdr, _, declared, hooks = _headers()
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
    m = re.search(r"#define\s+EK_HIP_XBATCH_NMAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 256 == solver.XBATCH_NMAX
    assert "the batched checks" not in hdr.split("#define EK_HIP_XBATCH_NMAX")[0][-400:]
    assert callable(solver.check_xbatched) and callable(solver.check_xbatched_chunk)
    assert lib.ek_hip_version() == 3


def test_chunk_hook_is_a_debug_entry():
    _, _, declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    fn = getattr(solver.load_library(), HOOK)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_int]
    # host state only: the previous value comes back, 0 restores the default; the solver's hook is another word
    solver_chunk = solver.xbatched_chunk(0)
    default = solver.check_xbatched_chunk(7)
    try:
        assert default == 1024
        assert solver.check_xbatched_chunk(3) == 7
        assert solver.xbatched_chunk(0) == solver_chunk
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

    def call(problem=1, n=n, batch=batch, A=p, lda=None, sA=None, B=p, ldb=None, sB=None, w=p, Z=p, ldz=None, sZ=None,
             info=ip, out=op, ipr=qp):
        lda, ldb, ldz = (n if x is None else x for x in (lda, ldb, ldz))
        sA, sB, sZ = (n * n if x is None else x for x in (sA, sB, sZ))
        return fn(problem, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, out, ipr, None)

    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(n=-1) == -2
    assert call(n=257) == -2
    assert call(batch=-1) == -3
    assert call(A=None) == -4
    assert call(lda=n - 1) == -5
    assert call(sA=n * n - 1) == -6
    assert call(sA=0) == -6                         # a stride of 0 is an argument error, not a broadcast
    assert call(lda=n + 2, sA=n * n) == -6
    assert call(B=None) == -7
    assert call(ldb=n - 1) == -8
    assert call(sB=0) == -9
    assert call(w=None) == -10
    assert call(Z=None) == -11
    assert call(ldz=n - 1) == -12
    assert call(sZ=n * n - 1) == -13
    assert call(out=None) == -15
    # orders 129 .. 256 are legal: the next offender decides, and no device is touched
    for big in (129, 200, 256):
        assert call(n=big, A=None) == -4
        assert call(n=big, lda=big - 1) == -5
        assert call(n=big, sA=big * big - 1) == -6
        assert call(n=big, B=None) == -7
        assert call(n=big, ldb=big - 1) == -8
        assert call(n=big, sB=big * big - 1) == -9
        assert call(n=big, w=None) == -10
        assert call(n=big, Z=None) == -11
        assert call(n=big, ldz=big - 1) == -12
        assert call(n=big, sZ=big * big - 1) == -13
        assert call(n=big, out=None) == -15
        assert call(n=big, info=None, ipr=None, out=None) == -15
        assert call(n=big, problem=0, B=None, ldb=0, sB=0, out=None) == -15
        assert call(n=big, batch=0, A=None, B=None, w=None, Z=None, info=None, out=None, ipr=None) == 0
    # the first offending argument decides
    assert call(problem=3, n=-1, batch=-1) == -1
    assert call(n=257, batch=-1, A=None) == -2
    assert call(n=200, batch=-1, A=None) == -3
    assert call(batch=-1, A=None, lda=0) == -3
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
    # B, ldb and strideB are not looked at for problem 0; info = NULL and ipr = NULL are legal: the next offender decides
    assert call(problem=0, B=None, ldb=0, sB=0, out=None) == -15
    assert call(problem=0, B=None, ldb=-5, sB=-5, w=None) == -10
    assert call(info=None, ipr=None, out=None) == -15
    assert call(info=None, ipr=None, Z=None) == -11
    # nothing to do: success with every pointer NULL, nothing written
    for kw in (dict(batch=0), dict(n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0), dict(n=200, batch=0)):
        sec = ctypes.c_double(-1.0)
        args = dict(problem=1, n=n, batch=batch, lda=n, sA=n * n, ldb=n, sB=n * n, ldz=n, sZ=n * n)
        args.update(kw)
        rc = fn(args["problem"], args["n"], args["batch"], None, args["lda"], args["sA"], None, args["ldb"], args["sB"],
                None, None, args["ldz"], args["sZ"], None, None, None, ctypes.byref(sec))
        assert rc == 0 and sec.value == 0.0
    assert np.all(buf == 3.5) and np.all(out == 777.0) and np.all(ipr == 777.0) and not info.any()


def test_the_old_entries_still_stop_at_128():
    lib = solver.load_library()
    out = np.full(4, 777.0)
    op = out.ctypes.data_as(_dp)
    k = 129
    for name in OLD:
        assert getattr(lib, name)(0, k, 1, None, k, k * k, None, k, k * k, None, None, k, k * k, None, op, None, None) == -2
    for name in ("ek_hip_check_sygv_batched_device", "ek_hip_check_sygv_batched"):
        assert getattr(lib, name)(2, k, 1, None, k, k * k, None, k, k * k, None, None, k, k * k, None, op, None, None) == -2
    n = np.array([k], dtype=np.int32)
    ptr = (ctypes.c_void_p * 1)(None)
    for name in ("ek_hip_check_vbatched_device", "ek_hip_check_vbatched"):
        assert getattr(lib, name)(0, 1, n.ctypes.data_as(_ip), ptr, n.ctypes.data_as(_ip), ptr, n.ctypes.data_as(_ip), ptr,
                                  ptr, n.ctypes.data_as(_ip), None, op, None, None) == -3
    for name in ("ek_hip_check_sygv_vbatched_device", "ek_hip_check_sygv_vbatched"):
        assert getattr(lib, name)(2, 1, n.ctypes.data_as(_ip), ptr, n.ctypes.data_as(_ip), ptr, n.ctypes.data_as(_ip), ptr,
                                  ptr, n.ctypes.data_as(_ip), None, op, None, None) == -3
    assert np.all(out == 777.0)


def test_python_mirror_rejects_bad_shapes_before_the_library():
    z3, z4 = np.zeros((2, 3, 3)), np.zeros((2, 4, 4))
    for bad in (dict(A=np.zeros((2, 3, 4))), dict(A=np.zeros((3, 3))), dict(B=z4), dict(Z=z4), dict(w=np.zeros((2, 4))),
                dict(w=np.zeros(6)), dict(info=np.zeros(3, dtype=np.int32)), dict(info=np.zeros((2, 1), dtype=np.int32))):
        kw = dict(A=z3, B=z3, w=np.zeros((2, 3)), Z=z3, info=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            solver.check_xbatched(kw["A"], kw["B"], kw["w"], kw["Z"], info=kw["info"])
    # decided without a device: nothing to check, an order of 0, an order beyond the last
    out, q = solver.check_xbatched(np.zeros((0, 200, 200)), None, np.zeros((0, 200)), np.zeros((0, 200, 200)))
    assert out.shape == (0, 4) and q.shape == (0, 200)
    out, q = solver.check_xbatched(np.zeros((2, 0, 0)), None, np.zeros((2, 0)), np.zeros((2, 0, 0)), info=[0, 1])
    assert out[0, 0] == 0.0 and np.all(np.isnan(out[0, 1:])) and np.all(np.isnan(out[1])) and q.shape == (2, 0)
    with pytest.raises(solver.SolverError) as ei:
        solver.check_xbatched(np.zeros((1, 257, 257)), None, np.zeros((1, 257)), np.zeros((1, 257, 257)))
    assert ei.value.info == -2
