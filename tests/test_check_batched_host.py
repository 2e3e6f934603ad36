"""Host-side checks of the batched acceptance checks (ek_hip_check_batched*, ek_hip_check_vbatched*): declared in the
boundary header, exported, bound by the Python mirror with the right argument types, and every argument error decided
before any device work and without dereferencing a data pointer (no GPU needed: the device forms get host addresses
or garbage, and there may be no GPU at all)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIFORM = ("ek_hip_check_batched_device", "ek_hip_check_batched")
VARIABLE = ("ek_hip_check_vbatched_device", "ek_hip_check_vbatched")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced


def test_check_entries_declared_exported_and_bound():
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
        assert getattr(lib, name).restype is ctypes.c_int
    for name in UNIFORM:
        at = getattr(lib, name).argtypes
        assert len(at) == 17
        assert at[5] is ctypes.c_longlong and at[8] is ctypes.c_longlong and at[12] is ctypes.c_longlong
        assert at[13] is _ip and at[14] is _dp and at[15] is _dp and at[16] is _dp      # info, out, ipr: host arrays
    for name in VARIABLE:
        at = getattr(lib, name).argtypes
        assert len(at) == 14
        assert at[2] is _ip and at[10] is _ip and at[11] is _dp and at[13] is _dp
    m = re.search(r"#define\s+EK_HIP_CHECK_NOUT\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 4 == solver.CHECK_NOUT
    assert callable(solver.check_batched) and callable(solver.check_vbatched)
    assert lib.ek_hip_version() == 3


@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_argument_errors_without_gpu(name, data):
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

    def call(problem=1, n=n, batch=batch, A=p, lda=n, sA=n * n, B=p, ldb=n, sB=n * n, w=p, Z=p, ldz=n, sZ=n * n,
             info=ip, out=op, ipr=qp):
        return fn(problem, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, out, ipr, None)

    big = dict(lda=129, ldb=129, ldz=129, sA=129 * 129, sB=129 * 129, sZ=129 * 129)
    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(n=-1) == -2
    assert call(n=129, **big) == -2
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
    # the first offending argument decides
    assert call(problem=3, n=-1, batch=-1) == -1
    assert call(n=200, batch=-1, A=None) == -2
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
    for kw in (dict(batch=0), dict(n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0)):
        sec = ctypes.c_double(-1.0)
        args = dict(problem=1, n=n, batch=batch, lda=n, sA=n * n, ldb=n, sB=n * n, ldz=n, sZ=n * n)
        args.update(kw)
        rc = fn(args["problem"], args["n"], args["batch"], None, args["lda"], args["sA"], None, args["ldb"], args["sB"],
                None, None, args["ldz"], args["sZ"], None, None, None, ctypes.byref(sec))
        assert rc == 0 and sec.value == 0.0
    assert np.all(buf == 3.5) and np.all(out == 777.0) and np.all(ipr == 777.0)


@pytest.mark.parametrize("data", ["host", "garbage"])
@pytest.mark.parametrize("name", VARIABLE)
def test_variable_argument_errors_without_gpu(name, data):
    lib = solver.load_library()
    fn = getattr(lib, name)
    orders = np.array([4, 0, 3], dtype=np.int32)
    batch = len(orders)
    bufs = [np.full(16, 3.5) for _ in range(batch)]
    out = np.full(batch * 4, 777.0)
    info = np.zeros(batch, dtype=np.int32)

    def ptrs(null_at=None):
        return (ctypes.c_void_p * batch)(*[None if b == null_at else (GARBAGE if data == "garbage" else bufs[b].ctypes.data)
                                          for b in range(batch)])

    def ints(v):
        return np.array(v, dtype=np.int32)

    ld_ok = ints([4, 1, 3])
    keep = []

    def call(problem=1, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok", ldz=ld_ok,
             info=info, out=out, ipr="ok"):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x, t=_ip):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(t)
        return fn(problem, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info), I(out, _dp), P(ipr),
                  None)

    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(batch=-1) == -2
    assert call(n=None) == -3
    assert call(n=ints([4, -1, 3])) == -3
    assert call(n=ints([4, 0, 129]), lda=ints([4, 1, 129]), ldb=ints([4, 1, 129]), ldz=ints([4, 1, 129])) == -3
    assert call(A=None) == -4
    assert call(A=ptrs(null_at=2)) == -4
    assert call(lda=None) == -5
    assert call(lda=ints([3, 1, 3])) == -5
    assert call(lda=ints([4, 0, 3])) == -5           # lda[b] >= max(1, n[b]) also for an empty problem
    assert call(B=None) == -6
    assert call(B=ptrs(null_at=0)) == -6
    assert call(ldb=None) == -7
    assert call(ldb=ints([4, 1, 2])) == -7
    assert call(w=None) == -8
    assert call(w=ptrs(null_at=2)) == -8
    assert call(Z=None) == -9
    assert call(Z=ptrs(null_at=0)) == -9
    assert call(ldz=None) == -10
    assert call(ldz=ints([4, 1, 2])) == -10
    assert call(out=None) == -12
    # a NULL entry is legal where the problem is empty: the next offender decides
    assert call(A=ptrs(null_at=1), B=ptrs(null_at=1), w=ptrs(null_at=1), Z=ptrs(null_at=1), out=None) == -12
    # the first offending argument decides
    assert call(problem=2, batch=-1, n=None) == -1
    assert call(batch=-1, n=None, A=None) == -2
    assert call(n=ints([4, 0, 200]), A=None) == -3
    assert call(A=ptrs(null_at=0), lda=ints([1, 1, 1]), out=None) == -4
    assert call(lda=ints([1, 1, 1]), B=None, out=None) == -5
    assert call(B=None, ldb=None, w=None) == -6
    assert call(ldb=None, w=None, Z=None) == -7
    assert call(w=None, Z=None, out=None) == -8
    assert call(Z=None, ldz=None, out=None) == -9
    assert call(ldz=None, out=None) == -10
    # B and ldb are not looked at for problem 0; info = NULL and ipr = NULL are legal
    assert call(problem=0, B=None, ldb=None, out=None) == -12
    assert call(problem=0, B=None, ldb=ints([0, 0, 0]), w=None) == -8
    assert call(info=None, ipr=None, out=None) == -12
    assert call(info=None, ipr=None, ldz=None) == -10
    # nothing to do: success without a device and without touching any pointer
    assert call(batch=0, n=None, A=None, lda=None, B=None, ldb=None, w=None, Z=None, ldz=None, info=None, out=None,
                ipr=None) == 0
    assert np.all(out == 777.0)
    for b in bufs:
        assert np.all(b == 3.5)


@pytest.mark.parametrize("name", VARIABLE)
def test_variable_all_orders_zero_or_skipped_needs_no_device(name):
    """Every problem empty or skipped: the slots are filled on the host and no data pointer is looked at -- a_norm = 0 and
    NaN (0 / 0) for an order of 0, four NaN for a skipped problem, whose IPR slots keep what they held."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    n = np.array([0, 5, 0], dtype=np.int32)
    ld = np.array([1, 5, 1], dtype=np.int32)
    info = np.array([0, 3, 7], dtype=np.int32)
    out = np.full(12, 777.0)
    q = np.full(5, 777.0)
    data = (ctypes.c_void_p * 3)(None, GARBAGE, None)
    iprs = (ctypes.c_void_p * 3)(None, q.ctypes.data, None)
    sec = ctypes.c_double(-1.0)
    rc = fn(1, 3, n.ctypes.data_as(_ip), data, ld.ctypes.data_as(_ip), data, ld.ctypes.data_as(_ip), data, data,
            ld.ctypes.data_as(_ip), info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), iprs, ctypes.byref(sec))
    assert rc == 0 and sec.value == 0.0
    assert out[0] == 0.0 and np.all(np.isnan(out[1:]))
    assert np.all(q == 777.0)


def test_python_mirrors_reject_bad_shapes_before_the_library():
    z3, z4 = np.zeros((2, 3, 3)), np.zeros((2, 4, 4))
    for bad in (dict(A=np.zeros((2, 3, 4))), dict(A=np.zeros((3, 3))), dict(B=z4), dict(Z=z4), dict(w=np.zeros((2, 4))),
                dict(w=np.zeros(6)), dict(info=np.zeros(3, dtype=np.int32)), dict(info=np.zeros((2, 1), dtype=np.int32))):
        kw = dict(A=z3, B=z3, w=np.zeros((2, 3)), Z=z3, info=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            solver.check_batched(kw["A"], kw["B"], kw["w"], kw["Z"], info=kw["info"])
    m3, m4 = np.zeros((3, 3)), np.zeros((4, 4))
    for bad in (dict(As=[np.zeros((3, 4))]), dict(As=[np.zeros(4)]), dict(Bs=[m4, m4]), dict(Bs=[m4]), dict(Zs=[m4, m4]),
                dict(Zs=[m4]), dict(ws=[np.zeros(4), np.zeros(4)]), dict(ws=[np.zeros(4)]),
                dict(info=np.zeros(3, dtype=np.int32))):
        kw = dict(As=[m4, m3], Bs=[m4, m3], ws=[np.zeros(4), np.zeros(3)], Zs=[m4, m3], info=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            solver.check_vbatched(kw["As"], kw["Bs"], kw["ws"], kw["Zs"], info=kw["info"])
    # decided without a device: nothing to check, orders of 0, skipped problems
    out, q = solver.check_vbatched([], None, [], [])
    assert out.shape == (0, 4) and q == []
    out, q = solver.check_batched(np.zeros((0, 5, 5)), None, np.zeros((0, 5)), np.zeros((0, 5, 5)))
    assert out.shape == (0, 4) and q.shape == (0, 5)
    out, q = solver.check_batched(np.zeros((2, 0, 0)), None, np.zeros((2, 0)), np.zeros((2, 0, 0)), info=[0, 1])
    assert out[0, 0] == 0.0 and np.all(np.isnan(out[0, 1:])) and np.all(np.isnan(out[1])) and q.shape == (2, 0)
    out, q = solver.check_vbatched([np.zeros((0, 0)), m3], [np.zeros((0, 0)), m3], [np.zeros(0), np.zeros(3)],
                                   [np.zeros((0, 0)), m3], info=[0, 2], ipr=False)
    assert q is None and out[0, 0] == 0.0 and np.all(np.isnan(out[0, 1:])) and np.all(np.isnan(out[1]))
    with pytest.raises(solver.SolverError) as ei:
        solver.check_vbatched([np.zeros((129, 129))], None, [np.zeros(129)], [np.zeros((129, 129))])
    assert ei.value.info == -3
