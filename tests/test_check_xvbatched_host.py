"""Host-side checks of the variable-order acceptance checks for orders up to EK_HIP_XBATCH_NMAX (ek_hip_check_xvbatched*,
ek_hip_check_sygv_xvbatched*): declared in the boundary header, exported, bound by the Python mirror argument for argument
as their vbatched counterparts, the last-call hook a debug entry, every argument error decided before any device work and
without dereferencing a pointer of the pointer arrays, and the driver's "nothing to launch" path with orders of the new
class in the batch (no GPU needed: the data pointers are NULL, host addresses of small buffers or garbage).  The pattern
is test_check_xbatched_host.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("ek_hip_check_xvbatched_device", "ek_hip_check_xvbatched")
SYGV = ("ek_hip_check_sygv_xvbatched_device", "ek_hip_check_sygv_xvbatched")
OLD = ("ek_hip_check_vbatched_device", "ek_hip_check_vbatched", "ek_hip_check_sygv_vbatched_device",
       "ek_hip_check_sygv_vbatched")
HOOK = "ek_hip_debug_check_xvbatched_last"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced
NB = 200                                            # the order above EK_HIP_BATCH_NMAX every batch here holds


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return hdr, dbg, set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_check_xvbatched_entries_declared_exported_and_bound():
    hdr, _, declared, hooks = _headers()
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in PLAIN + SYGV:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        twin = getattr(lib, name.replace("xvbatched", "vbatched"))
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
        assert list(fn.argtypes) == list(twin.argtypes)                  # argument for argument
        at = fn.argtypes
        assert at[2] is _ip and at[10] is _ip and at[11] is _dp and at[13] is _dp     # n, info, out, seconds: host arrays
    assert "Not offered: a check of the variable-order form" not in hdr
    assert "Not offered: acceptance checks of the variable form" not in hdr
    assert "Not offered at these orders: a check of the variable-order form" not in hdr
    assert callable(solver.check_xvbatched) and callable(solver.check_sygv_xvbatched)
    assert callable(solver.check_xvbatched_last)
    assert lib.ek_hip_version() == 3
    assert solver.BATCH_NMAX == 128 and solver.XBATCH_NMAX == 256


def test_last_call_hook_is_a_debug_entry_and_answers_without_a_device():
    _, _, declared, hooks = _headers()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(solver.LIB_PATH), HOOK)
    lib = solver.load_library()
    fn = getattr(lib, HOOK)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [_dp, _ip]
    # host state only: four seconds and four counts (classes of 256, 128, 64, 32), either pointer may be NULL
    sec, cnt = np.full(5, -1.0), np.full(5, -1, dtype=np.int32)
    assert fn(sec.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip)) == 0
    assert np.all(sec[:4] >= 0.0) and np.all(cnt[:4] >= 0) and sec[4] == -1.0 and cnt[4] == -1
    assert fn(None, None) == 0
    s2, c2 = solver.check_xvbatched_last()
    assert s2.shape == (4,) and c2.shape == (4,) and np.array_equal(s2, sec[:4]) and np.array_equal(c2, cnt[:4])


@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", PLAIN + SYGV)
def test_argument_errors_without_gpu(name, data):
    """-k for argument k of the prototype, the first offender deciding; no pointer of the pointer arrays is dereferenced
    (host addresses of 16 doubles, which an order-200 problem would overrun, or the garbage pointer)."""
    lib = solver.load_library()
    fn = getattr(lib, name)
    sygv = name in SYGV
    orders = np.array([4, 0, NB], dtype=np.int32)
    batch = len(orders)
    bufs = [np.full(16, 3.5) for _ in range(batch)]
    out = np.full(batch * 4, 777.0)
    iprs = [np.full(NB, 777.0) for _ in range(batch)]
    info = np.zeros(batch, dtype=np.int32)

    def ptrs(null_at=None):
        return (ctypes.c_void_p * batch)(*[None if b == null_at else (GARBAGE if data == "garbage" else bufs[b].ctypes.data)
                                           for b in range(batch)])

    def ints(v):
        return np.array(v, dtype=np.int32)

    ld_ok = ints([4, 1, NB])
    qtab = (ctypes.c_void_p * batch)(*[q.ctypes.data for q in iprs])
    keep = []

    def call(first=1, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok", ldz=ld_ok, info=info,
             out=out, ipr=qtab):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(_ip)
        return fn(first, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info),
                  out.ctypes.data_as(_dp) if out is not None else None, ipr, None)

    if sygv:
        assert call(first=0) == -1
        assert call(first=4) == -1
        for itype in (1, 2, 3):
            assert call(first=itype, out=None) == -12
    else:
        assert call(first=2) == -1
        assert call(first=-1) == -1
    assert call(batch=-1) == -2
    assert call(n=None) == -3
    assert call(n=ints([4, -1, NB])) == -3
    big = ints([4, 1, 257])
    assert call(n=ints([4, 0, 257]), lda=big, ldb=big, ldz=big) == -3
    assert call(A=None) == -4
    assert call(A=ptrs(null_at=2)) == -4
    assert call(lda=None) == -5
    assert call(lda=ints([4, 1, NB - 1])) == -5
    assert call(lda=ints([4, 0, NB])) == -5          # lda[b] >= max(1, n[b]) also for an empty problem
    assert call(B=None) == -6
    assert call(B=ptrs(null_at=2)) == -6
    assert call(ldb=None) == -7
    assert call(ldb=ints([4, 1, NB - 1])) == -7
    assert call(w=None) == -8
    assert call(w=ptrs(null_at=2)) == -8
    assert call(Z=None) == -9
    assert call(Z=ptrs(null_at=2)) == -9
    assert call(ldz=None) == -10
    assert call(ldz=ints([4, 1, NB - 1])) == -10
    assert call(out=None) == -12
    assert call(info=None, ipr=None, out=None) == -12   # 11 is info, 13 is ipr: NULL is legal for both
    # orders 129, 200 and 256 are legal: the next offender decides, and no device is touched
    for edge in (129, 200, 256):
        ld = ints([4, 1, edge])
        kw = dict(n=ints([4, 0, edge]), lda=ld, ldb=ld, ldz=ld)
        assert call(A=ptrs(null_at=2), **kw) == -4
        assert call(**dict(kw, lda=ints([4, 1, edge - 1]))) == -5
        assert call(B=ptrs(null_at=2), **kw) == -6
        assert call(**dict(kw, ldb=ints([4, 1, edge - 1]))) == -7
        assert call(w=ptrs(null_at=2), **kw) == -8
        assert call(Z=ptrs(null_at=2), **kw) == -9
        assert call(**dict(kw, ldz=ints([4, 1, edge - 1]))) == -10
        assert call(out=None, **kw) == -12
        assert call(info=None, ipr=None, out=None, **kw) == -12
    # a NULL entry is legal where the problem is empty: the next offender decides
    assert call(A=ptrs(null_at=1), B=ptrs(null_at=1), w=ptrs(null_at=1), Z=ptrs(null_at=1), out=None) == -12
    # the first offending argument decides
    assert call(first=7, batch=-1, n=None) == -1
    assert call(batch=-1, n=None, A=None) == -2
    assert call(n=ints([4, 0, 300]), A=None) == -3
    assert call(A=ptrs(null_at=2), lda=ints([1, 1, 1]), out=None) == -4
    assert call(lda=ints([1, 1, 1]), B=None, out=None) == -5
    assert call(B=None, ldb=None, w=None) == -6
    assert call(ldb=None, w=None, Z=None) == -7
    assert call(w=None, Z=None, out=None) == -8
    assert call(Z=None, ldz=None, out=None) == -9
    assert call(ldz=None, out=None) == -10
    # B and ldb are not looked at for problem 0 -- but the sygv forms always require B, whatever the type
    if sygv:
        for itype in (1, 2, 3):
            assert call(first=itype, B=None, ldb=None, out=None) == -6
            assert call(first=itype, B=ptrs(null_at=2), out=None) == -6
            assert call(first=itype, ldb=ints([0, 0, 0]), w=None) == -7
    else:
        assert call(first=0, B=None, ldb=None, out=None) == -12
        assert call(first=0, B=None, ldb=ints([0, 0, 0]), w=None) == -8
    # nothing to do: success without a device and without touching any pointer
    sec = ctypes.c_double(-1.0)
    assert fn(1, 0, None, None, None, None, None, None, None, None, None, None, None, ctypes.byref(sec)) == 0
    assert sec.value == 0.0
    assert np.all(out == 777.0) and not info.any()
    assert all(np.all(b == 3.5) for b in bufs) and all(np.all(q == 777.0) for q in iprs)


@pytest.mark.parametrize("name", OLD)
def test_the_old_variable_entries_still_stop_at_128(name):
    fn = getattr(solver.load_library(), name)
    bufs = [np.full(16, 3.5) for _ in range(2)]
    tab = (ctypes.c_void_p * 2)(*[b.ctypes.data for b in bufs])
    out = np.full(8, 777.0)

    def call(top, outp):
        n = np.array([4, top], dtype=np.int32)
        ni = n.ctypes.data_as(_ip)
        return fn(1, 2, ni, tab, ni, tab, ni, tab, tab, ni, None, outp, None, None)

    assert call(129, out.ctypes.data_as(_dp)) == -3
    assert call(256, out.ctypes.data_as(_dp)) == -3
    assert call(128, None) == -12
    assert np.all(out == 777.0) and all(np.all(b == 3.5) for b in bufs)


@pytest.mark.parametrize("name,first", [(nm, f) for nm in PLAIN for f in (0, 1)] + [(nm, f) for nm in SYGV for f in (1, 2, 3)])
def test_nothing_to_launch_needs_no_device(name, first):
    """Orders (0, 200, 256) with info = (0, 7, -5): nothing is launched, the slots are filled on the host, the skipped
    problems' ipr rows stay and none of their (garbage) data pointers is dereferenced -- in both forms."""
    fn = getattr(solver.load_library(), name)
    n = np.array([0, 200, 256], dtype=np.int32)
    ld = np.maximum(n, 1).astype(np.int32)
    info = np.array([0, 7, -5], dtype=np.int32)
    tab = (ctypes.c_void_p * 3)(None, GARBAGE, GARBAGE)
    out = np.full(12, 777.0)
    iprs = [np.full(256, 777.0) for _ in range(3)]
    qtab = (ctypes.c_void_p * 3)(*[q.ctypes.data for q in iprs])
    sec = ctypes.c_double(-1.0)
    ni, li = n.ctypes.data_as(_ip), ld.ctypes.data_as(_ip)
    rc = fn(first, 3, ni, tab, li, tab, li, tab, tab, li, info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), qtab,
            ctypes.byref(sec))
    assert rc == 0 and sec.value == 0.0
    o = out.reshape(3, 4)
    assert o[0, 0] == 0.0 and np.all(np.isnan(o[0, 1:]))
    assert np.all(np.isnan(o[1:]))
    assert all(np.all(q == 777.0) for q in iprs)
    sec4, cnt4 = solver.check_xvbatched_last()
    assert not cnt4.any() and not sec4.any()          # the call was given `seconds`: four empty classes


def test_python_mirror_errors_and_empty_batches():
    z3, z4 = np.zeros((3, 3)), np.zeros((4, 4))
    for fn in (solver.check_xvbatched, lambda As, Bs, ws, Zs, **kw: solver.check_sygv_xvbatched(As, Bs, ws, Zs, **kw)):
        for bad in (dict(As=[np.zeros((3, 4))]), dict(Bs=[z4]), dict(Zs=[z4]), dict(ws=[np.zeros(4)]),
                    dict(info=np.zeros(2, dtype=np.int32))):
            kw = dict(As=[z3], Bs=[z3], ws=[np.zeros(3)], Zs=[z3], info=None)
            kw.update(bad)
            with pytest.raises(ValueError):
                fn(kw["As"], kw["Bs"], kw["ws"], kw["Zs"], info=kw["info"])
        out, q = fn([], [], [], [])
        assert out.shape == (0, 4) and q == []
        # an order beyond the last: argument 3
        big = np.zeros((257, 257))
        with pytest.raises(solver.SolverError) as ei:
            fn([z4, big], [z4, big], [np.zeros(4), np.zeros(257)], [z4, big])
        assert ei.value.info == -3
        # decided on the host: an empty problem and a skipped one of order 200
        z0, zb = np.zeros((0, 0)), np.zeros((200, 200))
        out, q = fn([z0, zb], [z0, zb], [np.zeros(0), np.zeros(200)], [z0, zb], info=[0, 3])
        assert out[0, 0] == 0.0 and np.all(np.isnan(out[0, 1:])) and np.all(np.isnan(out[1]))
        assert q[0].shape == (0,) and np.all(np.isnan(q[1]))
    with pytest.raises(ValueError):
        solver.check_sygv_xvbatched([z4], None, [np.zeros(4)], [z4])
    for itype in (0, 4):
        with pytest.raises(ValueError):
            solver.check_sygv_xvbatched([z4], [z4], [np.zeros(4)], [z4], itype=itype)
    # the old wrapper still refuses order 129
    zz = np.zeros((129, 129))
    with pytest.raises(solver.SolverError) as ei:
        solver.check_vbatched([z4, zz], None, [np.zeros(4), np.zeros(129)], [z4, zz])
    assert ei.value.info == -3
