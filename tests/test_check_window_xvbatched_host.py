"""Host-side contract of the variable-order window checks (ek_hip_check_window_xvbatched*,
ek_hip_check_sygv_window_xvbatched*); no GPU: the symbols and their binding, every argument error in
prototype order with NULL, host and garbage data pointers (garbage must never be dereferenced), the skipped and empty
problems that are answered without a device, and that the neighbouring check entries refuse what they refused."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("ek_hip_check_window_xvbatched_device", "ek_hip_check_window_xvbatched")
SYGV = ("ek_hip_check_sygv_window_xvbatched_device", "ek_hip_check_sygv_window_xvbatched")
NAMES = PLAIN + SYGV
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced
ORDERS = (129, 200, 256)                            # the defaults: three problems, all above EK_HIP_BATCH_NMAX
SENTINEL = 777.0
ARGS = ["batch", "n", "dA", "lda", "dB", "ldb", "m", "dw", "dZ", "ldz", "zcap", "info", "out", "ipr", "seconds"]


def test_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    vp = ctypes.c_void_p
    for name in NAMES:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
        # first, batch, n | A, lda | B, ldb | m | w, Z, ldz, zcap | info, out, ipr, seconds
        assert list(fn.argtypes) == [ctypes.c_int, ctypes.c_int, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip, _ip, _dp, vp,
                                     _dp]
        # the 14 arguments of the full variable check with m in front of w and zcap behind ldz
        full = list(getattr(lib, name.replace("_window", "")).argtypes)
        assert full[:7] + [_ip] + full[7:10] + [_ip] + full[10:] == list(fn.argtypes)
        # the solver's own m, w, Z, ldz, zcap, info sit in the same order in its prototype
        twin = name.replace("check_sygv_window", "sygv_window").replace("check_window", "eigenpairs_window")
        assert list(getattr(lib, twin).argtypes)[13:19] == list(fn.argtypes)[7:13]
        proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        args = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
        first = "itype" if "sygv" in name else "problem"
        want = ARGS if name.endswith("_device") else [a[1:] if a in ("dA", "dB", "dw", "dZ") else a for a in ARGS]
        assert args == [first] + want
    assert callable(solver.check_window_xvbatched) and callable(solver.check_sygv_window_xvbatched)
    assert lib.ek_hip_version() == 3
    # the two uniform window checks point to the variable forms
    assert hdr.count("ek_hip_check_window_xvbatched* below") >= 1
    assert hdr.count("ek_hip_check_sygv_window_xvbatched* below") >= 1


class _Call:
    """One entry with legal defaults for a batch of three problems of the orders above: every data pointer is NULL-able, a
    host address of 16 doubles (which such a problem would overrun) or the garbage pointer."""

    def __init__(self, name, data):
        self.fn = getattr(solver.load_library(), name)
        self.sygv = "sygv" in name
        self.buf = np.full(16, 3.5)
        self.data = data
        self.out = np.full(3 * 4 + 1, SENTINEL)
        self.rows = [np.full(257, SENTINEL) for _ in range(3)]
        self.keep = []

    def table(self, v, count):
        """None: no array; "ok": `count` entries; a tuple of "ok" / None: those entries."""
        if v is None:
            return None
        if v == "ok":
            v = ("ok",) * count
        addr = GARBAGE if self.data == "garbage" else self.buf.ctypes.data
        t = (ctypes.c_void_p * max(len(v), 1))(*[addr if x is not None else None for x in v])
        self.keep.append(t)
        return t

    def ints(self, v):
        if v is None:
            return None
        a = np.array(v, dtype=np.int32)
        self.keep.append(a)
        return a.ctypes.data_as(_ip)

    def __call__(self, first=None, batch=3, n=ORDERS, A="ok", lda=ORDERS, B="ok", ldb=ORDERS, m=(5, 0, 256), w="ok",
                 Z="ok", ldz=ORDERS, zcap=(5, 0, 256), info=(0, 0, 0), out="ok", ipr="ok", seconds=None):
        if first is None:
            first = 3 if self.sygv else 1
        count = max(batch, 0)
        rows = None
        if ipr is not None:
            rows = (ctypes.c_void_p * 3)(*[r.ctypes.data for r in self.rows])
            self.keep.append(rows)
        return self.fn(first, batch, self.ints(n), self.table(A, count), self.ints(lda), self.table(B, count),
                       self.ints(ldb), self.ints(m), self.table(w, count), self.table(Z, count), self.ints(ldz),
                       self.ints(zcap), self.ints(info), self.out.ctypes.data_as(_dp) if out is not None else None, rows,
                       seconds)

    def untouched(self):
        return np.all(self.out == SENTINEL) and all(np.all(r == SENTINEL) for r in self.rows)


@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_in_prototype_order(name, data):
    call = _Call(name, data)
    ok = ("ok", "ok", None)
    big = (129, 200, solver.XBATCH_NMAX + 1)
    assert call(first=4 if call.sygv else 2) == -1
    assert call(first=0 if call.sygv else -1) == -1
    assert call(batch=-1) == -2
    assert call(n=None) == -3
    assert call(n=(129, -1, 256)) == -3
    assert call(n=big, lda=big, ldb=big, ldz=big) == -3               # 257
    assert call(A=None) == -4
    assert call(A=ok) == -4
    assert call(lda=None) == -5
    assert call(lda=(129, 199, 256)) == -5
    assert call(B=None) == -6
    assert call(B=ok) == -6
    assert call(ldb=None) == -7
    assert call(ldb=(128, 200, 256)) == -7
    assert call(m=None) == -8
    assert call(m=(5, -1, 256)) == -8
    assert call(m=(5, 201, 256), zcap=(5, 256, 256)) == -8            # above n[1] = 200
    assert call(w=None) == -9
    assert call(w=ok) == -9
    assert call(Z=None) == -10
    assert call(Z=ok) == -10                                           # zcap[2] > 0
    assert call(ldz=None) == -11
    assert call(ldz=(129, 200, 255)) == -11
    assert call(zcap=None) == -12
    assert call(zcap=(5, -1, 256)) == -12
    assert call(zcap=(4, 0, 256)) == -12                               # below m[0]
    assert call(out=None) == -14
    assert call.untouched()                                            # nothing was written on the way to an error
    # the orders 129, 200 and 256 are legal: with everything skipped or empty the call succeeds without a device
    assert call(m=(0, 0, 0), zcap=(0, 0, 0), Z=None) == -10
    assert call(m=(0, 0, 0), zcap=(0, 0, 0), Z=(None, None, None)) == 0    # a NULL dZ[b] where zcap[b] = 0
    assert call(m=(0, 0, 0), zcap=(0, 3, 0), Z=("ok", None, "ok")) == -10
    # an order 0 needs no entry anywhere and a leading dimension of 1
    assert call(n=(129, 0, 256), lda=(129, 1, 256), ldb=(129, 1, 256), ldz=(129, 1, 256), A=("ok", None, "ok"),
                B=("ok", None, "ok"), w=("ok", None, "ok"), Z=("ok", None, "ok"), m=(0, 0, 0), zcap=(1, 4, 1)) == 0
    assert call(n=(129, 0, 256), lda=(129, 0, 256), m=(0, 0, 0)) == -5
    assert call(n=(129, 0, 256), m=(0, 1, 0), zcap=(1, 4, 1)) == -8    # n[b] = 0 forces m[b] = 0


@pytest.mark.parametrize("name", PLAIN)
def test_problem_0_does_not_look_at_b(name):
    call = _Call(name, "garbage")
    assert call(first=0, B=None, ldb=None, out=None) == -14
    assert call(first=0, B=None, ldb=None, m=(0, 0, 0)) == 0
    assert call(first=1, B=None, m=(0, 0, 0)) == -6


@pytest.mark.parametrize("name", SYGV)
def test_sygv_forms_itype_first_and_b_always(name):
    call = _Call(name, "garbage")
    for bad in (0, 4, -1):
        assert call(first=bad, batch=0) == -1                          # before everything, batch = 0 included
        assert call(first=bad, batch=-1, n=None, out=None) == -1
    for itype in (1, 2, 3):
        assert call(first=itype, B=None) == -6
        assert call(first=itype, ldb=None) == -7
        assert call(first=itype, B=None, ldb=None, m=None) == -6
        assert call(first=itype, batch=0) == 0
        assert call(first=itype, m=(0, 0, 0)) == 0
    assert not call.untouched()                                        # the last calls wrote their NaN
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL


@pytest.mark.parametrize("name", NAMES)
def test_the_first_offender_decides(name):
    call = _Call(name, "garbage")
    assert call(first=7, batch=-1) == -1
    assert call(batch=-1, n=None) == -2
    assert call(n=None, A=None) == -3
    assert call(A=None, lda=None) == -4
    assert call(lda=None, B=None) == -5
    assert call(B=None, ldb=None) == -6
    assert call(ldb=None, m=None) == -7
    assert call(m=None, w=None) == -8
    assert call(m=(257, 0, 0), w=None) == -8
    assert call(m=(5, 0, 256), zcap=(3, 0, 256), w=None) == -9         # m against zcap is argument 12: w comes first
    assert call(w=None, Z=None) == -9
    assert call(Z=None, ldz=None) == -10
    assert call(Z=("ok", "ok", None), zcap=None) == -12                # without zcap a NULL entry of dZ cannot be judged
    assert call(ldz=None, zcap=None) == -11
    assert call(zcap=(4, 0, 256), out=None) == -12
    assert call(out=None, ipr=None) == -14
    assert call.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_m_beyond_zcap_or_n_is_ignored_under_info_and_refused_without(name):
    call = _Call(name, "garbage")
    # every problem skipped or empty: legal, and answered without a device (see below)
    assert call(m=(129 + 7, 0, -3), info=(-20, 0, 5), zcap=(4, 0, 4)) == 0
    assert call(m=(9, 0, 0), info=(-20, 0, 0), zcap=(4, 0, 4)) == 0
    # the same counts without the info that excuses them
    assert call(m=(129 + 7, 0, 0), info=(0, 0, 0), zcap=(4, 0, 4)) == -8
    assert call(m=(129 + 7, 0, 0), info=None, zcap=(4, 0, 4)) == -8
    assert call(m=(9, 0, 0), info=(0, 0, 0), zcap=(4, 0, 4)) == -12
    assert call(m=(9, 0, 0), info=None, zcap=(4, 0, 4)) == -12
    assert call(m=(0, 0, -3), info=(0, 0, 0)) == -8
    # a negative zcap is refused whatever info says
    assert call(m=(9, 0, 0), info=(-20, 0, 0), zcap=(-1, 0, 4)) == -12


@pytest.mark.parametrize("name", NAMES)
def test_batch_0_references_nothing(name):
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    assert call(batch=0, n=None, A=None, lda=None, B=None, ldb=None, m=None, w=None, Z=None, ldz=None, zcap=None,
                info=None, out=None, ipr=None, seconds=ctypes.byref(sec)) == 0
    assert sec.value == 0.0
    assert call(batch=0) == 0
    assert call.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_of_skipped_empty_and_order_0_problems_is_filled_without_a_device(name):
    """Garbage data pointers, and no ek_hip_init: four NaN per problem -- the order 0 included, which the full variable
    check would give a_norm = 0 --, the ipr rows and what lies behind `out` left as they were."""
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    one = (256, 0, 129)
    assert call(n=one, lda=(256, 1, 129), ldb=(256, 1, 129), ldz=(256, 1, 129), m=(300, 0, 0), info=(-20, 0, 0),
                zcap=(7, 0, 3), A=("ok", None, "ok"), B=("ok", None, "ok"), w=("ok", None, "ok"), Z=("ok", None, "ok"),
                seconds=ctypes.byref(sec)) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL
    assert all(np.all(r == SENTINEL) for r in call.rows)
    assert sec.value == 0.0
    call.out[:] = SENTINEL
    assert call(m=(0, 44, 0), info=(0, 3, 0), ipr=None) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL


def test_the_existing_check_entries_refuse_what_they_refused():
    lib = solver.load_library()
    g = ctypes.c_void_p(GARBAGE)
    gd = ctypes.cast(GARBAGE, _dp)
    out = np.full(4, SENTINEL)
    op = out.ctypes.data_as(_dp)
    N = 200
    nb = solver.XBATCH_NMAX + 1
    m = np.array([5], dtype=np.int32)
    mp = m.ctypes.data_as(_ip)
    for entry, first in (("ek_hip_check_window_xbatched", 1), ("ek_hip_check_sygv_window_xbatched", 3)):
        for suffix, p in (("_device", g), ("", gd)):
            fn = getattr(lib, entry + suffix)
            assert fn(first, nb, 1, p, nb, nb * nb, p, nb, nb * nb, mp, p, p, nb, nb, nb * nb, None, op, None, None) == -2
            assert fn(first, N, 1, p, N, N * N, p, N, N * N, None, p, p, N, N, N * N, None, op, None, None) == -10
            assert fn(first, N, 1, p, N, N * N, p, N, N * N, mp, p, p, N, 4, N * N, None, op, None, None) == -14
            assert fn(first, N, 1, p, N, N * N, p, N, N * N, mp, p, p, N, N, N * N, None, None, None, None) == -17
    n1 = np.array([nb], dtype=np.int32)
    n2 = np.array([N], dtype=np.int32)
    tab = (ctypes.c_void_p * 1)(GARBAGE)
    for entry, first in (("ek_hip_check_xvbatched", 1), ("ek_hip_check_sygv_xvbatched", 3)):
        for suffix in ("_device", ""):
            fn = getattr(lib, entry + suffix)
            i1, i2 = n1.ctypes.data_as(_ip), n2.ctypes.data_as(_ip)
            assert fn(first, 1, i1, tab, i1, tab, i1, tab, tab, i1, None, op, None, None) == -3
            assert fn(first, 1, i2, tab, i2, tab, i2, None, tab, i2, None, op, None, None) == -8
            assert fn(first, 1, i2, tab, i2, tab, i2, tab, tab, i2, None, None, None, None) == -12
    assert lib.ek_hip_check_sygv_xvbatched_device(0, 0, None, None, None, None, None, None, None, None, None, None, None,
                                                  None) == -1
    assert np.all(out == SENTINEL)


def test_python_wrappers_shapes_and_device_free_paths():
    As = [np.zeros((5, 5)), np.zeros((0, 0)), np.eye(200)]
    Zs = [np.zeros((5, 2)), np.zeros((0, 0)), np.zeros((200, 0))]
    ws = [np.zeros(2), np.zeros(0), np.zeros(0)]
    with pytest.raises(ValueError):
        solver.check_window_xvbatched(As, None, [1, 0], ws, Zs)
    with pytest.raises(ValueError):
        solver.check_window_xvbatched(As, None, [1, 0, 0], ws, [np.zeros((4, 2))] + Zs[1:])
    with pytest.raises(ValueError):
        solver.check_window_xvbatched(As, None, [1, 0, 0], ws, Zs, zcap=3)
    with pytest.raises(ValueError):
        solver.check_window_xvbatched(As, None, [2, 0, 0], [np.zeros(1)] + ws[1:], Zs)
    with pytest.raises(ValueError):
        solver.check_sygv_window_xvbatched(As, None, [0, 0, 0], ws, Zs, itype=2)
    with pytest.raises(ValueError):
        solver.check_sygv_window_xvbatched(As, As, [0, 0, 0], ws, Zs, itype=4)
    with pytest.raises(solver.SolverError) as e:
        solver.check_window_xvbatched(As, None, [3, 0, 0], [np.zeros(3)] + ws[1:], Zs)
    assert e.value.info == -12
    with pytest.raises(solver.SolverError) as e:
        solver.check_window_xvbatched(As, None, [0, 1, 0], ws, Zs)
    assert e.value.info == -8
    for call in (lambda **kw: solver.check_window_xvbatched(As, None, [7, 0, 0], ws, Zs, info=[-20, 0, 0], **kw),
                 lambda **kw: solver.check_sygv_window_xvbatched(As, As, [7, 0, 0], ws, Zs, itype=3, info=[-20, 0, 0],
                                                                 **kw)):
        out, ipr = call()
        assert out.shape == (3, 4) and np.all(np.isnan(out))
        assert [q.shape for q in ipr] == [(5,), (0,), (200,)] and all(np.all(np.isnan(q)) for q in ipr)
        out, ipr = call(ipr=False)
        assert ipr is None and np.all(np.isnan(out))
    out, ipr = solver.check_window_xvbatched([], None, [], [], [])
    assert out.shape == (0, 4) and ipr == []
