"""Host-side checks of the window check of DSYGV's types (ek_hip_check_sygv_window_xbatched*): declared in
the boundary header, exported, bound by the Python mirror argument for argument, every argument error decided in the order
of the prototype before any device work and without dereferencing a data pointer (-1 for the type before everything, B
required for every type), the device-free paths (n = 0, batch = 0, a batch of only skipped and empty problems), the
unchanged refusals of ek_hip_check_window_xbatched*, and the host mirror verifier.*_sygv on the window's columns against a
long-double evaluation.  No GPU needed: the data pointers are NULL, host addresses of small buffers or garbage.

Measured on the CPU (test_the_mirror_against_long_double, n = 129, 192, 256, c = n / 8 and 65, clean and planted): the
mirror's largest share of its bound -- 4 max(n, 8) eps, times max(1, cond_2(B)) for slot 3 and the IPRs of type 3 -- is
0.0183 (type 2 at n = 129: norm 0.0016, res_ave and res_max below 0.0001, orthogonality 0.0061, ipr 0.0183; type 3:
orthogonality 0.0012, ipr 0.0021 of the wider bound); the bound asserted is twice that, 0.037."""
import ctypes
import os
import re

import numpy as np
import pytest

import check_sygv_window_cases as cs
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_check_sygv_window_xbatched_device", "ek_hip_check_sygv_window_xbatched")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced
N = 200
SENTINEL = 777.0
MIRROR_BOUND = 0.037                                # twice the largest share measured (the docstring above)


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
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19
        at = list(fn.argtypes)
        # itype, n, batch | A, lda, strideA | B, ldb, strideB | m | w | Z, ldz, zcap, strideZ | info, out, ipr, seconds
        data = ctypes.c_void_p if name.endswith("_device") else _dp
        assert at == [ctypes.c_int] * 3 + [data, ctypes.c_int, ctypes.c_longlong] * 2 + [_ip, data, data, ctypes.c_int,
                                                                                        ctypes.c_int, ctypes.c_longlong,
                                                                                        _ip, _dp, _dp, _dp]
        # argument for argument the window check's own prototype
        assert at == list(getattr(lib, name.replace("check_sygv_window", "check_window")).argtypes)
        # the solvers' own m, w, Z, ldz, zcap, strideZ, info sit in the same order in their prototypes
        for solve in ("sygv_window_xbatched", "sygv_window_batched"):
            twin = list(getattr(lib, name.replace("check_sygv_window_xbatched", solve)).argtypes)
            assert twin[15:22] == at[9:16]
    proto = re.search(r"int ek_hip_check_sygv_window_xbatched_device\(([^;]*)\);", hdr).group(1)
    args = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert args == ["itype", "n", "batch", "dA", "lda", "strideA", "dB", "ldb", "strideB", "m", "dw", "dZ", "ldz", "zcap",
                    "strideZ", "info", "out", "ipr", "seconds"]
    assert callable(solver.check_sygv_window_xbatched)
    # the header offers what it said it did not, and still does not offer the variable-order form
    assert "Not offered: the window check of DSYGV's types 2 and 3" not in hdr
    assert "Not offered: a variable-order form" in hdr


class _Call:
    """One entry with legal defaults for a batch of three problems of order N: every data pointer is NULL-able, a host
    address of 16 doubles (which an order-200 problem would overrun) or the garbage pointer."""

    def __init__(self, name, data):
        self.fn = getattr(solver.load_library(), name)
        self.device = name.endswith("_device")
        self.buf = np.full(16, 3.5)
        self.data = data
        self.out = np.full(3 * 4 + 1, SENTINEL)
        self.ipr = np.full(3 * N + 1, SENTINEL)
        self.keep = []

    def ptr(self, x):
        if x is None:
            return None
        addr = GARBAGE if self.data == "garbage" else self.buf.ctypes.data
        return ctypes.c_void_p(addr) if self.device else ctypes.cast(addr, _dp)

    def ints(self, v):
        if v is None:
            return None
        a = np.array(v, dtype=np.int32)
        self.keep.append(a)
        return a.ctypes.data_as(_ip)

    def __call__(self, itype=2, n=N, batch=3, A="ok", lda=N, sA=N * N, B="ok", ldb=N, sB=N * N, m=(5, 0, N), w="ok",
                 Z="ok", ldz=N, zcap=N, sZ=N * N, info=(0, 0, 0), out="ok", ipr="ok", seconds=None):
        return self.fn(itype, n, batch, self.ptr(A), lda, sA, self.ptr(B), ldb, sB, self.ints(m), self.ptr(w),
                       self.ptr(Z), ldz, zcap, sZ, self.ints(info),
                       self.out.ctypes.data_as(_dp) if out is not None else None,
                       self.ipr.ctypes.data_as(_dp) if ipr is not None else None, seconds)


@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_in_prototype_order(name, data, itype):
    call = _Call(name, data)
    t = itype
    assert call(itype=0) == -1
    assert call(itype=4) == -1
    assert call(itype=-1) == -1
    assert call(itype=t, n=-1) == -2
    assert call(itype=t, n=solver.XBATCH_NMAX + 1, lda=300, ldb=300, ldz=300, sA=10 ** 6, sB=10 ** 6, sZ=10 ** 6) == -2
    assert call(itype=t, batch=-1) == -3
    assert call(itype=t, A=None) == -4
    assert call(itype=t, lda=N - 1) == -5
    assert call(itype=t, sA=N * N - 1) == -6
    assert call(itype=t, sA=0) == -6
    assert call(itype=t, B=None) == -7              # every type, type 1 included
    assert call(itype=t, ldb=N - 1) == -8
    assert call(itype=t, sB=N * N - 1) == -9
    assert call(itype=t, m=None) == -10
    assert call(itype=t, m=(5, -1, N)) == -10
    assert call(itype=t, m=(5, 0, N + 1)) == -10
    assert call(itype=t, w=None) == -11
    assert call(itype=t, Z=None) == -12
    assert call(itype=t, ldz=N - 1) == -13
    assert call(itype=t, zcap=-1) == -14
    assert call(itype=t, zcap=N - 1) == -14         # m[2] = N
    assert call(itype=t, m=(5, 0, 6), zcap=5, sZ=5 * N) == -14
    assert call(itype=t, sZ=N * N - 1) == -15
    assert call(itype=t, m=(0, 0, 0), zcap=0, sZ=N - 1) == -15        # ldz max(1, zcap)
    assert call(itype=t, out=None) == -17
    # nothing was written on the way to an error
    assert np.all(call.out == SENTINEL) and np.all(call.ipr == SENTINEL)


@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_the_first_offender_decides(name, itype):
    call = _Call(name, "garbage")
    t = itype
    # -1 comes before everything, n = 0 and batch = 0 included
    assert call(itype=0, n=-1, batch=-1, A=None, B=None, m=None, w=None, Z=None, out=None) == -1
    assert call(itype=4, n=0) == -1
    assert call(itype=0, batch=0) == -1
    assert call(itype=t, n=-1, batch=-1) == -2
    assert call(itype=t, batch=-1, A=None) == -3
    assert call(itype=t, A=None, lda=0) == -4
    assert call(itype=t, lda=0, sA=0) == -5
    assert call(itype=t, sA=0, B=None) == -6
    assert call(itype=t, B=None, ldb=0) == -7
    assert call(itype=t, ldb=0, sB=0) == -8
    assert call(itype=t, sB=0, m=(N + 1, 0, 0)) == -9
    assert call(itype=t, m=(N + 1, 0, 0), w=None) == -10
    assert call(itype=t, m=(5, 0, N), zcap=3, w=None) == -11          # m against zcap is argument 14: w comes first
    assert call(itype=t, w=None, Z=None) == -11
    assert call(itype=t, Z=None, ldz=0) == -12
    assert call(itype=t, ldz=0, zcap=-1) == -13
    assert call(itype=t, zcap=4, sZ=0) == -14       # m[0] = 5 > zcap before the stride
    assert call(itype=t, sZ=0, out=None) == -15
    assert call(itype=t, out=None, ipr=None) == -17
    assert np.all(call.out == SENTINEL) and np.all(call.ipr == SENTINEL)


@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_m_beyond_zcap_or_n_is_ignored_under_info_and_refused_without(name, itype):
    call = _Call(name, "garbage")
    t = itype
    # every problem skipped or empty: legal, and answered without a device (see below)
    assert call(itype=t, m=(N + 7, 0, -3), info=(-20, 0, 5), zcap=4, sZ=4 * N) == 0
    assert call(itype=t, m=(9, 0, 0), info=(-20, 0, 0), zcap=4, sZ=4 * N) == 0
    # the same counts without the info that excuses them
    assert call(itype=t, m=(N + 7, 0, 0), info=(0, 0, 0), zcap=4, sZ=4 * N) == -10
    assert call(itype=t, m=(N + 7, 0, 0), info=None, zcap=4, sZ=4 * N) == -10
    assert call(itype=t, m=(9, 0, 0), info=(0, 0, 0), zcap=4, sZ=4 * N) == -14
    assert call(itype=t, m=(9, 0, 0), info=None, zcap=4, sZ=4 * N) == -14
    assert call(itype=t, m=(0, 0, -3), info=(0, 0, 0)) == -10


@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_nothing_to_do_references_nothing(name, itype):
    """n = 0 and batch = 0: 0, nothing referenced or written, `seconds` aside (seconds = 0)."""
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    assert call(itype=itype, n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0, zcap=0, seconds=ctypes.byref(sec)) == 0
    assert sec.value == 0.0
    assert call(itype=itype, batch=0, m=None, info=None, A=None, B=None, w=None, Z=None, out=None, ipr=None) == 0
    assert call(itype=itype, n=0, m=None, A=None, B=None, w=None, Z=None, out=None, ipr=None) == 0
    assert np.all(call.out == SENTINEL) and np.all(call.ipr == SENTINEL)


@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_a_batch_of_skipped_and_empty_problems_is_filled_without_a_device(name, itype):
    """Garbage data pointers, and no ek_hip_init: four NaN per problem, the ipr rows and what lies behind `out` left."""
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    assert call(itype=itype, m=(0, 44, 0), info=(0, 3, 0), seconds=ctypes.byref(sec)) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL and np.all(call.ipr == SENTINEL)
    assert sec.value == 0.0
    call.out[:] = SENTINEL
    assert call(itype=itype, m=(0, 0, 0), info=None, zcap=0, sZ=N, ipr=None) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL


def test_the_window_check_itself_refuses_what_it_refused():
    """ek_hip_check_window_xbatched* keeps its codes: problem 2 and 3 are -1, problem 0 does not look at B."""
    lib = solver.load_library()
    out = np.full(4, SENTINEL)
    op = out.ctypes.data_as(_dp)
    m = np.array([5], dtype=np.int32)
    mp = m.ctypes.data_as(_ip)
    for name, p in (("ek_hip_check_window_xbatched_device", ctypes.c_void_p(GARBAGE)),
                    ("ek_hip_check_window_xbatched", ctypes.cast(GARBAGE, _dp))):
        fn = getattr(lib, name)
        for problem in (2, 3, -1):
            assert fn(problem, N, 1, p, N, N * N, p, N, N * N, mp, p, p, N, N, N * N, None, op, None, None) == -1
        assert fn(1, N, 1, p, N, N * N, None, N, N * N, mp, p, p, N, N, N * N, None, op, None, None) == -7
        assert fn(0, N, 1, p, N, N * N, None, 0, 0, mp, p, p, N, N, N * N, None, None, None, None) == -17
        assert fn(1, N, 1, p, N, N * N, p, N, N * N, mp, p, p, N, 4, N * N, None, op, None, None) == -14
    assert np.all(out == SENTINEL)


def test_python_wrapper_shapes_and_device_free_paths():
    A = np.zeros((3, 5, 5))
    Z = np.zeros((3, 5, 2))
    w = np.zeros((3, 5))
    for itype in (0, 4, None):
        with pytest.raises(ValueError):
            solver.check_sygv_window_xbatched(A, A, [1, 1, 1], w, Z, itype=itype)
    for itype in (1, 2, 3):
        with pytest.raises(ValueError):
            solver.check_sygv_window_xbatched(A, None, [1, 1, 1], w, Z, itype=itype)
        with pytest.raises(ValueError):
            solver.check_sygv_window_xbatched(A, A, [1, 1], w, Z, itype=itype)
        with pytest.raises(ValueError):
            solver.check_sygv_window_xbatched(A, A, [1, 1, 1], w, np.zeros((3, 4, 2)), itype=itype)
        with pytest.raises(ValueError):
            solver.check_sygv_window_xbatched(A, A, [1, 1, 1], w, Z, itype=itype, zcap=3)
        with pytest.raises(solver.SolverError) as e:
            solver.check_sygv_window_xbatched(A, A, [1, 3, 1], w, Z, itype=itype)
        assert e.value.info == -14
        out, ipr = solver.check_sygv_window_xbatched(A, A, [0, 7, 0], w, Z, itype=itype, info=[0, -20, 0])
        assert out.shape == (3, 4) and ipr.shape == (3, 5) and np.all(np.isnan(out)) and np.all(np.isnan(ipr))
        out, ipr = solver.check_sygv_window_xbatched(np.zeros((2, 0, 0)), np.zeros((2, 0, 0)), [0, 0], np.zeros((2, 0)),
                                                     np.zeros((2, 0, 0)), itype=itype, ipr=False)
        assert out.shape == (2, 4) and ipr is None


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", (129, 192, 256))
def test_the_mirror_against_long_double(n, itype):
    """The yardstick of the GPU tests, verifier.*_sygv on Z[:, :c], w[:c], against a long-double evaluation on the table's
    inputs, clean and planted: within MIRROR_BOUND of the bound of the GPU tests (twice the share measured here)."""
    worst = np.zeros(5)
    case = cs.cases(n, itype)
    assert case.cond.max() <= 16.0
    for c in (n // 8, 65):
        for plant in (False, True):
            for b in range(cs.COUNT):
                w, Z = cs.window(n, itype, b, c, plant)
                ref_out, ref_ipr = cs.mirrored(n, itype, b, c, plant)
                lo, li = cs.longdouble(itype, case.A[b], case.B[b], w, Z)
                worst = np.maximum(worst, cs.shares(itype, ref_out, ref_ipr, lo, li, n, case.cond[b]))
    print("n=%d itype=%d: the mirror's share of its bounds against long double: " % (n, itype)
          + ", ".join("%s %.4f" % kv for kv in zip(cs.NAMES, worst)))
    assert np.all(worst < MIRROR_BOUND), worst


def test_the_table():
    assert cs.columns(256) == (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)
    for itype in (2, 3):
        case = cs.cases(129, itype)
        for b in range(cs.COUNT):
            w, Z = cs.window(129, itype, b, 16, True)
            assert Z.shape == (129, 16) and w.shape == (16,)
            ref = cs.mirrored(129, itype, b, 16, True)
            clean = cs.mirrored(129, itype, b, 16, False)
            # the pairs are the type's: A B z = w z (2), B A z = w z (3)
            M = case.A[b] @ case.B[b] if itype == 2 else case.B[b] @ case.A[b]
            wc, Zc = cs.window(129, itype, b, 16, False)
            assert np.abs(M @ Zc - Zc * wc).max() < 1e-10 * np.abs(M).max()
            # the plants show in every slot: far above the rounding noise of the clean window
            assert ref[0][1] > 1e3 * clean[0][1] and ref[0][2] > 1e-8 and ref[0][3] > 1e-4
            assert clean[0][2] < 1e-13 and clean[0][3] < 1e-13
