"""Host-side checks of the window check (ek_hip_check_window_xbatched*): declared in the boundary header,
exported, bound by the Python mirror argument for argument, every argument error decided in the order of the prototype
before any device work and without dereferencing a data pointer, the device-free paths (n = 0, batch = 0, a batch of only
skipped and empty problems), and the host mirror on the window's columns against a long-double evaluation.  No GPU needed:
the data pointers are NULL, host addresses of small buffers or garbage.

Measured on the CPU (test_the_mirror_against_long_double, n = 129, 192, 256, c = n / 8 and 65, clean and planted): the
mirror's largest share of the tolerance 4 max(n, 8) eps is 0.020 (a_norm 0.0009, res_ave and res_max below 0.0001,
orthogonality 0.0037, ipr 0.0199, the last at n = 129); the bound is 1 / 4.  The full-width figure of
tests/test_gpu_check_xbatched.py is 0.022."""
import ctypes
import os
import re

import numpy as np
import pytest

import check_window_cases as cw
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ek_hip_check_window_xbatched_device", "ek_hip_check_window_xbatched")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced
N = 200
SENTINEL = 777.0


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
        # problem, n, batch | A, lda, strideA | B, ldb, strideB | m | w | Z, ldz, zcap, strideZ | info, out, ipr, seconds
        data = ctypes.c_void_p if name.endswith("_device") else _dp
        assert at == [ctypes.c_int] * 3 + [data, ctypes.c_int, ctypes.c_longlong] * 2 + [_ip, data, data, ctypes.c_int,
                                                                                        ctypes.c_int, ctypes.c_longlong,
                                                                                        _ip, _dp, _dp, _dp]
        # the solver's own m, w, Z, ldz, zcap, strideZ, info sit in the same order in its prototype
        twin = list(getattr(lib, name.replace("check_window", "eigenpairs_window")).argtypes)
        assert twin[15:22] == at[9:16]
    proto = re.search(r"int ek_hip_check_window_xbatched_device\(([^;]*)\);", hdr).group(1)
    args = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert args == ["problem", "n", "batch", "dA", "lda", "strideA", "dB", "ldb", "strideB", "m", "dw", "dZ", "ldz", "zcap",
                    "strideZ", "info", "out", "ipr", "seconds"]
    assert callable(solver.check_window_xbatched)
    assert lib.ek_hip_version() == 3


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

    def __call__(self, problem=1, n=N, batch=3, A="ok", lda=N, sA=N * N, B="ok", ldb=N, sB=N * N, m=(5, 0, N), w="ok",
                 Z="ok", ldz=N, zcap=N, sZ=N * N, info=(0, 0, 0), out="ok", ipr="ok", seconds=None):
        return self.fn(problem, n, batch, self.ptr(A), lda, sA, self.ptr(B), ldb, sB, self.ints(m), self.ptr(w),
                       self.ptr(Z), ldz, zcap, sZ, self.ints(info),
                       self.out.ctypes.data_as(_dp) if out is not None else None,
                       self.ipr.ctypes.data_as(_dp) if ipr is not None else None, seconds)


@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_in_prototype_order(name, data):
    call = _Call(name, data)
    assert call(problem=2) == -1
    assert call(problem=-1) == -1
    assert call(n=-1) == -2
    assert call(n=solver.XBATCH_NMAX + 1, lda=300, ldb=300, ldz=300, sA=10 ** 6, sB=10 ** 6, sZ=10 ** 6) == -2
    assert call(batch=-1) == -3
    assert call(A=None) == -4
    assert call(lda=N - 1) == -5
    assert call(sA=N * N - 1) == -6
    assert call(sA=0) == -6
    assert call(B=None) == -7
    assert call(ldb=N - 1) == -8
    assert call(sB=N * N - 1) == -9
    assert call(m=None) == -10
    assert call(m=(5, -1, N)) == -10
    assert call(m=(5, 0, N + 1)) == -10
    assert call(w=None) == -11
    assert call(Z=None) == -12
    assert call(ldz=N - 1) == -13
    assert call(zcap=-1) == -14
    assert call(zcap=N - 1) == -14                  # m[2] = N
    assert call(m=(5, 0, 6), zcap=5, sZ=5 * N) == -14
    assert call(sZ=N * N - 1) == -15
    assert call(m=(0, 0, 0), zcap=0, sZ=N - 1) == -15                 # ldz max(1, zcap)
    assert call(out=None) == -17
    # problem 0 does not look at B, ldb, strideB
    assert call(problem=0, B=None, ldb=0, sB=0, out=None) == -17
    # nothing was written on the way to an error
    assert np.all(call.out == SENTINEL) and np.all(call.ipr == SENTINEL)


@pytest.mark.parametrize("name", NAMES)
def test_the_first_offender_decides(name):
    call = _Call(name, "garbage")
    assert call(problem=3, n=-1) == -1
    assert call(n=-1, batch=-1) == -2
    assert call(batch=-1, A=None) == -3
    assert call(A=None, lda=0) == -4
    assert call(lda=0, sA=0) == -5
    assert call(sA=0, B=None) == -6
    assert call(B=None, m=None) == -7
    assert call(sB=0, m=(N + 1, 0, 0)) == -9
    assert call(m=(N + 1, 0, 0), w=None) == -10
    assert call(m=(5, 0, N), zcap=3, w=None) == -11  # m against zcap is argument 14: w comes first
    assert call(w=None, Z=None) == -11
    assert call(Z=None, ldz=0) == -12
    assert call(ldz=0, zcap=-1) == -13
    assert call(zcap=4, sZ=0) == -14                # m[0] = 5 > zcap before the stride
    assert call(sZ=0, out=None) == -15
    assert call(out=None, ipr=None) == -17


@pytest.mark.parametrize("name", NAMES)
def test_m_beyond_zcap_or_n_is_ignored_under_info_and_refused_without(name):
    call = _Call(name, "garbage")
    # every problem skipped or empty: legal, and answered without a device (see below)
    assert call(m=(N + 7, 0, -3), info=(-20, 0, 5), zcap=4, sZ=4 * N) == 0
    assert call(m=(9, 0, 0), info=(-20, 0, 0), zcap=4, sZ=4 * N) == 0
    # the same counts without the info that excuses them
    assert call(m=(N + 7, 0, 0), info=(0, 0, 0), zcap=4, sZ=4 * N) == -10
    assert call(m=(N + 7, 0, 0), info=None, zcap=4, sZ=4 * N) == -10
    assert call(m=(9, 0, 0), info=(0, 0, 0), zcap=4, sZ=4 * N) == -14
    assert call(m=(9, 0, 0), info=None, zcap=4, sZ=4 * N) == -14
    assert call(m=(0, 0, -3), info=(0, 0, 0)) == -10


@pytest.mark.parametrize("name", NAMES)
def test_nothing_to_do_references_nothing(name):
    """n = 0 and batch = 0: 0, nothing referenced or written, `out` and `seconds` aside (seconds = 0)."""
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    assert call(n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0, zcap=0, seconds=ctypes.byref(sec)) == 0
    assert sec.value == 0.0
    assert call(batch=0, m=None, info=None, A=None, B=None, w=None, Z=None, out=None, ipr=None) == 0
    assert call(n=0, m=None, A=None, B=None, w=None, Z=None, out=None, ipr=None) == 0
    assert np.all(call.out == SENTINEL) and np.all(call.ipr == SENTINEL)


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_of_skipped_and_empty_problems_is_filled_without_a_device(name):
    """Garbage data pointers, and no ek_hip_init: four NaN per problem, the ipr rows and what lies behind `out` left."""
    call = _Call(name, "garbage")
    sec = ctypes.c_double(-1.0)
    assert call(m=(0, 44, 0), info=(0, 3, 0), seconds=ctypes.byref(sec)) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL and np.all(call.ipr == SENTINEL)
    assert sec.value == 0.0
    call.out[:] = SENTINEL
    assert call(m=(0, 0, 0), info=None, zcap=0, sZ=N, ipr=None) == 0
    assert np.all(np.isnan(call.out[:12])) and call.out[12] == SENTINEL


def test_the_existing_check_entries_refuse_what_they_refused():
    lib = solver.load_library()
    g = ctypes.c_void_p(GARBAGE)
    gd = ctypes.cast(GARBAGE, _dp)
    out = np.full(4, SENTINEL)
    op = out.ctypes.data_as(_dp)
    big = solver.BATCH_NMAX + 1
    for entry, first in (("ek_hip_check_batched", 1), ("ek_hip_check_sygv_batched", 2)):
        for suffix, p in (("_device", g), ("", gd)):
            fn = getattr(lib, entry + suffix)
            assert fn(first, big, 1, p, big, big * big, p, big, big * big, p, p, big, big * big, None, op, None, None) == -2
            assert fn(first, 8, 1, p, 8, 64, p, 8, 64, p, p, 8, 63, None, op, None, None) == -13
            assert fn(first, 8, 1, p, 8, 64, p, 8, 64, p, p, 8, 64, None, None, None, None) == -15
    for entry, first in (("ek_hip_check_xbatched", 1), ("ek_hip_check_sygv_xbatched", 3)):
        for suffix, p in (("_device", g), ("", gd)):
            fn = getattr(lib, entry + suffix)
            nb = solver.XBATCH_NMAX + 1
            assert fn(first, nb, 1, p, nb, nb * nb, p, nb, nb * nb, p, p, nb, nb * nb, None, op, None, None) == -2
            assert fn(first, N, 1, p, N, N * N, p, N, N * N, None, p, N, N * N, None, op, None, None) == -10
            assert fn(first, N, 1, p, N, N * N, p, N, N * N, p, p, N, N * N, None, None, None, None) == -15
    assert np.all(out == SENTINEL)


def test_python_wrapper_shapes_and_device_free_paths():
    A = np.zeros((3, 5, 5))
    Z = np.zeros((3, 5, 2))
    w = np.zeros((3, 5))
    with pytest.raises(ValueError):
        solver.check_window_xbatched(A, None, [1, 1], w, Z)
    with pytest.raises(ValueError):
        solver.check_window_xbatched(A, None, [1, 1, 1], w, np.zeros((3, 4, 2)))
    with pytest.raises(ValueError):
        solver.check_window_xbatched(A, None, [1, 1, 1], w, Z, zcap=3)
    with pytest.raises(solver.SolverError) as e:
        solver.check_window_xbatched(A, None, [1, 3, 1], w, Z)
    assert e.value.info == -14
    out, ipr = solver.check_window_xbatched(A, None, [0, 7, 0], w, Z, info=[0, -20, 0])
    assert out.shape == (3, 4) and ipr.shape == (3, 5) and np.all(np.isnan(out)) and np.all(np.isnan(ipr))
    out, ipr = solver.check_window_xbatched(np.zeros((2, 0, 0)), None, [0, 0], np.zeros((2, 0)), np.zeros((2, 0, 0)),
                                            ipr=False)
    assert out.shape == (2, 4) and ipr is None


@pytest.mark.parametrize("n", (129, 192, 256))
def test_the_mirror_against_long_double(n):
    """The yardstick of the GPU tests, verifier.eval_residual_norm / eval_orthogonality / get_ipratios on Z[:, :c], w[:c],
    within a quarter of the tolerance of a long-double evaluation on the table's inputs, clean and planted."""
    worst = np.zeros(5)
    for problem in (0, 1):
        case = cw.cases(n, problem)
        for c in (n // 8, 65):
            for plant in (False, True):
                ws, Zs = cw.windows(n, problem, c, plant)
                ref = cw.mirrors(n, problem, c, plant)
                for b in range(cw.COUNT):
                    lo, li = cw.longdouble(case.A[b], case.B[b] if problem else None, ws[b], Zs[b])
                    worst = np.maximum(worst, cw.shares(ref[b][0], ref[b][1], lo, li, n))
    print("n=%d: the mirror's share of 4 max(n, 8) eps against long double: " % n
          + ", ".join("%s %.4f" % kv for kv in zip(cw.NAMES, worst)))
    assert np.all(worst < 0.25), worst


def test_the_table():
    assert cw.columns(1) == (1,) and cw.columns(2) == (1, 2)
    assert cw.columns(256) == (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)
    assert cw.columns(129) == (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129)
    assert cw.columns(64) == (1, 8, 15, 16, 17, 31, 32, 33, 63, 64)
    ws, Zs = cw.windows(129, 1, 16, True)
    ref = cw.mirrors(129, 1, 16, True)
    clean = cw.mirrors(129, 1, 16, False)
    for b in range(cw.COUNT):
        assert Zs[b].shape == (129, 16) and ws[b].shape == (16,)
        # the plants show in every slot: far above the rounding noise of the clean window
        assert ref[b][0][1] > 1e3 * clean[b][0][1] and ref[b][0][2] > 1e-6 and ref[b][0][3] > 1e-4
        assert clean[b][0][2] < 1e-13 and clean[b][0][3] < 1e-13
