"""Host-side checks of the variable-order window entries (ek_hip_eigenpairs_window_xvbatched*,
ek_hip_sygv_window_xvbatched*), no GPU needed: declared in the boundary header, exported and bound with 20 arguments; the
budget hook a debug entry; every argument error -1 .. -19 decided before any device work, in prototype order, with NULL,
host and garbage data pointers (none is dereferenced), orders 129, 200 and 256 legal and 257 not; a batch of empty
problems filled without a device; the uniform window entries and the xvbatched entries still accept and refuse what they
did; and the case table of tests/window_xvbatched_cases.py pinned against SciPy's windowed drivers: half of the eigenvalue
bound, a quarter of the residual and orthogonality bounds, every 'V' count that of the sliced full spectrum."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import window_xvbatched_cases as xc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG = ("ek_hip_eigenpairs_window_xvbatched_device", "ek_hip_eigenpairs_window_xvbatched")
SYGV = ("ek_hip_sygv_window_xvbatched_device", "ek_hip_sygv_window_xvbatched")
HOOK = "ek_hip_debug_window_xvbatched_budget"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


def _headers():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    return set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr)), set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))


def test_entries_declared_exported_and_bound():
    """Fails on a tree without the feature: the symbols are the signal."""
    declared, hooks = _headers()
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    vp = ctypes.c_void_p
    want = [ctypes.c_int] * 4 + [_ip, _dp, _dp, _ip, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip, _ip, _dp]
    for name in EIG + SYGV:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 20
        assert list(fn.argtypes) == want
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    for name in EIG + SYGV:                             # the prototype, argument for argument
        proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        args = [re.sub(r"\s+", " ", a).strip() for a in proto.split(",")]
        assert len(args) == 20
        assert [a.split()[-1].lstrip("*") for a in args] == [
            "itype" if "sygv" in name else "problem", "jobz", "range", "batch", "n", "vl", "vu", "il", "iu",
            "dA" if name.endswith("_device") else "A", "lda", "dB" if name.endswith("_device") else "B", "ldb", "m",
            "dw" if name.endswith("_device") else "w", "dZ" if name.endswith("_device") else "Z", "ldz", "zcap", "info",
            "seconds"]
    assert callable(solver.eigenpairs_window_xvbatched) and callable(solver.sygv_window_xvbatched)
    assert HOOK in hooks and HOOK not in declared and HOOK in solver.EXPORTED_SYMBOLS and hasattr(raw, HOOK)
    assert solver.window_xvbatched_budget(12345) == 0
    assert solver.window_xvbatched_budget(0) == 12345
    assert solver.window_xvbatched_budget(-5) == 0 and solver.window_xvbatched_budget(0) == 0


@pytest.mark.parametrize("pointers", ["host", "garbage"])
@pytest.mark.parametrize("name", EIG + SYGV)
def test_argument_errors_without_gpu(name, pointers):
    """-k for argument k of the prototype, before any device work.  The data pointers inside the pointer arrays are compared
    with NULL and never followed: host addresses to the device form, an address that belongs to nobody, and (for Z where
    zcap = 0) NULL itself."""
    fn = getattr(solver.load_library(), name)
    sygv = "sygv" in name
    batch = 4
    orders = [129, 200, 0, 256]
    buf = np.zeros(8)
    addr = buf.ctypes.data if pointers == "host" else 0x10
    hole = (ctypes.c_void_p * batch)(addr, None, None, addr)      # NULL at a problem of order > 0
    free = (ctypes.c_void_p * batch)(addr, addr, None, addr)      # NULL at the empty problem alone: legal
    info = np.full(batch, 7, dtype=np.int32)
    mm = np.full(batch, 7, dtype=np.int32)
    nan, inf = float("nan"), float("inf")
    keep = []

    def ints(x):
        a = np.array(x, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data_as(_ip)

    def dbls(x):
        a = np.array(x, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(_dp)

    def call(first=1, jobz=1, rng=0, batch=batch, n=orders, vl=(0.0,) * 4, vu=(1.0,) * 4, il=(1, 2, 0, 256),
             iu=(2, 2, 0, 256), A=free, lda="n", B=free, ldb="n", m=mm.ctypes.data_as(_ip), w=free, Z=free, ldz="n",
             zcap=(2, 1, 0, 3), info=info.ctypes.data_as(_ip)):
        ld = [max(k, 1) for k in (n if n is not None else orders)]
        lda, ldb, ldz = (ld if x == "n" else x for x in (lda, ldb, ldz))
        P = lambda x, f: None if x is None else f(x)    # noqa: E731
        return fn(first, jobz, rng, batch, P(n, ints), P(vl, dbls), P(vu, dbls), P(il, ints), P(iu, ints), A,
                  P(lda, ints), B, P(ldb, ints), m, w, Z, P(ldz, ints), P(zcap, ints), info, None)

    bad_first = (0, 4) if sygv else (2, -1)
    assert all(call(first=x) == -1 for x in bad_first)
    assert call(jobz=2) == -2 and call(jobz=-1) == -2
    assert call(rng=2) == -3 and call(rng=-1) == -3
    assert call(batch=-1) == -4
    assert call(n=None) == -5 and call(n=[129, 257, 0, 1]) == -5 and call(n=[-1, 1, 1, 1]) == -5
    for legal in (129, 200, 256):                       # the order is accepted: the next argument decides
        assert call(n=[legal] * 4, il=(1,) * 4, iu=(1,) * 4, A=None) == -10
    assert call(rng=1, vl=None) == -6 and call(rng=1, vl=(0.0, nan, 0.0, 0.0)) == -6
    assert call(rng=1, vu=None) == -7 and call(rng=1, vu=(1.0, 1.0, 1.0, nan)) == -7
    assert call(rng=1, vu=(1.0, 0.0, 1.0, 1.0)) == -7 and call(rng=1, vl=(inf,) * 4, vu=(inf,) * 4) == -7
    assert call(rng=1, vl=(0.0, 0.0, nan, 0.0), vu=(1.0, 1.0, nan, 1.0), A=None) == -10   # the empty problem's are not looked at
    assert call(rng=1, il=None, iu=None, A=None) == -10
    assert call(il=None) == -8 and call(il=(0, 1, 0, 1)) == -8 and call(il=(1, 201, 0, 1), iu=(1, 201, 0, 1)) == -8
    assert call(iu=None) == -9 and call(il=(2, 1, 0, 1), iu=(1, 1, 0, 1)) == -9 and call(iu=(130, 2, 0, 256)) == -9
    assert call(vl=None, vu=None, A=None) == -10        # 'I': vl and vu are not looked at
    assert call(A=None) == -10 and call(A=hole) == -10
    assert call(lda=None) == -11 and call(lda=[129, 199, 1, 256]) == -11 and call(lda=[129, 200, 0, 256]) == -11
    if sygv:
        assert call(B=None) == -12 and call(B=hole) == -12 and call(ldb=[128, 200, 1, 256]) == -13
    else:
        assert call(B=None) == -12 and call(B=hole) == -12 and call(ldb=None) == -13
        assert call(first=0, B=None, ldb=None, m=None) == -14     # what is not referenced is not checked
    assert call(m=None) == -14
    assert call(w=None) == -15 and call(w=hole) == -15
    assert call(Z=None) == -16 and call(Z=hole) == -16
    assert call(rng=1, Z=hole, zcap=(2, 0, 0, 3), info=None) == -19      # no Z is needed where it has no column
    assert call(Z=hole, zcap=None) == -16
    assert call(ldz=None) == -17 and call(ldz=[129, 200, 1, 255]) == -17
    assert call(zcap=None) == -18 and call(zcap=(2, 1, 0, -1)) == -18 and call(zcap=(1, 1, 0, 3)) == -18
    assert call(jobz=0, Z=None, ldz=None, zcap=(1, 1, 0, 3)) == -18     # with and without vectors
    assert call(jobz=0, Z=None, ldz=None, info=None) == -19
    assert call(rng=1, zcap=(0, 0, 0, 0), info=None) == -19
    assert call(info=None) == -19
    # the first offending argument decides
    assert call(first=bad_first[0], jobz=2, rng=5) == -1
    assert call(rng=5, batch=-1) == -3
    assert call(batch=-1, n=None) == -4
    assert call(n=[257] * 4, il=None) == -5
    assert call(rng=1, vl=(nan,) * 4, vu=(nan,) * 4) == -6
    assert call(il=(0,) * 4, iu=(0,) * 4, A=None) == -8
    assert call(m=None, w=None) == -14
    assert call(Z=None, zcap=None) == -16
    # nothing to do: success without a device and without a look at anything
    assert call(batch=0, n=None, il=None, iu=None, A=None, lda=None, B=None, ldb=None, m=None, w=None, Z=None, ldz=None,
                zcap=None, info=None) == 0
    assert (info == 7).all() and (mm == 7).all() and not buf.any()


@pytest.mark.parametrize("name", EIG + SYGV)
def test_a_batch_of_empty_problems_is_filled_without_a_device(name):
    fn = getattr(solver.load_library(), name)
    batch = 3
    none = (ctypes.c_void_p * batch)(None, None, None)
    z = np.zeros(batch, dtype=np.int32)
    one = np.ones(batch, dtype=np.int32)
    info = np.full(batch, 7, dtype=np.int32)
    m = np.full(batch, 7, dtype=np.int32)
    sec = np.full(1, 9.0)
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731
    assert fn(1, 1, 0, batch, I(z), None, None, I(z), I(z), none, I(one), none, I(one), I(m), none, none, I(one), I(z),
              I(info), sec.ctypes.data_as(_dp)) == 0
    assert not info.any() and not m.any() and sec[0] == 0.0


def test_the_neighbouring_entries_accept_and_refuse_what_they_did():
    lib = solver.load_library()
    none2 = [None] * 2
    for name in ("ek_hip_eigenpairs_window_batched_device", "ek_hip_eigenpairs_window_batched",
                 "ek_hip_sygv_window_batched_device", "ek_hip_sygv_window_batched"):
        fn = getattr(lib, name)
        assert fn(1, 0, 0, 129, 1, 0.0, 0.0, 1, 1, None, 129, 129 * 129, None, 129, 129 * 129, *none2, None, 129, 1, 129,
                  None, None) == -4
        assert fn(1, 0, 0, 128, 1, 0.0, 0.0, 1, 1, None, 128, 128 * 128, None, 128, 128 * 128, *none2, None, 128, 1, 128,
                  None, None) == -10
    for name in ("ek_hip_eigenpairs_window_xbatched_device", "ek_hip_eigenpairs_window_xbatched",
                 "ek_hip_sygv_window_xbatched_device", "ek_hip_sygv_window_xbatched"):
        fn = getattr(lib, name)
        assert fn(1, 0, 0, 257, 1, 0.0, 0.0, 1, 1, None, 257, 257 * 257, None, 257, 257 * 257, *none2, None, 257, 1, 257,
                  None, None) == -4
        assert fn(1, 0, 0, 256, 1, 0.0, 0.0, 1, 1, None, 256, 256 * 256, None, 256, 256 * 256, *none2, None, 256, 1, 256,
                  None, None) == -10
        assert fn(1, 0, 2, 256, 1, 0.0, 0.0, 1, 1, None, 256, 256 * 256, None, 256, 256 * 256, *none2, None, 256, 1, 256,
                  None, None) == -3
    n257 = np.array([257], dtype=np.int32).ctypes.data_as(_ip)
    n256 = np.array([256], dtype=np.int32).ctypes.data_as(_ip)
    for name in ("ek_hip_eigenpairs_xvbatched_device", "ek_hip_eigenpairs_xvbatched", "ek_hip_sygv_xvbatched_device",
                 "ek_hip_sygv_xvbatched"):
        fn = getattr(lib, name)
        assert fn(1, 1, 1, n257, None, None, None, None, None, None, None, None, None) == -4
        assert fn(1, 1, 1, n256, None, None, None, None, None, None, None, None, None) == -5
        assert fn(1, 1, -1, n256, None, None, None, None, None, None, None, None, None) == -3


def test_python_mirror_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xvbatched([np.zeros((3, 4))])
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xvbatched([np.zeros((3, 3))], [np.zeros((2, 2))])
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xvbatched([np.zeros((3, 3))], il=1, vu=0.0)
    with pytest.raises(ValueError):
        solver.eigenpairs_window_xvbatched([np.zeros((3, 3))], il=[1, 2])
    with pytest.raises(ValueError):
        solver.sygv_window_xvbatched([np.zeros((3, 3))], None)
    w, Z, m, info = solver.eigenpairs_window_xvbatched([])
    assert w == [] and Z == [] and m.shape == (0,) and info.shape == (0,)
    w, Z, m, info = solver.eigenpairs_window_xvbatched([np.zeros((0, 0)), np.zeros((0, 0))], il=1, iu=0)
    assert [x.shape for x in w] == [(0,), (0,)] and [x.shape for x in Z] == [(0, 0), (0, 0)]
    assert not m.any() and not info.any()
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_xvbatched([np.zeros((257, 257))])
    assert ei.value.info == -5
    with pytest.raises(solver.SolverError) as ei:
        solver.eigenpairs_window_xvbatched([np.zeros((5, 5)), np.zeros((9, 9))], il=[1, 5], iu=[2, 4])
    assert ei.value.info == -9
    with pytest.raises(solver.SolverError) as ei:
        solver.sygv_window_xvbatched([np.zeros((5, 5))], [np.eye(5)], itype=4)
    assert ei.value.info == -1


def test_the_case_table_is_what_the_issue_asks_for():
    for shuffle in xc.SHUFFLES:
        cases = xc.mixed(shuffle)
        assert sorted(c.n for c in cases) == sorted(2 * list(xc.ORDERS))
        differ = sum((a.n, a.il, a.iu) != (b.n, b.il, b.iu) for a, b in zip(cases, cases[1:]))
        assert differ >= len(cases) - 2
        assert any(c.extra == 0 for c in cases) and any(c.extra > 0 for c in cases)
        assert all((c.name, c.il, c.iu) in xc.windows(c.n) for c in cases)
    assert [c.key for c in xc.mixed(0)] != [c.key for c in xc.mixed(1)]


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_scipy_windowed_drivers_stay_inside_part_of_the_bounds(kind):
    """SciPy's eigh with subset_by_index and subset_by_value on every case: half of the eigenvalue bound, a quarter of the
    residual and orthogonality bounds of the judge the GPU file uses, and every 'V' count that of the sliced spectrum."""
    fails = []
    for c in xc.problems():
        kw = dict(lower=True) if kind == 0 else dict(b=c.B, type=kind, lower=True)
        w, Z = sl.eigh(c.A, subset_by_index=[c.il - 1, c.iu - 1], **kw)
        s, f = xc.judge_kind(c, kind, c.il - 1, w, Z, "%s 'I'" % (c.key,), ev_part=0.5, vec_part=0.25)
        fails += f
        vl, vu, first, m = xc.bounds(c, kind)
        w_ref = xc.spectrum(c, kind)[0]
        assert m >= c.iu - c.il + 1 and first <= c.il - 1
        assert m == int(((w_ref > vl) & (w_ref <= vu)).sum())
        wv, Zv = sl.eigh(c.A, subset_by_value=[vl, vu], **kw)
        assert len(wv) == m, (c.key, kind, len(wv), m)
        s, f = xc.judge_kind(c, kind, first, wv, Zv, "%s 'V'" % (c.key,), ev_part=0.5, vec_part=0.25)
        fails += f
    assert not fails, "\n".join(fails[:40])
