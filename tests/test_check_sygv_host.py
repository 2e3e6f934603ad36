"""Host-side checks of the acceptance checks for DSYGV's types 2 and 3 (ek_hip_check_sygv_batched*,
ek_hip_check_sygv_vbatched*, ek_hip_check_sygvx*): declared, exported and bound; every argument error decided before any
device work and without dereferencing a data pointer (no GPU needed: the device forms get host addresses or garbage);
the NumPy mirrors of eigenkernel_amd/verifier.py pinned on a 3 x 3 pencil worked out by hand, and on the shipped BNZ30
pair through scipy.linalg.eigh(type = 2 / 3)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import solver, verifier
from eigenkernel_amd.matrix_io import read_matrix_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIFORM = ("ek_hip_check_sygv_batched_device", "ek_hip_check_sygv_batched")
VARIABLE = ("ek_hip_check_sygv_vbatched_device", "ek_hip_check_sygv_vbatched")
SINGLE = ("ek_hip_check_sygvx_device", "ek_hip_check_sygvx")
EPS = 2.220446049250313e-16
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
GARBAGE = 0x10                                      # a data "pointer" that faults if it is ever dereferenced
itypes = pytest.mark.parametrize("itype", (1, 2, 3))


def test_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for name in UNIFORM + VARIABLE + SINGLE:
        assert name in declared and name not in hooks
        assert name in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        assert getattr(lib, name).restype is ctypes.c_int
    # argument k is argument k of the ek_hip_check_*batched* entry
    for name in UNIFORM:
        assert getattr(lib, name).argtypes == getattr(lib, name.replace("_sygv", "")).argtypes
        assert len(getattr(lib, name).argtypes) == 17
    for name in VARIABLE:
        assert getattr(lib, name).argtypes == getattr(lib, name.replace("_sygv", "")).argtypes
        assert len(getattr(lib, name).argtypes) == 14
    for name in SINGLE:
        at = getattr(lib, name).argtypes
        assert len(at) == 12 and at[10] is _dp and at[11] is _dp                    # out, ipr_host: host arrays
    for f in ("check_sygv_batched", "check_sygv_vbatched", "check_sygvx"):
        assert callable(getattr(solver, f))
    for f in ("eval_residual_norm_sygv", "eval_orthogonality_sygv", "get_ipratios_sygv"):
        assert callable(getattr(verifier, f))
    assert "remain checks of type 1" in hdr and "ek_hip_check_sygv_batched*" in hdr
    assert lib.ek_hip_version() == 3


@itypes
@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_argument_errors_without_gpu(name, data, itype):
    """-1 for an itype outside 1 .. 3, then the codes of ek_hip_check_batched* with problem = 1, the first offender
    deciding; no data pointer is dereferenced."""
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

    def call(itype=itype, n=n, batch=batch, A=p, lda=n, sA=n * n, B=p, ldb=n, sB=n * n, w=p, Z=p, ldz=n, sZ=n * n,
             info=ip, out=op, ipr=qp):
        return fn(itype, n, batch, A, lda, sA, B, ldb, sB, w, Z, ldz, sZ, info, out, ipr, None)

    big = dict(lda=129, ldb=129, ldz=129, sA=129 * 129, sB=129 * 129, sZ=129 * 129)
    assert call(itype=0) == -1
    assert call(itype=4) == -1
    assert call(itype=-1) == -1
    assert call(n=-1) == -2
    assert call(n=129, **big) == -2
    assert call(batch=-1) == -3
    assert call(A=None) == -4
    assert call(lda=n - 1) == -5
    assert call(sA=n * n - 1) == -6
    assert call(sA=0) == -6
    assert call(lda=n + 2, sA=n * n) == -6
    assert call(B=None) == -7                       # B is always required
    assert call(ldb=n - 1) == -8
    assert call(sB=0) == -9
    assert call(w=None) == -10
    assert call(Z=None) == -11
    assert call(ldz=n - 1) == -12
    assert call(sZ=n * n - 1) == -13
    assert call(out=None) == -15
    # the first offending argument decides
    assert call(itype=0, n=-1, batch=-1) == -1
    assert call(itype=4, A=None, out=None) == -1
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
    # info = NULL and ipr = NULL are legal: the next offender decides
    assert call(info=None, ipr=None, out=None) == -15
    assert call(info=None, ipr=None, Z=None) == -11
    # nothing to do: success with every pointer NULL, nothing written; an illegal itype is refused even then
    for kw in (dict(batch=0), dict(n=0, lda=0, ldb=0, ldz=0, sA=0, sB=0, sZ=0)):
        sec = ctypes.c_double(-1.0)
        args = dict(n=n, batch=batch, lda=n, sA=n * n, ldb=n, sB=n * n, ldz=n, sZ=n * n)
        args.update(kw)
        tail = (None, args["lda"], args["sA"], None, args["ldb"], args["sB"], None, None, args["ldz"], args["sZ"], None,
                None, None, ctypes.byref(sec))
        assert fn(itype, args["n"], args["batch"], *tail) == 0 and sec.value == 0.0
        assert fn(0, args["n"], args["batch"], *tail) == -1
    assert np.all(buf == 3.5) and np.all(out == 777.0) and np.all(ipr == 777.0)


@itypes
@pytest.mark.parametrize("data", ["host", "garbage"])
@pytest.mark.parametrize("name", VARIABLE)
def test_variable_argument_errors_without_gpu(name, data, itype):
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

    def call(itype=itype, batch=batch, n=orders, A="ok", lda=ld_ok, B="ok", ldb=ld_ok, w="ok", Z="ok", ldz=ld_ok,
             info=info, out=out, ipr="ok"):
        def P(x):
            return ptrs() if isinstance(x, str) else x

        def I(x, t=_ip):
            if x is None:
                return None
            keep.append(x)
            return x.ctypes.data_as(t)
        return fn(itype, batch, I(n), P(A), I(lda), P(B), I(ldb), P(w), P(Z), I(ldz), I(info), I(out, _dp), P(ipr),
                  None)

    assert call(itype=0) == -1
    assert call(itype=4) == -1
    assert call(batch=-1) == -2
    assert call(n=None) == -3
    assert call(n=ints([4, -1, 3])) == -3
    assert call(n=ints([4, 0, 129]), lda=ints([4, 1, 129]), ldb=ints([4, 1, 129]), ldz=ints([4, 1, 129])) == -3
    assert call(A=None) == -4
    assert call(A=ptrs(null_at=2)) == -4
    assert call(lda=None) == -5
    assert call(lda=ints([3, 1, 3])) == -5
    assert call(lda=ints([4, 0, 3])) == -5
    assert call(B=None) == -6                       # B is always required
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
    assert call(itype=0, batch=-1, n=None) == -1
    assert call(batch=-1, n=None, A=None) == -2
    assert call(n=ints([4, 0, 200]), A=None) == -3
    assert call(A=ptrs(null_at=0), lda=ints([1, 1, 1]), out=None) == -4
    assert call(lda=ints([1, 1, 1]), B=None, out=None) == -5
    assert call(B=None, ldb=None, w=None) == -6
    assert call(ldb=None, w=None, Z=None) == -7
    assert call(w=None, Z=None, out=None) == -8
    assert call(Z=None, ldz=None, out=None) == -9
    assert call(ldz=None, out=None) == -10
    assert call(info=None, ipr=None, out=None) == -12
    assert call(info=None, ipr=None, ldz=None) == -10
    # nothing to do: success without a device and without touching any pointer
    nothing = dict(batch=0, n=None, A=None, lda=None, B=None, ldb=None, w=None, Z=None, ldz=None, info=None, out=None,
                   ipr=None)
    assert call(**nothing) == 0
    assert call(itype=4, **nothing) == -1
    assert np.all(out == 777.0)
    for b in bufs:
        assert np.all(b == 3.5)


@itypes
@pytest.mark.parametrize("name", VARIABLE)
def test_variable_all_orders_zero_or_skipped_needs_no_device(name, itype):
    """Every problem empty or skipped: the slots are filled on the host and no data pointer is looked at."""
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
    rc = fn(itype, 3, n.ctypes.data_as(_ip), data, ld.ctypes.data_as(_ip), data, ld.ctypes.data_as(_ip), data, data,
            ld.ctypes.data_as(_ip), info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), iprs, ctypes.byref(sec))
    assert rc == 0 and sec.value == 0.0
    assert out[0] == 0.0 and np.all(np.isnan(out[1:]))
    assert np.all(q == 777.0)


@itypes
@pytest.mark.parametrize("data", ["null_or_host", "garbage"])
@pytest.mark.parametrize("name", SINGLE)
def test_one_problem_argument_errors_without_gpu(name, data, itype):
    lib = solver.load_library()
    fn = getattr(lib, name)
    n = 4
    buf = np.full(n * n, 3.5)
    out = np.full(4, 777.0)
    ipr = np.full(n, 777.0)
    if data == "garbage":
        p = ctypes.c_void_p(GARBAGE) if name.endswith("_device") else ctypes.cast(GARBAGE, _dp)
    else:
        p = ctypes.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(_dp)
    op, qp = out.ctypes.data_as(_dp), ipr.ctypes.data_as(_dp)

    def call(itype=itype, n=n, n_cols=2, A=p, lda=n, B=p, ldb=n, w=p, Z=p, ldz=n, out=op, ipr=qp):
        return fn(itype, n, n_cols, A, lda, B, ldb, w, Z, ldz, out, ipr)

    assert call(itype=0) == -1
    assert call(itype=4) == -1
    assert call(n=-1) == -2
    assert call(n_cols=-1) == -3
    assert call(n_cols=n + 1) == -3
    assert call(A=None) == -4
    assert call(lda=n - 1) == -5
    assert call(B=None) == -6
    assert call(ldb=n - 1) == -7
    assert call(w=None) == -8
    assert call(Z=None) == -9
    assert call(ldz=n - 1) == -10
    assert call(out=None) == -11
    # the first offending argument decides
    assert call(itype=5, n=-1, n_cols=-1) == -1
    assert call(n=-1, n_cols=-1, A=None) == -2
    assert call(n_cols=9, A=None, lda=0) == -3
    assert call(A=None, lda=0, B=None) == -4
    assert call(lda=0, B=None, ldb=0) == -5
    assert call(B=None, ldb=0, w=None) == -6
    assert call(ldb=0, w=None, Z=None) == -7
    assert call(w=None, Z=None, ldz=0) == -8
    assert call(Z=None, ldz=0, out=None) == -9
    assert call(ldz=0, out=None) == -10
    assert call(ipr=None, out=None) == -11          # ipr_host = NULL is legal
    # nothing to do: success without a device, nothing referenced or written
    assert call(n_cols=0, w=None, Z=None) == 0
    assert fn(itype, 0, 0, None, 1, None, 1, None, None, 1, op, None) == 0
    assert np.all(buf == 3.5) and np.all(out == 777.0) and np.all(ipr == 777.0)


def test_python_wrappers_reject_bad_input_before_the_library():
    z3 = np.zeros((2, 3, 3))
    m3 = np.zeros((3, 3))
    for itype in (0, 4):
        with pytest.raises(ValueError):
            solver.check_sygv_batched(z3, z3, np.zeros((2, 3)), z3, itype=itype)
        with pytest.raises(ValueError):
            solver.check_sygv_vbatched([m3], [m3], [np.zeros(3)], [m3], itype=itype)
        with pytest.raises(ValueError):
            solver.check_sygvx(m3, m3, np.zeros(3), m3, itype=itype)
        for f in (verifier.eval_orthogonality_sygv, verifier.get_ipratios_sygv):
            with pytest.raises(ValueError):
                f(itype, np.eye(3), np.eye(3))
        with pytest.raises(ValueError):
            verifier.eval_residual_norm_sygv(itype, m3, np.eye(3), np.zeros(3), np.eye(3))
    with pytest.raises(ValueError):
        solver.check_sygv_batched(z3, None, np.zeros((2, 3)), z3, itype=2)
    with pytest.raises(ValueError):
        solver.check_sygv_vbatched([m3], None, [np.zeros(3)], [m3], itype=3)
    with pytest.raises(ValueError):
        solver.check_sygv_batched(z3, np.zeros((2, 4, 4)), np.zeros((2, 3)), z3, itype=2)
    with pytest.raises(ValueError):
        solver.check_sygvx(m3, m3, np.zeros(2), m3, itype=2)
    with pytest.raises(ValueError):
        solver.check_sygvx(m3, np.zeros((4, 4)), np.zeros(3), m3, itype=2)
    # decided without a device: nothing to check, orders of 0, skipped problems, an order beyond the batched limit
    out, q = solver.check_sygv_vbatched([], [], [], [], itype=2)
    assert out.shape == (0, 4) and q == []
    out, q = solver.check_sygv_batched(np.zeros((2, 0, 0)), np.zeros((2, 0, 0)), np.zeros((2, 0)), np.zeros((2, 0, 0)),
                                       itype=3, info=[0, 1])
    assert out[0, 0] == 0.0 and np.all(np.isnan(out[0, 1:])) and np.all(np.isnan(out[1])) and q.shape == (2, 0)
    big = np.zeros((129, 129))
    with pytest.raises(solver.SolverError) as ei:
        solver.check_sygv_vbatched([big], [big], [np.zeros(129)], [big], itype=2)
    assert ei.value.info == -3
    with pytest.raises(solver.SolverError) as ei:
        solver.check_sygv_batched(big[None], big[None], np.zeros((1, 129)), big[None], itype=3)
    assert ei.value.info == -2


# ------------------------------------------------------------------------------------------- the mirrors, by hand
# A = [[2, 1, 0], [1, 3, 0], [0, 0, 1]], B = diag(1, 4, 9) = L L^T with L = diag(1, 2, 3); ||A||_F = 4, ||B||_F = 7 sqrt 2.
# V = [v1 v2] with v1 = (1, 1, 0), v2 = (0, 1, 1) (both of norm sqrt 2) and the "eigenvalues" (3, 12):
#   type 2   A B v1 = (6, 13, 0), r1 = (3, 10, 0), ||r1|| = sqrt 109;  A B v2 = (4, 12, 9), r2 = (4, 0, -3), ||r2|| = 5
#            G = V^T B V = [[5, 4], [4, 13]]
#   type 3   B A v1 = (3, 16, 0), r1 = (0, 13, 0), ||r1|| = 13;  B A v2 = (1, 12, 9), r2 = (1, 0, -3), ||r2|| = sqrt 10
#            G = V^T B^-1 V = [[5/4, 1/4], [1/4, 13/36]]
#   rho_j = ||r_j|| / (28 sqrt 2 * sqrt 2) = ||r_j|| / 56;  sum_i v_ij^4 = 2 for both columns
#   type 1   r_j = A v_j - w_j B v_j: r1 = (3, 4, 0) - (3, 12, 0) = (0, -8, 0), r2 = (1, 3, 1) - (0, 48, 108) = (1, -45, -107)
_A = np.array([[2.0, 99.0, -99.0], [1.0, 3.0, 99.0], [0.0, 0.0, 1.0]])         # the strictly upper triangle is not looked at
_B = np.array([[1.0, 55.0, 55.0], [0.0, 4.0, -55.0], [0.0, 0.0, 9.0]])
_V = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
_W = np.array([3.0, 12.0])
_HAND = {
    2: (28 * np.sqrt(2.0), (np.sqrt(109.0) + 5.0) / 112.0, np.sqrt(109.0) / 56.0, 4.0 * np.sqrt(2.0 / 65.0),
        np.array([2.0 / 25.0, 2.0 / 169.0])),
    3: (28 * np.sqrt(2.0), (13.0 + np.sqrt(10.0)) / 112.0, 13.0 / 56.0, 3.0 * np.sqrt(2.0 / 65.0),
        np.array([32.0 / 25.0, 2592.0 / 169.0])),
    1: (4.0, (8.0 + np.sqrt(1.0 + 45.0 ** 2 + 107.0 ** 2)) / 8.0, np.sqrt(1.0 + 45.0 ** 2 + 107.0 ** 2) / 4.0,
        4.0 * np.sqrt(2.0 / 65.0), np.array([2.0 / 25.0, 2.0 / 169.0])),
}


@itypes
def test_mirrors_on_a_pencil_worked_out_by_hand(itype):
    norm, ave, mx, orth, ipr = _HAND[itype]
    got = verifier.eval_residual_norm_sygv(itype, _A, _B, _W, _V)
    tol = 8 * EPS
    assert abs(got[0] - norm) <= tol * norm
    assert abs(got[1] - ave) <= tol * ave and abs(got[2] - mx) <= tol * mx
    assert abs(verifier.eval_orthogonality_sygv(itype, _V, _B) - orth) <= tol
    assert np.all(np.abs(verifier.get_ipratios_sygv(itype, _V, _B) - ipr) <= tol * ipr)


def test_mirrors_type_1_forwards_and_type_3_reports_a_b_that_is_not_spd():
    sym = lambda M: np.tril(M) + np.tril(M, -1).T
    assert verifier.eval_residual_norm_sygv(1, _A, _B, _W, _V) == verifier.eval_residual_norm(sym(_A), _W, _V, sym(_B))
    assert verifier.eval_orthogonality_sygv(1, _V, _B) == verifier.eval_orthogonality(_V, sym(_B))
    assert np.array_equal(verifier.get_ipratios_sygv(1, _V, _B), verifier.get_ipratios(_V, sym(_B)))
    bad = np.diag([1.0, -4.0, 9.0])
    assert np.isnan(verifier.eval_orthogonality_sygv(3, _V, bad))
    assert np.all(np.isnan(verifier.get_ipratios_sygv(3, _V, bad)))
    assert np.all(np.isfinite(verifier.eval_residual_norm_sygv(3, _A, bad, _W, _V)))


@pytest.mark.parametrize("itype", (2, 3))
def test_mirrors_on_the_reference_pair_bnz30(golden_dir, itype):
    """SciPy's eigh(type = itype) on the shipped pair: a backward-stable solve leaves ||r_j|| <= c n eps ||A|| ||B|| ||z_j||
    with a modest c, so res_max is held to the 64 n eps the suite uses for type 1; the metric of type 2 is formed with B
    (256 n eps, as for type 1), the metric of type 3 with B^-1, whose rounding is amplified by cond_2(B)."""
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx")).to_dense()
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense()
    n = A.shape[0]
    w, Z = sl.eigh(A, B, type=itype, lower=True)
    norm, ave, mx = verifier.eval_residual_norm_sygv(itype, A, B, w, Z)
    orth = verifier.eval_orthogonality_sygv(itype, Z, B)
    ipr = verifier.get_ipratios_sygv(itype, Z, B)
    cond = np.linalg.cond(B) if itype == 3 else 1.0
    print("BNZ30 type %d: norm %.6e res_ave %.3e res_max %.3e orthogonality %.3e cond(B) %.3e"
          % (itype, norm, ave, mx, orth, np.linalg.cond(B)))
    assert abs(norm - np.linalg.norm(A, "fro") * np.linalg.norm(B, "fro")) <= 4 * EPS * norm
    assert 0.0 < ave <= mx <= 64 * n * EPS
    assert orth <= 256 * n * EPS * cond
    assert ipr.shape == (n,) and np.all(ipr > 0.0)
    # SciPy normalises Z^T B Z = I (type 2) and Z^T B^-1 Z = I (type 3): the IPR is then sum_i z_ij^4
    assert np.all(np.abs(ipr - (Z ** 4).sum(axis=0)) <= 256 * n * EPS * cond * ipr)
