"""CPU suite of the triplet entries (ek_hip_solve_sparse, ek_hip_check_sparse*, ek_hip_sparse_to_dense): the symbols are
declared, exported and bound; every argument check answers without a GPU (the checks run before the library touches a
device); the canonical form -- the CSR of the mirrored matrix, built on the host -- is held against an explicit loop
that does what the reference's serial pdelset loop does (distribute_matrix.f90:411-418); the workspace hook is held
against the formula include/ek_hip_debug.h states.  No torch in this process (see tests/test_host_logic.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from eigenkernel_amd import descriptor as dsc
from eigenkernel_amd import solver
from eigenkernel_amd.matrix_io import SparseMat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ek_hip_solve_sparse", "ek_hip_check_sparse_device", "ek_hip_check_sparse", "ek_hip_sparse_to_dense")
HOOKS = ("ek_hip_debug_sparse_check_workspace_bytes", "ek_hip_debug_sparse_csr")


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_sparse_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    assert set(NEW) <= set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    assert set(HOOKS) <= set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    assert set(NEW) | set(HOOKS) <= set(solver.EXPORTED_SYMBOLS)
    lib = solver.load_library()
    for name in NEW + HOOKS:
        assert getattr(lib, name).argtypes is not None, name
    for fn in ("solve_sparse", "check_sparse", "sparse_to_dense", "sparse_csr", "sparse_check_workspace_bytes"):
        assert callable(getattr(solver, fn)), fn
    assert lib.ek_hip_version() == 3


# ---------------------------------------------------------------------------------------- the canonical form
def loop_mirror(n, suffix, value):
    """distribute_matrix.f90:411-418 on one rank: every entry is set in both triangles, in list order."""
    M = np.zeros((n, n), order="F")
    for k in range(len(value)):
        i, j = int(suffix[0, k]) - 1, int(suffix[1, k]) - 1
        M[i, j] = value[k]
        if i != j:
            M[j, i] = value[k]
    return M


def loop_pattern(n, suffix):
    P = np.zeros((n, n), dtype=bool)
    for k in range(suffix.shape[1]):
        i, j = int(suffix[0, k]) - 1, int(suffix[1, k]) - 1
        P[i, j] = P[j, i] = True
    return P


def csr_from_loop(n, suffix, value):
    M, P = loop_mirror(n, suffix, value), loop_pattern(n, suffix)
    rowptr, col, val = [0], [], []
    for i in range(n):
        for j in range(n):
            if P[i, j]:
                col.append(j); val.append(M[i, j])
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


def mat(n, entries):
    suf = np.array([[e[0] for e in entries], [e[1] for e in entries]], dtype=np.int32).reshape(2, -1)
    return SparseMat(n, len(entries), suf, np.array([e[2] for e in entries], dtype=np.float64))


def assert_canonical(A):
    rowptr, col, val = solver.sparse_csr(A)
    r_ref, c_ref, v_ref = csr_from_loop(A.size, A.suffix, A.value)
    assert np.array_equal(rowptr, r_ref)
    assert np.array_equal(col, c_ref)
    assert val.tobytes() == v_ref.tobytes()           # bit for bit, -0.0 and NaN included
    return rowptr, col, val


def test_entries_in_both_triangles():
    A = mat(5, [(1, 1, 2.0), (3, 1, -1.0), (2, 4, 0.5), (5, 5, 7.0), (4, 5, -0.0), (1, 5, 3.0)])
    rowptr, col, val = assert_canonical(A)
    assert rowptr[-1] == 10 and list(col[rowptr[0]:rowptr[1]]) == [0, 2, 4]


def test_a_pair_given_three_times_across_both_triangles_the_last_wins():
    A = mat(4, [(2, 3, 1.0), (1, 1, 4.0), (3, 2, 2.0), (4, 4, 1.0), (2, 3, 3.0), (1, 1, 5.0)])
    rowptr, col, val = assert_canonical(A)
    assert val[rowptr[1]:rowptr[2]].tolist() == [3.0] and val[rowptr[2]:rowptr[3]].tolist() == [3.0]
    assert val[0] == 5.0
    # the other order of the same three: the entry of the upper triangle is now the last
    B = mat(4, [(2, 3, 1.0), (2, 3, 3.0), (3, 2, 2.0)])
    _, _, vb = assert_canonical(B)
    assert vb.tolist() == [2.0, 2.0]


def test_an_empty_row_a_full_row_and_an_empty_list():
    n = 7
    full = [(3, j, float(j)) for j in range(1, n + 1) if j != 5]      # row 3 full but for column 5; row 5 stays empty
    A = mat(n, full + [(1, 1, 1.0)])
    rowptr, col, _ = assert_canonical(A)
    assert rowptr[5] == rowptr[4]
    assert list(col[rowptr[2]:rowptr[3]]) == [0, 1, 2, 3, 5, 6]
    E = SparseMat(n, 0, np.zeros((2, 0), dtype=np.int32), np.zeros(0))
    rowptr, col, val = solver.sparse_csr(E)
    assert not rowptr.any() and col.size == 0 and val.size == 0


def test_nonfinite_values_pass_through():
    A = mat(3, [(1, 2, np.nan), (3, 3, np.inf), (2, 2, -np.inf)])
    assert_canonical(A)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_lists_and_their_permutations(seed):
    rng = np.random.default_rng(seed)
    n, nnz = 23, 140
    suf = rng.integers(1, n + 1, size=(2, nnz)).astype(np.int32)       # duplicates, both triangles, diagonal entries
    val = rng.standard_normal(nnz)
    A = SparseMat(n, nnz, suf, val)
    assert_canonical(A)
    # a permuted duplicate-free list gives the identical CSR
    M, P = loop_mirror(n, suf, val), np.tril(loop_pattern(n, suf))
    ii, jj = np.nonzero(P)
    flip = rng.random(ii.size) < 0.5
    clean = np.array([np.where(flip, jj, ii), np.where(flip, ii, jj)], dtype=np.int32) + 1
    cval = M[ii, jj]
    ref = solver.sparse_csr(SparseMat(n, ii.size, clean, cval))
    for _ in range(3):
        p = rng.permutation(ii.size)
        got = solver.sparse_csr(SparseMat(n, ii.size, np.ascontiguousarray(clean[:, p]), cval[p]))
        for a, b in zip(ref, got):
            assert a.tobytes() == b.tobytes()
    assert ref[2].tobytes() == solver.sparse_csr(A)[2].tobytes()


def test_an_index_outside_1_to_n_is_an_error_of_the_suffix_argument():
    lib = solver.load_library()
    n = 4
    rp = np.zeros(n + 1, dtype=np.int64); col = np.zeros(8, dtype=np.int32); cv = np.zeros(8)
    rpp = rp.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    val = np.ones(3)
    for bad in ((0, 1), (1, 0), (n + 1, 1), (2, n + 1), (-3, 2)):
        suf = np.array([[1, 1], bad, [2, 2]], dtype=np.int32)
        assert lib.ek_hip_debug_sparse_csr(n, 3, _ip(suf), _dp(val), rpp, _ip(col), _dp(cv)) == -3
        with pytest.raises(solver.SolverError):
            solver.sparse_csr(SparseMat(n, 3, np.ascontiguousarray(suf.T), val))
    ok = np.array([[1, 1], [n, 1], [2, 2]], dtype=np.int32)
    assert lib.ek_hip_debug_sparse_csr(n, 3, _ip(ok), _dp(val), rpp, _ip(col), _dp(cv)) == 4
    assert lib.ek_hip_debug_sparse_csr(-1, 3, _ip(ok), _dp(val), rpp, _ip(col), _dp(cv)) == -1
    assert lib.ek_hip_debug_sparse_csr(n, -1, _ip(ok), _dp(val), rpp, _ip(col), _dp(cv)) == -2
    assert lib.ek_hip_debug_sparse_csr(n, 3, None, _dp(val), rpp, _ip(col), _dp(cv)) == -3
    assert lib.ek_hip_debug_sparse_csr(n, 3, _ip(ok), None, rpp, _ip(col), _dp(cv)) == -4
    assert lib.ek_hip_debug_sparse_csr(n, 3, _ip(ok), _dp(val), None, _ip(col), _dp(cv)) == -5
    assert lib.ek_hip_debug_sparse_csr(0, 0, None, None, rpp, None, None) == 0


# ---------------------------------------------------------------------------------------- argument errors
N = 4
SUF = np.array([[1, 1], [2, 1], [3, 3], [4, 2]], dtype=np.int32)
BAD0 = np.array([[1, 1], [0, 1], [3, 3], [4, 2]], dtype=np.int32)
BADN = np.array([[1, 1], [2, 1], [3, N + 1], [4, 2]], dtype=np.int32)
VAL = np.array([2.0, -1.0, 2.0, 0.5])
DUMMY = ctypes.c_void_p(16)              # never dereferenced: every call below fails its checks first


def test_solve_sparse_argument_checks_without_gpu():
    lib = solver.load_library()
    desc = dsc.descinit(N, N, N, N, 0, 0, 0, N)
    w = np.zeros(N); z = np.zeros((N, N), order="F")

    def call(problem=1, n=N, n_vec=N, nnzA=4, sufA=_ip(SUF), valA=_dp(VAL), nnzB=4, sufB=_ip(SUF), valB=_dp(VAL),
             W=_dp(w), Z=_dp(z), D=_ip(desc), grid=(1, 1, 0, 0)):
        return lib.ek_hip_solve_sparse(problem, n, n_vec, nnzA, sufA, valA, nnzB, sufB, valB, W, Z, D, *grid, None, 0)
    assert call(problem=2) == -1 and call(problem=-1) == -1
    assert call(n=-1) == -2
    assert call(n_vec=-1) == -3 and call(n_vec=N + 1) == -3
    assert call(nnzA=-1) == -4
    assert call(sufA=None) == -5
    assert call(sufA=_ip(BAD0)) == -5 and call(sufA=_ip(BADN)) == -5
    assert call(valA=None) == -6
    assert call(nnzB=-1) == -7
    assert call(sufB=None) == -8
    assert call(sufB=_ip(BAD0)) == -8 and call(sufB=_ip(BADN)) == -8
    assert call(valB=None) == -9
    assert call(W=None) == -10
    assert call(Z=None) == -11
    assert call(D=None) == -12
    bad = desc.copy(); bad[2] = N + 1
    assert call(D=_ip(bad)) == -1203
    assert call(grid=(0, 1, 0, 0)) == -13
    assert call(grid=(1, 0, 0, 0)) == -14
    assert call(grid=(2, 1, 2, 0)) == -15
    assert call(grid=(1, 2, 0, 2)) == -16
    # the first offender decides; B is not looked at for problem 0; an empty list needs no arrays
    assert call(nnzA=-1, sufB=None) == -4
    assert call(sufA=_ip(BADN), valA=None) == -5
    assert call(problem=0, nnzB=-1, sufB=None, valB=None, W=None) == -10
    assert call(nnzA=0, sufA=None, valA=None, W=None) == -10
    # n = 0: success, nothing referenced
    assert call(n=0, n_vec=0, sufA=None, valA=None, sufB=None, valB=None, W=None, Z=None, D=None) == 0


@pytest.mark.parametrize("device", [False, True])
def test_check_sparse_argument_checks_without_gpu(device):
    lib = solver.load_library()
    w = np.zeros(N); z = np.zeros((N, N), order="F"); out = np.zeros(4); ipr = np.zeros(N)
    fn = lib.ek_hip_check_sparse_device if device else lib.ek_hip_check_sparse
    Wd, Zd = (DUMMY, DUMMY) if device else (_dp(w), _dp(z))

    def call(problem=1, n=N, nnzA=4, sufA=_ip(SUF), valA=_dp(VAL), nnzB=4, sufB=_ip(SUF), valB=_dp(VAL), W=Wd, Z=Zd,
             ldz=N, n_check=N, i1=1, i2=N, n_ipr=N, O=_dp(out), I=_dp(ipr)):
        return fn(problem, n, nnzA, sufA, valA, nnzB, sufB, valB, W, Z, ldz, n_check, i1, i2, n_ipr, O, I)
    assert call(problem=2) == -1
    assert call(n=-1) == -2
    assert call(nnzA=-1) == -3
    assert call(sufA=None) == -4 and call(sufA=_ip(BAD0)) == -4 and call(sufA=_ip(BADN)) == -4
    assert call(valA=None) == -5
    assert call(nnzB=-1) == -6
    assert call(sufB=None) == -7 and call(sufB=_ip(BAD0)) == -7 and call(sufB=_ip(BADN)) == -7
    assert call(valB=None) == -8
    assert call(W=None) == -9
    assert call(Z=None) == -10
    assert call(ldz=N - 1) == -11
    assert call(n_check=-1) == -12 and call(n_check=N + 1, W=Wd) == -12
    assert call(i1=0) == -13
    assert call(i2=N + 1) == -14
    assert call(n_ipr=-1) == -15 and call(n_ipr=N + 1) == -15
    assert call(O=None) == -16
    # the first offender decides; B is not looked at for problem 0
    assert call(sufA=_ip(BAD0), n_check=-1) == -4
    assert call(problem=0, nnzB=-1, sufB=None, valB=None, ldz=0) == -11
    # what a skipped part does not reference: no residual -> w; nothing at all -> Z and out
    assert call(n_check=0, W=None, ldz=0) == -11
    assert call(n_check=0, i1=3, i2=2, n_ipr=0, W=None, Z=None, O=None, I=None) == 0
    assert call(n_check=0, i1=3, i2=2, I=None, W=None, Z=None, O=None) == 0
    assert call(n_check=0, i1=5, i2=0, n_ipr=N, O=None, Z=None) == -10
    # n = 0: success, nothing referenced
    assert call(n=0, sufA=None, valA=None, sufB=None, valB=None, W=None, Z=None, O=None, I=None) == 0


def test_sparse_to_dense_argument_checks_without_gpu():
    lib = solver.load_library()
    m = np.zeros((N, N), order="F")
    fn = lib.ek_hip_sparse_to_dense
    assert fn(-1, 4, _ip(SUF), _dp(VAL), _dp(m), N) == -1
    assert fn(N, -1, _ip(SUF), _dp(VAL), _dp(m), N) == -2
    assert fn(N, 4, None, _dp(VAL), _dp(m), N) == -3
    assert fn(N, 4, _ip(BAD0), _dp(VAL), _dp(m), N) == -3
    assert fn(N, 4, _ip(BADN), _dp(VAL), _dp(m), N) == -3
    assert fn(N, 4, _ip(SUF), None, _dp(m), N) == -4
    assert fn(N, 4, _ip(SUF), _dp(VAL), None, N) == -5
    assert fn(N, 4, _ip(SUF), _dp(VAL), _dp(m), N - 1) == -6
    assert fn(0, 0, None, None, None, 0) == 0


def test_python_mirror_rejects_dense_matrices_for_triplet_inputs():
    with pytest.raises(ValueError):
        solver.eigen_solver("hip", np.eye(3), inputs="triplets")
    with pytest.raises(ValueError):
        solver.eigen_solver("general_hip", mat(3, [(1, 1, 1.0)]), np.eye(3), inputs="triplets")


# ---------------------------------------------------------------------------------------- the workspace hook
def a256(x):
    return (x + 255) // 256 * 256


def formula(problem, n, nnzA, nnzB, n_check, i1, i2, n_ipr):
    """include/ek_hip_debug.h, ek_hip_debug_sparse_check_workspace_bytes."""
    def csr(nnz):
        return a256(8 * (n + 1)) + a256(8 * nnz) + a256(16 * nnz)
    n_orth = i2 - i1 + 1 if i2 >= i1 else 0
    U = n_check if problem == 0 else max(n_check, i2 if n_orth else 0, n_ipr)
    ldt = max(64, (U + 63) // 64 * 64)
    rows = max(8, -(-n // 128))
    chunks = -(-n // rows)
    t = csr(nnzA) + a256(8 * ldt * n if U else 0) + a256(8 * n_orth * n_orth) + a256(8 * chunks * ldt if U else 0)
    t += a256(8 * (max(n_check, n_orth) + 520)) + a256(8 * (n_ipr + 8))
    if problem == 1:
        t += csr(nnzB) + a256(8 * ldt * n if U else 0) + a256(8 * n * U)
    return t


@pytest.mark.parametrize("n", [30, 65, 400, 1000, 4096, 16384, 32768])
@pytest.mark.parametrize("problem", [0, 1])
def test_the_workspace_hook_matches_its_stated_formula(n, problem):
    nnz = 33 * n
    for n_check, i1, i2, n_ipr in ((n, 1, n, n), (1, 1, 0, 0), (0, 2, n - 1, 0), (0, 1, 0, n // 2), (min(63, n), 3, 17, 5),
                                   (n // 3, n // 2, n, 0)):
        got = solver.sparse_check_workspace_bytes(problem, n, nnz, nnz // 2, n_check, i1, i2, n_ipr)
        assert got == formula(problem, n, nnz, nnz // 2, n_check, i1, i2, n_ipr), (n, problem, n_check, i1, i2, n_ipr)
    # no n x n image of A or B: with a few columns the workspace is far below one matrix
    if n >= 4096:
        assert solver.sparse_check_workspace_bytes(problem, n, nnz, nnz, 64, 1, 64, 64) < 8 * n * n // 8


def test_the_workspace_hook_rejects_bad_arguments():
    f = solver.load_library().ek_hip_debug_sparse_check_workspace_bytes
    assert f(2, 100, 10, 10, 100, 1, 100, 100) == 0
    assert f(1, 0, 0, 0, 0, 1, 0, 0) == 0
    assert f(1, 100, -1, 10, 100, 1, 100, 100) == 0
    assert f(1, 100, 10, -1, 100, 1, 100, 100) == 0
    assert f(0, 100, 10, -1, 100, 1, 100, 100) > 0          # (B is not looked at for problem 0)
    assert f(1, 100, 10, 10, 101, 1, 100, 100) == 0
    assert f(1, 100, 10, 10, 100, 0, 100, 100) == 0
    assert f(1, 100, 10, 10, 100, 1, 101, 100) == 0
    assert f(1, 100, 10, 10, 100, 1, 100, 101) == 0
    assert f(1, 100, 10, 10, 0, 1, 0, 0) == 0                # nothing to do
