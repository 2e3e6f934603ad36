"""GPU suite of the triplet entries: ek_hip_sparse_to_dense (the densification alone), ek_hip_solve_sparse (the whole
path on the reference's own arguments) and ek_hip_check_sparse* (the acceptance quantities from the triplets).

Yardsticks.  The densification: an explicit loop that does what distribute_matrix.f90:411-418 does, byte for byte.  The
solve: ek_hip_solve_replicated on the mirrored dense matrices, bit for bit (the same Path runs on the same images).  The
check: the host mirror eigenkernel_amd/verifier.py on the dense mirrored matrices, and the dense device entries
ek_hip_residual_device / ek_hip_orthogonality_device / ek_hip_ipratios_device, within the suite's own 4 max(n, 8) eps --
a_norm relative, the rest absolute, as tests/test_gpu_check_sygv.py -- on SciPy eigenpairs of seeded banded pairs with
cond_2(B) <= 16 (asserted).  Each comparison prints the largest share of the bound it used (pytest -s shows it)."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import descriptor as dsc
from eigenkernel_amd import read_matrix_file, verifier
from eigenkernel_amd.matrix_io import SparseMat

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


def P(a):
    return a.ctypes.data_as(_dp)


def I(a):
    return a.ctypes.data_as(_ip)


# ------------------------------------------------------------------------------------------------ inputs
def loop_mirror(M):
    """distribute_matrix.f90:411-418 on one rank: every entry is set in both triangles, in list order."""
    D = np.zeros((M.size, M.size), order="F")
    for k in range(M.num_non_zeros):
        i, j = int(M.suffix[0, k]) - 1, int(M.suffix[1, k]) - 1
        D[i, j] = M.value[k]
        D[j, i] = M.value[k]
    return D


def triplets_of(D, seed=0, keep_zeros=False):
    """A duplicate-free list of the lower triangle of the symmetric D, each entry given in a triangle picked at random."""
    rng = np.random.default_rng(seed)
    ii, jj = np.nonzero(np.tril(np.ones_like(D)) if keep_zeros else np.tril(D != 0.0))
    flip = rng.random(ii.size) < 0.5
    suf = np.array([np.where(flip, jj, ii), np.where(flip, ii, jj)], dtype=np.int32) + 1
    return SparseMat(D.shape[0], ii.size, np.ascontiguousarray(suf), np.ascontiguousarray(D[ii, jj]))


def permuted(M, seed):
    p = np.random.default_rng(seed).permutation(M.num_non_zeros)
    return SparseMat(M.size, M.num_non_zeros, np.ascontiguousarray(M.suffix[:, p]), np.ascontiguousarray(M.value[p]))


def banded(n, bw, seed, spd):
    """Seeded symmetric band of half bandwidth bw.  spd: diagonal 2, off-diagonal row sums below 1: spectrum in [1, 3]."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    for k in range(1, min(bw, n - 1) + 1):
        v = rng.uniform(-1.0, 1.0, n - k) * (0.5 / bw if spd else 1.0)
        D += np.diag(v, -k) + np.diag(v, k)
    D += np.diag(np.full(n, 2.0) if spd else rng.uniform(-1.0, 1.0, n))
    return D


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(n, problem, variant="band"):
    """A seeded banded pair of order n with SciPy's eigenpairs, its triplets and the host mirror's figures.  Read only."""
    c = _Case()
    bw = min(8, n - 1)
    A = banded(n, bw, 100 + n, False)
    if variant == "full":                     # a row of length n in A
        A[3, :] = A[:, 3] = np.random.default_rng(7).uniform(0.5, 1.0, n)
    if variant == "empty":                    # a row of length 0 in A
        A[n // 2, :] = 0.0; A[:, n // 2] = 0.0
    B = banded(n, bw, 200 + n, True) if problem == 1 else None
    if B is not None:
        assert np.linalg.cond(B) <= 16.0
    c.w, c.Z = sl.eigh(A, B, lower=True) if B is not None else sl.eigh(A, lower=True)
    c.Z = np.asfortranarray(c.Z)
    c.n, c.A, c.B, c.problem = n, A, B, problem
    c.tA, c.tB = triplets_of(A, 1), (triplets_of(B, 2) if B is not None else None)
    assert np.array_equal(loop_mirror(c.tA), A)
    for a in (A, c.w, c.Z, c.tA.suffix, c.tA.value) + ((B, c.tB.suffix, c.tB.value) if B is not None else ()):
        a.setflags(write=False)
    return c


def mirror_figures(c, n_check, index1, index2, n_ipr):
    norm, ave, mx = verifier.eval_residual_norm(c.A, c.w[:n_check], c.Z[:, :n_check], c.B)
    orth = verifier.eval_orthogonality(c.Z, c.B, index1, index2)
    return np.array([norm, ave, mx, orth]), verifier.get_ipratios(c.Z[:, :n_ipr], c.B)


def shares(out, ipr, ref_out, ref_ipr, n):
    tol = 4 * max(n, 8) * EPS
    s = np.abs(np.asarray(out) - ref_out) / tol
    s[0] /= abs(ref_out[0])
    return np.append(s, np.abs(ipr - ref_ipr).max() / tol if len(ref_ipr) else 0.0)


class _Dev:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def up(self, a):
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), max(int(a.nbytes), 8)) == 0
        self.ptrs.append(p)
        if a.nbytes:
            assert self.lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def down(self, p, like):
        out = np.empty_like(like)
        assert self.lib.ek_hip_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)


def _args(M):
    """(nnz, suffix, value, keepalive) as the C-ABI takes a list; None stands for `not given`."""
    if M is None:
        return 0, None, None, None
    suf = np.ascontiguousarray(np.asarray(M.suffix, dtype=np.int32).T)
    val = np.ascontiguousarray(M.value, dtype=np.float64)
    return int(val.size), (I(suf) if val.size else None), (P(val) if val.size else None), (suf, val)


def check_device(lib, problem, n, tA, tB, dw, dZ, ldz, n_check, index1, index2, n_ipr):
    a, b = _args(tA), _args(tB)
    out = np.full(4, -7.25e77)
    ipr = np.full(max(n_ipr, 1), -7.25e77)
    rc = lib.ek_hip_check_sparse_device(problem, n, *a[:3], *b[:3], dw, dZ, ldz, n_check, index1, index2, n_ipr, P(out),
                                        P(ipr))
    assert rc == 0, rc
    return out, ipr[:n_ipr]


# ------------------------------------------------------------------------------------------------ the densification
def _golden(golden_dir, name):
    return read_matrix_file(os.path.join(golden_dir, name))


def _seeded_list(n, seed):
    """Duplicates, both triangles, diagonal entries, -0.0, and a row that no entry names."""
    rng = np.random.default_rng(seed)
    nnz = 6 * n
    suf = rng.integers(1, n + 1, size=(2, nnz)).astype(np.int32)
    empty = n // 2 + 1
    suf[suf == empty] = 1
    val = rng.standard_normal(nnz)
    val[::17] = -0.0
    return SparseMat(n, nnz, suf, val)


@pytest.mark.parametrize("which", ["BNZ30_A", "BNZ30_B", "VCNT400", "seeded65", "seeded257"])
def test_sparse_to_dense_equals_the_loop_mirror_byte_for_byte(hip, golden_dir, which):
    M = {"BNZ30_A": lambda: _golden(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"),
         "BNZ30_B": lambda: _golden(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx"),
         "VCNT400": lambda: _golden(golden_dir, "ELSES_MATRIX_VCNT400std_A.mtx"),
         "seeded65": lambda: _seeded_list(65, 65), "seeded257": lambda: _seeded_list(257, 257)}[which]()
    n = M.size
    ref = loop_mirror(M)
    if which.startswith("seeded"):
        assert not ref[n // 2].any() and M.num_non_zeros > np.count_nonzero(np.tril(ref))     # an empty row, duplicates
    lib = hip.load_library()
    ldm = n + 3
    buf = np.full((ldm, n), np.nan, order="F")
    a = _args(M)
    before = (a[3][0].copy(), a[3][1].copy())
    assert lib.ek_hip_sparse_to_dense(n, *a[:3], P(buf), ldm) == 0
    assert buf[:n].tobytes() == np.asfortranarray(ref).tobytes()
    assert np.isnan(buf[n:]).all()                                       # what lies between the columns survives
    assert before[0].tobytes() == a[3][0].tobytes() and before[1].tobytes() == a[3][1].tobytes()
    assert hip.sparse_to_dense(M).tobytes() == np.asfortranarray(ref).tobytes()
    if not which.startswith("seeded"):
        assert np.array_equal(ref, M.to_dense())


# ------------------------------------------------------------------------------------------------ the solve
def _solve(lib, sparse, problem, n, n_vec, tA, tB, A, B, grid=(1, 1, 0, 0), nb=None):
    """ek_hip_solve_sparse on the triplets or ek_hip_solve_replicated on the mirrored matrices, for one grid cell:
    (info, w, Z_loc)."""
    desc, Z = dsc.setup_distributed_matrix(n, n, *grid, block_size=nb)
    Z[...] = -7.25e77
    w = np.full(n, -7.25e77)
    if sparse:
        a, b = _args(tA), _args(tB if problem else None)
        info = lib.ek_hip_solve_sparse(problem, n, n_vec, *a[:3], *b[:3], P(w), P(Z), I(desc), *grid, None, 0)
    else:
        Ad = np.array(A, order="F", copy=True)
        Bd = np.array(B, order="F", copy=True) if problem else None
        info = lib.ek_hip_solve_replicated(problem, n, n_vec, P(Ad), n, P(Bd) if problem else None, n, P(w), P(Z), I(desc),
                                           *grid, None, 0)
    return info, w, Z


def _same_bits(lib, problem, n, n_vec, tA, tB, A, B, **kw):
    i1, w1, Z1 = _solve(lib, True, problem, n, n_vec, tA, tB, A, B, **kw)
    i0, w0, Z0 = _solve(lib, False, problem, n, n_vec, tA, tB, A, B, **kw)
    assert i1 == 0 and i0 == 0, (i1, i0)
    assert w1[:n_vec].tobytes() == w0[:n_vec].tobytes()
    assert Z1.tobytes() == Z0.tobytes()
    return w1, Z1


def test_solve_sparse_bnz30_generalized_bits_and_golden(hip, golden_dir):
    tA, tB = _golden(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"), _golden(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    w, _ = _same_bits(hip.load_library(), 1, 30, 30, tA, tB, loop_mirror(tA), loop_mirror(tB))
    assert np.abs(w - ev).max() <= 1e-14          # the bound of tests/test_gpu_path.py::test_golden_bnz30_generalized


def test_solve_sparse_vcnt400_standard_bits(hip, golden_dir):
    tA = _golden(golden_dir, "ELSES_MATRIX_VCNT400std_A.mtx")
    E = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_E.txt"))[:, 1]
    w, _ = _same_bits(hip.load_library(), 0, 400, 400, tA, None, loop_mirror(tA), None)
    assert np.abs(w - E).max() <= 1e-12


@pytest.mark.parametrize("n_vec", [600, 77])
def test_solve_sparse_two_stage_bits(hip, n_vec):
    c = _case(600, 1)
    lib = hip.load_library()
    w, Z = _same_bits(lib, 1, 600, n_vec, c.tA, c.tB, c.A, c.B)
    if n_vec == 600:                              # a permuted list changes no bit
        i2, w2, Z2 = _solve(lib, True, 1, 600, 600, permuted(c.tA, 5), permuted(c.tB, 6), None, None)
        assert i2 == 0 and w2.tobytes() == w.tobytes() and Z2.tobytes() == Z.tobytes()


def test_solve_sparse_every_cell_of_a_2x2_grid(hip):
    c = _case(130, 1)
    lib = hip.load_library()
    for myrow in range(2):
        for mycol in range(2):
            _same_bits(lib, 1, 130, 130, c.tA, c.tB, c.A, c.B, grid=(2, 2, myrow, mycol), nb=32)


def test_solve_sparse_info_of_a_b_that_is_not_spd(hip):
    c = _case(130, 1)
    Bbad = np.array(c.B); Bbad[40, 40] = -3.0
    lib = hip.load_library()
    i1, _, _ = _solve(lib, True, 1, 130, 130, c.tA, triplets_of(Bbad, 3), None, None)
    i0, _, _ = _solve(lib, False, 1, 130, 130, None, None, c.A, Bbad)
    assert i1 == i0 and i0 > 0, (i1, i0)


# ------------------------------------------------------------------------------------------------ the check
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [30, 200, 600])
def test_check_sparse_against_the_host_mirror(hip, n, problem):
    c = _case(n, problem)
    ref_out, ref_ipr = mirror_figures(c, n, 1, n, n)
    got = hip.check_sparse(c.tA, c.tB, c.w, c.Z)
    s = shares(got[:4], got[4], ref_out, ref_ipr, n)
    print("n=%d problem=%d shares of 4 max(n,8) eps: %s" % (n, problem, np.array2string(s, precision=4)))
    assert s.max() <= 1.0, s


def _dense_device(lib, dev, c, dw, dZ, ldz, n_check, index1, index2, n_ipr):
    """The three dense device entries on the mirrored matrices."""
    n = c.n
    dA = dev.up(np.asfortranarray(c.A))
    dB = dev.up(np.asfortranarray(c.B)) if c.problem else None
    r = [ctypes.c_double(-1.0) for _ in range(4)]
    ipr = np.zeros(max(n_ipr, 1))
    assert lib.ek_hip_residual_device(c.problem, n, n_check, dA, n, dB, n, dw, dZ, ldz, ctypes.byref(r[0]),
                                      ctypes.byref(r[1]), ctypes.byref(r[2])) == 0
    assert lib.ek_hip_orthogonality_device(c.problem, n, index1, index2, dB, n, dZ, ldz, ctypes.byref(r[3])) == 0
    assert lib.ek_hip_ipratios_device(c.problem, n, n_ipr, dB, n, dZ, ldz, P(ipr)) == 0
    return np.array([x.value for x in r]), ipr[:n_ipr]


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("variant", ["band", "full", "empty"])
@pytest.mark.parametrize("n_check", [1, 63, 65, 200])
def test_check_sparse_shapes_against_mirror_and_dense_entries(hip, n_check, variant, problem):
    n = 200
    c = _case(n, problem, variant)
    lens = np.diff(hip.sparse_csr(c.tA)[0])
    assert variant != "full" or lens[3] == n
    assert variant != "empty" or lens[n // 2] == 0
    index1, index2, n_ipr, ldz = 7, 150, 131, n + 5
    lib = hip.load_library()
    Zp = np.full((ldz, n), np.nan, order="F"); Zp[:n] = c.Z                # padded ldz among NaN
    with _Dev(lib) as dev:
        dw, dZ = dev.up(np.ascontiguousarray(c.w)), dev.up(Zp)
        out, ipr = check_device(lib, problem, n, c.tA, c.tB, dw, dZ, ldz, n_check, index1, index2, n_ipr)
        again = check_device(lib, problem, n, c.tA, c.tB, dw, dZ, ldz, n_check, index1, index2, n_ipr)
        perm = check_device(lib, problem, n, permuted(c.tA, 11), permuted(c.tB, 12) if problem else None, dw, dZ, ldz,
                            n_check, index1, index2, n_ipr)
        d_out, d_ipr = _dense_device(lib, dev, c, dw, dZ, ldz, n_check, index1, index2, n_ipr)
        # the inputs come back byte for byte
        assert dev.down(dZ, Zp).tobytes() == Zp.tobytes() and dev.down(dw, c.w).tobytes() == c.w.tobytes()
    for other in (again, perm):                                             # repeated calls, a permuted list: the same bits
        assert other[0].tobytes() == out.tobytes() and other[1].tobytes() == ipr.tobytes()
    ref_out, ref_ipr = mirror_figures(c, n_check, index1, index2, n_ipr)
    s_m = shares(out, ipr, ref_out, ref_ipr, n)
    s_d = shares(out, ipr, d_out, d_ipr, n)
    print("n_check=%d %s problem=%d shares: mirror %s dense entries %s"
          % (n_check, variant, problem, np.array2string(s_m, precision=4), np.array2string(s_d, precision=4)))
    assert s_m.max() <= 1.0 and s_d.max() <= 1.0, (s_m, s_d)
    if problem == 0:                                                        # the same GEMM call, the same kernels
        assert out[3] == d_out[3] and ipr.tobytes() == d_ipr.tobytes()


@pytest.mark.parametrize("problem", [0, 1])
def test_check_sparse_skipped_parts_and_an_empty_a(hip, problem):
    n = 200
    c = _case(n, problem)
    lib = hip.load_library()
    empty = SparseMat(n, 0, np.zeros((2, 0), dtype=np.int32), np.zeros(0))
    with _Dev(lib) as dev:
        dw, dZ = dev.up(np.ascontiguousarray(c.w)), dev.up(c.Z)
        full = check_device(lib, problem, n, c.tA, c.tB, dw, dZ, n, n, 1, n, n)
        # a skipped part leaves its outputs as they were (the sentinel of check_device)
        o, q = check_device(lib, problem, n, c.tA, c.tB, dw, dZ, n, 0, 1, n, n)
        assert (o[:3] == -7.25e77).all() and o[3] == full[0][3] and q.tobytes() == full[1].tobytes()
        o, q = check_device(lib, problem, n, c.tA, c.tB, dw, dZ, n, n, 2, 1, 0)
        assert o[:3].tobytes() == full[0][:3].tobytes() and o[3] == -7.25e77
        o, q = check_device(lib, problem, n, c.tA, c.tB, None, dZ, n, 0, 2, 1, 5)
        assert (o == -7.25e77).all() and q.tobytes() == full[1][:5].tobytes()
        # nnz = 0: a_norm = 0, plain IEEE divisions in the residual slots, the rest untouched by A
        o, q = check_device(lib, problem, n, empty, c.tB, dw, dZ, n, n, 1, n, n)
        assert o[0] == 0.0 and not np.isfinite(o[1]) and not np.isfinite(o[2])
        assert o[3] == full[0][3] and q.tobytes() == full[1].tobytes()


@pytest.mark.parametrize("problem", [0, 1])
def test_a_planted_error_in_one_column_shows_in_the_residual_alone(hip, problem):
    n = 200
    c = _case(n, problem)
    lib = hip.load_library()
    bad = n - 1                                    # the last column: checked by the residual, outside the other two parts
    Zb = np.array(c.Z, order="F"); Zb[5, bad] += 1e-6
    with _Dev(lib) as dev:
        dw = dev.up(np.ascontiguousarray(c.w))
        good = check_device(lib, problem, n, c.tA, c.tB, dw, dev.up(c.Z), n, n, 2, n - 2, n - 2)
        got = check_device(lib, problem, n, c.tA, c.tB, dw, dev.up(Zb), n, n, 2, n - 2, n - 2)
    assert good[0][2] <= 4e-14 and got[0][2] >= 1e-9, (good[0], got[0])
    assert got[0][0] == good[0][0] and got[0][3] == good[0][3] and got[1].tobytes() == good[1].tobytes()
    assert abs((got[0][1] - good[0][1]) - (got[0][2] - 0.0) / n) <= got[0][2] / n * 0.5       # res_ave: its share of it


def test_solve_sparse_then_check_sparse_on_bnz30(hip, golden_dir):
    tA, tB = _golden(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"), _golden(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")
    gipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    ep = hip.solve_sparse(tA, tB)
    a_norm, ave, mx, orth, ipr = hip.check_sparse(tA, tB, ep.values, ep.Vectors)
    assert a_norm > 0 and mx <= 4e-14 and orth <= 1e-11, (a_norm, ave, mx, orth)
    assert np.abs(ipr - gipr).max() <= 1e-6
    ep2, _ = hip.eigen_solver("general_hip", tA, tB, inputs="triplets")
    assert ep2.values.tobytes() == ep.values.tobytes() and ep2.Vectors.tobytes() == ep.Vectors.tobytes()
    assert "eigen_solver_scalapack_all:pdsytrd" in ep.stage_seconds


def test_fortran_host_with_triplets(tmp_path, golden_dir):
    """host/eigenkernel_hip_app --triplets on the BNZ30 pair against the run without the flag: eigenvalues.dat byte for
    byte, ipratios.dat within 4 max(n, 8) eps, the same stdout milestones (built as tests/test_gpu_path.py builds it)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "eigenkernel_hip_app")
    if not os.path.exists(exe):
        flang = "/opt/rocm/lib/llvm/bin/flang"
        assert os.path.exists(flang), "flang missing: cannot build the Fortran host"
        subprocess.check_call(["make", "-C", os.path.join(root, "host")])
    runs = {}
    for flag in ((), ("--triplets",)):
        d = tmp_path / ("t" if flag else "d")
        d.mkdir()
        out = subprocess.run([exe, "-s", "general_hip", "-c", "-1", "-t", "1,30", *flag,
                              os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"),
                              os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")],
                             cwd=d, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        runs[bool(flag)] = (d, out.stdout)
    (dd, sd), (dt, st) = runs[False], runs[True]
    assert (dt / "eigenvalues.dat").read_bytes() == (dd / "eigenvalues.dat").read_bytes()
    ipr_d, ipr_t = np.loadtxt(dd / "ipratios.dat"), np.loadtxt(dt / "ipratios.dat")
    assert ipr_t.shape == ipr_d.shape == (30, 2)
    assert np.abs(ipr_t[:, 1] - ipr_d[:, 1]).max() <= 4 * 30 * EPS
    gipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    assert np.abs(ipr_t[:, 1] - gipr).max() <= 1e-6
    miles = lambda s: [l.split(":")[0] for l in s.splitlines()]
    assert miles(st) == miles(sd) and "residual norm (max)" in miles(st) and "orthogonality criterion" in miles(st)
    val = lambda s, key: float([l for l in s.splitlines() if l.startswith(key)][0].split(":")[1])
    assert val(st, "residual norm (max)") <= 2e-15 and val(st, "orthogonality criterion") <= 1e-13
    assert abs(val(st, "A norm") / val(sd, "A norm") - 1.0) <= 4 * 30 * EPS


# ------------------------------------------------------------------------------------------------ cost
def test_check_sparse_costs_no_more_than_the_three_dense_checks(hip):
    """n = 4096, half bandwidth 32, generalized, all columns: ek_hip_check_sparse_device (CSR build and upload included)
    against ek_hip_residual_device + ek_hip_orthogonality_device + ek_hip_ipratios_device, best of 3, alternated.  The
    sparse call does one of their five dense products and nothing else of order n^3: above 1 x is a defect.  The measured
    ratio is in DESIGN.md 27."""
    n, bw = 4096, 32
    rng = np.random.default_rng(4096)
    off = np.arange(n)
    rows, cols, vals = [off], [off], [np.full(n, 2.0)]
    for k in range(1, bw + 1):
        rows.append(off[k:]); cols.append(off[:-k]); vals.append(rng.uniform(-1.0, 1.0, n - k) * 0.5 / bw)
    suf = np.ascontiguousarray(np.array([np.concatenate(rows), np.concatenate(cols)], dtype=np.int32) + 1)
    t = SparseMat(n, suf.shape[1], suf, np.concatenate(vals))
    D = t.to_dense()
    Z = np.asfortranarray(rng.standard_normal((n, n)))
    w = rng.standard_normal(n)
    lib = hip.load_library()
    ipr = np.zeros(n)
    r = [ctypes.c_double(0.0) for _ in range(4)]
    with _Dev(lib) as dev:
        dw, dZ, dA = dev.up(w), dev.up(Z), dev.up(D)

        def dense():
            assert lib.ek_hip_residual_device(1, n, n, dA, n, dA, n, dw, dZ, n, ctypes.byref(r[0]), ctypes.byref(r[1]),
                                              ctypes.byref(r[2])) == 0
            assert lib.ek_hip_orthogonality_device(1, n, 1, n, dA, n, dZ, n, ctypes.byref(r[3])) == 0
            assert lib.ek_hip_ipratios_device(1, n, n, dA, n, dZ, n, P(ipr)) == 0

        def sparse():
            check_device(lib, 1, n, t, t, dw, dZ, n, n, 1, n, n)
        dense(); sparse()                           # workspaces grown, kernels loaded
        td, ts = [], []
        for _ in range(3):
            t0 = time.perf_counter(); dense(); t1 = time.perf_counter(); sparse(); t2 = time.perf_counter()
            td.append(t1 - t0); ts.append(t2 - t1)
    print("dense checks %.2f ms, sparse check %.2f ms, ratio %.3f" % (min(td) * 1e3, min(ts) * 1e3, min(ts) / min(td)))
    assert min(ts) <= min(td), (ts, td)
