"""GPU suite of the eigenvalues-only interface: the bisection stage (ek_hip_stebz) on tridiagonals with analytic and
hard spectra, its range independence and determinism, and the whole values-only path (ek_hip_eigenvalues*) against
the fixtures, against the full path on the same inputs, on its error returns and on its speed."""
import ctypes
import os
import time

import numpy as np
import pytest

from eigenkernel_amd.matrix_io import read_matrix_file

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
_dp = ctypes.POINTER(ctypes.c_double)


def _bound(n, w_ref):
    return 4 * n * EPS * float(np.abs(w_ref).max())


# ------------------------------------------------------------------------------------------- the bisection stage
def _toeplitz121(n):
    k = np.arange(1, n + 1)
    return np.full(n, 2.0), np.full(max(n - 1, 0), -1.0), np.sort(2.0 - 2.0 * np.cos(k * np.pi / (n + 1)))


def _clement(n):
    i = np.arange(1, n)
    return np.zeros(n), np.sqrt(i * (n - i.astype(np.float64))), np.arange(-(n - 1), n, 2, dtype=np.float64)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 1000, 4097])
@pytest.mark.parametrize("kind", ["toeplitz121", "clement"])
def test_stebz_analytic_spectra(hip, kind, n):
    d, e, w_ref = (_toeplitz121 if kind == "toeplitz121" else _clement)(n)
    w = hip.stebz(d, e)
    assert w.shape == (n,)
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w_ref).max() <= _bound(n, w_ref) + (0.0 if n > 1 else 4 * EPS * abs(w_ref[0]))


def _wilkinson21():
    return np.abs(np.arange(21) - 10.0), np.ones(20)


def _glued_wilkinson(copies=10, delta=1e-14):
    d0, e0 = _wilkinson21()
    d = np.tile(d0, copies)
    e = np.concatenate([np.concatenate([e0, [delta]]) for _ in range(copies)])[:-1]
    return d, e


def _hard_cases():
    rng = np.random.default_rng(7)
    cases = {"wilkinson21": _wilkinson21(), "glued_wilkinson": _glued_wilkinson(),
             "diagonal": (rng.standard_normal(300), np.zeros(299)),
             "zero": (np.zeros(50), np.zeros(49))}
    out = []
    for name, (d, e) in cases.items():
        for scale in (1.0, 1e150, 1e-150):
            out.append(pytest.param(d * scale, e * scale, id="%s-%g" % (name, scale)))
    return out


@pytest.mark.parametrize("d,e", _hard_cases())
def test_stebz_hard_spectra_against_dense(hip, d, e):
    n = d.shape[0]
    T = np.diag(d) + np.diag(e, -1) + np.diag(e, 1)
    w_ref = np.linalg.eigvalsh(T)
    w = hip.stebz(d, e)
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w_ref).max() <= _bound(n, w_ref)
    if not np.any(e):
        assert np.abs(w - np.sort(d)).max() <= _bound(n, w_ref)


def test_stebz_range_independent_and_deterministic(hip):
    n = 3000
    rng = np.random.default_rng(11)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    w_all = hip.stebz(d, e)
    assert np.array_equal(w_all, hip.stebz(d, e))            # bit for bit, call to call
    for il, iu in [(1, 1), (n, n), (1234, 1234), (1, n), (2, 17), (1500, 1700), (2990, 3000), (999, 2001)]:
        w = hip.stebz(d, e, il, iu)
        assert np.array_equal(w, w_all[il - 1:iu]), (il, iu)
    T = np.diag(d) + np.diag(e, -1) + np.diag(e, 1)
    assert np.abs(w_all - np.linalg.eigvalsh(T)).max() <= _bound(n, w_all)


# ------------------------------------------------------------------------------------------- the whole path
def test_values_bnz30_generalized(hip, golden_dir):
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx")).to_dense()
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense()
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    w = hip.eigenvalues(A, B)
    assert np.abs(w - ev).max() <= 30 * EPS * np.abs(ev).max()
    assert np.array_equal(hip.eigenvalues(A, B, 3, 7), w[2:7])


def test_values_vcnt400_standard(hip, golden_dir):
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_A.mtx")).to_dense()
    E = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_E.txt"))[:, 1]
    w = hip.eigenvalues(A)
    assert np.abs(w - E).max() <= max(400 * EPS * np.abs(E).max(), 1e-12)   # (the fixture has 12 digits)


@pytest.mark.parametrize("name,n,gep", [("gep_n256_np4", 256, True), ("sep_n256_np4", 256, False),
                                         ("gep_n1000_np4", 1000, True), ("sep_n4096_np8", 4096, False)])
def test_values_against_scalapack_goldens(hip, oracle, golden_dir, name, n, gep):
    w_ref = np.loadtxt(os.path.join(golden_dir, "scalapack_synth_%s.txt" % name))
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    w = hip.eigenvalues(A, B)
    assert np.abs(w - w_ref).max() <= n * EPS * np.abs(w_ref).max()


class _Dev:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), max(int(nbytes), 8)) == 0
        self.ptrs.append(p)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)
        self.lib.ek_hip_finalize()


def _values_device(lib, dA, dB, dw, n, gep, il=1, iu=None, st=None):
    iu = n if iu is None else iu
    assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
    if gep:
        assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
    t0 = time.perf_counter()
    info = lib.ek_hip_eigenvalues_device(1 if gep else 0, n, il, iu, dA, n, dB if gep else None, n, dw,
                                         st.ctypes.data_as(_dp) if st is not None else None, 0 if st is None else len(st))
    return info, time.perf_counter() - t0


def test_values_c3_n16384_generalized_full_size(hip, golden_dir):
    lib = hip.load_library()
    n = 16384
    w_ref = np.loadtxt(os.path.join(golden_dir, "scalapack_synth_gep_n16384_np8.txt"))
    with _Dev(lib) as dev:
        dA, dB, dw = dev.alloc(n * n * 8), dev.alloc(n * n * 8), dev.alloc(n * 8)
        st = np.zeros(8)
        info, _ = _values_device(lib, dA, dB, dw, n, True, st=st)
        assert info == 0
        w = np.zeros(n)
        assert lib.ek_hip_memcpy_d2h(w.ctypes.data, dw, w.nbytes) == 0
        assert np.abs(w - w_ref).max() <= n * EPS * np.abs(w_ref).max()
        assert st[5] == 0.0 and st[6] == 0.0 and st[4] > 0.0 and st[2] > 0.0
        # a slice of the same problem: the same bits
        info, _ = _values_device(lib, dA, dB, dw, n, True, il=8000, iu=8100)
        assert info == 0
        w2 = np.zeros(101)
        assert lib.ek_hip_memcpy_d2h(w2.ctypes.data, dw, w2.nbytes) == 0
        assert np.array_equal(w2, w[7999:8100])


@pytest.mark.parametrize("gep", [False, True])
@pytest.mark.parametrize("n", [100, 511, 512, 513, 2048])
@pytest.mark.parametrize("two_stage", [True, False])
def test_values_against_full_path(hip, oracle, n, gep, two_stage):
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    hip.set_two_stage(3 if two_stage else 0)
    w = hip.eigenvalues(A, B)
    ep, _ = hip.eigen_solver("general_hip" if gep else "hip", A, B)
    assert np.abs(w - ep.values).max() <= _bound(n, ep.values)
    assert hip.last_solve_stats()[1] == (1.0 if two_stage else 0.0)


def _banded(n, bw, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A = A + A.T
    A[np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > bw] = 0.0
    return np.asfortranarray(A)


def _lowrank_plus_identity(n, r, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, r))
    return np.asfortranarray(U @ U.T + np.eye(n))


@pytest.mark.parametrize("case", ["band_input", "identity", "lowrank_plus_identity", "banded_gep"])
def test_values_special_inputs(hip, oracle, case):
    n = 1024
    hip.set_two_stage(3)
    B = None
    if case == "band_input":
        A = _banded(n, 40, 1)                          # the band short cut (standard, nothing below the 64th subdiagonal)
    elif case == "identity":
        A = np.asfortranarray(np.eye(n))
    elif case == "lowrank_plus_identity":
        A = _lowrank_plus_identity(n, 5, 2)            # panels of the first stage take the Householder rescue
    else:
        A = _banded(n, 100, 3)
        B = oracle.synth_matrix(n, 2)
    w = hip.eigenvalues(A, B)
    if case == "band_input":
        assert hip.last_solve_stats()[3] == 1.0
    if case == "identity":
        assert np.array_equal(w, np.ones(n)) or np.abs(w - 1.0).max() <= _bound(n, np.ones(1))
    ep, _ = hip.eigen_solver("general_hip" if B is not None else "hip", A, B)
    assert np.abs(w - ep.values).max() <= _bound(n, ep.values)
    assert np.all(np.diff(w) >= 0)


def test_values_errors_and_untouched_inputs(hip, oracle):
    lib = hip.load_library()
    n = 300
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    A0, B0 = A.copy(order="F"), B.copy(order="F")
    w = np.zeros(n)
    st = np.zeros(8)
    info = lib.ek_hip_eigenvalues(1, n, 1, n, A.ctypes.data_as(_dp), n, B.ctypes.data_as(_dp), n,
                                  w.ctypes.data_as(_dp), st.ctypes.data_as(_dp), 8)
    assert info == 0
    assert A.tobytes() == A0.tobytes() and B.tobytes() == B0.tobytes()
    # NaN in A: -5
    An = A.copy(order="F"); An[7, 3] = np.nan; An[3, 7] = np.nan
    with pytest.raises(hip.SolverError) as ex:
        hip.eigenvalues(An, B)
    assert ex.value.info == -5
    # a B that is not SPD: the positive info of the full device path for that B
    Bbad = B.copy(order="F"); Bbad[100, 100] = -5.0
    with pytest.raises(hip.SolverError) as ex:
        hip.eigenvalues(A, Bbad)
    ep_info = _full_device_info(lib, A, Bbad, n)
    assert ep_info > 0 and ex.value.info == ep_info
    # bad ranges
    for il, iu, code in [(0, 5, -3), (n + 1, n + 1, -3), (5, 4, -4), (1, n + 1, -4)]:
        with pytest.raises(hip.SolverError) as ex:
            hip.eigenvalues(A, B, il, iu)
        assert ex.value.info == code


def _full_device_info(lib, A, B, n):
    with _Dev(lib) as dev:
        dA, dB, dw, dZ = dev.alloc(n * n * 8), dev.alloc(n * n * 8), dev.alloc(n * 8), dev.alloc(n * n * 8)
        assert lib.ek_hip_memcpy_h2d(dA, A.ctypes.data, A.nbytes) == 0
        assert lib.ek_hip_memcpy_h2d(dB, B.ctypes.data, B.nbytes) == 0
        return lib.ek_hip_solve_device(1, n, n, dA, n, dB, n, dw, dZ, n, None, 0)


def test_values_speed_against_full_path_n16384(hip):
    """The values-only generalized solve at the headline order takes at most 0.6 x the full call (best of 3; measured
    0.45: DESIGN.md 9).  At N = 8192 the ratio is 0.65: the stages both calls share are a larger part of the call there,
    and the bisection is bound by the latency of its divisions."""
    lib = hip.load_library()
    n = 16384
    with _Dev(lib) as dev:
        dA, dB, dw, dZ = dev.alloc(n * n * 8), dev.alloc(n * n * 8), dev.alloc(n * 8), dev.alloc(n * n * 8)
        t_vals, t_full = [], []
        for _ in range(3):
            info, t = _values_device(lib, dA, dB, dw, n, True)
            assert info == 0
            t_vals.append(t)
            assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
            assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
            t0 = time.perf_counter()
            assert lib.ek_hip_solve_device(1, n, n, dA, n, dB, n, dw, dZ, n, None, 0) == 0
            t_full.append(time.perf_counter() - t0)
        assert min(t_vals) <= 0.6 * min(t_full), (t_vals, t_full)
