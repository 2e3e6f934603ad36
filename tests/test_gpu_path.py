"""GPU parity of the tridiagonal eigensolver, the back-transformation and the whole path,
through the C-ABI, against the CPU oracle, the reference's golden files and
oracle-independent identities.  Tolerances follow SURVEY.md 8(c):
    eigenvalues   max|l - l_oracle| <= N eps max|l|
    residual      max_j ||A v_j - l_j B v_j||_2 / ||A||_F <= 1e-14 sqrt(N/1024) (floor 1e-14)
    orthogonality ||V^T B V - I||_F (normalised as verifier.f90:310-325) <= 1e-11
"""
import os

import numpy as np
import pytest

from eigenkernel_amd import read_matrix_file
from eigenkernel_amd.verifier import eval_orthogonality, eval_residual_norm, get_ipratios

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16


def _check_pairs(A, B, w, Z, n_vec=None):
    n = A.shape[0]
    n_vec = n if n_vec is None else n_vec
    a_norm, ave, mx = eval_residual_norm(A, w[:n_vec], Z[:, :n_vec], B)
    orth = eval_orthogonality(Z[:, :n_vec], B)
    assert mx <= 1e-14 * max(1.0, np.sqrt(n / 1024.0)), mx
    assert orth <= 1e-11, orth


def _tridiag(n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1)
    if kind == "wilkinson":          # W_n^+: pairs of nearly equal eigenvalues
        m = (n - 1) / 2.0
        return np.abs(np.arange(n) - m), np.ones(n - 1)
    if kind == "toeplitz":           # 1-2-1: known spectrum 2 - 2 cos(k pi/(n+1))
        return 2.0 * np.ones(n), -np.ones(n - 1)
    if kind == "glued":              # weakly coupled identical blocks: heavy deflation
        d = np.tile(np.arange(1.0, 11.0), n // 10 + 1)[:n]
        e = np.ones(n - 1) * 0.5
        e[9::10] = 1e-9
        return d, e
    if kind == "zero_offdiag":       # already diagonal, unsorted
        return rng.uniform(-1, 1, n), np.zeros(n - 1)
    if kind == "identity":
        return np.ones(n), np.zeros(n - 1)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "wilkinson", "toeplitz", "glued", "zero_offdiag", "identity"])
@pytest.mark.parametrize("n", [1, 2, 21, 32, 33, 64, 100, 257, 600])
def test_stedc_matches_oracle(hip, oracle, n, kind):
    if n == 1:
        d, e = np.array([0.7]), np.zeros(0)
    else:
        d, e = _tridiag(n, n, kind)
    w_or, Z_or = oracle.stedc(d, e)
    w, Z, info = hip.stedc(d, e)
    assert info == 0
    T = np.diag(d) + np.diag(e, -1) + np.diag(e, 1)
    scale = max(np.abs(T).max(), 1e-300)
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w_or).max() <= 4 * n * EPS * scale
    assert np.abs(T @ Z - Z * w).max() <= 32 * n * EPS * scale
    assert np.abs(Z.T @ Z - np.eye(n)).max() <= 32 * n * EPS
    if kind == "toeplitz" and n > 1:
        exact = 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
        assert np.abs(w - exact).max() <= 4 * n * EPS * 4


@pytest.mark.parametrize("n,ncols", [(2, 2), (5, 3), (64, 64), (129, 129), (130, 7), (300, 300), (515, 100)])
def test_ormtr_matches_oracle(hip, oracle, n, ncols):
    A = oracle.synth_matrix(n, 1)
    Ar, d, e, tau = oracle.sytrd_lower(A)
    Z = np.asfortranarray(np.random.default_rng(n).uniform(-1, 1, (n, ncols)))
    ref = oracle.ormtr_lower(Ar, tau, Z)
    got, info = hip.ormtr(Ar, tau, Z)
    assert info == 0
    assert np.abs(got - ref).max() <= 32 * n * EPS * np.abs(ref).max()


@pytest.mark.parametrize("n", [1, 2, 30, 100, 128, 257, 640, 1000])
def test_solve_standard_matches_oracle(hip, oracle, n):
    A = oracle.synth_matrix(n, 1)
    w_or, _, info_or, _ = oracle.solve(A)
    ep, _ = hip.eigen_solver("hip", A)
    w = ep.values
    assert np.abs(w - w_or).max() <= n * EPS * np.abs(w_or).max() * 4
    _check_pairs(A, None, w, ep.Vectors)


@pytest.mark.parametrize("n", [1, 2, 30, 100, 128, 257, 640, 1000])
def test_solve_generalized_matches_oracle(hip, oracle, n):
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    w_or, _, info_or, _ = oracle.solve(A, B)
    ep, _ = hip.eigen_solver("general_hip", A, B)
    w = ep.values
    assert np.abs(w - w_or).max() <= 4 * n * EPS * np.abs(w_or).max()
    _check_pairs(A, B, w, ep.Vectors)
    names = set(ep.stage_seconds)
    assert "reduce_generalized:pdpotrf" in names and "eigen_solver_scalapack_all:pdsytrd" in names


def test_golden_bnz30_generalized(hip, golden_dir):
    """config C1: the reference's own shipped case, -s general_scalapack (README.md:22)."""
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"))
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx"))
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    ipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    ep, _ = hip.eigen_solver("general_hip", A, B)
    assert np.abs(ep.values - ev).max() <= 1e-14          # golden has 16 digits
    _check_pairs(A.to_dense(), B.to_dense(), ep.values, ep.Vectors)
    got_ipr = get_ipratios(ep.Vectors, B.to_dense())
    # near-degenerate pairs (l2,l3 differ by 4e-9) make individual IPRs ill-conditioned: 1e-6
    assert np.abs(got_ipr - ipr).max() <= 1e-6


def test_golden_vcnt400_standard(hip, golden_dir):
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_A.mtx"))
    E = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_E.txt"))[:, 1]
    ep, _ = hip.eigen_solver("hip", A)
    assert np.abs(ep.values - E).max() <= 1e-12           # golden has 12 digits
    _check_pairs(A.to_dense(), None, ep.values, ep.Vectors)


@pytest.mark.parametrize("n,n_vec", [(100, 10), (300, 300), (640, 64)])
def test_select_arms(hip, oracle, n, n_vec):
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    w_or, _, _, _ = oracle.solve(A, B)
    ep, _ = hip.eigen_solver("general_hip_select", A, B, n_vec=n_vec)
    assert np.abs(ep.values[:n_vec] - w_or[:n_vec]).max() <= 4 * n * EPS * np.abs(w_or).max()
    _check_pairs(A, B, ep.values, ep.Vectors, n_vec)
    ep2, _ = hip.eigen_solver("hip_select", A, n_vec=n_vec)
    w2, _, _, _ = oracle.solve(A)
    assert np.abs(ep2.values[:n_vec] - w2[:n_vec]).max() <= 4 * n * EPS * np.abs(w2).max()


def test_not_positive_definite_B_aborts_like_reference(hip, oracle):
    """generalized_to_standard.f90:25-30: info(pdpotrf) != 0 -> terminate."""
    n = 150
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    B[70, 70] = -3.0
    _, info_or = oracle.potrf_lower(B)
    with pytest.raises(hip.SolverError) as ei:
        hip.eigen_solver("general_hip", A, B)
    assert ei.value.info == info_or == 71


def test_unknown_solver_and_missing_B(hip, oracle):
    A = oracle.synth_matrix(10, 1)
    with pytest.raises(ValueError):
        hip.eigen_solver("general_elpa1", A, A)     # out of scope arms are not silently accepted
    with pytest.raises(ValueError):
        hip.eigen_solver("general_hip", A)


def test_device_resident_solve_and_synth(hip, oracle):
    """bench.py's entry: inputs generated and solved in HBM; generator is bit-equal to the oracle's."""
    import ctypes
    lib = hip.load_library()
    n = 384
    nn = n * n * 8
    ptrs = [ctypes.c_void_p() for _ in range(4)]
    for p, sz in zip(ptrs, (nn, nn, nn, n * 8)):
        assert lib.ek_hip_malloc(ctypes.byref(p), sz) == 0
    dA, dB, dZ, dw = ptrs
    assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
    assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
    hA = np.zeros((n, n), order="F")
    lib.ek_hip_memcpy_d2h(hA.ctypes.data, dA, nn)
    assert np.array_equal(hA, oracle.synth_matrix(n, 1))
    st = np.zeros(8)
    info = lib.ek_hip_solve_device(1, n, n, dA, n, dB, n, dw, dZ, n,
                                   st.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 8)
    assert info == 0
    w = np.zeros(n); Z = np.zeros((n, n), order="F")
    lib.ek_hip_memcpy_d2h(w.ctypes.data, dw, n * 8)
    lib.ek_hip_memcpy_d2h(Z.ctypes.data, dZ, nn)
    A = oracle.synth_matrix(n, 1); B = oracle.synth_matrix(n, 2)
    w_or, _, _, _ = oracle.solve(A, B)
    assert np.abs(w - w_or).max() <= 4 * n * EPS * np.abs(w_or).max()
    _check_pairs(A, B, w, Z)
    assert st[:7].sum() > 0
    for p in ptrs:
        lib.ek_hip_free(p)


def test_bench_dumps_the_eigenpairs_of_its_last_timed_step(oracle, tmp_path):
    """`bench.py --dump-outputs DIR` on one GPU: the line counts exactly --steps timed solves, and DIR holds the
    eigenvalues and (all of them fit at this order) the eigenvectors of the seeded pencil, in column order."""
    import json
    import subprocess
    import sys
    import scipy.linalg as sl
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 1024
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "bench.py"), "--gpus", "1",
                          "--order", str(n), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-host-path",
                          "--no-other-configs", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1
    w = np.load(tmp_path / "out" / "eigenvalues.npy")
    Z = np.load(tmp_path / "out" / "eigenvectors.npy")
    assert np.array_equal(np.load(tmp_path / "out" / "eigenvector_index.npy"), np.arange(n))
    assert w.dtype == Z.dtype == np.float64 and w.shape == (n,) and Z.shape == (n, n)
    A, B = oracle.synth_matrix(n, 1), oracle.synth_matrix(n, 2)
    w_ref = sl.eigh(A, B, eigvals_only=True)
    assert np.abs(w - w_ref).max() <= 4 * n * EPS * np.abs(w_ref).max()
    _check_pairs(A, B, w, Z)


def test_bench_leaves_the_extras_to_full():
    """A plain `bench.py` run times its steps and prints the line, nothing else: the parity check, the live GEMM ceiling
    of the roofline, the step on host arrays and the CPU baseline run with --full only (the CPU baseline is left out
    here: it takes minutes)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(*extra):
        out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "bench.py"), "--gpus", "1",
                              "--order", "1024", "--steps", "2", "--warmup", "1"] + list(extra),
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])

    plain = run()
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["roofline"]["launches"] > 0 and plain["roofline"]["measured_mfma_ceiling_tflops"] is None
    assert plain["parity"] is None
    assert not {"value_incl_copies", "other_configs", "cpu_baseline"} & set(plain), sorted(plain)
    full = run("--full", "--no-cpu-baseline")
    assert full["steps"] == 2 and "cpu_baseline" not in full
    assert full["parity"]["residual_norm_max"] <= full["parity"]["bounds"]["residual_norm_max"]
    assert full["parity"]["orthogonality"] <= full["parity"]["bounds"]["orthogonality"]
    assert full["roofline"]["measured_mfma_ceiling_tflops"] > 0
    assert "value_incl_copies" in full


@pytest.mark.parametrize("name,n,gep", [("gep_n256_np4", 256, True), ("sep_n256_np4", 256, False),
                                         ("gep_n1000_np4", 1000, True)])
def test_hip_vs_scalapack_goldens(hip, oracle, golden_dir, name, n, gep):
    """The HIP path against eigenvalues of the reference's ScaLAPACK path on the same inputs
    (fixtures from tests/golden/make_scalapack_goldens.sh). Tolerance N*eps*max|lambda|."""
    w_ref = np.loadtxt(os.path.join(golden_dir, "scalapack_synth_%s.txt" % name))
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    ep, _ = hip.eigen_solver("general_hip" if gep else "hip", A, B)
    assert np.abs(ep.values - w_ref).max() <= n * EPS * np.abs(w_ref).max()


@pytest.mark.parametrize("n,gep", [(30, True), (200, True), (333, False)])
def test_gpu_verifier_and_ipr_match_host_mirror(hip, oracle, n, gep):
    """residual / orthogonality / IPR computed on the GPU reproduce
    the reference's normalisations (host mirror = eigenkernel_amd/verifier.py)."""
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    w, Z, info, _ = oracle.solve(A, B)
    # make the check non-trivial: perturb one vector
    Zp = Z.copy(); Zp[:, 3] += 1e-6 * Z[:, 5]
    a_h, ave_h, mx_h = eval_residual_norm(A, w, Zp, B)
    a_g, ave_g, mx_g = hip.eval_residual_norm(A, w, Zp, B)
    assert abs(a_g - a_h) <= 1e-13 * a_h
    assert abs(ave_g - ave_h) <= 1e-10 * ave_h and abs(mx_g - mx_h) <= 1e-10 * mx_h
    o_h = eval_orthogonality(Zp, B)
    o_g = hip.eval_orthogonality(Zp, B)
    assert abs(o_g - o_h) <= 1e-9 * o_h
    o_h2 = eval_orthogonality(Zp, B, 2, 20)
    o_g2 = hip.eval_orthogonality(Zp, B, 2, 20)
    assert abs(o_g2 - o_h2) <= 1e-9 * o_h2
    i_h = get_ipratios(Zp, B)
    i_g = hip.get_ipratios(Zp, B)
    assert np.abs(i_g - i_h).max() <= 1e-12 * np.abs(i_h).max()
    # partial check (n_check < n), as `-c <n>` does
    a2, ave2, mx2 = hip.eval_residual_norm(A, w, Zp, B, n_check=7)
    _, ave2h, mx2h = eval_residual_norm(A, w[:7], Zp[:, :7], B)
    assert abs(ave2 - ave2h) <= 1e-10 * ave2h and abs(mx2 - mx2h) <= 1e-10 * mx2h


def test_gpu_ipr_matches_reference_golden(hip, golden_dir):
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"))
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx"))
    ipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    ep, _ = hip.eigen_solver("general_hip", A, B)
    got = hip.get_ipratios(ep.Vectors, B.to_dense())
    assert np.abs(got - ipr).max() <= 1e-6


def test_fortran_host_end_to_end(tmp_path, golden_dir):
    """The ISO_C_BINDING boundary for real: the flang-built host (host/eigenkernel_hip_app.f90,
    same CLI / file contract as the reference: SURVEY.md App. C) solves the shipped BNZ30 pair
    through libek_hip.so and reproduces the reference's golden eigenvalue and IPR files."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "eigenkernel_hip_app")
    if not os.path.exists(exe):
        flang = "/opt/rocm/lib/llvm/bin/flang"
        assert os.path.exists(flang), "flang missing: cannot build the Fortran host"
        subprocess.check_call(["make", "-C", os.path.join(root, "host")])
    out = subprocess.run([exe, "-s", "general_hip", "-c", "-1", "-t", "1,30", "-p", "1-2,30", "-d", str(tmp_path),
                          os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"),
                          os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    ev = np.loadtxt(tmp_path / "eigenvalues.dat")
    gold = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))
    assert ev.shape == gold.shape and np.array_equal(ev[:, 0], gold[:, 0])
    assert np.abs(ev[:, 1] - gold[:, 1]).max() <= 1e-14
    # the file format itself is the reference's: (I8, " ", E26.16e3)
    first = open(tmp_path / "eigenvalues.dat").readline().rstrip("\n")
    gfirst = open(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt")).readline().rstrip("\n")
    assert len(first) == len(gfirst) and first[:9] == gfirst[:9] and first[-5:] == gfirst[-5:]
    ipr = np.loadtxt(tmp_path / "ipratios.dat")[:, 1]
    gipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    assert np.abs(ipr - gipr).max() <= 1e-6
    txt = out.stdout
    res_max = float([l for l in txt.splitlines() if l.startswith("residual norm (max):")][0].split(":")[1])
    orth = float([l for l in txt.splitlines() if l.startswith("orthogonality criterion:")][0].split(":")[1])
    # SURVEY.md section 4 probe of the reference build on this case: 4.8e-16 and 5e-15
    assert res_max <= 2e-15 and orth <= 1e-13
    log = json.load(open(tmp_path / "log.json"))
    assert set(log) == {"setting", "events"} and log["setting"]["dimension"] == 30
    names = {e["name"] for e in log["events"]}
    assert {"reduce_generalized:pdpotrf", "eigen_solver_scalapack_all:pdsytrd", "recovery_generalized"} <= names
    # eigenvector files (-p 1-2,30): `i j value` lines, B-normalised vectors
    vec = np.loadtxt(tmp_path / "00000030.dat")
    assert vec.shape == (30, 3) and np.array_equal(vec[:, 0], np.arange(1, 31)) and np.all(vec[:, 1] == 30)
    Bd = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense()
    assert abs(vec[:, 2] @ Bd @ vec[:, 2] - 1.0) <= 1e-13
    assert (tmp_path / "00000001.dat").exists() and (tmp_path / "00000002.dat").exists()
    assert not (tmp_path / "00000003.dat").exists()
    # error contract: unknown solver -> "[Error] ..." on stderr, non-zero exit (processes.f90:133-138)
    bad = subprocess.run([exe, "-s", "general_elpa1", "a.mtx", "b.mtx"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and bad.stderr.startswith("[Error]")


def test_fortran_host_at_a_baseline_size(tmp_path, golden_dir):
    """BASELINE config C2 through the reference-language side of the boundary: the flang-built host
    makes the SURVEY.md 8(d) matrix with `--synthetic 4096`, solves it with `-s hip`, runs the
    reference's checks (-c -1 -t 1,4096) and writes eigenvalues.dat; the values are held to the
    reference's library path (ScaLAPACK fixture) within N eps max|lambda|."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "eigenkernel_hip_app")
    if not os.path.exists(exe):
        assert os.path.exists("/opt/rocm/lib/llvm/bin/flang"), "flang missing: cannot build the Fortran host"
        subprocess.check_call(["make", "-C", os.path.join(root, "host")])
    n = 4096
    out = subprocess.run([exe, "-s", "hip", "--synthetic", str(n), "-c", "-1", "-t", "1,%d" % n],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    ev = np.loadtxt(tmp_path / "eigenvalues.dat")
    assert ev.shape == (n, 2) and np.array_equal(ev[:, 0], np.arange(1, n + 1))
    w_ref = np.loadtxt(os.path.join(golden_dir, "scalapack_synth_sep_n4096_np8.txt"))
    assert np.abs(ev[:, 1] - w_ref).max() <= n * EPS * np.abs(w_ref).max()
    txt = out.stdout
    res_max = float([l for l in txt.splitlines() if l.startswith("residual norm (max):")][0].split(":")[1])
    orth = float([l for l in txt.splitlines() if l.startswith("orthogonality criterion:")][0].split(":")[1])
    assert res_max <= 2e-14 and orth <= 1e-11
    log = json.load(open(tmp_path / "log.json"))
    assert log["setting"]["dimension"] == n
    assert "eigen_solver_scalapack_all:pdsytrd" in {e["name"] for e in log["events"]}
    # --synthetic and matrix files exclude each other; the generalized pair comes with general_hip
    bad = subprocess.run([exe, "-s", "hip", "--synthetic", "64", "a.mtx"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and bad.stderr.startswith("[Error]")
    gen = subprocess.run([exe, "-s", "general_hip", "--synthetic", "300", "-c", "-1"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert gen.returncode == 0, gen.stderr
    assert np.loadtxt(tmp_path / "eigenvalues.dat").shape == (300, 2)


@pytest.mark.parametrize("n,gep", [(2048, True), (4096, False)])
def test_large_sizes_through_invariants(hip, n, gep):
    """Sizes the CPU oracle cannot reach in seconds: parity through size-independent
    properties evaluated on the GPU (residual, B-orthogonality, ordering, trace identities)."""
    import ctypes
    lib = hip.load_library()
    nn = n * n * 8
    ptrs = [ctypes.c_void_p() for _ in range(6)]
    for p, sz in zip(ptrs, (nn, nn, nn, n * 8, nn, nn)):
        assert lib.ek_hip_malloc(ctypes.byref(p), sz) == 0
    dA, dB, dZ, dw, dA0, dB0 = ptrs
    for dst in (dA, dA0):
        assert lib.ek_hip_synth_matrix_device(n, 1, dst, n) == 0
    for dst in (dB, dB0):
        assert lib.ek_hip_synth_matrix_device(n, 2, dst, n) == 0
    info = lib.ek_hip_solve_device(1 if gep else 0, n, n, dA, n, dB if gep else None, n, dw, dZ, n, None, 0)
    assert info == 0
    an, ave, mx, orth = (ctypes.c_double(0) for _ in range(4))
    assert lib.ek_hip_residual_device(1 if gep else 0, n, n, dA0, n, dB0 if gep else None, n, dw, dZ, n,
                                      ctypes.byref(an), ctypes.byref(ave), ctypes.byref(mx)) == 0
    assert lib.ek_hip_orthogonality_device(1 if gep else 0, n, 1, n, dB0 if gep else None, n, dZ, n,
                                           ctypes.byref(orth)) == 0
    assert mx.value <= 1e-14 * max(1.0, np.sqrt(n / 1024.0)), mx.value
    assert orth.value <= 1e-11, orth.value
    w = np.zeros(n)
    lib.ek_hip_memcpy_d2h(w.ctypes.data, dw, n * 8)
    assert np.all(np.diff(w) >= 0)
    if not gep:   # trace(A) = sum of eigenvalues; the generator's diagonal is 2 + u/sqrt(n)
        hA = np.zeros((n, n), order="F")
        lib.ek_hip_memcpy_d2h(hA.ctypes.data, dA0, nn)
        assert abs(w.sum() - np.trace(hA)) <= 64 * n * EPS * np.abs(w).sum()
        assert abs((w ** 2).sum() - (hA ** 2).sum()) <= 64 * n * EPS * (w ** 2).sum()
    for p in ptrs:
        lib.ek_hip_free(p)


@pytest.mark.parametrize("kind", ["zero", "identity", "diagonal", "scaled_up", "scaled_down", "negative",
                                  "rank_one", "arrowhead", "repeated_blocks"])
@pytest.mark.parametrize("n", [5, 64, 200])
def test_degenerate_inputs(hip, oracle, n, kind):
    """Corner paths of the reduction (tau = 0 reflectors, already-tridiagonal input), of the
    D&C (total deflation, multiple eigenvalues) and scaling robustness, against the oracle."""
    rng = np.random.default_rng(n)
    if kind == "zero":
        A = np.zeros((n, n))
    elif kind == "identity":
        A = np.eye(n)
    elif kind == "diagonal":
        A = np.diag(rng.uniform(-1, 1, n))
    elif kind == "scaled_up":
        A = oracle.synth_matrix(n, 1) * 1e8
    elif kind == "scaled_down":
        A = oracle.synth_matrix(n, 1) * 1e-8
    elif kind == "negative":
        A = -oracle.synth_matrix(n, 1)
    elif kind == "rank_one":
        u = rng.uniform(-1, 1, n)
        A = np.outer(u, u)
    elif kind == "arrowhead":
        A = np.diag(rng.uniform(1, 2, n)); A[:, 0] = A[0, :] = rng.uniform(-1, 1, n); A[0, 0] = 3.0
    else:  # repeated_blocks: many exactly repeated eigenvalues
        blk = oracle.synth_matrix(5, 3)
        A = np.kron(np.eye(n // 5 + 1), blk)[:n, :n]
    A = np.asfortranarray(A)
    scale = max(np.abs(A).max(), 1e-300)
    # standard problem
    w_or, _, info_or, _ = oracle.solve(A)
    ep, _ = hip.eigen_solver("hip", A)
    assert info_or == 0
    assert np.abs(ep.values - w_or).max() <= 8 * n * EPS * max(np.abs(w_or).max(), scale)
    Z = ep.Vectors
    assert np.abs(A @ Z - Z * ep.values).max() <= 64 * n * EPS * scale
    assert np.abs(Z.T @ Z - np.eye(n)).max() <= 64 * n * EPS
    # generalized problem with a well conditioned B
    B = oracle.synth_matrix(n, 2)
    w_or, _, info_or, _ = oracle.solve(A, B)
    ep, _ = hip.eigen_solver("general_hip", A, B)
    assert np.abs(ep.values - w_or).max() <= 8 * n * EPS * max(np.abs(w_or).max(), scale)
    Z = ep.Vectors
    assert np.abs(A @ Z - (B @ Z) * ep.values).max() <= 256 * n * EPS * scale
    assert np.abs(Z.T @ B @ Z - np.eye(n)).max() <= 256 * n * EPS


def test_ill_conditioned_B(hip, oracle):
    """cond(B) ~ 1e8: both paths lose the same digits; eigenvalues agree to cond(B)*eps."""
    n = 120
    A = oracle.synth_matrix(n, 1)
    Q, _ = np.linalg.qr(np.random.default_rng(1).normal(size=(n, n)))
    B = np.asfortranarray((Q * np.logspace(0, -8, n)) @ Q.T)
    B = 0.5 * (B + B.T)
    w_or, _, info_or, _ = oracle.solve(A, B)
    ep, _ = hip.eigen_solver("general_hip", A, B)
    assert info_or == 0
    assert np.abs(ep.values - w_or).max() <= 1e-5 * np.abs(w_or).max()
    Z = ep.Vectors
    assert np.abs(Z.T @ B @ Z - np.eye(n)).max() <= 1e-6


@pytest.mark.parametrize("scale", [1e200, 1e-200, 1e150, 1e-160])
def test_extreme_scaling_of_A(hip, oracle, scale):
    """Entries whose squares over/underflow: the solve rescales A like DSYEV does (the
    reference's PDSYTRD survives through PDNRM2's scaled sum of squares)."""
    n = 150
    A0 = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    w0, _, _, _ = oracle.solve(A0, B)
    ep, _ = hip.eigen_solver("general_hip", A0 * scale, B)
    assert np.all(np.isfinite(ep.values))
    assert np.abs(ep.values / scale - w0).max() <= 8 * n * EPS * np.abs(w0).max()
    Z = ep.Vectors
    assert np.abs(Z.T @ B @ Z - np.eye(n)).max() <= 256 * n * EPS
    ep2, _ = hip.eigen_solver("hip", A0 * scale)
    w1, _, _, _ = oracle.solve(A0)
    assert np.abs(ep2.values / scale - w1).max() <= 8 * n * EPS * np.abs(w1).max()


def test_non_finite_inputs_are_rejected_not_crashed(hip, oracle):
    """NaN / Inf in A -> info = -4 (illegal value); NaN in B -> the Cholesky reports the pivot.
    The process must survive (the reference would hand garbage to ScaLAPACK, not crash)."""
    n = 130
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2)
    for bad in (np.nan, np.inf, -np.inf):
        Ab = A.copy(); Ab[70, 3] = bad; Ab[3, 70] = bad
        with pytest.raises(hip.SolverError) as ei:
            hip.eigen_solver("general_hip", Ab, B)
        assert ei.value.info == -4
        with pytest.raises(hip.SolverError) as ei:
            hip.eigen_solver("hip", Ab)
        assert ei.value.info == -4
    Bb = B.copy(); Bb[40, 40] = np.nan
    with pytest.raises(hip.SolverError) as ei:
        hip.eigen_solver("general_hip", A, Bb)
    assert ei.value.info == 41
    # and the library is still healthy afterwards
    ep, _ = hip.eigen_solver("general_hip", A, B)
    w_or, _, _, _ = oracle.solve(A, B)
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * np.abs(w_or).max()


def test_descriptor_block_size_is_layout_only_on_1x1_grid(hip, golden_dir):
    """BNZ30 on the reference's 2x2 grid runs with NB = 15 (block-shrink rule,
    distribute_matrix.f90:114-120); on the 1x1 grid any NB describes the same column-major
    array, so the result must not depend on it (`--block-size`, solver_main.f90:44-46)."""
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"))
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx"))
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    ref = None
    for nb in (None, 15, 1, 7, 64):
        ep, _ = hip.eigen_solver("general_hip", A, B, block_size=nb)
        assert np.abs(ep.values - ev).max() <= 1e-14
        assert ep.desc[4] == (min(nb or 64, 30))
        if ref is None:
            ref = ep.Vectors.copy()
        else:
            assert np.array_equal(ep.Vectors, ref)     # bit-identical: NB never reaches a kernel


def test_bitwise_reproducible(hip, oracle):
    """No atomics, fixed reduction orders: two solves of the same input give identical bits."""
    n = 700
    A = oracle.synth_matrix(n, 1); B = oracle.synth_matrix(n, 2)
    ep1, _ = hip.eigen_solver("general_hip", A, B)
    ep2, _ = hip.eigen_solver("general_hip", A, B)
    assert np.array_equal(ep1.values, ep2.values)
    assert np.array_equal(ep1.Vectors, ep2.Vectors)


# ----------------------------------------------------------------------------- process grids
# One GPU plays every rank of the grid in turn ("virtual ranks"): each call is exactly what
# rank (myrow, mycol) would issue on its own GPU.  The pieces must assemble to the 1x1 result.
@pytest.mark.parametrize("n,grid,nb,gep,n_vec", [
    (300, (1, 4), 64, True, None),       # block-column cyclic, ragged last block
    (256, (2, 2), 64, True, None),       # layout_procs(4)
    (515, (2, 4), 64, False, None),      # layout_procs(8), standard problem, odd order
    (200, (1, 3), 200, True, None),      # NB larger than n/P: shrink rule of setup_distributed_matrix
    (640, (1, 8), 32, True, 100),        # *_select: only columns < n_vec, some ranks own few
    (30, (2, 2), 64, True, None),        # config 1 of the reference: N=30 on 4 ranks -> NB=15
])
def test_process_grid_replicated_mode(hip, oracle, n, grid, nb, gep, n_vec):
    from eigenkernel_amd import descriptor as d
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    name = ("general_hip" if gep else "hip") + ("_select" if n_vec else "")
    ref, _ = hip.eigen_solver(name, A, B, n_vec=n_vec)
    k = n_vec or n
    nprow, npcol = grid
    pieces, nb_used = {}, None
    for rank in range(nprow * npcol):
        _, _, myrow, mycol = d.make_process_grid(rank, nprow * npcol, nprow, npcol)
        proc = hip.Process(my_rank=rank, n_procs=nprow * npcol, n_procs_row=nprow, n_procs_col=npcol,
                           my_proc_row=myrow, my_proc_col=mycol)
        ep, _ = hip.eigen_solver(name, A, B, n_vec=n_vec, block_size=nb, proc=proc)
        assert np.array_equal(ep.values, ref.values)           # replicated, bitwise
        nb_used = int(ep.desc[d.BLOCK_ROW_])
        assert ep.desc[d.LOCAL_ROWS_] == max(1, d.numroc(n, nb_used, myrow, 0, nprow))
        pieces[(myrow, mycol)] = ep.Vectors
    assert nb_used == min(nb, max(min(n // nprow, n // npcol), 1))   # distribute_matrix.f90:114-120
    Zg = d.assemble_global(pieces, n, n, nb_used, nprow, npcol)
    # every rank back-transforms its own columns with the same K order: identical bits expected;
    # the tolerance is only the fallback statement of parity
    if not np.array_equal(Zg[:, :k], ref.Vectors[:, :k]):
        assert np.abs(Zg[:, :k] - ref.Vectors[:, :k]).max() <= 1e-13
    _check_pairs(A, B, ref.values, Zg, k)


def test_process_grid_argument_errors(hip, oracle):
    from eigenkernel_amd import descriptor as d
    lib = hip.load_library()
    n = 64
    A = oracle.synth_matrix(n, 1)
    w = np.zeros(n)
    desc, Z = d.setup_distributed_matrix(n, n, 1, 2, 0, 1)
    P, I = hip._P, hip._I
    call = lambda *g: lib.ek_hip_solve_replicated(0, n, n, P(A.copy(order="F")), n, None, n, P(w), P(Z), I(desc), *g, None, 0)
    assert call(0, 2, 0, 0) == -11
    assert call(1, 0, 0, 0) == -12
    assert call(1, 2, 1, 0) == -13
    assert call(1, 2, 0, 2) == -14
    bad = desc.copy(); bad[d.LOCAL_ROWS_] = n - 1
    assert lib.ek_hip_solve_replicated(0, n, n, P(A.copy(order="F")), n, None, n, P(w), P(Z), I(bad), 1, 2, 0, 1, None, 0) == -1009
    assert lib.ek_hip_solve_replicated(0, n, n, P(A.copy(order="F")), n - 1, None, n, P(w), P(Z), I(desc), 1, 2, 0, 1, None, 0) == -5


@pytest.mark.parametrize("n,grid,nb,gep,n_vec", [
    (30, (2, 2), 64, True, None),        # config 1: N=30, np=4 -> NB=15, the reference's own CPU case
    (300, (2, 4), 64, True, None),
    (257, (1, 2), 32, False, None),
    (256, (2, 2), 64, True, 40),
])
def test_process_grid_distributed_inputs(hip, oracle, n, grid, nb, gep, n_vec):
    """ek_hip_solve with the reference's own data contract on an nprow x npcol grid: block-cyclic
    pieces of A, B in, pieces of Z / reflectors / L out; the exchange goes through the host hook."""
    from eigenkernel_amd import descriptor as d
    from test_host_logic import virtual_allgatherv
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if gep else None
    name = ("general_hip" if gep else "hip") + ("_select" if n_vec else "")
    ref, _ = hip.eigen_solver(name, A, B, n_vec=n_vec)
    # what the 1x1 call leaves in A (reflectors) and B (L): run it through the C-ABI once more
    lib = hip.load_library()
    desc1, A1 = d.setup_distributed_matrix(n, n); A1[:, :] = A
    B1 = None
    if gep:
        _, B1 = d.setup_distributed_matrix(n, n); B1[:, :] = B
    _, Z1 = d.setup_distributed_matrix(n, n)
    w1 = np.zeros(n)
    k = n_vec or n
    assert lib.ek_hip_solve(1 if gep else 0, n, k, hip._P(A1), hip._I(desc1), hip._P(B1) if gep else None,
                            hip._I(desc1) if gep else None, hip._P(w1), hip._P(Z1), hip._I(desc1),
                            1, 1, 0, 0, None, 0) == 0
    nprow, npcol = grid
    nbu = int(d.setup_distributed_matrix(n, n, nprow, npcol, 0, 0, block_size=nb)[0][d.BLOCK_ROW_])
    hook = virtual_allgatherv([A, B] if gep else [A], nbu, nprow, npcol)
    hip.set_allgatherv(hook)
    try:
        Zp, Ap, Bp = {}, {}, {}
        for rank in range(nprow * npcol):
            hook.state["rank"] = rank
            _, _, myrow, mycol = d.make_process_grid(rank, nprow * npcol, nprow, npcol)
            proc = hip.Process(rank, nprow * npcol, 0, nprow, npcol, myrow, mycol)
            ep, _ = hip.eigen_solver(name, A, B, n_vec=n_vec, block_size=nb, proc=proc, inputs="distributed")
            assert np.array_equal(ep.values, ref.values)
            assert ep.stage_seconds["eigen_solver_scalapack_all:gather1"] > 0.0
            Zp[(myrow, mycol)] = ep.Vectors; Ap[(myrow, mycol)] = ep.A_loc
            if gep:
                Bp[(myrow, mycol)] = ep.B_loc
        Zg = d.assemble_global(Zp, n, n, nbu, nprow, npcol)
        if not np.array_equal(Zg[:, :k], ref.Vectors[:, :k]):
            assert np.abs(Zg[:, :k] - ref.Vectors[:, :k]).max() <= 1e-13
        _check_pairs(A, B, ref.values, Zg, k)
        # reflectors, d, e (uplo = 'L': the 1 x 1 call leaves the caller's upper triangle alone, a grid cell's piece comes
        # back whole)
        Ag = d.assemble_global(Ap, n, n, nbu, nprow, npcol)
        assert np.array_equal(np.tril(Ag), np.tril(A1))
        # (include/ek_hip.h: above the global diagonal a grid caller finds unspecified FINITE values)
        assert np.isfinite(Ag).all()
        if gep:
            Bg = d.assemble_global(Bp, n, n, nbu, nprow, npcol)
            assert np.array_equal(np.tril(Bg), np.tril(B1))  # L
            assert np.isfinite(Bg).all()
    finally:
        hip.set_allgatherv(None)


@pytest.mark.parametrize("inputs", ["replicated", "distributed"])
def test_golden_bnz30_on_the_reference_grid(hip, golden_dir, inputs):
    """config C1 as the reference runs it: `mpirun -np 4 ... -s general_scalapack` -> 2x2 grid,
    NB shrunk to 15 (distribute_matrix.f90:114-120); every rank's call is played on the one GPU."""
    from eigenkernel_amd import descriptor as d
    from test_host_logic import virtual_allgatherv
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx"))
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx"))
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    ipr = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
    nprow, npcol = d.layout_procs(4)
    assert (nprow, npcol) == (2, 2)
    hook = virtual_allgatherv([A.to_dense(), B.to_dense()], 15, nprow, npcol)
    hip.set_allgatherv(hook if inputs == "distributed" else None)
    try:
        pieces = {}
        for rank in range(4):
            hook.state["rank"] = rank
            _, _, myrow, mycol = d.make_process_grid(rank, 4)
            ep, _ = hip.eigen_solver("general_hip", A, B, proc=hip.Process(rank, 4, 0, nprow, npcol, myrow, mycol),
                                     inputs=inputs)
            assert int(ep.desc[d.BLOCK_ROW_]) == 15 and ep.Vectors.shape == (15, 15)
            assert np.abs(ep.values - ev).max() <= 1e-14
            pieces[(myrow, mycol)] = ep.Vectors
        Z = d.assemble_global(pieces, 30, 30, 15, nprow, npcol)
        _check_pairs(A.to_dense(), B.to_dense(), ev, Z)
        assert np.abs(get_ipratios(Z, B.to_dense()) - ipr).max() <= 1e-6
    finally:
        hip.set_allgatherv(None)


def test_no_eigenvectors_requested(hip, oracle):
    """n_vec = 0 (eigenvalues only) and grid cells that own no eigenvector column."""
    from eigenkernel_amd import descriptor as d
    lib = hip.load_library()
    n = 300
    A = oracle.synth_matrix(n, 1); B = oracle.synth_matrix(n, 2)
    ref, _ = hip.eigen_solver("general_hip", A, B)
    desc, Al = d.setup_distributed_matrix(n, n); Al[:, :] = A
    _, Bl = d.setup_distributed_matrix(n, n); Bl[:, :] = B
    _, Z = d.setup_distributed_matrix(n, n)
    w = np.zeros(n)
    assert lib.ek_hip_solve(1, n, 0, hip._P(Al), hip._I(desc), hip._P(Bl), hip._I(desc), hip._P(w), hip._P(Z),
                            hip._I(desc), 1, 1, 0, 0, None, 0) == 0
    assert np.array_equal(w, ref.values) and not Z.any()
    # 1 x 8 grid, NB = 64, n_vec = 100: process columns 2..7 own nothing
    for mycol in (1, 5):
        proc = hip.Process(mycol, 8, 0, 1, 8, 0, mycol)
        ep, _ = hip.eigen_solver("general_hip_select", A, B, n_vec=100, block_size=64, proc=proc)
        assert np.array_equal(ep.values, ref.values)
        own = d.local_indices(100, int(ep.desc[d.BLOCK_ROW_]), mycol, 8)
        if len(own):
            assert np.array_equal(ep.Vectors[:, :len(own)], ref.Vectors[:, own])
        else:
            assert not ep.Vectors.any()


@pytest.mark.parametrize("solver,n,n_vec", [("general_hip", 2304, 2304), ("hip", 2100, 2100), ("general_hip_select", 2304, 300)])
def test_staging_pipeline_of_the_host_path_changes_no_bit(hip, oracle, monkeypatch, solver, n, n_vec):
    """From order 2048 on ek_hip_solve overlaps its PCIe copies with the stages (B in first, A behind the Cholesky
    factorisation; L, the reflectors and Z out as they become final, Z in column slabs): eigenvalues, eigenvectors and
    the in-place results must be the bits of the serial staging (EK_HIP_PIPE_MIN=0), and pass the acceptance bounds."""
    from eigenkernel_amd.verifier import eval_orthogonality, eval_residual_norm
    A = oracle.synth_matrix(n, 1)
    Bm = oracle.synth_matrix(n, 2) if solver.startswith("general") else None
    monkeypatch.setenv("EK_HIP_PIPE_MIN", "0")
    ep0, _ = hip.eigen_solver(solver, A, Bm, n_vec=n_vec)
    monkeypatch.setenv("EK_HIP_PIPE_MIN", "1024")
    ep1, _ = hip.eigen_solver(solver, A, Bm, n_vec=n_vec)
    assert np.array_equal(ep0.values, ep1.values)
    assert np.array_equal(ep0.Vectors[:, :n_vec], ep1.Vectors[:, :n_vec])
    _, _, mx = eval_residual_norm(A, ep1.values[:n_vec], ep1.Vectors[:, :n_vec], Bm)
    assert mx <= 1e-14 * max(1.0, np.sqrt(n / 1024.0))
    assert eval_orthogonality(ep1.Vectors[:, :n_vec], Bm) <= 1e-11


@pytest.mark.parametrize("problem,n,n_vec,pipe_min", [(1, 2100, 2100, "0"), (1, 2100, 2100, "1024"), (0, 2304, 500, "1024"),
                                                      (1, 300, 300, "0")])
def test_caller_leading_dimensions_larger_than_the_order(hip, oracle, monkeypatch, problem, n, n_vec, pipe_min):
    """ScaLAPACK descriptors carry their own LLD (descriptor_parameters.f90:2-4): local arrays with LLD = n + 5, + 3 and
    + 7 for A, B and Z give the bits of the tightly packed call -- with the serial staging and with the pipeline (which
    moves lower triangles in trapezoid pieces) -- and the padding rows below row n come back untouched."""
    from eigenkernel_amd import descriptor as d
    lib = hip.load_library()
    monkeypatch.setenv("EK_HIP_PIPE_MIN", pipe_min)
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if problem == 1 else None

    def call(pa, pb, pz):
        la, lb, lz = n + pa, n + pb, n + pz
        Al = np.asfortranarray(np.full((la, n), 7.5)); Al[:n, :] = A
        Bl = None
        if B is not None:
            Bl = np.asfortranarray(np.full((lb, n), -3.25)); Bl[:n, :] = B
        Z = np.asfortranarray(np.full((lz, n), 1.125))
        w = np.zeros(n)
        da, db, dz = (d.descinit(n, n, n, n, 0, 0, 0, l) for l in (la, lb, lz))
        rc = lib.ek_hip_solve(problem, n, n_vec, hip._P(Al), hip._I(da), hip._P(Bl) if Bl is not None else None,
                              hip._I(db) if Bl is not None else None, hip._P(w), hip._P(Z), hip._I(dz), 1, 1, 0, 0, None, 0)
        assert rc == 0
        return Al, Bl, Z, w

    A0, B0, Z0, w0 = call(0, 0, 0)
    A1, B1, Z1, w1 = call(5, 3, 7)
    assert np.array_equal(w0, w1)
    assert np.array_equal(Z0[:, :n_vec], Z1[:n, :n_vec])
    assert np.array_equal(np.tril(A0), np.tril(A1[:n]))
    assert (A1[n:] == 7.5).all() and (Z1[n:] == 1.125).all()
    if B is not None:
        assert np.array_equal(np.tril(B0), np.tril(B1[:n]))
        assert (B1[n:] == -3.25).all()


@pytest.mark.parametrize("problem,n,pad,pipe_min", [(1, 2304, 0, "1024"), (1, 2100, 3, "1024"), (0, 3000, 0, "1024"),
                                                    (1, 2304, 0, "0"), (1, 700, 5, "0"), (0, 384, 0, "0")])
def test_upper_triangles_of_the_callers_arrays_are_left_alone(hip, oracle, monkeypatch, problem, n, pad, pipe_min):
    """uplo = 'L' (generalized_to_standard.f90:24,37, solver_scalapack_all.f90:59): PDPOTRF / PDSYTRD neither reference nor
    write the strictly upper triangles of A and B.  Here they hold a sentinel (a NaN with a payload) on entry; on a 1 x 1
    grid it must still be there, bit for bit, after ek_hip_solve -- through the pipeline (whose pieces are cut across the
    diagonal: the diagonal blocks of the way out go through a scratch) and through the serial staging -- and the
    results are those of clean symmetric inputs."""
    from eigenkernel_amd import descriptor as d
    lib = hip.load_library()
    monkeypatch.setenv("EK_HIP_PIPE_MIN", pipe_min)
    A = oracle.synth_matrix(n, 1)
    B = oracle.synth_matrix(n, 2) if problem == 1 else None
    sentinel = np.frombuffer(np.uint64(0x7FF8DEADBEEF1234).tobytes(), dtype=np.float64)[0]
    iu = np.triu_indices(n, 1)

    def call(marked):
        la = n + pad
        Al = np.asfortranarray(np.full((la, n), 7.5)); Al[:n, :] = A
        Bl = None
        if B is not None:
            Bl = np.asfortranarray(np.full((la, n), -3.25)); Bl[:n, :] = B
        if marked:
            Al[:n][iu] = sentinel
            if Bl is not None:
                Bl[:n][iu] = sentinel
        Z = np.asfortranarray(np.zeros((n, n)))
        w = np.zeros(n)
        da, dz = d.descinit(n, n, n, n, 0, 0, 0, la), d.descinit(n, n, n, n, 0, 0, 0, n)
        rc = lib.ek_hip_solve(problem, n, n, hip._P(Al), hip._I(da), hip._P(Bl) if Bl is not None else None,
                              hip._I(da) if Bl is not None else None, hip._P(w), hip._P(Z), hip._I(dz), 1, 1, 0, 0, None, 0)
        assert rc == 0
        return Al, Bl, Z, w

    A0, B0, Z0, w0 = call(False)
    A1, B1, Z1, w1 = call(True)
    assert np.array_equal(w0, w1) and np.array_equal(Z0, Z1)
    assert np.array_equal(np.tril(A0[:n]), np.tril(A1[:n]))
    want = np.full(len(iu[0]), sentinel).view(np.uint64)
    assert np.array_equal(A1[:n][iu].view(np.uint64), want)
    assert np.array_equal(A0[:n][iu], A[iu])                       # (clean inputs: the upper triangle is still the input's)
    if B is not None:
        assert np.array_equal(np.tril(B0[:n]), np.tril(B1[:n]))
        assert np.array_equal(B1[:n][iu].view(np.uint64), want)
        assert np.array_equal(B0[:n][iu], B[iu])
