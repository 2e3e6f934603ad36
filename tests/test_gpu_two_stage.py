"""GPU parity of the two-stage tridiagonalisation (dense -> band -> tridiagonal) that the whole-path
calls use for large orders in place of the one-stage PDSYTRD of solver_scalapack_all.f90:59 and the
PDORMTR of :115.  Stage level: oracle-independent identities at rounding level (orthogonal similarity,
band structure, spectrum); path level: the same oracle / ScaLAPACK-fixture / verifier bounds as the
one-stage path, with the two-stage form forced on at small orders so that the CPU
oracle can follow.  The full-size configurations run through it in tests/test_gpu_configs.py."""
import os

import numpy as np
import pytest

from eigenkernel_amd.verifier import eval_orthogonality, eval_residual_norm

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
B = 64


def _band_of(Ab):
    L = np.tril(Ab) - np.tril(Ab, -(B + 1))
    return L + np.tril(L, -1).T


def _q_from_reflectors(V, tau):
    n = V.shape[0]
    Q = np.eye(n)
    for j in range(n - 1, -1, -1):
        if tau[j] != 0.0:
            v = V[:, j]
            Q -= tau[j] * np.outer(v, v @ Q)
    return Q


def _random_band(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    M = np.tril(M) - np.tril(M, -(B + 1))
    return M + np.tril(M, -1).T


@pytest.mark.parametrize("n", [3, 64, 65, 66, 130, 200, 257, 258, 321, 449, 700, 1000])
def test_dense_to_band_is_an_orthogonal_similarity(hip, oracle, n):
    """Panels with >= 128 rows go through CholeskyQR2 + Householder reconstruction, the last ones (<= 127 rows)
    through the in-LDS Householder QR: both must give A = Q1 Bd Q1^T with Q1 orthogonal to rounding."""
    A = oracle.synth_matrix(n, 1)
    Ab, V, tau, flag = hip.sy2sb(A)
    assert flag == 0
    if n > B + 1:
        assert np.abs(np.tril(Ab, -(B + 1))).max() == 0.0          # nothing is left below the band
    Bd = _band_of(Ab)
    Q = _q_from_reflectors(V, tau)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 64 * n * EPS
    assert np.linalg.norm(Q.T @ A @ Q - Bd) <= 32 * n * EPS * np.linalg.norm(A)
    w0, w1 = np.linalg.eigvalsh(A), np.linalg.eigvalsh(Bd)
    assert np.abs(w0 - w1).max() <= 4 * n * EPS * np.abs(w0).max()
    # reflector j starts at row j + 64: zeros above, unit entry on it
    for j in range(0, max(n - B - 1, 0), 37):
        assert np.all(V[:j + B, j] == 0.0) and (tau[j] == 0.0 or V[j + B, j] == 1.0)


@pytest.mark.parametrize("n,kind", [(n, k) for k in ("synth", "graded", "band65", "parallel_columns") for n in (130, 193, 194, 257, 449)]
                         + [(1000, "synth"), (1000, "band65"), (1345, "synth")])
def test_dense_to_band_with_panels_in_pairs(hip, oracle, monkeypatch, n, kind):
    """From 5120 rows on the stage takes its panels in pairs: the second panel's Y = A V comes from the matrix the first
    panel has NOT yet updated plus two 64-wide corrections (DLATRD's rule), and one rank-256 update serves both.  Forced
    at every order here (EK_SY2SB_PAIR_MIN=1: every panel that has a successor is the first of a pair, so pairs also end
    on the in-LDS panels, on rescued panels and on the last panel): the same identities as the one-panel flow, and its
    spectrum."""
    rng = np.random.default_rng(n)
    A = oracle.synth_matrix(n, 1)
    if kind == "graded":
        s = 10.0 ** (-6.0 * np.arange(n) / n)
        A = A * s[:, None] * s[None, :]
    elif kind == "band65":
        M = np.tril(rng.standard_normal((n, n))); M = M - np.tril(M, -66); A = M + np.tril(M, -1).T
    elif kind == "parallel_columns":
        A[64:, 5] = A[64:, 4] * (1.0 + 1e-7); A[5, 64:] = A[64:, 5]
        if n > 200:
            A[140:, 70] = A[140:, 69] + 1e-6 * rng.standard_normal(n - 140); A[70, 140:] = A[140:, 70]
    monkeypatch.setenv("EK_SY2SB_PAIR_MIN", "0")
    Ab0, V0, tau0, flag0 = hip.sy2sb(A)
    monkeypatch.setenv("EK_SY2SB_PAIR_MIN", "1")
    Ab, V, tau, flag = hip.sy2sb(A)
    assert flag & 0xff == 0 and flag0 & 0xff == 0
    assert np.abs(np.tril(Ab, -(B + 1))).max() == 0.0
    Bd = _band_of(Ab)
    Q = _q_from_reflectors(V, tau)
    nrm = np.linalg.norm(A)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 64 * n * EPS
    assert np.linalg.norm(Q.T @ A @ Q - Bd) <= 32 * n * EPS * nrm
    w0, w1, w2 = np.linalg.eigvalsh(A), np.linalg.eigvalsh(Bd), np.linalg.eigvalsh(_band_of(Ab0))
    assert np.abs(w0 - w1).max() <= 4 * n * EPS * np.abs(w0).max()
    assert np.abs(w2 - w1).max() <= 4 * n * EPS * np.abs(w0).max()
    # the first panel of the stage is factored before anything is pending: same bits in both flows
    assert np.array_equal(V[:, :B], V0[:, :B]) and np.array_equal(tau[:B], tau0[:B])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 66, 100, 129, 200, 321, 640, 1000])
def test_band_to_tridiagonal_by_bulge_chasing(hip, n):
    Bd = _random_band(n, n)
    d, e, Q2, flag = hip.sb2st(Bd, np.eye(n))
    assert flag == 0
    T = np.diag(d) + (np.diag(e, 1) + np.diag(e, -1) if n > 1 else 0.0)
    nrm = max(np.linalg.norm(Bd), 1e-300)
    assert np.linalg.norm(Q2.T @ Q2 - np.eye(n)) <= 64 * n * EPS
    assert np.linalg.norm(Q2.T @ Bd @ Q2 - T) <= 32 * n * EPS * nrm
    w0, w1 = np.linalg.eigvalsh(Bd), np.linalg.eigvalsh(T)
    assert np.abs(w0 - w1).max() <= 4 * n * EPS * max(np.abs(w0).max(), 1e-300)


@pytest.mark.parametrize("kind", ["tridiagonal", "diagonal", "zero", "narrow_band", "block_diagonal"])
def test_band_to_tridiagonal_degenerate_bands(hip, kind):
    """tau = 0 reflectors, empty bulges, already tridiagonal input."""
    n = 300
    rng = np.random.default_rng(7)
    if kind == "tridiagonal":
        Bd = np.diag(rng.uniform(-1, 1, n)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    elif kind == "diagonal":
        Bd = np.diag(rng.uniform(-1, 1, n))
    elif kind == "zero":
        Bd = np.zeros((n, n))
    elif kind == "narrow_band":
        M = np.tril(rng.standard_normal((n, n))); M = M - np.tril(M, -8); Bd = M + np.tril(M, -1).T
    else:
        Bd = np.zeros((n, n))
        for i in range(0, n, 50):
            blk = rng.standard_normal((50, 50)); Bd[i:i + 50, i:i + 50] = blk + blk.T
    d, e, Q2, flag = hip.sb2st(Bd, np.eye(n))
    assert flag == 0
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    scale = max(np.linalg.norm(Bd), 1.0)
    assert np.linalg.norm(Q2.T @ Q2 - np.eye(n)) <= 64 * n * EPS
    assert np.linalg.norm(Q2.T @ Bd @ Q2 - T) <= 32 * n * EPS * scale


def test_narrow_band_whose_fill_decays_into_the_denormal_range(hip):
    """A bandwidth-5 matrix inside the 64-diagonal band: the fill decays geometrically across the band, columns of the
    bulges come to consist of entries around 1e-160 whose SQUARES are denormal; a reflector made from such a norm is
    not orthogonal (this input lost its spectrum at the 1e-2 level before reflector_of dropped such columns)."""
    from scipy.linalg import eigvalsh_tridiagonal
    n = 5000
    rng = np.random.default_rng(1)
    A = np.zeros((n, n), order="F")
    for dgn in range(5):
        v = rng.standard_normal(n - dgn)
        A[np.arange(dgn, n), np.arange(0, n - dgn)] = v
        A[np.arange(0, n - dgn), np.arange(dgn, n)] = v
    d, e, _, f = hip.sb2st(A)
    assert f == 0
    w_ref = np.linalg.eigvalsh(A)
    assert np.abs(eigvalsh_tridiagonal(d, e) - w_ref).max() <= 4 * n * EPS * np.abs(w_ref).max()


def test_bulge_chasing_is_bitwise_reproducible(hip):
    """The sweeps hand blocks to each other through agent-scope loads and stores guarded by progress
    words; a stale read would show up as run-to-run differences."""
    Bd = _random_band(777, 1)
    d0, e0, _, _ = hip.sb2st(Bd)
    for _ in range(4):
        d1, e1, _, f = hip.sb2st(Bd)
        assert f == 0 and np.array_equal(d0, d1) and np.array_equal(e0, e1)


@pytest.mark.parametrize("n", [130, 777, 1500])
def test_bulge_chasing_does_not_depend_on_the_width_of_the_pipeline(hip, n):
    """A sweep starts as soon as the previous sweep's task of the same index is complete and takes the 65 late
    numbers of the task after it from a mailbox line (ek_sb2st.hip): with 3 workgroups the pipeline is almost
    serial, with 7 or 40 its sweeps overtake each other's stores in other orders than at full width.  d, e and
    the applied Q2 must be the same bits every time (tools/chase_stress.py is the longer form)."""
    Bd = _random_band(n, n)
    Z0 = np.eye(n)[:, ::max(n // 16, 1)][:, :16].copy()
    ref = None
    try:
        for wgs in (None, 3, 7, 40, None):
            if wgs is None:
                os.environ.pop("EK_SB2ST_WGS", None)
            else:
                os.environ["EK_SB2ST_WGS"] = str(wgs)
            d, e, Z, f = hip.sb2st(Bd, Z0)
            assert f == 0
            if ref is None:
                ref = (d, e, Z)
                T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
                assert np.abs(np.linalg.eigvalsh(Bd) - np.linalg.eigvalsh(T)).max() <= 8 * n * EPS * np.abs(d).max()
            else:
                assert np.array_equal(ref[0], d) and np.array_equal(ref[1], e) and np.array_equal(ref[2], Z)
    finally:
        os.environ.pop("EK_SB2ST_WGS", None)


@pytest.mark.parametrize("n", [3, 4, 66, 130, 193, 777, 1500, 4200])
def test_both_bulge_chasing_kernels_give_the_same_bits(hip, n):
    """ek_sb2st.hip has two kernels for the chase: positions of the band held in registers, sweeps passing
    through them by mail (the default), and sweeps walking through memory (the fall-back).
    They share the arithmetic of a task, so d, e, the reflectors (seen through the applied Q2) must agree bit
    for bit -- which also shows that no hand-off of either protocol delivered a stale or a misplaced number.
    (The kernel is chosen through sb2st_lower's chase_mode, by ek_hip_debug_sb2st_stage: the switch EK_SB2ST_CHASE is
    read once per process, so flipping it between calls compared one kernel with itself.  The stage's control words
    say which kernel ran; tests/test_gpu_sb2st_stages.py compares the reflectors themselves, on more classes.)"""
    Bd = _random_band(n, 3 * n + 1)
    Z0 = np.eye(n)[:, ::max(n // 16, 1)][:, :16].copy()
    r1 = hip.sb2st_stage(Bd, Z0, chase_mode=1, reflectors=False)
    r2 = hip.sb2st_stage(Bd, Z0, chase_mode=2, reflectors=False)
    r3 = hip.sb2st_stage(Bd, Z0, chase_mode=2, reflectors=False)
    assert r1["ran"] == 1 and r2["ran"] == 2 and r3["ran"] == 2
    (d1, e1, Z1, f1), (d2, e2, Z2, f2), (d3, e3, Z3, f3) = ((r["d"], r["e"], r["Z"], r["flag"]) for r in (r1, r2, r3))
    assert f1 == 0 and f2 == 0 and f3 == 0
    assert np.array_equal(d1, d2) and np.array_equal(e1, e2) and np.array_equal(Z1, Z2)
    assert np.array_equal(d3, d2) and np.array_equal(e3, e2) and np.array_equal(Z3, Z2)
    T = np.diag(d2) + np.diag(e2, 1) + np.diag(e2, -1)
    assert np.abs(np.linalg.eigvalsh(Bd) - np.linalg.eigvalsh(T)).max() <= 8 * n * EPS * np.abs(d2).max()


@pytest.mark.parametrize("n,ncols", [(3, 3), (66, 66), (130, 17), (200, 200), (321, 64), (777, 100), (1000, 1000), (1500, 333)])
def test_q2_application_does_not_depend_on_the_blocks_of_sweeps_per_pass(hip, n, ncols):
    """Z <- Q2 Z streams Z once per bundle of blocks of 32 sweeps: three per pass (the default) or two (EK_Q2_NBLK=2, as
    in round 2).  Same groups in the same order on every element: the results must be the same bits, and Q2
    orthogonal.  (tools/q2_anchor.py compares two BUILDS of the library the same way: the round-2 pair kernel, retired
    in round 3, gave these bits too.)"""
    Bd = _random_band(n, 7 * n + 3)
    rng = np.random.default_rng(n)
    Z0 = rng.standard_normal((n, ncols))
    res = {}
    try:
        for nblk in ("2", "3", "4"):
            os.environ["EK_Q2_NBLK"] = nblk
            d, e, Z, f = hip.sb2st(Bd, Z0)
            assert f == 0
            res[nblk] = (d, e, Z)
    finally:
        os.environ.pop("EK_Q2_NBLK", None)
    assert np.array_equal(res["2"][2], res["3"][2]) and np.array_equal(res["2"][2], res["4"][2])
    if ncols == n:
        _, _, Q2, _ = hip.sb2st(Bd, np.eye(n))
        assert np.linalg.norm(Q2.T @ Q2 - np.eye(n)) <= 64 * n * EPS


def test_q2_application_keeps_the_bits_of_its_earlier_forms(hip):
    """tests/golden/q2_anchor_digests.txt: SHA-256 of Z <- Q2 Z on fixed inputs (tools/q2_anchor.py), identical for round 2's
    pair kernel and for every form of the kernel since (three and four blocks of sweeps per pass, the record written in
    halves between the matrix instructions, the LDS images re-laid for the banking of 64-bit reads).  A change of these
    digests means the arithmetic of the bulge chasing or of its back-transformation changed: legitimate only if
    deliberate -- regenerate the file with the tool then."""
    import hashlib
    path = os.path.join(os.path.dirname(__file__), "golden", "q2_anchor_digests.txt")
    for line in open(path):
        n, ncols, flag, digest = line.split()
        n, ncols = int(n), int(ncols)
        M = np.random.RandomState(7 * n + 3).standard_normal((n, n))
        M = np.tril(M) - np.tril(M, -(B + 1))
        Bd = M + np.tril(M, -1).T
        Z0 = np.random.RandomState(n).standard_normal((n, ncols))
        d, e, Z, f = hip.sb2st(Bd, Z0)
        assert f == int(flag)
        assert hashlib.sha256(np.ascontiguousarray(Z).tobytes()).hexdigest()[:16] == digest, (n, ncols)


@pytest.mark.parametrize("n", [777, 2100])
def test_position_kernel_under_shaken_timing(hip, n):
    """Pseudo-random pauses of single positions (EK_SB2ST_JITTER) change which neighbour waits for which: a mail line
    read too early, emptied too late or overwritten before it was taken would change d, e or the reflectors."""
    Bd = _random_band(n, 5 * n + 1)
    Z0 = np.eye(n)[:, ::max(n // 16, 1)][:, :16].copy()
    d0, e0, Z0r, f0 = hip.sb2st(Bd, Z0)
    try:
        for jit in ("1", "7", "12345"):
            os.environ["EK_SB2ST_JITTER"] = jit
            d1, e1, Z1, f1 = hip.sb2st(Bd, Z0)
            assert f1 == 0 and np.array_equal(d0, d1) and np.array_equal(e0, e1) and np.array_equal(Z0r, Z1)
    finally:
        os.environ.pop("EK_SB2ST_JITTER", None)
    assert f0 == 0


def test_position_kernel_falls_back_when_its_workgroups_cannot_all_be_resident(hip):
    """The position-owned kernel needs every workgroup on the chip at once; its census gives up after a bounded
    wait and the sweep kernel behind it redoes the stage from the repacked band (same bits).  A census of zero
    polls makes that happen whenever a workgroup is not the last to arrive."""
    n = 1500
    Bd = _random_band(n, 11)
    d0, e0, _, f0 = hip.sb2st(Bd)
    try:
        os.environ["EK_SB2ST_CENSUS_SPINS"] = "0"
        d1, e1, _, f1 = hip.sb2st(Bd)
    finally:
        os.environ.pop("EK_SB2ST_CENSUS_SPINS", None)
    assert f0 == 0 and f1 == 0
    assert np.array_equal(d0, d1) and np.array_equal(e0, e1)


@pytest.fixture()
def forced_two_stage(hip):
    hip.set_two_stage(100)
    yield
    hip.set_two_stage(-1)


def _check_pairs(A, Bm, w, Z, n_vec=None):
    n = A.shape[0]
    n_vec = n if n_vec is None else n_vec
    _, _, mx = eval_residual_norm(A, w[:n_vec], Z[:, :n_vec], Bm)
    assert mx <= 1e-14 * max(1.0, np.sqrt(n / 1024.0)), mx
    assert eval_orthogonality(Z[:, :n_vec], Bm) <= 1e-11


@pytest.mark.parametrize("n", [100, 129, 257, 640, 1000])
def test_whole_path_through_two_stages_matches_oracle(hip, oracle, forced_two_stage, n):
    A = oracle.synth_matrix(n, 1)
    Bm = oracle.synth_matrix(n, 2)
    w_or = oracle.solve(A, Bm)[0]
    ep, _ = hip.eigen_solver("general_hip", A, Bm)
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * np.abs(w_or).max()
    _check_pairs(A, Bm, ep.values, ep.Vectors)
    w_or = oracle.solve(A)[0]
    ep, _ = hip.eigen_solver("hip", A)
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * np.abs(w_or).max()
    _check_pairs(A, None, ep.values, ep.Vectors)
    ep, _ = hip.eigen_solver("general_hip_select", A, Bm, n_vec=37)
    _check_pairs(A, Bm, ep.values, ep.Vectors, 37)


def test_two_stage_and_one_stage_agree(hip, oracle):
    n = 700
    A = oracle.synth_matrix(n, 1); Bm = oracle.synth_matrix(n, 2)
    hip.set_two_stage(0)
    try:
        ep1, _ = hip.eigen_solver("general_hip", A, Bm)
        hip.set_two_stage(100)
        ep2, _ = hip.eigen_solver("general_hip", A, Bm)
    finally:
        hip.set_two_stage(-1)
    assert np.abs(ep1.values - ep2.values).max() <= 4 * n * EPS * np.abs(ep1.values).max()
    # eigenvectors agree up to sign (the spectrum of the generator is simple)
    Bz = Bm @ ep2.Vectors
    dots = np.abs(np.einsum("ij,ij->j", ep1.Vectors, Bz))
    assert np.abs(dots - 1.0).max() <= 1e-9


def _hard_input(oracle, kind, n, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "banded":
        M = np.tril(rng.standard_normal((n, n))); M = M - np.tril(M, -5); return M + np.tril(M, -1).T
    if kind == "diagonal":
        return np.diag(rng.uniform(1, 2, n))
    if kind == "rank_deficient_panel":
        A = oracle.synth_matrix(n, 1); A[64:, 3] = 0.0; A[3, 64:] = 0.0          # a zero column in the first panel
        return A
    if kind == "low_rank_plus_identity":
        u = rng.standard_normal((n, 3)); return u @ u.T + np.eye(n)
    if kind == "sparse_pattern":           # the reference's own family: few entries per row, anywhere in the row
        A = np.zeros((n, n))
        for i in range(n):
            for j in rng.integers(0, n, 4):
                A[i, j] += rng.standard_normal(); A[j, i] = A[i, j]
        return A + np.diag(rng.uniform(2, 3, n))
    if kind == "ill_conditioned_panel":    # two nearly parallel columns: cond of the first panel ~ 1e12
        A = oracle.synth_matrix(n, 1); A[64:, 5] = A[64:, 4] * (1.0 + 1e-12) ; A[5, 64:] = A[64:, 5]
        return A
    raise ValueError(kind)


HARD = ["banded", "diagonal", "rank_deficient_panel", "low_rank_plus_identity", "sparse_pattern", "ill_conditioned_panel"]


@pytest.mark.parametrize("kind", HARD)
def test_panels_cholesky_qr_cannot_factor_are_rescued_inside_the_stage(hip, oracle, forced_two_stage, kind):
    """A panel without full column rank (or too ill-conditioned) makes CholeskyQR2's device-side check fail; THAT panel is
    then factored by Householder reflections (any rank, as PDSYTRD's panels are) and the stage goes on in two stages:
    no flag, an orthogonal similarity to a band matrix at rounding level, correct pairs from the whole path."""
    n = 500
    A = _hard_input(oracle, kind, n)
    Ab, V, tau, flag = hip.sy2sb(A)
    assert flag & 0xff == 0
    if kind != "sparse_pattern":
        assert flag >> 8 >= 1                       # at least one panel went through the rescue
    assert np.abs(np.tril(Ab, -(B + 1))).max() == 0.0
    Q = _q_from_reflectors(V, tau)
    nrm = max(np.linalg.norm(A), 1.0)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 64 * n * EPS
    assert np.linalg.norm(Q.T @ A @ Q - _band_of(Ab)) <= 32 * n * EPS * nrm
    w_or = np.linalg.eigvalsh(A)
    import ctypes
    st = (ctypes.c_double * 8)()
    os.environ["EK_HIP_BAND_INPUT"] = "0"           # (a band on entry would skip the stage this test is about)
    try:
        ep, _ = hip.eigen_solver("hip", A)
        hip.load_library().ek_hip_debug_last_solve_stats(st, 8)
    finally:
        os.environ.pop("EK_HIP_BAND_INPUT", None)
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * max(np.abs(w_or).max(), 1.0)
    _check_pairs(A, None, ep.values, ep.Vectors)
    assert st[1] == 1.0 and st[3] == 0.0            # the solve stayed on the two-stage path, first stage included


@pytest.mark.parametrize("pairs", ["0", "1"])
def test_reference_matrix_through_two_stages(hip, golden_dir, forced_two_stage, monkeypatch, pairs):
    """The reference's own sparse Hamiltonian (VCNT400std, 8 200 non-zeros of 160 000) with the two-stage form forced on:
    its first panels are rank deficient; eigenvalues against the reference's golden file (12 digits) -- with the panels of
    the dense -> band stage one by one and in pairs (rescued panels inside pairs)."""
    from eigenkernel_amd import matrix_io
    monkeypatch.setenv("EK_SY2SB_PAIR_MIN", pairs)
    A = matrix_io.read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_A.mtx")).to_dense()
    w_ref = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_VCNT400std_E.txt"))[:, 1]
    ep, _ = hip.eigen_solver("hip", A)
    assert np.abs(ep.values - w_ref).max() <= 5e-12 * max(1.0, np.abs(w_ref).max())
    _check_pairs(A, None, ep.values, ep.Vectors)
    import ctypes
    st = (ctypes.c_double * 8)()
    hip.load_library().ek_hip_debug_last_solve_stats(st, 8)
    assert st[1] == 1.0


@pytest.mark.parametrize("halfwidth,taken", [(0, True), (4, True), (64, True), (65, False), (100, False), (200, False)])
def test_a_band_on_entry_skips_the_dense_to_band_stage(hip, halfwidth, taken):
    """A standard problem whose matrix has nothing below its 64th subdiagonal is already what the first stage would
    produce (the reference's sparse Hamiltonians are often banded): the solve goes straight to the bulge chasing and Q1 is
    the identity.  One subdiagonal more and it is a dense matrix like any other -- whose first panels are random
    TRIANGLES (condition ~1e7): CholeskyQR2 orthogonalises them, but forming Q1 with the explicit inverse of R1 lost
    seven digits (eigenvalues 1.5e-9 off); Q1 = A R1^-1 is formed by substitution since.  Same pairs either way."""
    import ctypes
    n = 1500
    rng = np.random.default_rng(11 + halfwidth)
    M = np.tril(rng.standard_normal((n, n))); M = M - np.tril(M, -(halfwidth + 1))
    A = M + np.tril(M, -1).T
    w_or = np.linalg.eigvalsh(A)
    st = (ctypes.c_double * 8)()
    ep, _ = hip.eigen_solver("hip", A)
    hip.load_library().ek_hip_debug_last_solve_stats(st, 8)
    assert st[1] == 1.0 and (st[3] == 1.0) == taken
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * max(np.abs(w_or).max(), 1.0)
    _check_pairs(A, None, ep.values, ep.Vectors)
    eps, _ = hip.eigen_solver("hip_select", A, n_vec=100)
    assert np.abs(eps.values[:100] - w_or[:100]).max() <= 4 * n * EPS * max(np.abs(w_or).max(), 1.0)
    _check_pairs(A, None, eps.values, eps.Vectors, n_vec=100)
    os.environ["EK_HIP_BAND_INPUT"] = "0"
    try:
        ep0, _ = hip.eigen_solver("hip", A)
        hip.load_library().ek_hip_debug_last_solve_stats(st, 8)
    finally:
        os.environ.pop("EK_HIP_BAND_INPUT", None)
    assert st[3] == 0.0
    assert np.abs(ep0.values - ep.values).max() <= 4 * n * EPS * max(np.abs(w_or).max(), 1.0)


@pytest.mark.parametrize("kind", ["banded", "sparse_pattern", "low_rank_plus_identity"])
def test_hard_inputs_at_a_two_stage_order(hip, oracle, kind):
    """N = 4096 (well inside the two-stage range) against numpy: the rescue at full panel heights."""
    n = 4096
    A = _hard_input(oracle, kind, n, seed=5)
    w_or = np.linalg.eigvalsh(A)
    ep, _ = hip.eigen_solver("hip", A)
    assert np.abs(ep.values - w_or).max() <= 4 * n * EPS * max(np.abs(w_or).max(), 1.0)
    _check_pairs(A, None, ep.values, ep.Vectors)


def test_grid_cell_piece_through_two_stages_is_bit_identical(hip, oracle, forced_two_stage):
    """Replicated-input mode on a 2 x 2 grid: the cell's block-cyclic piece equals the 1 x 1 result."""
    from eigenkernel_amd import descriptor as dsc
    n = 400
    A = oracle.synth_matrix(n, 1); Bm = oracle.synth_matrix(n, 2)
    ep, _ = hip.eigen_solver("general_hip", A, Bm)
    proc = hip.Process(my_rank=3, n_procs=4, n_procs_row=2, n_procs_col=2, my_proc_row=1, my_proc_col=1)
    epg, _ = hip.eigen_solver("general_hip", A, Bm, proc=proc)
    nb = int(epg.desc[dsc.BLOCK_ROW_])
    ri = dsc.local_indices(n, nb, 1, 2); ci = dsc.local_indices(n, nb, 1, 2)
    assert np.array_equal(epg.values, ep.values)
    assert np.array_equal(epg.Vectors[:len(ri), :len(ci)], ep.Vectors[np.ix_(ri, ci)])


def test_an_abandoned_bulge_chasing_is_repeated_from_the_saved_band(hip, oracle):
    """The whole-path call keeps no copy of the reduced matrix any more (round 4): a bulge chasing that abandons a bounded
    wait -- a matter of timing, simulated here by a debug hook -- is repeated from the band it started from with the
    older kernel, up to twice; the result is the undisturbed one bit for bit (both kernels run the same arithmetic), and a
    third failure ends the call with -992."""
    n = 900
    A = oracle.synth_matrix(n, 1); B = oracle.synth_matrix(n, 2)
    lib = hip.load_library()
    ref, _ = hip.eigen_solver("general_hip", A, B)
    for times in (1, 2):
        assert lib.ek_hip_debug_fail_next_chase(times) == 0
        ep, _ = hip.eigen_solver("general_hip", A, B)
        assert np.array_equal(ep.values, ref.values) and np.array_equal(ep.Vectors, ref.Vectors)
    assert lib.ek_hip_debug_fail_next_chase(3) == 0
    with pytest.raises(Exception) as err:
        hip.eigen_solver("general_hip", A, B)
    assert "-992" in str(err.value)
    assert lib.ek_hip_debug_fail_next_chase(0) == 0
    ep, _ = hip.eigen_solver("general_hip", A, B)
    assert np.array_equal(ep.values, ref.values)
