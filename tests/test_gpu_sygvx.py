"""GPU suite of DSYGVX's problem types 2 and 3 (ek_hip_sygvx*, ek_hip_sygst_ibtype, ek_hip_trmm): A B x = l x and
B A x = l x through C = L^T A L.  The reference is NumPy: L = cholesky(B), C = L^T A L, eigh(C), then x = L^-T y
(type 2) or x = L y (type 3).  Building blocks against NumPy, solves over both jobz and both ranges, the invariants
between the types, ill-conditioned and non-SPD B, and the headline order's accuracy and speed against type 1."""
import ctypes
import os
import time

import numpy as np
import pytest

from eigenkernel_amd.matrix_io import read_matrix_file

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16


def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return np.asfortranarray((G + G.T) / 2.0)


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return np.asfortranarray((B + B.T) / 2.0)


def _upper_nan(M):
    M = np.array(M, order="F", copy=True)
    M[np.triu_indices(M.shape[0], 1)] = np.nan
    return M


def _reference(A, B, itype):
    """NumPy: (w, X) of the type's problem with its normalisation."""
    L = np.linalg.cholesky(B)
    w, Y = np.linalg.eigh(L.T @ A @ L)
    X = np.linalg.solve(L.T, Y) if itype == 2 else L @ Y
    return w, X


def _residual(A, B, itype, w, X):
    """max_j ||M x_j - l_j x_j|| / (||A|| ||B|| ||x_j||), M = A B (type 2) or B A (type 3)."""
    R = (A @ (B @ X) if itype == 2 else B @ (A @ X)) - X * w
    scale = np.linalg.norm(A, 2) * np.linalg.norm(B, 2)
    return float((np.linalg.norm(R, axis=0) / (scale * np.linalg.norm(X, axis=0))).max())


def _orth(B, itype, X):
    """max |X^T B X - I| (type 2) or max |X^T B^-1 X - I| (type 3)."""
    if itype == 2:
        G = X.T @ (B @ X)
    else:
        V = np.linalg.solve(np.linalg.cholesky(B), X)
        G = V.T @ V
    return float(np.abs(G - np.eye(X.shape[1])).max())


def _check(A, B, itype, w, X, w_ref, X_ref, cond=1.0):
    amax = float(np.abs(w_ref).max()) if len(w_ref) else 1.0
    assert np.abs(w - w_ref).max() <= 1e-12 * cond * max(amax, 1e-300), (itype, np.abs(w - w_ref).max())
    if X is None:
        return
    r, r_np = _residual(A, B, itype, w, X), _residual(A, B, itype, w_ref, X_ref)
    assert r <= 10.0 * max(r_np, 1e-15), (itype, r, r_np)
    assert _orth(B, itype, X) <= 1e-11 * cond, (itype, _orth(B, itype, X))


# ------------------------------------------------------------------------------------------- 1. building blocks
BLOCK_SIZES = [1, 2, 5, 129, 255, 256, 257, 1000, 4097, 5000]


@pytest.mark.parametrize("n", BLOCK_SIZES)
def test_sygst_ibtype_and_trmm_against_numpy(hip, n):
    rng = np.random.default_rng(1000 + n)
    A = _sym(rng, n)
    B = _spd(rng, n)
    L = np.tril(np.linalg.cholesky(B))
    C = L.T @ A @ L
    bound = 4 * n * EPS * float((np.abs(L).T @ np.abs(A) @ np.abs(L)).max()) + 1e-300
    lo = np.tril_indices(n)
    # NaN in the strict upper triangles of A and of L (after potrf B's upper part is the caller's): never read
    for ibtype in (2, 3):
        out, info = hip.sygst_ibtype(_upper_nan(A), _upper_nan(L), ibtype)
        assert info == 0
        assert np.isfinite(out[lo]).all(), ibtype
        assert np.abs(out[lo] - C[lo]).max() <= bound, (ibtype, np.abs(out[lo] - C[lo]).max(), bound)
    # ibtype 1 is ek_hip_sygst, bit for bit
    a1, info1 = hip.sygst_ibtype(A, L, 1)
    a1r, info1r = hip.sygst(A, L)
    assert info1 == info1r == 0 and np.array_equal(a1[lo], a1r[lo])
    for nrhs in (1, 7, n + 3):
        Z = np.asfortranarray(rng.standard_normal((n, nrhs)))
        X, info = hip.trmm(_upper_nan(L), Z)
        assert info == 0 and np.isfinite(X).all()
        tb = 4 * n * EPS * float((np.abs(L) @ np.abs(Z)).max())
        assert np.abs(X - L @ Z).max() <= tb, (nrhs, np.abs(X - L @ Z).max(), tb)


# ------------------------------------------------------------------------------------------- 2. solves
def _fixture_bnz30(golden_dir):
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx")).to_dense()
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense()
    return np.asfortranarray(A), np.asfortranarray(B)


def _cut(w, k):
    """A value between eigenvalues k-1 and k (0-based) at the widest nearby gap."""
    if k <= 0:
        return w[0] - 1.0 - abs(w[0])
    if k >= len(w):
        return w[-1] + 1.0 + abs(w[-1])
    return 0.5 * (w[k - 1] + w[k])


@pytest.mark.parametrize("n", [1, 30, 300, 511, 512, 1000, 2049])
def test_types_2_and_3_solves(hip, golden_dir, n):
    if n == 30:
        A, B = _fixture_bnz30(golden_dir)
    else:
        rng = np.random.default_rng(n)
        A, B = _sym(rng, n), _spd(rng, n)
    for itype in (2, 3):
        w_ref, X_ref = _reference(A, B, itype)
        # every pair, both ways
        w, Z, f = hip.sygvx(A, B, itype=itype)
        assert f == 1 and len(w) == n
        _check(A, B, itype, w, Z, w_ref, X_ref)
        w0, Z0, _ = hip.sygvx(A, B, itype=itype, vectors=False)
        assert Z0 is None
        _check(A, B, itype, w0, None, w_ref, None)
        # an index window and a value window, with and without vectors
        il, iu = max(1, n // 4), max(1, (3 * n) // 4)
        lo, hi = il - 1, iu                   # the value window that holds il..iu
        vl, vu = _cut(w_ref, lo), _cut(w_ref, hi)
        for vectors in (True, False):
            wi, Zi, fi = hip.sygvx(A, B, itype=itype, il=il, iu=iu, vectors=vectors)
            assert fi == il and len(wi) == iu - il + 1
            _check(A, B, itype, wi, Zi, w_ref[lo:hi], None if Zi is None else X_ref[:, lo:hi])
            wv, Zv, fv = hip.sygvx(A, B, itype=itype, vl=vl, vu=vu, vectors=vectors)
            assert fv == il and len(wv) == iu - il + 1
            _check(A, B, itype, wv, Zv, w_ref[lo:hi], None if Zv is None else X_ref[:, lo:hi])


# ------------------------------------------------------------------------------------------- 3. invariants
def test_types_2_and_3_share_eigenvalues_and_y(hip):
    rng = np.random.default_rng(7)
    n = 700
    A, B = _sym(rng, n), _spd(rng, n)
    w2, Z2, _ = hip.sygvx(A, B, itype=2)
    w3, Z3, _ = hip.sygvx(A, B, itype=3)
    assert w2.tobytes() == w3.tobytes()
    v2, _, _ = hip.sygvx(A, B, itype=2, vectors=False)
    v3, _, _ = hip.sygvx(A, B, itype=3, vectors=False)
    assert v2.tobytes() == v3.tobytes()
    # x2 = L^-T y and x3 = L y: B x2 = x3, column by column
    BZ2 = B @ Z2
    tol = 8 * n * EPS * np.linalg.norm(B, 2) * np.abs(Z2).max(axis=0)
    assert (np.abs(BZ2 - Z3).max(axis=0) <= tol).all()
    # NaN in the strict upper triangles of A and B changes no bit
    w2n, Z2n, _ = hip.sygvx(_upper_nan(A), _upper_nan(B), itype=2)
    w3n, Z3n, _ = hip.sygvx(_upper_nan(A), _upper_nan(B), itype=3)
    assert w2n.tobytes() == w2.tobytes() and Z2n.tobytes() == Z2.tobytes()
    assert w3n.tobytes() == w3.tobytes() and Z3n.tobytes() == Z3.tobytes()


def test_type_1_is_eigenpairs_bit_for_bit(hip):
    rng = np.random.default_rng(11)
    n = 600
    A, B = _sym(rng, n), _spd(rng, n)
    for kw in (dict(), dict(il=100, iu=300), dict(vl=-1.0, vu=2.0), dict(vectors=False), dict(il=5, iu=9, vectors=False)):
        w1, Z1, f1 = hip.sygvx(A, B, itype=1, **kw)
        we, Ze, fe = hip.eigenpairs(A, B, **kw)
        assert f1 == fe and w1.tobytes() == we.tobytes(), kw
        assert (Z1 is None and Ze is None) or Z1.tobytes() == Ze.tobytes(), kw


def test_identity_b_is_the_standard_problem(hip):
    rng = np.random.default_rng(3)
    n = 300
    A = _sym(rng, n)
    I = np.asfortranarray(np.eye(n))
    w_std = np.linalg.eigvalsh(A)
    bound = n * EPS * np.abs(w_std).max()
    for itype in (2, 3):
        w, Z, _ = hip.sygvx(A, I, itype=itype)
        assert np.abs(w - w_std).max() <= bound, (itype, np.abs(w - w_std).max(), bound)
        assert np.abs(A @ Z - Z * w).max() <= 1e-13 * np.abs(w_std).max()


def test_ill_conditioned_b(hip):
    rng = np.random.default_rng(5)
    n, cond = 400, 1e6
    A, B = _sym(rng, n), _spd(rng, n, cond=cond)
    for itype in (2, 3):
        w_ref, X_ref = _reference(A, B, itype)
        w, Z, _ = hip.sygvx(A, B, itype=itype)
        _check(A, B, itype, w, Z, w_ref, X_ref, cond=cond)


def test_errors_match_type_1(hip):
    rng = np.random.default_rng(9)
    n = 300
    A, B = _sym(rng, n), _spd(rng, n)
    Bbad = B.copy(order="F"); Bbad[100, 100] = -5.0
    with pytest.raises(hip.SolverError) as ex1:
        hip.eigenpairs(A, Bbad)
    assert ex1.value.info > 0
    for itype in (2, 3):
        for kw in (dict(), dict(il=3, iu=9), dict(vl=-1.0, vu=1.0, vectors=False)):
            with pytest.raises(hip.SolverError) as ex:
                hip.sygvx(A, Bbad, itype=itype, **kw)
            assert ex.value.info == ex1.value.info, (itype, kw)
        An = A.copy(order="F"); An[7, 3] = np.nan; An[3, 7] = np.nan
        with pytest.raises(hip.SolverError) as ex:
            hip.sygvx(An, B, itype=itype)
        assert ex.value.info == -9


# ------------------------------------------------------------------------------------------- 4. headline order
N_BIG = 16384


def _forward(L, X, nb=512):
    """L^-1 X by block forward substitution (n^2 per column: the host check at the headline order)."""
    V = np.zeros_like(X)
    for i in range(0, L.shape[0], nb):
        j = min(i + nb, L.shape[0])
        V[i:j] = np.linalg.solve(L[i:j, i:j], X[i:j] - L[i:j, :i] @ V[:i])
    return V


class _Dev:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), max(int(nbytes), 8)) == 0
        self.ptrs.append(p)
        return p

    def down(self, p, shape):
        out = np.zeros(shape, order="F")
        assert self.lib.ek_hip_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)


def _sygvx_dev(lib, itype, jobz, dA, dB, dw, dZ, n, st=None):
    """ek_hip_sygvx_device on the synthetic pair (regenerated in place): (info, seconds)."""
    assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
    assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
    assert lib.ek_hip_synchronize() == 0
    m, f = ctypes.c_int(-1), ctypes.c_int(-1)
    sp = st.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if st is not None else None
    t0 = time.perf_counter()
    info = lib.ek_hip_sygvx_device(itype, jobz, 0, n, 0.0, 0.0, 1, n, dA, n, dB, n, ctypes.byref(m), ctypes.byref(f),
                                   dw, dZ, n, n, sp, 0 if st is None else len(st))
    return info, time.perf_counter() - t0


def test_headline_order_type_3_accuracy_and_speed(hip):
    lib = hip.load_library()
    n = N_BIG
    with _Dev(lib) as dev:
        dA, dB, dZ = dev.alloc(n * n * 8), dev.alloc(n * n * 8), dev.alloc(n * n * 8)
        dw = dev.alloc(n * 8)
        # accuracy of type 3 on 64 sampled columns, on the host
        assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
        assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
        A = dev.down(dA, (n, n))             # (the generator fills both triangles)
        B = dev.down(dB, (n, n))
        info, _ = _sygvx_dev(lib, 3, 1, dA, dB, dw, dZ, n)
        assert info == 0
        w = dev.down(dw, (n,))
        assert np.all(np.diff(w) >= 0)
        cols = np.unique(np.linspace(0, n - 1, 64).astype(int))
        Zs = np.zeros((n, len(cols)), order="F")
        for k, j in enumerate(cols):
            assert lib.ek_hip_memcpy_d2h(Zs[:, k].ctypes.data, ctypes.c_void_p(dZ.value + int(j) * n * 8), n * 8) == 0
        R = B @ (A @ Zs) - Zs * w[cols]
        scale = np.linalg.norm(A, 1) * np.linalg.norm(B, 1)
        res = float((np.linalg.norm(R, axis=0) / (scale * np.linalg.norm(Zs, axis=0))).max())
        assert res <= 1e-14 * np.sqrt(n / 1024.0), res
        Lb = np.linalg.cholesky(B)
        V = _forward(Lb, Zs)
        orth = float(np.abs(V.T @ V - np.eye(len(cols))).max())
        assert orth <= 1e-11, orth
        del A, B, Lb, V
        # speed: best of 3 after a warm-up, every type in the same process, alternated
        t = {1: [], 2: [], 3: []}
        tv = {1: [], 2: []}
        sg = {1: [], 2: [], 3: []}
        for it in (1, 2, 3):
            assert _sygvx_dev(lib, it, 1, dA, dB, dw, dZ, n)[0] == 0
        for _ in range(3):
            for it in (1, 2, 3):
                st = np.zeros(8)
                info, sec = _sygvx_dev(lib, it, 1, dA, dB, dw, dZ, n, st)
                assert info == 0
                t[it].append(sec)
                sg[it].append(st[1])
            for it in (1, 2):
                info, sec = _sygvx_dev(lib, it, 0, dA, dB, dw, dZ, n)
                assert info == 0
                tv[it].append(sec)
        best = {k: min(v) for k, v in t.items()}
        print("sygvx N=%d full: %s values: %s sygst: %s" % (n, best, {k: min(v) for k, v in tv.items()},
                                                             {k: min(v) for k, v in sg.items()}))
        assert best[2] <= 1.10 * best[1], t
        assert best[3] <= 1.10 * best[1], t
        assert min(tv[2]) <= 1.15 * min(tv[1]), tv
        assert min(sg[2]) <= 1.25 * min(sg[1]), sg
        assert min(sg[3]) <= 1.25 * min(sg[1]), sg
