"""GPU suite of the batched entries (ek_hip_eigenpairs_batched*): many problems of order <= 128 in one launch, a
workgroup per problem with the matrix in LDS.  The reference is SciPy on the CPU (scipy.linalg.eigh(A, B)) on seeded
inputs of the kind tests/test_gpu_sygvx.py uses; bounds are those of tests/test_gpu_path.py (4 n eps on eigenvalues with
n floored at 8, 64 / 256 n eps on residual and orthogonality).  Accuracy on both sides of every class boundary, the
reference's shipped BNZ30 pair, the contract (bit-identity wherever a problem sits, untouched upper triangles and
padding, per-problem info), and the speed against the only other way to do the job: a host loop over
ek_hip_solve_device."""
import ctypes
import os
import time

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd.matrix_io import read_matrix_file

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (1, 2, 3, 17, 30, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128)
SENTINEL = -7.25e77


def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


def _pairs(seed, batch, n):
    rng = np.random.default_rng(seed)
    A = np.stack([_sym(rng, n) for _ in range(batch)])
    B = np.stack([_spd(rng, n) for _ in range(batch)])
    return A, B


def _view(flat, batch, n, ld, stride):
    """[b, j, i] view of element (i, j) of problem b in a strided column-major buffer."""
    it = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat, shape=(batch, n, n), strides=(stride * it, ld * it, it))


def _pack(M, ld, stride, fill=SENTINEL):
    batch, n = M.shape[0], M.shape[1]
    flat = np.full(max(batch * stride, 1), fill)
    _view(flat, batch, n, ld, stride)[...] = M.transpose(0, 2, 1)
    return flat


def _unpack(flat, batch, n, ld, stride):
    return _view(flat, batch, n, ld, stride).transpose(0, 2, 1).copy()


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

    def put(self, p, a):
        assert self.lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    def down(self, p, like):
        out = np.empty_like(like)
        if out.nbytes:
            assert self.lib.ek_hip_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)


class _Out:
    pass


def _batched_device(lib, A, B, jobz, lda=None, sA=None, ldb=None, sB=None, ldz=None, sZ=None):
    """ek_hip_eigenpairs_batched_device on strided device images of A[b], B[b] (full matrices: both triangles as
    given).  Returns rc, info, w, Z and the device images after the call."""
    batch, n = A.shape[0], A.shape[1]
    lda = lda or n; ldb = ldb or n; ldz = ldz or n
    sA = sA or lda * n; sB = sB or ldb * n; sZ = sZ or ldz * n
    hA = _pack(A, lda, sA)
    hB = _pack(B, ldb, sB) if B is not None else None
    hZ = np.full(max(batch * sZ, 1), SENTINEL)
    hw = np.full(max(batch * n, 1), SENTINEL)
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    o = _Out()
    with _Dev(lib) as dev:
        dA = dev.up(hA)
        dB = dev.up(hB) if B is not None else None
        dw, dZ = dev.up(hw), dev.up(hZ)
        sec = ctypes.c_double(-1.0)
        o.rc = lib.ek_hip_eigenpairs_batched_device(0 if B is None else 1, jobz, n, batch, dA, lda, sA, dB, ldb, sB, dw,
                                                    dZ if jobz else None, ldz, sZ,
                                                    info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(sec))
        o.seconds = sec.value
        o.info = info[:batch].copy()
        o.w = dev.down(dw, hw)[:batch * n].reshape(batch, n)
        o.Zflat = dev.down(dZ, hZ)
        o.Z = _unpack(o.Zflat, batch, n, ldz, sZ)
        o.Aflat = dev.down(dA, hA)
        o.Bflat = dev.down(dB, hB) if B is not None else None
        o.hA, o.hB = hA, hB
    return o


def _solve_device(lib, A, B):
    """ek_hip_solve_device on one pair: (info, w)."""
    n = A.shape[0]
    with _Dev(lib) as dev:
        dA = dev.up(np.asfortranarray(A))
        dB = dev.up(np.asfortranarray(B)) if B is not None else None
        w, Z = np.zeros(n), np.zeros((n, n), order="F")
        dw, dZ = dev.up(w), dev.up(Z)
        info = lib.ek_hip_solve_device(0 if B is None else 1, n, n, dA, n, dB, n, dw, dZ, n, None, 0)
        return info, dev.down(dw, w)


def _ref(A, B):
    return sl.eigh(A, B, lower=True) if B is not None else sl.eigh(A, lower=True)


def _check_problem(A, B, w, Z, w_ref, what):
    n = A.shape[0]
    tol_w = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
    err = np.abs(w - w_ref).max()
    assert np.all(np.diff(w) >= 0), what
    assert err <= tol_w, (what, "eigenvalues", err, tol_w)
    if Z is None:
        return err / tol_w, 0.0, 0.0
    c = 256 if B is not None else 64
    BZ = B @ Z if B is not None else Z
    res = np.abs(A @ Z - BZ * w).max()
    orth = np.abs(Z.T @ BZ - np.eye(n)).max()
    assert res <= c * n * EPS * np.abs(A).max(), (what, "residual", res, c * n * EPS * np.abs(A).max())
    assert orth <= c * n * EPS, (what, "orthogonality", orth, c * n * EPS)
    return err / tol_w, res / (c * n * EPS * np.abs(A).max()), orth / (c * n * EPS)


# ------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", ORDERS)
def test_batched_accuracy_against_scipy(hip, n, problem, jobz):
    """24 problems of one order in one batch against scipy.linalg.eigh; with vectors also each problem's eigenvalues
    against ek_hip_solve_device on the same pair (other algorithms: to the bound, not to the bit)."""
    lib = hip.load_library()
    batch = 24
    A, B = _pairs(1000 + n, batch, n)
    if not problem:
        B = None
    o = _batched_device(lib, A, B, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    worst = np.zeros(4)                     # the largest share of each bound any problem of the batch used
    for b in range(batch):
        Bb = B[b] if problem else None
        w_ref = _ref(A[b], Bb)[0]
        used = _check_problem(A[b], Bb, o.w[b], o.Z[b] if jobz else None, w_ref, (n, problem, jobz, b))
        worst[:3] = np.maximum(worst[:3], used)
        if jobz:
            info, w_lib = _solve_device(lib, A[b], Bb)
            assert info == 0
            tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
            worst[3] = max(worst[3], np.abs(o.w[b] - w_lib).max() / tol)
            assert np.abs(o.w[b] - w_lib).max() <= tol, (n, problem, b, np.abs(o.w[b] - w_lib).max(), tol)
    print("n=%d problem=%d jobz=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f "
          "against ek_hip_solve_device %.3f" % ((n, problem, jobz) + tuple(worst)))


def test_batched_golden_bnz30(hip, golden_dir):
    """64 copies of the reference's shipped generalized pair in one batch: every copy within 1e-14 of its eigenvalue
    file (the bound test_golden_bnz30_generalized uses), all copies the same bits."""
    lib = hip.load_library()
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx")).to_dense()
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense()
    ev = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ev.txt"))[:, 1]
    A3, B3 = np.stack([A] * 64), np.stack([B] * 64)
    o = _batched_device(lib, A3, B3, 1)
    assert o.rc == 0 and not o.info.any()
    for b in range(64):
        assert np.abs(o.w[b] - ev).max() <= 1e-14, (b, np.abs(o.w[b] - ev).max())
        assert np.array_equal(o.w[b], o.w[0]) and np.array_equal(o.Z[b], o.Z[0])
    _check_problem(A, B, o.w[0], o.Z[0], ev, "bnz30")


# ------------------------------------------------------------------------------------------------- contract
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [30, 64, 100])
def test_batched_bit_identity_wherever_a_problem_sits(hip, n, problem):
    """(a) the same pair alone, at positions 0, 7 and last of batches of 8 and 300, and through the host form."""
    lib = hip.load_library()
    A1, B1 = _pairs(7 * n + problem, 1, n)
    alone = _batched_device(lib, A1, B1 if problem else None, 1)
    assert alone.rc == 0 and alone.info[0] == 0
    alone0 = _batched_device(lib, A1, B1 if problem else None, 0)
    for batch in (8, 300):
        Af, Bf = _pairs(99 + batch, batch, n)
        for pos in sorted({0, 7, batch - 1}):
            A, B = Af.copy(), Bf.copy()
            A[pos], B[pos] = A1[0], B1[0]
            o = _batched_device(lib, A, B if problem else None, 1)
            assert o.rc == 0 and not o.info.any()
            assert np.array_equal(o.w[pos], alone.w[0]) and np.array_equal(o.Z[pos], alone.Z[0]), (batch, pos)
            o0 = _batched_device(lib, A, B if problem else None, 0)
            assert np.array_equal(o0.w[pos], alone0.w[0]), (batch, pos)
    A, B = _pairs(5, 8, n)
    A[3], B[3] = A1[0], B1[0]
    A_in, B_in = A.copy(), B.copy()
    w, Z, info = hip.eigenpairs_batched(A, B if problem else None)
    assert not info.any()
    assert np.array_equal(w[3], alone.w[0]) and np.array_equal(Z[3], alone.Z[0])
    assert np.array_equal(A, A_in) and np.array_equal(B, B_in)          # the host form leaves its inputs alone
    w0, Z0, info0 = hip.eigenpairs_batched(A, B if problem else None, vectors=False)
    assert Z0 is None and not info0.any() and np.array_equal(w0[3], alone0.w[0])


@pytest.mark.parametrize("n", [30, 64, 128])
def test_batched_upper_triangles_are_neither_read_nor_written(hip, n):
    """(b) NaN in the strictly upper triangles of every A and B: same bits out, and the NaNs are still there."""
    lib = hip.load_library()
    batch = 6
    A, B = _pairs(31 + n, batch, n)
    clean = _batched_device(lib, A, B, 1)
    An, Bn = A.copy(), B.copy()
    iu = np.triu_indices(n, 1)
    An[:, iu[0], iu[1]] = np.nan
    Bn[:, iu[0], iu[1]] = np.nan
    o = _batched_device(lib, An, Bn, 1)
    assert o.rc == 0 and not o.info.any() and not clean.info.any()
    assert np.array_equal(o.w, clean.w) and np.array_equal(o.Z, clean.Z)
    for flat_after, flat_before in ((o.Aflat, o.hA), (o.Bflat, o.hB)):
        after = _unpack(flat_after, batch, n, n, n * n)
        before = _unpack(flat_before, batch, n, n, n * n)
        assert np.array_equal(after[:, iu[0], iu[1]].view(np.uint64), before[:, iu[0], iu[1]].view(np.uint64))
        assert np.isnan(after[:, iu[0], iu[1]]).all()
    # dB's lower triangle holds L
    L = np.tril(_unpack(o.Bflat, batch, n, n, n * n)[2])
    assert np.abs(L @ L.T - B[2]).max() <= 16 * n * EPS * np.abs(B[2]).max()
    # the standard problem reads no B at all
    s = _batched_device(lib, An, None, 1)
    s_clean = _batched_device(lib, A, None, 1)
    assert np.array_equal(s.w, s_clean.w) and np.array_equal(s.Z, s_clean.Z) and not s.info.any()


@pytest.mark.parametrize("n", [30, 100])
def test_batched_failures_stay_in_their_own_slots(hip, n):
    """(c) problem 5 with a B that is not SPD, problem 9 with a NaN in A's lower triangle: return 0, the two infos,
    and the other 14 problems bit-identical to the same batch with healthy problems in those slots."""
    lib = hip.load_library()
    A, B = _pairs(200 + n, 16, n)
    healthy = _batched_device(lib, A, B, 1)
    assert healthy.rc == 0 and not healthy.info.any()
    Ab, Bb = A.copy(), B.copy()
    Bb[5, n // 2, n // 2] = -3.0
    Ab[9, n - 1, 2] = np.nan                  # lower triangle: row n-1, column 2
    o = _batched_device(lib, Ab, Bb, 1)
    assert o.rc == 0
    info_lib, _ = _solve_device(lib, Ab[5], Bb[5])
    assert o.info[5] > 0 and o.info[5] == info_lib == n // 2 + 1
    assert o.info[9] == -5
    for b in range(16):
        if b in (5, 9):
            continue
        assert o.info[b] == 0
        assert np.array_equal(o.w[b], healthy.w[b]) and np.array_equal(o.Z[b], healthy.Z[b]), b
    # a NaN in B is a failing pivot too; values only takes the same exits
    Bb[5] = B[5]; Bb[5, 3, 3] = np.nan
    o0 = _batched_device(lib, Ab, Bb, 0)
    assert o0.rc == 0 and o0.info[5] == 4 and o0.info[9] == -5
    assert _solve_device(lib, Ab[5], Bb[5])[0] == 4
    h0 = _batched_device(lib, A, B, 0)
    keep = [b for b in range(16) if b not in (5, 9)]
    assert np.array_equal(o0.w[keep], h0.w[keep]) and not o0.info[keep].any()
    # the Python mirror reports per-problem failures in info, not as an exception
    w, Z, info = hip.eigenpairs_batched(Ab, Bb)
    assert info[5] == 4 and info[9] == -5 and np.array_equal(w[keep], healthy.w[keep])


@pytest.mark.parametrize("n", [5, 17, 64, 128])
def test_batched_degenerate_inputs(hip, n):
    """(d) zero matrix, identity, diagonal, rank one, exactly repeated blocks -- one batch, the bounds of
    tests/test_gpu_path.py::test_degenerate_inputs."""
    lib = hip.load_library()
    rng = np.random.default_rng(n)
    u = rng.uniform(-1, 1, n)
    blk = _sym(np.random.default_rng(3), 5)
    mats = [np.zeros((n, n)), np.eye(n), np.diag(rng.uniform(-1, 1, n)), np.outer(u, u),
            np.kron(np.eye(n // 5 + 1), blk)[:n, :n]]
    A = np.stack(mats)
    B = np.stack([_spd(rng, n) for _ in mats])
    for Bx in (None, B):
        o = _batched_device(lib, A, Bx, 1)
        assert o.rc == 0 and not o.info.any()
        c = 64 if Bx is None else 256
        for b in range(len(mats)):
            Bb = Bx[b] if Bx is not None else None
            scale = max(np.abs(A[b]).max(), 1e-300)
            w_ref = _ref(A[b], Bb)[0]
            w, Z = o.w[b], o.Z[b]
            BZ = Bb @ Z if Bb is not None else Z
            assert np.abs(w - w_ref).max() <= 8 * n * EPS * max(np.abs(w_ref).max(), scale), (n, b)
            assert np.abs(A[b] @ Z - BZ * w).max() <= c * n * EPS * scale, (n, b)
            assert np.abs(Z.T @ BZ - np.eye(n)).max() <= c * n * EPS, (n, b)


@pytest.mark.parametrize("n", [30, 64, 128])
def test_batched_padding_is_left_alone(hip, n):
    """(e) padded lda / ldb / ldz and strides beyond ld * n: the same bits as the compact layout, and the sentinels
    between the columns and between the problems untouched (device and host form)."""
    lib = hip.load_library()
    batch = 5
    A, B = _pairs(77 + n, batch, n)
    compact = _batched_device(lib, A, B, 1)
    lda, ldb, ldz = n + 3, n + 1, n + 5
    sA, sB, sZ = lda * n + 11, ldb * n + 2, ldz * n + 7
    o = _batched_device(lib, A, B, 1, lda=lda, sA=sA, ldb=ldb, sB=sB, ldz=ldz, sZ=sZ)
    assert o.rc == 0 and not o.info.any()
    assert np.array_equal(o.w, compact.w) and np.array_equal(o.Z, compact.Z)

    def padding_mask(size, ld, stride):
        m = np.ones(size, dtype=bool)
        _view(m, batch, n, ld, stride)[...] = False
        return m

    for flat, ld, stride in ((o.Aflat, lda, sA), (o.Bflat, ldb, sB), (o.Zflat, ldz, sZ)):
        pad = flat[padding_mask(flat.size, ld, stride)]
        assert pad.size > 0 and np.all(pad == SENTINEL)
    # host form, strided, called directly
    hA, hB = _pack(A, lda, sA), _pack(B, ldb, sB)
    hA0, hB0 = hA.copy(), hB.copy()
    hZ, hw = np.full(batch * sZ, SENTINEL), np.zeros(batch * n)
    info = np.full(batch, 777, dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.ek_hip_eigenpairs_batched(1, 1, n, batch, hA.ctypes.data_as(dp), lda, sA, hB.ctypes.data_as(dp), ldb, sB,
                                       hw.ctypes.data_as(dp), hZ.ctypes.data_as(dp), ldz, sZ,
                                       info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
    assert rc == 0 and not info.any()
    assert np.array_equal(hA, hA0) and np.array_equal(hB, hB0)
    assert np.array_equal(hw.reshape(batch, n), compact.w)
    assert np.array_equal(_unpack(hZ, batch, n, ldz, sZ), compact.Z)
    assert np.all(hZ[padding_mask(hZ.size, ldz, sZ)] == SENTINEL)


def test_batched_empty_batch(hip):
    """(f) batch = 0 and n = 0: success, nothing touched."""
    lib = hip.load_library()
    info = np.full(4, 777, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    sec = ctypes.c_double(-1.0)
    assert lib.ek_hip_eigenpairs_batched_device(1, 1, 30, 0, None, 30, 900, None, 30, 900, None, None, 30, 900, ip,
                                                ctypes.byref(sec)) == 0
    assert lib.ek_hip_eigenpairs_batched_device(1, 1, 0, 4, None, 1, 1, None, 1, 1, None, None, 1, 1, ip, None) == 0
    assert np.all(info == 777) and sec.value == 0.0
    w, Z, inf = hip.eigenpairs_batched(np.zeros((0, 30, 30)), np.zeros((0, 30, 30)))
    assert w.shape == (0, 30) and Z.shape == (0, 30, 30) and inf.size == 0


def test_batched_more_workgroups_than_fit_the_device(hip):
    """(g) 20 000 problems of order 30 in one launch against the CPU on a seeded sample of 64 of them."""
    lib = hip.load_library()
    n, batch = 30, 20000
    A, B = _pairs(2024, batch, n)
    o = _batched_device(lib, A, B, 1)
    assert o.rc == 0 and not o.info.any()
    sample = np.random.default_rng(64).choice(batch, 64, replace=False)
    for b in sample:
        _check_problem(A[b], B[b], o.w[b], o.Z[b], _ref(A[b], B[b])[0], ("20000", int(b)))


# ------------------------------------------------------------------------------------------------- speed
def _speed(lib, n, batch, nloop):
    """(t_batched, t_loop): best of 3 after a warm-up, device-resident arrays both ways, one process.  t_loop is
    batch / nloop times a loop of ek_hip_solve_device over the first nloop pairs."""
    A, B = _pairs(4000 + n, batch, n)
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    info = np.zeros(batch, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))

        def at(p, b, per):
            return ctypes.c_void_p(p.value + b * per * 8)

        def batched():
            dev.put(dA, hA); dev.put(dB, hB)           # both calls work in place: fresh inputs, outside the clock
            t0 = time.perf_counter()
            rc = lib.ek_hip_eigenpairs_batched_device(1, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n, ip,
                                                      None)
            t = time.perf_counter() - t0
            assert rc == 0 and not info.any()
            return t

        def loop():
            dev.put(dA, hA); dev.put(dB, hB)
            t0 = time.perf_counter()
            for b in range(nloop):
                rc = lib.ek_hip_solve_device(1, n, n, at(dA, b, n * n), n, at(dB, b, n * n), n, at(dw, b, n),
                                             at(dZ, b, n * n), n, None, 0)
                assert rc == 0
            return (time.perf_counter() - t0) * (batch / nloop)

        tb, tl = [], []
        batched(); loop()                               # warm-up
        for _ in range(3):                              # kinds alternated
            tb.append(batched()); tl.append(loop())
    return min(tb), min(tl)


@pytest.mark.parametrize("n,batch,nloop", [(64, 1024, 32), (128, 512, 16)])
def test_batched_beats_the_host_loop_tenfold(hip, n, batch, nloop):
    """Generalized pairs with vectors: t_batched <= t_loop / 10, t_loop being what the parent commit's only way costs
    (a host loop over ek_hip_solve_device, measured on nloop pairs and scaled to the batch).  Under 10 x the batch is
    not running in parallel.  Measured on one MI355X: 805 x (n = 64) and 105 x (n = 128), DESIGN.md 12."""
    lib = hip.load_library()
    t_batched, t_loop = _speed(lib, n, batch, nloop)
    print("n=%d batch=%d: batched %.3f ms (%.1f us per problem, %.0f problems/s), loop %.1f ms (%.1f us per problem), "
          "ratio %.1f" % (n, batch, t_batched * 1e3, t_batched / batch * 1e6, batch / t_batched, t_loop * 1e3,
                          t_loop / batch * 1e6, t_loop / t_batched))
    assert t_batched <= t_loop / 10.0, (t_batched, t_loop)
