"""GPU suite of the variable-order batched entries (ek_hip_eigenpairs_vbatched*): problems of different orders
(0 .. 128) in one call.  The oracle of the contract needs no tolerance: a problem's w, Z, info and in-place images are
the bits ek_hip_eigenpairs_batched_device returns for that pair alone.  Accuracy is checked against SciPy with the bounds
of tests/test_gpu_batched.py; inputs are its seeded _sym / _spd pairs (helpers copied from there).  The speed test
compares one variable call with what the uniform entries offer for the same work: a call per distinct order, and
padding every problem to order 128."""
import ctypes
import time

import numpy as np
import pytest
import scipy.linalg as sl

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (0, 1, 2, 3, 17, 30, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128)
SENTINEL = -7.25e77
_ip = ctypes.POINTER(ctypes.c_int)


# ------------------------------------------------------------------------------- helpers of tests/test_gpu_batched.py
def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


def _view(flat, batch, n, ld, stride):
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


def _batched_device(lib, A, B, jobz):
    """The uniform entry (ek_hip_eigenpairs_batched_device) on compact device images of A[b], B[b]."""
    batch, n = A.shape[0], A.shape[1]
    hA = _pack(A, n, n * n)
    hB = _pack(B, n, n * n) if B is not None else None
    hZ = np.full(max(batch * n * n, 1), SENTINEL)
    hw = np.full(max(batch * n, 1), SENTINEL)
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    o = _Out()
    with _Dev(lib) as dev:
        dA = dev.up(hA)
        dB = dev.up(hB) if B is not None else None
        dw, dZ = dev.up(hw), dev.up(hZ)
        o.rc = lib.ek_hip_eigenpairs_batched_device(0 if B is None else 1, jobz, n, batch, dA, n, n * n, dB, n, n * n,
                                                    dw, dZ if jobz else None, n, n * n, info.ctypes.data_as(_ip), None)
        o.info = info[:batch].copy()
        o.w = dev.down(dw, hw)[:batch * n].reshape(batch, n)
        o.Z = _unpack(dev.down(dZ, hZ), batch, n, n, n * n)
        o.A = _unpack(dev.down(dA, hA), batch, n, n, n * n)
        o.B = _unpack(dev.down(dB, hB), batch, n, n, n * n) if B is not None else None
    return o


def _solve_device(lib, A, B):
    """ek_hip_solve_device on one pair: info."""
    n = A.shape[0]
    with _Dev(lib) as dev:
        dA = dev.up(np.asfortranarray(A))
        dB = dev.up(np.asfortranarray(B)) if B is not None else None
        w, Z = np.zeros(n), np.zeros((n, n), order="F")
        dw, dZ = dev.up(w), dev.up(Z)
        return lib.ek_hip_solve_device(0 if B is None else 1, n, n, dA, n, dB, n, dw, dZ, n, None, 0)


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


# ------------------------------------------------------------------------------------------- the variable call
def _pair(seed, n):
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 0)), np.zeros((0, 0))
    return _sym(rng, n), _spd(rng, n)


def _mixed(seed, orders):
    """One seeded pair per entry of orders."""
    return [_pair(seed * 100003 + i, int(n)) for i, n in enumerate(orders)]


class _Place:
    """Where the problems of a batch lie in one flat buffer per array kind: problem b's n x n matrix column-major with
    ld = max(n, 1) + pad at off[b], `gap` doubles behind every problem (matrices and w)."""

    def __init__(self, orders, pad):
        self.orders = np.asarray(orders, dtype=np.int64)
        self.batch = len(self.orders)
        gap = 5 if pad else 0
        self.ld = (np.maximum(self.orders, 1) + pad).astype(np.int32)
        self.off = np.concatenate(([0], np.cumsum(self.ld * self.orders + gap)))
        self.woff = np.concatenate(([0], np.cumsum(self.orders + gap)))
        self.n32 = self.orders.astype(np.int32)

    def block(self, flat, b):
        n, ld = int(self.orders[b]), int(self.ld[b])
        return flat[self.off[b]:self.off[b] + ld * n].reshape(n, ld)[:, :n]      # [j, i] = element (i, j)

    def fill(self, mats):
        flat = np.full(max(int(self.off[-1]), 1), SENTINEL)
        for b, M in enumerate(mats):
            if M.shape[0]:
                self.block(flat, b)[...] = M.T
        return flat

    def take(self, flat):
        return [self.block(flat, b).T.copy() for b in range(self.batch)]

    def wtake(self, flat):
        return [flat[self.woff[b]:self.woff[b] + self.orders[b]].copy() for b in range(self.batch)]

    def padding(self, flat):
        """What lies between the columns and between the problems."""
        m = np.ones(flat.size, dtype=bool)
        for b in range(self.batch):
            if self.orders[b]:
                self.block(m, b)[...] = False
        return flat[m]

    def wpadding(self, flat):
        m = np.ones(flat.size, dtype=bool)
        for b in range(self.batch):
            m[self.woff[b]:self.woff[b] + self.orders[b]] = False
        return flat[m]

    def pointers(self, base, off):
        return (ctypes.c_void_p * self.batch)(*[base + int(off[b]) * 8 for b in range(self.batch)])


def _vbatched(lib, pairs, problem, jobz, pad=0, host=False):
    """ek_hip_eigenpairs_vbatched_device (host=False) or ek_hip_eigenpairs_vbatched on the pairs (full matrices: both
    triangles as given), every problem in its own region of one buffer per kind.  Returns rc, info and per problem w, Z
    and the images of A and B after the call, plus the flat buffers before and after."""
    pl = _Place([A.shape[0] for A, _ in pairs], pad)
    hA = pl.fill([A for A, _ in pairs])
    hB = pl.fill([B for _, B in pairs]) if problem else None
    hZ = np.full(max(int(pl.off[-1]), 1), SENTINEL)
    hw = np.full(max(int(pl.woff[-1]), 1), SENTINEL)
    info = np.full(pl.batch, 777, dtype=np.int32)
    sec = ctypes.c_double(-1.0)
    o = _Out()
    o.place, o.hA, o.hB = pl, hA.copy(), hB.copy() if problem else None
    ld = pl.ld.ctypes.data_as(_ip)

    def run(fn, bA, bB, bw, bZ):
        return fn(problem, jobz, pl.batch, pl.n32.ctypes.data_as(_ip), pl.pointers(bA, pl.off), ld,
                  pl.pointers(bB, pl.off) if problem else None, ld, pl.pointers(bw, pl.woff),
                  pl.pointers(bZ, pl.off) if jobz else None, ld, info.ctypes.data_as(_ip), ctypes.byref(sec))

    if host:
        o.rc = run(lib.ek_hip_eigenpairs_vbatched, hA.ctypes.data, hB.ctypes.data if problem else 0, hw.ctypes.data,
                   hZ.ctypes.data)
        o.Aflat, o.Bflat, o.wflat, o.Zflat = hA, hB, hw, hZ
    else:
        with _Dev(lib) as dev:
            dA = dev.up(hA)
            dB = dev.up(hB) if problem else None
            dw, dZ = dev.up(hw), dev.up(hZ)
            o.rc = run(lib.ek_hip_eigenpairs_vbatched_device, dA.value, dB.value if problem else 0, dw.value, dZ.value)
            o.Aflat = dev.down(dA, hA)
            o.Bflat = dev.down(dB, hB) if problem else None
            o.wflat, o.Zflat = dev.down(dw, hw), dev.down(dZ, hZ)
    o.seconds = sec.value
    o.info = info.copy()
    o.w, o.Z, o.A = pl.wtake(o.wflat), pl.take(o.Zflat), pl.take(o.Aflat)
    o.B = pl.take(o.Bflat) if problem else None
    return o


_alone_cache = {}


def _alone(lib, key, A, B, problem, jobz):
    """The uniform call on one pair alone: (info, w, Z, lower triangle of dA after, of dB after)."""
    k = (key, problem, jobz)
    if k not in _alone_cache:
        o = _batched_device(lib, A[None], B[None] if problem else None, jobz)
        assert o.rc == 0
        _alone_cache[k] = (int(o.info[0]), o.w[0], o.Z[0], np.tril(o.A[0]), np.tril(o.B[0]) if problem else None)
    return _alone_cache[k]


def _same_as_alone(lib, key, pair, o, b, problem, jobz, what):
    A, B = pair
    n = A.shape[0]
    if n == 0:
        assert o.info[b] == 0, what
        return
    info, w, Z, La, Lb = _alone(lib, key, A, B, problem, jobz)
    assert o.info[b] == info, (what, o.info[b], info)
    assert np.array_equal(np.tril(o.A[b]), La, equal_nan=True), (what, "dA")
    if problem:
        assert np.array_equal(np.tril(o.B[b]), Lb, equal_nan=True), (what, "dB")
    if info == 0:
        assert np.array_equal(o.w[b], w), (what, "w")
        if jobz:
            assert np.array_equal(o.Z[b], Z), (what, "Z")


def _the_batch():
    """Every order of ORDERS three times, and two seeded shuffles of the 48 problems."""
    orders = list(ORDERS) * 3
    pairs = _mixed(7, orders)
    p1 = np.random.default_rng(11).permutation(len(orders))
    p2 = np.random.default_rng(12).permutation(len(orders))
    return pairs, p1, p2


# ------------------------------------------------------------------------------------------------- contract
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
def test_vbatched_bit_identity_with_the_uniform_call(hip, problem, jobz):
    """Every order of ORDERS three times in a seeded shuffle: w, Z, info and the lower triangles left in dA / dB are
    those of ek_hip_eigenpairs_batched_device on the pair alone; a second permutation gives the same bits per problem;
    a batch of equal orders gives the uniform call's bits at every position; host form = device form, inputs
    unchanged."""
    lib = hip.load_library()
    pairs, p1, p2 = _the_batch()
    o = _vbatched(lib, [pairs[i] for i in p1], problem, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    assert o.wflat.size == o.place.woff[-1]           # compact: every slot belongs to a problem
    for b, i in enumerate(p1):
        _same_as_alone(lib, ("batch", int(i)), pairs[i], o, b, problem, jobz, (problem, jobz, b, int(i)))
    if not jobz:
        assert np.all(o.Zflat == SENTINEL)
    # the same problems in another order
    o2 = _vbatched(lib, [pairs[i] for i in p2], problem, jobz)
    assert o2.rc == 0 and not o2.info.any()
    where = {int(i): b for b, i in enumerate(p1)}
    for b2, i in enumerate(p2):
        b = where[int(i)]
        assert np.array_equal(o2.w[b2], o.w[b]) and np.array_equal(o2.Z[b2], o.Z[b]), (b2, int(i))
        assert np.array_equal(np.tril(o2.A[b2]), np.tril(o.A[b]))
        if problem:
            assert np.array_equal(np.tril(o2.B[b2]), np.tril(o.B[b]))
    # all orders equal: the uniform call's bits at every position
    for n in (30, 100):
        same = _mixed(300 + n, [n] * 9)
        A = np.stack([x for x, _ in same])
        B = np.stack([y for _, y in same])
        u = _batched_device(lib, A, B if problem else None, jobz)
        v = _vbatched(lib, same, problem, jobz)
        assert u.rc == 0 and v.rc == 0 and not u.info.any() and not v.info.any()
        for b in range(9):
            assert np.array_equal(v.w[b], u.w[b]), (n, b)
            assert np.array_equal(np.tril(v.A[b]), np.tril(u.A[b])), (n, b)
            if jobz:
                assert np.array_equal(v.Z[b], u.Z[b]), (n, b)
            if problem:
                assert np.array_equal(np.tril(v.B[b]), np.tril(u.B[b])), (n, b)
    # host form: the device form's bits, the inputs as they were
    h = _vbatched(lib, [pairs[i] for i in p1], problem, jobz, host=True)
    assert h.rc == 0 and not h.info.any()
    assert np.array_equal(h.Aflat, h.hA) and (not problem or np.array_equal(h.Bflat, h.hB))
    assert np.array_equal(h.wflat, o.wflat) and np.array_equal(h.Zflat, o.Zflat)
    # ... and through the Python mirror
    As = [pairs[i][0] for i in p1]
    Bs = [pairs[i][1] for i in p1]
    As_in, Bs_in = [x.copy() for x in As], [x.copy() for x in Bs]
    w, Z, info = hip.eigenpairs_vbatched(As, Bs if problem else None, vectors=bool(jobz))
    assert not info.any() and (Z is None) == (not jobz)
    for b in range(len(As)):
        assert np.array_equal(w[b], o.w[b]), b
        if jobz:
            assert np.array_equal(Z[b], o.Z[b]), b
        assert np.array_equal(As[b], As_in[b]) and np.array_equal(Bs[b], Bs_in[b])


@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
def test_vbatched_accuracy_against_scipy(hip, problem, jobz):
    """The same batch against scipy.linalg.eigh with the bounds of tests/test_gpu_batched.py: 4 max(n, 8) eps max|l| on
    eigenvalues, 64 / 256 n eps on residual and orthogonality; every problem of order > 0."""
    lib = hip.load_library()
    pairs, p1, _ = _the_batch()
    batch = [pairs[i] for i in p1]
    o = _vbatched(lib, batch, problem, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    worst = np.zeros(3)
    checked = 0
    for b, (A, B) in enumerate(batch):
        n = A.shape[0]
        if n == 0:
            assert o.w[b].size == 0
            continue
        Bb = B if problem else None
        used = _check_problem(A, Bb, o.w[b], o.Z[b] if jobz else None, _ref(A, Bb)[0], (n, problem, jobz, b))
        worst = np.maximum(worst, used)
        checked += 1
    assert checked == 3 * (len(ORDERS) - 1)
    print("problem=%d jobz=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((problem, jobz) + tuple(worst)))


def test_vbatched_failures_stay_in_their_own_slots(hip):
    """A non-SPD B at one order-100 problem, a NaN in the lower triangle of A at one order-30 problem, a NaN pivot in B
    at one order-33 problem: return 0, the infos of ek_hip_solve_device for those pairs / -5, every other problem
    bit-identical to the healthy batch; values only takes the same exits; the host form leaves a failed problem's w
    and Z as they were."""
    lib = hip.load_library()
    pairs, p1, _ = _the_batch()
    batch = [pairs[i] for i in p1]
    orders = [A.shape[0] for A, _ in batch]
    b100, b30, b33 = orders.index(100), orders.index(30), orders.index(33)
    healthy = _vbatched(lib, batch, 1, 1)
    assert healthy.rc == 0 and not healthy.info.any()
    bad = [(A.copy(), B.copy()) for A, B in batch]
    bad[b100][1][50, 50] = -3.0
    bad[b30][0][29, 2] = np.nan                      # lower triangle: row n-1, column 2
    bad[b33][1][3, 3] = np.nan
    failing = (b100, b30, b33)
    for jobz in (1, 0):
        o = _vbatched(lib, bad, 1, jobz)
        h = healthy if jobz else _vbatched(lib, batch, 1, 0)
        assert o.rc == 0
        assert o.info[b100] == _solve_device(lib, *bad[b100]) == 51
        assert o.info[b33] == _solve_device(lib, *bad[b33]) == 4
        assert o.info[b30] == -5
        for b in range(len(batch)):
            if b in failing:
                continue
            assert o.info[b] == 0
            assert np.array_equal(o.w[b], h.w[b]) and np.array_equal(o.Z[b], h.Z[b]), (jobz, b)
            assert np.array_equal(np.tril(o.A[b]), np.tril(h.A[b])), (jobz, b)
            assert np.array_equal(np.tril(o.B[b]), np.tril(h.B[b])), (jobz, b)
        # a failed problem's bits are the uniform call's too (info and what it left in dA / dB)
        for b in failing:
            _same_as_alone(lib, ("bad", b), bad[b], o, b, 1, jobz, ("failed", jobz, b))
        # no eigenvalue and no vector was written for them
        for b in failing:
            assert np.all(o.w[b] == SENTINEL) and np.all(o.Z[b] == SENTINEL)
    hf = _vbatched(lib, bad, 1, 1, host=True)
    assert hf.rc == 0 and np.array_equal(hf.info, o.info)
    for b in range(len(batch)):
        if b in failing:
            assert np.all(hf.w[b] == SENTINEL) and np.all(hf.Z[b] == SENTINEL)
        else:
            assert np.array_equal(hf.w[b], healthy.w[b]) and np.array_equal(hf.Z[b], healthy.Z[b]), b
    # the Python mirror reports per-problem failures in info, not as an exception
    w, Z, info = hip.eigenpairs_vbatched([A for A, _ in bad], [B for _, B in bad])
    assert np.array_equal(info, o.info)


@pytest.mark.parametrize("host", [False, True])
def test_vbatched_isolation(hip, host):
    """Each problem in its own padded region (ld = n + 3, sentinels between the columns and between the problems, NaN
    in all strictly upper triangles of A and B): the compact batch's bits, every sentinel and every upper-triangle NaN
    still there bit for bit."""
    lib = hip.load_library()
    pairs, p1, _ = _the_batch()
    batch = [pairs[i] for i in p1]
    compact = _vbatched(lib, batch, 1, 1)
    assert compact.rc == 0 and not compact.info.any()
    nan = []
    for A, B in batch:
        iu = np.triu_indices(A.shape[0], 1)
        An, Bn = A.copy(), B.copy()
        An[iu] = np.nan
        Bn[iu] = np.nan
        nan.append((An, Bn))
    o = _vbatched(lib, nan, 1, 1, pad=3, host=host)
    assert o.rc == 0 and not o.info.any()
    pl = o.place
    assert np.all(pl.ld == np.maximum(pl.orders, 1) + 3)
    for b in range(len(batch)):
        assert np.array_equal(o.w[b], compact.w[b]) and np.array_equal(o.Z[b], compact.Z[b]), b
        if not host:
            assert np.array_equal(np.tril(o.A[b]), np.tril(compact.A[b])), b
            assert np.array_equal(np.tril(o.B[b]), np.tril(compact.B[b])), b
        iu = np.triu_indices(pl.orders[b], 1)
        for after, before in ((o.A[b], nan[b][0]), (o.B[b], nan[b][1])):
            assert np.array_equal(after[iu].view(np.uint64), before[iu].view(np.uint64)), b
            assert np.isnan(after[iu]).all()
    for flat in (o.Aflat, o.Bflat, o.Zflat):
        padding = pl.padding(flat)
        assert padding.size > 0 and np.all(padding == SENTINEL)
    wpad = pl.wpadding(o.wflat)
    assert wpad.size > 0 and np.all(wpad == SENTINEL)
    if host:                                          # the host form leaves A and B as a whole alone
        assert np.array_equal(o.Aflat.view(np.uint64), o.hA.view(np.uint64))
        assert np.array_equal(o.Bflat.view(np.uint64), o.hB.view(np.uint64))


def test_vbatched_empty_batch_and_empty_problems(hip):
    """batch = 0: nothing touched; a batch of empty problems only: info 0; NULL entries where the order is 0."""
    lib = hip.load_library()
    info = np.full(4, 777, dtype=np.int32)
    sec = ctypes.c_double(-1.0)
    assert lib.ek_hip_eigenpairs_vbatched_device(1, 1, 0, None, None, None, None, None, None, None, None, None,
                                                 ctypes.byref(sec)) == 0
    assert sec.value == 0.0
    w, Z, inf = hip.eigenpairs_vbatched([], [])
    assert w == [] and Z == [] and inf.size == 0
    A, B = _pair(5, 30)
    E = np.zeros((0, 0))
    w, Z, inf = hip.eigenpairs_vbatched([E, A, E], [E, B, E])
    assert not inf.any() and w[0].size == 0 and Z[2].shape == (0, 0)
    _check_problem(A, B, w[1], Z[1], _ref(A, B)[0], "between two empty problems")
    assert np.all(info == 777)


def test_vbatched_more_workgroups_than_fit_the_device(hip):
    """20 000 problems with orders drawn from 1 .. 40 in one call against the CPU on a seeded sample of 64."""
    lib = hip.load_library()
    batch = 20000
    orders = np.random.default_rng(2025).integers(1, 41, batch)
    pairs = _mixed(9, orders)
    o = _vbatched(lib, pairs, 1, 1)
    assert o.rc == 0 and not o.info.any()
    sample = np.random.default_rng(64).choice(batch, 64, replace=False)
    for b in sample:
        A, B = pairs[b]
        _check_problem(A, B, o.w[b], o.Z[b], _ref(A, B)[0], ("20000", int(b), A.shape[0]))


# ------------------------------------------------------------------------------------------------- speed
def _speed(lib):
    """(t_var, t_grouped, t_pad): best of 3 after a warm-up, the kinds alternated in one process, device-resident
    arrays, inputs refreshed outside the clock (all three work in place)."""
    batch = 2048
    orders = np.random.default_rng(2048).integers(8, 129, batch)
    pairs = _mixed(13, orders)
    pl = _Place(orders, 0)
    hA, hB = pl.fill([A for A, _ in pairs]), pl.fill([B for _, B in pairs])
    # the grouped copy: the problems of one order behind each other, order after order
    by_order = np.argsort(orders, kind="stable")
    gl = _Place(orders[by_order], 0)
    gA, gB = gl.fill([pairs[b][0] for b in by_order]), gl.fill([pairs[b][1] for b in by_order])
    distinct, first, counts = np.unique(orders[by_order], return_index=True, return_counts=True)
    # the padded batch: 2 048 seeded pairs of order 128
    rng = np.random.default_rng(128)
    pA = _pack(np.stack([_sym(rng, 128) for _ in range(batch)]), 128, 128 * 128)
    pB = _pack(np.stack([_spd(rng, 128) for _ in range(batch)]), 128, 128 * 128)
    info = np.zeros(batch, dtype=np.int32)
    ip = info.ctypes.data_as(_ip)
    with _Dev(lib) as dev:
        dA, dB, dgA, dgB, dpA, dpB = (dev.up(x) for x in (hA, hB, gA, gB, pA, pB))
        dw, dZ = dev.up(np.zeros(batch * 128)), dev.up(np.zeros(batch * 128 * 128))
        n32, ld = pl.n32.ctypes.data_as(_ip), pl.ld.ctypes.data_as(_ip)
        tA, tB = pl.pointers(dA.value, pl.off), pl.pointers(dB.value, pl.off)
        tw, tZ = pl.pointers(dw.value, pl.woff), pl.pointers(dZ.value, pl.off)

        def at(p, off):
            return ctypes.c_void_p(p.value + int(off) * 8)

        def var():
            dev.put(dA, hA); dev.put(dB, hB)
            t0 = time.perf_counter()
            rc = lib.ek_hip_eigenpairs_vbatched_device(1, 1, batch, n32, tA, ld, tB, ld, tw, tZ, ld, ip, None)
            t = time.perf_counter() - t0
            assert rc == 0 and not info.any()
            return t

        def grouped():
            dev.put(dgA, gA); dev.put(dgB, gB)
            t = 0.0
            for n, f, c in zip(distinct, first, counts):
                n, c = int(n), int(c)
                off, woff = gl.off[f], gl.woff[f]
                t0 = time.perf_counter()
                rc = lib.ek_hip_eigenpairs_batched_device(1, 1, n, c, at(dgA, off), n, n * n, at(dgB, off), n, n * n,
                                                          at(dw, woff), at(dZ, off), n, n * n, ip, None)
                t += time.perf_counter() - t0
                assert rc == 0 and not info[:c].any()
            return t

        def pad():
            dev.put(dpA, pA); dev.put(dpB, pB)
            t0 = time.perf_counter()
            rc = lib.ek_hip_eigenpairs_batched_device(1, 1, 128, batch, dpA, 128, 128 * 128, dpB, 128, 128 * 128, dw, dZ,
                                                      128, 128 * 128, ip, None)
            t = time.perf_counter() - t0
            assert rc == 0 and not info.any()
            return t

        tv, tg, tp = [], [], []
        var(); grouped(); pad()                         # warm-up
        for _ in range(3):                              # kinds alternated
            tv.append(var()); tg.append(grouped()); tp.append(pad())
    return min(tv), min(tg), min(tp), len(distinct)


def test_vbatched_beats_a_call_per_order_and_padding(hip):
    """Generalized with vectors, 2 048 problems with orders drawn uniformly from 8 .. 128: t_var <= t_grouped / 3
    (t_grouped: one uniform call per distinct order, what the parent commit offers) and t_var <= t_pad (one uniform
    call of 2 048 pairs of order 128: every workgroup does at least the variable call's work).  Under a third of
    t_grouped the classes run one problem after another or the long problems start last; above t_pad the scheduling
    lost more than the shorter problems saved.  Measured values: DESIGN.md 13."""
    lib = hip.load_library()
    t_var, t_grouped, t_pad, distinct = _speed(lib)
    print("2048 problems of order 8..128 (%d distinct): variable %.3f ms, call per order %.3f ms (ratio %.1f), "
          "padded to 128 %.3f ms (ratio %.2f)" % (distinct, t_var * 1e3, t_grouped * 1e3, t_grouped / t_var,
                                                   t_pad * 1e3, t_pad / t_var))
    assert t_var <= t_grouped / 3.0, (t_var, t_grouped)
    assert t_var <= t_pad, (t_var, t_pad)
