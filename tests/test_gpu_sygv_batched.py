"""GPU suite of the batched entries for DSYGV's problem types 2 and 3 (ek_hip_sygv_batched*, ek_hip_sygv_vbatched*):
A B x = l x and B A x = l x for many pencils of order <= 128 in one launch.  The reference is SciPy on the CPU
(scipy.linalg.eigh(A, B, type=itype, lower=True)) on the seeded pairs of tests/test_gpu_batched.py; the bounds are that
suite's (4 max(n, 8) eps on eigenvalues, 256 n eps on residual and orthogonality) with the normalisations of the type:

  residual       max_j |M z_j - w_j z_j|_2 / (max|A| |B|_2 |z_j|_2),  M = A B (type 2), B A (type 3)
  orthogonality  max|Z^T B Z - I| (type 2),  max|(L^-1 Z)^T (L^-1 Z) - I| (type 3, B = L L^T: Z^T B^-1 Z = I)

and for the hard pencils of tests/batched_cases.py the hard suite's rule: residual and orthogonality <= 4 max(LAPACK's
own on the same pencil, 16 n eps).  Type 3's orthogonality of those pencils is asserted twice.  With LAPACK's factor of
B, as for the random pairs, against 4 max(LAPACK's own, 16 n eps, n eps cond2(B)): for cond2(B) <= 16 (A = B and the
banded pair: 1.2 .. 2.4, asserted) the third term is below the floor and this is the rule as it stands; for cond_b:1e6
and cond_b:1e10 it is not, because two factors of B that are both exact to the last bit of B lie cond(B) eps apart, so
LAPACK's factor applied to anybody else's Z measures that distance (L1^-1 L2 - I is 2.8e-12 at cond(B) = 1e6 and 7.5e-8
at 1e10, order 3, NumPy's factor against a right-looking one on the CPU) and the rule can be met only by a Cholesky
that is LAPACK's to the bit.  Measured on one MI355X, type 3: 1.7e-12 .. 8.3e-12 at 1e6 (4.6 to 28 times the rule) and
3.6e-8 .. 1.3e-7 at 1e10 (1 600 to 11 600 times the rule), at most 0.005 of the limit with n eps cond2(B) in it; the
well-conditioned pencils use 0.026 of the rule.  And with the factor the library itself left in dB, which is what
LAPACK's own figure is for LAPACK's Z, against the rule as it stands, that factor held to max|L L^T - B| <= 16 n eps
max|B|: at most 0.38 of the rule.  Type 2 needs no factor (Z^T B Z) and uses up to 0.93 of the rule (cond_b:1e10 at
order 17: 9.4e-8 where LAPACK's own is 2.5e-8).  The contract is the batched suite's: the same bits wherever a problem
sits and in every form, untouched upper triangles and padding, failures in their own slots; and between the types:
types 2 and 3 share w and the images left in dA and dB bit for bit, Z3 = B Z2 to rounding, and itype 1 is problem 1 to
the bit.

Largest shares of the bounds used on one MI355X (all orders, 24 pairs each; eigenvalues / residual / orthogonality):
random pairs 0.204 / 0.009 / 0.010, Z3 = B Z2 0.004, hard pencils 0.084 / 0.014 / 0.93."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
from test_gpu_batched import _pairs
from test_gpu_vbatched import SENTINEL, _Dev, _Out, _Place, _mixed, _pack, _unpack, _view

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (1, 2, 3, 17, 30, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128)
HARD_ORDERS = (3, 17, 30, 32, 33, 64, 65, 100, 128)
HARD_CASES = ("cond_b:1e6", "cond_b:1e10", "a_equals_b", "band5_band5")
_ip = ctypes.POINTER(ctypes.c_int)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _device(lib, first, A, B, jobz, lda=None, sA=None, ldb=None, sB=None, ldz=None, sZ=None,
            entry="ek_hip_sygv_batched_device"):
    """`entry` (ek_hip_sygv_batched_device with first = itype, or ek_hip_eigenpairs_batched_device with first =
    problem) on strided device images of A[b], B[b] (full matrices: both triangles as given).  Returns rc, info, w, Z,
    the images of A and B after the call and the flat buffers before and after."""
    batch, n = A.shape[0], A.shape[1]
    lda = lda or n; ldb = ldb or n; ldz = ldz or n
    sA = sA or lda * n; sB = sB or ldb * n; sZ = sZ or ldz * n
    hA, hB = _pack(A, lda, sA), _pack(B, ldb, sB)
    hZ = np.full(max(batch * sZ, 1), SENTINEL)
    hw = np.full(max(batch * n, 1), SENTINEL)
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    o = _Out()
    with _Dev(lib) as dev:
        dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
        sec = ctypes.c_double(-1.0)
        o.rc = getattr(lib, entry)(first, jobz, n, batch, dA, lda, sA, dB, ldb, sB, dw, dZ if jobz else None, ldz, sZ,
                                   info.ctypes.data_as(_ip), ctypes.byref(sec))
        o.seconds = sec.value
        o.info = info[:batch].copy()
        o.wflat, o.Zflat = dev.down(dw, hw), dev.down(dZ, hZ)
        o.Aflat, o.Bflat = dev.down(dA, hA), dev.down(dB, hB)
    o.hA, o.hB = hA, hB
    o.w = o.wflat[:batch * n].reshape(batch, n)
    o.Z = _unpack(o.Zflat, batch, n, ldz, sZ)
    o.A = _unpack(o.Aflat, batch, n, lda, sA)
    o.B = _unpack(o.Bflat, batch, n, ldb, sB)
    return o


def _variable(lib, itype, pairs, jobz, pad=0, host=False):
    """ek_hip_sygv_vbatched_device (host=False) or ek_hip_sygv_vbatched on the pairs, every problem in its own region of
    one buffer per kind (tests/test_gpu_vbatched.py::_Place)."""
    pl = _Place([A.shape[0] for A, _ in pairs], pad)
    hA, hB = pl.fill([A for A, _ in pairs]), pl.fill([B for _, B in pairs])
    hZ = np.full(max(int(pl.off[-1]), 1), SENTINEL)
    hw = np.full(max(int(pl.woff[-1]), 1), SENTINEL)
    info = np.full(pl.batch, 777, dtype=np.int32)
    o = _Out()
    o.place, o.hA, o.hB = pl, hA.copy(), hB.copy()
    ld = pl.ld.ctypes.data_as(_ip)

    def run(fn, bA, bB, bw, bZ):
        return fn(itype, jobz, pl.batch, pl.n32.ctypes.data_as(_ip), pl.pointers(bA, pl.off), ld,
                  pl.pointers(bB, pl.off), ld, pl.pointers(bw, pl.woff), pl.pointers(bZ, pl.off) if jobz else None, ld,
                  info.ctypes.data_as(_ip), None)

    if host:
        o.rc = run(lib.ek_hip_sygv_vbatched, hA.ctypes.data, hB.ctypes.data, hw.ctypes.data, hZ.ctypes.data)
        o.Aflat, o.Bflat, o.wflat, o.Zflat = hA, hB, hw, hZ
    else:
        with _Dev(lib) as dev:
            dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
            o.rc = run(lib.ek_hip_sygv_vbatched_device, dA.value, dB.value, dw.value, dZ.value)
            o.Aflat, o.Bflat = dev.down(dA, hA), dev.down(dB, hB)
            o.wflat, o.Zflat = dev.down(dw, hw), dev.down(dZ, hZ)
    o.info = info.copy()
    o.w, o.Z, o.A, o.B = pl.wtake(o.wflat), pl.take(o.Zflat), pl.take(o.Aflat), pl.take(o.Bflat)
    return o


_ref_cache = {}


def _ref(key, itype, A, B):
    """scipy.linalg.eigh(A, B, type=itype, lower=True), computed once per (key, itype) and never modified."""
    k = (key, itype)
    if k not in _ref_cache:
        w, Z = sl.eigh(A, B, type=itype, lower=True)
        w.setflags(write=False); Z.setflags(write=False)
        _ref_cache[k] = (w, Z)
    return _ref_cache[k]


def _quantities(itype, A, B, w, Z, L=None):
    """(residual, orthogonality) with the normalisations of the module docstring, as plain numbers (not in units).
    L: the Cholesky factor that type 3's orthogonality is measured with (None: LAPACK's, np.linalg.cholesky(B))."""
    n = A.shape[0]
    MZ = A @ (B @ Z) if itype == 2 else B @ (A @ Z)
    R = MZ - Z * w
    scale = np.abs(A).max() * np.linalg.norm(B, 2)
    res = (np.linalg.norm(R, axis=0) / (scale * np.linalg.norm(Z, axis=0))).max()
    if itype == 2:
        G = Z.T @ (B @ Z)
    else:
        Y = sl.solve_triangular(np.linalg.cholesky(B) if L is None else L, Z, lower=True)
        G = Y.T @ Y
    return res, np.abs(G - np.eye(n)).max()


# ------------------------------------------------------------------------------------------------- 1: accuracy
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", ORDERS)
def test_sygv_batched_accuracy_against_scipy(hip, n, itype, jobz):
    """24 pairs of one order in one launch against scipy.linalg.eigh(A, B, type=itype).  An entry that forwards to
    type 1 fails here: the eigenvalues are those of another problem."""
    lib = hip.load_library()
    batch = 24
    A, B = _pairs(1000 + n, batch, n)
    o = _device(lib, itype, A, B, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    worst = np.zeros(3)
    fails = []
    for b in range(batch):
        w_ref = _ref(("pairs", n, b), itype, A[b], B[b])[0]
        tol_w = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
        err = np.abs(o.w[b] - w_ref).max()
        worst[0] = max(worst[0], err / tol_w)
        if not np.all(np.diff(o.w[b]) >= 0):
            fails.append((b, "w not ascending"))
        if not err <= tol_w:
            fails.append((b, "eigenvalues", err, tol_w))
        if jobz:
            res, orth = _quantities(itype, A[b], B[b], o.w[b], o.Z[b])
            lim = 256 * n * EPS
            worst[1:] = np.maximum(worst[1:], (res / lim, orth / lim))
            if not res <= lim:
                fails.append((b, "residual", res, lim))
            if not orth <= lim:
                fails.append((b, "orthogonality", orth, lim))
    print("n=%d itype=%d jobz=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, itype, jobz) + tuple(worst)))
    assert not fails, fails
    if not jobz:
        assert np.all(o.Zflat == SENTINEL)


# ------------------------------------------------------------------------------------------------- 2: between the types
@pytest.mark.parametrize("n", ORDERS)
def test_sygv_batched_invariants_between_the_types(hip, n):
    """The same batch through types 1, 2 and 3: w and the image left in dA of types 2 and 3 are the same bits, dB is
    type 1's L, Z3 = B Z2 to rounding, and itype 1 is ek_hip_eigenpairs_batched_device(problem = 1) bit for bit, with
    and without vectors."""
    lib = hip.load_library()
    batch = 24
    A, B = _pairs(1000 + n, batch, n)
    t = {(i, j): _device(lib, i, A, B, j) for i in (1, 2, 3) for j in (0, 1)}
    for o in t.values():
        assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    for j in (0, 1):
        assert np.array_equal(_bits(t[2, j].wflat), _bits(t[3, j].wflat)), ("w of types 2 and 3", j)
        assert np.array_equal(_bits(t[2, j].Aflat), _bits(t[3, j].Aflat)), ("dA of types 2 and 3", j)
        for i in (2, 3):
            assert np.array_equal(_bits(t[i, j].Bflat), _bits(t[1, j].Bflat)), ("dB against type 1's L", i, j)
            assert np.array_equal(_bits(t[i, j].wflat), _bits(t[i, 1].wflat)), ("values only gives another w", i)
            assert np.array_equal(_bits(t[i, j].Aflat), _bits(t[i, 1].Aflat)), ("values only leaves another dA", i)
        p = _device(lib, 1, A, B, j, entry="ek_hip_eigenpairs_batched_device")
        assert p.rc == 0
        assert np.array_equal(t[1, j].info, p.info)
        for name in ("wflat", "Zflat", "Aflat", "Bflat"):
            assert np.array_equal(_bits(getattr(t[1, j], name)), _bits(getattr(p, name))), ("itype 1", j, name)
    worst = 0.0
    for b in range(batch):
        Z2, Z3 = t[2, 1].Z[b], t[3, 1].Z[b]
        worst = max(worst, np.abs(B[b] @ Z2 - Z3).max() / np.abs(Z3).max())
    print("n=%d: max|B Z2 - Z3| / max|Z3| uses %.4f of 256 n eps" % (n, worst / (256 * n * EPS)))
    assert worst <= 256 * n * EPS, (worst, 256 * n * EPS)
    assert not np.array_equal(t[2, 1].wflat, t[1, 1].wflat)       # another problem than type 1's


# ------------------------------------------------------------------------------------------------- 3: the same bits
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [30, 64, 100])
def test_sygv_batched_bit_identity_wherever_a_problem_sits(hip, n, itype):
    """The same pair alone, at positions 0, 7 and last of batches of 8 and 300, and through the host form."""
    lib = hip.load_library()
    A1, B1 = _pairs(7 * n + itype, 1, n)
    alone, alone0 = _device(lib, itype, A1, B1, 1), _device(lib, itype, A1, B1, 0)
    assert alone.rc == 0 and alone.info[0] == 0 and alone0.rc == 0 and alone0.info[0] == 0
    for batch in (8, 300):
        Af, Bf = _pairs(99 + batch, batch, n)
        for pos in sorted({0, 7, batch - 1}):
            A, B = Af.copy(), Bf.copy()
            A[pos], B[pos] = A1[0], B1[0]
            o = _device(lib, itype, A, B, 1)
            assert o.rc == 0 and not o.info.any()
            assert np.array_equal(_bits(o.w[pos]), _bits(alone.w[0])), (batch, pos)
            assert np.array_equal(_bits(o.Z[pos]), _bits(alone.Z[0])), (batch, pos)
            assert np.array_equal(_bits(np.tril(o.A[pos])), _bits(np.tril(alone.A[0]))), (batch, pos)
            assert np.array_equal(_bits(np.tril(o.B[pos])), _bits(np.tril(alone.B[0]))), (batch, pos)
            o0 = _device(lib, itype, A, B, 0)
            assert np.array_equal(_bits(o0.w[pos]), _bits(alone0.w[0])), (batch, pos)
    A, B = _pairs(5, 8, n)
    A[3], B[3] = A1[0], B1[0]
    A_in, B_in = A.copy(), B.copy()
    w, Z, info = hip.sygv_batched(A, B, itype=itype)
    assert not info.any()
    assert np.array_equal(_bits(w[3]), _bits(alone.w[0])) and np.array_equal(_bits(Z[3]), _bits(alone.Z[0]))
    assert np.array_equal(_bits(A), _bits(A_in)) and np.array_equal(_bits(B), _bits(B_in))
    w0, Z0, info0 = hip.sygv_batched(A, B, itype=itype, vectors=False)
    assert Z0 is None and not info0.any() and np.array_equal(_bits(w0[3]), _bits(alone0.w[0]))
    # the host form of the variable call on the same pairs
    wv, Zv, infov = hip.sygv_vbatched(list(A), list(B), itype=itype)
    assert not infov.any()
    for b in range(8):
        assert np.array_equal(_bits(wv[b]), _bits(w[b])) and np.array_equal(_bits(Zv[b]), _bits(Z[b])), b
    assert np.array_equal(_bits(A), _bits(A_in)) and np.array_equal(_bits(B), _bits(B_in))


@pytest.mark.parametrize("itype", [2, 3])
def test_sygv_vbatched_gives_the_uniform_calls_bits(hip, itype):
    """One ek_hip_sygv_vbatched_device call of 512 seeded orders 1 .. 128: every problem's info, w, Z and the lower
    triangles left in dA and dB are those of ek_hip_sygv_batched_device on the pair alone."""
    lib = hip.load_library()
    orders = np.random.default_rng(512 + itype).integers(1, 129, 512)
    pairs = _mixed(40 + itype, orders)
    o = _variable(lib, itype, pairs, 1)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert len(set(int(k) for k in orders)) >= 100
    fails = []
    for b, (A, B) in enumerate(pairs):
        u = _device(lib, itype, A[None], B[None], 1)
        assert u.rc == 0 and u.info[0] == 0
        for name, x, y in (("w", o.w[b], u.w[0]), ("Z", o.Z[b], u.Z[0]), ("dA", np.tril(o.A[b]), np.tril(u.A[0])),
                           ("dB", np.tril(o.B[b]), np.tril(u.B[0]))):
            if not np.array_equal(_bits(x), _bits(y)):
                fails.append((b, int(orders[b]), name))
    assert not fails, fails[:20]
    # what lies between the problems stays alone, and the strictly upper triangles are the caller's
    assert np.all(o.place.padding(o.Zflat) == SENTINEL) and np.all(o.place.wpadding(o.wflat) == SENTINEL)
    for b in (0, 255, 511):
        iu = np.triu_indices(int(orders[b]), 1)
        assert np.array_equal(_bits(o.A[b][iu]), _bits(pairs[b][0][iu]))
        assert np.array_equal(_bits(o.B[b][iu]), _bits(pairs[b][1][iu]))


# ------------------------------------------------------------------------------------------------- 4: what is not the call's
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [30, 64, 128])
def test_sygv_batched_leaves_alone_what_is_not_its_own(hip, n, itype):
    """NaN in the strictly upper triangles of A and B is never read and survives bit for bit; with ld > n and
    stride > ld n the sentinels between columns and between problems of A, B and Z come back as they were; the host
    forms leave A and B bit for bit."""
    lib = hip.load_library()
    batch = 5
    A, B = _pairs(31 + n + itype, batch, n)
    clean = _device(lib, itype, A, B, 1)
    assert clean.rc == 0 and not clean.info.any()
    An, Bn = A.copy(), B.copy()
    iu = np.triu_indices(n, 1)
    An[:, iu[0], iu[1]] = np.nan
    Bn[:, iu[0], iu[1]] = np.nan
    o = _device(lib, itype, An, Bn, 1)
    assert o.rc == 0 and not o.info.any()
    assert np.array_equal(_bits(o.w), _bits(clean.w)) and np.array_equal(_bits(o.Z), _bits(clean.Z))
    for after, before in ((o.A, An), (o.B, Bn)):
        assert np.array_equal(_bits(after[:, iu[0], iu[1]]), _bits(before[:, iu[0], iu[1]]))
        assert np.isnan(after[:, iu[0], iu[1]]).all()
    L = np.tril(o.B[2])
    assert np.abs(L @ L.T - B[2]).max() <= 16 * n * EPS * np.abs(B[2]).max()
    # padding, device form
    lda, ldb, ldz = n + 3, n + 1, n + 5
    sA, sB, sZ = lda * n + 11, ldb * n + 2, ldz * n + 7
    p = _device(lib, itype, A, B, 1, lda=lda, sA=sA, ldb=ldb, sB=sB, ldz=ldz, sZ=sZ)
    assert p.rc == 0 and not p.info.any()
    assert np.array_equal(_bits(p.w), _bits(clean.w)) and np.array_equal(_bits(p.Z), _bits(clean.Z))

    def padding_mask(size, ld, stride):
        m = np.ones(size, dtype=bool)
        _view(m, batch, n, ld, stride)[...] = False
        return m

    for flat, ld, stride in ((p.Aflat, lda, sA), (p.Bflat, ldb, sB), (p.Zflat, ldz, sZ)):
        pad = flat[padding_mask(flat.size, ld, stride)]
        assert pad.size > 0 and np.all(pad == SENTINEL)
    # host form, strided, called directly: inputs untouched, Z's padding untouched
    hA, hB = _pack(An, lda, sA), _pack(Bn, ldb, sB)
    hA0, hB0 = hA.copy(), hB.copy()
    hZ, hw = np.full(batch * sZ, SENTINEL), np.zeros(batch * n)
    info = np.full(batch, 777, dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.ek_hip_sygv_batched(itype, 1, n, batch, hA.ctypes.data_as(dp), lda, sA, hB.ctypes.data_as(dp), ldb, sB,
                                 hw.ctypes.data_as(dp), hZ.ctypes.data_as(dp), ldz, sZ, info.ctypes.data_as(_ip), None)
    assert rc == 0 and not info.any()
    assert np.array_equal(_bits(hA), _bits(hA0)) and np.array_equal(_bits(hB), _bits(hB0))
    assert np.array_equal(_bits(hw.reshape(batch, n)), _bits(clean.w))
    assert np.array_equal(_bits(_unpack(hZ, batch, n, ldz, sZ)), _bits(clean.Z))
    assert np.all(hZ[padding_mask(hZ.size, ldz, sZ)] == SENTINEL)
    # host form of the variable call, padded: the same
    pairs = [(An[b], Bn[b]) for b in range(batch)]
    v = _variable(lib, itype, pairs, 1, pad=3, host=True)
    assert v.rc == 0 and not v.info.any()
    assert np.array_equal(_bits(v.Aflat), _bits(v.hA)) and np.array_equal(_bits(v.Bflat), _bits(v.hB))
    assert np.all(v.place.padding(v.Zflat) == SENTINEL)
    for b in range(batch):
        assert np.array_equal(_bits(v.w[b]), _bits(clean.w[b])) and np.array_equal(_bits(v.Z[b]), _bits(clean.Z[b])), b


# ------------------------------------------------------------------------------------------------- 5: failures
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [30, 100])
def test_sygv_batched_failures_stay_in_their_own_slots(hip, n, itype):
    """Problem 5 with a B whose pivot n / 2 + 1 is not positive, problem 9 with a NaN and problem 12 with +Inf in A's
    lower triangle: return 0, info k (type 1's for that B), -5 and -5, and outside those three problems' slots every
    output is the clean batch's bit for bit."""
    lib = hip.load_library()
    batch, spoiled = 16, (5, 9, 12)
    A, B = _pairs(200 + n + itype, batch, n)
    clean = _device(lib, itype, A, B, 1)
    assert clean.rc == 0 and not clean.info.any()
    Ab, Bb = A.copy(), B.copy()
    Bb[5, n // 2, n // 2] = -3.0
    Ab[9, n - 1, 2] = np.nan                   # lower triangle: row n-1, column 2
    Ab[12, n // 3, 0] = np.inf
    keep = np.array([b for b in range(batch) if b not in spoiled])
    type1 = _device(lib, 1, Ab, Bb, 1, entry="ek_hip_eigenpairs_batched_device")
    for jobz in (1, 0):
        o = _device(lib, itype, Ab, Bb, jobz)
        ref = clean if jobz else _device(lib, itype, A, B, 0)
        assert o.rc == 0
        assert o.info[5] == n // 2 + 1 == type1.info[5], (o.info[5], type1.info[5])
        assert o.info[9] == -5 and o.info[12] == -5, o.info
        assert not o.info[keep].any()
        assert np.array_equal(_bits(o.w[keep]), _bits(ref.w[keep]))
        assert np.array_equal(_bits(o.Z[keep]), _bits(ref.Z[keep]))
        assert np.array_equal(_bits(o.A[keep]), _bits(ref.A[keep]))
        assert np.array_equal(_bits(o.B[keep]), _bits(ref.B[keep]))
    # the Python mirrors report per-problem failures in info, not as an exception
    w, Z, info = hip.sygv_batched(Ab, Bb, itype=itype)
    assert info[5] == n // 2 + 1 and info[9] == -5 and info[12] == -5 and not info[keep].any()
    assert np.array_equal(_bits(w[keep]), _bits(clean.w[keep])) and np.array_equal(_bits(Z[keep]), _bits(clean.Z[keep]))
    wv, Zv, infov = hip.sygv_vbatched(list(Ab), list(Bb), itype=itype)
    assert np.array_equal(infov, info)
    for b in keep:
        assert np.array_equal(_bits(wv[b]), _bits(clean.w[b])) and np.array_equal(_bits(Zv[b]), _bits(clean.Z[b])), b


# ------------------------------------------------------------------------------------------------- 6: hard pencils
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", HARD_ORDERS)
def test_sygv_batched_hard_pencils(hip, n, itype):
    """cond(B) = 1e6 and 1e10, A = B, banded pencils (tests/batched_cases.py) and, from order 14, the Hilbert B, all in
    one launch: eigenvalues within 4 max(n, 8) eps max|w_ref| of SciPy's with no cond(B) factor, residual and
    orthogonality within 4 max(LAPACK's own, 16 n eps); the Hilbert B fails with the pivot type 1 reports.  Type 3's
    orthogonality: with the library's own factor against that rule, and with LAPACK's factor against the rule with
    n eps cond2(B) beside the floor, which is the rule itself wherever cond2(B) <= 16 (module docstring)."""
    lib = hip.load_library()
    cases = [bc.make(name, n) for name in HARD_CASES]
    if n >= 14:
        cases.append(bc.make("hilbert_b", n))
    A, B = np.stack([c.A for c in cases]), np.stack([c.B for c in cases])
    o = _device(lib, itype, A, B, 1)
    o0 = _device(lib, itype, A, B, 0)
    assert o.rc == 0 and o0.rc == 0
    fails, worst, foreign, foreign_hi = [], np.zeros(3), 0.0, 0.0
    for b, c in enumerate(cases):
        what = "n=%d itype=%d %s" % (n, itype, c.name)
        if c.name == "hilbert_b":
            t1 = _device(lib, 1, A[b:b + 1], B[b:b + 1], 1, entry="ek_hip_eigenpairs_batched_device")
            if not (o.info[b] > 0 and o.info[b] == t1.info[0] == o0.info[b]):
                fails.append("%s: info %d / %d, type 1 says %d" % (what, o.info[b], o0.info[b], t1.info[0]))
            continue
        if o.info[b] != 0 or o0.info[b] != 0:
            fails.append("%s: info = %d / %d where 0 is required" % (what, o.info[b], o0.info[b]))
            continue
        w_ref, Z_ref = _ref(("hard", c.name, n), itype, c.A, c.B)
        tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
        err = np.abs(o.w[b] - w_ref).max()
        L = np.tril(o.B[b])                         # the factor the kernel used, held to its own backward error
        back = np.abs(L @ L.T - c.B).max()
        if not back <= 16 * n * EPS * np.abs(c.B).max():
            fails.append("%s: |L L^T - B| = %.3e > %.3e" % (what, back, 16 * n * EPS * np.abs(c.B).max()))
        res, orth = _quantities(itype, c.A, c.B, o.w[b], o.Z[b], L)
        res_l, orth_l = _quantities(itype, c.A, c.B, w_ref, Z_ref)
        lim_r, lim_o = 4 * max(res_l, 16 * n * EPS), 4 * max(orth_l, 16 * n * EPS)
        # the same Z measured with LAPACK's factor, as the random pairs are: the figure of the issue's rule
        orth_f = _quantities(itype, c.A, c.B, o.w[b], o.Z[b])[1]
        cond = np.linalg.cond(c.B)
        lim_f = 4 * max(orth_l, 16 * n * EPS, n * EPS * cond)     # cond(B) <= 16: the rule as it stands
        if cond <= 16:
            foreign = max(foreign, orth_f / lim_o)
        else:
            foreign_hi = max(foreign_hi, orth_f / lim_o)
        print("  %s: cond(B) = %.2e; orthogonality with the library's factor %.2e, with LAPACK's %.2e; the rule "
              "%.2e, with n eps cond(B) in it %.2e" % (what, cond, orth, orth_f, lim_o, lim_f))
        if c.name in ("a_equals_b", "band5_band5") and not cond <= 16:
            fails.append("%s: cond(B) = %.3e: the case is no longer a well-conditioned one" % (what, cond))
        if not orth_f <= lim_f:
            fails.append("%s: orthogonality with LAPACK's factor %.3e > %.3e (LAPACK's own %.3e, cond(B) %.2e)"
                         % (what, orth_f, lim_f, orth_l, cond))
        worst = np.maximum(worst, (err / tol, res / lim_r, orth / lim_o))
        if not np.all(np.isfinite(o.w[b])) or not np.all(np.isfinite(o.Z[b])):
            fails.append("%s: info = 0 with a non-finite result" % what)
        if not np.all(np.diff(o.w[b]) >= 0):
            fails.append("%s: w not ascending" % what)
        if not err <= tol:
            fails.append("%s: eigenvalues, error %.3e > %.3e" % (what, err, tol))
        if not res <= lim_r:
            fails.append("%s: residual %.3e > %.3e (LAPACK's own %.3e)" % (what, res, lim_r, res_l))
        if not orth <= lim_o:
            fails.append("%s: orthogonality %.3e > %.3e (LAPACK's own %.3e)" % (what, orth, lim_o, orth_l))
        if not np.array_equal(_bits(o0.w[b]), _bits(o.w[b])):
            fails.append("%s: values only gives another w" % what)
    print("n=%d itype=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f "
          "(orthogonality with LAPACK's factor: %.3f of the rule where cond(B) <= 16, %.3g times the rule on cond_b:*)"
          % ((n, itype) + tuple(worst) + (foreign, foreign_hi)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", HARD_ORDERS)
def test_sygv_batched_scale_covariance_and_overflow(hip, n, itype):
    """band5_band5 times 2^+-531 and 2^+-664 returns 2^k w, the same Z and the same reflector tails in dA, to the bit;
    with A 2^600 and B 2^600 the eigenvalues are 2^1200 times the unscaled ones: info = 100000 + n + 1 and nothing is
    written, never a silent info = 0."""
    lib = hip.load_library()
    base = bc.make("band5_band5", n)
    cases = [base] + [bc.scaled(base, k) for k in bc.COVARIANT_SCALES] + [bc.scaled(base, 600, 600)]
    A, B = np.stack([c.A for c in cases]), np.stack([c.B for c in cases])
    o, o0 = _device(lib, itype, A, B, 1), _device(lib, itype, A, B, 0)
    last = len(cases) - 1
    assert o.rc == 0 and o0.rc == 0
    assert not o.info[:last].any() and not o0.info[:last].any(), (o.info, o0.info)
    band = np.tri(n, n, 0, dtype=bool) & ~np.tri(n, n, -2, dtype=bool)      # diagonal and subdiagonal: d and e
    tails = np.tri(n, n, -2, dtype=bool)
    fails = []
    for j, k in enumerate(bc.COVARIANT_SCALES):
        b = 1 + j
        what = "n=%d itype=%d 2^%d" % (n, itype, k)
        if not np.array_equal(_bits(o.w[b]), _bits(np.ldexp(o.w[0], k))):
            fails.append("%s: w is not 2^k times w of the unscaled case" % what)
        if not np.array_equal(_bits(o0.w[b]), _bits(o.w[b])):
            fails.append("%s: values only gives another w" % what)
        if not np.array_equal(_bits(o.Z[b]), _bits(o.Z[0])):
            fails.append("%s: Z differs" % what)
        if not np.array_equal(_bits(o.A[b][tails]), _bits(o.A[0][tails])):
            fails.append("%s: reflector tails in dA differ" % what)
        if not np.array_equal(_bits(o.A[b][band]), _bits(np.ldexp(o.A[0][band], k))):
            fails.append("%s: d, e in dA are not 2^k times the unscaled case's" % what)
        if not np.array_equal(_bits(np.tril(o.B[b])), _bits(np.tril(o.B[0]))):
            fails.append("%s: L in dB differs" % what)
    for x in (o, o0):
        if x.info[last] != 100000 + n + 1:
            fails.append("n=%d itype=%d A 2^600, B 2^600: info = %d" % (n, itype, x.info[last]))
        if not (np.all(x.w[last] == SENTINEL) and np.all(x.Z[last] == SENTINEL)):
            fails.append("n=%d itype=%d A 2^600, B 2^600: w or Z was written" % (n, itype))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------- 7: cost
@pytest.mark.parametrize("n,batch", [(64, 1024), (128, 512)])
def test_sygv_batched_costs_what_type_1_costs(hip, n, batch):
    """Device seconds with vectors, best of 3, the three types alternated in one process: types 2 and 3 take at most
    1.25 x type 1's time.  Cholesky plus reduction is 11 % and 10 % of a workgroup's time at these orders (DESIGN.md
    12), so a reduction twice as expensive as type 1's stays below 1.13 and two launches of one batch lie within 0.5 %:
    1.25 is passed only by a mistake such as a one-lane loop or conflicting banks.  Measured on one MI355X: 0.957 and
    0.970 at order 64, 0.965 and 0.974 at order 128."""
    lib = hip.load_library()
    A, B = _pairs(4000 + n, batch, n)
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    info = np.zeros(batch, dtype=np.int32)
    best = {1: np.inf, 2: np.inf, 3: np.inf}
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))

        def run(itype):
            dev.put(dA, hA); dev.put(dB, hB)               # the call works in place: fresh inputs, outside the clock
            sec = ctypes.c_double(-1.0)
            rc = lib.ek_hip_sygv_batched_device(itype, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                info.ctypes.data_as(_ip), ctypes.byref(sec))
            assert rc == 0 and not info.any() and sec.value > 0.0
            return sec.value

        for itype in (1, 2, 3):                            # warm-up
            run(itype)
        for _ in range(3):
            for itype in (1, 2, 3):
                best[itype] = min(best[itype], run(itype))
    print("n=%d batch=%d: type 1 %.3f ms, type 2 %.3f ms (%.3f x), type 3 %.3f ms (%.3f x)"
          % (n, batch, best[1] * 1e3, best[2] * 1e3, best[2] / best[1], best[3] * 1e3, best[3] / best[1]))
    assert best[2] <= 1.25 * best[1], (best[2], best[1])
    assert best[3] <= 1.25 * best[1], (best[3], best[1])
