"""GPU suite of the variable-order batched entries for orders up to 256 (ek_hip_eigenpairs_xvbatched*,
ek_hip_sygv_xvbatched*): problems of different orders in one call, a problem above 128 in the kernel of
ek_hip_*_xbatched* (image in device memory), every other one in the class ek_hip_*_vbatched* give it.

The oracle of the contract needs no tolerance: a problem's w, Z, info and in-place images are the bits
ek_hip_eigenpairs_xbatched_device / ek_hip_sygv_xbatched_device return for that pair alone.  Helpers and bounds are those of
tests/test_gpu_xbatched.py, tests/test_gpu_vbatched.py, tests/test_gpu_sygv_batched.py and tests/test_gpu_batched_hard.py,
imported as they stand.

ORDERS_XV: both sides of every class limit (32 | 33, 64 | 65, 128 | 129), the first order of the new class, 130 for the
even / odd split of a pair of threads, both sides of the wave boundary at 192, and the full class; two seeded problems
each.  Every call sees all problems of the new class at once, so it costs about one workgroup's latency."""
import ctypes
import time

import numpy as np
import pytest

import batched_cases as bc
import test_gpu_batched_hard as hard
import test_gpu_sygv_batched as sg
import test_gpu_vbatched as vb
import test_gpu_xbatched as xb
from test_gpu_vbatched import EPS, _Dev, _Out, _Place, _check_problem, _mixed, _ref, _solve_device

pytestmark = pytest.mark.gpu
ORDERS_XV = (0, 1, 32, 33, 64, 65, 128, 129, 130, 192, 193, 255, 256)
NANS = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload: the sentinel
_ip = ctypes.POINTER(ctypes.c_int)
# (entry family, first argument, jobz): problems 0 and 1 with and without vectors, types 2 and 3 with vectors
CASES = [("eig", 0, 0), ("eig", 0, 1), ("eig", 1, 0), ("eig", 1, 1), ("sygv", 2, 1), ("sygv", 3, 1)]
case_ids = ["%s-%d-jobz%d" % c for c in CASES]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _eq(x, y):
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _names(kind, device):
    stem = "ek_hip_eigenpairs_" if kind == "eig" else "ek_hip_sygv_"
    return stem + "xvbatched" + ("_device" if device else ""), stem + "xbatched_device"


def _fill(pl, mats, upper_nan):
    flat = np.full(max(int(pl.off[-1]), 1), NANS)
    for b, M in enumerate(mats):
        n = M.shape[0]
        if n:
            M = M.copy()
            if upper_nan:
                M[np.triu_indices(n, 1)] = NANS
            pl.block(flat, b)[...] = M.T
    return flat


def _xv(lib, pairs, kind, first, jobz, pad=0, host=False):
    """The variable entry of `kind` ("eig": first = problem; "sygv": first = itype) on the pairs, every problem in its
    own region of one buffer per array kind (test_gpu_vbatched._Place).  Everything that is not a problem's own is the
    NaN sentinel; with pad > 0 so are the strictly upper triangles of A and B.  Returns rc, info, per problem w, Z and the
    images of A and B after the call, and the flat buffers before and after."""
    withB = kind == "sygv" or first == 1
    pl = _Place([A.shape[0] for A, _ in pairs], pad)
    hA = _fill(pl, [A for A, _ in pairs], pad > 0)
    hB = _fill(pl, [B for _, B in pairs], pad > 0) if withB else None
    hZ = np.full(max(int(pl.off[-1]), 1), NANS)
    hw = np.full(max(int(pl.woff[-1]), 1), NANS)
    info = np.full(pl.batch, 777, dtype=np.int32)
    sec = ctypes.c_double(-1.0)
    o = _Out()
    o.place, o.hA, o.hB = pl, hA.copy(), hB.copy() if withB else None
    ld = pl.ld.ctypes.data_as(_ip)
    fn = getattr(lib, _names(kind, not host)[0])

    def run(bA, bB, bw, bZ):
        return fn(first, jobz, pl.batch, pl.n32.ctypes.data_as(_ip), pl.pointers(bA, pl.off), ld,
                  pl.pointers(bB, pl.off) if withB else None, ld, pl.pointers(bw, pl.woff),
                  pl.pointers(bZ, pl.off) if jobz else None, ld, info.ctypes.data_as(_ip), ctypes.byref(sec))

    if host:
        o.rc = run(hA.ctypes.data, hB.ctypes.data if withB else 0, hw.ctypes.data, hZ.ctypes.data)
        o.Aflat, o.Bflat, o.wflat, o.Zflat = hA, hB, hw, hZ
    else:
        with _Dev(lib) as dev:
            dA = dev.up(hA)
            dB = dev.up(hB) if withB else None
            dw, dZ = dev.up(hw), dev.up(hZ)
            o.rc = run(dA.value, dB.value if withB else 0, dw.value, dZ.value)
            o.Aflat = dev.down(dA, hA)
            o.Bflat = dev.down(dB, hB) if withB else None
            o.wflat, o.Zflat = dev.down(dw, hw), dev.down(dZ, hZ)
    o.seconds = sec.value
    o.info = info.copy()
    o.w, o.Z, o.A = pl.wtake(o.wflat), pl.take(o.Zflat), pl.take(o.Aflat)
    o.B = pl.take(o.Bflat) if withB else None
    return o


def _uniform(lib, kind, first, A, B, jobz):
    """The uniform entry for orders up to 256 on a stack of pairs of one order (tests' own helpers, as they stand)."""
    entry = _names(kind, True)[1]
    if kind == "eig":
        return xb._device(lib, A, B if first else None, jobz, entry=entry)
    return sg._device(lib, first, A, B, jobz, entry=entry)


_alone_cache = {}


def _alone(lib, key, A, B, kind, first, jobz):
    """The uniform call on one pair alone: (info, w, Z, lower triangle of dA after, of dB after), computed once."""
    k = (key, kind, first, jobz)
    if k not in _alone_cache:
        withB = kind == "sygv" or first == 1
        o = _uniform(lib, kind, first, A[None], B[None] if withB else None, jobz)
        assert o.rc == 0
        out = (int(o.info[0]), o.w[0], o.Z[0], np.tril(o.A[0]), np.tril(o.B[0]) if withB else None)
        for x in out[1:]:
            if x is not None:
                x.setflags(write=False)
        _alone_cache[k] = out
    return _alone_cache[k]


def _same_as_alone(lib, key, pair, o, b, kind, first, jobz, what):
    A, B = pair
    if A.shape[0] == 0:
        assert o.info[b] == 0, what
        return
    info, w, Z, La, Lb = _alone(lib, key, A, B, kind, first, jobz)
    assert o.info[b] == info, (what, o.info[b], info)
    assert _eq(np.tril(o.A[b]), La), (what, "dA")
    if Lb is not None:
        assert _eq(np.tril(o.B[b]), Lb), (what, "dB")
    if info == 0:
        assert _eq(o.w[b], w), (what, "w")
        if jobz:
            assert _eq(o.Z[b], Z), (what, "Z")


def _untouched(o, jobz):
    """Everything that is not a problem's own keeps its bits: what lies between the columns (rows n .. ld-1) and between
    the problems in A, B, Z and w, and the strictly upper triangles of A and B."""
    pl = o.place
    for after, before in ((o.Aflat, o.hA), (o.Bflat, o.hB)):
        if after is None:
            continue
        assert _eq(pl.padding(after), pl.padding(before))
        for b in range(pl.batch):
            iu = np.triu_indices(int(pl.orders[b]), 1)
            assert _eq(pl.block(after, b).T[iu], pl.block(before, b).T[iu]), b
    zp, wp = pl.padding(o.Zflat), pl.wpadding(o.wflat)
    assert np.all(_bits(zp) == _bits(NANS)) and np.all(_bits(wp) == _bits(NANS))
    if not jobz:
        assert np.all(_bits(o.Zflat) == _bits(NANS))


def _the_batch():
    """Every order of ORDERS_XV twice, and two seeded shuffles of the 26 problems."""
    orders = list(ORDERS_XV) * 2
    pairs = _mixed(21, orders)
    p1 = np.random.default_rng(211).permutation(len(orders))
    p2 = np.random.default_rng(212).permutation(len(orders))
    return pairs, p1, p2


# ------------------------------------------------------------------------------------------------- 1: the same bits
@pytest.mark.parametrize("kind,first,jobz", CASES, ids=case_ids)
def test_xvbatched_bit_identity_with_the_uniform_call(hip, kind, first, jobz):
    """Every problem's w, Z, info and lower triangles of dA and dB are those of the uniform entry on the pair alone; a
    second permutation with padded leading dimensions, gaps and NaN above the diagonals gives the same bits and leaves
    every NaN where it was; the host form is the device form."""
    lib = hip.load_library()
    pairs, p1, p2 = _the_batch()
    o = _xv(lib, [pairs[i] for i in p1], kind, first, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    for b, i in enumerate(p1):
        _same_as_alone(lib, ("batch", int(i)), pairs[i], o, b, kind, first, jobz, (kind, first, jobz, b, int(i)))
    _untouched(o, jobz)
    o2 = _xv(lib, [pairs[i] for i in p2], kind, first, jobz, pad=3)
    assert o2.rc == 0 and not o2.info.any(), (o2.rc, o2.info)
    assert np.all(o2.place.ld == np.maximum(o2.place.orders, 1) + 3)
    where = {int(i): b for b, i in enumerate(p1)}
    for b2, i in enumerate(p2):
        b = where[int(i)]
        assert _eq(o2.w[b2], o.w[b]) and _eq(o2.Z[b2], o.Z[b]), (b2, int(i))
        assert _eq(np.tril(o2.A[b2]), np.tril(o.A[b])), (b2, int(i))
        if o.B is not None:
            assert _eq(np.tril(o2.B[b2]), np.tril(o.B[b])), (b2, int(i))
    _untouched(o2, jobz)
    h = _xv(lib, [pairs[i] for i in p1], kind, first, jobz, host=True)
    assert h.rc == 0 and not h.info.any()
    assert _eq(h.Aflat, h.hA) and (h.hB is None or _eq(h.Bflat, h.hB))      # the inputs as they were
    assert _eq(h.wflat, o.wflat) and _eq(h.Zflat, o.Zflat)
    # the class times of the last timed call: every class had its problems
    sec, cnt = np.zeros(4), np.zeros(4, dtype=np.int32)
    assert lib.ek_hip_debug_xvbatched_last(sec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           cnt.ctypes.data_as(_ip)) == 0
    assert list(cnt) == [12, 4, 4, 4] and np.all(sec > 0.0), (cnt, sec)


def test_xvbatched_type_1_is_the_eigenpairs_form_and_the_python_mirror(hip):
    """ek_hip_sygv_xvbatched_device(itype = 1) returns the bits of ek_hip_eigenpairs_xvbatched_device(problem = 1); the
    Python wrappers return the device form's bits and leave their inputs alone."""
    lib = hip.load_library()
    pairs, p1, _ = _the_batch()
    batch = [pairs[i] for i in p1]
    e = _xv(lib, batch, "eig", 1, 1)
    s = _xv(lib, batch, "sygv", 1, 1)
    assert e.rc == 0 and s.rc == 0 and not e.info.any() and not s.info.any()
    for name in ("wflat", "Zflat", "Aflat", "Bflat"):
        assert _eq(getattr(e, name), getattr(s, name)), name
    As, Bs = [A for A, _ in batch], [B for _, B in batch]
    As_in, Bs_in = [x.copy() for x in As], [x.copy() for x in Bs]
    w, Z, info = hip.eigenpairs_xvbatched(As, Bs)
    w3, Z3, info3 = hip.sygv_xvbatched(As, Bs, itype=3)
    o3 = _xv(lib, batch, "sygv", 3, 1)
    assert not info.any() and not info3.any() and o3.rc == 0
    for b in range(len(As)):
        assert _eq(w[b], e.w[b]) and _eq(Z[b], e.Z[b]), b
        assert _eq(w3[b], o3.w[b]) and _eq(Z3[b], o3.Z[b]), b
        assert np.array_equal(As[b], As_in[b]) and np.array_equal(Bs[b], Bs_in[b])
    w0, Z0, info0 = hip.eigenpairs_xvbatched(As, vectors=False)
    s0 = _xv(lib, batch, "eig", 0, 0)
    assert Z0 is None and not info0.any() and all(_eq(w0[b], s0.w[b]) for b in range(len(As)))


# ------------------------------------------------------------------------------------------------- 2: the seams of the batch
@pytest.mark.parametrize("problem", [0, 1])
def test_xvbatched_without_a_large_order_is_the_vbatched_entry(hip, problem):
    """No order above 128: the bits of ek_hip_eigenpairs_vbatched_device in every buffer.  Only orders above 128, and one
    problem of order 256 alone, give the uniform call's bits."""
    lib = hip.load_library()
    small = _mixed(31, [128, 0, 1, 33, 64, 17, 128, 65, 32])
    old = vb._vbatched(lib, small, problem, 1)
    new = _xv(lib, small, "eig", problem, 1)
    assert old.rc == 0 and new.rc == 0 and np.array_equal(old.info, new.info) and not new.info.any()
    for b in range(len(small)):
        assert _eq(new.w[b], old.w[b]) and _eq(new.Z[b], old.Z[b]), b
        assert _eq(np.tril(new.A[b]), np.tril(old.A[b])), b
        if problem:
            assert _eq(np.tril(new.B[b]), np.tril(old.B[b])), b
    large = _mixed(32, [129, 256, 200, 130])
    o = _xv(lib, large, "eig", problem, 1)
    assert o.rc == 0 and not o.info.any()
    for b in range(len(large)):
        _same_as_alone(lib, ("large", b), large[b], o, b, "eig", problem, 1, ("only large orders", b))
    one = _xv(lib, large[1:2], "eig", problem, 1)
    assert one.rc == 0 and one.info[0] == 0
    _same_as_alone(lib, ("large", 1), large[1], one, 0, "eig", problem, 1, "one problem of order 256")


# ------------------------------------------------------------------------------------------------- 3: accuracy
@pytest.mark.parametrize("kind,first", [("eig", 0), ("eig", 1), ("sygv", 2), ("sygv", 3)])
def test_xvbatched_accuracy_against_scipy(hip, kind, first):
    """Every problem of the batch against scipy.linalg.eigh within the suite's bounds: 4 max(n, 8) eps max|l| on the
    eigenvalues and test_gpu_vbatched._check_problem's residual and orthogonality bounds; types 2 and 3: the quantities
    and the 256 n eps of tests/test_gpu_sygv_xbatched.py."""
    lib = hip.load_library()
    pairs, p1, _ = _the_batch()
    batch = [pairs[i] for i in p1]
    o = _xv(lib, batch, kind, first, 1)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    worst = np.zeros(3)
    for b, (A, B) in enumerate(batch):
        n = A.shape[0]
        if n == 0:
            assert o.w[b].size == 0
            continue
        if kind == "eig":
            Bb = B if first else None
            used = _check_problem(A, Bb, o.w[b], o.Z[b], _ref(A, Bb)[0], (n, first, b))
        else:
            w_ref = sg._ref(("xv", int(p1[b])), first, A, B)[0]
            tol_w = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
            err = np.abs(o.w[b] - w_ref).max()
            res, orth = sg._quantities(first, A, B, o.w[b], o.Z[b])
            lim = 256 * n * EPS
            assert np.all(np.isfinite(o.w[b])) and np.all(np.diff(o.w[b]) >= 0), (n, first, b)
            assert err <= tol_w, (n, first, b, "eigenvalues", err, tol_w)
            assert res <= lim, (n, first, b, "residual", res, lim)
            assert orth <= lim, (n, first, b, "orthogonality", orth, lim)
            used = (err / tol_w, res / lim, orth / lim)
        worst = np.maximum(worst, used)
    print("%s first=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((kind, first) + tuple(worst)))


# ------------------------------------------------------------------------------------------------- 4: the chunk seam
@pytest.mark.parametrize("kind,first", [("eig", 1), ("sygv", 3)])
def test_xvbatched_chunk_seam(hip, kind, first):
    """Five problems of the new class (256, 255, 200, 130, 129) between small ones in chunks of 2 (three launches of the
    class, the slots reused) and of 1: the default chunking's bits."""
    lib = hip.load_library()
    pairs = _mixed(41, [20, 130, 64, 256, 100, 200, 5, 129, 255, 128, 33])
    whole = _xv(lib, pairs, kind, first, 1)
    assert whole.rc == 0 and not whole.info.any()
    before = lib.ek_hip_debug_xbatched_chunk(2)
    try:
        assert before == 1024
        twos = _xv(lib, pairs, kind, first, 1)
        assert lib.ek_hip_debug_xbatched_chunk(1) == 2
        ones = _xv(lib, pairs, kind, first, 1)
    finally:
        lib.ek_hip_debug_xbatched_chunk(0)
    assert lib.ek_hip_debug_xbatched_chunk(0) == 1024
    for o in (twos, ones):
        assert o.rc == 0 and np.array_equal(o.info, whole.info)
        for name in ("wflat", "Zflat", "Aflat", "Bflat"):
            assert _eq(getattr(o, name), getattr(whole, name)), name
    for b in (3, 7):
        _same_as_alone(lib, ("chunk", b), pairs[b], ones, b, kind, first, 1, ("chunk 1", b))


# ------------------------------------------------------------------------------------------------- 5: failures
def test_xvbatched_failures_stay_in_their_own_slots(hip):
    """A B that is not SPD at order 200 (the pivot ek_hip_solve_device reports), a NaN in A's lower triangle at order 150
    (-5) and a failing pencil of the class of 128 among good problems: the neighbours keep their alone-bits, a failed
    problem's info and images are the uniform call's, and the host form leaves its w and Z slots as they were."""
    lib = hip.load_library()
    orders = [129, 200, 30, 150, 256, 100, 64, 193]
    good = _mixed(51, orders)
    bad = [(A.copy(), B.copy()) for A, B in good]
    bad[1][1][150, 150] = -3.0
    bad[3][0][149, 2] = np.nan
    bad[5][1][50, 50] = -3.0
    failing = (1, 3, 5)
    for kind, first in (("eig", 1), ("sygv", 2)):
        o = _xv(lib, bad, kind, first, 1, pad=2)
        assert o.rc == 0
        assert o.info[1] == _solve_device(lib, *bad[1]) == 151, o.info
        assert o.info[3] == -5, o.info
        assert o.info[5] == _solve_device(lib, *bad[5]) == 51, o.info
        for b in range(len(orders)):
            key = ("bad", b) if b in failing else ("good", b)
            _same_as_alone(lib, key, bad[b], o, b, kind, first, 1, (kind, first, b))
            assert (o.info[b] != 0) == (b in failing)
        _untouched(o, 1)
        h = _xv(lib, bad, kind, first, 1, host=True)
        assert h.rc == 0 and np.array_equal(h.info, o.info)
        for b in range(len(orders)):
            if b in failing:
                assert np.all(_bits(h.w[b]) == _bits(NANS)) and np.all(_bits(h.Z[b]) == _bits(NANS)), b
            else:
                assert _eq(h.w[b], o.w[b]) and _eq(h.Z[b], o.Z[b]), b
        assert _eq(h.Aflat, h.hA) and _eq(h.Bflat, h.hB)
    w, Z, info = hip.sygv_xvbatched([A for A, _ in bad], [B for _, B in bad], itype=2)
    assert np.array_equal(info, o.info)                 # per-problem failures come back in info, not as an exception


# ------------------------------------------------------------------------------------------------- 6: many workgroups
def test_xvbatched_more_workgroups_than_fit_the_device(hip):
    """600 problems of order 129 and 8 of order 256 in a seeded shuffle (more than two workgroups per CU on 256 CUs):
    the bits of one uniform call per order."""
    lib = hip.load_library()
    A1, B1 = xb._pairs(6129, 600, 129)
    A2, B2 = xb._pairs(6256, 8, 256)
    u1, u2 = xb._device(lib, A1, B1, 1), xb._device(lib, A2, B2, 1)
    assert u1.rc == 0 and u2.rc == 0 and not u1.info.any() and not u2.info.any()
    src = [(0, b) for b in range(600)] + [(1, b) for b in range(8)]
    perm = np.random.default_rng(608).permutation(len(src))
    stacks = ((A1, B1), (A2, B2))
    pairs = [(stacks[src[i][0]][0][src[i][1]], stacks[src[i][0]][1][src[i][1]]) for i in perm]
    o = _xv(lib, pairs, "eig", 1, 1)
    assert o.rc == 0 and not o.info.any()
    for b, i in enumerate(perm):
        u, ub = (u1, u2)[src[i][0]], src[i][1]
        assert _eq(o.w[b], u.w[ub]) and _eq(o.Z[b], u.Z[ub]), (b, src[i])
        assert _eq(np.tril(o.A[b]), np.tril(u.A[ub])) and _eq(np.tril(o.B[b]), np.tril(u.B[ub])), (b, src[i])


# ------------------------------------------------------------------------------------------------- 7: hard inputs
@pytest.mark.parametrize("problem", [0, 1])
def test_xvbatched_hard_cases_in_one_call(hip, problem):
    """Every case of batched_cases at orders 129, 193 and 256 in ONE variable call per kind, judged by
    test_gpu_batched_hard._judge and _tridiagonal_kept as they stand."""
    lib = hip.load_library()
    cases = []
    for n in (129, 193, 256):
        cases += bc.pencil_batch(n) if problem else bc.standard_batch(n)
    o = _xv(lib, [(c.A, c.B) for c, _ in cases], "eig", problem, 1)
    assert o.rc == 0, o.rc
    shares, fails = hard._Shares(), []
    for b, (c, base) in enumerate(cases):
        what = "n=%d problem=%d %s" % (c.A.shape[0], problem, c.name)
        s, f = hard._judge(lib, c, base, int(o.info[b]), o.w[b], o.Z[b], what)
        shares.add(c.family, s)
        fails += f
        if not c.spd and o.info[b] <= 0:
            fails.append("%s: info = %d where a pivot of B's Cholesky factorisation should fail" % (what, o.info[b]))
        if c.tridiagonal and o.info[b] == 0:
            fails += hard._tridiagonal_kept(c, o.A[b], what)
    shares.show("variable call, problem=%d (%d cases)" % (problem, len(cases)))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails)


@pytest.mark.parametrize("problem", [0, 1])
def test_xvbatched_scale_covariance_to_the_bit(hip, problem):
    """test_scale_covariance_to_the_bit at order 193 through the variable call, small problems between the cases: w of
    A 2^k is 2^k times w of A bit for bit, Z and the reflector tails are the same bits, d and e in dA are 2^k times the
    unscaled case's, L is the same; values only gives that w."""
    lib = hip.load_library()
    n = 193
    names = bc.COVARIANT_PENCILS if problem else bc.COVARIANT_STANDARD
    group = 1 + len(bc.COVARIANT_SCALES)
    cases = []
    for name in names:
        base = bc.make(name, n)
        cases += [base] + [bc.scaled(base, k) for k in bc.COVARIANT_SCALES]
    filler = _mixed(71, [40, 128, 130])
    pairs = []
    for b, c in enumerate(cases):
        pairs += [(c.A, c.B), filler[b % 3]]
    o, o0 = _xv(lib, pairs, "eig", problem, 1), _xv(lib, pairs, "eig", problem, 0)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o0.rc == 0 and not o0.info.any(), (o0.rc, o0.info)
    band = np.tri(n, n, 0, dtype=bool) & ~np.tri(n, n, -2, dtype=bool)
    tails = np.tri(n, n, -2, dtype=bool)
    fails = []
    for g in range(len(names)):
        b0 = 2 * g * group
        for j, k in enumerate(bc.COVARIANT_SCALES):
            b = b0 + 2 * (1 + j)
            what = "n=%d problem=%d %s" % (n, problem, cases[b // 2].name)
            if not _eq(o.w[b], np.ldexp(o.w[b0], k)):
                fails.append("%s: w is not 2^k times w of the unscaled case" % what)
            if not _eq(o0.w[b], o.w[b]):
                fails.append("%s: values only gives another w" % what)
            if not _eq(o.Z[b], o.Z[b0]):
                fails.append("%s: Z differs" % what)
            if not _eq(o.A[b][tails], o.A[b0][tails]):
                fails.append("%s: reflector tails in dA differ" % what)
            if not _eq(o.A[b][band], np.ldexp(o.A[b0][band], k)):
                fails.append("%s: d, e in dA are not 2^k times the unscaled case's" % what)
            if problem and not _eq(np.tril(o.B[b]), np.tril(o.B[b0])):
                fails.append("%s: L in dB differs" % what)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------- 8: speed
def _speed(lib):
    """(t_var, t_grouped, t_pad, distinct): best of 3 after a warm-up, the kinds alternated in one process, device-resident
    arrays, inputs refreshed outside the clock (all three work in place).  512 generalized problems with vectors, 16 of
    each of 32 orders spread over 129 .. 256; two seeded pairs per order, each standing 8 times in the batch (every copy
    its own memory; a problem's time does not depend on its neighbours' data).  t_grouped: one
    ek_hip_eigenpairs_xbatched_device call per distinct order; t_pad: one such call with every problem padded to order
    256 by a unit block (A: 0.5 I, B: I)."""
    distinct = np.unique(np.round(np.linspace(129, 256, 32)).astype(np.int64))
    assert len(distinct) == 32 and distinct[0] == 129 and distinct[-1] == 256
    seeds = _mixed(81, np.repeat(distinct, 2))
    pick = np.repeat(np.arange(64), 8)                  # grouped order: the problems of one order behind each other
    batch = len(pick)
    gl = _Place([seeds[i][0].shape[0] for i in pick], 0)
    gA, gB = gl.fill([seeds[i][0] for i in pick]), gl.fill([seeds[i][1] for i in pick])
    shuffle = np.random.default_rng(512).permutation(batch)
    pl = _Place(gl.orders[shuffle], 0)
    hA, hB = pl.fill([seeds[pick[i]][0] for i in shuffle]), pl.fill([seeds[pick[i]][1] for i in shuffle])
    N = 256
    PA, PB = np.zeros((batch, N, N)), np.zeros((batch, N, N))
    PA[:, np.arange(N), np.arange(N)] = 0.5
    PB[:, np.arange(N), np.arange(N)] = 1.0
    for b, i in enumerate(pick):
        n = seeds[i][0].shape[0]
        PA[b, :n, :n], PB[b, :n, :n] = seeds[i]
    pA, pB = vb._pack(PA, N, N * N), vb._pack(PB, N, N * N)
    del PA, PB
    first = np.arange(32) * 16                          # where an order's 16 problems begin
    info = np.zeros(batch, dtype=np.int32)
    ip = info.ctypes.data_as(_ip)
    with _Dev(lib) as dev:
        dA, dB, dgA, dgB, dpA, dpB = (dev.up(x) for x in (hA, hB, gA, gB, pA, pB))
        dw, dZ = dev.up(np.zeros(batch * N)), dev.up(np.zeros(batch * N * N))
        n32, ld = pl.n32.ctypes.data_as(_ip), pl.ld.ctypes.data_as(_ip)
        tA, tB = pl.pointers(dA.value, pl.off), pl.pointers(dB.value, pl.off)
        tw, tZ = pl.pointers(dw.value, pl.woff), pl.pointers(dZ.value, pl.off)

        def at(p, off):
            return ctypes.c_void_p(p.value + int(off) * 8)

        def var():
            dev.put(dA, hA); dev.put(dB, hB)
            t0 = time.perf_counter()
            rc = lib.ek_hip_eigenpairs_xvbatched_device(1, 1, batch, n32, tA, ld, tB, ld, tw, tZ, ld, ip, None)
            t = time.perf_counter() - t0
            assert rc == 0 and not info.any()
            return t

        def grouped():
            dev.put(dgA, gA); dev.put(dgB, gB)
            t = 0.0
            for n, f in zip(distinct, first):
                n, c = int(n), 16
                off, woff = gl.off[f], gl.woff[f]
                t0 = time.perf_counter()
                rc = lib.ek_hip_eigenpairs_xbatched_device(1, 1, n, c, at(dgA, off), n, n * n, at(dgB, off), n, n * n,
                                                           at(dw, woff), at(dZ, off), n, n * n, ip, None)
                t += time.perf_counter() - t0
                assert rc == 0 and not info[:c].any()
            return t

        def pad():
            dev.put(dpA, pA); dev.put(dpB, pB)
            t0 = time.perf_counter()
            rc = lib.ek_hip_eigenpairs_xbatched_device(1, 1, N, batch, dpA, N, N * N, dpB, N, N * N, dw, dZ, N, N * N, ip,
                                                       None)
            t = time.perf_counter() - t0
            assert rc == 0 and not info.any()
            return t

        tv, tg, tp = [], [], []
        var(); grouped(); pad()                         # warm-up
        for _ in range(3):                              # kinds alternated
            tv.append(var()); tg.append(grouped()); tp.append(pad())
    return min(tv), min(tg), min(tp), len(distinct)


def test_xvbatched_beats_a_call_per_order_and_padding(hip):
    """Generalized with vectors, 512 problems of 32 distinct orders over 129 .. 256: t_var <= t_grouped / 3 (t_grouped: one
    uniform call per distinct order, the gate of test_gpu_vbatched.py) and t_var <= t_pad (one uniform call with every
    problem padded to order 256: a variable call that loses to padding has no reason to exist).  Measured on one MI355X
    (DESIGN.md 21): t_var = 42.631 ms, t_grouped = 673.507 ms (15.8 x), t_pad = 58.217 ms (1.37 x)."""
    lib = hip.load_library()
    t_var, t_grouped, t_pad, distinct = _speed(lib)
    print("512 problems of order 129..256 (%d distinct): variable %.3f ms, call per order %.3f ms (ratio %.1f), "
          "padded to 256 %.3f ms (ratio %.2f)" % (distinct, t_var * 1e3, t_grouped * 1e3, t_grouped / t_var,
                                                   t_pad * 1e3, t_pad / t_var))
    assert t_var <= t_grouped / 3.0, (t_var, t_grouped)
    assert t_var <= t_pad, (t_var, t_pad)
