"""GPU suite of ek_hip_eigenpairs_ybatched*: the batched solver for orders 257 .. 512, the class of 512 rows and 1024
threads of ek_batched_x.hip's kernel.  Helpers, references and bounds are those of
tests/test_gpu_batched.py, tests/test_gpu_batched_hard.py and tests/test_gpu_xbatched.py, unchanged: SciPy on the CPU on
seeded inputs, 4 max(n, 8) eps max|lambda| on eigenvalues, 64 / 256 n eps on residual and orthogonality, the hard-input
table of tests/batched_cases.py under _judge.  tests/test_ybatched_host.py holds LAPACK alone to half of these bounds at the
new orders.

ORDERS_Y: 257 is the class's first order (a wave of one row), 263 is no multiple of 16 (the remainder loops of the
eight-deep batches at two threads per row), 320 a multiple of 64, 384 and 385 the two sides of a wave boundary, 511 and 512
fill the class.  A launch at order 512 lasts a few tenths of a second whatever the batch up to 256 (the one-lane QL chain
sets the pace), so every case of an order shares a launch."""
import ctypes
import time

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import test_gpu_batched_hard as hard
from test_gpu_batched import EPS, SENTINEL, _Dev, _check_problem, _pack, _pairs, _ref, _solve_device, _unpack, _view
from test_gpu_xbatched import _bits, _device, _same

pytestmark = pytest.mark.gpu
ORDERS_Y = (257, 263, 320, 384, 385, 511, 512)
NEW = "ek_hip_eigenpairs_ybatched_device"
OLD = "ek_hip_eigenpairs_xbatched_device"
_ip = ctypes.POINTER(ctypes.c_int)


def _run(lib, A, B, jobz, **kw):
    return _device(lib, A, B, jobz, entry=NEW, **kw)


# ------------------------------------------------------------------------------------------------- accuracy
_lapack = {}


def _w_ref(n, problem, b, A, B):
    """scipy.linalg.eigh's eigenvalues, computed once per (order, kind, problem of the batch) and shared by jobz 0 / 1"""
    key = (n, problem, b)
    if key not in _lapack:
        _lapack[key] = _ref(A, B)[0]
        _lapack[key].setflags(write=False)
    return _lapack[key]


@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", ORDERS_Y)
def test_ybatched_accuracy_against_scipy(hip, n, problem, jobz):
    """4 seeded problems of one order in one batch against scipy.linalg.eigh; with vectors also each problem's
    eigenvalues against ek_hip_solve_device on the same pair (other algorithms: to the bound, not to the bit)."""
    lib = hip.load_library()
    batch = 4
    A, B = _pairs(1000 + n, batch, n)
    if not problem:
        B = None
    o = _run(lib, A, B, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    worst = np.zeros(4)
    for b in range(batch):
        Bb = B[b] if problem else None
        w_ref = _w_ref(n, problem, b, A[b], Bb)
        used = _check_problem(A[b], Bb, o.w[b], o.Z[b] if jobz else None, w_ref, (n, problem, jobz, b))
        worst[:3] = np.maximum(worst[:3], used)
        if jobz:
            info, w_lib = _solve_device(lib, A[b], Bb)
            assert info == 0
            tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
            worst[3] = max(worst[3], np.abs(o.w[b] - w_lib).max() / tol)
            assert np.abs(o.w[b] - w_lib).max() <= tol, (n, problem, b, np.abs(o.w[b] - w_lib).max(), tol)
    if not jobz:
        assert np.all(o.Zflat == SENTINEL)
    print("n=%d problem=%d jobz=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f "
          "against ek_hip_solve_device %.3f" % ((n, problem, jobz) + tuple(worst)))


# ------------------------------------------------------------------------------------------------- contract
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [1, 128, 129, 256])
def test_ybatched_is_the_xbatched_entry_up_to_256(hip, n, problem, jobz):
    """The seam at 256: up to it the new entry runs the code behind the xbatched one -- equal bits in info, w, Z, dA, dB."""
    lib = hip.load_library()
    A, B = _pairs(50 + n, 4, n)
    if not problem:
        B = None
    new = _run(lib, A, B, jobz)
    old = _device(lib, A, B, jobz, entry=OLD)
    assert new.rc == 0 and old.rc == 0 and not old.info.any()
    assert np.array_equal(new.info, old.info)
    assert np.array_equal(_bits(new.wflat), _bits(old.wflat))
    assert np.array_equal(_bits(new.Zflat), _bits(old.Zflat))
    assert np.array_equal(_bits(new.Aflat), _bits(old.Aflat))
    if problem:
        assert np.array_equal(_bits(new.Bflat), _bits(old.Bflat))


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [257, 512])
def test_ybatched_bit_identity_wherever_a_problem_sits(hip, n, problem):
    """The same pair alone, at positions 0, 2 and last of a batch of 5, with and without vectors, and through the host
    form."""
    lib = hip.load_library()
    A1, B1 = _pairs(7 * n + problem, 1, n)
    alone = _run(lib, A1, B1 if problem else None, 1)
    alone0 = _run(lib, A1, B1 if problem else None, 0)
    assert alone.rc == 0 and alone.info[0] == 0 and alone0.rc == 0 and alone0.info[0] == 0
    assert np.array_equal(_bits(alone0.w), _bits(alone.w))
    assert np.array_equal(_bits(np.tril(alone0.A[0])), _bits(np.tril(alone.A[0])))
    places = (0, 2, 4)
    A, B = _pairs(99 + n, 5, n)
    for pos in places:
        A[pos], B[pos] = A1[0], B1[0]
    o = _run(lib, A, B if problem else None, 1)
    assert o.rc == 0 and not o.info.any()
    o0 = _run(lib, A, B if problem else None, 0)
    for pos in places:
        _same(o, pos, alone, 0, 1, (n, problem, pos))
        _same(o0, pos, alone0, 0, 0, (n, problem, pos, "values only"))
    A_in, B_in = A.copy(), B.copy()
    w, Z, info = hip.eigenpairs_ybatched(A, B if problem else None)
    assert not info.any()
    assert np.array_equal(_bits(w[2]), _bits(alone.w[0])) and np.array_equal(_bits(Z[2]), _bits(alone.Z[0]))
    assert np.array_equal(_bits(w), _bits(o.w)) and np.array_equal(_bits(Z), _bits(o.Z))
    assert np.array_equal(A, A_in) and np.array_equal(B, B_in)      # the host form leaves its inputs alone


def test_ybatched_chunk_seam(hip):
    """A batch of 5 distinct pairs of order 257 in chunks of 2 (three launches, the slots reused) and of 1: the default
    chunk's bits.  The hook returns the previous setting and 0 restores the default."""
    lib = hip.load_library()
    n = 257
    A, B = _pairs(4242, 5, n)
    whole = _run(lib, A, B, 1)
    assert whole.rc == 0 and not whole.info.any()
    before = lib.ek_hip_debug_ybatched_chunk(2)
    try:
        assert before == 256
        parts = _run(lib, A, B, 1)
        parts0 = _run(lib, A, None, 0)
        assert lib.ek_hip_debug_ybatched_chunk(1) == 2
        ones = _run(lib, A, B, 1)
    finally:
        assert lib.ek_hip_debug_ybatched_chunk(0) == 1
    assert lib.ek_hip_debug_ybatched_chunk(0) == 256
    whole0 = _run(lib, A, None, 0)
    assert parts.rc == 0 and ones.rc == 0 and parts0.rc == 0
    for b in range(5):
        _same(parts, b, whole, b, 1, ("chunk 2", b))
        _same(ones, b, whole, b, 1, ("chunk 1", b))
        _same(parts0, b, whole0, b, 0, ("chunk 2, standard, values only", b))


def test_ybatched_layout_contract(hip):
    """n = 263, every leading dimension 270, strides 270 * 263 + 11, sentinels everywhere and NaN in the strict upper
    triangles of A and B.  Everything outside the lower triangles of A and B and the n x n blocks of Z keeps its bits;
    the compact layout gives the same bits; values only writes nothing to Z; dB holds L (max|L L^T - B| <= 16 n eps
    max|B|); dA holds DSYTD2's lower layout of C = L^-1 A L^-T with tau_k = 2 / (1 + |tail_k|^2): LAPACK's eigenvalues of
    its (d, e) are w to 4 n eps max|lambda|, and Q T Q^T rebuilt from it is C to 256 n eps ||C||_2.  Two tridiagonal
    inputs (Toeplitz, Wilkinson; H = I throughout) keep d and e to the bit."""
    lib = hip.load_library()
    n, ld, batch = 263, 270, 3
    stride = ld * n + 11
    A, B = _pairs(263263, batch, n)
    compact = _run(lib, A, B, 1)
    An, Bn = A.copy(), B.copy()
    iu = np.triu_indices(n, 1)
    An[:, iu[0], iu[1]] = np.nan
    Bn[:, iu[0], iu[1]] = np.nan
    o = _run(lib, An, Bn, 1, ld=ld, stride=stride)
    o0 = _run(lib, An, Bn, 0, ld=ld, stride=stride)
    assert o.rc == 0 and not o.info.any() and not compact.info.any() and o0.rc == 0 and not o0.info.any()
    assert np.all(o0.Zflat == SENTINEL)                          # values only writes no Z at all
    for b in range(batch):
        _same(o, b, compact, b, 1, ("padded against compact", b))
        _same(o0, b, compact, b, 0, ("padded, values only, against compact", b))
    low = np.tri(n, n, 0, dtype=bool)
    for after, before in ((o.Aflat, o.hA), (o.Bflat, o.hB)):
        keep = np.ones(after.size, dtype=bool)
        _view(keep, batch, n, ld, stride)[...] = ~low.T          # [b, j, i] view: the lower triangle is i >= j
        assert keep.sum() > batch * n * (n - 1) // 2
        assert np.array_equal(_bits(after[keep]), _bits(before[keep]))
        assert np.isnan(_unpack(after, batch, n, ld, stride)[:, iu[0], iu[1]]).all()
    pad = np.ones(o.Zflat.size, dtype=bool)
    _view(pad, batch, n, ld, stride)[...] = False
    assert pad.sum() > 0 and np.all(o.Zflat[pad] == SENTINEL)
    assert np.all(o.wflat[batch * n:] == SENTINEL)
    for b in range(batch):
        L = np.tril(o.B[b])
        assert np.abs(L @ L.T - B[b]).max() <= 16 * n * EPS * np.abs(B[b]).max(), b
        C = sl.solve_triangular(L, sl.solve_triangular(L, A[b], lower=True).T, lower=True).T
        d, e = np.diag(o.A[b]).copy(), np.diag(o.A[b], -1).copy()
        w_t = sl.eigvalsh_tridiagonal(d, e)
        tol = 4 * n * EPS * np.abs(o.w[b]).max()
        assert np.abs(w_t - o.w[b]).max() <= tol, (b, np.abs(w_t - o.w[b]).max(), tol)
        Q = np.eye(n)
        for k in range(n - 2):
            v = np.zeros(n)
            v[k + 1] = 1.0
            v[k + 2:] = o.A[b][k + 2:, k]
            tau = 2.0 / (1.0 + v[k + 2:] @ v[k + 2:])
            Q = Q - tau * np.outer(Q @ v, v)                     # Q <- Q H_k
        Tm = np.diag(d) + np.diag(e, -1) + np.diag(e, 1)
        err, lim = np.abs(Q @ Tm @ Q.T - C).max(), 256 * n * EPS * np.linalg.norm(C, 2)
        print("problem %d: |Q T Q^T - C| = %.3e, %.4f of the bound" % (b, err, err / lim))
        assert err <= lim, (b, err, lim)
    # the standard problem in the same layout on tridiagonal inputs, against bc.dsytd2_unscaled
    S2 = np.stack([bc.make("toeplitz121", n).A, bc.make("wilkinson", n).A])
    s = _run(lib, S2, None, 0, ld=ld, stride=stride)
    assert s.rc == 0 and not s.info.any()
    for b in range(2):
        d_ref, e_ref = bc.dsytd2_unscaled(S2[b])
        d, e = np.diag(s.A[b]).copy(), np.diag(s.A[b], -1).copy()
        assert np.array_equal(_bits(d), _bits(d_ref)) and np.array_equal(_bits(e), _bits(e_ref)), b
        assert np.array_equal(_bits(d), _bits(np.diag(S2[b]).copy())), b
        assert np.array_equal(_bits(e), _bits(np.diag(S2[b], -1).copy())), b


def test_ybatched_failures_stay_in_their_own_slots(hip):
    """One batch of 5 at order 257: a NaN in A's lower triangle (-5), an Inf in A (-5), a B with a negative entry at
    diagonal index 128 (its 1-based pivot, the code ek_hip_solve_device returns), two good problems whose bits are those
    they have alone."""
    lib = hip.load_library()
    n = 257
    A, B = _pairs(257257, 5, n)
    Ab, Bb = A.copy(), B.copy()
    Ab[1, n - 1, 2] = np.nan
    Ab[2, 100, 100] = np.inf
    Bb[3, 128, 128] = -3.0
    o = _run(lib, Ab, Bb, 1)
    assert o.rc == 0
    assert o.info[1] == -5 and o.info[2] == -5, o.info
    info_lib, _ = _solve_device(lib, Ab[3], Bb[3])
    assert o.info[3] == info_lib == 129, (o.info[3], info_lib)
    for b in (0, 4):
        solo = _run(lib, A[b:b + 1], B[b:b + 1], 1)
        assert solo.rc == 0 and solo.info[0] == 0
        _same(o, b, solo, 0, 1, ("good problem against its solo run", b))
    iu = np.triu_indices(n, 1)
    for b in (1, 2, 3):                            # a failed problem leaves the strictly upper triangles alone too
        assert np.array_equal(_bits(o.A[b][iu]), _bits(Ab[b][iu])) and np.array_equal(_bits(o.B[b][iu]), _bits(Bb[b][iu]))
    assert o.wflat.size == 5 * n and o.Zflat.size == 5 * n * n       # compact: the slots are all there is
    o0 = _run(lib, Ab, Bb, 0)
    assert o0.rc == 0 and list(o0.info) == list(o.info)
    for b in (0, 4):
        assert np.array_equal(_bits(o0.w[b]), _bits(o.w[b]))
    assert np.all(o0.Zflat == SENTINEL)                          # values only writes no Z at all
    w, Z, info = hip.eigenpairs_ybatched(Ab, Bb)
    assert list(info) == list(o.info) and np.array_equal(_bits(w[[0, 4]]), _bits(o.w[[0, 4]]))


# ------------------------------------------------------------------------------------------------- hard inputs
def _hard_batch(lib, cases, n, problem, jobz):
    A = np.stack([c.A for c, _ in cases])
    B = np.stack([c.B for c, _ in cases]) if problem else None
    o = _run(lib, A, B, jobz)
    assert o.rc == 0, o.rc
    shares, fails = hard._Shares(), []
    for b, (c, base) in enumerate(cases):
        what = "n=%d problem=%d jobz=%d %s" % (n, problem, jobz, c.name)
        s, f = hard._judge(lib, c, base, int(o.info[b]), o.w[b], o.Z[b] if jobz else None, what)
        shares.add(c.family, s)
        fails += f
        if not c.spd and o.info[b] <= 0:
            fails.append("%s: info = %d where a pivot of B's Cholesky factorisation should fail" % (what, o.info[b]))
        if c.tridiagonal and o.info[b] == 0:
            fails += hard._tridiagonal_kept(c, o.A[b], what)
    shares.show("n=%d problem=%d jobz=%d (%d cases)" % (n, problem, jobz, len(cases)))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails)


@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
def test_ybatched_hard_cases_in_one_batch_at_257(hip, problem, jobz):
    """Every case of batched_cases at order 257 and one kind in one launch, judged by test_gpu_batched_hard._judge and
    _tridiagonal_kept as they stand."""
    lib = hip.load_library()
    n = 257
    _hard_batch(lib, bc.pencil_batch(n) if problem else bc.standard_batch(n), n, problem, jobz)


@pytest.mark.parametrize("problem", [0, 1])
def test_ybatched_hard_cases_one_per_family_at_512(hip, problem):
    """Order 512 with vectors: the first case of every family of the table (SciPy's reference on the whole table at this
    order costs more host time than the suite can spend), one launch."""
    lib = hip.load_library()
    n = 512
    first = {}
    for c, base in (bc.pencil_batch(n) if problem else bc.standard_batch(n)):
        first.setdefault(c.family, (c, base))
    assert len(first) >= 2
    _hard_batch(lib, list(first.values()), n, problem, 1)


@pytest.mark.parametrize("problem", [0, 1])
def test_ybatched_scale_covariance_to_the_bit(hip, problem):
    """test_scale_covariance_to_the_bit at order 320: w of A 2^k is 2^k times w of A bit for bit, Z and the reflector
    tails are the same bits, d and e in dA are 2^k times the unscaled case's, L is the same; values only gives that w."""
    lib = hip.load_library()
    n = 320
    names = bc.COVARIANT_PENCILS if problem else bc.COVARIANT_STANDARD
    group = 1 + len(bc.COVARIANT_SCALES)
    cases = []
    for name in names:
        base = bc.make(name, n)
        cases += [base] + [bc.scaled(base, k) for k in bc.COVARIANT_SCALES]
    A = np.stack([c.A for c in cases])
    B = np.stack([c.B for c in cases]) if problem else None
    o = _run(lib, A, B, 1)
    o0 = _run(lib, A, B, 0)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o0.rc == 0 and not o0.info.any(), (o0.rc, o0.info)
    band = np.tri(n, n, 0, dtype=bool) & ~np.tri(n, n, -2, dtype=bool)
    tails = np.tri(n, n, -2, dtype=bool)
    fails = []
    for g in range(len(names)):
        b0 = g * group
        for j, k in enumerate(bc.COVARIANT_SCALES):
            b = b0 + 1 + j
            what = "n=%d problem=%d %s" % (n, problem, cases[b].name)
            if not np.array_equal(_bits(o.w[b]), _bits(np.ldexp(o.w[b0], k))):
                fails.append("%s: w is not 2^k times w of the unscaled case" % what)
            if not np.array_equal(_bits(o0.w[b]), _bits(o.w[b])):
                fails.append("%s: values only gives another w" % what)
            if not np.array_equal(_bits(o.Z[b]), _bits(o.Z[b0])):
                fails.append("%s: Z differs" % what)
            if not np.array_equal(_bits(o.A[b][tails]), _bits(o.A[b0][tails])):
                fails.append("%s: reflector tails in dA differ" % what)
            if not np.array_equal(_bits(o.A[b][band]), _bits(np.ldexp(o.A[b0][band], k))):
                fails.append("%s: d, e in dA are not 2^k times the unscaled case's" % what)
            if problem and not np.array_equal(_bits(np.tril(o.B[b])), _bits(np.tril(o.B[b0]))):
                fails.append("%s: L in dB differs" % what)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------- speed
# t_loop / t_batched must reach this on top of t_batched < t_loop: half the ratio measured for 256 pairs on one MI355X (28.6
# at n = 257, 3.6 at n = 512: DESIGN.md 40, profiles/r23_ybatched_timing_v1.txt), the factor two being for a shared machine
GATE = {257: 14.3, 512: 1.8}


def _speed(lib, n, batch, nloop):
    """(t_batched, t_loop): best of 3 after a warm-up, the kinds alternated, device-resident arrays both ways.
    t_batched is the device time the call reports; t_loop is batch / nloop times a host loop of ek_hip_solve_device over
    the first nloop pairs."""
    A, B = _pairs(4000 + n, nloop, n)
    reps = -(-batch // nloop)
    A, B = np.tile(A, (reps, 1, 1))[:batch], np.tile(B, (reps, 1, 1))[:batch]
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    info = np.zeros(batch, dtype=np.int32)
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))

        def at(p, b, per):
            return ctypes.c_void_p(p.value + b * per * 8)

        def batched():
            dev.put(dA, hA); dev.put(dB, hB)           # both calls work in place: fresh inputs, outside the clock
            sec = ctypes.c_double(0.0)
            rc = lib.ek_hip_eigenpairs_ybatched_device(1, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                       info.ctypes.data_as(_ip), ctypes.byref(sec))
            assert rc == 0 and not info.any()
            return sec.value

        def loop():
            dev.put(dA, hA); dev.put(dB, hB)
            t0 = time.perf_counter()
            for b in range(nloop):
                rc = lib.ek_hip_solve_device(1, n, n, at(dA, b, n * n), n, at(dB, b, n * n), n, at(dw, b, n),
                                             at(dZ, b, n * n), n, None, 0)
                assert rc == 0
            return (time.perf_counter() - t0) * (batch / nloop)

        tb, tl = [], []
        batched(); loop()
        for _ in range(3):
            tb.append(batched()); tl.append(loop())
    return min(tb), min(tl)


@pytest.mark.parametrize("n", [257, 512])
def test_xbatched_beats_the_host_loop(hip, n):
    """256 generalized pairs with vectors (8 seeded pairs, repeated: a problem's time depends on (n, A, B) alone) through
    ek_hip_eigenpairs_ybatched_device: the batched call must be faster than the only other way to do the job, a host loop
    over ek_hip_solve_device (measured on 8 pairs and scaled to the batch); otherwise the entry has no use.  GATE holds
    the ratio to reach on top of that."""
    lib = hip.load_library()
    t_batched, t_loop = _speed(lib, n, 256, 8)
    print("n=%d batch=256: batched %.3f ms (%.1f us per problem), loop %.1f ms (%.1f us per problem), ratio %.1f"
          % (n, t_batched * 1e3, t_batched / 256 * 1e6, t_loop * 1e3, t_loop / 256 * 1e6, t_loop / t_batched))
    assert t_batched < t_loop, (t_batched, t_loop)
    assert t_loop / t_batched >= GATE[n], (t_loop / t_batched, GATE[n])
