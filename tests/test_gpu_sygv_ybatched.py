"""GPU suite of ek_hip_sygv_ybatched*: DSYGV's problem types 2 and 3 (A B x = l x, B A x = l x) at orders 257 .. 512 of
the batched solver, the class of 512 rows of ek_batched_x.hip's kernel in its CONG instantiation.  The
reference is SciPy on the CPU (scipy.linalg.eigh(A, B, type=itype, lower=True)) on the seeded pairs of
tests/test_gpu_ybatched.py; helpers, normalisations and bounds are those of tests/test_gpu_sygv_batched.py (its module
docstring) and the rules for the hard pencils those of tests/test_gpu_sygv_xbatched.py: 4 max(n, 8) eps max|w_ref| on
eigenvalues, 256 n eps on residual and orthogonality, and for the hard pencils of tests/batched_cases.py
4 max(LAPACK's own, 16 n eps) with the factor the library left in dB, that factor held to 16 n eps max|B|.  The contract is
the xbatched suite's: the same bits wherever a problem sits, in every chunk and in both forms, untouched upper triangles
and padding, failures in their own slots; between the types: types 2 and 3 share w and the image left in dA bit for bit,
dB is type 1's L, Z3 = B Z2 to rounding, and itype 1 is ek_hip_eigenpairs_ybatched_device(problem = 1) to the bit.

ORDERS_Y: the class's first order, one that is no multiple of 16, a wave boundary, the full class."""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from test_gpu_batched import _pairs
from test_gpu_sygv_batched import _bits, _device, _quantities, _ref
from test_gpu_vbatched import SENTINEL, _Dev, _pack, _unpack, _view

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS_Y = (257, 263, 384, 512)
HARD_CASES = ("cond_b:1e6", "cond_b:1e10", "a_equals_b", "band5_band5", "hilbert_b")
NEW = "ek_hip_sygv_ybatched_device"
OLD = "ek_hip_sygv_xbatched_device"
TYPE1 = "ek_hip_eigenpairs_ybatched_device"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
types23 = pytest.mark.parametrize("itype", [2, 3])


def _run(lib, itype, A, B, jobz, **kw):
    return _device(lib, itype, A, B, jobz, entry=NEW, **kw)


def _same(o, b, ref, rb, jobz, what):
    """Problem b of o and problem rb of ref: info, w, Z and the lower triangles left in dA and dB, bit for bit."""
    n = o.w.shape[1]
    low = np.tri(n, n, 0, dtype=bool)
    assert o.info[b] == ref.info[rb], (what, "info", o.info[b], ref.info[rb])
    assert np.array_equal(_bits(o.w[b]), _bits(ref.w[rb])), (what, "w")
    if jobz:
        assert np.array_equal(_bits(o.Z[b]), _bits(ref.Z[rb])), (what, "Z")
    assert np.array_equal(_bits(o.A[b][low]), _bits(ref.A[rb][low])), (what, "dA")
    assert np.array_equal(_bits(o.B[b][low]), _bits(ref.B[rb][low])), (what, "dB")


# ------------------------------------------------------------------------------------------------- 1: accuracy
@pytest.mark.parametrize("jobz", [0, 1])
@types23
@pytest.mark.parametrize("n", ORDERS_Y)
def test_sygv_ybatched_accuracy_against_scipy(hip, n, itype, jobz):
    """4 seeded pairs of one order in one launch against scipy.linalg.eigh(A, B, type=itype), with the type's
    normalisations.  An entry that forwards to type 1 fails here: the eigenvalues are those of another problem."""
    lib = hip.load_library()
    batch = 4
    A, B = _pairs(1000 + n, batch, n)
    o = _run(lib, itype, A, B, jobz)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o.seconds > 0.0
    worst = np.zeros(3)
    fails = []
    for b in range(batch):
        w_ref = _ref(("ypairs", n, b), itype, A[b], B[b])[0]
        tol_w = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
        err = np.abs(o.w[b] - w_ref).max()
        worst[0] = max(worst[0], err / tol_w)
        if not np.all(np.isfinite(o.w[b])):
            fails.append((b, "info = 0 with a non-finite w"))
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
@pytest.mark.parametrize("n", ORDERS_Y)
def test_sygv_ybatched_invariants_between_the_types(hip, n):
    """The same batch through types 1, 2 and 3: w and the image left in dA of types 2 and 3 are the same bits, dB is
    type 1's L, values only gives the same w and dA, Z3 = B Z2 to rounding, and itype 1 is
    ek_hip_eigenpairs_ybatched_device(problem = 1) bit for bit, with and without vectors."""
    lib = hip.load_library()
    batch = 3
    A, B = _pairs(1000 + n, batch, n)
    t = {(i, j): _run(lib, i, A, B, j) for i in (1, 2, 3) for j in (0, 1)}
    for o in t.values():
        assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    for j in (0, 1):
        assert np.array_equal(_bits(t[2, j].wflat), _bits(t[3, j].wflat)), ("w of types 2 and 3", j)
        assert np.array_equal(_bits(t[2, j].Aflat), _bits(t[3, j].Aflat)), ("dA of types 2 and 3", j)
        for i in (2, 3):
            assert np.array_equal(_bits(t[i, j].Bflat), _bits(t[1, j].Bflat)), ("dB against type 1's L", i, j)
            assert np.array_equal(_bits(t[i, j].wflat), _bits(t[i, 1].wflat)), ("values only gives another w", i)
            assert np.array_equal(_bits(t[i, j].Aflat), _bits(t[i, 1].Aflat)), ("values only leaves another dA", i)
        p = _device(lib, 1, A, B, j, entry=TYPE1)
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


# ------------------------------------------------------------------------------------------------- 3: up to 256
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("itype", [1, 2, 3])
@pytest.mark.parametrize("n", [128, 129, 256])
def test_sygv_ybatched_is_the_xbatched_entry_up_to_256(hip, n, itype, jobz):
    """The seam at 256: up to it the new entry runs the code behind ek_hip_sygv_xbatched_device: equal bits in info, w,
    Z, dA and dB."""
    lib = hip.load_library()
    A, B = _pairs(50 + n, 4, n)
    new = _run(lib, itype, A, B, jobz)
    old = _device(lib, itype, A, B, jobz, entry=OLD)
    assert new.rc == 0 and old.rc == 0 and not old.info.any()
    assert np.array_equal(new.info, old.info)
    for name in ("wflat", "Zflat", "Aflat", "Bflat"):
        assert np.array_equal(_bits(getattr(new, name)), _bits(getattr(old, name))), name


# ------------------------------------------------------------------------------------------------- 4: the same bits
@types23
def test_sygv_ybatched_bit_identity_wherever_a_problem_sits(hip, itype):
    """Order 257: the same pair alone, at positions 0, 2 and 4 of one batch of 5, through the host form, and in chunks of
    2 and of 1 against the default chunk."""
    lib = hip.load_library()
    n = 257
    A1, B1 = _pairs(7 * n + itype, 1, n)
    alone, alone0 = _run(lib, itype, A1, B1, 1), _run(lib, itype, A1, B1, 0)
    assert alone.rc == 0 and alone.info[0] == 0 and alone0.rc == 0 and alone0.info[0] == 0
    assert np.array_equal(_bits(alone0.w), _bits(alone.w))
    A, B = _pairs(99 + n, 5, n)
    for pos in (0, 2, 4):
        A[pos], B[pos] = A1[0], B1[0]
    o = _run(lib, itype, A, B, 1)
    assert o.rc == 0 and not o.info.any()
    for pos in (0, 2, 4):
        _same(o, pos, alone, 0, 1, (n, itype, pos))
    o0 = _run(lib, itype, A, B, 0)
    _same(o0, 4, alone0, 0, 0, (n, itype, "values only"))
    # host form against device form
    A_in, B_in = A.copy(), B.copy()
    w, Z, info = hip.sygv_ybatched(A, B, itype=itype)
    assert not info.any()
    assert np.array_equal(_bits(w), _bits(o.w)) and np.array_equal(_bits(Z), _bits(o.Z))
    assert np.array_equal(_bits(A), _bits(A_in)) and np.array_equal(_bits(B), _bits(B_in))
    w0, Z0, info0 = hip.sygv_ybatched(A, B, itype=itype, vectors=False)
    assert Z0 is None and not info0.any() and np.array_equal(_bits(w0), _bits(o.w))
    # chunks of 2 (three launches, the slots reused) and of 1 against the default
    before = lib.ek_hip_debug_ybatched_chunk(2)
    try:
        assert before == 256
        parts = _run(lib, itype, A, B, 1)
        assert lib.ek_hip_debug_ybatched_chunk(1) == 2
        ones = _run(lib, itype, A, B, 1)
    finally:
        lib.ek_hip_debug_ybatched_chunk(0)
    assert lib.ek_hip_debug_ybatched_chunk(0) == 256
    assert parts.rc == 0 and ones.rc == 0
    for b in range(5):
        _same(parts, b, o, b, 1, ("chunk 2", b))
        _same(ones, b, o, b, 1, ("chunk 1", b))


# ------------------------------------------------------------------------------------------------- 5: what is not its own
@types23
def test_sygv_ybatched_leaves_alone_what_is_not_its_own(hip, itype):
    """Order 263: NaN in the strictly upper triangles of A and B is never read and survives bit for bit; with lda = ldb
    = ldz = n + 3 and strides with a gap every byte outside the lower triangles of A and B, w and the n x n blocks of Z
    comes back as it was; the host form leaves A and B bit for bit."""
    lib = hip.load_library()
    n, batch = 263, 3
    A, B = _pairs(31 + n + itype, batch, n)
    clean = _run(lib, itype, A, B, 1)
    assert clean.rc == 0 and not clean.info.any()
    An, Bn = A.copy(), B.copy()
    iu = np.triu_indices(n, 1)
    An[:, iu[0], iu[1]] = np.nan
    Bn[:, iu[0], iu[1]] = np.nan
    ld = n + 3
    stride = ld * n + 11
    o = _run(lib, itype, An, Bn, 1, lda=ld, sA=stride, ldb=ld, sB=stride, ldz=ld, sZ=stride)
    assert o.rc == 0 and not o.info.any()
    for b in range(batch):
        _same(o, b, clean, b, 1, ("padded, NaN above the diagonal, against compact", b))
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
    # host form, strided, called directly: inputs untouched, Z's padding untouched
    hA, hB = _pack(An, ld, stride), _pack(Bn, ld, stride)
    hA0, hB0 = hA.copy(), hB.copy()
    hZ, hw = np.full(batch * stride, SENTINEL), np.zeros(batch * n)
    info = np.full(batch, 777, dtype=np.int32)
    rc = lib.ek_hip_sygv_ybatched(itype, 1, n, batch, hA.ctypes.data_as(_dp), ld, stride, hB.ctypes.data_as(_dp), ld,
                                  stride, hw.ctypes.data_as(_dp), hZ.ctypes.data_as(_dp), ld, stride,
                                  info.ctypes.data_as(_ip), None)
    assert rc == 0 and not info.any()
    assert np.array_equal(_bits(hA), _bits(hA0)) and np.array_equal(_bits(hB), _bits(hB0))
    assert np.array_equal(_bits(hw.reshape(batch, n)), _bits(clean.w))
    assert np.array_equal(_bits(_unpack(hZ, batch, n, ld, stride)), _bits(clean.Z))
    assert np.all(hZ[pad] == SENTINEL)


# ------------------------------------------------------------------------------------------------- 6: failures
@types23
def test_sygv_ybatched_failures_stay_in_their_own_slots(hip, itype):
    """Order 257, a batch of 5: problem 1 with a B whose pivot n / 2 + 1 is not positive (info: what type 1 of this class
    reports for it), problem 3 with a NaN in A's lower triangle (-5), three good problems whose w, Z, dA and dB are the
    bits of the clean batch (which test 4 ties to a solo run)."""
    lib = hip.load_library()
    n, batch, keep = 257, 5, (0, 2, 4)
    A, B = _pairs(200 + n + itype, batch, n)
    Ab, Bb = A.copy(), B.copy()
    Bb[1, n // 2, n // 2] = -3.0
    Ab[3, n - 1, 2] = np.nan                   # lower triangle: row n-1, column 2
    type1 = _device(lib, 1, Ab, Bb, 1, entry=TYPE1)
    assert type1.rc == 0 and type1.info[1] == n // 2 + 1
    o = _run(lib, itype, Ab, Bb, 1)
    assert o.rc == 0
    assert o.info[1] == type1.info[1], (o.info[1], type1.info[1])
    assert o.info[3] == -5, o.info
    clean = _run(lib, itype, A, B, 1)
    assert clean.rc == 0 and not clean.info.any()
    for b in keep:
        _same(o, b, clean, b, 1, ("good problem against the clean batch", itype, b))
    assert o.wflat.size == batch * n and o.Zflat.size == batch * n * n      # compact: the slots are all there is
    iu = np.triu_indices(n, 1)
    for b in (1, 3):                           # a failed problem leaves the strictly upper triangles alone too
        assert np.array_equal(_bits(o.A[b][iu]), _bits(Ab[b][iu])) and np.array_equal(_bits(o.B[b][iu]), _bits(Bb[b][iu]))
    good = np.array(keep)
    o0 = _run(lib, itype, Ab, Bb, 0)
    assert o0.rc == 0 and list(o0.info) == list(o.info)
    assert np.array_equal(_bits(o0.w[good]), _bits(o.w[good]))
    assert np.all(o0.Zflat == SENTINEL)
    w, Z, info = hip.sygv_ybatched(Ab, Bb, itype=itype)
    assert list(info) == list(o.info) and np.array_equal(_bits(w[good]), _bits(o.w[good]))


# ------------------------------------------------------------------------------------------------- 7: hard pencils
@types23
def test_sygv_ybatched_hard_pencils(hip, itype):
    """Order 257: cond(B) = 1e6 and 1e10, A = B, the banded pencil and the Hilbert B (tests/batched_cases.py) in one
    launch, judged as tests/test_gpu_sygv_xbatched.py::test_sygv_xbatched_hard_pencils judges them: eigenvalues within
    4 max(n, 8) eps max|w_ref| of SciPy's, residual and orthogonality within 4 max(LAPACK's own, 16 n eps) with the factor
    the library left in dB (held to max|L L^T - B| <= 16 n eps max|B|); the same Z with LAPACK's factor against the limit
    that carries n eps cond2(B); the Hilbert B fails with the pivot type 1 of this class reports."""
    lib = hip.load_library()
    n = 257
    cases = [bc.make(name, n) for name in HARD_CASES]
    A, B = np.stack([c.A for c in cases]), np.stack([c.B for c in cases])
    o = _run(lib, itype, A, B, 1)
    o0 = _run(lib, itype, A, B, 0)
    assert o.rc == 0 and o0.rc == 0
    fails, worst, back_share = [], np.zeros(3), 0.0
    for b, c in enumerate(cases):
        what = "n=%d itype=%d %s" % (n, itype, c.name)
        if c.name == "hilbert_b":
            t1 = _device(lib, 1, A[b:b + 1], B[b:b + 1], 1, entry=TYPE1)
            if not (o.info[b] > 0 and o.info[b] == t1.info[0] == o0.info[b]):
                fails.append("%s: info %d / %d, type 1 says %d" % (what, o.info[b], o0.info[b], t1.info[0]))
            continue
        if o.info[b] != 0 or o0.info[b] != 0:
            fails.append("%s: info = %d / %d where 0 is required" % (what, o.info[b], o0.info[b]))
            continue
        w_ref, Z_ref = _ref(("yhard", c.name, n), itype, c.A, c.B)
        tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
        err = np.abs(o.w[b] - w_ref).max()
        L = np.tril(o.B[b])                         # the factor the kernel used, held to its own backward error
        back, back_lim = np.abs(L @ L.T - c.B).max(), 16 * n * EPS * np.abs(c.B).max()
        back_share = max(back_share, back / back_lim)
        if not back <= back_lim:
            fails.append("%s: |L L^T - B| = %.3e > %.3e" % (what, back, back_lim))
        res, orth = _quantities(itype, c.A, c.B, o.w[b], o.Z[b], L)
        res_l, orth_l = _quantities(itype, c.A, c.B, w_ref, Z_ref)
        lim_r, lim_o = 4 * max(res_l, 16 * n * EPS), 4 * max(orth_l, 16 * n * EPS)
        orth_f = _quantities(itype, c.A, c.B, o.w[b], o.Z[b])[1]  # the same Z measured with LAPACK's factor
        cond = np.linalg.cond(c.B)
        lim_f = 4 * max(orth_l, 16 * n * EPS, n * EPS * cond)     # cond(B) <= 16: the rule as it stands
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
    print("n=%d itype=%d: share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f, the factor's bound "
          "%.3f" % ((n, itype) + tuple(worst) + (back_share,)))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------- 8: the GPU's own check
@types23
def test_sygv_ybatched_behind_the_acceptance_check_at_512(hip, itype):
    """One pencil of order 512: the original A and B and the returned w and Z through ek_hip_check_sygvx_device; its
    res_max (out[2]) and orthogonality (out[3]) are within 256 n eps, the bound tests/test_gpu_check_sygv.py uses behind
    the solvers."""
    lib = hip.load_library()
    n = 512
    A, B = _pairs(900 + n + itype, 1, n)
    o = _run(lib, itype, A, B, 1)
    assert o.rc == 0 and not o.info.any()
    lim = 256 * n * EPS
    out, q = np.zeros(4), np.zeros(n)
    with _Dev(lib) as dev:
        dA, dB = dev.up(np.asfortranarray(A[0])), dev.up(np.asfortranarray(B[0]))
        dw, dZ = dev.up(np.ascontiguousarray(o.w[0])), dev.up(np.asfortranarray(o.Z[0]))
        rc = lib.ek_hip_check_sygvx_device(itype, n, n, dA, n, dB, n, dw, dZ, n, out.ctypes.data_as(_dp),
                                           q.ctypes.data_as(_dp))
    assert rc == 0
    print("n=%d itype=%d: res_max %.4f, orthogonality %.4f of 256 n eps" % (n, itype, out[2] / lim, out[3] / lim))
    assert out[2] <= lim and out[1] <= out[2] and out[3] <= lim, (out, lim)


# ------------------------------------------------------------------------------------------------- 9: cost
def test_sygv_ybatched_costs_what_type_1_costs(hip):
    """64 pencils of order 512 (8 seeded pairs, repeated), device seconds with vectors, best of 3 after a warm-up, the
    three types alternated in one process, inputs restored outside the clock: types 2 and 3 take at most 1.25 x type 1's
    time, the gate of tests/test_gpu_sygv_xbatched.py::test_sygv_xbatched_costs_what_type_1_costs (its reasoning: the
    congruence does 5 n^3 / 6 multiply-adds where type 1's reduction does 2 n^3 / 3, plus one n^2 transpose)."""
    lib = hip.load_library()
    n, batch = 512, 64
    A, B = _pairs(4000 + n, 8, n)
    A, B = np.tile(A, (8, 1, 1)), np.tile(B, (8, 1, 1))
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    info = np.zeros(batch, dtype=np.int32)
    best = {1: np.inf, 2: np.inf, 3: np.inf}
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))

        def run(itype):
            dev.put(dA, hA); dev.put(dB, hB)               # the call works in place: fresh inputs, outside the clock
            sec = ctypes.c_double(-1.0)
            rc = lib.ek_hip_sygv_ybatched_device(itype, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
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
