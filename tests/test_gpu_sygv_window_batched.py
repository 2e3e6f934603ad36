"""ek_hip_sygv_window_batched* on the GPU: a window of eigenpairs (RANGE 'I' / 'V') of A B x = l x (itype 2) and
B A x = l x (itype 3) for every pencil of a batch, orders 1 .. 128 on both sides of every class limit, batches of 8.

  1 accuracy       types 2 and 3, every window of window_batched_cases.windows, 'I' and 'V', jobz 0 and 1, against SciPy's
                   full spectrum of the type, sliced, under the bounds of tests/sygv_window_cases.py; m is the reference
                   count; jobz = 0 leaves Z alone.  An entry that ignores itype fails here
  2 between types  itype 1 is ek_hip_eigenpairs_window_batched_device(problem = 1) bit for bit in m, info, w, Z, dA and dB;
                   types 2 and 3 share w, m and dA bit for bit, dB is type 1's L, jobz = 0 gives the same w and dA,
                   max|B Z2 - Z3| / max|Z3| <= 256 n eps, and type 2's w is not type 1's
  3 the full call  dA and dB are what ek_hip_sygv_batched_device leaves, bit for bit; w within the eigenvalue bound of its w
  4 bits           the value of index k is the same bits in every window that holds it, for both ranges and both jobz,
                   alone and in a batch of 8, at another position, across a chunk seam and through the host form
  5 left alone     NaN in the strictly upper triangles, rows n .. ld - 1, the gaps, the rest of a row of w and the columns
                   of Z from m[b] on come back bit for bit -- type 3 in particular, whose Z <- L Z stops at the window
  6 own slots      a non-SPD B, a NaN in A, a 'V' window wider than zcap (-20, m the count, nothing written) and an empty
                   'V' window (m = 0, info 0) in one batch: the neighbours keep the bits of a clean run
  7 hard pencils   cond_b:1e6, cond_b:1e10, a_equals_b, band5_band5 under the rule with the library's own factor; the
                   planted-cluster pencils with the cluster-cut window and the whole spectrum; no 200000 + k;
                   band5_band5 times 2^+-531 returns 2^k w and the same Z, to the bit
  8 the GPU check  two problems per type through ek_hip_check_sygvx_device on the window's m columns
  9 cost           device seconds, best of 3 after a warm-up, kinds alternated in one process: a window of n / 8 pairs
                   with vectors and all n values without take <= 0.6 of ek_hip_sygv_batched_device of the same type and
                   jobz, and <= 1.25 of the type-1 window call

The groups are plain functions of a Config, so that tests/test_gpu_sygv_window_xbatched.py runs them at orders 129 .. 256.

Largest shares of the bounds used on one MI355X (eigenvalues / residual / orthogonality): random pairs 0.052 / 0.006 /
0.004, Z3 = B Z2 0.0026, hard pencils 0.074 / 0.012 / 0.395 of the rule, planted clusters 0.030 / 0.009 / 0.010, behind the
GPU's own check < 0.0001 / 0.0012."""
import collections
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import sygv_window_cases as sw
import window_batched_cases as wc
from test_gpu_sygv_batched import _bits, _device
from test_gpu_vbatched import _Dev
from test_gpu_window_batched import _untouched

pytestmark = pytest.mark.gpu
EPS = sw.EPS
ORDERS = (1, 2, 3, 31, 32, 33, 64, 65, 128)
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)

Config = collections.namedtuple("Config", "window eigenpairs full mirror chunk")
CFG = Config("ek_hip_sygv_window_batched_device", "ek_hip_eigenpairs_window_batched_device",
             "ek_hip_sygv_batched_device", "sygv_window_batched", "window_batched_chunk")


def _run(lib, cfg, itype, A, B, jobz, **kw):
    return sw.window_device(lib, cfg.window, itype, A, B, jobz, **kw)


def _refs(n, itype, batch=8):
    A, B = sw.pairs(n, batch)
    return A, B, [sw.reference(("pairs", n, b), itype, A[b], B[b]) for b in range(batch)]


def _bounds(n, il, iu):
    """The 'V' bounds of a window for the random pairs of an order: clear of the reference spectra of both types (the
    host test checks them on exactly this list).  Returns vl, vu and the spans of the 8 pairs."""
    A, B = sw.pairs(n)
    both = [sw.reference(("pairs", n, b), t, A[b], B[b])[0] for t in (2, 3) for b in range(A.shape[0])]
    vl, vu, span = wc.value_bounds(both, il, iu)
    return vl, vu, span[:A.shape[0]]


def _low(n):
    return np.tril(np.ones((n, n), dtype=bool))


# ------------------------------------------------------------------------------------------------------- 1: accuracy
def check_accuracy(hip, cfg, n, itype):
    lib = hip.load_library()
    A, B, ref = _refs(n, itype)
    batch = A.shape[0]
    worst, fails = [0.0, 0.0, 0.0], []
    for wname, il, iu in wc.windows(n):
        vl, vu, span = _bounds(n, il, iu)
        for by_value in (False, True):
            for jobz in (0, 1):
                what = "n=%d itype=%d %s %s jobz=%d" % (n, itype, wname, "V" if by_value else "I", jobz)
                o = (_run(lib, cfg, itype, A, B, jobz, vl=vl, vu=vu, pad=3, gap=5) if by_value
                     else _run(lib, cfg, itype, A, B, jobz, il=il, iu=iu, pad=3, gap=5))
                assert o.rc == 0 and not o.info.any(), (what, o.rc, o.info)
                _untouched(o, n, what)
                if not jobz:
                    assert np.all(np.isnan(o.flatZ)), what + ": Z written under jobz = 0"
                for b in range(batch):
                    first, m = span[b] if by_value else (il - 1, iu - il + 1)
                    # the count of this type's own reference spectrum
                    if by_value:
                        assert m == int(((ref[b][0] > vl) & (ref[b][0] <= vu)).sum()), (what, b)
                    assert o.m[b] == m, (what, b, o.m[b], m)
                    s, f = sw.judge(itype, A[b], B[b], ref[b][0], first, o.w[b, :m], o.Z[b][:, :m] if jobz else None,
                                    "%s b=%d" % (what, b))
                    fails += f
                    worst = sw.worse(worst, s)
    print("n=%d itype=%d share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, itype) + tuple(worst)))
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", ORDERS)
def test_accuracy_against_scipy(hip, n, itype):
    check_accuracy(hip, CFG, n, itype)


# -------------------------------------------------------------------------------------------------- 2: between the types
def check_between_the_types(hip, cfg, n):
    lib = hip.load_library()
    A, B = sw.pairs(n)
    batch = A.shape[0]
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    vl, vu, span = _bounds(n, il, iu)
    worst = 0.0
    for kw in (dict(il=il, iu=iu), dict(vl=vl, vu=vu)):
        t = {(i, j): _run(lib, cfg, i, A, B, j, pad=1, gap=2, **kw) for i in (1, 2, 3) for j in (0, 1)}
        for key, o in t.items():
            assert o.rc == 0 and not o.info.any(), (key, o.rc, o.info)
        for j in (0, 1):
            p = sw.window_device(lib, cfg.eigenpairs, 1, A, B, j, pad=1, gap=2, **kw)
            assert p.rc == 0
            assert np.array_equal(t[1, j].info, p.info) and np.array_equal(t[1, j].m, p.m)
            for name in ("w", "flatZ", "flatA", "flatB"):
                assert np.array_equal(_bits(getattr(t[1, j], name)), _bits(getattr(p, name))), ("itype 1", j, name)
            assert np.array_equal(t[2, j].m, t[3, j].m), ("m of types 2 and 3", j)
            assert np.array_equal(_bits(t[2, j].w), _bits(t[3, j].w)), ("w of types 2 and 3", j)
            assert np.array_equal(_bits(t[2, j].flatA), _bits(t[3, j].flatA)), ("dA of types 2 and 3", j)
            for i in (2, 3):
                assert np.array_equal(_bits(t[i, j].flatB), _bits(t[1, j].flatB)), ("dB against type 1's L", i, j)
                assert np.array_equal(t[i, j].m, t[i, 1].m)
                assert np.array_equal(_bits(t[i, j].w), _bits(t[i, 1].w)), ("values only gives another w", i)
                assert np.array_equal(_bits(t[i, j].flatA), _bits(t[i, 1].flatA)), ("values only leaves another dA", i)
        for b in range(batch):
            m = int(t[2, 1].m[b])
            if m:
                Z2, Z3 = t[2, 1].Z[b][:, :m], t[3, 1].Z[b][:, :m]
                worst = max(worst, np.abs(B[b] @ Z2 - Z3).max() / np.abs(Z3).max())
        if "il" in kw:
            m = iu - il + 1
            assert not np.array_equal(t[2, 1].w[:, :m], t[1, 1].w[:, :m])     # another problem than type 1's
    print("n=%d: max|B Z2 - Z3| / max|Z3| uses %.4f of 256 n eps" % (n, worst / (256 * n * EPS)))
    assert worst <= 256 * n * EPS, (worst, 256 * n * EPS)


@pytest.mark.parametrize("n", ORDERS)
def test_invariants_between_the_types(hip, n):
    check_between_the_types(hip, CFG, n)


# ---------------------------------------------------------------------------------------------- 3: against the full call
def check_against_the_full_call(hip, cfg, n, itype):
    lib = hip.load_library()
    A, B = sw.pairs(n)
    low = _low(n)
    for jobz in (0, 1):
        full = _device(lib, itype, A, B, jobz, entry=cfg.full)
        assert full.rc == 0 and not full.info.any()
        for wname, il, iu in wc.windows(n):
            o = _run(lib, cfg, itype, A, B, jobz, il=il, iu=iu)
            assert o.rc == 0 and not o.info.any()
            assert np.array_equal(_bits(o.A[:, low]), _bits(full.A[:, low])), (wname, jobz, "dA is not the full call's")
            assert np.array_equal(_bits(o.B[:, low]), _bits(full.B[:, low])), (wname, jobz, "dB is not the full call's")
            for b in range(A.shape[0]):
                lim = 4 * max(n, 8) * EPS * np.abs(full.w[b]).max()
                assert np.abs(o.w[b, :iu - il + 1] - full.w[b, il - 1:iu]).max() <= lim, (wname, jobz, b)


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", ORDERS)
def test_images_are_those_of_the_full_call(hip, n, itype):
    check_against_the_full_call(hip, CFG, n, itype)


# ------------------------------------------------------------------------------------------------------------ 4: bits
def check_bits_of_the_values(hip, cfg, n, itype, chunk=3):
    lib = hip.load_library()
    A, B = sw.pairs(n)
    batch = A.shape[0]
    whole = _run(lib, cfg, itype, A, B, 0, il=1, iu=n)
    assert whole.rc == 0 and not whole.info.any()
    for wname, il, iu in wc.windows(n):
        m = iu - il + 1
        vl, vu, span = _bounds(n, il, iu)
        for jobz in (0, 1):
            o = _run(lib, cfg, itype, A, B, jobz, il=il, iu=iu, zcap=n)
            assert np.array_equal(_bits(o.w[:, :m]), _bits(whole.w[:, il - 1:iu])), (wname, jobz, "I")
            o = _run(lib, cfg, itype, A, B, jobz, vl=vl, vu=vu)
            for b, (first, mb) in enumerate(span):
                assert o.m[b] == mb
                assert np.array_equal(_bits(o.w[b, :mb]), _bits(whole.w[b, first:first + mb])), (wname, jobz, "V", b)
    # alone, at another position, across a chunk seam, in the host form: w, and with them Z and the images
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    m = iu - il + 1
    low = _low(n)
    ref = _run(lib, cfg, itype, A, B, 1, il=il, iu=iu)
    alone = _run(lib, cfg, itype, A[2:3], B[2:3], 1, il=il, iu=iu)
    perm = np.roll(np.arange(batch), 3)             # problem b of the batch sits at position (b + 3) % batch
    moved = _run(lib, cfg, itype, A[perm], B[perm], 1, il=il, iu=iu, pad=2, gap=1)
    before = getattr(hip, cfg.chunk)(chunk)
    try:
        seam = _run(lib, cfg, itype, A, B, 1, il=il, iu=iu)
    finally:
        getattr(hip, cfg.chunk)(before)
    assert getattr(hip, cfg.chunk)(before) == before

    def same(o, pos, b, what):
        assert o.rc == 0 and o.info[pos] == 0 and o.m[pos] == m, what
        assert np.array_equal(_bits(o.w[pos, :m]), _bits(ref.w[b, :m])), what + ": w"
        assert np.array_equal(_bits(o.Z[pos][:, :m]), _bits(ref.Z[b][:, :m])), what + ": Z"
        assert np.array_equal(_bits(o.A[pos][low]), _bits(ref.A[b][low])), what + ": dA"
        assert np.array_equal(_bits(o.B[pos][low]), _bits(ref.B[b][low])), what + ": dB"

    same(alone, 0, 2, "alone")
    for pos in range(batch):
        same(moved, pos, int(perm[pos]), "moved to position %d" % pos)
        same(seam, pos, pos, "chunks of %d, position %d" % (chunk, pos))
    A_in, B_in = A.copy(), B.copy()
    w, Z, mm, info = getattr(hip, cfg.mirror)(A, B, itype=itype, il=il, iu=iu)
    assert not info.any() and np.all(mm == m)
    assert np.array_equal(_bits(w[:, :m]), _bits(ref.w[:, :m])), "host form: w"
    assert np.array_equal(_bits(Z[:, :, :m]), _bits(ref.Z[:, :, :m])), "host form: Z"
    assert not w[:, m:].any(), "host form: w written behind m"
    assert np.array_equal(_bits(A), _bits(A_in)) and np.array_equal(_bits(B), _bits(B_in)), "host form: A or B written"


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [3, 33, 64, 128])
def test_value_of_an_index_is_the_same_bits_everywhere(hip, n, itype):
    check_bits_of_the_values(hip, CFG, n, itype)


# ------------------------------------------------------------------------------------------------------ 5: left alone
def check_left_alone(hip, cfg, n, itype):
    """zcap above every m[b], ld above n, gaps between the problems: what is not the call's is NaN before and after."""
    lib = hip.load_library()
    A, B = sw.pairs(n)
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    vl, vu, span = _bounds(n, il, iu)
    zcap = min(n, max(mb for _, mb in span) + 2)
    for kw in (dict(il=il, iu=iu, zcap=min(n, iu - il + 3)), dict(vl=vl, vu=vu, zcap=zcap), dict(il=1, iu=1, zcap=n)):
        for jobz in (1, 0):
            o = _run(lib, cfg, itype, A, B, jobz, pad=3, gap=5, **kw)
            assert o.rc == 0 and not o.info.any(), (kw, o.info)
            _untouched(o, n, "n=%d itype=%d %s jobz=%d" % (n, itype, sorted(kw), jobz))
            if jobz:
                for b in range(A.shape[0]):
                    assert np.all(np.isfinite(o.Z[b][:, :o.m[b]])), (kw, b)


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [2, 33, 65, 128])
def test_what_is_not_the_calls_is_left_alone(hip, n, itype):
    check_left_alone(hip, CFG, n, itype)


# -------------------------------------------------------------------------------------------------------- 6: own slots
def check_failures_keep_to_their_own_slots(hip, cfg, n, itype):
    lib = hip.load_library()
    A, B, ref = _refs(n, itype)
    idx = np.arange(9) % 5
    A9, B9 = A[idx].copy(), B[idx].copy()
    w0 = ref[0][0]
    vl, vu = 0.5 * (w0[n // 4 - 1] + w0[n // 4]), 0.5 * (w0[n // 2 - 1] + w0[n // 2])
    count = lambda a, b: int(((sl.eigh(a, b, type=itype, eigvals_only=True) > vl)           # noqa: E731
                              & (sl.eigh(a, b, type=itype, eigvals_only=True) <= vu)).sum())
    zcap = max(count(A9[b], B9[b]) for b in range(5)) + 1
    clean = _run(lib, cfg, itype, A9, B9, 1, vl=vl, vu=vu, zcap=zcap)
    assert clean.rc == 0 and not clean.info.any() and clean.m.min() > 0
    inv = lambda M: (np.linalg.inv(M) + np.linalg.inv(M).T) / 2.0                            # noqa: E731
    B9[1] = B9[1] - 3.0 * np.eye(n)                 # not SPD
    A9[3, n // 2, 0] = np.nan                       # lower triangle
    A9[5] = 1e-6 * A9[5] + 0.5 * (vl + vu) * inv(B9[5])   # L^T A L = mid I + small: every eigenvalue inside (vl, vu]
    A9[7] = A9[7] + 1e4 * inv(B9[7])                # L^T A L moves up by 1e4: an empty window
    assert count(A9[5], B9[5]) == n > zcap and count(A9[7], B9[7]) == 0
    o = _run(lib, cfg, itype, A9, B9, 1, vl=vl, vu=vu, zcap=zcap)
    assert o.rc == 0
    assert o.info[1] > 0 and o.m[1] == 0
    assert o.info[3] == -5 and o.m[3] == 0
    assert o.info[5] == -20 and o.m[5] == n
    assert o.info[7] == 0 and o.m[7] == 0
    for b in (1, 3, 5, 7):
        assert np.all(np.isnan(o.w[b])) and np.all(np.isnan(o.Z[b])), b
    _untouched(o, n, "planted")
    for b in (0, 2, 4, 6, 8):
        assert o.info[b] == 0 and o.m[b] == clean.m[b]
        assert np.array_equal(_bits(o.w[b, :o.m[b]]), _bits(clean.w[b, :o.m[b]])), b
        assert np.array_equal(_bits(o.Z[b][:, :o.m[b]]), _bits(clean.Z[b][:, :o.m[b]])), b
        assert np.array_equal(_bits(o.A[b][_low(n)]), _bits(clean.A[b][_low(n)])), b
        assert np.array_equal(_bits(o.B[b][_low(n)]), _bits(clean.B[b][_low(n)])), b


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [33, 128])
def test_failures_keep_to_their_own_slots(hip, n, itype):
    check_failures_keep_to_their_own_slots(hip, CFG, n, itype)


# ------------------------------------------------------------------------------------------ 7: hard pencils and clusters
def check_hard_pencils(hip, cfg, n, itype):
    """The four hard pencils in one launch per window, under the rule of test_sygv_batched_hard_pencils: eigenvalues with
    no cond(B) factor, residual and orthogonality <= 4 max(LAPACK's full driver's own, 16 n eps), type 3's orthogonality
    with the factor the library left in dB, that factor held to its backward error."""
    lib = hip.load_library()
    AB = [sw.hard(name, n) for name in sw.HARD]
    A, B = np.stack([a for a, _ in AB]), np.stack([b for _, b in AB])
    worst, fails = [0.0, 0.0, 0.0], []
    for wname, il, iu in wc.windows(n):
        o = _run(lib, cfg, itype, A, B, 1, il=il, iu=iu)
        assert o.rc == 0
        assert not o.info.any(), (wname, o.info)
        for b, name in enumerate(sw.HARD):
            what = "n=%d itype=%d %s %s" % (n, itype, name, wname)
            w_ref, Z_ref = sw.reference(("hard", name, n), itype, A[b], B[b])
            L = np.tril(o.B[b])
            back = np.abs(L @ L.T - B[b]).max()
            if not back <= 16 * n * EPS * np.abs(B[b]).max():
                fails.append("%s: |L L^T - B| = %.3e" % (what, back))
            rule = sw.quantities(itype, A[b], B[b], w_ref, Z_ref)
            m = iu - il + 1
            s, f = sw.judge(itype, A[b], B[b], w_ref, il - 1, o.w[b, :m], o.Z[b][:, :m], what, rule=rule, L=L)
            fails += f
            worst = sw.worse(worst, s)
    print("n=%d itype=%d hard pencils, share of the rule used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, itype) + tuple(worst)))
    assert not fails, "\n".join(fails[:40])


def check_planted_clusters(hip, cfg, n, itype):
    """The planted-cluster pencils with the window that cuts their clusters and with the whole spectrum, two copies of a
    pencil per launch (all_equal with all pairs wanted is n rounds of inverse iteration): info 0 (no 200000 + k), the
    suite's bounds, and both copies the same bits."""
    lib = hip.load_library()
    worst, fails = [0.0, 0.0, 0.0], []
    for name in wc.CLUSTERED:
        A, B, C = sw.planted(name, n)
        w_ref = sw.reference(("planted", name, n), itype, A, B)[0]
        cut = wc.cluster_cut(w_ref)
        assert cut is not None and cut == wc.cluster_cut(sl.eigvalsh(C)), (name, n)
        Ab, Bb = np.stack([A, A]), np.stack([B, B])
        for wname, il, iu in (("cluster cut",) + cut, ("whole", 1, n)):
            what = "n=%d itype=%d %s %s %d..%d" % (n, itype, name, wname, il, iu)
            o = _run(lib, cfg, itype, Ab, Bb, 1, il=il, iu=iu)
            assert o.rc == 0 and not o.info.any(), (what, o.info)
            m = iu - il + 1
            assert np.array_equal(_bits(o.w[0]), _bits(o.w[1])) and np.array_equal(_bits(o.Z[0]), _bits(o.Z[1])), what
            s, f = sw.judge(itype, A, B, w_ref, il - 1, o.w[0, :m], o.Z[0][:, :m], what)
            fails += f
            worst = sw.worse(worst, s)
    print("n=%d itype=%d planted clusters, share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, itype) + tuple(worst)))
    assert not fails, "\n".join(fails[:40])


def check_scale_covariance(hip, cfg, n, itype):
    """band5_band5 times 2^531 and 2^-531: 2^k w and the same Z, to the bit."""
    lib = hip.load_library()
    base = bc.make("band5_band5", n)
    cases = [base, bc.scaled(base, 531), bc.scaled(base, -531)]
    A, B = np.stack([c.A for c in cases]), np.stack([c.B for c in cases])
    il, iu = n // 4 + 1, n // 2
    m = iu - il + 1
    o = _run(lib, cfg, itype, A, B, 1, il=il, iu=iu)
    assert o.rc == 0 and not o.info.any(), o.info
    for b, k in ((1, 531), (2, -531)):
        assert np.array_equal(_bits(o.w[b, :m]), _bits(np.ldexp(o.w[0, :m], k))), k
        assert np.array_equal(_bits(o.Z[b][:, :m]), _bits(o.Z[0][:, :m])), k
    w_ref = sw.reference(("hard", "band5_band5", n), itype, base.A, base.B)[0]
    _, f = sw.judge(itype, base.A, base.B, w_ref, il - 1, o.w[0, :m], o.Z[0][:, :m], "band5_band5")
    assert not f, f


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [3, 33, 128])
def test_hard_pencils_under_the_rule(hip, n, itype):
    check_hard_pencils(hip, CFG, n, itype)


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [33, 128])
def test_planted_clusters(hip, n, itype):
    check_planted_clusters(hip, CFG, n, itype)


@pytest.mark.parametrize("itype", [2, 3])
def test_scale_covariance(hip, itype):
    check_scale_covariance(hip, CFG, 65, itype)


# ------------------------------------------------------------------------------------------ 8: behind the GPU's own check
def check_behind_the_gpu_check(hip, cfg, n, itype):
    lib = hip.load_library()
    A, B = sw.pairs(n)
    A, B = A[:2], B[:2]
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    m = iu - il + 1
    o = _run(lib, cfg, itype, A, B, 1, il=il, iu=iu)
    assert o.rc == 0 and not o.info.any()
    lim = 256 * n * EPS
    for b in range(2):
        out, q = np.zeros(4), np.zeros(m)
        hA = np.asfortranarray(A[b]).ravel(order="F").copy()
        hB = np.asfortranarray(B[b]).ravel(order="F").copy()
        hZ = np.asfortranarray(o.Z[b][:, :m]).ravel(order="F").copy()
        hw = o.w[b, :m].copy()
        with _Dev(lib) as dev:
            dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
            rc = lib.ek_hip_check_sygvx_device(itype, n, m, dA, n, dB, n, dw, dZ, n, out.ctypes.data_as(_dp),
                                               q.ctypes.data_as(_dp))
        assert rc == 0
        print("n=%d itype=%d problem %d, %d columns: res_max %.4f, orthogonality %.4f of 256 n eps"
              % (n, itype, b, m, out[2] / lim, out[3] / lim))
        assert out[2] <= lim and out[3] <= lim, (out, lim)


@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("n", [33, 128])
def test_behind_the_gpus_own_check(hip, n, itype):
    check_behind_the_gpu_check(hip, CFG, n, itype)


# ------------------------------------------------------------------------------------------------------------ 9: cost
def speed(lib, cfg, n, batch):
    """Device seconds, best of 3 after a warm-up round, the kinds alternated in one process, inputs restored outside the
    clock (every call works in place).  Kinds: (itype, 'full1' | 'full0' | 'window' | 'values') for itype 2 and 3, and
    the type-1 window call as (1, 'window') and (1, 'values')."""
    A8, B8 = sw.pairs(n)
    A, B = A8[np.arange(batch) % 8], B8[np.arange(batch) % 8]
    hA = np.ascontiguousarray(A.transpose(0, 2, 1)).ravel()
    hB = np.ascontiguousarray(B.transpose(0, 2, 1)).ravel()
    info = np.zeros(batch, dtype=np.int32)
    m = np.zeros(batch, dtype=np.int32)
    sec = ctypes.c_double(0.0)
    best = {}
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        ipp, mp = info.ctypes.data_as(_ip), m.ctypes.data_as(_ip)

        def full(itype, jobz):
            return getattr(lib, cfg.full)(itype, jobz, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ if jobz else None, n,
                                          n * n, ipp, ctypes.byref(sec))

        def window(itype, jobz, iu):
            return getattr(lib, cfg.window)(itype, jobz, 0, n, batch, 0.0, 0.0, 1, iu, dA, n, n * n, dB, n, n * n, mp, dw,
                                            dZ if jobz else None, n, n, n * n, ipp, ctypes.byref(sec))

        kinds = {}
        for itype in (1, 2, 3):
            kinds[itype, "window"] = lambda t=itype: window(t, 1, n // 8)
            kinds[itype, "values"] = lambda t=itype: window(t, 0, n)
            if itype != 1:
                kinds[itype, "full1"] = lambda t=itype: full(t, 1)
                kinds[itype, "full0"] = lambda t=itype: full(t, 0)
        for rep in range(4):                        # the first round warms up
            for name, fn in kinds.items():
                dev.put(dA, hA)
                dev.put(dB, hB)
                assert fn() == 0 and not info.any(), (name, info[info != 0][:4])
                if rep:
                    best[name] = min(best.get(name, np.inf), sec.value)
    return best


def check_cost(hip, cfg, n, batch, gate):
    t = speed(hip.load_library(), cfg, n, batch)
    fails = []
    for itype in (2, 3):
        r1, r0 = t[itype, "window"] / t[itype, "full1"], t[itype, "values"] / t[itype, "full0"]
        q1, q0 = t[itype, "window"] / t[1, "window"], t[itype, "values"] / t[1, "values"]
        print("n=%d batch=%d itype=%d ms: full with vectors %.3f, window of n/8 with vectors %.3f (%.3f of it, %.3f of "
              "type 1's window); full values %.3f, all values by bisection %.3f (%.3f of it, %.3f of type 1's)"
              % (n, batch, itype, 1e3 * t[itype, "full1"], 1e3 * t[itype, "window"], r1, q1, 1e3 * t[itype, "full0"],
                 1e3 * t[itype, "values"], r0, q0))
        for what, r, lim in (("window / full", r1, gate), ("values / full", r0, gate), ("window / type 1's", q1, 1.25),
                             ("values / type 1's", q0, 1.25)):
            if not r <= lim:
                fails.append("n=%d itype=%d %s: %.3f > %.2f" % (n, itype, what, r, lim))
    assert not fails, fails


@pytest.mark.parametrize("n,batch", [(128, 512), (64, 1024)])
def test_a_window_of_types_2_and_3_costs_what_it_should(hip, n, batch):
    """<= 0.6 of ek_hip_sygv_batched_device of the same type and jobz (the gate of the type-1 window call against its full
    call; that call's kernels are the parent's instructions), and <= 1.25 of the type-1 window call of the same build
    (the project's gate for types 2 / 3 against type 1: their full calls measure 0.95 .. 1.01 of type 1's, so the
    reductions differ by about 5 % of a full call, which is about 12 % of a window call at 0.4 of it).
    Measured on one MI355X, types 2 / 3: 512 pencils of order 128: window / full 0.346 / 0.354, values /
    full 0.282 / 0.282, window / type 1's 0.918 / 0.948, values / type 1's 0.893 / 0.893; 1024 of order 64: 0.431 / 0.437,
    0.391 / 0.393, 0.944 / 0.971, 0.930 / 0.934.  None is within 10 % of its gate."""
    check_cost(hip, CFG, n, batch, 0.6)
