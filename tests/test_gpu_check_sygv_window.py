"""GPU suite of the window check of DSYGV's types (ek_hip_check_sygv_window_xbatched*): norm, res_ave,
res_max, orthogonality and the inverse participation ratios of the m[b] columns that problem b of a batch holds in its
n x zcap array, types 2 (A B x = l x) and 3 (B A x = l x), orders 1 .. 256.

  1 the mirror      types 2 and 3, device and host form, every order of tests/check_window_cases.py: ONE call carries all
                    column counts of the order as different m[b], clean and planted, within 4 max(n, 8) eps of the host
                    mirror verifier.*_sygv on Z[:, :c], w[:c] (max(1, cond_2(B)) wider for slot 3 and the IPRs of type 3)
  2 m per problem   m = 0, 1, 16, 17, 64, 65, n in one batch with zcap = n: the bits of each problem alone with zcap = m
  3 type 1, type 2  itype = 1 is ek_hip_check_window_xbatched_device(1, ...) to the bit; type 2's slot 3 and IPRs are that
                    call's bits for the same (B, Z, m)
  4 bits            another position, another batch, another zcap / ldz / stride, the host form, a chunk seam (7 problems,
                    3 a launch)
  5 never read      NaN in the columns of Z and in w from m[b] on, in the strictly upper triangles, the rows n .. ld-1 and
                    the gaps: the bits of a clean run; A, B, w, Z come back byte for byte
  6 own slots       a skipped problem, a -20 problem with m > zcap, an empty window and a NaN in one problem's Z in one
                    batch; a B with B[k, k] negated (k = 0, n - 1): type 3 reports NaN in slot 3 and the m[b] IPRs, keeps
                    the residual slots, returns 0 and leaves the neighbours alone; type 2 gives numbers
  7 m = n           within twice the bounds of ek_hip_check_sygv_xbatched_device on the same full Z
  8 the solver      ek_hip_sygv_window_xbatched_device's m, w, Z, info handed over unchanged, 'I' and 'V': res_max and
                    orthogonality <= 256 n eps (tests/test_gpu_sygv_window_xbatched.py), the first problem within the
                    bounds of ek_hip_check_sygvx_device(itype, n, m[0])
  9 cost            256 pencils, a window of n / 8 columns: cheaper than the full check of the same batch, no dearer than
                    the window solve, faster than the host loop over ek_hip_check_sygvx_device

Each test prints the largest share of the bounds it used (pytest -s shows it).  Largest shares on one MI355X: against
the mirror 0.066 (an IPR; norm 0.021, res_ave and res_max 0.004, orthogonality 0.017), m = n against the full check 0.009 of
twice the bounds, against ek_hip_check_sygvx_device 0.018; behind the solver res_max below 0.0001 and orthogonality 0.0028
of 256 n eps; cost, types 2 / 3 at n = 128, 129, 256: window / full 0.134, 0.219, 0.189 / 0.426, 0.481, 0.329, window / solve
0.028, 0.029, 0.019 / 0.173, 0.167, 0.163, host loop / window 228, 177, 98 / 91, 106, 33, window / type 1's window check
1.12, 1.21, 1.14 / 7.11, 7.09, 9.77."""
import ctypes
import time

import numpy as np
import pytest

import check_sygv_window_cases as cs
import window_batched_cases as wc
from test_gpu_check_window import SENTINEL, _Dev, _nan_upper, _Out, _pack, _same

pytestmark = pytest.mark.gpu
EPS = cs.EPS
COUNT = cs.COUNT
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
SYGV = "ek_hip_check_sygv_window_xbatched"
PLAIN = "ek_hip_check_window_xbatched"
WAYS = [(2, "device"), (2, "host"), (3, "device"), (3, "host")]
ways = pytest.mark.parametrize("itype,form", WAYS)


def _window(lib, form, first, A, B, m, ws, Zs, zcap, info=None, ipr=True, pad=0, fill=SENTINEL, entry=SYGV):
    """entry[_device](first, ...).  Problem b: the first m[b] values of ws[b] and columns of Zs[b] (n x at least m[b];
    nothing of them when the problem is skipped or m[b] exceeds what there is) in a row of w and an n x zcap array; every
    other word of w and Z, the rows n .. ld-1 and the gaps hold `fill`.  pad = 0: the compact layout; pad > 0: leading
    dimensions n + pad .. and strides beyond.  o.untouched: A, B, w, Z after the call equal those before."""
    batch, n = A.shape[0], A.shape[1]
    m = np.asarray(m, dtype=np.int32)
    lda, ldb, ldz = (n + pad, n + 2 * pad, n + 3 * pad) if pad else (n, n, n)
    sA, sB = lda * n + (5 if pad else 0), ldb * n + (3 if pad else 0)
    sZ = ldz * max(zcap, 1) + (7 if pad else 0)
    hw = np.full(batch * n, fill)
    hZ = np.full(batch * sZ, fill)
    it = hZ.itemsize
    Zv = np.lib.stride_tricks.as_strided(hZ, shape=(batch, max(zcap, 1), n), strides=(sZ * it, ldz * it, it))
    for b in range(batch):
        k = int(m[b])
        if (info is not None and info[b] != 0) or not 0 < k <= min(zcap, n):
            continue
        hw[b * n:b * n + k] = ws[b][:k]
        Zv[b, :k, :] = Zs[b][:, :k].T
    h = [_pack(A, lda, sA, fill), _pack(B, ldb, sB, fill), hw, hZ]
    out = np.full(batch * 4 + 2, SENTINEL)
    q = np.full(batch * n + 3, SENTINEL)
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    marr = m.copy()
    sec = ctypes.c_double(-1.0)
    o = _Out()
    tail = (None if iarr is None else iarr.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
            q.ctypes.data_as(_dp) if ipr else None, ctypes.byref(sec))
    mp = marr.ctypes.data_as(_ip)
    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) for x in h]
            o.rc = getattr(lib, entry + "_device")(first, n, batch, d[0], lda, sA, d[1], ldb, sB, mp, d[2], d[3], ldz, zcap,
                                                   sZ, *tail)
            o.untouched = all(_same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [x.copy() for x in h]
        P = [x.ctypes.data_as(_dp) for x in g]
        o.rc = getattr(lib, entry)(first, n, batch, P[0], lda, sA, P[1], ldb, sB, mp, P[2], P[3], ldz, zcap, sZ, *tail)
        o.untouched = all(_same(y, x) for y, x in zip(g, h))
    o.seconds = sec.value
    o.out, o.ipr = out[:batch * 4].reshape(batch, 4), q[:batch * n].reshape(batch, n)
    o.tails = (out[batch * 4:], q[batch * n:] if ipr else q)
    assert np.array_equal(marr, m) and (iarr is None or np.array_equal(iarr, np.asarray(info, dtype=np.int32)))
    return o


def _clean(o, m, n, info=None):
    """The call succeeded, wrote nothing behind out and ipr, nothing of an ipr row from m[b] on, nothing of A, B, w, Z."""
    assert o.rc == 0 and o.untouched and o.seconds >= 0.0
    assert np.all(o.tails[0] == SENTINEL) and np.all(o.tails[1] == SENTINEL)
    for b, k in enumerate(m):
        live = (info is None or info[b] == 0) and k > 0
        assert np.all(o.ipr[b, (k if live else 0):] == SENTINEL)
        if not live:
            assert np.all(np.isnan(o.out[b]))


def _assert_shares(shares, what):
    shares = np.asarray(shares).reshape(-1, 5).max(axis=0)
    print("shares of the bounds %s: " % (what,) + ", ".join("%s %.3f" % kv for kv in zip(cs.NAMES, shares)))
    assert np.all(shares <= 1.0), (what, shares)


def _pick(n, itype, idx, cols, plant=True):
    """Problem idx[k] of the table with a window of cols[k] columns, per entry: A, B, ws, Zs, mirrors, cond_2(B)."""
    case = cs.cases(n, itype)
    idx = np.asarray(idx)
    ws, Zs, ref = [], [], []
    for b, c in zip(idx, cols):
        if c > 0:
            w, Z = cs.window(n, itype, int(b), int(c), plant)
            ws.append(w)
            Zs.append(Z)
            ref.append(cs.mirrored(n, itype, int(b), int(c), plant))
        else:
            ws.append(np.zeros(0))
            Zs.append(np.zeros((n, 0)))
            ref.append(None)
    return case.A[idx], case.B[idx], ws, Zs, ref, case.cond[idx]


# --------------------------------------------------------------------------------------------- 1: against the host mirror
@ways
@pytest.mark.parametrize("n", cs.ORDERS)
def test_matches_the_host_mirror(hip, n, itype, form):
    """All column counts of the order in one call, one problem each (problem k % COUNT of the table), padded layout with one
    spare column, the gaps and the spare column holding a sentinel.  Clean and planted windows; the planted one moves
    res_ave, res_max and orthogonality by what the mirror's move by, within twice the bound."""
    lib = hip.load_library()
    tol = cs.tol(n)
    m = list(cs.columns(n))
    idx = np.arange(len(m)) % COUNT
    shares, got = [], []
    for plant in (False, True):
        A, B, ws, Zs, ref, cond = _pick(n, itype, idx, m, plant)
        o = _window(lib, form, itype, A, B, m, ws, Zs, n + 1, pad=3)
        _clean(o, m, n)
        for k, c in enumerate(m):
            s = cs.shares(itype, o.out[k], o.ipr[k, :c], ref[k][0], ref[k][1], n, cond[k])
            print("n=%d itype=%d %s c=%d %s: " % (n, itype, form, c, "planted" if plant else "clean")
                  + " ".join("%.3f" % x for x in s))
            shares.append(s)
        got.append((o, ref))
    (o0, r0), (o1, r1) = got
    for k, c in enumerate(m):
        wide = tol * (max(1.0, cond[k]) if itype == 3 else 1.0)
        assert o1.out[k, 0] == o0.out[k, 0]                                # the same A and B
        assert r1[k][0][2] > 1e-9 and o1.out[k, 2] > 1e-9                 # the wrong eigenvalue shows
        if c >= 2:
            assert r1[k][0][3] > 1e-4 and o1.out[k, 3] > 1e-4             # ... and the two columns
        for s, bound in ((1, tol), (2, tol), (3, wide)):
            assert abs((o1.out[k, s] - o0.out[k, s]) - (r1[k][0][s] - r0[k][0][s])) <= 2 * bound, (c, k, s)
    _assert_shares(shares, (n, itype, form))


# ------------------------------------------------------------------------------------------ 2: a different m per problem
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_a_different_m_per_problem(hip, n, itype, form):
    lib = hip.load_library()
    m = [0, 1, 16, 17, 64, 65, n]
    idx = np.arange(len(m)) % COUNT
    A, B, ws, Zs, ref, cond = _pick(n, itype, idx, m)
    o = _window(lib, form, itype, A, B, m, ws, Zs, n)
    _clean(o, m, n)
    shares = []
    for b, c in enumerate(m):
        alone = _window(lib, form, itype, A[b:b + 1], B[b:b + 1], [c], ws[b:b + 1], Zs[b:b + 1], c)
        _clean(alone, [c], n)
        assert _same(alone.out[0], o.out[b]) and _same(alone.ipr[0], o.ipr[b]), (b, c)
        if c:
            shares.append(cs.shares(itype, o.out[b], o.ipr[b, :c], ref[b][0], ref[b][1], n, cond[b]))
    _assert_shares(shares, ("m per problem", n, itype, form))


# ------------------------------------------------------------------------------ 3: type 1 and what type 2 shares with it
@pytest.mark.parametrize("form", ("device", "host"))
@pytest.mark.parametrize("n", (65, 129, 256))
def test_type_1_is_the_window_check_and_type_2_shares_its_metric(hip, n, form):
    """The windows of the type-2 table (any Z serves): itype = 1 through this entry and problem = 1 through
    ek_hip_check_window_xbatched* give the same bits in every slot; type 2's slot 3 and IPRs are those bits."""
    lib = hip.load_library()
    cols = [max(n // 8, 1), min(65, n), min(17, n), n, 1, min(33, n)]
    idx = np.arange(len(cols)) % COUNT
    A, B, ws, Zs, _, _ = _pick(n, 2, idx, cols)
    plain = _window(lib, form, 1, A, B, cols, ws, Zs, n, pad=2, entry=PLAIN)
    one = _window(lib, form, 1, A, B, cols, ws, Zs, n, pad=2)
    two = _window(lib, form, 2, A, B, cols, ws, Zs, n, pad=2)
    for o in (plain, one, two):
        _clean(o, cols, n)
    assert _same(one.out, plain.out) and _same(one.ipr, plain.ipr)
    assert _same(two.out[:, 3], plain.out[:, 3]) and _same(two.ipr, plain.ipr)
    assert not np.array_equal(two.out[:, 0], plain.out[:, 0])            # ||A|| ||B|| against ||A||


# ------------------------------------------------------------------------------ 4: the same bits wherever a problem sits
_plain = {}


def _reference_bits(lib, n, itype):
    """Four problems with windows of n / 8, 65 (clipped), 17 and n columns through the device form in the compact layout
    with zcap = n, once: what every other position, batch, layout, form and chunk must reproduce bit for bit."""
    key = (n, itype)
    if key not in _plain:
        cols = [max(n // 8, 1), min(65, n), min(17, n), n]
        A, B, ws, Zs, ref, cond = _pick(n, itype, np.arange(COUNT), cols)
        o = _window(lib, "device", itype, A, B, cols, ws, Zs, n)
        _clean(o, cols, n)
        _assert_shares([cs.shares(itype, o.out[b], o.ipr[b, :cols[b]], ref[b][0], ref[b][1], n, cond[b])
                        for b in range(COUNT)], ("the reference bits", n, itype))
        o.out.setflags(write=False)
        o.ipr.setflags(write=False)
        _plain[key] = (cols, o.out, o.ipr)
    return _plain[key]


def _against_reference(o, idx, cols, ref_out, ref_ipr):
    for k, b in enumerate(idx):
        assert _same(o.out[k], ref_out[b]) and _same(o.ipr[k, :cols[b]], ref_ipr[b, :cols[b]]), (k, b)


@pytest.mark.parametrize("itype", (2, 3))
@pytest.mark.parametrize("n", (65, 129, 256))
def test_same_bits_wherever_a_problem_sits(hip, n, itype):
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, itype)

    def run(form, idx, zcap, **kw):
        m = [cols[b] for b in idx]
        A, B, ws, Zs, _, _ = _pick(n, itype, idx, m)
        o = _window(lib, form, itype, A, B, m, ws, Zs, zcap, **kw)
        _clean(o, m, n)
        _against_reference(o, idx, cols, ref_out, ref_ipr)

    run("device", [3, 2, 1, 0], n)                                  # another position
    run("device", [1, 1, 0, 3, 2, 0, 3, 1], n)                      # another batch
    run("device", [0], cols[0])                                     # alone, zcap = m
    run("device", [0, 1, 2, 3], n + 5, pad=3)                       # another zcap, ldz and stride
    run("host", [0, 1, 2, 3], n)                                    # the host form
    run("host", [2, 0, 3], n + 1, pad=2)
    try:                                                            # across a chunk seam: 7 problems, 3 a launch
        assert hip.check_xbatched_chunk(3) == 1024
        run("device", [0, 1, 2, 3, 0, 1, 2], n)
        run("host", [3, 3, 2, 1, 0, 0, 1], n)
    finally:
        hip.check_xbatched_chunk(0)


# ------------------------------------------------------------------------- 5: what is never read, what is never written
@ways
@pytest.mark.parametrize("n", (33, 129, 256))
def test_what_is_never_read(hip, n, itype, form):
    """NaN in the columns of Z from m[b] on, in w from m[b] on, in the strictly upper triangles of A and B, in the rows
    n .. ld-1 and in the gaps between problems: the bits of the clean compact run.  A, B, w and Z come back byte for byte
    (o.untouched), the ipr rows keep their sentinel from m[b] on and the words behind out and ipr theirs (_clean)."""
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, itype)
    idx = [0, 1, 2, 3]
    A, B, ws, Zs, _, _ = _pick(n, itype, idx, cols)
    o = _window(lib, form, itype, _nan_upper(A), _nan_upper(B), cols, ws, Zs, n, pad=3, fill=np.nan)
    _clean(o, cols, n)
    _against_reference(o, idx, cols, ref_out, ref_ipr)
    o = _window(lib, form, itype, A, B, cols, ws, Zs, n, ipr=False, fill=np.nan)            # ipr = NULL
    assert o.rc == 0 and o.untouched and np.all(o.tails[0] == SENTINEL)
    assert _same(o.out, ref_out) and np.all(o.ipr == SENTINEL)


# ------------------------------------------------------------------------------------------------------- 6: own slots
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_own_slots(hip, n, itype, form):
    """One batch: a skipped problem (info = 3, its m, w and Z garbage), a -20 problem whose m exceeds zcap, an empty window,
    a NaN in one problem's Z.  The first three get four NaN and keep their ipr row, the fourth reports NaN in its own
    outputs, the neighbours keep the bits of a clean run."""
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, itype)
    zcap = cols[1]                                  # 65: room for the windows of problems 0, 1, 2
    idx = [0, 1, 2, 0, 1, 2]
    live = [cols[0], 0, 0, 0, cols[1], cols[2]]
    m = [cols[0], n + 9, zcap + 5, 0, cols[1], cols[2]]
    info = [0, 3, -20, 0, 0, 0]
    A, B, ws, Zs, _, _ = _pick(n, itype, idx, live)
    Zs[4] = Zs[4].copy()
    Zs[4][n // 2, cols[1] // 3] = np.nan
    o = _window(lib, form, itype, A, B, m, ws, Zs, zcap, info=info, fill=np.nan)
    _clean(o, live, n, info)
    for b in (1, 2, 3):
        assert np.all(np.isnan(o.out[b])) and np.all(o.ipr[b] == SENTINEL)
    assert o.out[4, 0] == ref_out[1, 0] and np.all(np.isnan(o.out[4, 1:])) and np.isnan(o.ipr[4, cols[1] // 3])
    others = np.arange(cols[1]) != cols[1] // 3     # the other columns' IPRs are their own: G_jj is a column's affair
    assert _same(o.ipr[4, :cols[1]][others], ref_ipr[1, :cols[1]][others])
    for k, b in ((0, 0), (5, 2)):
        assert _same(o.out[k], ref_out[b]) and _same(o.ipr[k, :cols[b]], ref_ipr[b, :cols[b]])


@pytest.mark.parametrize("form", ("device", "host"))
@pytest.mark.parametrize("where", ("first", "last"))
@pytest.mark.parametrize("n", (129, 256))
def test_a_b_that_is_not_positive_definite(hip, n, where, form):
    """B[k, k] negated in problem 1 of three, k = 0 or n - 1.  Type 3: NaN in slot 3 and in the m[b] IPRs, the residual
    slots those of the mirror, 0 returned, the neighbours the bits of a clean run.  Type 2 factors nothing: numbers, those
    of the mirror."""
    lib = hip.load_library()
    k = 0 if where == "first" else n - 1
    for itype in (3, 2):
        cols, ref_out, ref_ipr = _reference_bits(lib, n, itype)
        idx = [0, 1, 2]
        m = [cols[b] for b in idx]
        A, B, ws, Zs, _, cond = _pick(n, itype, idx, m)
        B = B.copy()
        B[1, k, k] = -B[1, k, k]
        o = _window(lib, form, itype, A, B, m, ws, Zs, n)
        _clean(o, m, n)
        for b in (0, 2):
            assert _same(o.out[b], ref_out[b]) and _same(o.ipr[b, :m[b]], ref_ipr[b, :m[b]])
        m_out, m_ipr = cs.mirror(itype, A[1], B[1], ws[1], Zs[1])
        assert np.all(np.isfinite(o.out[1, :3]))
        if itype == 3:
            assert np.isnan(m_out[3]) and np.all(np.isnan(m_ipr))         # the mirror's own factor fails too
            assert np.isnan(o.out[1, 3]) and np.all(np.isnan(o.ipr[1, :m[1]]))
        else:
            assert np.all(np.isfinite(m_out)) and np.all(np.isfinite(m_ipr))
            assert np.isfinite(o.out[1, 3]) and np.all(np.isfinite(o.ipr[1, :m[1]]))
        _assert_shares([cs.shares(itype, o.out[1], o.ipr[1, :m[1]], m_out, m_ipr, n, cond[1])],
                       ("B[%d, %d] negated" % (k, k), n, itype, form))


# ------------------------------------------------------------------------------------------------------------ 7: m = n
@pytest.mark.parametrize("itype", (2, 3))
@pytest.mark.parametrize("n", (64, 128, 129, 256))
def test_all_n_columns_against_the_full_check(hip, n, itype):
    lib = hip.load_library()
    m = [n] * COUNT
    A, B, ws, Zs, _, cond = _pick(n, itype, np.arange(COUNT), m)
    o = _window(lib, "device", itype, A, B, m, ws, Zs, n)
    _clean(o, m, n)
    out, q = np.zeros(COUNT * 4), np.zeros(COUNT * n)
    with _Dev(lib) as dev:
        dA = dev.up(_pack(A, n, n * n, 0.0))
        dB = dev.up(_pack(B, n, n * n, 0.0))
        dw = dev.up(np.ascontiguousarray(np.stack(ws)))
        dZ = dev.up(_pack(np.stack(Zs), n, n * n, 0.0))
        assert lib.ek_hip_check_sygv_xbatched_device(itype, n, COUNT, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n, None,
                                                     out.ctypes.data_as(_dp), q.ctypes.data_as(_dp), None) == 0
    out, q = out.reshape(COUNT, 4), q.reshape(COUNT, n)
    shares = np.array([cs.shares(itype, o.out[b], o.ipr[b], out[b], q[b], n, cond[b]) for b in range(COUNT)]) / 2.0
    _assert_shares(shares, ("m = n against the full check, shares of twice the bounds", n, itype))


# ------------------------------------------------------------------------------------------------ 8: behind the solver
@pytest.mark.parametrize("rng", ("I", "V"))
@pytest.mark.parametrize("itype", (2, 3))
@pytest.mark.parametrize("n", (33, 128, 129, 256))
def test_behind_the_window_solver(hip, n, itype, rng):
    """ek_hip_sygv_window_xbatched_device on four pencils per window of window_batched_cases.windows(n); its m, w, Z and
    info go to the check as they are, A and B from kept copies (the solver overwrites its own)."""
    lib = hip.load_library()
    case = cs.cases(n, itype)
    hA = _pack(case.A, n, n * n, 0.0)
    hB = _pack(case.B, n, n * n, 0.0)
    refs = [case.w[b] for b in range(COUNT)]
    lim = 256 * n * EPS
    worst_r = worst_o = 0.0
    shares = []
    with _Dev(lib) as dev:
        dA0, dA, dB0, dB = dev.up(hA), dev.up(hA), dev.up(hB), dev.up(hB)
        dw, dZ = dev.up(np.zeros(COUNT * n)), dev.up(np.zeros(COUNT * n * n))
        for name, il, iu in wc.windows(n):
            if rng == "I":
                vl, vu, zcap, want = -np.inf, np.inf, iu - il + 1, [iu - il + 1] * COUNT
            else:
                vl, vu, span = wc.value_bounds(refs, il, iu)
                zcap, want = n, [s[1] for s in span]
            m = np.full(COUNT, -1, dtype=np.int32)
            info = np.full(COUNT, -1, dtype=np.int32)
            sZ = n * max(zcap, 1)
            dev.put(dA, hA)
            dev.put(dB, hB)
            assert lib.ek_hip_sygv_window_xbatched_device(itype, 1, int(rng == "V"), n, COUNT, vl, vu, il, iu, dA, n, n * n,
                                                          dB, n, n * n, m.ctypes.data_as(_ip), dw, dZ, n, zcap, sZ,
                                                          info.ctypes.data_as(_ip), None) == 0
            assert not info.any() and list(m) == want, (name, info, m, want)
            m0, info0 = m.copy(), info.copy()
            hw, hZ = dev.down(dw, np.zeros(COUNT * n)), dev.down(dZ, np.zeros(COUNT * n * n))
            out, q = np.full(COUNT * 4, SENTINEL), np.full(COUNT * n, SENTINEL)
            assert lib.ek_hip_check_sygv_window_xbatched_device(itype, n, COUNT, dA0, n, n * n, dB0, n, n * n,
                                                                m.ctypes.data_as(_ip), dw, dZ, n, zcap, sZ,
                                                                info.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                                                                q.ctypes.data_as(_dp), None) == 0
            # m, w, Z, info unchanged
            assert np.array_equal(m, m0) and np.array_equal(info, info0)
            assert _same(dev.down(dw, hw), hw) and _same(dev.down(dZ, hZ), hZ)
            out, q = out.reshape(COUNT, 4), q.reshape(COUNT, n)
            live = m > 0                            # a 'V' window cut from the first spectrum may be empty in another
            assert live[0] and np.all(np.isnan(out[~live])) and np.all(q[~live] == SENTINEL)
            cond = case.cond[live]
            out = out[live]
            assert np.all(out[:, 2] <= lim), (name, out[:, 2].max(), lim)
            assert np.all(out[:, 1] <= out[:, 2])
            assert np.all(out[:, 3] <= lim), (name, out[:, 3].max(), lim)
            worst_r, worst_o = max(worst_r, out[:, 2].max() / lim), max(worst_o, out[:, 3].max() / lim)
            one, q1 = np.zeros(4), np.zeros(n)
            assert lib.ek_hip_check_sygvx_device(itype, n, int(m[0]), dA0, n, dB0, n, dw, dZ, n, one.ctypes.data_as(_dp),
                                                 q1.ctypes.data_as(_dp)) == 0
            shares.append(cs.shares(itype, out[0], q[0, :m[0]], one, q1[:m[0]], n, cond[0]))
            assert np.all(q[0, m[0]:] == SENTINEL)
    print("behind the solver %s: res_max %.4f, orthogonality %.4f of 256 n eps" % ((n, itype, rng), worst_r, worst_o))
    _assert_shares(shares, ("against ek_hip_check_sygvx_device", n, itype, rng))


# ------------------------------------------------------------------------------------------------------------ 9: cost
@pytest.mark.parametrize("itype", (2, 3))
@pytest.mark.parametrize("n", (128, 129, 256))
def test_cost(hip, n, itype):
    """256 pencils, the window of n / 8 pairs from index n / 4 + 1.  Device seconds, best of 3 after a warm-up, the kinds
    alternated in one process: (a) the window check against ek_hip_check_sygv_xbatched_device on all n columns of the same
    batch -- type 2's three products shrink eightfold, type 3's factor stays while its solve and products shrink --, (b)
    against the window solve that produced its input; (c) its wall time against a host loop over
    ek_hip_check_sygvx_device on the same 256 windows.  The ratio to the type-1 window check of the same words is printed."""
    lib = hip.load_library()
    batch, c = 256, n // 8
    il, iu = n // 4 + 1, n // 4 + c
    rng = np.random.default_rng(8900 + n)
    A16 = np.stack([cs.cw._sym(rng, n) for _ in range(16)])
    B16 = np.stack([cs.cw._spd(rng, n) for _ in range(16)])
    hA, hB = _pack(np.tile(A16, (batch // 16, 1, 1)), n, n * n, 0.0), _pack(np.tile(B16, (batch // 16, 1, 1)), n, n * n, 0.0)
    info, infoF = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    m = np.zeros(batch, dtype=np.int32)
    out, q = np.zeros(batch * 4), np.zeros(batch * n)
    out1, q1w = np.zeros(batch * 4), np.zeros(batch * n)
    outF, qF = np.zeros(batch * 4), np.zeros(batch * n)
    ip, mp = info.ctypes.data_as(_ip), m.ctypes.data_as(_ip)
    t_solve, t_win, t_full, t_one, w_win, w_loop = [], [], [], [], [], []
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * c))
        dwF, dZF = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        assert lib.ek_hip_sygv_xbatched_device(itype, 1, n, batch, dA, n, n * n, dB, n, n * n, dwF, dZF, n, n * n,
                                               infoF.ctypes.data_as(_ip), None) == 0
        assert not infoF.any()
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_sygv_window_xbatched_device(itype, 1, 0, n, batch, -np.inf, np.inf, il, iu, dA, n, n * n, dB,
                                                          n, n * n, mp, dw, dZ, n, c, n * c, ip, ctypes.byref(sec)) == 0
            assert not info.any() and np.all(m == c)
            t_solve.append(sec.value)
            sec = ctypes.c_double(-1.0)
            t0 = time.perf_counter()
            assert lib.ek_hip_check_sygv_window_xbatched_device(itype, n, batch, dA0, n, n * n, dB0, n, n * n, mp, dw, dZ,
                                                                n, c, n * c, ip, out.ctypes.data_as(_dp),
                                                                q.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
            w_win.append(time.perf_counter() - t0)
            t_win.append(sec.value)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_check_sygv_xbatched_device(itype, n, batch, dA0, n, n * n, dB0, n, n * n, dwF, dZF, n, n * n,
                                                         infoF.ctypes.data_as(_ip), outF.ctypes.data_as(_dp),
                                                         qF.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
            t_full.append(sec.value)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_check_window_xbatched_device(1, n, batch, dA0, n, n * n, dB0, n, n * n, mp, dw, dZ, n, c,
                                                           n * c, ip, out1.ctypes.data_as(_dp), q1w.ctypes.data_as(_dp),
                                                           ctypes.byref(sec)) == 0
            t_one.append(sec.value)
        one, q1 = np.zeros(4), np.zeros(n)
        loop = np.zeros((batch, 4))

        def at(p, words):
            return ctypes.c_void_p(p.value + 8 * words)

        for it in range(3):
            t0 = time.perf_counter()
            for b in range(batch):
                assert lib.ek_hip_check_sygvx_device(itype, n, c, at(dA0, b * n * n), n, at(dB0, b * n * n), n,
                                                     at(dw, b * n), at(dZ, b * n * c), n, one.ctypes.data_as(_dp),
                                                     q1.ctypes.data_as(_dp)) == 0
                loop[b] = one
            w_loop.append(time.perf_counter() - t0)
    o = out.reshape(batch, 4)
    lim = 256 * n * EPS
    assert np.all(o[:, 2] <= lim) and np.all(o[:, 3] <= lim)
    tol = cs.tol(n)
    wide = tol * (10.0 if itype == 3 else 1.0)      # cond_2(B) = 10 by construction
    assert np.all(np.abs(o[:, 1:3] - loop[:, 1:3]) <= tol) and np.all(np.abs(o[:, 3] - loop[:, 3]) <= wide)
    assert np.all(np.abs(o[:, 0] - loop[:, 0]) <= tol * loop[:, 0])
    ts, tw, tf, t1 = min(t_solve[1:]), min(t_win[1:]), min(t_full[1:]), min(t_one[1:])
    ww, wl = min(w_win[1:]), min(w_loop)
    print("cost n=%d itype=%d batch=%d c=%d: window check %.3f ms device (%.3f ms wall), full check %.3f ms, window solve "
          "%.3f ms, type-1 window check %.3f ms, host loop %.1f ms; window / full %.3f, window / solve %.3f, loop / window "
          "%.1f, window / type-1 window %.3f"
          % (n, itype, batch, c, tw * 1e3, ww * 1e3, tf * 1e3, ts * 1e3, t1 * 1e3, wl * 1e3, tw / tf, tw / ts, wl / ww,
             tw / t1))
    assert 0.0 < tw < tf, (tw, tf)                  # (a) checking an eighth costs less than checking everything
    assert tw <= ts, (tw, ts)                       # (b) no dearer than the solve that produced its input
    assert ww < wl, (ww, wl)                        # (c) faster than the host loop
