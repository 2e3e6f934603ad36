"""GPU suite of the window check (ek_hip_check_window_xbatched*): a_norm, res_ave, res_max, orthogonality and
the inverse participation ratios of the m[b] columns that problem b of a batch holds in its n x zcap array, orders 1 .. 256.

  1 the mirror      both problems, device and host form, every order x column count of tests/check_window_cases.py, clean
                    and with planted errors, within 4 max(n, 8) eps of the host mirror on Z[:, :c], w[:c]; what a plant
                    moves, it moves by what the mirror says within twice that
  2 m per problem   m = 0, 1, 16, 17, 64, 65, n in one batch with zcap = n: the bits of each problem alone with zcap = m
  3 bits            another position, another batch, another zcap / ldz / stride, the host form, a chunk seam
  4 never read      NaN in the columns of Z and in w from m[b] on, in the strictly upper triangles, the rows n .. ld-1 and
                    the gaps: the bits of a clean run; A, B, w, Z come back byte for byte
  5 own slots       a skipped problem, a -20 problem with m > zcap, an empty window and a NaN in one problem's Z in one batch
  6 m = n           within twice the tolerance of ek_hip_check_xbatched_device on the same full Z
  7 the solver      ek_hip_eigenpairs_window_xbatched_device's m, w, Z, info handed over unchanged, 'I' and 'V': res_max
                    <= 64 n eps, orthogonality <= 256 n eps, the first problem within the tolerance of
                    ek_hip_check_sygvx_device(1, n, m[0])
  8 cost            256 generalized problems, a window of n / 8 columns: cheaper than the full check of the same batch,
                    no dearer than the window solve, faster than the host loop over ek_hip_check_sygvx_device

Each test prints the largest share of the tolerance it used (pytest -s shows it).  Largest shares on one MI355X: against
the mirror 0.072 (an IPR at n = 17; a_norm 0.025, res_ave and res_max 0.013, orthogonality 0.008), m = n against the full
check 0.011 of twice the tolerance, against ek_hip_check_sygvx_device 0.026; behind the solver res_max 0.0006 of 64 n eps and
orthogonality 0.0027 of 256 n eps; cost: window / full 0.164, 0.205, 0.182 at n = 128, 129, 256, window / solve 0.023, 0.022,
0.014, host loop / window 405, 315, 166."""
import ctypes
import time

import numpy as np
import pytest

import check_window_cases as cw
import window_batched_cases as wc

pytestmark = pytest.mark.gpu
EPS = cw.EPS
COUNT = cw.COUNT
SENTINEL = -7.25e77
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
WAYS = [(0, "device"), (0, "host"), (1, "device"), (1, "host")]
ways = pytest.mark.parametrize("problem,form", WAYS)


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _nan_upper(M):
    X = np.array(M, dtype=np.float64)
    iu = np.triu_indices(X.shape[-1], 1)
    X[..., iu[0], iu[1]] = np.nan
    return X


def _pack(M, ld, stride, fill):
    """(batch, n, n) matrices as column-major images with leading dimension ld, `stride` doubles apart."""
    batch, n = M.shape[0], M.shape[1]
    flat = np.full(max(batch * stride, 1), fill)
    it = flat.itemsize
    view = np.lib.stride_tricks.as_strided(flat, shape=(batch, n, n), strides=(stride * it, ld * it, it))
    view[...] = M.transpose(0, 2, 1)
    return flat


def _window(lib, form, problem, A, B, m, ws, Zs, zcap, info=None, ipr=True, pad=0, fill=SENTINEL):
    """ek_hip_check_window_xbatched[_device].  Problem b: the first m[b] values of ws[b] and columns of Zs[b] (n x at least
    m[b]; nothing of them when the problem is skipped or m[b] exceeds what there is) in a row of w and an n x zcap array;
    every other word of w and Z, the rows n .. ld-1 and the gaps hold `fill`.  pad = 0: the compact layout; pad > 0:
    leading dimensions n + pad .. and strides beyond.  o.untouched: A, B, w, Z after the call equal those before."""
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
    h = [_pack(A, lda, sA, fill), _pack(B, ldb, sB, fill) if problem else None, hw, hZ]
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
            d = [dev.up(x) if x is not None else None for x in h]
            o.rc = lib.ek_hip_check_window_xbatched_device(problem, n, batch, d[0], lda, sA, d[1], ldb, sB, mp, d[2], d[3],
                                                           ldz, zcap, sZ, *tail)
            o.untouched = all(x is None or _same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [None if x is None else x.copy() for x in h]
        P = [None if x is None else x.ctypes.data_as(_dp) for x in g]
        o.rc = lib.ek_hip_check_window_xbatched(problem, n, batch, P[0], lda, sA, P[1], ldb, sB, mp, P[2], P[3], ldz, zcap,
                                                sZ, *tail)
        o.untouched = all(x is None or _same(y, x) for y, x in zip(g, h))
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
    print("shares of the tolerance %s: " % (what,) + ", ".join("%s %.3f" % kv for kv in zip(cw.NAMES, shares)))
    assert np.all(shares <= 1.0), (what, shares)


def _pick(n, problem, idx, cols, plant=True):
    """Problem idx[k] of the table with a window of cols[k] columns, per entry: A, B, ws, Zs, mirrors."""
    case = cw.cases(n, problem)
    idx = np.asarray(idx)
    ws, Zs, ref = [], [], []
    for b, c in zip(idx, cols):
        if c > 0:
            w_all, Z_all = cw.windows(n, problem, c, plant)
            ws.append(w_all[b])
            Zs.append(Z_all[b])
            ref.append(cw.mirrors(n, problem, c, plant)[b])
        else:
            ws.append(np.zeros(0))
            Zs.append(np.zeros((n, 0)))
            ref.append(None)
    return case.A[idx], (case.B[idx] if problem else None), ws, Zs, ref


# --------------------------------------------------------------------------------------------- 1: against the host mirror
@ways
@pytest.mark.parametrize("n", cw.ORDERS)
def test_matches_the_host_mirror(hip, n, problem, form):
    """Every column count of the order, four problems a call, padded layout with one spare column, the gaps and the spare
    column holding a sentinel.  Clean and planted windows; the planted one moves res_ave, res_max, orthogonality and the
    IPR of the last column by what the mirror's move by, within twice the tolerance."""
    lib = hip.load_library()
    tol = cw.tol(n)
    idx = np.arange(COUNT)
    shares = []
    for c in cw.columns(n):
        m = [c] * COUNT
        got = []
        for plant in (False, True):
            A, B, ws, Zs, ref = _pick(n, problem, idx, m, plant)
            o = _window(lib, form, problem, A, B, m, ws, Zs, c + 1, pad=3)
            _clean(o, m, n)
            shares += [cw.shares(o.out[b], o.ipr[b, :c], ref[b][0], ref[b][1], n) for b in range(COUNT)]
            got.append((o, ref))
        (o0, r0), (o1, r1) = got
        for b in range(COUNT):
            assert o1.out[b, 0] == o0.out[b, 0]                            # the same A
            assert r1[b][0][2] > 1e-8 and o1.out[b, 2] > 1e-8             # the wrong eigenvalue shows
            if c >= 2:
                assert r1[b][0][3] > 1e-4 and o1.out[b, 3] > 1e-4         # ... and the two columns
            for k in (1, 2, 3):
                assert abs((o1.out[b, k] - o0.out[b, k]) - (r1[b][0][k] - r0[b][0][k])) <= 2 * tol, (c, b, k)
            j = c - 1
            assert abs((o1.ipr[b, j] - o0.ipr[b, j]) - (r1[b][1][j] - r0[b][1][j])) <= 2 * tol * r0[b][1][j], (c, b)
    _assert_shares(shares, (n, problem, form))


# ------------------------------------------------------------------------------------------ 2: a different m per problem
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_a_different_m_per_problem(hip, n, problem, form):
    lib = hip.load_library()
    m = [0, 1, 16, 17, 64, 65, n]
    idx = np.arange(len(m)) % COUNT
    A, B, ws, Zs, ref = _pick(n, problem, idx, m)
    o = _window(lib, form, problem, A, B, m, ws, Zs, n)
    _clean(o, m, n)
    shares = []
    for b, c in enumerate(m):
        alone = _window(lib, form, problem, A[b:b + 1], B[b:b + 1] if problem else None, [c], ws[b:b + 1], Zs[b:b + 1], c)
        _clean(alone, [c], n)
        assert _same(alone.out[0], o.out[b]) and _same(alone.ipr[0], o.ipr[b]), (b, c)
        if c:
            shares.append(cw.shares(o.out[b], o.ipr[b, :c], ref[b][0], ref[b][1], n))
    _assert_shares(shares, ("m per problem", n, problem, form))


# ------------------------------------------------------------------------------ 3: the same bits wherever a problem sits
_plain = {}


def _reference_bits(lib, n, problem):
    """Four problems with windows of n / 8, 65 (clipped), 17 and n columns through the device form in the compact layout
    with zcap = n, once: what every other position, batch, layout, form and chunk must reproduce bit for bit."""
    key = (n, problem)
    if key not in _plain:
        cols = [max(n // 8, 1), min(65, n), min(17, n), n]
        A, B, ws, Zs, _ = _pick(n, problem, np.arange(COUNT), cols)
        o = _window(lib, "device", problem, A, B, cols, ws, Zs, n)
        _clean(o, cols, n)
        o.out.setflags(write=False)
        o.ipr.setflags(write=False)
        _plain[key] = (cols, o.out, o.ipr)
    return _plain[key]


def _against_reference(o, idx, cols, ref_out, ref_ipr):
    for k, b in enumerate(idx):
        assert _same(o.out[k], ref_out[b]) and _same(o.ipr[k, :cols[b]], ref_ipr[b, :cols[b]]), (k, b)


@pytest.mark.parametrize("problem", (0, 1))
@pytest.mark.parametrize("n", (65, 129, 256))
def test_same_bits_wherever_a_problem_sits(hip, n, problem):
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, problem)

    def run(form, idx, zcap, **kw):
        A, B, ws, Zs, _ = _pick(n, problem, idx, [cols[b] for b in idx])
        m = [cols[b] for b in idx]
        o = _window(lib, form, problem, A, B, m, ws, Zs, zcap, **kw)
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


# ------------------------------------------------------------------------- 4: what is never read, what is never written
@ways
@pytest.mark.parametrize("n", (33, 129, 256))
def test_what_is_never_read(hip, n, problem, form):
    """NaN in the columns of Z from m[b] on, in w from m[b] on, in the strictly upper triangles of A and B, in the rows
    n .. ld-1 and in the gaps between problems: the bits of the clean compact run.  A, B, w and Z come back byte for byte
    (o.untouched), the ipr rows keep their sentinel from m[b] on and the words behind out and ipr theirs (_clean)."""
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, problem)
    idx = [0, 1, 2, 3]
    A, B, ws, Zs, _ = _pick(n, problem, idx, cols)
    o = _window(lib, form, problem, _nan_upper(A), _nan_upper(B) if problem else None, cols, ws, Zs, n, pad=3, fill=np.nan)
    _clean(o, cols, n)
    _against_reference(o, idx, cols, ref_out, ref_ipr)
    o = _window(lib, form, problem, A, B, cols, ws, Zs, n, ipr=False, fill=np.nan)          # ipr = NULL
    assert o.rc == 0 and o.untouched and np.all(o.tails[0] == SENTINEL)
    assert _same(o.out, ref_out) and np.all(o.ipr == SENTINEL)


# ------------------------------------------------------------------------------------------------------- 5: own slots
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_own_slots(hip, n, problem, form):
    """One batch: a skipped problem (info = 3, its m, w and Z garbage), a -20 problem whose m exceeds zcap, an empty window,
    a NaN in one problem's Z.  The first three get four NaN and keep their ipr row, the fourth reports NaN in its own
    outputs, the neighbours keep the bits of a clean run."""
    lib = hip.load_library()
    cols, ref_out, ref_ipr = _reference_bits(lib, n, problem)
    zcap = cols[1]                                  # 65: room for the windows of problems 0, 1, 2
    idx = [0, 1, 2, 0, 1, 2]
    m = [cols[0], n + 9, zcap + 5, 0, cols[1], cols[2]]
    info = [0, 3, -20, 0, 0, 0]
    A, B, ws, Zs, _ = _pick(n, problem, idx, [cols[0], 0, 0, 0, cols[1], cols[2]])
    Zs[4] = Zs[4].copy()
    Zs[4][n // 2, cols[1] // 3] = np.nan
    o = _window(lib, form, problem, A, B, m, ws, Zs, zcap, info=info, fill=np.nan)
    _clean(o, [cols[0], 0, 0, 0, cols[1], cols[2]], n)
    for b in (1, 2, 3):
        assert np.all(np.isnan(o.out[b])) and np.all(o.ipr[b] == SENTINEL)
    assert o.out[4, 0] == ref_out[1, 0] and np.all(np.isnan(o.out[4, 1:])) and np.isnan(o.ipr[4, cols[1] // 3])
    others = np.arange(cols[1]) != cols[1] // 3
    assert _same(o.ipr[4, :cols[1]][others], ref_ipr[1, :cols[1]][others])     # the other columns' IPRs are their own
    for k, b in ((0, 0), (5, 2)):
        assert _same(o.out[k], ref_out[b]) and _same(o.ipr[k, :cols[b]], ref_ipr[b, :cols[b]])


# ------------------------------------------------------------------------------------------------------------ 6: m = n
@pytest.mark.parametrize("problem", (0, 1))
@pytest.mark.parametrize("n", (64, 128, 129, 256))
def test_all_n_columns_against_the_full_check(hip, n, problem):
    lib = hip.load_library()
    m = [n] * COUNT
    A, B, ws, Zs, _ = _pick(n, problem, np.arange(COUNT), m)
    o = _window(lib, "device", problem, A, B, m, ws, Zs, n)
    _clean(o, m, n)
    out, q = np.zeros(COUNT * 4), np.zeros(COUNT * n)
    with _Dev(lib) as dev:
        dA = dev.up(_pack(A, n, n * n, 0.0))
        dB = dev.up(_pack(B, n, n * n, 0.0)) if problem else None
        dw = dev.up(np.ascontiguousarray(np.stack(ws)))
        dZ = dev.up(_pack(np.stack(Zs), n, n * n, 0.0))
        assert lib.ek_hip_check_xbatched_device(problem, n, COUNT, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n, None,
                                                out.ctypes.data_as(_dp), q.ctypes.data_as(_dp), None) == 0
    out, q = out.reshape(COUNT, 4), q.reshape(COUNT, n)
    shares = np.array([cw.shares(o.out[b], o.ipr[b], out[b], q[b], n) for b in range(COUNT)]) / 2.0      # 2 tol
    _assert_shares(shares, ("m = n against the full check, shares of 2 tol", n, problem))


# ------------------------------------------------------------------------------------------------ 7: behind the solver
@pytest.mark.parametrize("rng", ("I", "V"))
@pytest.mark.parametrize("problem", (0, 1))
@pytest.mark.parametrize("n", (33, 128, 129, 256))
def test_behind_the_window_solver(hip, n, problem, rng):
    """ek_hip_eigenpairs_window_xbatched_device on four pairs per window of window_batched_cases.windows(n); its m, w, Z
    and info go to the check as they are, A and B from kept copies (the solver overwrites its own)."""
    lib = hip.load_library()
    case = cw.cases(n, problem)
    hA = _pack(case.A, n, n * n, 0.0)
    hB = _pack(case.B, n, n * n, 0.0) if problem else None
    eye = np.eye(n).ravel()
    refs = [case.w[b] for b in range(COUNT)]
    lim_r, lim_o = 64 * n * EPS, 256 * n * EPS
    worst_r = worst_o = 0.0
    shares = []
    with _Dev(lib) as dev:
        dA0, dA = dev.up(hA), dev.up(hA)
        dB0, dB = (dev.up(hB), dev.up(hB)) if problem else (None, None)
        dI = dev.up(eye)
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
            if problem:
                dev.put(dB, hB)
            assert lib.ek_hip_eigenpairs_window_xbatched_device(problem, 1, int(rng == "V"), n, COUNT, vl, vu, il, iu, dA,
                                                                n, n * n, dB, n, n * n, m.ctypes.data_as(_ip), dw, dZ, n,
                                                                zcap, sZ, info.ctypes.data_as(_ip), None) == 0
            assert not info.any() and list(m) == want, (name, info, m, want)
            out, q = np.full(COUNT * 4, SENTINEL), np.full(COUNT * n, SENTINEL)
            assert lib.ek_hip_check_window_xbatched_device(problem, n, COUNT, dA0, n, n * n, dB0, n, n * n,
                                                           m.ctypes.data_as(_ip), dw, dZ, n, zcap, sZ,
                                                           info.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                                                           q.ctypes.data_as(_dp), None) == 0
            out, q = out.reshape(COUNT, 4), q.reshape(COUNT, n)
            live = m > 0                            # a 'V' window cut from the first spectrum may be empty in another
            assert live[0] and np.all(np.isnan(out[~live])) and np.all(q[~live] == SENTINEL)
            out = out[live]
            assert np.all(out[:, 2] <= lim_r), (name, out[:, 2].max(), lim_r)
            assert np.all(out[:, 1] <= out[:, 2])
            assert np.all(out[:, 3] <= lim_o), (name, out[:, 3].max(), lim_o)
            worst_r, worst_o = max(worst_r, out[:, 2].max() / lim_r), max(worst_o, out[:, 3].max() / lim_o)
            one, q1 = np.zeros(4), np.zeros(n)
            assert lib.ek_hip_check_sygvx_device(1, n, int(m[0]), dA0, n, dB0 if problem else dI, n, dw, dZ, n,
                                                 one.ctypes.data_as(_dp), q1.ctypes.data_as(_dp)) == 0
            shares.append(cw.shares(out[0], q[0, :m[0]], one, q1[:m[0]], n))
            assert np.all(q[0, m[0]:] == SENTINEL)
    print("behind the solver %s: res_max %.4f of 64 n eps, orthogonality %.4f of 256 n eps"
          % ((n, problem, rng), worst_r, worst_o))
    _assert_shares(shares, ("against ek_hip_check_sygvx_device", n, problem, rng))


# ------------------------------------------------------------------------------------------------------------ 8: cost
@pytest.mark.parametrize("n", (128, 129, 256))
def test_cost(hip, n):
    """256 generalized problems, the window of n / 8 pairs from index n / 4 + 1.  Device seconds, best of 3 after a warm-up,
    the kinds alternated in one process: (a) the window check against ek_hip_check_xbatched_device on all n columns of the
    same batch, (b) against the window solve that produced its input; (c) its wall time against a host loop over
    ek_hip_check_sygvx_device on the same 256 windows."""
    lib = hip.load_library()
    batch, c = 256, n // 8
    il, iu = n // 4 + 1, n // 4 + c
    rng = np.random.default_rng(8800 + n)
    A16 = np.stack([cw._sym(rng, n) for _ in range(16)])
    B16 = np.stack([cw._spd(rng, n) for _ in range(16)])
    hA, hB = _pack(np.tile(A16, (batch // 16, 1, 1)), n, n * n, 0.0), _pack(np.tile(B16, (batch // 16, 1, 1)), n, n * n, 0.0)
    info, infoF = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    m = np.zeros(batch, dtype=np.int32)
    out, q = np.zeros(batch * 4), np.zeros(batch * n)
    outF, qF = np.zeros(batch * 4), np.zeros(batch * n)
    ip, mp = info.ctypes.data_as(_ip), m.ctypes.data_as(_ip)
    t_solve, t_win, t_full, w_win, w_loop = [], [], [], [], []
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * c))
        dwF, dZF = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        assert lib.ek_hip_eigenpairs_xbatched_device(1, 1, n, batch, dA, n, n * n, dB, n, n * n, dwF, dZF, n, n * n,
                                                     infoF.ctypes.data_as(_ip), None) == 0
        assert not infoF.any()
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_eigenpairs_window_xbatched_device(1, 1, 0, n, batch, -np.inf, np.inf, il, iu, dA, n, n * n, dB,
                                                                n, n * n, mp, dw, dZ, n, c, n * c, ip,
                                                                ctypes.byref(sec)) == 0
            assert not info.any() and np.all(m == c)
            t_solve.append(sec.value)
            sec = ctypes.c_double(-1.0)
            t0 = time.perf_counter()
            assert lib.ek_hip_check_window_xbatched_device(1, n, batch, dA0, n, n * n, dB0, n, n * n, mp, dw, dZ, n, c,
                                                           n * c, ip, out.ctypes.data_as(_dp), q.ctypes.data_as(_dp),
                                                           ctypes.byref(sec)) == 0
            w_win.append(time.perf_counter() - t0)
            t_win.append(sec.value)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_check_xbatched_device(1, n, batch, dA0, n, n * n, dB0, n, n * n, dwF, dZF, n, n * n,
                                                    infoF.ctypes.data_as(_ip), outF.ctypes.data_as(_dp),
                                                    qF.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
            t_full.append(sec.value)
        one, q1 = np.zeros(4), np.zeros(n)
        loop = np.zeros((batch, 4))

        def at(p, words):
            return ctypes.c_void_p(p.value + 8 * words)

        for it in range(3):
            t0 = time.perf_counter()
            for b in range(batch):
                assert lib.ek_hip_check_sygvx_device(1, n, c, at(dA0, b * n * n), n, at(dB0, b * n * n), n, at(dw, b * n),
                                                     at(dZ, b * n * c), n, one.ctypes.data_as(_dp),
                                                     q1.ctypes.data_as(_dp)) == 0
                loop[b] = one
            w_loop.append(time.perf_counter() - t0)
    o = out.reshape(batch, 4)
    assert np.all(o[:, 2] <= 64 * n * EPS) and np.all(o[:, 3] <= 256 * n * EPS)
    tol = cw.tol(n)
    assert np.all(np.abs(o[:, 1:] - loop[:, 1:]) <= tol) and np.all(np.abs(o[:, 0] - loop[:, 0]) <= tol * loop[:, 0])
    ts, tw, tf = min(t_solve[1:]), min(t_win[1:]), min(t_full[1:])
    ww, wl = min(w_win[1:]), min(w_loop)
    print("cost n=%d batch=%d c=%d: window check %.3f ms device (%.3f ms wall), full check %.3f ms, window solve %.3f ms, "
          "host loop %.1f ms; window / full %.3f, window / solve %.3f, loop / window %.1f"
          % (n, batch, c, tw * 1e3, ww * 1e3, tf * 1e3, ts * 1e3, wl * 1e3, tw / tf, tw / ts, wl / ww))
    assert 0.0 < tw < tf, (tw, tf)                  # (a) checking an eighth costs less than checking everything
    assert tw <= ts, (tw, ts)                       # (b) no dearer than the solve that produced its input
    assert ww < wl, (ww, wl)                        # (c) faster than the host loop
