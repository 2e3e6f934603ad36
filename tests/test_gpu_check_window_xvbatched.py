"""GPU suite of the variable-order window checks (ek_hip_check_window_xvbatched*, ek_hip_check_sygv_window_xvbatched*,
DESIGN.md 37): the four words and the m[b] inverse participation ratios of problem b of a batch of DIFFERENT orders
0 .. 256, which holds m[b] pairs in an n[b] x zcap[b] array.  kind: 0 the standard problem, 1 A x = l B x, 2 A B x = l x,
3 B A x = l x (the entries' problem 0 / 1 and itype 2 / 3).

The batch of tests 1 .. 5: the orders of tests/check_window_cases.py and 0 in a seeded shuffle, two problems per order, m[b]
cycling through columns(n); zcap[b] = m[b] + 1, padded leading dimensions; NaN in everything that must not be read (Z and w
from m[b] on, the strictly upper triangles, the rows n .. ld-1, the gaps between the problems).

  1 bits of the uniform call   every problem's words and IPRs are those of the one-problem uniform window check: device and
                               host form, a second permutation with other leading dimensions and zcap
  2 identities                 itype = 1 is problem = 1; type 2's slot 3 and IPRs are type 1's
  3 host mirror                verifier.py on Z[:, :m], clean and planted, 4 max(n, 8) eps (cond_2(B) wider for type 3's metric)
  4 chunk seams                3 and 1 entries a launch, a skipped problem at the seam
  5 own slots                  skipped, -20 with m > zcap, empty, order 0, a NaN in a read column, a B that is not SPD
  6 m = n                      against the full variable checks to twice the bound
  7 many workgroups            608 problems of order 129, m = 17, 256 a launch
  8 behind the solvers         m, w, Z, zcap, info of the variable window solvers handed over unchanged, 'I' and 'V'
  9 one pool                   the other check entries before and after
 10 cost                       against 16 uniform calls, the window solve and the full check of the full solve

Largest shares on one MI355X are recorded in DESIGN.md 37."""
import ctypes
import time

import numpy as np
import pytest

import check_window_cases as cw
import check_sygv_window_cases as cs
import window_xvbatched_cases as xc
from test_gpu_check_window import _Dev, _same
from test_gpu_check_window import _window as _uniform_plain
from test_gpu_check_sygv_window import _window as _uniform_sygv

pytestmark = pytest.mark.gpu
EPS = cw.EPS
SENTINEL = -7.25e77
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
KINDS = pytest.mark.parametrize("kind", [0, 1, 2, 3])
LAYOUTS = ((1, 2, 3, 1, 5), (4, 0, 2, 3, 1))        # pads of lda, ldb, ldz; spare columns of Z; gap between problems
_alone_cache = {}


class _Problem:
    """One problem: order n, the pair, m pairs (w of m values, Z of n x m), the host mirror and cond_2(B)."""

    def __init__(self, kind, n, b, c, plant=False):
        self.key, self.kind, self.n, self.m = (kind, n, b, c, plant), kind, n, c
        self.ref, self.cond = None, 1.0
        if n == 0:
            self.A, self.B, self.w, self.Z = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0), np.zeros((0, 0))
            return
        if kind in (0, 1):
            case = cw.cases(n, kind)
            self.A, self.B = case.A[b], case.B[b] if kind else None
            if c:
                self.w, self.Z = (x[b] for x in cw.windows(n, kind, c, plant))
                self.ref = cw.mirrors(n, kind, c, plant)[b]
        else:
            case = cs.cases(n, kind)
            self.A, self.B, self.cond = case.A[b], case.B[b], float(case.cond[b])
            if c:
                self.w, self.Z = cs.window(n, kind, b, c, plant)
                self.ref = cs.mirrored(n, kind, b, c, plant)
        if not c:
            self.w, self.Z = np.zeros(0), np.zeros((n, 0))

    def shares(self, out, ipr, ref=None):
        ref = ref or self.ref
        if self.kind in (0, 1):
            return cw.shares(out, ipr, ref[0], ref[1], self.n)
        return cs.shares(self.kind, out, ipr, ref[0], ref[1], self.n, self.cond)


def _batch(kind, plant=False, shuffle=0):
    """Two problems of every order of the table and of order 0, shuffled; m cycles through the column counts."""
    probs, k = [], 0
    for n in cw.ORDERS + (0,):
        for b in range(2):
            cols = cw.columns(n) if n else (0,)
            probs.append(_Problem(kind, n, b, cols[k % len(cols)], plant))
            k += 1
    perm = np.random.default_rng(3700 + shuffle).permutation(len(probs))
    return [probs[i] for i in perm]


class _Out:
    pass


def _entry(kind, sygv1=False):
    if kind in (2, 3) or sygv1:
        return "ek_hip_check_sygv_window_xvbatched", kind
    return "ek_hip_check_window_xvbatched", kind


def _vcheck(lib, form, kind, probs, lay=0, info=None, m=None, rows=None, sygv1=False, full=False, alias=False):
    """The variable window entry of the kind on one arena per array kind.  m: the counts handed over (default: the
    problems'); problem b's w and Z hold its own m values and columns unless info[b] != 0.  rows: which IPR rows are wanted
    (default all).  full: the FULL variable check (ek_hip_check_[sygv_]xvbatched*) on the same arenas, zcap = n.  alias: every
    problem is problems[0] and reads the same memory."""
    batch = len(probs)
    slot = np.zeros(batch, dtype=np.int64) if alias else np.arange(batch)
    pa, pb, pz, spare, gap = LAYOUTS[lay]
    n = np.array([p.n for p in probs], dtype=np.int32)
    own = np.array([p.m for p in probs], dtype=np.int32)
    marr = own.copy() if m is None else np.asarray(m, dtype=np.int32).copy()
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    lda, ldb, ldz = (np.maximum(n + x, 1).astype(np.int32) for x in (pa, pb, pz))
    zcap = (n if full else own + spare).astype(np.int32)
    has_b = kind != 0

    def offsets(size):
        return np.concatenate([[0], np.cumsum(size.astype(np.int64) + gap)])[slot.tolist() + [int(slot[-1]) + 1]]

    offa, offb, offw = offsets(lda * n), offsets(ldb * n), offsets(n)
    offz = offsets(ldz * zcap)
    hA, hB = np.full(offa[-1] + 1, np.nan), np.full(offb[-1] + 1, np.nan)
    hw, hZ = np.full(offw[-1] + 1, np.nan), np.full(offz[-1] + 1, np.nan)
    for b, p in enumerate(probs[:1] if alias else probs):
        if p.n == 0:
            continue
        low = np.tril(np.ones((p.n, p.n), dtype=bool)).T
        hA[offa[b]:offa[b] + lda[b] * p.n].reshape(p.n, lda[b])[:, :p.n][low] = p.A.T[low]
        if has_b:
            hB[offb[b]:offb[b] + ldb[b] * p.n].reshape(p.n, ldb[b])[:, :p.n][low] = p.B.T[low]
        if (iarr is not None and iarr[b] != 0) or p.m == 0:
            continue
        hw[offw[b]:offw[b] + p.m] = p.w[:p.m]
        hZ[offz[b]:offz[b] + ldz[b] * zcap[b]].reshape(zcap[b], ldz[b])[:p.m, :p.n] = p.Z[:, :p.m].T
    h = [hA, hB if has_b else None, hw, hZ]
    offs = [offa, offb, offw, offz]
    out = np.full(batch * 4 + 2, SENTINEL)
    q = [np.full(p.n + 2, SENTINEL) for p in probs]
    wanted = [True] * batch if rows is None else rows
    qt = (ctypes.c_void_p * batch)(*[q[b].ctypes.data if wanted[b] else None for b in range(batch)])
    sec = ctypes.c_double(-1.0)
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731

    def table(base, off):
        return (ctypes.c_void_p * batch)(*[base + int(off[b]) * 8 if n[b] else None for b in range(batch)])

    def call(name, bases):
        t = [table(bases[k], offs[k]) if bases[k] is not None else None for k in range(4)]
        tail = (None if iarr is None else I(iarr), out.ctypes.data_as(_dp), qt, ctypes.byref(sec))
        if full:
            fn = getattr(lib, ("ek_hip_check_sygv_xvbatched" if kind > 1 else "ek_hip_check_xvbatched") + name)
            return fn(kind, batch, I(n), t[0], I(lda), t[1], I(ldb), t[2], t[3], I(ldz), *tail)
        entry, first = _entry(kind, sygv1)
        return getattr(lib, entry + name)(first, batch, I(n), t[0], I(lda), t[1], I(ldb), I(marr), t[2], t[3], I(ldz),
                                          I(zcap), *tail)

    o = _Out()
    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) if x is not None else None for x in h]
            o.rc = call("_device", [None if p is None else p.value for p in d])
            o.untouched = all(x is None or _same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [None if x is None else x.copy() for x in h]
        o.rc = call("", [None if x is None else x.ctypes.data for x in g])
        o.untouched = all(x is None or _same(y, x) for y, x in zip(g, h))
    assert np.array_equal(n, [p.n for p in probs]) and (m is not None or np.array_equal(marr, own))
    o.seconds = sec.value
    o.out, o.rows = out[:batch * 4].reshape(batch, 4), q
    o.tail = out[batch * 4:]
    return o


def _clean(o, probs, info=None, m=None, rows=None, width=None):
    """The call succeeded, wrote nothing behind out, nothing of an IPR row from m[b] on (an unwanted, skipped or empty
    problem's row: nothing at all) and nothing of A, B, w, Z; a problem that is not checked has four NaN."""
    assert o.rc == 0 and o.untouched and o.seconds >= 0.0
    assert np.all(o.tail == SENTINEL)
    for b, p in enumerate(probs):
        k = p.m if m is None else m[b]
        live = (info is None or info[b] == 0) and k > 0
        wrote = (k if width is None else width[b]) if live and (rows is None or rows[b]) else 0
        assert np.all(o.rows[b][wrote:] == SENTINEL), b
        assert not np.any(o.rows[b][:wrote] == SENTINEL), b
        if not live:
            assert np.all(np.isnan(o.out[b])), b


def _alone(lib, p):
    """The one-problem uniform window check on p in the compact layout with zcap = m, device form: (out of 4, ipr of m)."""
    if p.key not in _alone_cache:
        fn = _uniform_plain if p.kind in (0, 1) else _uniform_sygv
        o = fn(lib, "device", p.kind, p.A[None], None if p.B is None else p.B[None], [p.m], [p.w], [p.Z], p.m)
        assert o.rc == 0 and o.untouched
        res = (o.out[0].copy(), o.ipr[0, :p.m].copy())
        for x in res:
            x.setflags(write=False)
        _alone_cache[p.key] = res
    return _alone_cache[p.key]


def _bits_of_alone(lib, o, probs, skip=()):
    for b, p in enumerate(probs):
        if b in skip or p.m == 0:
            continue
        out, ipr = _alone(lib, p)
        assert _same(o.out[b], out), (b, p.key, o.out[b], out)
        assert _same(o.rows[b][:p.m], ipr), (b, p.key)


def _report(shares, names, what, limit=1.0):
    shares = np.asarray(shares).reshape(-1, 5).max(axis=0)
    print("shares of the bounds %s: " % (what,) + ", ".join("%s %.3f" % kv for kv in zip(names, shares)))
    assert np.all(shares <= limit), (what, shares)


# ---------------------------------------------------------------------------------------- 1: bits of the uniform call
@KINDS
def test_bits_of_the_uniform_call(hip, kind):
    lib = hip.load_library()
    for shuffle, lay in ((0, 0), (1, 1)):
        probs = _batch(kind, shuffle=shuffle)
        for form in ("device", "host"):
            o = _vcheck(lib, form, kind, probs, lay=lay)
            _clean(o, probs)
            _bits_of_alone(lib, o, probs)
            live = np.array([p.m > 0 for p in probs])
            assert not np.isnan(o.out[live]).any()                       # no NaN comes out of a clean problem
            assert not any(np.isnan(o.rows[b][:p.m]).any() for b, p in enumerate(probs))


# ---------------------------------------------------------------------------------------- 2: identities
@pytest.mark.parametrize("form", ["device", "host"])
def test_itype_1_is_problem_1_and_type_2_shares_its_metric(hip, form):
    """The windows of the type-2 table (any Z serves) through the three ways."""
    lib = hip.load_library()
    probs = _batch(2)
    plain = _vcheck(lib, form, 1, probs)
    one = _vcheck(lib, form, 1, probs, sygv1=True)
    two = _vcheck(lib, form, 2, probs)
    for o in (plain, one, two):
        _clean(o, probs)
    live = [b for b, p in enumerate(probs) if p.m]
    assert _same(one.out, plain.out) and all(_same(one.rows[b], plain.rows[b]) for b in range(len(probs)))
    assert _same(two.out[:, 3], plain.out[:, 3]) and all(_same(two.rows[b], plain.rows[b]) for b in range(len(probs)))
    assert not np.array_equal(two.out[live, 0], plain.out[live, 0])      # ||A|| ||B|| against ||A||


# ---------------------------------------------------------------------------------------- 3: the host mirror
@KINDS
@pytest.mark.parametrize("plant", [False, True])
def test_matches_the_host_mirror(hip, kind, plant):
    lib = hip.load_library()
    probs = _batch(kind, plant=plant)
    o = _vcheck(lib, "device", kind, probs)
    _clean(o, probs)
    shares = [p.shares(o.out[b], o.rows[b][:p.m]) for b, p in enumerate(probs) if p.m]
    if plant:
        for b, p in enumerate(probs):
            if p.m:
                assert o.out[b, 2] > 1e-9 and p.ref[0][2] > 1e-9         # the wrong eigenvalue shows
                assert p.m < 2 or (o.out[b, 3] > 1e-4 and p.ref[0][3] > 1e-4)
    _report(shares, cw.NAMES, ("mirror", kind, "planted" if plant else "clean"))


# ---------------------------------------------------------------------------------------- 4: chunk seams
@KINDS
def test_chunk_seams_leave_the_bits_alone(hip, kind):
    """13 problems of mixed orders (type 3: slots of n^2 + n m doubles of different sizes meet at a seam) in launches of 3
    and of 1, with and without a skipped problem where the first seam falls in the order of execution."""
    lib = hip.load_library()
    probs = [p for p in _batch(kind) if p.n in (0, 17, 65, 129, 192, 256)] + [_Problem(kind, 130, 1, 130)]
    whole = _vcheck(lib, "device", kind, probs)
    _clean(whole, probs)
    work = [(-(p.n * p.n * p.m + (p.n ** 3 // 3 if kind == 3 else 0)), b) for b, p in enumerate(probs) if p.m]
    third = sorted(work)[2][1]                                           # the last entry of the first launch of 3
    before = lib.ek_hip_debug_check_xbatched_chunk(3)
    try:
        for chunk in (3, 1):
            lib.ek_hip_debug_check_xbatched_chunk(chunk)
            o = _vcheck(lib, "device", kind, probs)
            _clean(o, probs)
            assert _same(o.out, whole.out) and all(_same(x, y) for x, y in zip(o.rows, whole.rows)), chunk
            info = np.zeros(len(probs), dtype=np.int32)
            info[third] = 7
            o = _vcheck(lib, "host" if chunk == 1 else "device", kind, probs, info=info)
            _clean(o, probs, info=info)
            keep = info == 0
            assert _same(o.out[keep], whole.out[keep]), chunk
            assert all(_same(o.rows[b], whole.rows[b]) for b in np.flatnonzero(keep)), chunk
    finally:
        assert lib.ek_hip_debug_check_xbatched_chunk(before) == 1
    assert lib.ek_hip_debug_check_xbatched_chunk(before) == before       # the hook is restored
    _bits_of_alone(lib, whole, probs)


# ---------------------------------------------------------------------------------------- 5: own slots
@KINDS
def test_failures_keep_to_their_own_slots(hip, kind):
    lib = hip.load_library()
    n = 130
    probs = [_Problem(kind, n, b % cw.COUNT, c) for b, c in enumerate((17, 33, 16, 0, 65, 130, 17, 31))]
    probs.insert(4, _Problem(kind, 0, 0, 0))
    probs.insert(7, _Problem(kind, 192, 1, 64))
    clean = _vcheck(lib, "device", kind, probs)
    _clean(clean, probs)
    batch = len(probs)
    info = np.zeros(batch, dtype=np.int32)
    m = np.array([p.m for p in probs], dtype=np.int32)
    info[0] = 3                                                          # skipped: its m, w and Z are not looked at
    info[2], m[2] = -20, 40                                              # the count of a window that did not fit: > zcap
    bad = [p for p in probs]
    nan_at = 5                                                           # the m = 65 problem: a NaN in a read column
    hurt = _Problem(kind, probs[nan_at].n, probs[nan_at].key[2], probs[nan_at].m)
    hurt.Z = hurt.Z.copy()
    hurt.Z[n // 2, 64] = np.nan
    bad[nan_at] = hurt
    spd_at = 8                                                           # type 3: B[k, k] negated
    if kind == 3:
        ind = _Problem(kind, probs[spd_at].n, probs[spd_at].key[2], probs[spd_at].m)
        ind.B = ind.B.copy()
        ind.B[n - 1, n - 1] = -ind.B[n - 1, n - 1]
        bad[spd_at] = ind
    for form in ("device", "host"):
        o = _vcheck(lib, form, kind, bad, info=info, m=m)
        _clean(o, bad, info=info, m=m)
        touched = {0, 2, nan_at} | ({spd_at} if kind == 3 else set())
        for b in range(batch):
            if b not in touched:
                assert _same(o.out[b], clean.out[b]) and _same(o.rows[b], clean.rows[b]), (form, b)
        # the NaN shows in the maximum (which keeps it), the average, the metric and that column's IPR
        assert np.isnan(o.out[nan_at, 1:]).all() and np.isnan(o.rows[nan_at][64])
        assert _same(o.out[nan_at, :1], clean.out[nan_at, :1])
        if kind == 3:
            assert np.isnan(o.out[spd_at, 3]) and np.isnan(o.rows[spd_at][:bad[spd_at].m]).all()
            assert np.isfinite(o.out[spd_at, :3]).all()
    # order 0 and the empty window: four NaN (asserted by _clean), not the a_norm = 0 of the full variable check
    assert probs[4].n == 0 and probs[3].m == 0


# ---------------------------------------------------------------------------------------- 6: m = n throughout
@KINDS
def test_whole_spectra_agree_with_the_full_variable_check(hip, kind):
    lib = hip.load_library()
    probs = [_Problem(kind, n, b, n) for n in cw.ORDERS for b in range(2)]
    perm = np.random.default_rng(61).permutation(len(probs))
    probs = [probs[i] for i in perm]
    o = _vcheck(lib, "device", kind, probs)
    _clean(o, probs)
    f = _vcheck(lib, "device", kind, probs, full=True)
    assert f.rc == 0
    shares = [p.shares(o.out[b], o.rows[b][:p.n], ref=(f.out[b].astype(np.longdouble), f.rows[b][:p.n]))
              for b, p in enumerate(probs)]
    _report(np.asarray(shares) / 2.0, cw.NAMES, ("m = n against the full variable check, of twice the bound", kind))


# ---------------------------------------------------------------------------------------- 7: many workgroups
@KINDS
def test_608_problems_of_order_129_in_three_launches(hip, kind):
    lib = hip.load_library()
    p = _Problem(kind, 129, 0, 17)
    probs = [p] * 608
    before = lib.ek_hip_debug_check_xbatched_chunk(256)
    try:
        o = _vcheck(lib, "device", kind, probs, lay=1, alias=True)
    finally:
        lib.ek_hip_debug_check_xbatched_chunk(before)
    _clean(o, probs)
    out, ipr = _alone(lib, p)
    assert _same(o.out, np.tile(out, (608, 1)))
    assert all(_same(r[:17], ipr) for r in o.rows)


# ---------------------------------------------------------------------------------------- 8: behind the solvers
@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("kind", [1, 3])
def test_behind_the_variable_window_solvers(hip, kind, by_value):
    """A mixed batch of orders 1 .. 256 through ek_hip_eigenpairs_window_xvbatched_device (problem 1) or
    ek_hip_sygv_window_xvbatched_device (type 3), then n, m, dw, dZ, ldz, zcap and info handed over unchanged.  By value,
    every fifth problem gets an interval below its spectrum: an empty window."""
    lib = hip.load_library()
    cases = xc.mixed(0)
    batch = len(cases)
    n = np.array([c.n for c in cases], dtype=np.int32)
    il = np.array([c.il for c in cases], dtype=np.int32)
    iu = np.array([c.iu for c in cases], dtype=np.int32)
    vl, vu = np.zeros(batch), np.zeros(batch)
    zcap = np.array([c.zcap for c in cases], dtype=np.int32)
    empty = np.zeros(batch, dtype=bool)
    if by_value:
        for b, c in enumerate(cases):
            vl[b], vu[b], _, mb = xc.bounds(c, kind)
            zcap[b] = mb + c.extra
            if b % 5 == 4:
                vl[b], vu[b], empty[b] = -3e9, -2e9, True
    offm = np.concatenate([[0], np.cumsum(n.astype(np.int64) * n)])
    offw = np.concatenate([[0], np.cumsum(n)])
    offz = np.concatenate([[0], np.cumsum(n.astype(np.int64) * np.maximum(zcap, 1))])
    hA, hB = np.zeros(offm[-1]), np.zeros(offm[-1])
    for b, c in enumerate(cases):
        hA[offm[b]:offm[b + 1]] = c.A.T.ravel()
        hB[offm[b]:offm[b + 1]] = c.B.T.ravel()
    m = np.full(batch, 777, dtype=np.int32)
    info = np.full(batch, 777, dtype=np.int32)
    out = np.full((batch, 4), SENTINEL)
    rows = [np.full(k + 1, SENTINEL) for k in n]
    qt = (ctypes.c_void_p * batch)(*[r.ctypes.data for r in rows])
    one, ipr1 = np.zeros(4), np.zeros(256)
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731
    D = lambda a: a.ctypes.data_as(_dp)                 # noqa: E731
    solve = lib.ek_hip_sygv_window_xvbatched_device if kind == 3 else lib.ek_hip_eigenpairs_window_xvbatched_device
    with _Dev(lib) as dev:
        dA, dB, dA0, dB0 = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.full(offw[-1], np.nan)), dev.up(np.full(offz[-1], np.nan))

        def table(base, off):
            return (ctypes.c_void_p * batch)(*[base.value + int(off[b]) * 8 for b in range(batch)])

        tw, tZ = table(dw, offw), table(dZ, offz)
        rc = solve(kind, 1, 1 if by_value else 0, batch, I(n), D(vl), D(vu), I(il), I(iu), table(dA, offm), I(n),
                   table(dB, offm), I(n), I(m), tw, tZ, I(n), I(zcap), I(info), None)
        assert rc == 0 and not info.any()
        assert np.array_equal(m == 0, empty)
        check = lib.ek_hip_check_sygv_window_xvbatched_device if kind == 3 else lib.ek_hip_check_window_xvbatched_device
        rc = check(kind, batch, I(n), table(dA0, offm), I(n), table(dB0, offm), I(n), I(m), tw, tZ, I(n), I(zcap), I(info),
                   D(out), qt, None)
        assert rc == 0
        first = int(np.flatnonzero(m > 0)[0])
        k = int(n[first])
        at = lambda p, off: ctypes.c_void_p(p.value + int(off) * 8)      # noqa: E731
        rc = lib.ek_hip_check_sygvx_device(kind, k, int(m[first]), at(dA0, offm[first]), k, at(dB0, offm[first]), k,
                                           at(dw, offw[first]), at(dZ, offz[first]), k, D(one), D(ipr1))
        assert rc == 0
    worst = np.zeros(2)
    for b in range(batch):
        if empty[b]:
            assert np.all(np.isnan(out[b])) and np.all(rows[b] == SENTINEL)
            continue
        assert np.all(np.isfinite(out[b])) and np.all(rows[b][m[b]:] == SENTINEL)
        assert np.all(np.isfinite(rows[b][:m[b]]) & (rows[b][:m[b]] > 0.0))
        share = np.array([out[b, 2] / (64 * n[b] * EPS), out[b, 3] / (256 * n[b] * EPS)])
        assert np.all(share <= 1.0), (b, n[b], m[b], out[b])
        worst = np.maximum(worst, share)
    p = _Problem(kind, 0, 0, 0)
    p.n, p.cond = k, float(np.linalg.cond(cases[first].B))
    s = p.shares(out[first], rows[first][:m[first]], ref=(one.astype(np.longdouble), ipr1[:m[first]]))
    print("behind the solver, kind %d, %s: res_max %.4f of 64 n eps, orthogonality %.4f of 256 n eps; against "
          "ek_hip_check_sygvx_device %.3f of the bound" % (kind, "V" if by_value else "I", worst[0], worst[1], s.max()))
    assert np.all(s <= 1.0), s


# ---------------------------------------------------------------------------------------- 9: one pool
@KINDS
def test_one_pool_with_the_other_check_entries(hip, kind):
    """The variable window check after ek_hip_check_batched, ek_hip_check_xbatched, ek_hip_check_window_xbatched and
    ek_hip_check_xvbatched have used the pool, and the same calls after it again: the same bits both ways."""
    lib = hip.load_library()
    probs = [p for p in _batch(kind) if p.n in (0, 33, 129, 256)]

    def others():
        res = []
        for n in (64, 200):
            c = cw.cases(n, 1)
            fn = hip.check_batched if n <= 128 else hip.check_xbatched
            res.append(fn(c.A, c.B, c.w, c.Z))
        c = cw.cases(129, 1)
        ws, Zs = cw.windows(129, 1, 17, False)
        res.append(hip.check_window_xbatched(c.A, c.B, [17] * cw.COUNT, np.pad(np.stack(ws), ((0, 0), (0, 112))),
                                             np.stack(Zs)))
        f = _vcheck(lib, "device", 1, [_Problem(1, n, 0, n) for n in (33, 129, 256)], full=True)
        assert f.rc == 0
        res.append((f.out, np.concatenate(f.rows)))
        return res

    first = _vcheck(lib, "device", kind, probs)
    a = others()
    second = _vcheck(lib, "device", kind, probs)
    b = others()
    for o in (first, second):
        _clean(o, probs)
    assert _same(first.out, second.out) and all(_same(x, y) for x, y in zip(first.rows, second.rows))
    for (o1, q1), (o2, q2) in zip(a, b):
        assert _same(o1, o2) and _same(q1, q2)
    _bits_of_alone(lib, second, probs)


# ---------------------------------------------------------------------------------------- 10: cost
def test_cost_against_uniform_calls_the_solve_and_the_full_check(hip):
    """128 generalized problems, 8 at each of 16 orders 129 .. 256, the n / 8 pairs from index n / 4 + 1.  Device seconds,
    best of 3 after a warm-up, the kinds alternated.  The variable window check is no dearer than the 16 uniform
    window-check calls (wall time against wall time), no dearer than the variable window solve that produced the pairs, and
    cheaper than ek_hip_check_xvbatched_device on the full solve of the same batch.  Conditions, no tighter gate: the
    measured ratios are in DESIGN.md 37."""
    lib = hip.load_library()
    distinct = np.unique(np.round(np.linspace(129, 256, 16)).astype(np.int64))
    assert len(distinct) == 16
    rng = np.random.default_rng(3710)
    orders = np.repeat(distinct, 8)
    batch = len(orders)
    cols = orders // 8
    offm = np.concatenate([[0], np.cumsum(orders * orders)])
    offw = np.concatenate([[0], np.cumsum(orders)])
    offz = np.concatenate([[0], np.cumsum(orders * cols)])
    hA, hB = np.zeros(offm[-1]), np.zeros(offm[-1])
    for g, k in enumerate(distinct):
        for r in range(8):
            G = rng.standard_normal((k, k))
            M = rng.standard_normal((k, k))
            B = M @ M.T / k + np.eye(k)
            hA[offm[g * 8 + r]:offm[g * 8 + r + 1]] = ((G + G.T) / 2.0).ravel()
            hB[offm[g * 8 + r]:offm[g * 8 + r + 1]] = ((B + B.T) / 2.0).ravel()
    perm = rng.permutation(batch)
    n32 = orders[perm].astype(np.int32)
    il = (n32 // 4 + 1).astype(np.int32)
    iu = (il + n32 // 8 - 1).astype(np.int32)
    zc = (n32 // 8).astype(np.int32)
    m = np.zeros(batch, dtype=np.int32)
    m8 = np.zeros(8, dtype=np.int32)
    info = np.zeros(batch, dtype=np.int32)
    sec = np.zeros(1)
    out = np.zeros((batch, 4))
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731
    D = lambda a: a.ctypes.data_as(_dp)                 # noqa: E731
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(offw[-1])), dev.up(np.zeros(offz[-1]))
        dwf, dZf = dev.up(np.zeros(offw[-1])), dev.up(np.zeros(offm[-1]))

        def table(base, off):
            return (ctypes.c_void_p * batch)(*[base.value + int(off[b]) * 8 for b in perm])

        def at(p, off):
            return ctypes.c_void_p(p.value + int(off) * 8)

        tA0, tB0, tA, tB = table(dA0, offm), table(dB0, offm), table(dA, offm), table(dB, offm)
        tw, tZ, twf, tZf = table(dw, offw), table(dZ, offz), table(dwf, offw), table(dZf, offm)

        def solve():
            dev.put(dA, hA); dev.put(dB, hB)
            rc = lib.ek_hip_eigenpairs_window_xvbatched_device(1, 1, 0, batch, I(n32), None, None, I(il), I(iu), tA, I(n32),
                                                               tB, I(n32), I(m), tw, tZ, I(n32), I(zc), I(info), D(sec))
            assert rc == 0 and not info.any() and (m == zc).all()
            return float(sec[0])

        def solve_full():
            dev.put(dA, hA); dev.put(dB, hB)
            rc = lib.ek_hip_eigenpairs_xvbatched_device(1, 1, batch, I(n32), tA, I(n32), tB, I(n32), twf, tZf, I(n32),
                                                        I(info), D(sec))
            assert rc == 0 and not info.any()

        def variable():
            t0 = time.perf_counter()
            rc = lib.ek_hip_check_window_xvbatched_device(1, batch, I(n32), tA0, I(n32), tB0, I(n32), I(m), tw, tZ, I(n32),
                                                          I(zc), I(info), D(out), None, D(sec))
            wall = time.perf_counter() - t0
            assert rc == 0
            return float(sec[0]), wall

        def per_order():
            t0 = time.perf_counter()
            for g, k in enumerate(distinct):
                k, f, c = int(k), g * 8, int(k) // 8
                m8[:] = c
                rc = lib.ek_hip_check_window_xbatched_device(1, k, 8, at(dA0, offm[f]), k, k * k, at(dB0, offm[f]), k, k * k,
                                                             I(m8), at(dw, offw[f]), at(dZ, offz[f]), k, c, k * c, None,
                                                             D(out), None, None)
                assert rc == 0
            return time.perf_counter() - t0

        def full():
            rc = lib.ek_hip_check_xvbatched_device(1, batch, I(n32), tA0, I(n32), tB0, I(n32), twf, tZf, I(n32), I(info),
                                                   D(out), None, D(sec))
            assert rc == 0
            return float(sec[0])

        solve_full()
        t_solve = [solve() for _ in range(4)][1:]
        variable(); per_order(); full()                 # warm-up
        t_var, t_wall, t_uni, t_full = [], [], [], []
        for _ in range(3):
            s, w = variable()
            t_var.append(s); t_wall.append(w); t_uni.append(per_order()); t_full.append(full())
        assert np.all(np.isfinite(out)) and out[:, 2].max() <= 64 * 256 * EPS
    t_var, t_wall, t_uni, t_full, t_solve = min(t_var), min(t_wall), min(t_uni), min(t_full), min(t_solve)
    print("128 problems of order 129..256, n / 8 pairs: variable window check %.3f ms (wall %.3f ms), 16 uniform "
          "window-check calls %.3f ms wall (ratio %.3f), variable window solve %.3f ms (ratio %.3f), full variable check "
          "%.3f ms (ratio %.3f)" % (t_var * 1e3, t_wall * 1e3, t_uni * 1e3, t_wall / t_uni, t_solve * 1e3,
                                    t_var / t_solve, t_full * 1e3, t_var / t_full))
    assert t_wall <= t_uni, (t_wall, t_uni)
    assert t_var <= t_solve, (t_var, t_solve)
    assert t_var < t_full, (t_var, t_full)
