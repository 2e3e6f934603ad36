"""ek_hip_eigenpairs_window_xvbatched* and ek_hip_sygv_window_xvbatched* on the GPU: a window of eigenpairs per problem for
problems of different orders in one call.

The contract is the family's bit contract: problem b's m, info, w[:m], Z[:, :m] and the in-place images of dA[b] and dB[b]
are, by tobytes, what a one-problem ek_hip_*_window_xbatched_device call returns for (n[b], A, B, window b, zcap[b]) --
wherever the problem sits, in whichever launch, under either stream setting, in the host and the device form.  Cases,
windows, bounds and judges are those of tests/window_xvbatched_cases.py; no tolerance is new.

kind: 0 the standard problem, 1 A x = l B x (the eigenpairs entries), 2 and 3 DSYGV's types (the sygv entries)."""
import ctypes

import numpy as np
import pytest

import sygv_window_cases as sc
import window_xvbatched_cases as xc
from test_gpu_vbatched import _Dev, _Out

pytestmark = pytest.mark.gpu
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
_uniform = {}                                           # one-problem uniform calls, made once and never modified


def _entries(kind):
    """(variable device, variable host, uniform device, first argument)"""
    if kind in (0, 1):
        return ("ek_hip_eigenpairs_window_xvbatched_device", "ek_hip_eigenpairs_window_xvbatched",
                "ek_hip_eigenpairs_window_xbatched_device", kind)
    return ("ek_hip_sygv_window_xvbatched_device", "ek_hip_sygv_window_xvbatched", "ek_hip_sygv_window_xbatched_device",
            kind)


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def _window(case, kind, by_value, alt=False):
    """(il, iu, vl, vu, zcap) of the case; alt: a second, different index window that holds the first one's first index
    (order 1 has no second window)."""
    if alt:
        if case.il > 1:
            il, iu = case.il - 1, case.il
        elif case.iu < case.n:
            il, iu = 1, case.iu + 1
        else:
            il, iu = 1, max(1, case.n - 1)
        return il, iu, None, None, iu - il + 1
    if not by_value:
        return case.il, case.iu, None, None, case.zcap
    vl, vu, _, m = xc.bounds(case, kind)
    return None, None, vl, vu, m + case.extra


def _alone(lib, case, kind, jobz, by_value, alt=False):
    """The uniform device entry on the one problem, as sygv_window_cases.window_device runs it."""
    key = (case.key, kind, jobz, by_value, alt, case.il, case.iu, case.extra)
    if key not in _uniform:
        il, iu, vl, vu, zcap = _window(case, kind, by_value, alt)
        uni, first = _entries(kind)[2:]
        _uniform[key] = sc.window_device(lib, uni, first, case.A[None], case.B[None] if kind else None, jobz, il=il,
                                         iu=iu, vl=vl, vu=vu, zcap=zcap)
        assert _uniform[key].rc == 0
    return _uniform[key]


def _variable(lib, cases, kind, jobz, by_value, host=False, pad=0, gap=0, alt=False, data=None, wins=None, entry=None):
    """The variable entry on one arena per array kind: lower triangles only, NaN in the strictly upper triangles, the rows
    n .. ld-1, the gaps between the problems, all of w and all of Z.  data: {position: (A, B)} in place of a case's pair;
    wins: {position: (il, iu, vl, vu, zcap)} in place of its window; entry: (name, first argument) in place of the kind's
    device entry.  Returns the per-problem pieces and the arenas before and after."""
    dev_entry, host_entry, _, first = _entries(kind)
    if entry:
        dev_entry, first = entry
    batch = len(cases)
    n = np.array([c.n for c in cases], dtype=np.int32)
    ld = np.maximum(n + pad, 1).astype(np.int32)
    win = [(wins or {}).get(b) or _window(c, kind, by_value, alt) for b, c in enumerate(cases)]
    zcap = np.array([w[4] for w in win], dtype=np.int32)
    il = np.array([w[0] or 0 for w in win], dtype=np.int32)
    iu = np.array([w[1] or 0 for w in win], dtype=np.int32)
    vl = np.array([w[2] if w[2] is not None else 0.0 for w in win])
    vu = np.array([w[3] if w[3] is not None else 0.0 for w in win])
    offm = np.concatenate([[0], np.cumsum(ld.astype(np.int64) * n + gap)])
    offw = np.concatenate([[0], np.cumsum(n.astype(np.int64) + gap)])
    offz = np.concatenate([[0], np.cumsum(ld.astype(np.int64) * np.maximum(zcap, 1) + gap)])
    hA, hB = np.full(max(offm[-1], 1), np.nan), np.full(max(offm[-1], 1), np.nan)
    hw, hZ = np.full(max(offw[-1], 1), np.nan), np.full(max(offz[-1], 1), np.nan)
    for b, c in enumerate(cases):
        A, B = (c.A, c.B) if not data or b not in data else data[b]
        low = np.tril(np.ones((c.n, c.n), dtype=bool))
        for flat, M in ((hA, A), (hB, B)):
            img = flat[offm[b]:offm[b] + ld[b] * c.n].reshape(c.n, ld[b])
            img[:, :c.n][low.T] = M.T[low.T]
    m = np.full(batch, 777, dtype=np.int32)
    info = np.full(batch, 777, dtype=np.int32)
    sec = np.zeros(1)
    o = _Out()

    def table(base, off):
        return (ctypes.c_void_p * batch)(*[base + int(off[b]) * 8 for b in range(batch)])

    def call(entry, pA, pB, pw, pZ):
        return getattr(lib, entry)(first, jobz, 1 if by_value else 0, batch, n.ctypes.data_as(_ip),
                                   vl.ctypes.data_as(_dp), vu.ctypes.data_as(_dp), il.ctypes.data_as(_ip),
                                   iu.ctypes.data_as(_ip), table(pA, offm), ld.ctypes.data_as(_ip),
                                   table(pB, offm) if kind else None, ld.ctypes.data_as(_ip), m.ctypes.data_as(_ip),
                                   table(pw, offw), table(pZ, offz) if jobz else None, ld.ctypes.data_as(_ip),
                                   zcap.ctypes.data_as(_ip), info.ctypes.data_as(_ip), sec.ctypes.data_as(_dp))

    if host:
        aA, aB, aw, aZ = hA.copy(), hB.copy(), hw.copy(), hZ.copy()
        o.rc = call(host_entry, aA.ctypes.data, aB.ctypes.data, aw.ctypes.data, aZ.ctypes.data)
    else:
        with _Dev(lib) as dev:
            dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
            o.rc = call(dev_entry, dA.value, dB.value, dw.value, dZ.value)
            aA, aB, aw, aZ = dev.down(dA, hA), dev.down(dB, hB), dev.down(dw, hw), dev.down(dZ, hZ)
    o.m, o.info, o.seconds, o.zcap, o.n = m, info, float(sec[0]), zcap, n
    o.before, o.after = (hA, hB, hw, hZ), (aA, aB, aw, aZ)
    o.A = [aA[offm[b]:offm[b] + ld[b] * n[b]].reshape(n[b], ld[b])[:, :n[b]].T for b in range(batch)]
    o.B = [aB[offm[b]:offm[b] + ld[b] * n[b]].reshape(n[b], ld[b])[:, :n[b]].T for b in range(batch)]
    o.w = [aw[offw[b]:offw[b] + n[b]] for b in range(batch)]
    o.Z = [aZ[offz[b]:offz[b] + ld[b] * max(zcap[b], 1)].reshape(max(zcap[b], 1), ld[b])[:, :n[b]].T
           for b in range(batch)]
    # what the call may have written: lower triangles of A (and B), m[b] values, m[b] columns of n[b] rows
    allowed = tuple(np.zeros(len(x), dtype=bool) for x in o.before)
    for b in range(batch):
        low = np.tril(np.ones((n[b], n[b]), dtype=bool))
        for k in (0, 1):
            if host or (k == 1 and not kind):
                continue
            allowed[k][offm[b]:offm[b] + ld[b] * n[b]].reshape(n[b], ld[b])[:, :n[b]][low.T] = True
        mb = int(m[b]) if info[b] == 0 else 0
        allowed[2][offw[b]:offw[b] + mb] = True
        if jobz and mb:
            allowed[3][offz[b]:offz[b] + ld[b] * mb].reshape(mb, ld[b])[:, :n[b]] = True
    o.allowed = allowed
    return o


def _untouched(o):
    """Everything outside what the call may write is the same bits as before (NaN sentinels included)."""
    for before, after, ok in zip(o.before, o.after, o.allowed):
        assert _bits(before[~ok]) == _bits(after[~ok])
        assert not np.isnan(after[ok]).any()


def _same_as_alone(lib, o, cases, kind, jobz, by_value, host=False, alt=False, skip=()):
    for b, c in enumerate(cases):
        if b in skip:
            continue
        u = _alone(lib, c, kind, jobz, by_value, alt)
        what = (b, c.key, c.name, kind, jobz, by_value)
        assert o.m[b] == u.m[0] and o.info[b] == u.info[0], (what, o.m[b], u.m[0], o.info[b], u.info[0])
        mb = int(o.m[b]) if o.info[b] == 0 else 0
        assert _bits(o.w[b][:mb]) == _bits(u.w[0][:mb]), what
        if jobz:
            assert _bits(o.Z[b][:, :mb]) == _bits(u.Z[0][:, :mb]), what
        if not host:
            assert _bits(o.A[b]) == _bits(u.A[0]), what
            if kind:
                assert _bits(o.B[b]) == _bits(u.B[0]), what


# ---------------------------------------------------------------------------------- 1: the bits of the uniform call
@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_bits_of_the_uniform_call(hip, kind, by_value, jobz):
    """Both shuffles in the device form (the second with padded leading dimensions and gaps) and the first in the host
    form: every problem the bits of the one-problem uniform device call, and nothing else touched."""
    lib = hip.load_library()
    for shuffle in xc.SHUFFLES:
        cases = xc.mixed(shuffle)
        o = _variable(lib, cases, kind, jobz, by_value, pad=3 * shuffle, gap=5 * shuffle)
        assert o.rc == 0
        assert not o.info.any(), o.info
        if not by_value:
            assert all(o.m[b] == c.iu - c.il + 1 for b, c in enumerate(cases))
        else:
            assert all(o.m[b] == xc.bounds(c, kind)[3] for b, c in enumerate(cases))
        _same_as_alone(lib, o, cases, kind, jobz, by_value)
        _untouched(o)
    cases = xc.mixed(0)
    h = _variable(lib, cases, kind, jobz, by_value, host=True, pad=2, gap=3)
    assert h.rc == 0 and not h.info.any()
    _same_as_alone(lib, h, cases, kind, jobz, by_value, host=True)
    _untouched(h)                                       # A and B are inputs here: not a bit of them changes


@pytest.mark.parametrize("kind", [1, 3])
def test_value_of_an_index_in_another_window(hip, kind):
    """The value (and, alone in both windows, nothing else) of an index is the same bits in a second, different window."""
    lib = hip.load_library()
    cases = xc.mixed(1)
    a = _variable(lib, cases, kind, 1, False)
    b = _variable(lib, cases, kind, 1, False, alt=True)
    assert a.rc == 0 and b.rc == 0 and not a.info.any() and not b.info.any()
    other = 0
    for k, c in enumerate(cases):
        il2, iu2 = _window(c, kind, False, alt=True)[:2]
        other += (il2, iu2) != (c.il, c.iu)
        assert _bits(a.w[k][:1]) == _bits(b.w[k][c.il - il2:c.il - il2 + 1]), (k, c.key)
    assert other >= len(cases) - 2                      # every order but 1 has a second window
    _same_as_alone(lib, b, cases, kind, 1, False, alt=True)


# ---------------------------------------------------------------------------------- 2: other bit equalities
def test_small_orders_launch_no_class_of_256(hip):
    lib = hip.load_library()
    cases = xc.mixed(0, xc.SMALL_ORDERS)
    o = _variable(lib, cases, 1, 1, False)
    assert o.rc == 0 and not o.info.any()
    _same_as_alone(lib, o, cases, 1, 1, False)
    sec, cnt = np.zeros(4), np.zeros(4, dtype=np.int32)
    assert lib.ek_hip_debug_xvbatched_last(sec.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip)) == 0
    orders = np.array([c.n for c in cases])
    assert cnt[0] == 0 and sec[0] == 0.0
    assert list(cnt[1:]) == [int(((orders > 64)).sum()), int(((orders > 32) & (orders <= 64)).sum()),
                             int((orders <= 32).sum())]


@pytest.mark.parametrize("by_value", [False, True])
def test_itype_1_is_the_eigenpairs_entry_and_types_2_and_3_agree(hip, by_value):
    lib = hip.load_library()
    cases = xc.mixed(0)
    e = _variable(lib, cases, 1, 1, by_value)
    s = _variable(lib, cases, 1, 1, by_value, entry=("ek_hip_sygv_window_xvbatched_device", 1))
    assert e.rc == 0 and s.rc == 0
    for x, y in zip(e.after, s.after):
        assert _bits(x) == _bits(y)
    assert _bits(e.m) == _bits(s.m) and _bits(e.info) == _bits(s.info)
    t2, t3 = _variable(lib, cases, 2, 1, by_value), _variable(lib, cases, 3, 1, by_value)
    assert t2.rc == 0 and t3.rc == 0 and not t2.info.any() and not t3.info.any()
    assert _bits(t2.m) == _bits(t3.m)
    assert _bits(t2.after[2]) == _bits(t3.after[2]) and _bits(t2.after[0]) == _bits(t3.after[0])
    worst = 0.0
    for b, c in enumerate(cases):                       # Z3 = B Z2, the bound of sygv_window_cases: 256 n eps
        mb = int(t2.m[b])
        Z2, Z3 = t2.Z[b][:, :mb], t3.Z[b][:, :mb]
        BZ = c.B @ Z2
        err = (np.linalg.norm(Z3 - BZ, axis=0) / np.linalg.norm(BZ, axis=0)).max()
        worst = max(worst, err / (256 * c.n * sc.EPS))
        assert err <= 256 * c.n * sc.EPS, (b, c.key, err)
    print("Z3 = B Z2: share of 256 n eps used %.4f" % worst)


# ---------------------------------------------------------------------------------- 4: failures in their own slots
@pytest.mark.parametrize("kind", [1, 2])
def test_failures_keep_to_their_own_slots(hip, kind):
    """A B that is not SPD, a NaN in A, a 'V' window wider than its zcap, an empty 'V' window and an empty problem among
    the mixed batch: each reports in its own slot and the neighbours' bits are those of the batch without failures."""
    lib = hip.load_library()
    cases = list(xc.mixed(0))
    good = _variable(lib, cases, kind, 1, True)
    assert good.rc == 0 and not good.info.any()
    pos = {c.n: b for b, c in enumerate(cases)}
    b_spd, b_nan, b_empty, b_zero = pos[130], pos[65], pos[33], pos[2]
    b_wide = next(b for b, c in enumerate(cases) if c.n > 128 and good.m[b] >= 2 and b != b_spd)
    data, wins = {}, {}
    Bbad = np.array(cases[b_spd].B)
    Bbad[40, 40] = -1.0                                 # the pivot that ek_hip_solve_device reports: 41
    data[b_spd] = (cases[b_spd].A, Bbad)
    Anan = np.array(cases[b_nan].A)
    Anan[7, 3] = np.nan
    data[b_nan] = (Anan, cases[b_nan].B)
    count = int(good.m[b_wide])
    wins[b_wide] = _window(cases[b_wide], kind, True)[:4] + (count - 1,)
    low = xc.spectrum(cases[b_empty], kind)[0][0]
    wins[b_empty] = (None, None, low - 2.0, low - 1.0, 1)   # an interval below the whole spectrum
    batch = list(cases)
    batch[b_zero] = xc.Case(("zero",), np.zeros((0, 0)), np.zeros((0, 0)), 1, 0, 0, "order 0")
    wins[b_zero] = (None, None, 0.0, 1.0, 0)
    o = _variable(lib, batch, kind, 1, True, data=data, wins=wins)
    assert o.rc == 0
    assert o.info[b_spd] == 41 and o.m[b_spd] == 0
    assert o.info[b_nan] == -5 and o.m[b_nan] == 0
    assert o.info[b_wide] == -20 and o.m[b_wide] == count
    assert o.info[b_empty] == 0 and o.m[b_empty] == 0
    assert o.info[b_zero] == 0 and o.m[b_zero] == 0
    failed = (b_spd, b_nan, b_wide, b_empty, b_zero)
    for b in failed:                                    # w and Z sentinels intact
        assert np.isnan(o.w[b]).all() and np.isnan(o.Z[b]).all()
    for b in range(len(cases)):
        if b in failed:
            continue
        assert o.info[b] == 0 and o.m[b] == good.m[b]
        for x, y in ((o.w, good.w), (o.Z, good.Z), (o.A, good.A), (o.B, good.B)):
            assert _bits(x[b]) == _bits(y[b]), b


# ---------------------------------------------------------------------------------- 5, 6: seams and streams
def _eight_per_class():
    cases = []
    for n in (20, 31, 50, 64, 100, 128, 200, 256):
        cases += [c for c in xc.problems((n,), 4)]
    perm = np.random.default_rng(88).permutation(len(cases))
    return [cases[i] for i in perm]


def test_chunk_seams_leave_the_bits_alone(hip):
    """Both chunk hooks at 3 on a batch with 8 problems per class, then a byte budget that ends the launches: the bits of
    the unhooked call."""
    lib = hip.load_library()
    cases = _eight_per_class()
    ref = _variable(lib, cases, 1, 1, False)
    assert ref.rc == 0 and not ref.info.any()
    try:
        lib.ek_hip_debug_window_batched_chunk(3)
        lib.ek_hip_debug_window_xbatched_chunk(3)
        o = _variable(lib, cases, 1, 1, False)
        lib.ek_hip_debug_window_batched_chunk(0)
        lib.ek_hip_debug_window_xbatched_chunk(0)
        # the widest slot of the batch and a little: a launch holds one wide problem or a few narrow ones
        widest = max(5 * c.n * (c.iu - c.il + 1) * 8 for c in cases)
        lib.ek_hip_debug_window_xvbatched_budget(widest + 4096)
        p = _variable(lib, cases, 1, 1, False)
        lib.ek_hip_debug_window_xvbatched_budget(1)     # no slot fits: a problem per launch
        q = _variable(lib, cases, 1, 1, False)
    finally:
        lib.ek_hip_debug_window_batched_chunk(0)
        lib.ek_hip_debug_window_xbatched_chunk(0)
        lib.ek_hip_debug_window_xvbatched_budget(0)
    for x in (o, p, q):
        assert x.rc == 0
        assert _bits(x.m) == _bits(ref.m) and _bits(x.info) == _bits(ref.info)
        for u, v in zip(x.after, ref.after):
            assert _bits(u) == _bits(v)


@pytest.mark.parametrize("kind", [1, 3])
def test_streams_give_the_same_bits(hip, kind):
    """All four classes present, vectors wanted: one stream and a stream per class.  Overlapping LU regions of classes
    that run beside each other would show here."""
    lib = hip.load_library()
    cases = _eight_per_class()
    try:
        lib.ek_hip_debug_vbatched_streams(1)
        one = _variable(lib, cases, kind, 1, False)
        lib.ek_hip_debug_vbatched_streams(3)
        three = _variable(lib, cases, kind, 1, False)
    finally:
        lib.ek_hip_debug_vbatched_streams(3)
    assert one.rc == 0 and three.rc == 0 and not one.info.any() and not three.info.any()
    for u, v in zip(one.after, three.after):
        assert _bits(u) == _bits(v)
    _same_as_alone(lib, three, cases, kind, 1, False)


# ---------------------------------------------------------------------------------- 7: accuracy
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_accuracy_of_the_mixed_batch(hip, kind):
    lib = hip.load_library()
    cases = xc.mixed(0)
    worst, fails = [0.0, 0.0, 0.0], []
    for by_value in (False, True):
        o = _variable(lib, cases, kind, 1, by_value)
        assert o.rc == 0 and not o.info.any()
        for b, c in enumerate(cases):
            first = xc.bounds(c, kind)[2] if by_value else c.il - 1
            mb = int(o.m[b])
            s, f = xc.judge_kind(c, kind, first, o.w[b][:mb], o.Z[b][:, :mb], "%s %s" % (c.key, c.name))
            fails += f
            worst = sc.worse(worst, s)
    print("kind %d mixed batch, share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((kind,) + tuple(worst)))
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("itype", [2, 3])
def test_hard_pencils_and_planted_clusters_through_the_variable_call(hip, itype):
    """Orders 33, 128, 129 and 256 in one call: the hard pencils under the rule of tests/sygv_window_cases.py (whole
    spectrum), the planted clusters with the window that cuts them under the suite's bounds."""
    lib = hip.load_library()
    table = xc.hard_cases()
    cases = [c for c, _ in table]
    o = _variable(lib, cases, itype, 1, False)
    assert o.rc == 0
    assert not o.info.any(), o.info
    worst_h, worst_p, fails = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], []
    for b, (c, hard_name) in enumerate(table):
        w_ref, Z_ref = sc.reference(c.key, itype, c.A, c.B)
        mb = int(o.m[b])
        what = "itype=%d %s" % (itype, c.key)
        if hard_name:
            L = np.tril(o.B[b])
            back = np.abs(L @ L.T - c.B).max()
            if not back <= 16 * c.n * sc.EPS * np.abs(c.B).max():
                fails.append("%s: |L L^T - B| = %.3e" % (what, back))
            rule = sc.quantities(itype, c.A, c.B, w_ref, Z_ref)
            s, f = sc.judge(itype, c.A, c.B, w_ref, c.il - 1, o.w[b][:mb], o.Z[b][:, :mb], what, rule=rule, L=L)
            worst_h = sc.worse(worst_h, s)
        else:
            s, f = sc.judge(itype, c.A, c.B, w_ref, c.il - 1, o.w[b][:mb], o.Z[b][:, :mb], what)
            worst_p = sc.worse(worst_p, s)
        fails += f
    print("itype %d hard pencils, share of the rule used: %.3f %.3f %.3f; planted clusters, share of the bound: %.3f %.3f "
          "%.3f" % ((itype,) + tuple(worst_h) + tuple(worst_p)))
    assert not fails, "\n".join(fails[:40])


# ---------------------------------------------------------------------------------- 8: a launch wider than the device
def test_608_problems_of_order_129_in_one_launch(hip):
    lib = hip.load_library()
    A, B = xc.pairs(129)
    cases = [xc.Case(("pair", 129, k % 8), A[k % 8], B[k % 8], 64, 65, 0, "two") for k in range(608)]
    o = _variable(lib, cases, 1, 1, False)
    assert o.rc == 0 and not o.info.any() and (o.m == 2).all()
    _same_as_alone(lib, o, cases, 1, 1, False, skip=set(range(608)) - {0, 512, 607})


# ---------------------------------------------------------------------------------- 9: cost
def _cost(lib, lo, hi, full_entry):
    """Device seconds (best of 3 after a warm-up, the calls alternated, inputs restored outside the clock) of the variable
    window call, of the full variable call `full_entry` and of a uniform window call per distinct order: 512 generalized
    problems, 16 of each of 32 orders spread over lo .. hi, the lowest max(1, n / 8) pairs with vectors.  Two seeded pairs
    per order, each standing 8 times in the batch, every copy its own memory."""
    distinct = np.unique(np.round(np.linspace(lo, hi, 32)).astype(np.int64))
    assert len(distinct) == 32
    rng = np.random.default_rng(9009)
    orders = np.repeat(distinct, 16)
    batch = len(orders)
    offm = np.concatenate([[0], np.cumsum(orders * orders)])
    offw = np.concatenate([[0], np.cumsum(orders)])
    hA, hB = np.zeros(offm[-1]), np.zeros(offm[-1])
    for g, n in enumerate(distinct):
        for k in range(2):
            G = rng.standard_normal((n, n))
            M = rng.standard_normal((n, n))
            A, B = (G + G.T) / 2.0, M @ M.T / n + np.eye(n)
            for r in range(8):
                b = g * 16 + k * 8 + r
                hA[offm[b]:offm[b + 1]] = A.ravel()
                hB[offm[b]:offm[b + 1]] = ((B + B.T) / 2.0).ravel()
    perm = rng.permutation(batch)
    n32 = orders[perm].astype(np.int32)
    il = np.ones(batch, dtype=np.int32)
    iu = np.maximum(1, n32 // 8).astype(np.int32)
    m = np.zeros(batch, dtype=np.int32)
    info = np.zeros(batch, dtype=np.int32)
    sec = np.zeros(1)
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(offw[-1])), dev.up(np.zeros(offm[-1]))

        def table(base, off):
            return (ctypes.c_void_p * batch)(*[base.value + int(off[b]) * 8 for b in perm])

        tA, tB, tw, tZ = table(dA, offm), table(dB, offm), table(dw, offw), table(dZ, offm)

        def at(p, off):
            return ctypes.c_void_p(p.value + int(off) * 8)

        def window():
            dev.put(dA, hA); dev.put(dB, hB)
            rc = lib.ek_hip_eigenpairs_window_xvbatched_device(1, 1, 0, batch, I(n32), None, None, I(il), I(iu), tA,
                                                               I(n32), tB, I(n32), I(m), tw, tZ, I(n32), I(iu), I(info),
                                                               sec.ctypes.data_as(_dp))
            assert rc == 0 and not info.any() and (m == iu).all()
            return float(sec[0])

        def full():
            dev.put(dA, hA); dev.put(dB, hB)
            rc = getattr(lib, full_entry)(1, 1, batch, I(n32), tA, I(n32), tB, I(n32), tw, tZ, I(n32), I(info),
                                          sec.ctypes.data_as(_dp))
            assert rc == 0 and not info.any()
            return float(sec[0])

        def per_order():
            dev.put(dA, hA); dev.put(dB, hB)
            t = 0.0
            for g, n in enumerate(distinct):
                n, f, c = int(n), g * 16, max(1, int(n) // 8)
                rc = lib.ek_hip_eigenpairs_window_xbatched_device(
                    1, 1, 0, n, 16, ctypes.c_double(0.0), ctypes.c_double(0.0), 1, c, at(dA, offm[f]), n, n * n,
                    at(dB, offm[f]), n, n * n, I(m), at(dw, offw[f]), at(dZ, offm[f]), n, c, n * n, I(info),
                    sec.ctypes.data_as(_dp))
                assert rc == 0 and not info[:16].any()
                t += float(sec[0])
            return t

        tw_, tf_, tg_ = [], [], []
        window(); full(); per_order()                   # warm-up
        for _ in range(3):
            tw_.append(window()); tf_.append(full()); tg_.append(per_order())
    return min(tw_), min(tf_), min(tg_)


@pytest.mark.parametrize("lo,hi,full_entry,gate", [(8, 256, "ek_hip_eigenpairs_xvbatched_device", 0.75),
                                                    (8, 128, "ek_hip_eigenpairs_vbatched_device", 0.6)])
def test_a_variable_window_costs_what_it_should(hip, lo, hi, full_entry, gate):
    """512 generalized problems, the lowest max(1, n / 8) pairs with vectors: at most `gate` of the full variable call (0.75
    over 8 .. 256, DESIGN.md 32's gate; 0.6 over 8 .. 128, DESIGN.md 30's) and less than a uniform window call per distinct
    order.  Measured on one MI355X: 8 .. 256: 12.81 ms against 35.92 ms (0.357) and 134.05 ms per order;
    8 .. 128: 2.56 ms against 7.69 ms (0.333) and 38.62 ms."""
    lib = hip.load_library()
    t_win, t_full, t_order = _cost(lib, lo, hi, full_entry)
    print("512 problems of order %d..%d: variable window %.3f ms, full variable call %.3f ms (ratio %.3f, gate %.2f), "
          "uniform window call per order %.3f ms (ratio %.2f)"
          % (lo, hi, t_win * 1e3, t_full * 1e3, t_win / t_full, gate, t_order * 1e3, t_order / t_win))
    assert t_win <= gate * t_full, (t_win, t_full)
    assert t_win < t_order, (t_win, t_order)
