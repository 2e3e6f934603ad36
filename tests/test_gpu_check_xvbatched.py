"""GPU suite of the variable-order acceptance checks for orders up to 256 (ek_hip_check_xvbatched*,
ek_hip_check_sygv_xvbatched*): residual, orthogonality and IPRs of problems of DIFFERENT orders in one call, a problem
above 128 in the kernel of ek_hip_check_*xbatched* reading its problem from the table, every other one in the class
ek_hip_check_*vbatched* give it.

The oracle of the contract needs no tolerance: a problem's four words and IPRs are the bits the uniform entry
(ek_hip_check_xbatched_device / ek_hip_check_sygv_xbatched_device) returns for it alone.  The generators are those of
tests/test_gpu_check_xbatched.py, copied: symmetric A, SPD B of cond 10, (w, Z) from SciPy, Z perturbed by
1e-3 N(0, 1) / sqrt(n) so that the quantities stand above rounding noise.  ORDERS is the list of tests/test_gpu_xvbatched.py:
both sides of every class limit, 130 (even), 193 (a K tail that is no multiple of 16), 192 / 256 (the tile edges), twice
each in a seeded shuffle.  Against the host mirror eigenkernel_amd/verifier.py the bound is the project's 4 max(n, 8) eps
(times cond_2(B) for slot 3 and the IPRs of type 3), as in the uniform suites.  The tests print what they measured
(pytest -s shows it).

Measured on one MI355X: the largest share of the mirror's bound 0.044 (an IPR of problem 1; 0.012 for a
residual slot, 0.0005 for orthogonality); behind the solver res_max at most 0.004 of 64 n eps and orthogonality at most
0.005 of 256 n eps; cost, 128 generalized problems of 16 orders 129 .. 256: one variable call 1.294 ms of wall time
(1.240 ms on the device) against 11.628 ms for the 16 uniform calls (0.111 of it), and against 34.556 ms of device time
for the solve (0.036 of it)."""
import ctypes
import functools
import time

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import verifier

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (0, 1, 32, 33, 64, 65, 128, 129, 130, 192, 193, 255, 256)
SENTINEL = -7.25e77
NAMES = ("norm", "res_ave", "res_max", "orthogonality", "ipr")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
# (sygv family?, first argument): problems 0 and 1 of ek_hip_check_xvbatched*, types 2 and 3 of ek_hip_check_sygv_xvbatched*
KINDS = [(False, 0), (False, 1), (True, 2), (True, 3)]
kinds = pytest.mark.parametrize("sygv,first", KINDS, ids=["problem0", "problem1", "itype2", "itype3"])
forms = pytest.mark.parametrize("form", ["device", "host"])


# --------------------------------------------------------------------- generators of tests/test_gpu_check_xbatched.py
def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


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
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _pencils(seed, orders):
    """One seeded (A, B) per order.  Read only."""
    rng = np.random.default_rng(seed)
    pairs = []
    for n in orders:
        A, B = _sym(rng, n), _spd(rng, n)
        A.setflags(write=False)
        B.setflags(write=False)
        pairs.append((A, B))
    return pairs


@functools.lru_cache(maxsize=None)
def _problems(seed, orders, first):
    """The pencils with SciPy's (w, Z) for the kind (first = 0 the standard problem, 1 .. 3 DSYGV's types), Z perturbed, and
    cond_2(B).  Problem i carries key = (seed, i, first) for the caches of the uniform call.  Read only."""
    rng = np.random.default_rng(99000 + 7 * seed + first)
    probs = []
    for i, (A, B) in enumerate(_pencils(seed, orders)):
        n = A.shape[0]
        p = _Out()
        p.n, p.A, p.B, p.key = n, A, B, (seed, i, first)
        if n:
            p.w, p.Z = sl.eigh(A, B, type=first, lower=True) if first else sl.eigh(A, lower=True)
            p.cond = float(np.linalg.cond(B))
            assert p.cond <= 16.0
        else:
            p.w, p.Z, p.cond = np.zeros(0), np.zeros((0, 0)), 1.0
        p.Zp = p.Z + 1e-3 * rng.standard_normal(p.Z.shape) / np.sqrt(max(n, 1))
        for a in (p.w, p.Z, p.Zp):
            a.setflags(write=False)
        probs.append(p)
    return probs


def _the_batch(first):
    """Every order of ORDERS twice, and two seeded shuffles of the 26 problems."""
    probs = _problems(21, ORDERS * 2, first)
    p1 = np.random.default_rng(211).permutation(len(probs))
    p2 = np.random.default_rng(212).permutation(len(probs))
    return probs, p1, p2


# ------------------------------------------------------------------------------------------------------- the calls
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

    def fill(self, mats, fill, upper=None):
        flat = np.full(max(int(self.off[-1]), 1), fill)
        for b, M in enumerate(mats):
            if M.shape[0]:
                M = np.array(M)
                if upper is not None:
                    M[np.triu_indices(M.shape[0], 1)] = upper
                self.block(flat, b)[...] = M.T
        return flat

    def wfill(self, vecs, fill):
        flat = np.full(max(int(self.woff[-1]), 1), fill)
        for b, v in enumerate(vecs):
            flat[self.woff[b]:self.woff[b] + len(v)] = v
        return flat

    def pointers(self, base, off):
        """NULL for a problem of order 0."""
        return (ctypes.c_void_p * self.batch)(*[base + int(off[b]) * 8 if self.orders[b] else None
                                                for b in range(self.batch)])


def _var(lib, form, sygv, first, probs, info=None, want=None, pad=0, nan=False, stem="xvbatched", Zs=None, ws=None,
         Bs=None, timed=True):
    """The variable entry of the kind on the problems, every problem in its own region of one buffer per array kind.
    pad > 0: leading dimensions max(n, 1) + pad and gaps between the problems; nan: NaN in the padding, the gaps and the
    strictly upper triangles of A and B (the sentinel otherwise, the triangles as given).  want: None every IPR, False
    ipr = NULL, or a list of booleans (False: a NULL entry).  Zs, ws, Bs replace the problems' own arrays.
    o.untouched: the buffers of A, B, w and Z after the call equal those before it, bit for bit."""
    withB = sygv or first == 1
    fill = np.nan if nan else SENTINEL
    pl = _Place([p.n for p in probs], pad)
    h = [pl.fill([p.A for p in probs], fill, np.nan if nan else None),
         pl.fill([p.B for p in probs] if Bs is None else Bs, fill, np.nan if nan else None) if withB else None,
         pl.wfill([p.w for p in probs] if ws is None else ws, fill),
         pl.fill([p.Zp for p in probs] if Zs is None else Zs, fill)]
    batch = pl.batch
    out = np.full(batch * 4 + 2, SENTINEL)
    qs = [np.full(p.n + 1, SENTINEL) for p in probs]
    if want is False:
        qtab = None
    else:
        flags = [True] * batch if want is None else want
        qtab = (ctypes.c_void_p * batch)(*[q.ctypes.data if f else None for q, f in zip(qs, flags)])
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    sec = ctypes.c_double(-1.0)
    ld = pl.ld.ctypes.data_as(_ip)
    name = ("ek_hip_check_sygv_" if sygv else "ek_hip_check_") + stem + ("_device" if form == "device" else "")
    fn = getattr(lib, name)
    o = _Out()

    def run(bA, bB, bw, bZ):
        return fn(first, batch, pl.n32.ctypes.data_as(_ip), pl.pointers(bA, pl.off), ld,
                  pl.pointers(bB, pl.off) if withB else None, ld, pl.pointers(bw, pl.woff), pl.pointers(bZ, pl.off), ld,
                  None if iarr is None else iarr.ctypes.data_as(_ip), out.ctypes.data_as(_dp), qtab,
                  ctypes.byref(sec) if timed else None)

    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) if x is not None else None for x in h]
            o.rc = run(d[0].value, d[1].value if withB else 0, d[2].value, d[3].value)
            o.untouched = all(x is None or _same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [None if x is None else x.copy() for x in h]
        o.rc = run(g[0].ctypes.data, g[1].ctypes.data if withB else 0, g[2].ctypes.data, g[3].ctypes.data)
        o.untouched = all(x is None or _same(y, x) for y, x in zip(g, h))
    o.seconds = sec.value
    o.out = out[:batch * 4].reshape(batch, 4)
    o.ipr = [q[:-1] for q in qs]
    assert np.all(out[batch * 4:] == SENTINEL) and all(q[-1] == SENTINEL for q in qs)   # nothing behind out and the rows
    if iarr is not None:
        assert np.array_equal(iarr, np.asarray(info, dtype=np.int32))
    return o


def _clean(o):
    assert o.rc == 0 and o.untouched and o.seconds >= 0.0, (o.rc, o.untouched, o.seconds)


_alone_cache = {}


def _alone(lib, sygv, first, p, Z=None, B=None):
    """The uniform entry for orders up to 256 (device form, compact layout) on one problem alone: (out[4], ipr[n]).  With
    the problem's own arrays the answer is computed once."""
    key = (p.key, sygv, first) if Z is None and B is None else None
    if key is not None and key in _alone_cache:
        return _alone_cache[key]
    n = p.n
    assert n > 0
    withB = sygv or first == 1
    out, q = np.full(4, SENTINEL), np.full(n, SENTINEL)
    fn = lib.ek_hip_check_sygv_xbatched_device if sygv else lib.ek_hip_check_xbatched_device
    with _Dev(lib) as dev:
        dA = dev.up(np.asfortranarray(p.A).ravel(order="F"))
        dB = dev.up(np.asfortranarray(p.B if B is None else B).ravel(order="F")) if withB else None
        dw = dev.up(np.ascontiguousarray(p.w))
        dZ = dev.up(np.asfortranarray(p.Zp if Z is None else Z).ravel(order="F"))
        rc = fn(first, n, 1, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n, None, out.ctypes.data_as(_dp),
                q.ctypes.data_as(_dp), None)
    assert rc == 0
    out.setflags(write=False)
    q.setflags(write=False)
    if key is not None:
        _alone_cache[key] = (out, q)
    return out, q


def _empty(row):
    """The four words of a problem of order 0: a_norm = 0 and three NaN."""
    return row[0] == 0.0 and np.all(np.isnan(row[1:]))


def _assert_alone(lib, sygv, first, probs, o, what, skip=()):
    for b, p in enumerate(probs):
        if b in skip:
            continue
        if p.n == 0:
            assert _empty(o.out[b]), (what, b)
            continue
        ref_out, ref_ipr = _alone(lib, sygv, first, p)
        assert _same(o.out[b], ref_out), (what, b, p.n, o.out[b], ref_out)
        assert _same(o.ipr[b], ref_ipr), (what, b, p.n)


def _last(lib):
    sec, cnt = np.zeros(4), np.zeros(4, dtype=np.int32)
    assert lib.ek_hip_debug_check_xvbatched_last(sec.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip)) == 0
    return sec, cnt


# ------------------------------------------------------------------------------ 1: bit identity with the uniform call
@forms
@kinds
def test_bit_identity_with_the_uniform_call(hip, sygv, first, form):
    """Every problem's four words and IPRs are those of the uniform entry on the problem alone; a second permutation with
    padded leading dimensions, gaps, and NaN in the padding and above the diagonals gives the same bits and no NaN."""
    lib = hip.load_library()
    probs, p1, p2 = _the_batch(first)
    batch = [probs[i] for i in p1]
    o = _var(lib, form, sygv, first, batch)
    _clean(o)
    _assert_alone(lib, sygv, first, batch, o, (sygv, first, form))
    sec, cnt = _last(lib)
    assert list(cnt) == [12, 4, 4, 4] and np.all(sec > 0.0) and o.seconds > 0.0, (cnt, sec)
    batch2 = [probs[i] for i in p2]
    o2 = _var(lib, form, sygv, first, batch2, pad=3, nan=True)
    _clean(o2)
    _assert_alone(lib, sygv, first, batch2, o2, (sygv, first, form, "padded"))
    for b, p in enumerate(batch2):
        if p.n:
            assert not np.isnan(o2.out[b]).any() and not np.isnan(o2.ipr[b]).any(), (b, p.n)


# ---------------------------------------------------------------------------------------- 2: without a large order
@kinds
def test_without_a_large_order_it_is_the_vbatched_call(hip, sygv, first):
    """Orders up to 128 only: the bits of ek_hip_check_vbatched_device / ek_hip_check_sygv_vbatched_device, and no problem
    in the class of 256."""
    lib = hip.load_library()
    probs, p1, _ = _the_batch(first)
    batch = [probs[i] for i in p1 if probs[i].n <= 128]
    assert len(batch) == 14
    old = _var(lib, "device", sygv, first, batch, stem="vbatched")
    new = _var(lib, "device", sygv, first, batch)
    _clean(old)
    _clean(new)
    assert _same(new.out[:, 0], old.out[:, 0])
    for b, p in enumerate(batch):
        assert _same(new.out[b], old.out[b]) and _same(new.ipr[b], old.ipr[b]), (b, p.n)
    sec, cnt = _last(lib)
    assert list(cnt) == [0, 4, 4, 4] and sec[0] == 0.0 and np.all(sec[1:] > 0.0), (cnt, sec)


# ------------------------------------------------------------------------------------------------ 3: type 1 identities
@forms
def test_type_1_identities_and_the_python_mirror(hip, form):
    lib = hip.load_library()
    probs, p1, _ = _the_batch(1)
    batch = [probs[i] for i in p1]
    e = _var(lib, form, False, 1, batch)
    s = _var(lib, form, True, 1, batch)
    _clean(e)
    _clean(s)
    for b in range(len(batch)):
        assert _same(s.out[b], e.out[b]) and _same(s.ipr[b], e.ipr[b]), b
    # type 2 on the same (B, Z): slot 3 and the IPRs are type 1's bits
    t2 = _var(lib, form, True, 2, batch)
    _clean(t2)
    for b, p in enumerate(batch):
        if p.n:
            assert _same(t2.out[b, 3], e.out[b, 3]) and _same(t2.ipr[b], e.ipr[b]), (b, p.n)
    if form == "host":
        As, Bs, ws, Zs = ([getattr(p, k) for p in batch] for k in ("A", "B", "w", "Zp"))
        secs = np.zeros(1)
        out, q = hip.check_xvbatched(As, Bs, ws, Zs, seconds=secs)
        assert secs[0] > 0.0 and list(hip.check_xvbatched_last()[1]) == [12, 4, 4, 4]
        out1, q1 = hip.check_sygv_xvbatched(As, Bs, ws, Zs, itype=1)
        out2, q2 = hip.check_sygv_xvbatched(As, Bs, ws, Zs, itype=2)
        for b, p in enumerate(batch):
            assert _same(out[b], e.out[b]) and _same(q[b], e.ipr[b]), b
            assert _same(out1[b], e.out[b]) and _same(q1[b], e.ipr[b]), b
            assert _same(out2[b], t2.out[b]) and _same(q2[b], t2.ipr[b]), b
        p0 = _the_batch(0)[0]
        b0 = [p0[i] for i in p1]
        out0, q0 = hip.check_xvbatched([p.A for p in b0], None, [p.w for p in b0], [p.Zp for p in b0])
        o0 = _var(lib, "device", False, 0, b0)
        for b in range(len(b0)):
            assert _same(out0[b], o0.out[b]) and _same(q0[b], o0.ipr[b]), b


# ------------------------------------------------------------------------------------------ 4: against the host mirror
def _tol(n):
    return 4 * max(n, 8) * EPS


def _mirror(sygv, first, p):
    if sygv:
        norm, ave, mx = verifier.eval_residual_norm_sygv(first, p.A, p.B, p.w, p.Zp)
        return (np.array([norm, ave, mx, verifier.eval_orthogonality_sygv(first, p.Zp, p.B)]),
                verifier.get_ipratios_sygv(first, p.Zp, p.B))
    B = p.B if first else None
    a_norm, ave, mx = verifier.eval_residual_norm(p.A, p.w, p.Zp, B)
    return np.array([a_norm, ave, mx, verifier.eval_orthogonality(p.Zp, B)]), verifier.get_ipratios(p.Zp, B)


def _shares(itype3, out, ipr, ref_out, ref_ipr, n, cond):
    """|difference| / bound per quantity: out[0] and the IPRs relative, the other three absolute; slot 3 and the IPRs of
    type 3 with max(1, cond_2(B)) in the bound (tests/test_gpu_check_sygv_xbatched.py).  NaN against a number uses
    everything."""
    tol = _tol(n)
    wide = tol * (max(1.0, cond) if itype3 else 1.0)

    def share(x, y, bound):
        with np.errstate(invalid="ignore"):
            s = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)) / bound
        return float(np.where(np.isnan(s), np.inf, s).max())

    return np.array([share(out[0], ref_out[0], tol * abs(ref_out[0])), share(out[1], ref_out[1], tol),
                     share(out[2], ref_out[2], tol), share(out[3], ref_out[3], wide),
                     share(ipr, ref_ipr, wide * np.abs(ref_ipr))])


@kinds
def test_matches_the_host_mirror(hip, sygv, first):
    lib = hip.load_library()
    probs, p1, _ = _the_batch(first)
    batch = [probs[i] for i in p1]
    o = _var(lib, "device", sygv, first, batch, pad=2)
    _clean(o)
    shares = []
    for b, p in enumerate(batch):
        if p.n == 0:
            continue
        ref_out, ref_ipr = _mirror(sygv, first, p)
        if p.n >= 32:                                   # the perturbation shows: a hundred times the bound, not rounding noise
            assert 100 * _tol(p.n) < o.out[b, 1] and 100 * _tol(p.n) < o.out[b, 3], (b, p.n, o.out[b])
        shares.append(_shares(sygv and first == 3, o.out[b], o.ipr[b], ref_out, ref_ipr, p.n, p.cond))
    shares = np.asarray(shares).max(axis=0)
    print("shares of the bounds %s: " % ((sygv, first),) + ", ".join("%s %.4f" % kv for kv in zip(NAMES, shares)))
    assert np.all(shares <= 1.0), shares


# ---------------------------------------------------------------------------------------------------- 5: the chunk seam
@pytest.mark.parametrize("sygv,first", [(False, 1), (True, 3)], ids=["problem1", "itype3"])
def test_same_bits_in_any_chunk(hip, sygv, first):
    """Orders (256, 255, 193, 130, 129) in chunks of 2 and of 1: the default's bits (type 3: 2 n^2 of scratch an entry)."""
    lib = hip.load_library()
    probs = _problems(33, (256, 255, 193, 130, 129), first)
    ref = _var(lib, "device", sygv, first, probs)
    _clean(ref)
    _assert_alone(lib, sygv, first, probs, ref, "default chunk")
    try:
        for chunk in (2, 1):
            hip.check_xbatched_chunk(chunk)
            for form in ("device", "host"):
                o = _var(lib, form, sygv, first, probs)
                _clean(o)
                for b in range(len(probs)):
                    assert _same(o.out[b], ref.out[b]) and _same(o.ipr[b], ref.ipr[b]), (chunk, form, b)
                assert _last(lib)[1][0] == 5
            info = [0, 0, 6, 0, 0]
            o = _var(lib, "device", sygv, first, probs, info=info)
            _clean(o)
            assert np.all(np.isnan(o.out[2])) and np.all(o.ipr[2] == SENTINEL) and _last(lib)[1][0] == 4
            for b in (0, 1, 3, 4):
                assert _same(o.out[b], ref.out[b]) and _same(o.ipr[b], ref.ipr[b]), (chunk, "skipped", b)
    finally:
        hip.check_xbatched_chunk(0)


# ------------------------------------------------------------------------------------------ 6: skipped, empty, poisoned
@forms
@pytest.mark.parametrize("sygv,first", [(False, 0), (False, 1), (True, 3)], ids=["problem0", "problem1", "itype3"])
def test_skipped_empty_and_poisoned(hip, sygv, first, form):
    lib = hip.load_library()
    probs = _problems(44, (200, 40, 0, 129, 64, 256, 33), first)
    ref = _var(lib, "device", sygv, first, probs)
    _clean(ref)
    _assert_alone(lib, sygv, first, probs, ref, "plain")
    # a large and a small problem skipped, their w and Z full of NaN; a NULL entry in ipr
    Zs = [np.array(p.Zp) for p in probs]
    ws = [np.array(p.w) for p in probs]
    for b in (0, 4):
        Zs[b][...] = np.nan
        ws[b][...] = np.nan
    info = [9, 0, 0, 0, -5, 0, 0]
    want = [True, True, True, False, True, True, True]
    o = _var(lib, form, sygv, first, probs, info=info, want=want, Zs=Zs, ws=ws)
    _clean(o)
    for b in (0, 4):
        assert np.all(np.isnan(o.out[b])) and np.all(o.ipr[b] == SENTINEL), b
    assert _empty(o.out[2])
    assert _same(o.out[3], ref.out[3]) and np.all(o.ipr[3] == SENTINEL)      # not wanted: the row is left alone
    for b in (1, 5, 6):
        assert _same(o.out[b], ref.out[b]) and _same(o.ipr[b], ref.ipr[b]), b
    assert list(_last(lib)[1]) == [2, 0, 2, 0]
    # ipr = NULL
    o = _var(lib, form, sygv, first, probs, want=False)
    _clean(o)
    assert all(np.all(q == SENTINEL) for q in o.ipr)
    for b in (0, 1, 3, 4, 5, 6):
        assert _same(o.out[b], ref.out[b]), b
    # one NaN in Z of a large problem and of a small one, info = 0: their own slots only
    Zs = [np.array(p.Zp) for p in probs]
    Zs[3][70, 40] = np.nan
    Zs[1][7, 5] = np.nan
    o = _var(lib, form, sygv, first, probs, info=[0] * 7, Zs=Zs)
    _clean(o)
    assert not np.isfinite(o.out[3, 1:]).any() and np.isnan(o.ipr[3][40])
    assert not np.isfinite(o.out[1, 1:]).any() and np.isnan(o.ipr[1][5])
    for b in (0, 4, 5, 6):
        assert _same(o.out[b], ref.out[b]) and _same(o.ipr[b], ref.ipr[b]), b
    if first == 3:
        # B of a large problem not SPD (a negative pivot at column 3): NaN in slot 3 and the IPRs, the residual slots stand
        Bs = [np.array(p.B) for p in probs]
        Bs[5][3, 3] = -1.0
        o = _var(lib, form, sygv, first, probs, Bs=Bs)
        _clean(o)
        alone_out, alone_ipr = _alone(lib, sygv, first, probs[5], B=Bs[5])
        assert np.isnan(o.out[5, 3]) and np.all(np.isnan(o.ipr[5])) and np.all(np.isfinite(o.out[5, :3]))
        assert _same(o.out[5], alone_out) and _same(o.ipr[5], alone_ipr)
        for b in (0, 1, 3, 4, 6):
            assert _same(o.out[b], ref.out[b]) and _same(o.ipr[b], ref.ipr[b]), b


# ------------------------------------------------------------------- 7: more workgroups than one chunk and one round
def test_more_problems_than_a_chunk_and_a_round(hip):
    """600 + 8 problems of order 129 by pointer arrays that reuse 8 distinct pencils, 256 a launch: every one has its
    pencil's bits."""
    lib = hip.load_library()
    n, distinct, batch = 129, 8, 608
    probs = _problems(55, (n,) * distinct, 1)
    ref = [_alone(lib, False, 1, p) for p in probs]
    idx = np.random.default_rng(5).integers(0, distinct, batch)
    idx[:distinct] = np.arange(distinct)
    out = np.full(batch * 4, SENTINEL)
    q = np.full((batch, n), SENTINEL)
    sec = ctypes.c_double(-1.0)
    n32 = np.full(batch, n, dtype=np.int32)
    try:
        hip.check_xbatched_chunk(256)
        with _Dev(lib) as dev:
            d = {k: [dev.up(np.asfortranarray(getattr(p, k)).ravel(order="F")) for p in probs]
                 for k in ("A", "B", "w", "Zp")}

            def tab(k):
                return (ctypes.c_void_p * batch)(*[d[k][i].value for i in idx])

            qtab = (ctypes.c_void_p * batch)(*[q[b].ctypes.data for b in range(batch)])
            ni = n32.ctypes.data_as(_ip)
            rc = lib.ek_hip_check_xvbatched_device(1, batch, ni, tab("A"), ni, tab("B"), ni, tab("w"), tab("Zp"), ni, None,
                                                   out.ctypes.data_as(_dp), qtab, ctypes.byref(sec))
    finally:
        hip.check_xbatched_chunk(0)
    assert rc == 0 and sec.value > 0.0
    assert list(_last(lib)[1]) == [608, 0, 0, 0]
    out = out.reshape(batch, 4)
    for b, i in enumerate(idx):
        assert _same(out[b], ref[i][0]) and _same(q[b], ref[i][1]), (b, i)


# ------------------------------------------------------------------------------------------------- 8: behind the solver
@pytest.mark.parametrize("sygv,first", [(False, 1), (True, 3)], ids=["problem1", "itype3"])
def test_behind_the_xvbatched_solver(hip, sygv, first):
    """The solver's own w, Z and info on the shuffled batch (it overwrites its A and B: the check gets the originals):
    the suite's bounds on res_max (64 n eps) and orthogonality (256 n eps), per problem."""
    lib = hip.load_library()
    probs, p1, _ = _the_batch(first)
    batch = [probs[i] for i in p1]
    pl = _Place([p.n for p in batch], 0)
    hA, hB = pl.fill([p.A for p in batch], SENTINEL), pl.fill([p.B for p in batch], SENTINEL)
    nb = pl.batch
    info = np.full(nb, 777, dtype=np.int32)
    out = np.full(nb * 4, SENTINEL)
    qs = [np.full(p.n, SENTINEL) for p in batch]
    qtab = (ctypes.c_void_p * nb)(*[x.ctypes.data if x.size else None for x in qs])
    ni, ld = pl.n32.ctypes.data_as(_ip), pl.ld.ctypes.data_as(_ip)
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw = dev.up(np.zeros(max(int(pl.woff[-1]), 1)))
        dZ = dev.up(np.zeros(max(int(pl.off[-1]), 1)))
        solve = lib.ek_hip_sygv_xvbatched_device if sygv else lib.ek_hip_eigenpairs_xvbatched_device
        assert solve(first, 1, nb, ni, pl.pointers(dA.value, pl.off), ld, pl.pointers(dB.value, pl.off), ld,
                     pl.pointers(dw.value, pl.woff), pl.pointers(dZ.value, pl.off), ld, info.ctypes.data_as(_ip), None) == 0
        assert not info.any()
        check = lib.ek_hip_check_sygv_xvbatched_device if sygv else lib.ek_hip_check_xvbatched_device
        assert check(first, nb, ni, pl.pointers(dA0.value, pl.off), ld, pl.pointers(dB0.value, pl.off), ld,
                     pl.pointers(dw.value, pl.woff), pl.pointers(dZ.value, pl.off), ld, info.ctypes.data_as(_ip),
                     out.ctypes.data_as(_dp), qtab, None) == 0
    out = out.reshape(nb, 4)
    worst = [0.0, 0.0]
    for b, p in enumerate(batch):
        if p.n == 0:
            assert _empty(out[b])
            continue
        worst = [max(worst[0], out[b, 2] / (64 * p.n * EPS)), max(worst[1], out[b, 3] / (256 * p.n * EPS))]
        assert out[b, 2] <= 64 * p.n * EPS, (b, p.n, out[b, 2])
        assert out[b, 1] <= out[b, 2]
        assert out[b, 3] <= 256 * p.n * EPS, (b, p.n, out[b, 3])
        assert np.all(np.isfinite(qs[b])) and np.all(qs[b] > 0.0)
    print("behind the solver %s: res_max %.3f of 64 n eps, orthogonality %.3f of 256 n eps" % ((sygv, first), *worst))


# ----------------------------------------------------------------------------------------------------------- 9: one pool
def test_one_pool_behind_all_entries(hip):
    """ek_hip_check_batched (n = 40), the variable call (orders 0, 33, 129, 256, type 3, chunk 1), ek_hip_check_xbatched
    (n = 130), the variable call again: the second round's bits are the first's (a table where a map was, and back)."""
    lib = hip.load_library()
    probs = _problems(66, (0, 33, 129, 256), 3)
    p40 = _problems(67, (40, 40, 40), 1)
    p130 = _problems(68, (130, 130), 1)

    def stack(ps, k):
        return np.stack([getattr(p, k) for p in ps])

    try:
        hip.check_xbatched_chunk(1)
        out40, q40 = hip.check_batched(stack(p40, "A"), stack(p40, "B"), stack(p40, "w"), stack(p40, "Zp"), info=[0, 3, 0])
        assert np.all(np.isnan(out40[1])) and np.all(np.isfinite(out40[[0, 2]]))
        first_round = _var(lib, "host", True, 3, probs)
        _clean(first_round)
        _assert_alone(lib, True, 3, probs, first_round, "first round")
        out130, q130 = hip.check_xbatched(stack(p130, "A"), stack(p130, "B"), stack(p130, "w"), stack(p130, "Zp"),
                                          info=[2, 0])
        assert np.all(np.isnan(out130[0])) and np.all(np.isfinite(out130[1]))
        ref130 = _alone(lib, False, 1, p130[1])
        assert _same(out130[1], ref130[0]) and _same(q130[1], ref130[1])
        second = _var(lib, "host", True, 3, probs)
        _clean(second)
    finally:
        hip.check_xbatched_chunk(0)
    for b in range(len(probs)):
        assert _same(second.out[b], first_round.out[b]) and _same(second.ipr[b], first_round.ipr[b]), b


# --------------------------------------------------------------------------------------------------------------- 10: cost
def test_cost_against_the_grouped_calls_and_the_solve(hip):
    """128 generalized problems, 8 at each of 16 orders spread over 129 .. 256 (both ends), IPRs wanted, device-resident;
    best of 3 after a warm-up, the kinds alternated.  One variable call takes no more wall time than the 16 uniform
    ek_hip_check_xbatched_device calls a caller makes today, and no more device time than ek_hip_eigenpairs_xvbatched_device
    on the same batch."""
    lib = hip.load_library()
    orders16 = tuple(int(round(x)) for x in np.linspace(129, 256, 16))
    assert orders16[0] == 129 and orders16[-1] == 256 and len(set(orders16)) == 16
    pencils = _pencils(77, orders16)
    per = 8
    # problem (k, r): copy r of pencil k; in the variable batch they are interleaved (r outer), in the grouped calls stacked
    nb = 16 * per
    order_of = [orders16[b % 16] for b in range(nb)]
    pl = _Place(order_of, 0)
    hA, hB = (pl.fill([pencils[b % 16][k] for b in range(nb)], SENTINEL) for k in (0, 1))
    info = np.zeros(nb, dtype=np.int32)
    out = np.zeros(nb * 4)
    qs = [np.zeros(n) for n in order_of]
    qtab = (ctypes.c_void_p * nb)(*[x.ctypes.data for x in qs])
    ni, ld = pl.n32.ctypes.data_as(_ip), pl.ld.ctypes.data_as(_ip)
    t_solve, t_var, w_var, w_grouped = [], [], [], []
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw = dev.up(np.zeros(int(pl.woff[-1])))
        dZ = dev.up(np.zeros(int(pl.off[-1])))
        # the grouped caller's arrays: per order a strided stack of its 8 problems, filled from the solver's results below
        gA = [dev.up(np.concatenate([np.asfortranarray(pencils[k][0]).ravel(order="F")] * per)) for k in range(16)]
        gB = [dev.up(np.concatenate([np.asfortranarray(pencils[k][1]).ravel(order="F")] * per)) for k in range(16)]
        gw = [dev.up(np.zeros(per * orders16[k])) for k in range(16)]
        gZ = [dev.up(np.zeros(per * orders16[k] ** 2)) for k in range(16)]
        gout = [np.zeros(per * 4) for _ in range(16)]
        gq = [np.zeros(per * orders16[k]) for k in range(16)]
        tabs = (pl.pointers(dA.value, pl.off), pl.pointers(dB.value, pl.off), pl.pointers(dw.value, pl.woff),
                pl.pointers(dZ.value, pl.off), pl.pointers(dA0.value, pl.off), pl.pointers(dB0.value, pl.off))
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_eigenpairs_xvbatched_device(1, 1, nb, ni, tabs[0], ld, tabs[1], ld, tabs[2], tabs[3], ld,
                                                          info.ctypes.data_as(_ip), ctypes.byref(sec)) == 0
            assert not info.any()
            t_solve.append(sec.value)
            if it == 0:                                 # the grouped arrays get the solver's w and Z, once
                hw, hZ = dev.down(dw, np.zeros(int(pl.woff[-1]))), dev.down(dZ, np.zeros(int(pl.off[-1])))
                for k in range(16):
                    n = orders16[k]
                    mine = [b for b in range(nb) if b % 16 == k]
                    dev.put(gw[k], np.concatenate([hw[pl.woff[b]:pl.woff[b] + n] for b in mine]))
                    dev.put(gZ[k], np.concatenate([hZ[pl.off[b]:pl.off[b] + n * n] for b in mine]))
            sec = ctypes.c_double(-1.0)
            t0 = time.perf_counter()
            assert lib.ek_hip_check_xvbatched_device(1, nb, ni, tabs[4], ld, tabs[5], ld, tabs[2], tabs[3], ld,
                                                     info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), qtab,
                                                     ctypes.byref(sec)) == 0
            w_var.append(time.perf_counter() - t0)
            t_var.append(sec.value)
            t0 = time.perf_counter()
            for k in range(16):
                n = orders16[k]
                assert lib.ek_hip_check_xbatched_device(1, n, per, gA[k], n, n * n, gB[k], n, n * n, gw[k], gZ[k], n, n * n,
                                                        None, gout[k].ctypes.data_as(_dp), gq[k].ctypes.data_as(_dp),
                                                        None) == 0
            w_grouped.append(time.perf_counter() - t0)
    o = out.reshape(nb, 4)
    for b in range(nb):                                 # the same problems both ways: the same bits
        k, r, n = b % 16, b // 16, order_of[b]
        assert _same(o[b], gout[k].reshape(per, 4)[r]) and _same(qs[b], gq[k].reshape(per, n)[r]), b
        assert o[b, 2] <= 64 * n * EPS and o[b, 3] <= 256 * n * EPS
    ts, tv = min(t_solve[1:]), min(t_var[1:])
    wv, wg = min(w_var[1:]), min(w_grouped[1:])
    print("cost, 128 problems of 16 orders 129 .. 256: variable check %.3f ms wall (%.3f ms device), 16 uniform calls "
          "%.3f ms wall, variable / grouped %.3f; solve %.3f ms device, check / solve %.3f"
          % (wv * 1e3, tv * 1e3, wg * 1e3, wv / wg, ts * 1e3, tv / ts))
    assert wv <= wg, (wv, wg)
    assert 0.0 < tv <= ts, (tv, ts)
