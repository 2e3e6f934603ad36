"""GPU suite of the batched acceptance checks of DSYGV's types 2 (A B x = l x) and 3 (B A x = l x) for orders 129 .. 256
(ek_hip_check_sygv_xbatched*): ||A||_F ||B||_F, res_ave, res_max, orthogonality and the inverse participation ratios of
every problem of a batch, a workgroup per problem, the products on the fp64 matrix cores.

The yardstick is the host mirror eigenkernel_amd/verifier.py (*_sygv) in float64, on the seeded _sym / _spd (cond 10)
inputs _pairs(1000 + n, 4, n) (helpers copied from tests/test_gpu_check_xbatched.py), (w, Z) from
scipy.linalg.eigh(A, B, type=itype, lower=True) and Zp = Z + 1e-3 N(0, 1) / sqrt(n).  The tolerance is the project's
4 max(n, 8) eps -- relative for out[0] and every IPR, absolute for out[1 .. 3] -- multiplied by max(1, cond_2(B)) for
out[3] and the IPRs of type 3 (two exact factors of B lie cond(B) eps apart); cond_2(B) <= 16 is asserted on the CPU.
On the CPU, with these generators at n = 129, 192 and 256, both types, Z and Zp, the mirror uses at most 0.019 of any of
these bounds against a long-double evaluation and against a float64 one with LAPACK's blocked factor and
solve_triangular (an IPR of type 2, relative; <= 0.002 for type 3's slot 3 and IPRs, <= 0.013 for type 2's orthogonality).
Unless it says otherwise a test runs in four ways: types 2 and 3, device and host form.  Each test prints the largest
share of each bound it used (pytest -s shows it).

Largest shares used on one MI355X: against the mirror 0.019 (an IPR of type 2) and 0.002 (type 3), norm
0.002, the residual slots and orthogonality at most 0.0004; 256 pencils: check / solve 0.056 and 0.148 at n = 129, 0.037 and
0.176 at n = 256 for types 2 and 3, the host loop over the one-problem check 11 to 60 times the batched check."""
import ctypes
import functools
import time

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import verifier

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (129, 130, 160, 191, 192, 193, 255, 256)   # first, even, K tail not a multiple of 4, the 64 / 128 tile edges, last
COUNT = 4
SENTINEL = -7.25e77
NAMES = ("norm", "res_ave", "res_max", "orthogonality", "ipr")
NEW = "ek_hip_check_sygv_xbatched"
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
WAYS = [(2, "device"), (2, "host"), (3, "device"), (3, "host")]
ways = pytest.mark.parametrize("itype,form", WAYS)
forms = pytest.mark.parametrize("form", ["device", "host"])


# --------------------------------------------------------------------- helpers of tests/test_gpu_check_xbatched.py
def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


def _pairs(seed, batch, n):
    rng = np.random.default_rng(seed)
    A = np.stack([_sym(rng, n) for _ in range(batch)])
    B = np.stack([_spd(rng, n) for _ in range(batch)])
    return A, B


def _view(flat, batch, n, ld, stride):
    it = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat, shape=(batch, n, n), strides=(stride * it, ld * it, it))


def _pack(M, ld, stride, fill=SENTINEL):
    batch, n = M.shape[0], M.shape[1]
    flat = np.full(max(batch * stride, 1), fill)
    _view(flat, batch, n, ld, stride)[...] = M.transpose(0, 2, 1)
    return flat


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


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _cases(n, itype):
    """COUNT seeded pencils of order n, SciPy's w and Z of the type, Z perturbed by 1e-3 N(0, 1) / sqrt(n) per entry, and
    cond_2(B) of each.  Read only."""
    A, B = _pairs(1000 + n, COUNT, n)
    w, Z = np.zeros((COUNT, n)), np.zeros((COUNT, n, n))
    for b in range(COUNT):
        w[b], Z[b] = sl.eigh(A[b], B[b], type=itype, lower=True)
    rng = np.random.default_rng(88000 + 4 * n + itype)
    Zp = Z + 1e-3 * rng.standard_normal(Z.shape) / np.sqrt(n)
    c = _Out()
    c.n, c.A, c.B, c.w, c.Z, c.Zp = n, A, B, w, Z, Zp
    c.cond = np.array([np.linalg.cond(B[b]) for b in range(COUNT)])
    assert c.cond.max() <= 16.0, c.cond                # small enough for the bounds of type 3 to mean something
    for a in (A, B, w, Z, Zp, c.cond):
        a.setflags(write=False)
    return c


def _mirror(itype, A, B, w, Z):
    norm, ave, mx = verifier.eval_residual_norm_sygv(itype, A, B, w, Z)
    return (np.array([norm, ave, mx, verifier.eval_orthogonality_sygv(itype, Z, B)]),
            verifier.get_ipratios_sygv(itype, Z, B))


@functools.lru_cache(maxsize=None)
def _mirror_cases(n, itype):
    c = _cases(n, itype)
    return [_mirror(itype, c.A[b], c.B[b], c.w[b], c.Zp[b]) for b in range(COUNT)]


def _tol(n):
    return 4 * max(n, 8) * EPS


def _shares(itype, out, ipr, ref_out, ref_ipr, n, cond):
    """|difference| / bound per quantity: out[0] and the IPRs relative, the other three absolute; slot 3 and the IPRs of
    type 3 with max(1, cond_2(B)) in the bound.  NaN against NaN uses nothing, NaN against a number everything."""
    tol = _tol(n)
    wide = tol * (max(1.0, cond) if itype == 3 else 1.0)

    def share(x, y, bound):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        both = np.isnan(x) & np.isnan(y)
        with np.errstate(invalid="ignore"):
            s = np.abs(x - y) / bound
        s = np.where(both, 0.0, s)
        return float(np.where(np.isnan(s), np.inf, s).max())

    return np.array([share(out[0], ref_out[0], tol * abs(ref_out[0])), share(out[1], ref_out[1], tol),
                     share(out[2], ref_out[2], tol), share(out[3], ref_out[3], wide),
                     share(ipr, ref_ipr, wide * np.abs(ref_ipr))])


def _assert_shares(shares, what):
    shares = np.asarray(shares).reshape(-1, 5).max(axis=0)
    print("shares of the bounds %s: " % (what,) + ", ".join("%s %.4f" % kv for kv in zip(NAMES, shares)))
    assert np.all(shares <= 1.0), (what, shares)
    return shares


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- the calls
def _uniform(lib, form, first, A, B, w, Z, info=None, ipr=True, pad=0, fill=SENTINEL, entry=NEW):
    """entry[_device](first, ...) on strided images of A[b], B[b], Z[b] (full matrices: both triangles as given; B = None: a
    null pointer, for the standard problem of the first family); `first` is the entry's first argument (itype, or problem
    for ek_hip_check_[x]batched): pad = 0 the compact layout, pad > 0 leading
    dimensions n + pad .. and strides beyond ld * n, the gaps holding `fill`.  o.untouched: the images of A, B, w, Z after
    the call equal those before it, byte for byte."""
    batch, n = A.shape[0], A.shape[1]
    lda, ldb, ldz = (n + pad, n + 2 * pad, n + 3 * pad) if pad else (n, n, n)
    sA, sB, sZ = lda * n + (5 if pad else 0), ldb * n + (3 if pad else 0), ldz * n + (7 if pad else 0)
    h = [_pack(A, lda, sA, fill), _pack(B, ldb, sB, fill) if B is not None else np.zeros(1),
         np.ascontiguousarray(w).reshape(-1).copy() if w.size else np.zeros(1), _pack(Z, ldz, sZ, fill)]
    out = np.full(batch * 4 + 2, SENTINEL)
    q = np.full(batch * n + 3, SENTINEL)
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    ip = None if iarr is None else iarr.ctypes.data_as(_ip)
    sec = ctypes.c_double(-1.0)
    o = _Out()
    tail = (ip, out.ctypes.data_as(_dp), q.ctypes.data_as(_dp) if ipr else None, ctypes.byref(sec))
    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) for x in h]
            o.rc = getattr(lib, entry + "_device")(first, n, batch, d[0], lda, sA, d[1] if B is not None else None, ldb, sB,
                                                   d[2], d[3], ldz, sZ, *tail)
            o.untouched = all(_same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [x.copy() for x in h]
        P = [x.ctypes.data_as(_dp) for x in g]
        o.rc = getattr(lib, entry)(first, n, batch, P[0], lda, sA, P[1] if B is not None else None, ldb, sB, P[2], P[3],
                                   ldz, sZ, *tail)
        o.untouched = all(_same(y, x) for y, x in zip(g, h))
    o.seconds = sec.value
    o.out, o.ipr = out[:batch * 4].reshape(batch, 4), q[:batch * n].reshape(batch, n)
    o.tails = (out[batch * 4:], q[batch * n:] if ipr else q)
    if iarr is not None:
        assert np.array_equal(iarr, np.asarray(info, dtype=np.int32))
    return o


def _clean(o, batch):
    assert o.rc == 0 and o.untouched and o.seconds >= 0.0
    assert np.all(o.tails[0] == SENTINEL) and np.all(o.tails[1] == SENTINEL)
    assert o.out.shape == (batch, 4)


_plain = {}


def _reference_bits(lib, n, itype):
    """The perturbed cases of order n through the device form in the compact layout, once: what every other form, layout,
    position, batch and chunk must reproduce bit for bit."""
    key = (n, itype)
    if key not in _plain:
        c = _cases(n, itype)
        o = _uniform(lib, "device", itype, c.A, c.B, c.w, c.Zp)
        _clean(o, COUNT)
        o.out.setflags(write=False)
        o.ipr.setflags(write=False)
        _plain[key] = (o.out, o.ipr)
    return _plain[key]


# ------------------------------------------------------------------- 1: against the host mirror, above rounding noise
@ways
@pytest.mark.parametrize("n", ORDERS)
def test_matches_the_host_mirror(hip, n, itype, form):
    """Padded leading dimensions and strides, the gaps holding a sentinel."""
    lib = hip.load_library()
    c = _cases(n, itype)
    o = _uniform(lib, form, itype, c.A, c.B, c.w, c.Zp, pad=3)
    _clean(o, COUNT)
    ref = _mirror_cases(n, itype)
    assert 1e-6 < o.out[:, 3].min()                 # the perturbation shows: not rounding noise
    _assert_shares([_shares(itype, o.out[b], o.ipr[b], ref[b][0], ref[b][1], n, c.cond[b]) for b in range(COUNT)],
                   ("mirror", n, itype, form))


# -------------------------------------------------------------------------------------------------------- 2: forwarding
@ways
@pytest.mark.parametrize("n", (1, 33, 128))
def test_orders_up_to_128_are_forwarded(hip, n, itype, form):
    """The bits of ek_hip_check_sygv_batched* in out and ipr, with and without a skipped problem."""
    lib = hip.load_library()
    A, B = _pairs(500 + n, 3, n)
    rng = np.random.default_rng(n)
    w, Z = rng.standard_normal((3, n)), rng.standard_normal((3, n, n))
    for info in (None, [0, 4, 0]):
        pad = 2 if info is None else 0
        old = _uniform(lib, form, itype, A, B, w, Z, info=info, pad=pad, entry="ek_hip_check_sygv_batched")
        new = _uniform(lib, form, itype, A, B, w, Z, info=info, pad=pad)
        _clean(old, 3)
        _clean(new, 3)
        assert _same(new.out, old.out) and _same(new.ipr, old.ipr)
        if info is not None:
            assert np.all(np.isnan(new.out[1])) and np.all(new.ipr[1] == SENTINEL)


@forms
@pytest.mark.parametrize("n", (129, 256))
def test_type_1_is_the_xbatched_check(hip, n, form):
    """itype = 1 above 128: the bits of ek_hip_check_xbatched*(problem = 1)."""
    lib = hip.load_library()
    c = _cases(n, 2)
    old = _uniform(lib, form, 1, c.A[:2], c.B[:2], c.w[:2], c.Zp[:2], pad=1, entry="ek_hip_check_xbatched")
    new = _uniform(lib, form, 1, c.A[:2], c.B[:2], c.w[:2], c.Zp[:2], pad=1)
    _clean(old, 2)
    _clean(new, 2)
    assert _same(new.out, old.out) and _same(new.ipr, old.ipr) and np.isfinite(new.out).all()


# -------------------------------------------------------------- 3: type 2's metric is type 1's, bit for bit
@forms
@pytest.mark.parametrize("n", ORDERS)
def test_type_2_slot_3_and_iprs_are_type_1_bits(hip, n, form):
    lib = hip.load_library()
    c = _cases(n, 2)
    t1 = _uniform(lib, form, 1, c.A, c.B, c.w, c.Zp, entry="ek_hip_check_xbatched")
    t2 = _uniform(lib, form, 2, c.A, c.B, c.w, c.Zp)
    _clean(t1, COUNT)
    _clean(t2, COUNT)
    assert np.isfinite(t2.out).all() and np.isfinite(t2.ipr).all()
    assert _same(t2.out[:, 3], t1.out[:, 3]) and _same(t2.ipr, t1.ipr)
    assert not _same(t2.out[:, :3], t1.out[:, :3])  # another residual than type 1's


# ---------------------------------------------------------------------------- 4: end to end behind the batched solver
_solved = {}


def _solver_pairs(lib, n, itype):
    """ek_hip_sygv_xbatched_device on the unperturbed pencils (it overwrites its A and B: the check gets the originals)."""
    key = (n, itype)
    if key not in _solved:
        c = _cases(n, itype)
        w, Z = np.zeros(COUNT * n), np.zeros(COUNT * n * n)
        info = np.full(COUNT, -1, dtype=np.int32)
        with _Dev(lib) as dev:
            dA, dB = dev.up(_pack(c.A, n, n * n)), dev.up(_pack(c.B, n, n * n))
            dw, dZ = dev.up(w), dev.up(Z)
            assert lib.ek_hip_sygv_xbatched_device(itype, 1, n, COUNT, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                   info.ctypes.data_as(_ip), None) == 0
            w, Z = dev.down(dw, w).reshape(COUNT, n), dev.down(dZ, Z).reshape(COUNT, n, n).transpose(0, 2, 1).copy()
        assert not info.any()
        _solved[key] = (w, Z, [_mirror(itype, c.A[b], c.B[b], w[b], Z[b]) for b in range(COUNT)])
    return _solved[key]


@ways
@pytest.mark.parametrize("n", (129, 256))
def test_end_to_end_behind_the_xbatched_solver(hip, n, itype, form):
    """The solver's own w and Z against copies of the original A and B: res_max and orthogonality within 256 n eps (the
    bound tests/test_gpu_sygv_xbatched.py uses behind the one-problem check), res_ave <= res_max, and the four slots and
    the IPRs within the bounds of the mirror on the same Z."""
    lib = hip.load_library()
    c = _cases(n, itype)
    w, Z, ref = _solver_pairs(lib, n, itype)
    o = _uniform(lib, form, itype, c.A, c.B, w, Z)
    _clean(o, COUNT)
    lim = 256 * n * EPS
    print("end to end %s: res_max %.4f, orthogonality %.4f of 256 n eps"
          % ((n, itype, form), o.out[:, 2].max() / lim, o.out[:, 3].max() / lim))
    assert np.all(o.out[:, 2] <= lim), (o.out[:, 2].max(), lim)
    assert np.all(o.out[:, 1] <= o.out[:, 2])
    assert np.all(o.out[:, 3] <= lim), (o.out[:, 3].max(), lim)
    _assert_shares([_shares(itype, o.out[b], o.ipr[b], ref[b][0], ref[b][1], n, c.cond[b]) for b in range(COUNT)],
                   ("end to end", n, itype, form))


# ------------------------------------------------------------------------------ 5: against the one-problem GPU check
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_against_the_one_problem_check(hip, n, itype, form):
    lib = hip.load_library()
    c = _cases(n, itype)
    o = _uniform(lib, form, itype, c.A[:2], c.B[:2], c.w[:2], c.Zp[:2])
    _clean(o, 2)
    shares = []
    for b in range(2):
        out, q = np.zeros(4), np.zeros(n)
        with _Dev(lib) as dev:
            dA, dB = dev.up(np.asfortranarray(c.A[b])), dev.up(np.asfortranarray(c.B[b]))
            dw, dZ = dev.up(np.ascontiguousarray(c.w[b])), dev.up(np.asfortranarray(c.Zp[b]))
            assert lib.ek_hip_check_sygvx_device(itype, n, n, dA, n, dB, n, dw, dZ, n, out.ctypes.data_as(_dp),
                                                 q.ctypes.data_as(_dp)) == 0
        shares.append(_shares(itype, o.out[b], o.ipr[b], out, q, n, c.cond[b]))
    _assert_shares(shares, ("one-problem check", n, itype, form))


# ------------------------------------------------------------------------------------------------ 6: closed forms, exact
@ways
@pytest.mark.parametrize("n", (129, 256))
def test_closed_forms_are_exact(hip, n, itype, form):
    """A = diag(1 .. n), B = diag(b) with b cycling through 1, 4, 16, 1/4 (and B = I), z_i = e_i / sqrt(b_i) (type 2) or
    e_i sqrt(b_i) (type 3), w_i = a_i b_i: sqrt(b_i) is a power of two, so every product is exact, every other entry an
    exact zero: residuals and orthogonality 0, ipr_i = 1 / b_i^2 (type 2: G_ii = 1, z^4 = 1 / b_i^2) or b_i^2 (type 3:
    l_ii = sqrt(b_i), w_ii = 1), out[0] the product of two rounded roots."""
    lib = hip.load_library()
    k = np.arange(1.0, n + 1)
    b = np.array([1.0, 4.0, 16.0, 0.25])[np.arange(n) % 4]
    bs = np.stack([b, np.ones(n)])
    A = np.stack([np.diag(k), np.diag(k)])
    B = np.stack([np.diag(x) for x in bs])
    w = np.stack([k * x for x in bs])
    Z = np.stack([np.diag(1.0 / np.sqrt(x)) if itype == 2 else np.diag(np.sqrt(x)) for x in bs])
    o = _uniform(lib, form, itype, A, B, w, Z)
    _clean(o, 2)
    for i in range(2):
        norm = np.sqrt((k * k).sum()) * np.sqrt((bs[i] * bs[i]).sum())
        assert abs(o.out[i, 0] - norm) <= _tol(n) * norm
        assert o.out[i, 1] == 0.0 and o.out[i, 2] == 0.0 and o.out[i, 3] == 0.0
        assert np.array_equal(o.ipr[i], 1.0 / bs[i] ** 2 if itype == 2 else bs[i] ** 2)
    assert np.all(o.ipr[1] == 1.0)


# ------------------------------------------------------------------------------ 7: the same bits wherever a problem sits
@ways
@pytest.mark.parametrize("n", (129, 193))
def test_same_bits_at_any_position_and_in_both_forms(hip, n, itype, form):
    """A problem alone, first, last and in the middle of a batch of 5; `form` against the device form's reference."""
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    o = _uniform(lib, form, itype, c.A[:1], c.B[:1], c.w[:1], c.Zp[:1])
    _clean(o, 1)
    assert _same(o.out[0], ref_out[0]) and _same(o.ipr[0], ref_ipr[0])
    idx = np.array([0, 1, 0, 2, 0])
    o = _uniform(lib, form, itype, c.A[idx], c.B[idx], c.w[idx], c.Zp[idx])
    _clean(o, 5)
    assert _same(o.out, ref_out[idx]) and _same(o.ipr, ref_ipr[idx])


@ways
@pytest.mark.parametrize("n", (129, 193))
def test_same_bits_in_any_chunk(hip, n, itype, form):
    """Five problems in chunks of 2 and of 1, with and without a skipped one, against the default."""
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    idx = np.array([0, 1, 2, 3, 0])
    info = np.array([0, 0, 6, 0, 0], dtype=np.int32)
    live = info == 0
    try:
        for chunk in (2, 1):
            hip.check_xbatched_chunk(chunk)
            o = _uniform(lib, form, itype, c.A[idx], c.B[idx], c.w[idx], c.Zp[idx])
            _clean(o, 5)
            assert _same(o.out, ref_out[idx]) and _same(o.ipr, ref_ipr[idx])
            o = _uniform(lib, form, itype, c.A[idx], c.B[idx], c.w[idx], c.Zp[idx], info=info)
            _clean(o, 5)
            assert _same(o.out[live], ref_out[idx][live]) and _same(o.ipr[live], ref_ipr[idx][live])
            assert np.all(np.isnan(o.out[2])) and np.all(o.ipr[2] == SENTINEL)
    finally:
        hip.check_xbatched_chunk(0)


# --------------------------------------------------------------------- 8: what is not referenced, what is not written
def _nan_upper(M):
    X = np.array(M, dtype=np.float64)
    iu = np.triu_indices(X.shape[-1], 1)
    X[..., iu[0], iu[1]] = np.nan
    return X


@ways
@pytest.mark.parametrize("n", (129, 193))
def test_upper_triangles_and_padding_are_not_referenced(hip, n, itype, form):
    """NaN in the strictly upper triangles of A and B, in the rows n .. ld-1 and between the problems; ld > n and strides
    beyond ld * n: the bits of the clean compact layout.  A, B, w and Z come back byte for byte (o.untouched), and the
    slots behind out and ipr keep their sentinel (_clean)."""
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    o = _uniform(lib, form, itype, _nan_upper(c.A), _nan_upper(c.B), c.w, c.Zp, pad=3, fill=np.nan)
    _clean(o, COUNT)
    assert _same(o.out, ref_out) and _same(o.ipr, ref_ipr)


# ------------------------------------------------------------------------------------------------------- 9: isolation
@ways
@pytest.mark.parametrize("k_of", ("first", "last"))
@pytest.mark.parametrize("n", (129, 193))
def test_per_problem_isolation(hip, n, k_of, itype, form):
    """A batch of 4, a fault each: problem 0 skipped by info (its Z full of NaN is not looked at), problem 1 with a NaN
    in Z, problem 2 with the sign of B[k, k] flipped (k = 0, or k = n - 1: the last row of the second 128-row tile; type
    3: B is not SPD, type 2: merely indefinite), problem 3 sound."""
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    k = 0 if k_of == "first" else n - 1
    A, B, w, Z = c.A.copy(), c.B.copy(), c.w.copy(), c.Zp.copy()
    Z[0] = np.nan
    Z[1, n // 2, n // 3] = np.nan
    B[2, k, k] = -B[2, k, k]
    info = np.array([5, 0, 0, 0], dtype=np.int32)
    m_out, m_ipr = _mirror(itype, A[2], B[2], w[2], Z[2])
    for ipr in (True, False):
        o = _uniform(lib, form, itype, A, B, w, Z, info=info, ipr=ipr)
        _clean(o, 4)
        assert np.all(np.isnan(o.out[0]))
        assert np.all(o.ipr == SENTINEL) if not ipr else np.all(o.ipr[0] == SENTINEL)
        assert o.out[1, 0] == ref_out[1, 0] and not np.isfinite(o.out[1, 1:]).any()
        if ipr:
            assert np.isnan(o.ipr[1, n // 3])
        # the residual slots of the problem with the flipped pivot are the mirror's
        s = _shares(itype, o.out[2], o.ipr[2] if ipr else m_ipr, m_out, m_ipr, n, c.cond[2])
        assert np.all(s[:3] <= 1.0), s
        if itype == 3:
            assert np.isnan(o.out[2, 3]) and np.isnan(m_out[3])
            if ipr:
                assert np.all(np.isnan(o.ipr[2])) and np.all(np.isnan(m_ipr))
        else:
            assert np.all(s <= 1.0), s
        assert _same(o.out[3], ref_out[3])
        if ipr:
            assert _same(o.ipr[3], ref_ipr[3])


# ------------------------------------------------------------------------------------------------ 10: a planted error
@ways
def test_a_planted_error_moves_what_the_mirror_says(hip, itype, form):
    """n = 200, SciPy's pairs: column 17 of Z scaled by 1 + 1e-6 (the check scales by the computed G_jj and divides the
    residual by ||z_j||: nothing moves beyond rounding, that column's IPR included) and the sign of w[40] flipped (rho of
    that column becomes 2 |w_40| / (||A||_F ||B||_F)).  What moves moves as the mirror's does."""
    lib = hip.load_library()
    n = 200
    c = _cases(n, itype)
    A, B = c.A[:1], c.B[:1]
    w, Z = c.w[:1].copy(), c.Z[:1].copy()
    before = _uniform(lib, form, itype, A, B, w, Z)
    _clean(before, 1)
    ref0 = _mirror(itype, A[0], B[0], w[0], Z[0])
    Z[0, :, 17] *= 1.0 + 1e-6
    w[0, 40] = -w[0, 40]
    after = _uniform(lib, form, itype, A, B, w, Z)
    _clean(after, 1)
    ref1 = _mirror(itype, A[0], B[0], w[0], Z[0])
    assert ref0[0][2] < 1e-12 and ref1[0][2] > 1e3 * ref0[0][2]          # the plant shows in the mirror
    cond = c.cond[0]
    _assert_shares([_shares(itype, before.out[0], before.ipr[0], ref0[0], ref0[1], n, cond),
                    _shares(itype, after.out[0], after.ipr[0], ref1[0], ref1[1], n, cond)], ("planted", n, itype, form))
    tol = _tol(n)
    wide = tol * (max(1.0, cond) if itype == 3 else 1.0)
    assert abs((after.out[0, 2] - before.out[0, 2]) - (ref1[0][2] - ref0[0][2])) <= 2 * tol
    assert abs((after.out[0, 3] - before.out[0, 3]) - (ref1[0][3] - ref0[0][3])) <= 2 * wide
    assert abs((after.ipr[0, 17] - before.ipr[0, 17]) - (ref1[1][17] - ref0[1][17])) <= 2 * wide * ref0[1][17]


# --------------------------------------------------------------------------------------------------------- 11: cost
@pytest.mark.parametrize("itype", (2, 3))
@pytest.mark.parametrize("n", (129, 256))
def test_the_check_against_the_solve_and_the_host_loop(hip, n, itype):
    """256 pencils with vectors: best of 3 of the check's device time against best of 3 of the solver's
    (ek_hip_sygv_xbatched_device of the same type) on the same device arrays, alternated, after one warm-up of each: the
    check costs no more than the solve (the project's gate of DESIGN.md 14, 16 and 18).  Then the check's wall time
    against a host loop over ek_hip_check_sygvx_device on 64 of those pencils, scaled to 256: the batched check is the
    faster one.  Both yardsticks are older entries; the type-1 check is timed for the record only."""
    lib = hip.load_library()
    batch, loop_n = 256, 64
    A16, B16 = _pairs(4242 + n, 16, n)
    A, B = np.tile(A16, (batch // 16, 1, 1)), np.tile(B16, (batch // 16, 1, 1))
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    out, q = np.zeros(batch * 4), np.zeros(batch * n)
    out1, q1 = np.zeros(batch * 4), np.zeros(batch * n)
    info = np.zeros(batch, dtype=np.int32)
    t_solve, t_check, t_check1, w_check, w_loop = [], [], [], [], []
    tail = (info.ctypes.data_as(_ip), out.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_sygv_xbatched_device(itype, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                   info.ctypes.data_as(_ip), ctypes.byref(sec)) == 0
            assert not info.any()
            t_solve.append(sec.value)
            sec = ctypes.c_double(-1.0)
            t0 = time.perf_counter()
            assert lib.ek_hip_check_sygv_xbatched_device(itype, n, batch, dA0, n, n * n, dB0, n, n * n, dw, dZ, n, n * n,
                                                         *tail, ctypes.byref(sec)) == 0
            w_check.append(time.perf_counter() - t0)
            t_check.append(sec.value)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_check_xbatched_device(1, n, batch, dA0, n, n * n, dB0, n, n * n, dw, dZ, n, n * n,
                                                    info.ctypes.data_as(_ip), out1.ctypes.data_as(_dp),
                                                    q1.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
            t_check1.append(sec.value)
        o1, qq = np.zeros(4), np.zeros(n)
        loop = np.zeros((loop_n, 4))

        def at(p, words):
            return ctypes.c_void_p(p.value + 8 * words)

        for it in range(3):
            t0 = time.perf_counter()
            for b in range(loop_n):
                assert lib.ek_hip_check_sygvx_device(itype, n, n, at(dA0, b * n * n), n, at(dB0, b * n * n), n,
                                                     at(dw, b * n), at(dZ, b * n * n), n, o1.ctypes.data_as(_dp),
                                                     qq.ctypes.data_as(_dp)) == 0
                loop[b] = o1
            w_loop.append((time.perf_counter() - t0) * (batch / loop_n))
    o = out.reshape(batch, 4)
    lim = 256 * n * EPS
    assert np.all(o[:, 2] <= lim) and np.all(o[:, 3] <= lim)
    wide = _tol(n) * (10.0 if itype == 3 else 1.0)  # cond_2(B) = 10 by construction
    assert np.all(np.abs(o[:loop_n, 1:3] - loop[:, 1:3]) <= _tol(n)) and np.all(np.abs(o[:loop_n, 3] - loop[:, 3]) <= wide)
    assert np.all(np.abs(o[:loop_n, 0] - loop[:, 0]) <= _tol(n) * loop[:, 0])
    ts, tc, t1 = min(t_solve[1:]), min(t_check[1:]), min(t_check1[1:])
    wc, wl = min(w_check[1:]), min(w_loop)
    print("cost n=%d itype=%d batch=%d: solve %.3f ms, check %.3f ms device (%.3f ms wall), check / solve %.3f, "
          "check / type-1 check %.2f; host loop %.1f ms (64 scaled to 256), loop / check %.1f"
          % (n, itype, batch, ts * 1e3, tc * 1e3, wc * 1e3, tc / ts, tc / t1, wl * 1e3, wl / wc))
    assert 0.0 < tc <= ts, (tc, ts)
    assert wc < wl, (wc, wl)


# ------------------------------------------------------------------------ 12: one device pool behind every family
def _mirror1(A, B, w, Z):
    """The mirror of the standard problem (B = None) and of type 1."""
    a_norm, ave, mx = verifier.eval_residual_norm(A, w, Z, B)
    return np.array([a_norm, ave, mx, verifier.eval_orthogonality(Z, B)]), verifier.get_ipratios(Z, B)


@functools.lru_cache(maxsize=None)
def _pool_inputs():
    """The fixed inputs of the five calls below, from _pairs and SciPy's pairs perturbed as in _cases.  Read only."""
    def solved(seed, batch, n, itype, with_b=True):
        A, B = _pairs(seed, batch, n) if n else (np.zeros((batch, 0, 0)), np.zeros((batch, 0, 0)))
        w, Z = np.zeros((batch, n)), np.zeros((batch, n, n))
        for b in range(batch if n else 0):
            w[b], Z[b] = sl.eigh(A[b], B[b], type=itype, lower=True) if with_b else sl.eigh(A[b], lower=True)
        Zp = Z + 1e-3 * np.random.default_rng(seed + 7).standard_normal(Z.shape) / np.sqrt(n)
        for a in (A, B, w, Zp):
            a.setflags(write=False)
        return A, (B if with_b else None), w, Zp

    c = _Out()
    c.gen40 = solved(31040, 5, 40, 1)
    c.x129 = tuple(a[:3] for a in (_cases(129, 3).A, _cases(129, 3).B, _cases(129, 3).w, _cases(129, 3).Zp))
    c.std130 = solved(31130, 3, 130, 1, with_b=False)
    c.var = [solved(31200 + n, 1, n, 1) for n in (0, 33, 64)]
    c.t2_40 = solved(32040, 5, 40, 2)
    return c


def _pool_round(hip, lib):
    """The entries of all three units and the variable form one after the other, host forms: each call finds in the pool
    what the call before it left there."""
    c = _pool_inputs()
    r = []
    # an int map in the table buffer, a small scratch
    r.append(_uniform(lib, "host", 1, *c.gen40, info=[0, 3, 0, 0, 0], entry="ek_hip_check_batched"))
    # the scratch grows to 2 * 2 * 129^2 doubles, two launches, no map
    try:
        hip.check_xbatched_chunk(2)
        r.append(_uniform(lib, "host", 3, *c.x129))
    finally:
        hip.check_xbatched_chunk(0)
    # no scratch asked for while the pool holds a large one, a map shorter than the first call's, no IPRs
    r.append(_uniform(lib, "host", 0, *c.std130, info=[0, 0, 2], ipr=False, entry="ek_hip_check_xbatched"))
    # a table of descriptors where the map was
    v = _Out()
    v.out, v.iprs = hip.check_vbatched([x[0][0] for x in c.var], [x[1][0] for x in c.var], [x[2][0] for x in c.var],
                                       [x[3][0] for x in c.var])
    r.append(v)
    r.append(_uniform(lib, "host", 2, *c.t2_40, entry="ek_hip_check_sygv_batched"))
    return r


def test_one_pool_serves_every_family_in_turn(hip):
    """ek_hip_check_batched (generalized, n = 40, a skipped problem), ek_hip_check_sygv_xbatched (type 3, n = 129, chunks of
    2), ek_hip_check_xbatched (standard, n = 130, a skipped problem, no IPRs), ek_hip_check_vbatched (orders 0, 33, 64) and
    ek_hip_check_sygv_batched (type 2, n = 40) share one scratch, one buffer of output words, one table / map buffer and
    two events.  The sequence runs twice: the second round's words are the first round's bit for bit, NaN
    slots included; a skipped problem has NaN in its four slots and its IPR row untouched; every call of the first round
    agrees with the host mirror within the bounds of the tests above (4 max(n, 8) eps, max(1, cond_2(B)) wider for slot 3
    and the IPRs of type 3)."""
    lib = hip.load_library()
    c = _pool_inputs()
    first, second = _pool_round(hip, lib), _pool_round(hip, lib)
    for k, (a, b) in enumerate(zip(first, second)):
        if k == 3:
            assert _same(a.out, b.out) and all(_same(x, y) for x, y in zip(a.iprs, b.iprs))
        else:
            _clean(a, a.out.shape[0])
            _clean(b, b.out.shape[0])
            assert _same(a.out, b.out) and _same(a.ipr, b.ipr), k
    g40, x129, s130, var, t40 = first
    # the skipped problems
    assert np.all(np.isnan(g40.out[1])) and np.all(g40.ipr[1] == SENTINEL)
    assert np.all(np.isnan(s130.out[2])) and np.all(s130.ipr == SENTINEL)
    # the mirror
    A, B, w, Z = c.gen40
    _assert_shares([_shares(1, g40.out[b], g40.ipr[b], *_mirror1(A[b], B[b], w[b], Z[b]), 40, 1.0) for b in (0, 2, 3, 4)],
                   ("pool", "check_batched", 40))
    ref, cond = _mirror_cases(129, 3), _cases(129, 3).cond
    _assert_shares([_shares(3, x129.out[b], x129.ipr[b], ref[b][0], ref[b][1], 129, cond[b]) for b in range(3)],
                   ("pool", "check_sygv_xbatched", 129))
    A, _, w, Z = c.std130
    for b in (0, 1):
        m_out, m_ipr = _mirror1(A[b], None, w[b], Z[b])
        _assert_shares([_shares(1, s130.out[b], m_ipr, m_out, m_ipr, 130, 1.0)], ("pool", "check_xbatched", 130, b))
    assert var.out[0, 0] == 0.0 and np.all(np.isnan(var.out[0, 1:])) and var.iprs[0].size == 0
    for b, n in ((1, 33), (2, 64)):
        A, B, w, Z = (x[0] for x in c.var[b])
        _assert_shares([_shares(1, var.out[b], var.iprs[b], *_mirror1(A, B, w, Z), n, 1.0)],
                       ("pool", "check_vbatched", n))
    A, B, w, Z = c.t2_40
    _assert_shares([_shares(2, t40.out[b], t40.ipr[b], *_mirror(2, A[b], B[b], w[b], Z[b]), 40, 1.0) for b in range(5)],
                   ("pool", "check_sygv_batched", 40))
