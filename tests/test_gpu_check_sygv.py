"""GPU suite of the acceptance checks for DSYGV's types 2 (A B x = l x) and 3 (B A x = l x): ek_hip_check_sygv_batched*,
ek_hip_check_sygv_vbatched* (a workgroup per problem, order <= 128) and ek_hip_check_sygvx* (one problem of any order).

The yardstick is the host mirror eigenkernel_amd/verifier.py (*_sygv) in float64 on the seeded _sym / _spd pairs of
tests/test_gpu_batched.py (helpers copied from there) with SciPy's eigh(A, B, type=itype) as (w, Z).  Bounds, per
problem of order n: 4 max(n, 8) eps on the relative difference of out[0] and on the absolute difference of out[1 .. 3] and
of every IPR -- the figure tests/test_gpu_check_batched.py uses against the mirror -- multiplied by max(1, cond_2(B)) for
slot 3 and the IPRs of type 3, because two exact factors of B lie cond(B) eps apart (docstring of
tests/test_gpu_sygv_batched.py).  cond_2(B) of these pairs is computed here on the CPU: the largest is 10.0 (the
spectrum of _spd is log-spaced in [1, 10]; 1.0 at order 1), asserted <= 16, so that the widest bound of the suite is
64 * 128 eps = 1.8e-12, six orders below the 1e-6 perturbations that the detection test plants.  Each test prints the
largest share of each bound it used (pytest -s shows it).

Closed forms: with A = diag(a), B = diag(b) and z_i = e_i / sqrt(b_i) (type 2) or e_i sqrt(b_i) (type 3), G = I, the
residual and the orthogonality are exactly 0 and ipr_i = sum z^4 / G_ii^2 is exactly 1 / b_i^2 (type 2) and b_i^2 (type 3):
exactly 1 where b_i = 1, which the test covers with B = I beside a B of powers of 4."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import verifier

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (1, 2, 3, 31, 32, 33, 64, 65, 127, 128)
SENTINEL = -7.25e77
NAMES = ("norm", "res_ave", "res_max", "orthogonality", "ipr")
COUNT = 6
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
types23 = pytest.mark.parametrize("itype", (2, 3))
forms = pytest.mark.parametrize("form", ("device", "host"))


# ------------------------------------------------------------------------------- helpers of tests/test_gpu_batched.py
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
    """COUNT seeded pairs of order n with SciPy's eigenpairs of the type, and cond_2(B) of each.  Read only."""
    A, B = _pairs(1000 + n, COUNT, n)
    w, Z = np.zeros((COUNT, n)), np.zeros((COUNT, n, n))
    for b in range(COUNT):
        w[b], Z[b] = sl.eigh(A[b], B[b], type=itype, lower=True)
    c = _Out()
    c.n, c.A, c.B, c.w, c.Z = n, A, B, w, Z
    c.cond = np.array([np.linalg.cond(B[b]) for b in range(COUNT)])
    assert c.cond.max() <= 16.0, c.cond                # small enough for the bounds of type 3 to mean something
    for a in (A, B, w, Z, c.cond):
        a.setflags(write=False)
    return c


def _mirror(itype, A, B, w, Z):
    norm, ave, mx = verifier.eval_residual_norm_sygv(itype, A, B, w, Z)
    return np.array([norm, ave, mx, verifier.eval_orthogonality_sygv(itype, Z, B)]), verifier.get_ipratios_sygv(itype, Z, B)


@functools.lru_cache(maxsize=None)
def _mirror_cases(n, itype):
    c = _cases(n, itype)
    return [_mirror(itype, c.A[b], c.B[b], c.w[b], c.Z[b]) for b in range(COUNT)]


def _shares(itype, out, ipr, ref_out, ref_ipr, n, cond):
    """|difference| / bound per quantity: out[0] relative, out[1 .. 3] and the IPRs absolute; slot 3 and the IPRs of type 3
    with max(1, cond_2(B)) in the bound."""
    tol = 4 * max(n, 8) * EPS
    wide = tol * (max(1.0, cond) if itype == 3 else 1.0)
    s = np.abs(out - ref_out) / tol
    s[0] /= abs(ref_out[0])
    s[3] = abs(out[3] - ref_out[3]) / wide
    return np.append(s, np.abs(ipr - ref_ipr).max() / wide)


def _assert_shares(shares, what):
    shares = np.asarray(shares).reshape(-1, 5).max(axis=0)
    print("shares of the bounds %s: " % (what,) + ", ".join("%s %.3f" % kv for kv in zip(NAMES, shares)))
    assert np.all(shares <= 1.0), (what, shares)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- the calls
def _uniform(lib, form, first, A, B, w, Z, info=None, ipr=True, pad=0, fill=SENTINEL, family="sygv"):
    """ek_hip_check_sygv_batched[_device] (family "sygv", first = itype) or ek_hip_check_batched[_device] (family "plain",
    first = problem) on strided images of A[b], B[b], Z[b] (full matrices: both triangles as given): pad = 0 the compact
    layout, pad > 0 leading dimensions n + pad .. and strides beyond ld * n, the gaps holding `fill`.  o.untouched: the
    images of A, B, w, Z after the call equal those before it, byte for byte."""
    batch, n = A.shape[0], A.shape[1]
    lda, ldb, ldz = (n + pad, n + 2 * pad, n + 3 * pad) if pad else (n, n, n)
    sA, sB, sZ = lda * n + (5 if pad else 0), ldb * n + (3 if pad else 0), ldz * n + (7 if pad else 0)
    h = [_pack(A, lda, sA, fill), _pack(B, ldb, sB, fill), np.ascontiguousarray(w).reshape(-1).copy(),
         _pack(Z, ldz, sZ, fill)]
    out = np.full(batch * 4 + 2, SENTINEL)
    q = np.full(batch * n + 3, SENTINEL)
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    ip = None if iarr is None else iarr.ctypes.data_as(_ip)
    sec = ctypes.c_double(-1.0)
    o = _Out()
    tail = (ip, out.ctypes.data_as(_dp), q.ctypes.data_as(_dp) if ipr else None, ctypes.byref(sec))
    stem = "ek_hip_check_sygv_batched" if family == "sygv" else "ek_hip_check_batched"
    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) for x in h]
            o.rc = getattr(lib, stem + "_device")(first, n, batch, d[0], lda, sA, d[1], ldb, sB, d[2], d[3], ldz, sZ, *tail)
            o.untouched = all(_same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [x.copy() for x in h]
        P = [x.ctypes.data_as(_dp) for x in g]
        o.rc = getattr(lib, stem)(first, n, batch, P[0], lda, sA, P[1], ldb, sB, P[2], P[3], ldz, sZ, *tail)
        o.untouched = all(_same(y, x) for y, x in zip(g, h))
    o.seconds = sec.value
    o.out, o.ipr = out[:batch * 4].reshape(batch, 4), q[:batch * n].reshape(batch, n)
    o.tails = (out[batch * 4:], q[batch * n:] if ipr else q)
    if iarr is not None:
        assert np.array_equal(iarr, np.asarray(info, dtype=np.int32))
    return o


def _variable(lib, form, first, As, Bs, ws, Zs, info=None, ipr=True, pad=0, fill=SENTINEL, no_ipr=(), family="sygv"):
    """ek_hip_check_sygv_vbatched[_device] (or the plain family): problem b in its own column-major array with leading
    dimension max(1, n[b]) + pad (A), + 2 pad (B), + 3 pad (Z), the rows below n[b] holding `fill`; ipr[b] has two slots
    more than n[b], and the problems listed in no_ipr pass a NULL entry."""
    batch = len(As)
    n = np.array([M.shape[0] for M in As], dtype=np.int32)
    lds = [np.maximum(n, 1).astype(np.int32) + k * pad for k in (1, 2, 3)]

    def image(M, ld):
        X = np.full((ld, M.shape[0]), fill, order="F")
        X[:M.shape[0], :] = M
        return X

    h = [[image(M, lds[0][b]) for b, M in enumerate(As)], [image(M, lds[1][b]) for b, M in enumerate(Bs)],
         [np.array(v, dtype=np.float64) for v in ws], [image(M, lds[2][b]) for b, M in enumerate(Zs)]]
    out = np.full(batch * 4 + 2, SENTINEL)
    qs = [np.full(k + 2, SENTINEL) for k in n]
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    sec = ctypes.c_double(-1.0)
    o = _Out()
    stem = "ek_hip_check_sygv_vbatched" if family == "sygv" else "ek_hip_check_vbatched"

    def table(ptrs):
        return (ctypes.c_void_p * batch)(*ptrs)

    def call(fn, P):
        return fn(first, batch, n.ctypes.data_as(_ip), table(P[0]), lds[0].ctypes.data_as(_ip), table(P[1]),
                  lds[1].ctypes.data_as(_ip), table(P[2]), table(P[3]), lds[2].ctypes.data_as(_ip),
                  None if iarr is None else iarr.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                  table([None if b in no_ipr else qs[b].ctypes.data for b in range(batch)]) if ipr else None,
                  ctypes.byref(sec))

    if form == "device":
        with _Dev(lib) as dev:
            d = [[dev.up(x) if x.size else None for x in k] for k in h]
            o.rc = call(getattr(lib, stem + "_device"), [[p.value if p else None for p in k] for k in d])
            o.untouched = all(_same(dev.down(p, x), x) for k, hk in zip(d, h) for p, x in zip(k, hk) if p is not None)
    else:
        g = [[x.copy(order="K") for x in k] for k in h]
        o.rc = call(getattr(lib, stem), [[x.ctypes.data if x.size else None for x in k] for k in g])
        o.untouched = all(_same(y, x) for k, hk in zip(g, h) for y, x in zip(k, hk))
    o.seconds = sec.value
    o.out = out[:batch * 4].reshape(batch, 4)
    o.ipr = [q[:k] for q, k in zip(qs, n)]
    o.tails = (out[batch * 4:], np.concatenate([q[k:] for q, k in zip(qs, n)]))
    return o


def _clean(o, batch):
    assert o.rc == 0 and o.untouched and o.seconds >= 0.0
    assert np.all(o.tails[0] == SENTINEL) and np.all(o.tails[1] == SENTINEL)
    assert o.out.shape == (batch, 4)


_plain = {}


def _reference_bits(lib, n, itype):
    """The COUNT cases of order n through the uniform device form in the compact layout, once: what every other form,
    layout, position and batch must reproduce bit for bit."""
    key = (n, itype)
    if key not in _plain:
        c = _cases(n, itype)
        o = _uniform(lib, "device", itype, c.A, c.B, c.w, c.Z)
        _clean(o, COUNT)
        o.out.setflags(write=False)
        o.ipr.setflags(write=False)
        _plain[key] = (o.out, o.ipr)
    return _plain[key]


# ------------------------------------------------------------------------------------------ 1: against the host mirror
@forms
@types23
@pytest.mark.parametrize("n", ORDERS)
def test_uniform_matches_the_host_mirror(hip, n, itype, form):
    """A batch of 8 (the six cases and two of them again) through the uniform forms."""
    lib = hip.load_library()
    c = _cases(n, itype)
    idx = np.array([0, 1, 2, 3, 4, 5, 0, 1])
    o = _uniform(lib, form, itype, c.A[idx], c.B[idx], c.w[idx], c.Z[idx])
    _clean(o, 8)
    ref = _mirror_cases(n, itype)
    _assert_shares([_shares(itype, o.out[k], o.ipr[k], ref[b][0], ref[b][1], n, c.cond[b]) for k, b in enumerate(idx)],
                   (n, itype, form))


@forms
@types23
def test_variable_matches_the_host_mirror(hip, itype, form):
    """Six problems of every order, and two of order 0, in one call (at most three launches)."""
    lib = hip.load_library()
    sel = [(n, b) for b in range(COUNT) for n in ORDERS]
    cs = {n: _cases(n, itype) for n in ORDERS}
    e = np.zeros((0, 0))
    o = _variable(lib, form, itype, [e] + [cs[n].A[b] for n, b in sel] + [e], [e] + [cs[n].B[b] for n, b in sel] + [e],
                  [np.zeros(0)] + [cs[n].w[b] for n, b in sel] + [np.zeros(0)],
                  [e] + [cs[n].Z[b] for n, b in sel] + [e])
    _clean(o, len(sel) + 2)
    for k in (0, len(sel) + 1):                      # order 0: 0 / 0, as in the plain family
        assert o.out[k, 0] == 0.0 and np.all(np.isnan(o.out[k, 1:])) and o.ipr[k].size == 0
    shares = []
    for k, (n, b) in enumerate(sel):
        ref = _mirror_cases(n, itype)[b]
        shares.append(_shares(itype, o.out[k + 1], o.ipr[k + 1], ref[0], ref[1], n, cs[n].cond[b]))
    _assert_shares(shares, ("variable", itype, form))


# -------------------------------------------------------------------------------------- 2: it detects what it must
@types23
@pytest.mark.parametrize("n", (2, 3, 33, 65, 128))
def test_detects_a_scaled_column_a_moved_eigenvalue_and_a_duplicate_column(hip, n, itype):
    """Problem 2: one column of Z scaled by 1 + 1e-6 (every quantity of types 2 and 3 is invariant under it: the slots
    must still be the mirror's); problem 4: the w_j of largest magnitude moved by 1e-6 |w_j|; problem 6: one column
    replaced by a copy of its neighbour.  Each shows, to the mirror's value, in its own slots and in no other's."""
    lib = hip.load_library()
    c = _cases(n, itype)
    idx = np.array([0, 1, 2, 3, 4, 5, 0, 1])
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    A, B, w, Z = c.A[idx], c.B[idx], c.w[idx].copy(), c.Z[idx].copy()
    col = n // 2
    Z[2, :, col] *= 1.0 + 1e-6
    j = int(np.argmax(np.abs(w[4])))
    w[4, j] += 1e-6 * abs(w[4, j])
    Z[6, :, col] = Z[6, :, col - 1] if col else Z[6, :, 1]
    o = _uniform(lib, "device", itype, A, B, w, Z)
    _clean(o, 8)
    hit = (2, 4, 6)
    shares = []
    for k in hit:
        m_out, m_ipr = _mirror(itype, A[k], B[k], w[k], Z[k])
        shares.append(_shares(itype, o.out[k], o.ipr[k], m_out, m_ipr, n, c.cond[idx[k]]))
    _assert_shares(shares, ("detection", n, itype))
    # the moved eigenvalue: r_j moves by 1e-6 |w_j| z_j, so rho_j is 1e-6 |w_j| / (||A||_F ||B||_F) to the rounding it was
    planted = 1e-6 * abs(w[4, j]) / o.out[4, 0]
    assert o.out[4, 2] >= 0.99 * planted > 1e4 * ref_out[idx[4], 2]
    assert _same(o.out[4, 3:], ref_out[idx[4], 3:]) and _same(o.ipr[4], ref_ipr[idx[4]])
    # the duplicate column: two off-diagonal entries of the scaled G are 1
    assert o.out[6, 3] > 1.4
    for k in range(8):
        if k not in hit:
            assert _same(o.out[k], ref_out[idx[k]]) and _same(o.ipr[k], ref_ipr[idx[k]])


# ----------------------------------------------------------------------------------------------------- 3: closed forms
@forms
@types23
@pytest.mark.parametrize("n", ORDERS)
def test_closed_forms(hip, n, itype, form):
    """A = diag(a), B = diag(b), w = a b and z_i = e_i / sqrt(b_i) (type 2), e_i sqrt(b_i) (type 3), a small integers and b
    powers of 4, so that every product is exact: residual exactly 0, orthogonality exactly 0, ipr_i exactly 1 / b_i^2
    (type 2) and b_i^2 (type 3) -- exactly 1 for B = I (problem 1)."""
    lib = hip.load_library()
    a = np.arange(1.0, n + 1)
    b4 = 4.0 ** (np.arange(n) % 4)
    A = np.stack([np.diag(a), np.diag(a)])
    B = np.stack([np.diag(b4), np.eye(n)])
    w = np.stack([a * b4, a])
    root = np.sqrt(b4)
    Z = np.stack([np.diag(1.0 / root if itype == 2 else root), np.eye(n)])
    o = _uniform(lib, form, itype, A, B, w, Z)
    _clean(o, 2)
    tol = 4 * max(n, 8) * EPS
    for k, b in enumerate((b4, np.ones(n))):
        norm = np.sqrt((a * a).sum()) * np.sqrt((b * b).sum())
        assert abs(o.out[k, 0] - norm) <= tol * norm
        assert o.out[k, 1] == 0.0 and o.out[k, 2] == 0.0 and o.out[k, 3] == 0.0
        assert np.array_equal(o.ipr[k], 1.0 / b ** 2 if itype == 2 else b ** 2)
    assert np.all(o.ipr[1] == 1.0)


# ------------------------------------------------------------------------------------------- 4: behind the solver
@types23
@pytest.mark.parametrize("n", ORDERS)
def test_behind_the_batched_solver(hip, n, itype):
    """ek_hip_sygv_batched_device on copies, its w and Z checked where they lie: residual and orthogonality within the
    256 n eps of tests/test_gpu_sygv_batched.py (whose residual is divided by max|A| |B|_2 <= ||A||_F ||B||_F)."""
    lib = hip.load_library()
    c = _cases(n, itype)
    hA, hB = _pack(c.A, n, n * n), _pack(c.B, n, n * n)
    out, q = np.zeros(COUNT * 4), np.zeros(COUNT * n)
    info = np.full(COUNT, -1, dtype=np.int32)
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(COUNT * n)), dev.up(np.zeros(COUNT * n * n))
        assert lib.ek_hip_sygv_batched_device(itype, 1, n, COUNT, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                              info.ctypes.data_as(_ip), None) == 0
        assert not info.any()
        assert lib.ek_hip_check_sygv_batched_device(itype, n, COUNT, dA0, n, n * n, dB0, n, n * n, dw, dZ, n, n * n,
                                                    info.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                                                    q.ctypes.data_as(_dp), None) == 0
    o = out.reshape(COUNT, 4)
    lim = 256 * n * EPS
    print("behind the solver %s: res_max %.3f, orthogonality %.3f of 256 n eps" % ((n, itype), o[:, 2].max() / lim,
                                                                                 o[:, 3].max() / lim))
    assert np.all(o[:, 2] <= lim) and np.all(o[:, 1] <= o[:, 2]) and np.all(o[:, 3] <= lim)
    assert np.all(q > 0.0) and np.all(np.isfinite(q))


# ------------------------------------------------------------------------------------------------ 5: bit contracts
@forms
@pytest.mark.parametrize("n", (1, 33, 64, 127))
def test_itype_1_is_problem_1_of_the_plain_checks(hip, n, form):
    lib = hip.load_library()
    c = _cases(n, 1)
    o1 = _uniform(lib, form, 1, c.A, c.B, c.w, c.Z)
    op = _uniform(lib, form, 1, c.A, c.B, c.w, c.Z, family="plain")
    _clean(o1, COUNT)
    _clean(op, COUNT)
    assert _same(o1.out, op.out) and _same(o1.ipr, op.ipr)
    v1 = _variable(lib, form, 1, list(c.A), list(c.B), list(c.w), list(c.Z))
    vp = _variable(lib, form, 1, list(c.A), list(c.B), list(c.w), list(c.Z), family="plain")
    _clean(v1, COUNT)
    assert _same(v1.out, vp.out) and all(_same(x, y) for x, y in zip(v1.ipr, vp.ipr))
    assert _same(v1.out, o1.out)


@pytest.mark.parametrize("n", ORDERS)
def test_type_2_shares_slot_3_and_the_iprs_with_type_1(hip, n):
    """For the same (B, Z): G = Z^T B Z in both types, accumulated in the same order."""
    lib = hip.load_library()
    c = _cases(n, 2)
    o2 = _uniform(lib, "device", 2, c.A, c.B, c.w, c.Z)
    o1 = _uniform(lib, "device", 1, c.A, c.B, c.w, c.Z)
    _clean(o2, COUNT)
    _clean(o1, COUNT)
    assert _same(o2.out[:, 3], o1.out[:, 3]) and _same(o2.ipr, o1.ipr)
    assert not _same(o2.out[:, :3], o1.out[:, :3])


@forms
@types23
@pytest.mark.parametrize("n", (31, 64, 127, 128))
def test_same_bits_at_any_position_of_any_batch(hip, n, itype, form):
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    o = _uniform(lib, form, itype, c.A[:1], c.B[:1], c.w[:1], c.Z[:1])
    _clean(o, 1)
    assert _same(o.out[0], ref_out[0]) and _same(o.ipr[0], ref_ipr[0])
    for batch in (8, 300):                           # 300 of class 128: more workgroups than the device has CUs
        idx = np.array([(3 * b + 1) % 5 + 1 for b in range(batch)])      # filler: cases 1 .. 5
        spots = (0, 7, batch - 1)
        idx[list(spots)] = 0
        o = _uniform(lib, form, itype, c.A[idx], c.B[idx], c.w[idx], c.Z[idx])
        _clean(o, batch)
        assert _same(o.out, ref_out[idx]) and _same(o.ipr, ref_ipr[idx])


@forms
@types23
def test_same_bits_through_the_variable_form(hip, itype, form):
    """Every order in one call, in two permutations: each problem's bits are the uniform call's."""
    lib = hip.load_library()
    rng = np.random.default_rng(5)
    for perm in (np.arange(len(ORDERS)), rng.permutation(len(ORDERS))):
        orders = [ORDERS[k] for k in perm]
        cs = [_cases(n, itype) for n in orders]
        o = _variable(lib, form, itype, [c.A[0] for c in cs], [c.B[0] for c in cs], [c.w[0] for c in cs],
                      [c.Z[0] for c in cs])
        _clean(o, len(orders))
        for k, n in enumerate(orders):
            ref_out, ref_ipr = _reference_bits(lib, n, itype)
            assert _same(o.out[k], ref_out[0]) and _same(o.ipr[k], ref_ipr[0]), (n, k)


# --------------------------------------------------------------------- 6: what is not referenced, what is not written
def _nan_upper(M):
    X = np.array(M, dtype=np.float64)
    iu = np.triu_indices(X.shape[-1], 1)
    X[..., iu[0], iu[1]] = np.nan
    return X


@forms
@types23
@pytest.mark.parametrize("n", (1, 3, 32, 33, 65, 128))
def test_upper_triangles_and_padding_are_not_referenced(hip, n, itype, form):
    """NaN in the strictly upper triangles of A and B, in the rows n .. ld-1 and between the problems: the bits of the
    clean compact layout; A, B, w and Z come back byte for byte (o.untouched)."""
    lib = hip.load_library()
    c = _cases(n, itype)
    ref_out, ref_ipr = _reference_bits(lib, n, itype)
    o = _uniform(lib, form, itype, _nan_upper(c.A), _nan_upper(c.B), c.w, c.Z, pad=3, fill=np.nan)
    _clean(o, COUNT)
    assert _same(o.out, ref_out) and _same(o.ipr, ref_ipr)
    o = _variable(lib, form, itype, list(_nan_upper(c.A)), list(_nan_upper(c.B)), list(c.w), list(c.Z), pad=2,
                  fill=np.nan, no_ipr=(4,))
    _clean(o, COUNT)
    assert _same(o.out, ref_out)
    for b in range(COUNT):
        assert np.all(o.ipr[b] == SENTINEL) if b == 4 else _same(o.ipr[b], ref_ipr[b])
    o = _uniform(lib, form, itype, c.A, c.B, c.w, c.Z, ipr=False)            # ipr = NULL
    _clean(o, COUNT)
    assert _same(o.out, ref_out) and np.all(o.ipr == SENTINEL)


@forms
@types23
@pytest.mark.parametrize("n", (30, 64, 100))
def test_per_problem_isolation(hip, n, itype, form):
    lib = hip.load_library()
    A6, B6 = _pairs(1000 + n, COUNT, n)
    w6, Z6 = np.zeros((COUNT, n)), np.zeros((COUNT, n, n))
    for b in range(COUNT):
        w6[b], Z6[b] = sl.eigh(A6[b], B6[b], type=itype, lower=True)
    idx = np.array([0, 1, 2, 3, 4, 5, 0, 1])
    o = _uniform(lib, "device", itype, A6, B6, w6, Z6)
    _clean(o, COUNT)
    ref_out, ref_ipr = o.out[idx], o.ipr[idx]
    A, B, w, Z = A6[idx], B6[idx].copy(), w6[idx], Z6[idx].copy()
    others = np.arange(8) != 3
    # a failed problem: skipped, its arrays (full of NaN) are not looked at
    Z[3] = np.nan
    info = np.zeros(8, dtype=np.int32)
    info[3] = 5
    for run in (lambda: _uniform(lib, form, itype, A, B, w, Z, info=info),
                lambda: _variable(lib, form, itype, list(A), list(B), list(w), list(Z), info=info)):
        o = run()
        _clean(o, 8)
        assert np.all(np.isnan(o.out[3])) and np.all(np.asarray(o.ipr[3]) == SENTINEL)
        assert _same(o.out[others], ref_out[others])
        assert all(_same(np.asarray(o.ipr[b]), ref_ipr[b]) for b in range(8) if b != 3)
    # info = NULL: every problem is checked, the NaN of problem 3 stays in problem 3
    o = _uniform(lib, form, itype, A, B, w, Z)
    _clean(o, 8)
    assert o.out[3, 0] == ref_out[3, 0] and not np.isfinite(o.out[3, 1:]).any() and not np.isfinite(o.ipr[3]).any()
    assert _same(o.out[others], ref_out[others]) and _same(o.ipr[others], ref_ipr[others])
    # one NaN in Z of problem 5, info = 0: its outputs are not finite, the others unchanged, the call succeeds
    Z = Z6[idx].copy()
    Z[5, n // 2, n // 3] = np.nan
    others = np.arange(8) != 5
    o = _uniform(lib, form, itype, A, B, w, Z, info=np.zeros(8, dtype=np.int32))
    _clean(o, 8)
    assert not np.isfinite(o.out[5, 1:]).any() and np.isnan(o.ipr[5, n // 3])
    assert _same(o.out[others], ref_out[others]) and _same(o.ipr[others], ref_ipr[others])
    # a B that is not SPD (problem 2, a negative diagonal entry in the middle) under info = NULL: type 3 gives NaN in slot 3
    # and in the IPRs and the mirror's residual slots (type 2 needs no factor: its residual slots are the mirror's too)
    Z = Z6[idx]
    B[2, n // 2, n // 2] = -1.0
    others = np.arange(8) != 2
    o = _uniform(lib, form, itype, A, B, w, Z)
    _clean(o, 8)
    m_out, m_ipr = _mirror(itype, A[2], B[2], w[2], Z[2])
    tol = 4 * max(n, 8) * EPS
    assert np.all(np.isfinite(o.out[2, :3]))
    assert abs(o.out[2, 0] - m_out[0]) <= tol * m_out[0] and np.all(np.abs(o.out[2, 1:3] - m_out[1:3]) <= tol)
    if itype == 3:
        assert np.isnan(o.out[2, 3]) and np.all(np.isnan(o.ipr[2]))
        assert np.isnan(m_out[3]) and np.all(np.isnan(m_ipr))
    assert _same(o.out[others], ref_out[others]) and _same(o.ipr[others], ref_ipr[others])


# ------------------------------------------------------------------------------------------- 7: one-problem entries
@functools.lru_cache(maxsize=None)
def _single(n, itype):
    """One seeded pair of order n.  The bound on the IPRs is absolute and presumes IPRs of at most 1, as type 1 has them
    where B >= I: Z^T B Z = I bounds |z_j|^2 by 1 / lambda_min(B), and type 3's Z^T B^-1 Z = I by lambda_max(B).  So type 3
    takes B / 10 (spectrum in [0.1, 1]) where types 1 and 2 take B (spectrum in [1, 10]); otherwise an IPR of type 3
    reaches 100, whose last place is twice the bound at order 1."""
    A, B = _pairs(2000 + n, 1, n)
    B = B / 10.0 if itype == 3 else B
    for a in (A, B):
        a.setflags(write=False)
    return A[0], B[0]


def _padded(M, ld):
    X = np.full((ld, M.shape[1]), np.nan, order="F")
    X[:M.shape[0], :] = M
    return X


def _sygvx_check(lib, form, itype, A, B, w, Z, pad=3):
    """ek_hip_check_sygvx[_device] with lda / ldb / ldz = n + pad .., NaN in the rows below n and in the strictly upper
    triangles of A and B.  Returns (out, ipr); asserts that A, B, w and Z come back bit for bit."""
    n, m = Z.shape
    h = [_padded(_nan_upper(A), n + pad), _padded(_nan_upper(B), n + 2 * pad), np.array(w, dtype=np.float64),
         _padded(Z, n + 3 * pad)]
    out, q = np.full(6, SENTINEL), np.full(m + 2, SENTINEL)
    if form == "device":
        with _Dev(lib) as dev:
            d = [dev.up(x) for x in h]
            rc = lib.ek_hip_check_sygvx_device(itype, n, m, d[0], n + pad, d[1], n + 2 * pad, d[2], d[3], n + 3 * pad,
                                               out.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
            assert all(_same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [x.copy(order="K") for x in h]
        rc = lib.ek_hip_check_sygvx(itype, n, m, g[0].ctypes.data_as(_dp), n + pad, g[1].ctypes.data_as(_dp), n + 2 * pad,
                                    g[2].ctypes.data_as(_dp), g[3].ctypes.data_as(_dp), n + 3 * pad,
                                    out.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
        assert all(_same(y, x) for y, x in zip(g, h))
    assert rc == 0 and np.all(out[4:] == SENTINEL) and np.all(q[m:] == SENTINEL)
    return out[:4], q[:m]


@forms
@types23
@pytest.mark.parametrize("n", (1, 5, 129, 300, 515))
def test_one_problem_matches_the_host_mirror(hip, n, itype, form):
    """The first n_cols < n columns of SciPy's eigenvectors (n_cols = 1 at order 1), leading dimensions beyond n."""
    lib = hip.load_library()
    A, B = _single(n, itype)
    w, Z = sl.eigh(A, B, type=itype, lower=True)
    m = max(1, (2 * n) // 3)
    out, q = _sygvx_check(lib, form, itype, A, B, w[:m], Z[:, :m])
    m_out, m_ipr = _mirror(itype, A, B, w[:m], Z[:, :m])
    cond = np.linalg.cond(B)
    assert cond <= 16.0
    _assert_shares(_shares(itype, out, q, m_out, m_ipr, n, cond), ("one problem", n, m, itype, form))
    # the same detection as in the batches: a duplicate column and a moved eigenvalue show to the mirror's value
    if m >= 2:
        Zd, wd = Z[:, :m].copy(), w[:m].copy()
        Zd[:, 0] = Zd[:, 1]
        wd[m - 1] += 1e-6 * abs(wd[m - 1])
        out, q = _sygvx_check(lib, form, itype, A, B, wd, Zd)
        m_out, m_ipr = _mirror(itype, A, B, wd, Zd)
        assert out[3] > 1.4 and out[2] >= 0.99e-6 * abs(wd[m - 1]) / m_out[0]
        _assert_shares(_shares(itype, out, q, m_out, m_ipr, n, cond), ("one problem, planted", n, m, itype, form))


@pytest.mark.parametrize("n", (5, 129, 300))
def test_one_problem_itype_1_is_the_three_existing_entries(hip, n):
    lib = hip.load_library()
    A, B = _single(n, 1)
    w, Z = sl.eigh(A, B, lower=True)
    m = (2 * n) // 3
    Zp = Z[:, :m] + 1e-4 * np.random.default_rng(n).standard_normal((n, m))
    with _Dev(lib) as dev:
        dA, dB = dev.up(np.asfortranarray(A)), dev.up(np.asfortranarray(B))
        dw, dZ = dev.up(np.ascontiguousarray(w[:m])), dev.up(np.asfortranarray(Zp))
        out, q = np.zeros(4), np.zeros(m)
        assert lib.ek_hip_check_sygvx_device(1, n, m, dA, n, dB, n, dw, dZ, n, out.ctypes.data_as(_dp),
                                             q.ctypes.data_as(_dp)) == 0
        r = [ctypes.c_double() for _ in range(4)]
        q0 = np.zeros(m)
        assert lib.ek_hip_residual_device(1, n, m, dA, n, dB, n, dw, dZ, n, ctypes.byref(r[0]), ctypes.byref(r[1]),
                                          ctypes.byref(r[2])) == 0
        assert lib.ek_hip_orthogonality_device(1, n, 1, m, dB, n, dZ, n, ctypes.byref(r[3])) == 0
        assert lib.ek_hip_ipratios_device(1, n, m, dB, n, dZ, n, q0.ctypes.data_as(_dp)) == 0
    assert _same(out, np.array([x.value for x in r])) and _same(q, q0)
    assert out[1] > 1e-6 and out[3] > 1e-4              # the perturbation shows: these are not rounding noise


@types23
@pytest.mark.parametrize("n", (129, 515))
def test_one_problem_behind_sygvx_with_an_index_window(hip, n, itype):
    """ek_hip_sygvx_device for the eigenpairs il .. iu on copies, its w and Z checked where they lie: res_max and
    orthogonality within 256 n eps (the bound of item 4: the window's vectors obey the same contract as the batch's), and
    the mirror's values on the same w and Z."""
    lib = hip.load_library()
    A, B = _single(n, itype)
    il, iu = n // 4, n // 4 + n // 3
    cap = iu - il + 1
    hA, hB = np.asfortranarray(A), np.asfortranarray(B)
    out, q = np.zeros(4), np.zeros(cap)
    m, ifirst = ctypes.c_int(0), ctypes.c_int(0)
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        hw, hZ = np.zeros(cap), np.zeros((n, cap), order="F")
        dw, dZ = dev.up(hw), dev.up(hZ)
        assert lib.ek_hip_sygvx_device(itype, 1, 0, n, 0.0, 0.0, il, iu, dA, n, dB, n, ctypes.byref(m),
                                       ctypes.byref(ifirst), dw, dZ, n, cap, None, 0) == 0
        assert m.value == cap
        assert lib.ek_hip_check_sygvx_device(itype, n, cap, dA0, n, dB0, n, dw, dZ, n, out.ctypes.data_as(_dp),
                                             q.ctypes.data_as(_dp)) == 0
        w, Z = dev.down(dw, hw), dev.down(dZ, hZ)
    lim = 256 * n * EPS
    print("behind sygvx %s: res_max %.3f, orthogonality %.3f of 256 n eps" % ((n, itype), out[2] / lim, out[3] / lim))
    assert out[2] <= lim and out[1] <= out[2] and out[3] <= lim
    m_out, m_ipr = _mirror(itype, A, B, w, Z)
    _assert_shares(_shares(itype, out, q, m_out, m_ipr, n, np.linalg.cond(B)), ("behind sygvx", n, itype))


# ---------------------------------------------------------------------------------------------------------- 8: cost
@types23
@pytest.mark.parametrize("n,batch", [(64, 1024), (128, 512)])
def test_the_check_costs_no_more_than_the_solve(hip, n, batch, itype):
    """Best of 3 of the check's device time against best of 3 of ek_hip_sygv_batched_device's on the same batch,
    alternated, after one warm-up of each; the type-1 check of the same batch is timed beside them and its ratio printed
    (no number is asserted for it)."""
    lib = hip.load_library()
    A16, B16 = _pairs(4242 + n, 16, n)
    A, B = np.tile(A16, (batch // 16, 1, 1)), np.tile(B16, (batch // 16, 1, 1))
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    out, q = np.zeros(batch * 4), np.zeros(batch * n)
    out1, q1 = np.zeros(batch * 4), np.zeros(batch * n)
    info = np.zeros(batch, dtype=np.int32)
    t_solve, t_check, t_one = [], [], []
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_sygv_batched_device(itype, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                  info.ctypes.data_as(_ip), ctypes.byref(sec)) == 0
            assert not info.any()
            t_solve.append(sec.value)
            for first, o_, q_, ts in ((itype, out, q, t_check), (1, out1, q1, t_one)):
                sec = ctypes.c_double(-1.0)
                assert lib.ek_hip_check_sygv_batched_device(first, n, batch, dA0, n, n * n, dB0, n, n * n, dw, dZ, n,
                                                            n * n, info.ctypes.data_as(_ip), o_.ctypes.data_as(_dp),
                                                            q_.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
                ts.append(sec.value)
    o = out.reshape(batch, 4)
    assert np.all(o[:, 2] <= 256 * n * EPS) and np.all(o[:, 3] <= 256 * n * EPS)
    ts, tc, t1 = min(t_solve[1:]), min(t_check[1:]), min(t_one[1:])
    print("cost itype=%d n=%d batch=%d: solve %.3f ms, check %.3f ms (%.3f of the solve), type-1 check %.3f ms (ratio %.2f)"
          % (itype, n, batch, ts * 1e3, tc * 1e3, tc / ts, t1 * 1e3, tc / t1))
    assert 0.0 < tc <= ts, (tc, ts)
