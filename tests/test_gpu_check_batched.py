"""GPU suite of the batched acceptance checks (ek_hip_check_batched*, ek_hip_check_vbatched*): a_norm, res_ave, res_max,
orthogonality and the inverse participation ratios of every problem of a batch, a workgroup per problem.

The yardstick is the host mirror eigenkernel_amd/verifier.py in float64, on the seeded _sym / _spd (cond 10) inputs of
tests/test_gpu_batched.py (helpers copied from there).  The tolerance is 4 max(n, 8) eps -- absolute for res_ave, res_max
and orthogonality, relative for a_norm and every IPR: two float64 evaluations in different summation orders each lie
within 0.45 max(n, 8) eps of a long-double evaluation on these inputs (measured on the CPU, both problems, with and
without the perturbation, the IPR of the generalized problem being the worst), so they differ by less than one unit and
4 leaves a fourfold margin for the GPU's order and its fused multiply-adds.  Every test runs in four ways: both problems,
device and host form.  Each test prints the largest share of the tolerance it used (pytest -s shows it)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.linalg as sl

from eigenkernel_amd import verifier
from eigenkernel_amd.matrix_io import read_matrix_file

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
UNIFORM = (1, 2, 3, 31, 32, 33, 64, 65, 127, 128)
VARIABLE = (0, 1, 2, 3, 17, 30, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128)
SENTINEL = -7.25e77
NAMES = ("a_norm", "res_ave", "res_max", "orthogonality")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
WAYS = [(0, "device"), (0, "host"), (1, "device"), (1, "host")]
ways = pytest.mark.parametrize("problem,form", WAYS)


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
def _cases(n, problem, count=6):
    """count seeded problems of order n: A, B (None for problem 0), SciPy's w and Z, and Z perturbed by
    1e-3 N(0, 1) / sqrt(n) per entry, which puts res_* near 1e-4 and orthogonality near 1e-2.  Read only."""
    A, B = _pairs(1000 + n, count, n) if n else (np.zeros((count, 0, 0)), np.zeros((count, 0, 0)))
    w, Z = np.zeros((count, n)), np.zeros((count, n, n))
    if n:
        for b in range(count):
            w[b], Z[b] = sl.eigh(A[b], B[b], lower=True) if problem else sl.eigh(A[b], lower=True)
    rng = np.random.default_rng(77000 + 2 * n + problem)
    Zp = Z + 1e-3 * rng.standard_normal(Z.shape) / np.sqrt(max(n, 1))
    c = _Out()
    c.n, c.A, c.B, c.w, c.Z, c.Zp = n, A, (B if problem else None), w, Z, Zp
    for a in (A, B, w, Z, Zp):
        a.setflags(write=False)
    return c


def _mirror(A, B, w, Z):
    a_norm, ave, mx = verifier.eval_residual_norm(A, w, Z, B)
    return np.array([a_norm, ave, mx, verifier.eval_orthogonality(Z, B)]), verifier.get_ipratios(Z, B)


@functools.lru_cache(maxsize=None)
def _mirror_cases(n, problem):
    c = _cases(n, problem)
    return [_mirror(c.A[b], c.B[b] if problem else None, c.w[b], c.Zp[b]) for b in range(c.A.shape[0])]


def _tol(n):
    return 4 * max(n, 8) * EPS


def _shares(out, ipr, ref_out, ref_ipr, n):
    """|difference| / tolerance per quantity: a_norm and the IPRs relative, the other three absolute."""
    tol = _tol(n)
    s = np.abs(out - ref_out) / tol
    s[0] /= abs(ref_out[0])
    return np.append(s, (np.abs(ipr - ref_ipr) / np.abs(ref_ipr)).max() / tol if n else 0.0)


def _assert_shares(shares, what):
    shares = np.asarray(shares).reshape(-1, 5).max(axis=0)
    print("shares of the tolerance %s: " % (what,) + ", ".join("%s %.3f" % kv for kv in zip(NAMES + ("ipr",), shares)))
    assert np.all(shares <= 1.0), (what, shares)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- the calls
def _uniform(lib, form, problem, A, B, w, Z, info=None, ipr=True, pad=0, fill=SENTINEL):
    """ek_hip_check_batched[_device] on strided images of A[b], B[b], Z[b] (full matrices: both triangles as given):
    pad = 0 the compact layout, pad > 0 leading dimensions n + pad .. and strides beyond ld * n, the gaps holding
    `fill`.  o.untouched: the images of A, B, w, Z after the call equal those before it, byte for byte."""
    batch, n = A.shape[0], A.shape[1]
    lda, ldb, ldz = (n + pad, n + 2 * pad, n + 3 * pad) if pad else (n, n, n)
    sA, sB, sZ = lda * n + (5 if pad else 0), ldb * n + (3 if pad else 0), ldz * n + (7 if pad else 0)
    h = [_pack(A, lda, sA, fill), _pack(B, ldb, sB, fill) if problem else None,
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
            d = [dev.up(x) if x is not None else None for x in h]
            o.rc = lib.ek_hip_check_batched_device(problem, n, batch, d[0], lda, sA, d[1], ldb, sB, d[2], d[3], ldz, sZ,
                                                   *tail)
            o.untouched = all(x is None or _same(dev.down(p, x), x) for p, x in zip(d, h))
    else:
        g = [None if x is None else x.copy() for x in h]
        P = [None if x is None else x.ctypes.data_as(_dp) for x in g]
        o.rc = lib.ek_hip_check_batched(problem, n, batch, P[0], lda, sA, P[1], ldb, sB, P[2], P[3], ldz, sZ, *tail)
        o.untouched = all(x is None or _same(y, x) for y, x in zip(g, h))
    o.seconds = sec.value
    o.out, o.ipr = out[:batch * 4].reshape(batch, 4), q[:batch * n].reshape(batch, n)
    o.tails = (out[batch * 4:], q[batch * n:] if ipr else q)
    if iarr is not None:
        assert np.array_equal(iarr, np.asarray(info, dtype=np.int32))
    return o


def _variable(lib, form, problem, As, Bs, ws, Zs, info=None, ipr=True, pad=0, fill=SENTINEL, no_ipr=()):
    """ek_hip_check_vbatched[_device]: problem b in its own column-major array with leading dimension max(1, n[b]) +
    pad (A), + 2 pad (B), + 3 pad (Z), the rows below n[b] holding `fill`; ipr[b] has two slots more than n[b], and the
    problems listed in no_ipr pass a NULL entry."""
    batch = len(As)
    n = np.array([M.shape[0] for M in As], dtype=np.int32)
    lds = [np.maximum(n, 1).astype(np.int32) + k * pad for k in (1, 2, 3)]

    def image(M, ld):
        X = np.full((ld, M.shape[0]), fill, order="F")
        X[:M.shape[0], :] = M
        return X

    h = [[image(M, lds[0][b]) for b, M in enumerate(As)],
         [image(M, lds[1][b]) for b, M in enumerate(Bs)] if problem else None,
         [np.array(v, dtype=np.float64) for v in ws], [image(M, lds[2][b]) for b, M in enumerate(Zs)]]
    out = np.full(batch * 4 + 2, SENTINEL)
    qs = [np.full(k + 2, SENTINEL) for k in n]
    iarr = None if info is None else np.asarray(info, dtype=np.int32).copy()
    sec = ctypes.c_double(-1.0)
    o = _Out()

    def table(ptrs):
        return (ctypes.c_void_p * batch)(*ptrs)

    def call(fn, P):
        return fn(problem, batch, n.ctypes.data_as(_ip), table(P[0]), lds[0].ctypes.data_as(_ip),
                  table(P[1]) if problem else None, lds[1].ctypes.data_as(_ip), table(P[2]), table(P[3]),
                  lds[2].ctypes.data_as(_ip), None if iarr is None else iarr.ctypes.data_as(_ip),
                  out.ctypes.data_as(_dp),
                  table([None if b in no_ipr else qs[b].ctypes.data for b in range(batch)]) if ipr else None,
                  ctypes.byref(sec))

    if form == "device":
        with _Dev(lib) as dev:
            d = [None if k is None else [dev.up(x) if x.size else None for x in k] for k in h]
            o.rc = call(lib.ek_hip_check_vbatched_device, [None if k is None else [p.value if p else None for p in k]
                                                           for k in d])
            o.untouched = all(_same(dev.down(p, x), x) for k, hk in zip(d, h) if k is not None
                              for p, x in zip(k, hk) if p is not None)
    else:
        g = [None if k is None else [x.copy(order="K") for x in k] for k in h]
        o.rc = call(lib.ek_hip_check_vbatched, [None if k is None else [x.ctypes.data if x.size else None for x in k]
                                                for k in g])
        o.untouched = all(_same(y, x) for k, hk in zip(g, h) if k is not None for y, x in zip(k, hk))
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


def _reference_bits(lib, n, problem):
    """The six perturbed cases of order n through the uniform device form in the compact layout, once: what every
    other form, layout, position and batch must reproduce bit for bit."""
    key = (n, problem)
    if key not in _plain:
        c = _cases(n, problem)
        o = _uniform(lib, "device", problem, c.A, c.B, c.w, c.Zp)
        _clean(o, 6)
        o.out.setflags(write=False)
        o.ipr.setflags(write=False)
        _plain[key] = (o.out, o.ipr)
    return _plain[key]


# ------------------------------------------------------------------- 1: against the host mirror, above rounding noise
@ways
@pytest.mark.parametrize("n", UNIFORM)
def test_uniform_matches_the_host_mirror(hip, n, problem, form):
    lib = hip.load_library()
    c = _cases(n, problem)
    o = _uniform(lib, form, problem, c.A, c.B, c.w, c.Zp)
    _clean(o, 6)
    ref = _mirror_cases(n, problem)
    if n >= 31:                                     # the perturbation shows: these are not rounding noise
        assert 1e-6 < o.out[:, 1].min() and 1e-4 < o.out[:, 3].min()
    _assert_shares([_shares(o.out[b], o.ipr[b], ref[b][0], ref[b][1], n) for b in range(6)], (n, problem, form))


@ways
def test_variable_matches_the_host_mirror(hip, problem, form):
    """Six problems of every variable order in one call (96 problems, at most three launches)."""
    lib = hip.load_library()
    sel = [(n, b) for b in range(6) for n in VARIABLE]
    cs = {n: _cases(n, problem) for n in VARIABLE}
    o = _variable(lib, form, problem, [cs[n].A[b] for n, b in sel], [cs[n].B[b] for n, b in sel] if problem else None,
                  [cs[n].w[b] for n, b in sel], [cs[n].Zp[b] for n, b in sel])
    _clean(o, len(sel))
    shares = []
    for k, (n, b) in enumerate(sel):
        if n == 0:
            assert o.out[k, 0] == 0.0 and np.all(np.isnan(o.out[k, 1:])) and o.ipr[k].size == 0
            continue
        ref = _mirror_cases(n, problem)[b]
        shares.append(_shares(o.out[k], o.ipr[k], ref[0], ref[1], n))
    _assert_shares(shares, ("variable", problem, form))


# ---------------------------------------------------------------------------- 2: end to end behind the batched solver
_solved = {}


def _solver_pairs(hip, n, problem):
    key = (n, problem)
    if key not in _solved:
        c = _cases(n, problem)
        w, Z, info = hip.eigenpairs_batched(c.A, c.B)
        assert not info.any()
        _solved[key] = (w, Z, [_mirror(c.A[b], c.B[b] if problem else None, w[b], Z[b])[1] for b in range(6)])
    return _solved[key]


@ways
@pytest.mark.parametrize("n", UNIFORM)
def test_end_to_end_behind_the_batched_solver(hip, n, problem, form):
    """The batched solver's own w and Z on the unperturbed pairs: the suite's bounds on res_max (64 n eps) and
    orthogonality (256 n eps), and the IPR within the tolerance of the mirror on the same Z."""
    lib = hip.load_library()
    c = _cases(n, problem)
    w, Z, ipr_ref = _solver_pairs(hip, n, problem)
    o = _uniform(lib, form, problem, c.A, c.B, w, Z)
    _clean(o, 6)
    assert np.all(o.out[:, 2] <= 64 * n * EPS), (o.out[:, 2].max(), 64 * n * EPS)
    assert np.all(o.out[:, 1] <= o.out[:, 2])
    assert np.all(o.out[:, 3] <= 256 * n * EPS), (o.out[:, 3].max(), 256 * n * EPS)
    share = max((np.abs(o.ipr[b] - ipr_ref[b]) / np.abs(ipr_ref[b])).max() for b in range(6)) / _tol(n)
    print("end to end %s: res_max %.2e of 64 n eps, orthogonality %.2e of 256 n eps, ipr share %.3f"
          % ((n, problem, form), o.out[:, 2].max() / (64 * n * EPS), o.out[:, 3].max() / (256 * n * EPS), share))
    assert share <= 1.0


# ----------------------------------------------------------------------------------------------------- 3: closed forms
@ways
@pytest.mark.parametrize("n", UNIFORM)
def test_closed_forms(hip, n, problem, form):
    lib = hip.load_library()
    tol = _tol(n)
    eye = np.eye(n)
    k = np.arange(1.0, n + 1)
    flat = eye.copy()                               # columns 0 and 1 (the same vector twice): ones / sqrt(n)
    flat[:, :2] = 1.0 / np.sqrt(n)
    c = _cases(n, problem)
    A = np.stack([np.diag(k), np.diag(k), c.A[0], c.A[0]])
    B = np.stack([eye, eye, c.B[0], c.B[0]]) if problem else None
    w = np.stack([k, k, c.w[0], c.w[0]])
    Z = np.stack([eye, flat, c.Zp[0], 3.0 * c.Zp[0]])
    o = _uniform(lib, form, problem, A, B, w, Z)
    _clean(o, 4)
    # A = diag(1..n), B = I, Z = I, w = 1..n
    assert abs(o.out[0, 0] - np.sqrt((k * k).sum())) <= tol * np.sqrt((k * k).sum())
    assert o.out[0, 1] == 0.0 and o.out[0, 2] == 0.0 and o.out[0, 3] == 0.0
    assert np.all(o.ipr[0] == 1.0)
    # Z = ones / sqrt(n): IPR = 1 / n; a duplicated column: orthogonality > 1
    assert np.all(np.abs(o.ipr[1][:2] * n - 1.0) <= tol) and np.all(o.ipr[1][2:] == 1.0)
    if n >= 2:
        assert o.out[1, 3] > 1.0
    # the orthogonality check scales by the computed G_jj: 3 Z gives what Z gives
    assert abs(o.out[3, 3] - o.out[2, 3]) <= tol
    assert np.all(np.abs(o.ipr[3] - o.ipr[2]) <= tol * np.abs(o.ipr[2]))


# ----------------------------------------------------------------------------------------------- 4: the reference's pair
@ways
def test_reference_pair_bnz30(hip, golden_dir, problem, form):
    """64 copies of the shipped BNZ30 pair through the batched solve and the batched check: the same bits 64 times, and
    (generalized, as the reference ran it) the IPR within 1e-6 of its ipratios.dat -- the tolerance of
    test_gpu_ipr_matches_reference_golden in tests/test_gpu_path.py, which says why."""
    lib = hip.load_library()
    A = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_A.mtx")).to_dense()
    B = read_matrix_file(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_B.mtx")).to_dense() if problem else None
    A3 = np.stack([A] * 64)
    B3 = np.stack([B] * 64) if problem else None
    w, Z, info = hip.eigenpairs_batched(A3, B3)
    assert not info.any()
    o = _uniform(lib, form, problem, A3, B3, w, Z)
    _clean(o, 64)
    for b in range(1, 64):
        assert _same(o.out[b], o.out[0]) and _same(o.ipr[b], o.ipr[0])
    n = A.shape[0]
    assert o.out[0, 2] <= 64 * n * EPS and o.out[0, 3] <= 256 * n * EPS
    ref = _mirror(A, B, w[0], Z[0])
    _assert_shares(_shares(o.out[0], o.ipr[0], ref[0], ref[1], n), ("BNZ30", problem, form))
    if problem:
        gold = np.loadtxt(os.path.join(golden_dir, "ELSES_MATRIX_BNZ30_ipr.txt"))[:, 1]
        assert np.abs(o.ipr[0] - gold).max() <= 1e-6


# ------------------------------------------------------------------------------ 5: against the one-problem GPU verifier
@ways
@pytest.mark.parametrize("n", (30, 64, 128))
def test_against_the_one_problem_verifier(hip, n, problem, form):
    lib = hip.load_library()
    c = _cases(n, problem)
    o = _uniform(lib, form, problem, c.A[:2], c.B[:2] if problem else None, c.w[:2], c.Zp[:2])
    _clean(o, 2)
    shares = []
    for b in range(2):
        with _Dev(lib) as dev:
            dA = dev.up(np.asfortranarray(c.A[b]))
            dB = dev.up(np.asfortranarray(c.B[b])) if problem else None
            dw, dZ = dev.up(np.ascontiguousarray(c.w[b])), dev.up(np.asfortranarray(c.Zp[b]))
            r = [ctypes.c_double() for _ in range(3)]
            orth = ctypes.c_double()
            q = np.zeros(n)
            assert lib.ek_hip_residual_device(problem, n, n, dA, n, dB, n, dw, dZ, n, ctypes.byref(r[0]),
                                              ctypes.byref(r[1]), ctypes.byref(r[2])) == 0
            assert lib.ek_hip_orthogonality_device(problem, n, 1, n, dB, n, dZ, n, ctypes.byref(orth)) == 0
            assert lib.ek_hip_ipratios_device(problem, n, n, dB, n, dZ, n, q.ctypes.data_as(_dp)) == 0
        shares.append(_shares(o.out[b], o.ipr[b], np.array([r[0].value, r[1].value, r[2].value, orth.value]), q, n))
    _assert_shares(shares, ("one-problem verifier", n, problem, form))


# ------------------------------------------------------------------------------ 6: the same bits wherever a problem sits
@ways
@pytest.mark.parametrize("n", (31, 64, 127))
def test_same_bits_at_any_position_of_any_batch(hip, n, problem, form):
    lib = hip.load_library()
    c = _cases(n, problem)
    ref_out, ref_ipr = _reference_bits(lib, n, problem)
    o = _uniform(lib, form, problem, c.A[:1], c.B[:1] if problem else None, c.w[:1], c.Zp[:1])
    _clean(o, 1)
    assert _same(o.out[0], ref_out[0]) and _same(o.ipr[0], ref_ipr[0])
    for batch in (8, 300):
        idx = np.array([(3 * b + 1) % 5 + 1 for b in range(batch)])      # filler: cases 1 .. 5
        spots = (0, 7, batch - 1)
        idx[list(spots)] = 0
        o = _uniform(lib, form, problem, c.A[idx], c.B[idx] if problem else None, c.w[idx], c.Zp[idx])
        _clean(o, batch)
        assert _same(o.out, ref_out[idx]) and _same(o.ipr, ref_ipr[idx])


@ways
def test_same_bits_through_the_variable_form(hip, problem, form):
    """Every variable order in one call, in two permutations: each problem's bits are the uniform call's."""
    lib = hip.load_library()
    rng = np.random.default_rng(5)
    for perm in (np.arange(len(VARIABLE)), rng.permutation(len(VARIABLE))):
        orders = [VARIABLE[k] for k in perm]
        cs = [_cases(n, problem) for n in orders]
        o = _variable(lib, form, problem, [c.A[0] for c in cs], [c.B[0] for c in cs] if problem else None,
                      [c.w[0] for c in cs], [c.Zp[0] for c in cs])
        _clean(o, len(orders))
        for k, n in enumerate(orders):
            if n == 0:
                assert o.out[k, 0] == 0.0 and np.all(np.isnan(o.out[k, 1:]))
                continue
            ref_out, ref_ipr = _reference_bits(lib, n, problem)
            assert _same(o.out[k], ref_out[0]) and _same(o.ipr[k], ref_ipr[0]), (n, k)


# --------------------------------------------------------------------- 7: what is not referenced, what is not written
def _nan_upper(M):
    X = np.array(M, dtype=np.float64)
    iu = np.triu_indices(X.shape[-1], 1)
    X[..., iu[0], iu[1]] = np.nan
    return X


@ways
@pytest.mark.parametrize("n", (1, 3, 32, 33, 65, 128))
def test_upper_triangles_and_padding_are_not_referenced(hip, n, problem, form):
    """NaN in the strictly upper triangles of A and B, in the rows n .. ld-1 and between the problems; ld > n and strides
    beyond ld * n: the bits of the clean compact layout.  A, B, w and Z come back byte for byte (o.untouched), and the
    slots behind out and ipr keep their sentinel (_clean)."""
    lib = hip.load_library()
    c = _cases(n, problem)
    ref_out, ref_ipr = _reference_bits(lib, n, problem)
    o = _uniform(lib, form, problem, _nan_upper(c.A), _nan_upper(c.B) if problem else None, c.w, c.Zp, pad=3,
                 fill=np.nan)
    _clean(o, 6)
    assert _same(o.out, ref_out) and _same(o.ipr, ref_ipr)
    o = _variable(lib, form, problem, list(_nan_upper(c.A)), list(_nan_upper(c.B)) if problem else None, list(c.w),
                  list(c.Zp), pad=2, fill=np.nan, no_ipr=(4,))
    _clean(o, 6)
    assert _same(o.out, ref_out)
    for b in range(6):
        assert np.all(o.ipr[b] == SENTINEL) if b == 4 else _same(o.ipr[b], ref_ipr[b])
    o = _uniform(lib, form, problem, c.A, c.B, c.w, c.Zp, ipr=False)        # ipr = NULL
    _clean(o, 6)
    assert _same(o.out, ref_out) and np.all(o.ipr == SENTINEL)


# ------------------------------------------------------------------------------------------- 8: per-problem isolation
@ways
@pytest.mark.parametrize("n", (30, 64, 100))
def test_per_problem_isolation(hip, n, problem, form):
    lib = hip.load_library()
    c = _cases(n, problem)
    idx = np.array([0, 1, 2, 3, 4, 5, 0, 1])
    ref_out, ref_ipr = _reference_bits(lib, n, problem)
    ref_out, ref_ipr = ref_out[idx], ref_ipr[idx]
    A, B, w, Z = c.A[idx], (c.B[idx] if problem else None), c.w[idx], c.Zp[idx].copy()
    others = np.arange(8) != 3
    # a failed problem: skipped, its Z (full of NaN) is not looked at
    Z[3] = np.nan
    info = np.zeros(8, dtype=np.int32)
    info[3] = 5
    for run in (lambda: _uniform(lib, form, problem, A, B, w, Z, info=info),
                lambda: _variable(lib, form, problem, list(A), list(B) if problem else None, list(w), list(Z),
                                  info=info)):
        o = run()
        _clean(o, 8)
        assert np.all(np.isnan(o.out[3])) and np.all(np.asarray(o.ipr[3]) == SENTINEL)
        assert _same(o.out[others], ref_out[others])
        assert all(_same(np.asarray(o.ipr[b]), ref_ipr[b]) for b in range(8) if b != 3)
    # info = NULL: every problem is checked, the NaN of problem 3 stays in problem 3
    o = _uniform(lib, form, problem, A, B, w, Z)
    _clean(o, 8)
    assert o.out[3, 0] == ref_out[3, 0] and not np.isfinite(o.out[3, 1:]).any() and not np.isfinite(o.ipr[3]).any()
    assert _same(o.out[others], ref_out[others]) and _same(o.ipr[others], ref_ipr[others])
    # one NaN in Z of problem 5, info = 0: its outputs are not finite, the others unchanged, the call succeeds
    Z = c.Zp[idx].copy()
    Z[5, n // 2, n // 3] = np.nan
    others = np.arange(8) != 5
    o = _uniform(lib, form, problem, A, B, w, Z, info=np.zeros(8, dtype=np.int32))
    _clean(o, 8)
    assert not np.isfinite(o.out[5, 1:]).any() and np.isnan(o.ipr[5, n // 3])
    assert _same(o.out[others], ref_out[others]) and _same(o.ipr[others], ref_ipr[others])


@ways
def test_orders_zero_and_one_and_a_zero_matrix(hip, problem, form):
    lib = hip.load_library()
    c1, c3 = _cases(1, problem), _cases(33, problem)
    e = np.zeros((0, 0))
    As = [e, c1.A[0], np.zeros((33, 33)), c3.A[1], e]
    Bs = [e, c1.B[0], c3.B[0], c3.B[1], e] if problem else None
    o = _variable(lib, form, problem, As, Bs, [np.zeros(0), c1.w[0], c3.w[0], c3.w[1], np.zeros(0)],
                  [e, c1.Zp[0], c3.Zp[0], c3.Zp[1], e], info=[0, 0, 0, 0, 9])
    _clean(o, 5)
    assert o.out[0, 0] == 0.0 and np.all(np.isnan(o.out[0, 1:]))          # order 0: 0 / 0
    assert np.all(np.isnan(o.out[4]))                                      # order 0 and skipped
    r1 = _reference_bits(lib, 1, problem)
    r3 = _reference_bits(lib, 33, problem)
    assert _same(o.out[1], r1[0][0]) and _same(o.ipr[1], r1[1][0])
    assert _same(o.out[3], r3[0][1]) and _same(o.ipr[3], r3[1][1])
    # A = 0: a_norm = 0 and plain IEEE divisions; what does not depend on A is what the nonzero A gave
    assert o.out[2, 0] == 0.0 and not np.isfinite(o.out[2, 1:3]).any()
    assert _same(o.out[2, 3:], r3[0][0, 3:]) and _same(o.ipr[2], r3[1][0])
    # a zero column of Z: NaN in orthogonality and in its own IPR slot only
    Z = c3.Zp[:1].copy()
    Z[0, :, 7] = 0.0
    o = _uniform(lib, form, problem, c3.A[:1], c3.B[:1] if problem else None, c3.w[:1], Z)
    _clean(o, 1)
    assert np.isnan(o.out[0, 3]) and np.isfinite(o.out[0, :3]).all()
    assert np.isnan(o.ipr[0, 7]) and np.isfinite(np.delete(o.ipr[0], 7)).all()


# ---------------------------------------------------------------------------------------------------------- 9: cost
@pytest.mark.parametrize("n,batch", [(64, 1024), (128, 512)])
def test_the_check_costs_no_more_than_the_solve(hip, n, batch):
    """Generalized pairs with vectors: best of 3 of the check's device time against best of 3 of the solver's on the same
    arrays, alternated, after one warm-up of each.  The solver entry is the only other device-time number a batched
    caller has, and this change does not touch it."""
    lib = hip.load_library()
    A16, B16 = _pairs(4242 + n, 16, n)
    A, B = np.tile(A16, (batch // 16, 1, 1)), np.tile(B16, (batch // 16, 1, 1))
    hA, hB = _pack(A, n, n * n), _pack(B, n, n * n)
    out, q = np.zeros(batch * 4), np.zeros(batch * n)
    info = np.zeros(batch, dtype=np.int32)
    t_solve, t_check = [], []
    with _Dev(lib) as dev:
        dA0, dB0, dA, dB = dev.up(hA), dev.up(hB), dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        for it in range(4):
            dev.put(dA, hA)
            dev.put(dB, hB)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_eigenpairs_batched_device(1, 1, n, batch, dA, n, n * n, dB, n, n * n, dw, dZ, n, n * n,
                                                        info.ctypes.data_as(_ip), ctypes.byref(sec)) == 0
            assert not info.any()
            t_solve.append(sec.value)
            sec = ctypes.c_double(-1.0)
            assert lib.ek_hip_check_batched_device(1, n, batch, dA0, n, n * n, dB0, n, n * n, dw, dZ, n, n * n,
                                                   info.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                                                   q.ctypes.data_as(_dp), ctypes.byref(sec)) == 0
            t_check.append(sec.value)
    o = out.reshape(batch, 4)
    assert np.all(o[:, 2] <= 64 * n * EPS) and np.all(o[:, 3] <= 256 * n * EPS)
    ts, tc = min(t_solve[1:]), min(t_check[1:])
    print("cost n=%d batch=%d: solve %.3f ms, check %.3f ms, ratio %.3f" % (n, batch, ts * 1e3, tc * 1e3, tc / ts))
    assert 0.0 < tc <= ts, (tc, ts)
