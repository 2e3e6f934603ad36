"""Inputs, mirrors of the geometry, references and bounds of the stage tests of the bulge chasing and of Q2's application
(ek_sb2st.hip): tests/test_sb2st_cases_host.py (no GPU) and tests/test_gpu_sb2st_stages.py.

The stage: a symmetric band Bd of half width 64 -> T = Q2^T Bd Q2 tridiagonal, Q2 = prod_s prod_k H(s, k) in sweep order
(s ascending, inside a sweep k ascending), H(s, k) = I - tau v v^T on rows s+1+64k .. min(s+64(k+1), n-1); task (s, k)
exists iff s+1+64k <= n-2.  The stage leaves the reflectors in V2 (column s = the reflectors of sweep s stacked) and tau2
(entry [k, s]); Z <- Q2 Z applies them in blocks of 32 sweeps, NBLK blocks per pass, 64 columns per slab.

Band classes (band(cls, n), seeded, symmetric, nothing outside the 64 sub-diagonals):
    random, graded (s_i s_j, s = 10**(-8 i / n)), graded_up (s reversed), entrywise (every entry times its own
    10**U(-12, 0)), big and tiny (x 1e80, x 1e-80), width5, width63, outer_only (the diagonal and the 64th sub-diagonal:
    most reflectors are the identity), zero_columns (every third column of the lower band zero below the diagonal),
    near_identity (I + 1e-10 band), outlier (one diagonal entry 1e8), ones, and dead_first_column_<amp> (random with
    B[1:65, 0] = amp U(0.5, 1), amp 1e-158, 1e-160, 1e-161: the squares are denormal, the drop rule of reflector_of must
    make reflector (0, 0) the identity).

References, numpy.longdouble, plain and sequential, from the DEVICE's V2 and tau2 (so the chase and the application of Q2
are judged separately): sim applies the reflectors two-sidedly to Bd, one rank-1 update each side, in sweep order, inside
the window of +-128 columns outside which a reflector meets exact zeros; apply forms Q2 Z on sample columns, the last
reflector first; apply_t forms Q2^T Z.  From order 322 on the residual and the orthogonality are taken on 8 sample
columns of Q2 (sub-blocks of the same matrices, so the same bounds hold).

Bounds, m = max(n, 32) (the float64 emulation below spends at most 0.062 / 0.180 / 0.117 of the first three and 3.5 eps
of the 16 eps, over every class at every order of CHASE_CASES; the kernels may sum in another order and keep a factor
of four):
    ||sim - T||_F <= m eps ||Bd||_F            ||Q2^T Q2 - I||_F <= 2 m eps            |Z - ref| <= m eps max|ref| per column
    per live reflector v_0 == 1, max|v| <= 1, 1 <= tau <= 2, |tau v^T v - 2| <= 16 eps
    zero outside a reflector's rows; a dropped task has tau = 0 and v = e_1, a task that does not exist tau = 0 and no rows.

emulate() is the column-wise scheme in float64 numpy (DLARFG as reflector_of makes it, with its drop rule; tasks in
order; dense two-sided updates): it stands in for the kernels where there is no GPU."""
import functools

import numpy as np

EPS = 2.220446049250313e-16
LD = np.longdouble
SB = 64                # half bandwidth, rows of a reflector
QG = 32                # sweeps per compact-WY block of Q2
QNC = 64               # columns per slab of Q2's application
Q2_WORKGROUPS = 512    # at most this many workgroups take the passes from the ticket counter
DROP_NRM2 = 1e-290     # reflector_of: a column whose squared norm is not above this is dropped

DEAD_AMPS = ("1e-158", "1e-160", "1e-161")
DEAD_CLASSES = tuple("dead_first_column_" + a for a in DEAD_AMPS)
BASE_CLASSES = ("random", "graded", "graded_up", "entrywise", "big", "tiny", "width5", "width63", "outer_only",
                "zero_columns", "near_identity", "outlier", "ones")
CLASSES = BASE_CLASSES + DEAD_CLASSES
LARGE_CLASSES = ("random", "graded", "width5", "zero_columns")
# orders at the edges of the geometry: degenerate; n - 1 = 0 (mod 32); also n - 3 = 0 (mod 64); three blocks per bundle; ...
EDGE_ORDERS = (1, 2, 3, 4, 33, 34, 35, 65, 66, 67, 68, 97, 98, 99, 129, 130, 131, 193, 194, 195, 196, 321)
LARGE_ORDERS = (513, 1025)
LD_FULL_MAX = 321      # up to this order the long-double residual and orthogonality are taken on the whole matrix
# (order, classes) of the chase tests: every class at the edge orders, four at the large ones; one case per class from
# order 193 on, where the long-double work of a class takes a noticeable part of a second
CHASE_CASES = tuple((n, CLASSES) for n in EDGE_ORDERS if n < 193) \
    + tuple((n, (c,)) for n in EDGE_ORDERS if n >= 193 for c in CLASSES) \
    + tuple((n, (c,)) for n in LARGE_ORDERS for c in LARGE_CLASSES)


def case_id(case):
    return "%d-%s" % (case[0], "all" if len(case[1]) > 1 else case[1][0])


def m_of(n):
    return max(n, 32)


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ inputs
def _sym_from_lower(L):
    L = np.tril(L) - np.tril(L, -(SB + 1))
    return np.asfortranarray(L + np.tril(L, -1).T)


@functools.lru_cache(maxsize=None)
def band(cls, n):
    """the symmetric n x n band of class cls (made once, shared, read-only)"""
    seed = 1000 * n + sorted(CLASSES).index(cls)
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((n, n))
    i = np.arange(n)
    if cls == "random":
        B = _sym_from_lower(R)
    elif cls in ("graded", "graded_up"):
        s = 10.0 ** (-8.0 * i / n)
        if cls == "graded_up":
            s = s[::-1]
        B = _sym_from_lower(R * s[:, None] * s[None, :])
    elif cls == "entrywise":
        B = _sym_from_lower(R * 10.0 ** rng.uniform(-12.0, 0.0, (n, n)))
    elif cls == "big":
        B = _sym_from_lower(R * 1e80)
    elif cls == "tiny":
        B = _sym_from_lower(R * 1e-80)
    elif cls in ("width5", "width63"):
        w = 5 if cls == "width5" else 63
        B = _sym_from_lower(np.tril(R) - np.tril(R, -(w + 1)))
    elif cls == "outer_only":
        B = _sym_from_lower(np.diag(np.diag(R)) + (np.diag(np.diag(R, -SB), -SB) if n > SB else 0.0))
    elif cls == "zero_columns":
        L = np.tril(R)
        for c in range(2, n, 3):
            L[c + 1:, c] = 0.0
        B = _sym_from_lower(L)
    elif cls == "near_identity":
        B = _sym_from_lower(1e-10 * R)
        B[i, i] += 1.0
    elif cls == "outlier":
        B = _sym_from_lower(R)
        B[n // 2, n // 2] = 1e8
    elif cls == "ones":
        B = _sym_from_lower(np.ones((n, n)))
    elif cls in DEAD_CLASSES:
        B = _sym_from_lower(R)
        hi = min(SB + 1, n)
        col = float(cls.rsplit("_", 1)[1]) * rng.uniform(0.5, 1.0, max(hi - 1, 0))
        B[1:hi, 0] = col
        B[0, 1:hi] = col
    else:
        raise ValueError(cls)
    B.setflags(write=False)
    return B


def tridiagonal(d, e):
    n = d.shape[0]
    T = np.zeros((n, n), dtype=d.dtype)
    T[np.arange(n), np.arange(n)] = d
    if n > 1:
        T[np.arange(1, n), np.arange(n - 1)] = e[:n - 1]
        T[np.arange(n - 1), np.arange(1, n)] = e[:n - 1]
    return T


# ------------------------------------------------------------------ mirrors of the geometry
def task_exists(n, s, k):
    return s >= 0 and k >= 0 and s + 1 + SB * k <= n - 2


def tasks_of_sweep(n, s):
    return (n - 3 - s) // SB + 1 if 0 <= s <= n - 3 else 0


def kmax_of(n):
    return max(n - 3, 0) // SB + 1


def task_rows(n, s, k):
    """first row and one past the last row of reflector (s, k)"""
    return s + 1 + SB * k, min(s + SB * (k + 1), n - 1) + 1


def tasks(n):
    """every task in sweep order"""
    for s in range(max(n - 2, 0)):
        for k in range(tasks_of_sweep(n, s)):
            yield s, k


def q2_first_sweep(S):
    return S * QG - 1


def q2_groups_of_block(n, S):
    s0 = max(q2_first_sweep(S), 0)
    return (n - 3 - s0) // SB + 1 if s0 <= n - 3 else 0


def q2_nS(n):
    nsweeps = max(n - 2, 0)
    return _ceil_div(max(nsweeps, 1) + 1, QG)


def q2_default_nblk(n):
    return 4 if n >= 8192 else 3


def q2_passes(n, ncols, nblk):
    """(npair, nslab, npass) of one application on ncols columns"""
    npair, nslab = _ceil_div(q2_nS(n), nblk), _ceil_div(ncols, QNC)
    return npair, nslab, npair * nslab


# ------------------------------------------------------------------ the reflectors as the stage leaves them
def reflectors(V2, tau2):
    """[(r0, r1, v, tau)] of every task in sweep order, from V2 (n x n) and tau2 ((kmax+1) x max(n-2, 1)), in long double"""
    n = V2.shape[0]
    return [(r0, r1, V2[r0:r1, s].astype(LD), LD(tau2[k, s]))
            for s, k in tasks(n) for r0, r1 in (task_rows(n, s, k),)]


def check_structure(V2, tau2, dropped=()):
    """the structural bounds of the docstring; returns the worst |tau v^T v - 2| / eps over the live reflectors.  dropped: tasks
    that must be the identity"""
    n = V2.shape[0]
    assert tau2.shape == (kmax_of(n) + 1, max(n - 2, 1))
    mask = np.zeros((n, n), dtype=bool)
    worst = 0.0
    for s, k in tasks(n):
        r0, r1 = task_rows(n, s, k)
        mask[r0:r1, s] = True
        v, tau = V2[r0:r1, s], tau2[k, s]
        assert v[0] == 1.0, (s, k)
        if tau == 0.0:
            assert not v[1:].any(), (s, k)
        else:
            assert (s, k) not in dropped, (s, k)
            assert np.abs(v).max() <= 1.0 and 1.0 <= tau <= 2.0, (s, k, tau)
            vl = v.astype(LD)
            r = float(abs(LD(tau) * (vl @ vl) - 2)) / EPS
            worst = max(worst, r)
            assert r <= 16.0, (s, k, r)
    for s, k in dropped:
        assert tau2[k, s] == 0.0, (s, k)
    assert not V2[~mask].any()                              # zero outside the reflectors' rows
    live = np.zeros(tau2.shape, dtype=bool)
    for s, k in tasks(n):
        live[k, s] = True
    assert not tau2[~live].any()                            # tau = 0 for the tasks that do not exist
    return worst


# ------------------------------------------------------------------ long-double references
def sim(refl, B):
    """H_last ... H_1 B H_1 ... H_last in long double, one rank-1 update per side and reflector, in sweep order"""
    n = B.shape[0]
    A = np.array(B, dtype=LD)
    for r0, r1, v, tau in refl:
        if tau == 0:
            continue
        lo, hi = max(r0 - 2 * SB, 0), min(r1 + 2 * SB, n)
        A[r0:r1, lo:hi] -= np.multiply.outer(tau * v, v @ A[r0:r1, lo:hi])
        A[lo:hi, r0:r1] -= np.multiply.outer(A[lo:hi, r0:r1] @ v, tau * v)
    return A


def apply(refl, Z):
    """Q2 Z in long double: the last reflector first"""
    Y = np.array(Z, dtype=LD)
    for r0, r1, v, tau in reversed(refl):
        if tau != 0:
            Y[r0:r1] -= np.multiply.outer(tau * v, v @ Y[r0:r1])
    return Y


def apply_t(refl, Z):
    """Q2^T Z in long double: the first reflector first"""
    Y = np.array(Z, dtype=LD)
    for r0, r1, v, tau in refl:
        if tau != 0:
            Y[r0:r1] -= np.multiply.outer(tau * v, v @ Y[r0:r1])
    return Y


def sample_columns(n, count=8):
    return sorted(set(int(c) for c in np.linspace(0, n - 1, min(count, n)).round()))


def chase_ratios(B, d, e, V2, tau2):
    """(residual, orthogonality) of a chase as shares of their bounds, from the exported reflectors in long double: on the
    whole matrix up to order LD_FULL_MAX, on 8 sample columns of Q2 above (sub-blocks: the same bounds)"""
    n = B.shape[0]
    m = m_of(n)
    refl = reflectors(V2, tau2)
    T = tridiagonal(d.astype(LD), e.astype(LD))
    nrm = float(np.sqrt((B.astype(LD) ** 2).sum()))
    if n <= LD_FULL_MAX:
        R = sim(refl, B) - T
        Q = apply(refl, np.eye(n))
        G = Q.T @ Q - np.eye(n, dtype=LD)
    else:
        cols = sample_columns(n)
        Q = apply(refl, np.eye(n)[:, cols])
        R = apply_t(refl, B.astype(LD) @ Q) - T[:, cols]   # columns of Q2^T B Q2 - T
        G = Q.T @ Q - np.eye(len(cols), dtype=LD)
    res = float(np.sqrt((R ** 2).sum())) / (m * EPS * nrm) if nrm > 0 else float(np.abs(R).max())
    orth = float(np.sqrt((G ** 2).sum())) / (2 * m * EPS)
    return res, orth


def z_ratio(got, ref, n):
    """worst |got - ref| / (m eps max|ref| of the column); an all-zero reference column must be matched exactly"""
    scale = np.abs(ref).max(axis=0)
    err = np.abs(got.astype(LD) - ref).max(axis=0)
    worst = 0.0
    for s, x in zip(scale, err):
        if s == 0:
            assert x == 0
        else:
            worst = max(worst, float(x / (m_of(n) * EPS * s)))
    return worst


# ------------------------------------------------------------------ the float64 emulation
def larfg(x, drop_rule=True):
    """(v, tau, beta) as reflector_of makes them: no rescaling, and a column of squared norm <= DROP_NRM2 is dropped.  The
    squares are summed as wave_sum sums its 64 lanes (neighbours in pairs, level by level; lane 0 gives 0), and alpha0^2 joins
    them in one fused operation (here: in long double, rounded once more)."""
    alpha0 = float(x[0])
    sq = np.zeros(SB)
    sq[1:x.shape[0]] = x[1:] * x[1:]
    while sq.shape[0] > 1:
        sq = sq[0::2] + sq[1::2]
    ssq = float(sq[0])
    nrm2 = float(LD(alpha0) * LD(alpha0) + LD(ssq))
    v = np.zeros_like(x)
    v[0] = 1.0
    if ssq != 0.0 and (nrm2 > DROP_NRM2 or not drop_rule):
        beta = -np.copysign(np.sqrt(nrm2), alpha0)
        v[1:] = x[1:] * (1.0 / (alpha0 - beta))
        return v, (beta - alpha0) / beta, beta
    return v, 0.0, alpha0


def emulate(B, drop_rule=True):
    """the column-wise scheme in float64: (d, e, V2, tau2) as the stage leaves them"""
    n = B.shape[0]
    A = np.array(B, dtype=np.float64, order="F")
    V2 = np.zeros((n, n), order="F")
    tau2 = np.zeros((kmax_of(n) + 1, max(n - 2, 1)), order="F")
    with np.errstate(all="ignore"):
        for s, k in tasks(n):
            r0, r1 = task_rows(n, s, k)
            c = s if k == 0 else r0 - SB                   # the column the reflector annihilates: s, or column 0 of the bulge
            v, tau, beta = larfg(A[r0:r1, c].copy(), drop_rule)
            V2[r0:r1, s] = v
            tau2[k, s] = tau
            if tau != 0.0:
                lo, hi = max(r0 - 2 * SB, 0), min(r1 + 2 * SB, n)
                A[r0:r1, lo:hi] -= np.outer(tau * v, v @ A[r0:r1, lo:hi])
                A[lo:hi, r0:r1] -= np.outer(A[lo:hi, r0:r1] @ v, tau * v)
            A[r0:r1, c] = 0.0
            A[c, r0:r1] = 0.0
            A[r0, c] = A[c, r0] = beta
    d = np.diag(A).copy()
    e = np.diag(A, -1).copy() if n > 1 else np.zeros(0)
    return d, e, V2, tau2


def emulate_q2(V2, tau2, Z):
    """Q2 Z in float64, the last reflector first"""
    n = V2.shape[0]
    Y = np.array(Z, dtype=np.float64)
    for s, k in reversed(list(tasks(n))):
        tau = tau2[k, s]
        if tau != 0.0:
            r0, r1 = task_rows(n, s, k)
            v = V2[r0:r1, s]
            Y[r0:r1] -= np.outer(tau * v, v @ Y[r0:r1])
    return Y


# ------------------------------------------------------------------ eigenvector-like inputs of Q2
@functools.lru_cache(maxsize=None)
def z_input(n, ncols, kind):
    """random: standard normal; scaled: the same with column c times 10**100 (c even) or 10**-100 (c odd)"""
    rng = np.random.default_rng(77 * n + ncols)
    Z = np.asfortranarray(rng.standard_normal((n, ncols)))
    if kind == "scaled":
        Z *= np.where(np.arange(ncols) % 2 == 0, 1e100, 1e-100)[None, :]
    elif kind != "random":
        raise ValueError(kind)
    Z.setflags(write=False)
    return Z
