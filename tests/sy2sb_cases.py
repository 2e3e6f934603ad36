"""Inputs, mirrors of the geometry, references and bounds of the stage tests of the dense -> band reduction (ek_sy2sb.hip):
tests/test_sy2sb_cases_host.py (no GPU) and tests/test_gpu_sy2sb_stages.py.

The stage: a symmetric A (lower triangle read) -> Bd = Q1^T A Q1 of half width 64, Q1 = H_0 H_1 ..., H_j = I - tau_j v_j v_j^T
with v_j zero above row j + 64 and 1 on it (column j of V).  Panel p holds columns 64 p .. 64 p + 63 and rows r0 = 64 (p + 1)
.. n - 1 (m = n - r0 of them): panels of m <= SMALL_MAX = 127 rows are factored inside one workgroup's LDS, taller ones by
the CholeskyQR2 chain in chunks of CH = 64 rows (and, where CholeskyQR2 gives up, by the Householder rescue, counted in bits
8.. of the flag); Y = A22 V is a SYMM over T = ceil(m / 128) block rows cut into nsplit <= 16 ranges of tps tiles.

Matrix classes (matrix(cls, n): seeded, symmetric, made once, read-only):
    random; graded (s_i s_j, s = 10**(-6 i / n)) and graded_up (s reversed); entrywise (every entry times its own
    10**U(-8, 0)); big and tiny (x 1e80, x 1e-80); band65 (half width 65: the tall panels are upper Hessenberg in their
    first 65 rows and zero below -- random triangles CholeskyQR2 cannot factor, and nz chunks of the rescue well short of
    the panel); band64 (a band already: every panel is a random triangle, which goes to the rescue,
    and every reflector the identity); zero_columns (every third
    column zero in the whole of its panel, rows 64 (c // 64 + 1) and on: the first panel has 21 zero columns); parallel_columns (column 5 = (1 + 1e-7)
    column 4 below the band, and from order 201 on column 70 = column 69 + 1e-6 noise below row 140); lowrank_plus_identity
    (I + U U^T, U n x 5); near_identity (I + 1e-10 R); outlier (one diagonal entry 1e8); ones; and far_entry_<where>:
    band64 with column 3 zero in the first panel (a random triangle alone is beyond CholeskyQR2 at most seeds, not at all:
    two of forty went through with conditions of 9e8 and 9e9) plus the single pair A[r, 0] = A[0, r] = 1 at r = 64 + 64 k - 1 (before), 64 + 64 k (at), 64 + 64 k + 1 (after)
    for the largest k >= 1 that fits, and r = n - 1 (last) -- the last non-zero chunk of the rescue's short cut ends at
    a chunk edge, one row past it, two rows past it, and in the panel's last row.  (Where the order has no such row the
    class is band64.)

Flows (pair_min, lookahead_min) as ek_hip_debug_set_sy2sb_flow takes them, 0 = never: plain (0, 0), pairs (1, 0),
lookahead (0, 2), both (1, 2), and from order 449 on handover (257, 257): the stage begins in pairs with look-ahead,
goes on in pairs without, and ends one panel at a time.  lookahead_min = 2 takes the look-ahead on every panel that has
a successor (m - 64 >= 2), down to a staged rank-k update of a 2-row trailing matrix that production (5120 rows) never
sees; the kernels take it as they take any partial tile, so it was NOT raised.

Mirrors: panels(n, pair_min, lookahead_min) gives every panel's rows, kind, chunks, T / nsplit / tps, place in a pair and
whether the update that applies it takes the look-ahead branch, in closed form; walk() is the loop of sy2sb_lower
transcribed (tests/test_sy2sb_cases_host.py holds them against each other).

References in numpy.longdouble from the DEVICE's V and tau: Q1 applied as a product of the reflectors, the last first; up
to order 321 ||Q1^T Q1 - I||_F and ||Q1^T A Q1 - Bd||_F on the whole matrix, above on 8 sample columns j of the first, a
middle and the last panel: A (Q1 e_j) - Q1 (Bd e_j) and Q1^T (Q1 e_j) - e_j (sub-blocks of the same matrices up to the
orthogonal Q1: the same bounds).  eigvalsh of A against Bd up to order 1025.

Bounds (the project's own, tests/test_gpu_two_stage.py):
    ||Q1^T Q1 - I||_F <= 64 n eps        ||Q1^T A Q1 - Bd||_F <= 32 n eps ||A||_F        max|w(A) - w(Bd)| <= 4 n eps max|w|
    V zero above row j + 64, V[j + 64, j] = 1 or tau_j = 0, tau_j in {0} u [1, 2], V and tau zero where there is no reflector.

emulate() is the plain column-by-column Householder reduction in float64 numpy (DLARFG with the scaled norm and the drop
rule of the stage's own Householder kernels); it stands in for the kernels where there is no GPU.  Its shares of the
three bounds, the worst over the edge orders up to 321 with (order) -- the kernels sum in other orders and keep a factor
of four and more:

    class                    orthogonality   similarity      spectrum
    random                   0.0022 (128)    0.0005 (128)    0.0463 (130)
    graded                   0.0019 (129)    0.0000 (320)    0.0165 (127)
    graded_up                0.0020 (131)    0.0005 (66)     0.0174 (67)
    entrywise                0.0022 (131)    0.0005 (129)    0.0334 (67)
    big                      0.0021 (129)    0.0004 (129)    0.0471 (67)
    tiny                     0.0020 (191)    0.0004 (131)    0.0574 (129)
    band65                   0.0012 (131)    0.0002 (127)    0.0554 (67)
    band64                   0               0               0
    zero_columns             0.0018 (257)    0.0004 (191)    0.0437 (255)
    parallel_columns         0.0020 (130)    0.0005 (127)    0.0448 (66)
    lowrank_plus_identity    0.0023 (129)    0.0003 (129)    0.0092 (131)
    near_identity            0.0020 (130)    0.0005 (193)    0.0265 (66)
    outlier                  0.0020 (131)    0.0008 (131)    0.0170 (128)
    ones                     0.0009 (191)    0.0015 (320)    0.0114 (130)
    far_entry_before         0.0014 (319)    0.0003 (256)    0.0424 (193)
    far_entry_at             0.0015 (321)    0.0003 (257)    0.0428 (191)
    far_entry_after          0.0014 (257)    0.0003 (257)    0.0392 (131)
    far_entry_last           0.0015 (129)    0.0003 (255)    0.0534 (128)

No parameter of a class had to be tamed.  (The spectrum's share is mostly the two eigvalsh calls' own error.  Without the
drop rule the ones class broke orthogonality by twelve orders of magnitude from order 258 on: after the first reflector
its columns are rounding errors of rounding errors, down to denormal entries.)"""
import functools

import numpy as np

EPS = 2.220446049250313e-16
LD = np.longdouble
SB = 64                # panel width = half bandwidth
CH = 64                # rows per workgroup of the tall-skinny passes
SMALL_MAX = 127        # panels of at most this many rows are factored in LDS
SYMM_TILE = 128        # rows of a block row of the SYMM
MAXSPLIT = 16          # at most this many K ranges of the SYMM
NEVER = 0
DROP_NRM2 = 1e-290     # a column whose squared norm is not above this gets no reflector (house_tall_kernel; reflector_of)

FAR_WHERE = ("before", "at", "after", "last")
FAR_CLASSES = tuple("far_entry_" + w for w in FAR_WHERE)
BASE_CLASSES = ("random", "graded", "graded_up", "entrywise", "big", "tiny", "band65", "band64", "zero_columns",
                "parallel_columns", "lowrank_plus_identity", "near_identity", "outlier", "ones")
CLASSES = BASE_CLASSES + FAR_CLASSES
LARGE_CLASSES = ("random", "graded", "band65", "zero_columns")
RESCUED_CLASSES = ("band65", "zero_columns", "lowrank_plus_identity") + FAR_CLASSES   # >= 1 rescued panel from order 193 on
# degenerate; one panel of 1, 2, 3 rows; SMALL_MAX and the first chain panel (m = 128: two chunks, one block row; 129:
# three chunks, two block rows; n = 130: has_next); two panels; m = 127 / 128 / 129 again with a panel in front; ...
EDGE_ORDERS = (3, 64, 65, 66, 67, 127, 128, 129, 130, 131, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321, 449, 513)
LARGE_ORDERS = (1025, 2113)
LD_FULL_MAX = 321      # up to this order the long-double residual and orthogonality are taken on the whole matrix
SPECTRUM_MAX = 1025    # up to this order eigvalsh of A is held against eigvalsh of the band
GROUP_MAX = 127        # up to this order one test case runs every class (the long-double work is a few milliseconds each)
HANDOVER_MIN = 449

FLOWS = {"plain": (0, 0), "pairs": (1, 0), "lookahead": (0, 2), "both": (1, 2), "handover": (257, 257)}

CASES = tuple((n, CLASSES) for n in EDGE_ORDERS if n <= GROUP_MAX) \
    + tuple((n, (c,)) for n in EDGE_ORDERS if n > GROUP_MAX for c in CLASSES) \
    + tuple((n, (c,)) for n in LARGE_ORDERS for c in LARGE_CLASSES)


def case_id(case):
    return "%d-%s" % (case[0], "all" if len(case[1]) > 1 else case[1][0])


def flows_of(n):
    return ("plain", "pairs", "lookahead", "both") + (("handover",) if n >= HANDOVER_MIN else ())


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ inputs
def _sym(L):
    L = np.tril(L)
    return np.asfortranarray(L + np.tril(L, -1).T)


def _band(L, w):
    return _sym(np.tril(L) - np.tril(L, -(w + 1)))


def far_row(where, n):
    """the row r of far_entry_<where> at order n, or None where the order has none"""
    if where == "last":
        return n - 1 if n - 1 > SB else None
    k = (n - SB - 2) // SB                       # the largest k with 64 + 64 k + 1 <= n - 1
    if k < 1:
        return None
    return SB + SB * k + {"before": -1, "at": 0, "after": 1}[where]


@functools.lru_cache(maxsize=64)
def matrix(cls, n):
    """the symmetric n x n matrix of class cls (made once, shared, read-only)"""
    rng = np.random.default_rng(1000 * n + sorted(CLASSES).index(cls))
    R = rng.standard_normal((n, n))
    i = np.arange(n)
    if cls == "random":
        A = _sym(R)
    elif cls in ("graded", "graded_up"):
        s = 10.0 ** (-6.0 * i / n)
        if cls == "graded_up":
            s = s[::-1]
        A = _sym(R * s[:, None] * s[None, :])
    elif cls == "entrywise":
        A = _sym(R * 10.0 ** rng.uniform(-8.0, 0.0, (n, n)))
    elif cls == "big":
        A = _sym(R * 1e80)
    elif cls == "tiny":
        A = _sym(R * 1e-80)
    elif cls == "band65":
        A = _band(R, SB + 1)
    elif cls == "band64":
        A = _band(R, SB)
    elif cls == "zero_columns":
        L = np.tril(R)
        L[(i[:, None] >= SB * (i[None, :] // SB + 1)) & (i[None, :] % 3 == 2)] = 0.0
        A = _sym(L)
    elif cls == "parallel_columns":
        A = _sym(R)
        if n > SB + 1:
            A[SB:, 5] = A[SB:, 4] * (1.0 + 1e-7)
            A[5, SB:] = A[SB:, 5]
        if n > 200:
            A[140:, 70] = A[140:, 69] + 1e-6 * rng.standard_normal(n - 140)
            A[70, 140:] = A[140:, 70]
    elif cls == "lowrank_plus_identity":
        U = rng.standard_normal((n, 5))
        A = _sym(U @ U.T + np.eye(n))
    elif cls == "near_identity":
        A = _sym(1e-10 * R)
        A[i, i] += 1.0
    elif cls == "outlier":
        A = _sym(R)
        A[n // 2, n // 2] = 1e8
    elif cls == "ones":
        A = _sym(np.ones((n, n)))
    elif cls in FAR_CLASSES:
        A = _band(R, SB)
        r = far_row(cls.rsplit("_", 1)[1], n)
        if r is not None:
            A[r, 0] = A[0, r] = 1.0
            A[SB:, 3] = 0.0                                  # (a zero column: no CholeskyQR2 of the first panel, whatever the seed)
            A[3, SB:] = 0.0
    else:
        raise ValueError(cls)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=64)
def spectrum(cls, n):
    """eigvalsh of matrix(cls, n) (computed once)"""
    w = np.linalg.eigvalsh(matrix(cls, n))
    w.setflags(write=False)
    return w


def band_of(Ab):
    """the symmetric band matrix whose lower band is the lower band of Ab"""
    L = np.tril(Ab) - np.tril(Ab, -(SB + 1))
    return L + np.tril(L, -1).T


# ------------------------------------------------------------------ mirrors of the geometry
def symm_split(m):
    """(T, nsplit, tps) of the SYMM on a trailing matrix of m rows"""
    T = max(_ceil_div(m, SYMM_TILE), 1)
    tps = _ceil_div(T, min(MAXSPLIT, T))
    return T, _ceil_div(T, tps), tps


def rows_of(n, p):
    return n - SB * (p + 1)


def _panel(n, p, pair, lookahead):
    m = rows_of(n, p)
    d = {"p": p, "c0": SB * p, "r0": SB * (p + 1), "m": m, "kind": "lds" if m <= SMALL_MAX else "chain",
         "chunks": _ceil_div(m, CH) if m > 0 else 0, "pair": pair, "lookahead": lookahead}
    d["T"], d["nsplit"], d["tps"] = symm_split(m) if m >= 2 else (0, 0, 0)   # (a panel of fewer than 2 rows has no SYMM)
    return d


def panels(n, pair_min=NEVER, lookahead_min=NEVER):
    """every panel sy2sb_lower factors at order n, in closed form: a list of dicts with p, c0, r0, m (rows), kind ('lds' /
    'chain'), chunks, T, nsplit, tps (of its SYMM; zeros without one), pair (0: on its own, 1 / 2: first / second of a pair)
    and lookahead (whether the trailing update that applies it -- the pair's one update for both of a pair -- takes the
    look-ahead branch).  Panel 0 is factored at every order above 2, later panels iff they have at least 2 rows."""
    if n <= 2:
        return []
    count = max(sum(1 for p in range(n // SB + 1) if rows_of(n, p) >= 2), 1)
    # pairs: (p, p + 1) for even p while the first has pair_min rows and the second at least 2
    paired = 0
    while pair_min > 0 and rows_of(n, paired) >= pair_min and rows_of(n, paired + 1) >= 2:
        paired += 2
    out = []
    for p in range(count):
        pair = 0 if p >= paired else 1 + p % 2
        mu = rows_of(n, p + 1) if pair == 1 else rows_of(n, p)          # rows of the update that applies this panel
        la = lookahead_min > 0 and mu - SB >= 2 and mu >= lookahead_min
        out.append(_panel(n, p, pair, bool(la)))
    return out


def walk(n, pair_min=NEVER, lookahead_min=NEVER):
    """the loop of sy2sb_lower transcribed: the same list as panels(), plus 'waited' (whether the main stream had to wait for
    the second stream's chain before this panel's SYMM)"""
    if n <= 2:
        return []
    la_min = lookahead_min if lookahead_min > 0 else 1 << 31
    out = {}
    state = {"waited": True}

    def update(m, applies):
        has_next = m - SB >= 2
        la = has_next and m >= la_min
        for q in applies:
            out[q]["lookahead"] = la
        state["waited"] = not la

    def factor(p, pair):
        out[p] = _panel(n, p, pair, False)

    factor(0, 0)                                           # chain(s, 0, 0, 0)
    c0, p = 0, 0
    while True:
        r0 = c0 + SB
        m = n - r0
        if m < 2:
            break
        out[p]["waited"] = not state["waited"]
        m2 = m - SB
        if pair_min > 0 and m >= pair_min and m2 >= 2:
            out[p]["pair"] = 1
            factor(p + 1, 2)                               # chain(s, r0, pb, 1)
            out[p + 1]["waited"] = False
            update(m2, (p, p + 1))
            if m2 - SB >= 2:
                factor(p + 2, 0)
            c0 += 2 * SB
            p += 2
        else:
            update(m, (p,))
            if m - SB >= 2:
                factor(p + 1, 0)
            c0 += SB
            p += 1
    return [out[q] for q in sorted(out)]


def chain_panels(n):
    return sum(1 for q in panels(n) if q["kind"] == "chain")


# ------------------------------------------------------------------ the reflectors as the stage leaves them
def check_structure(V, tau):
    """the structural bounds of the docstring"""
    n = V.shape[0]
    assert V.shape == (n, n) and tau.shape == (n,)
    assert np.isfinite(V).all() and np.isfinite(tau).all()
    i = np.arange(n)
    assert not V[i[:, None] < i[None, :] + SB].any()                    # zero above row j + 64
    for j in range(n):
        if j + SB >= n:                                                 # no row: no reflector
            assert tau[j] == 0.0 and not V[:, j].any(), j
        elif tau[j] == 0.0:
            assert V[j + SB, j] in (0.0, 1.0), j                       # the identity, with or without its unit entry
        else:
            assert j + SB < n - 1, j                                    # (a reflector on one row is the identity)
            assert V[j + SB, j] == 1.0 and 1.0 <= tau[j] <= 2.0, (j, tau[j])


def below_band_is_zero(Ab):
    return not np.tril(Ab, -(SB + 1)).any()


# ------------------------------------------------------------------ long-double references
def reflectors(V, tau):
    """[(r0, v, tau)] of the live reflectors in column order, in long double"""
    n = V.shape[0]
    return [(j + SB, V[j + SB:, j].astype(LD), LD(tau[j])) for j in range(max(n - SB, 0)) if tau[j] != 0.0]


def apply(refl, X):
    """Q1 X in long double: the last reflector first"""
    Y = np.array(X, dtype=LD)
    for r0, v, tau in reversed(refl):
        Y[r0:] -= np.multiply.outer(tau * v, v @ Y[r0:])
    return Y


def apply_t(refl, X):
    """Q1^T X in long double: the first reflector first"""
    Y = np.array(X, dtype=LD)
    for r0, v, tau in refl:
        Y[r0:] -= np.multiply.outer(tau * v, v @ Y[r0:])
    return Y


def sample_columns(n):
    """8 columns of the first, a middle and the last panel"""
    npan = _ceil_div(n, SB)
    mid, last = SB * (npan // 2), SB * (npan - 1)
    cols = (0, 37, 63, mid, mid + 29, last, n - 2, n - 1)
    return sorted(set(min(max(c, 0), n - 1) for c in cols))


def _fro(X):
    return float(np.sqrt((X * X).sum()))


def ratios(A, Ab, V, tau, w_ref=None):
    """(orthogonality, similarity, spectrum) as shares of their bounds, from the band left in the lower band of Ab and the
    reflectors, in long double (whole matrices up to order LD_FULL_MAX, 8 sample columns above); spectrum (float64 eigvalsh
    of the band against w_ref) is None above SPECTRUM_MAX or without w_ref"""
    n = A.shape[0]
    refl = reflectors(V, tau)
    Bd = band_of(Ab).astype(LD)
    Al = np.asarray(A, dtype=LD)
    nrm = _fro(Al)
    if n <= LD_FULL_MAX:
        Q = apply(refl, np.eye(n))
        G = Q.T @ Q - np.eye(n, dtype=LD)
        R = apply_t(refl, apply_t(refl, Al).T) - Bd                    # Q1^T (Q1^T A)^T = Q1^T A Q1
    else:
        cols = sample_columns(n)
        E = np.eye(n)[:, cols]
        Q = apply(refl, E)
        G = apply_t(refl, Q) - E
        R = Al @ Q - apply(refl, Bd[:, cols])
    orth = _fro(G) / (64 * n * EPS)
    sim = _fro(R) / (32 * n * EPS * nrm)
    spec = None
    if w_ref is not None and n <= SPECTRUM_MAX:
        wmax = float(np.abs(w_ref).max())
        spec = float(np.abs(np.linalg.eigvalsh(band_of(Ab)) - w_ref).max()) / (4 * n * EPS * wmax)
    return orth, sim, spec


def spectra_ratio(Ab1, Ab2, w_ref):
    """max|w(band 1) - w(band 2)| as a share of 4 n eps max|w_ref|"""
    n = Ab1.shape[0]
    d = np.abs(np.linalg.eigvalsh(band_of(Ab1)) - np.linalg.eigvalsh(band_of(Ab2))).max()
    return float(d) / (4 * n * EPS * float(np.abs(w_ref).max()))


# ------------------------------------------------------------------ the float64 emulation
def larfg(x):
    """(v, tau, beta) of DLARFG with the scaled norm, and the drop rule of the stage's own Householder kernels: a column whose
    squared norm is not above DROP_NRM2 is left to the identity and zeroed by the caller (the ones class leaves columns of
    rounding errors of rounding errors behind, down to denormal entries, from which no reflector is orthogonal)"""
    v = np.zeros_like(x)
    v[0] = 1.0
    alpha = float(x[0])
    scale = float(np.abs(x[1:]).max()) if x.shape[0] > 1 else 0.0
    xnorm = scale * float(np.sqrt((x[1:] / scale) @ (x[1:] / scale))) if scale > 0.0 else 0.0
    if xnorm == 0.0 or np.hypot(alpha, xnorm) <= np.sqrt(DROP_NRM2):
        return v, 0.0, alpha
    beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
    v[1:] = x[1:] / (alpha - beta)
    return v, (beta - alpha) / beta, beta


def emulate(A):
    """the dense -> band reduction column by column in float64: (Ab with the band in its lower band and zeros below, V, tau)
    as the stage leaves them"""
    n = A.shape[0]
    W = np.array(A, dtype=np.float64, order="F")
    V = np.zeros((n, n), order="F")
    tau = np.zeros(n)
    for j in range(max(n - SB - 1, 0)):
        r0 = j + SB
        v, t, beta = larfg(W[r0:, j].copy())
        V[r0:, j] = v
        tau[j] = t
        if t != 0.0:
            W[r0:, :] -= np.outer(t * v, v @ W[r0:, :])
            W[:, r0:] -= np.outer(W[:, r0:] @ v, t * v)
        W[r0:, j] = 0.0
        W[j, r0:] = 0.0
        W[r0, j] = W[j, r0] = beta
    return np.asfortranarray(np.tril(W)), V, tau
