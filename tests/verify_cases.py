"""The table behind the tests of the one-problem verifier (ek_hip_residual_device, ek_hip_orthogonality_device,
ek_hip_ipratios_device, ek_hip_check): the cases, their references, the bounds and the judge.  Plain
functions, no fixtures, no GPU; tests/test_verify_cases_host.py pins the host mirror and the judge on the CPU,
tests/test_gpu_verify.py runs the kernels through the same judge.

A verifier here is a function v(A, B, w, Z, parts, n_check, index1, index2, n_vec) -> dict with the keys of the parts it
was asked for: "residual" gives a_norm, res_ave, res_max over the first n_check columns, "orthogonality" the criterion
over the columns index1 .. index2 (1-based), "ipr" an array of n_vec ratios.  A and B count by their lower triangles.

Closed-form cases (kind "exact") are exact in fp64 up to the last square roots and divisions, so their expectations need
no reference implementation; the bounds are counted in ulp.  Seeded dense cases (kind "dense") are SciPy eigenpairs with
every column perturbed far above rounding; the reference is long double with explicit sums of squares, the bounds are
forward-error bounds with the project's constant c = 4 max(n, 8) eps (tol)."""
import functools

import numpy as np
import scipy.linalg as sl

from eigenkernel_amd import verifier

EPS = 2.220446049250313e-16
L = np.longdouble
ORDERS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 333, 513)
BIG = 1030                                          # closed form only: scale_cols_kernel's second trip starts at column 1024
KEYS = ("a_norm", "res_ave", "res_max", "orthogonality", "ipr")
PARTS = ("residual", "orthogonality", "ipr")
POSITIONS = (0, 63, 64, 255, 256)                   # where an extreme sits, besides the last checked column


def n_checks(n):
    return tuple(sorted({c for c in (1, 7, 255, 256, 257, n) + ((1024, 1025) if n == BIG else ()) if c <= n}))


def windows(n):
    """The 1-based column windows of order n: (1, 1), (1, n), (n, n), (2, 20), (65, 257), (n - 1, n), clipped to n."""
    raw = ((1, 1), (1, n), (n, n), (2, 20), (65, 257), (n - 1, n))
    return tuple(sorted({(a, min(b, n)) for a, b in raw if 1 <= a <= min(b, n)}))


def n_vecs(n):
    return tuple(sorted({c for c in (1, 64, 65, n) if c <= n}))


def tol(n):
    return 4 * max(n, 8) * EPS


def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


class Case:
    """name, kind, n, problem, parts, the inputs A, B (None for problem 0), w, Z as a caller stores them, the selection
    n_check, index1, index2, n_vec, and ref / bound: a long-double value and an absolute bound per judged key."""

    def run(self, v):
        return v(self.A, self.B, self.w, self.Z, self.parts, self.n_check, self.index1, self.index2, self.n_vec)


def _case(name, kind, n, problem, parts, A, B, w, Z, n_check=0, index1=1, index2=0, n_vec=0):
    c = Case()
    c.name, c.kind, c.n, c.problem, c.parts = name, kind, n, problem, tuple(parts)
    c.A, c.B, c.w, c.Z = A, B, w, Z
    c.n_check, c.index1, c.index2, c.n_vec = n_check, index1, index2, n_vec
    c.ref, c.bound = {}, {}
    for a in (A, B, w, Z):
        if a is not None:
            a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------ closed-form cases
@functools.lru_cache(maxsize=None)
def _exact_residual_inputs(n, problem):
    """A: symmetric integers in -8 .. 8; B: diag of 2^-2 .. 2^3; V: I with permuted columns; w_j: the diagonal quotient plus
    delta_j, a non-zero multiple of 1/64 in -1 .. 1.  Column j of R = A V - B V diag(w) is column p_j of A with its diagonal
    entry replaced by -delta_j b_pj: colsq[j] holds 2^16 times its sum of squares, asq the one of A, both integers."""
    rng = np.random.default_rng(41000 + 2 * n + problem)
    T = rng.integers(-8, 9, (n, n))
    Ai = np.tril(T) + np.tril(T, -1).T
    if not Ai.any():
        Ai[0, 0] = 3
    bexp = rng.integers(-2, 4, n) if problem else np.zeros(n, dtype=np.int64)
    p = rng.permutation(n)
    d64 = rng.integers(1, 65, n) * rng.choice((-1, 1), n)          # delta_j * 64
    A, b = Ai.astype(np.float64), 2.0 ** bexp
    Z = np.zeros((n, n), order="F")
    Z[p, np.arange(n)] = 1.0
    w = Ai[p, p] / b[p] + d64 / 64.0
    off = (Ai[:, p].astype(object) ** 2).sum(axis=0) - Ai[p, p].astype(object) ** 2
    colsq = off * 2 ** 16 + (d64.astype(object) * (2 ** (bexp[p] + 2)).astype(object)) ** 2
    asq = int((Ai.astype(object) ** 2).sum())
    return A, (np.diag(b) if problem else None), w, Z, [int(x) for x in colsq], asq


def exact_residual_case(n, problem, n_check):
    A, B, w, Z, colsq, asq = _exact_residual_inputs(n, problem)
    c = _case("exact residual n=%d problem=%d n_check=%d" % (n, problem, n_check), "exact", n, problem, ("residual",),
              A, B, w, Z, n_check=n_check)
    a_norm = np.sqrt(L(asq))
    rho = np.array([np.sqrt(L(x)) / 256 for x in colsq[:n_check]], dtype=L) / a_norm
    c.ref = {"a_norm": a_norm, "res_ave": rho.sum() / n_check, "res_max": rho.max()}
    c.bound = {"a_norm": 2 * _ulp(a_norm), "res_ave": n_check * EPS * c.ref["res_ave"], "res_max": 2 * _ulp(c.ref["res_max"])}
    return c


ORTH_EPS = 2.0 ** -10


def orth_pairs(n):
    """(j, k): column j of I gets 2^-10 e_k.  The corners of every window of windows(n) and the 255 / 256 seam."""
    raw = ((0, n - 1), (n - 1, n - 2), (1, 19), (64, 256), (255, 256), (256, 65), (n // 2, 0))
    seen, out = set(), []
    for j, k in raw:
        if 0 <= j < n and 0 <= k < n and j != k and j not in seen:
            seen.add(j)
            out.append((j, k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _exact_orth_inputs(n, problem):
    rng = np.random.default_rng(42000 + 2 * n + problem)
    b = 2.0 ** rng.integers(-2, 4, n) if problem else np.ones(n)
    Z = np.eye(n, order="F")
    for j, k in orth_pairs(n):
        Z[k, j] += ORTH_EPS
    G = Z.T @ (b[:, None] * Z)                      # exact: every entry is a sum of at most three dyadic terms of < 30 bits
    return (np.diag(b) if problem else None), Z, G


def exact_orth_case(n, problem, index1, index2):
    B, Z, G = _exact_orth_inputs(n, problem)
    A, w = np.zeros((n, n)), np.zeros(n)
    c = _case("exact orthogonality n=%d problem=%d window=(%d, %d)" % (n, problem, index1, index2), "exact", n, problem,
              ("orthogonality",), A, B, w, Z, index1=index1, index2=index2)
    Gw = G[index1 - 1:index2, index1 - 1:index2].astype(L)
    s = 1 / np.sqrt(np.diag(Gw))
    Gs = Gw * s[:, None] * s[None, :]
    np.fill_diagonal(Gs, 0)
    c.ref = {"orthogonality": np.sqrt((Gs * Gs).sum())}
    c.bound = {"orthogonality": (index2 - index1 + 1) * EPS * c.ref["orthogonality"]}
    return c


def disjoint_pairs_orthogonality(pairs):
    """The criterion of I + 2^-10 e_k e_j^T over disjoint pairs (j, k), B absent: each pair gives two entries
    eps / sqrt(1 + eps^2)."""
    e = L(ORTH_EPS)
    return np.sqrt(2 * len(pairs) * (e / np.sqrt(1 + e * e)) ** 2)


@functools.lru_cache(maxsize=None)
def _exact_ipr_inputs(n, problem):
    """Column j: m_j equal entries 2^-p_j at seeded rows, m_j cycling through 1, 2, 64, 256, n (those <= n)."""
    rng = np.random.default_rng(43000 + 2 * n + problem)
    b = 2.0 ** rng.integers(-2, 4, n) if problem else np.ones(n)
    ms = [m for m in (1, 2, 64, 256, n) if m <= n]
    Z = np.zeros((n, n), order="F")
    ipr = np.zeros(n, dtype=L)
    for j in range(n):
        m, p = ms[j % len(ms)], j % 6
        rows = rng.permutation(n)[:m]
        Z[rows, j] = 2.0 ** -p
        ipr[j] = L(m) / L(b[rows].sum()) ** 2       # sum v^4 = m 2^-4p, (sum b v^2)^2 = 2^-4p (sum b)^2: 1 / m for B absent
    return (np.diag(b) if problem else None), Z, ipr


def exact_ipr_case(n, problem, n_vec):
    B, Z, ipr = _exact_ipr_inputs(n, problem)
    A, w = np.zeros((n, n)), np.zeros(n)
    c = _case("exact ipr n=%d problem=%d n_vec=%d" % (n, problem, n_vec), "exact", n, problem, ("ipr",), A, B, w, Z,
              n_vec=n_vec)
    c.ref = {"ipr": ipr[:n_vec].copy()}
    c.bound = {"ipr": 4 * _ulp(ipr[:n_vec])}
    return c


def exact_cases(n, problem):
    out = [exact_residual_case(n, problem, k) for k in n_checks(n)]
    out += [exact_orth_case(n, problem, a, b) for a, b in windows(n)]
    return out + [exact_ipr_case(n, problem, k) for k in n_vecs(n)]


# ------------------------------------------------------------------------------------------------ seeded dense cases
def _sym_lower(M):
    return np.tril(M) + np.tril(M, -1).T


class DenseBase:
    """A seeded pair with perturbed SciPy eigenpairs and what every selection of columns needs of it: the long-double
    products A Z, S = B Z (Z for problem 0) and G = Z^T S, and the float64 products of the absolute values for the bounds.
    with_w / with_columns / with_zero_a give a changed copy and recompute only what the change touches."""

    def __init__(self, n, problem, A, B, w, Z, extreme):
        self.n, self.problem, self.A, self.B, self.w, self.Z, self.extreme = n, problem, A, B, w, Z, extreme
        self.AZ = np.zeros((n, n), dtype=L)
        self.S = np.zeros((n, n), dtype=L)
        self.G = np.zeros((n, n), dtype=L)
        self.absAZ, self.absS, self.absG = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        self._products(np.arange(n))

    def _products(self, cols):
        with np.errstate(all="ignore"):
            Zl, Za = self.Z.astype(L), np.abs(self.Z)
            self.AZ[:, cols] = self.A.astype(L) @ Zl[:, cols]
            self.S[:, cols] = self.B.astype(L) @ Zl[:, cols] if self.B is not None else Zl[:, cols]
            self.G[:, cols] = Zl.T @ self.S[:, cols]
            self.G[cols, :] = self.G[:, cols].T
            self.absAZ[:, cols] = np.abs(self.A) @ Za[:, cols]
            self.absS[:, cols] = np.abs(self.B) @ Za[:, cols] if self.B is not None else Za[:, cols]
            self.absG[:, cols] = Za.T @ self.absS[:, cols]
            self.absG[cols, :] = self.absG[:, cols].T

    def _copy(self):
        o = object.__new__(DenseBase)
        o.__dict__.update(self.__dict__)
        return o

    def with_w(self, j, value):
        o = self._copy()
        o.w = self.w.copy()
        o.w[j] = value
        return o

    def with_columns(self, cols, values):
        o = self._copy()
        o.Z = self.Z.copy(order="F")
        o.Z[:, cols] = values
        for name in ("AZ", "S", "G", "absAZ", "absS", "absG"):
            setattr(o, name, getattr(self, name).copy())
        o._products(np.atleast_1d(cols))
        return o

    def with_zero_a(self):
        o = self._copy()
        o.A = np.zeros_like(self.A)
        o.AZ, o.absAZ = np.zeros_like(self.AZ), np.zeros_like(self.absAZ)
        return o

    def rho(self):
        """(a_norm, rho_j and its bound for every column)"""
        with np.errstate(all="ignore"):
            Al = self.A.astype(L)
            a_norm = np.sqrt((Al * Al).sum())
            R = self.AZ - self.S * self.w.astype(L)
            rho = np.sqrt((R * R).sum(axis=0)) / a_norm
            T = self.absAZ + self.absS * np.abs(self.w)
            return a_norm, rho, tol(self.n) * np.sqrt((T * T).sum(axis=0)) / np.float64(a_norm)

    def case(self, name, parts=PARTS, n_check=None, index1=1, index2=None, n_vec=None, dirty=False):
        """The selection as a Case.  dirty: NaN wherever the selection's parts must not look -- the strictly upper
        triangles of A and B, w from n_check on, the columns of Z that no part of `parts` reads."""
        n = self.n
        n_check = n if n_check is None else n_check
        index2 = n if index2 is None else index2
        n_vec = n if n_vec is None else n_vec
        A, B, w, Z = self.A.copy(order="F"), (self.B.copy(order="F") if self.B is not None else None), self.w.copy(), self.Z.copy(order="F")
        if dirty:
            up = np.triu_indices(n, 1)
            A[up] = np.nan
            if B is not None:
                B[up] = np.nan
            read = np.zeros(n, dtype=bool)
            if "residual" in parts:
                read[:n_check] = True
                w[n_check:] = np.nan
            else:
                w[:] = np.nan
            if "orthogonality" in parts:
                read[index1 - 1:index2] = True
            if "ipr" in parts:
                read[:n_vec] = True
            Z[:, ~read] = np.nan
        c = _case("dense n=%d problem=%d %s" % (n, self.problem, name), "dense", n, self.problem, parts, A, B, w, Z,
                  n_check=n_check, index1=index1, index2=index2, n_vec=n_vec)
        t = tol(n)
        with np.errstate(all="ignore"):
            if "residual" in parts:
                a_norm, rho, brho = self.rho()
                c.ref.update(a_norm=a_norm, res_ave=rho[:n_check].sum() / n_check, res_max=rho[:n_check].max())
                c.bound.update(a_norm=t * np.float64(a_norm), res_ave=brho[:n_check].mean(), res_max=brho[:n_check].max())
            if "orthogonality" in parts:
                win = slice(index1 - 1, index2)
                Gw = self.G[win, win]
                s = 1 / np.sqrt(np.diag(Gw))
                Gs = Gw * s[:, None] * s[None, :]
                np.fill_diagonal(Gs, 0)
                sa = s.astype(np.float64)
                Ga = self.absG[win, win] * sa[:, None] * sa[None, :]
                np.fill_diagonal(Ga, 0)
                c.ref["orthogonality"] = np.sqrt((Gs * Gs).sum())
                c.bound["orthogonality"] = t * np.sqrt((Ga * Ga).sum())
            if "ipr" in parts:
                Zl = self.Z[:, :n_vec].astype(L)
                g = np.diag(self.G)[:n_vec]
                c.ref["ipr"] = ((Zl * Zl) ** 2).sum(axis=0) / g ** 2
                c.bound["ipr"] = t * c.ref["ipr"].astype(np.float64) * np.diag(self.absG)[:n_vec] / g.astype(np.float64)
        return c


@functools.lru_cache(maxsize=None)
def dense_base(n, problem):
    """A = _sym, B = _spd (cond 10), SciPy's pairs, then w_j += 1e-5 g_j and Z += 1e-6 G: every quantity far above
    rounding.  No column is singled out yet; planted() does that."""
    rng = np.random.default_rng(44000 + 2 * n + problem)
    A = _sym(rng, n)
    B = _spd(rng, n) if problem else None
    w, Z = sl.eigh(A, B, lower=True) if problem else sl.eigh(A, lower=True)
    w = w + 1e-5 * rng.standard_normal(n)
    Z = np.asfortranarray(Z + 1e-6 * rng.standard_normal((n, n)))
    return DenseBase(n, problem, A, B, w, Z, None)


@functools.lru_cache(maxsize=None)
def planted(n, problem, j):
    """dense_base with w_j moved on by 1000 max_k rho_k ||A||_F / ||S_j||: the residual of column j becomes 1000 times the
    largest of the others (to within one of them)."""
    base = dense_base(n, problem)
    a_norm, rho, _ = base.rho()
    shift = 1000 * (np.delete(rho, j).max() if n > 1 else rho[0]) * a_norm / np.sqrt((base.S[:, j] ** 2).sum())
    o = base.with_w(j, base.w[j] + float(shift))
    o.extreme = j
    return o


def dense_cases(n, problem):
    """Every n_check, window and n_vec of the order as one-part cases, the extreme column in the middle of each n_check."""
    out = []
    for k in n_checks(n):
        out.append(planted(n, problem, k // 2).case("n_check=%d" % k, ("residual",), n_check=k))
    base = planted(n, problem, n // 2)
    out += [base.case("window=(%d, %d)" % (a, b), ("orthogonality",), index1=a, index2=b) for a, b in windows(n)]
    return out + [base.case("n_vec=%d" % k, ("ipr",), n_vec=k) for k in n_vecs(n)]


EXTREME_N = 300


def extreme_cases(problem):
    """Order 300: the 1000-fold column at every position of POSITIONS and at the last checked column, n_check 300 and 257;
    a planted non-orthogonal pair (column j += 1e-3 column k) at the corners and at the 255 / 256 seam of two windows."""
    n, out = EXTREME_N, []
    for k in (300, 257):
        for j in POSITIONS + (k - 1,):
            out.append(planted(n, problem, j).case("n_check=%d extreme at %d" % (k, j), ("residual",), n_check=k))
    base = dense_base(n, problem)
    for a, b in ((1, n), (3, 290)):
        lo, hi = a - 1, b - 1                       # the window's corners, 0-based; its seam lies at lo + 255 | lo + 256
        for j, k in ((lo, hi), (hi, lo), (lo + 255, lo + 256), (lo + 256, lo + 255), (lo, lo + 1), (hi, hi - 1)):
            o = base.with_columns(j, base.Z[:, j] + 1e-3 * base.Z[:, k])
            out.append(o.case("window=(%d, %d) pair (%d, %d)" % (a, b, j, k), ("orthogonality",), index1=a, index2=b))
    return out


def unread_cases(n, problem, dirty=True):
    """What must never be looked at holds NaN (Case.A, .B, .w, .Z); the reference is that of the clean arrays.  dirty =
    False: the same selections on the clean arrays, full symmetric matrices."""
    base = planted(n, problem, 3 % n)
    k, (a, b) = min(7, n), (min(2, n), min(20, n))
    tag = "dirty" if dirty else "clean"
    return [base.case("%s n_check=%d" % (tag, k), ("residual",), n_check=k, dirty=dirty),
            base.case("%s window=(%d, %d)" % (tag, a, b), ("orthogonality",), index1=a, index2=b, dirty=dirty),
            base.case("%s n_vec=%d" % (tag, k), ("ipr",), n_vec=k, dirty=dirty),
            base.case("%s all parts" % tag, PARTS, n_check=n, dirty=dirty)]


NONFINITE_KINDS = ("w nan", "w inf", "z nan", "z zero column", "a zero")


def nonfinite_case(problem, kind, j, n_check=EXTREME_N):
    """Order 300, all three parts over n_check columns; j: the column that holds the non-finite value (not used by "a zero")."""
    n = EXTREME_N
    base = planted(n, problem, 100)
    if kind == "w nan":
        o = base.with_w(j, np.nan)
    elif kind == "w inf":
        o = base.with_w(j, np.inf)
    elif kind == "z nan":
        col = base.Z[:, j].copy()
        col[(7 * j + 5) % n] = np.nan
        o = base.with_columns(j, col)
    elif kind == "z zero column":
        o = base.with_columns(j, np.zeros(n))
    elif kind == "a zero":
        o = base.with_zero_a()
    else:
        raise ValueError(kind)
    return o.case("%s at %d, n_check=%d" % (kind, j, n_check), PARTS, n_check=n_check, index1=1, index2=n_check,
                  n_vec=n_check)


def nonfinite_positions(n_check=EXTREME_N):
    return (0, 255, 256, n_check - 1)


def nonfinite_cases(problem):
    out = [nonfinite_case(problem, kind, j) for kind in NONFINITE_KINDS[:4] for j in nonfinite_positions()]
    return out + [nonfinite_case(problem, "a zero", 0)]


def clean_case(problem, n_check=EXTREME_N):
    """The case the non-finite ones are changed from: the slots they leave finite keep its bits."""
    return planted(EXTREME_N, problem, 100).case("clean n_check=%d" % n_check, PARTS, n_check=n_check, index1=1,
                                                 index2=n_check, n_vec=n_check)


def table(orders=ORDERS):
    """Every case that runs on the host: both problem kinds at every order, the closed form also at BIG."""
    out = []
    for problem in (0, 1):
        for n in orders:
            out += exact_cases(n, problem) + dense_cases(n, problem)
        out += exact_cases(BIG, problem)
        out += extreme_cases(problem) + nonfinite_cases(problem) + [clean_case(problem)]
        for n in (33, 65, 257):
            out += unread_cases(n, problem)
    return out


# ------------------------------------------------------------------------------------------------ verifiers on the host
def mirror(A, B, w, Z, parts, n_check, index1, index2, n_vec):
    """eigenkernel_amd/verifier.py on the lower-triangle-symmetrised matrices."""
    out = {}
    Bs = _sym_lower(B) if B is not None else None
    with np.errstate(all="ignore"):
        if "residual" in parts:
            out["a_norm"], out["res_ave"], out["res_max"] = verifier.eval_residual_norm(_sym_lower(A), w[:n_check],
                                                                                        Z[:, :n_check], Bs)
        if "orthogonality" in parts:
            out["orthogonality"] = verifier.eval_orthogonality(Z, Bs, index1, index2)
        if "ipr" in parts:
            out["ipr"] = verifier.get_ipratios(Z[:, :n_vec], Bs)
    return out


FLAWS = ("rows 0..n-2 only", "norm of the lower triangle without mirroring", "upper triangle read as stored",
         "res_ave divided by n", "orthogonality window shifted by one column", "G scaled on one side only",
         "diagonal of G not zeroed", "ipr denominator with V.V where B is present",
         "columns from 1024 on not scaled by -w", "maximum that drops NaN")


def numpy_verifier(flaw=None):
    """The three quantities in plain float64 NumPy; flaw (one of FLAWS) makes it wrong in one way a kernel could be."""
    assert flaw is None or flaw in FLAWS

    def v(A, B, w, Z, parts, n_check, index1, index2, n_vec):
        n = A.shape[0]
        sym = (lambda M: M) if flaw == FLAWS[2] else _sym_lower
        Bs = sym(B) if B is not None else None
        rows = slice(0, n - 1) if flaw == FLAWS[0] else slice(0, n)
        out = {}
        with np.errstate(all="ignore"):
            if "residual" in parts:
                As, V = sym(A), Z[:, :n_check]
                scale = -w[:n_check]
                if flaw == FLAWS[8]:
                    scale[1024:] = 1.0
                R = (Bs @ V if Bs is not None else V) * scale + As @ V
                norms = np.sqrt((R[rows] ** 2).sum(axis=0))
                a_norm = np.sqrt(((np.tril(A) if flaw == FLAWS[1] else As[rows]) ** 2).sum())
                mx = np.fmax.reduce(norms) if flaw == FLAWS[9] else norms.max()
                out.update(a_norm=a_norm, res_ave=norms.sum() / a_norm / (n if flaw == FLAWS[3] else n_check),
                           res_max=mx / a_norm)
            if "orthogonality" in parts:
                shift = 1 if flaw == FLAWS[4] else 0
                Vs = Z[:, index1 - 1 + shift:index2 + shift]
                G = Vs[rows].T @ (Bs @ Vs if Bs is not None else Vs)[rows]
                s = 1.0 / np.sqrt(np.diag(G))
                G = G * s[:, None] * (1.0 if flaw == FLAWS[5] else s[None, :])
                if flaw != FLAWS[6]:
                    np.fill_diagonal(G, 0.0)
                out["orthogonality"] = np.sqrt((G * G).sum())
            if "ipr" in parts:
                V = Z[:, :n_vec]
                SV = Bs @ V if Bs is not None and flaw != FLAWS[7] else V
                out["ipr"] = ((V * V) ** 2)[rows].sum(axis=0) / (V * SV)[rows].sum(axis=0) ** 2
        return out

    return v


# ------------------------------------------------------------------------------------------------ the judge
def judge(case, got):
    """(failures, shares): a line per judged slot that is missing, is finite where the reference is not (or the reverse), is
    no NaN where the reference is NaN, or lies outside its bound; and per key the largest |got - ref| / bound over the slots
    that are finite on both sides (0 where a zero bound is met exactly)."""
    fails, shares = [], {}
    for key in KEYS:
        if key not in case.ref:
            continue
        if key not in got:
            fails.append("%s: missing" % key)
            continue
        ref = np.atleast_1d(np.asarray(case.ref[key], dtype=L))
        val = np.atleast_1d(np.asarray(got[key], dtype=np.float64))
        bnd = np.broadcast_to(np.atleast_1d(np.asarray(case.bound[key], dtype=np.float64)), ref.shape)
        if val.shape != ref.shape:
            fails.append("%s: shape %s, reference %s" % (key, val.shape, ref.shape))
            continue
        worst = 0.0
        for i in range(ref.size):
            slot = key if ref.size == 1 and key != "ipr" else "%s[%d]" % (key, i)
            if np.isfinite(ref[i]) != np.isfinite(val[i]) or (np.isnan(ref[i]) and not np.isnan(val[i])):
                fails.append("%s: %r where the reference is %r" % (slot, float(val[i]), float(ref[i])))
            elif np.isfinite(ref[i]):
                err = float(abs(L(val[i]) - ref[i]))
                share = err / bnd[i] if bnd[i] > 0 else (0.0 if err == 0 else np.inf)
                if not share <= 1.0:
                    fails.append("%s: %r, reference %r, %.3g of the bound %.3g" % (slot, float(val[i]), float(ref[i]), share,
                                                                                  bnd[i]))
                worst = max(worst, share)
        shares[key] = worst
    return fails, shares
