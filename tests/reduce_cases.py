"""Inputs, references and bounds that tests/test_reduce_stages_host.py (no GPU) and tests/test_gpu_reduce_stages.py share.

Three classes of pencils (A, B) with B = L L^T, each with the reduced matrix C = L^-1 A L^-T, right-hand sides Z of the
recovery and its solution X = L^-T Z:

  "integer"  the answer is known exactly.  L = D + E with D a diagonal of 1, 2 and 4 and E strictly lower, sparse, with
             entries in -2 .. 2 at (odd row, even column) only, so that (D^-1 E)^2 = 0 and L^-1 = (I - D^-1 E) D^-1 is
             dyadic.  C is symmetric with integer entries in -3 .. 3, Y has integer entries in -3 .. 3;
             A = L C L^T, B = L L^T and Z = L^T Y are float64 BLAS products, exact because every entry (and every partial
             sum) is a small integer.  The reference carries no error, and every intermediate of a blocked algorithm is a
             dyadic number of few bits: a wrong tile, offset, sign or a skipped update is an O(1) error.
  "random"   B = G G^T / n + I (cond_2(B) < 10), A symmetric normal; the reference is scipy.linalg.
  "ill"      B = Q diag(logspace(0, -8)) Q^T, A symmetric normal; the reference is scipy.linalg and every bound is
             multiplied by cond_2(B) as numpy.linalg.cond computes it.

The bounds are those of tests/test_gpu_blocks.py (multiples of n eps scale); no constant comes from the code under test.
"""
import functools

import numpy as np
import scipy.linalg as sl

EPS = 2.220446049250313e-16
CLASSES = ("integer", "random", "ill")

# orders round every boundary of the 256-leaves of the solves: 255 takes no leaf, 256 is exactly one, 257 and 513 are a
# leaf plus a sliver, 384 and 640 mix a leaf with a 128-block
LEAF_ORDERS = (255, 256, 257, 384, 511, 512, 513, 640, 768, 1000, 1280)
# the blocked recursion of the reduction at its default direct order of 4096: at 4097 n2 > n1 (the two lower-only
# products), at 5000 n2 <= n1 (one product and the fold)
BLOCKED_ORDERS = (4097, 5000)
# with the direct order at 256: depth >= 2 of the recursion (700 -> 512 + 188, 512 -> 256 + 256; ...); 513 = 256 + 257
# adds the form n2 > n1 at a small order
DEPTH_ORDERS = (513, 700, 1100, 1300)
POTRF_ORDERS = (256, 257, 1000, 1024, 1500, 2177)      # from 1024 on the look-ahead form


# ------------------------------------------------------------------------------------------------ bounds
def bound_sygst_forward(n, C, cond=1.0):
    return 32 * n * EPS * float(np.abs(C).max()) * cond


def bound_sygst_backward(n, A, cond=1.0):
    return 64 * n * EPS * float(np.abs(A).max()) * cond


def bound_trtrs(n, X, cond=1.0):
    return 16 * n * EPS * float(np.abs(X).max()) * cond


def bound_potrf(n, L):
    return 8 * n * EPS * float(np.abs(L).max())


def bound_sygst2(n, A, L):
    """types 2 and 3, C = L^T A L: the bound of tests/test_gpu_sygvx.py"""
    return 4 * n * EPS * float((np.abs(L).T @ np.abs(A) @ np.abs(L)).max()) + 1e-300


# ------------------------------------------------------------------------------------------------ the integer pencil
def integer_factor(n, seed=0, per_row=8):
    """(D, E): the diagonal (1, 2, 4) and the strictly lower part of L, float64 arrays with integer entries."""
    rng = np.random.default_rng(7000 + 31 * n + seed)
    D = rng.choice(np.array([1.0, 2.0, 4.0]), size=n)
    E = np.zeros((n, n), order="F")
    odd = np.arange(1, n, 2)
    if len(odd):
        vals = np.array([-2.0, -1.0, 1.0, 2.0])
        for _ in range(per_row):
            cols = 2 * np.floor(rng.random(len(odd)) * ((odd + 1) // 2)).astype(np.int64)    # an even column < row
            E[odd, cols] = rng.choice(vals, size=len(odd))
        E[odd, odd - 1] = rng.choice(vals, size=len(odd))        # the diagonal blocks are never trivial
    return D, E


def integer_pencil(n, nrhs_max, seed=0):
    D, E = integer_factor(n, seed)
    rng = np.random.default_rng(9000 + 17 * n + seed)
    L = np.asfortranarray(E + np.diag(D))
    T = rng.integers(-3, 4, size=(n, n)).astype(np.float64)
    C = np.asfortranarray(np.tril(T) + np.tril(T, -1).T)
    Y = np.asfortranarray(rng.integers(-3, 4, size=(n, nrhs_max)).astype(np.float64))
    A = np.asfortranarray(L @ C @ L.T)
    B = np.asfortranarray(L @ L.T)
    Z = np.asfortranarray(L.T @ Y)
    return {"cls": "integer", "n": n, "A": A, "B": B, "L": L, "C": C, "Z": Z, "X": Y, "cond": 1.0, "D": D, "E": E}


def integer_inverse(D, E):
    """L^-1 = (I - D^-1 E) D^-1, exact in float64"""
    n = len(D)
    return (np.eye(n) - E / D[:, None]) / D[None, :]


# ------------------------------------------------------------------------------------------------ the SciPy classes
def reduce_scipy(A, L):
    """C = L^-1 A L^-T by two substitutions (A symmetric, in full)"""
    W = sl.solve_triangular(L, A, lower=True, check_finite=False)              # L^-1 A
    return np.asfortranarray(sl.solve_triangular(L, W.T, lower=True, check_finite=False))   # L^-1 (L^-1 A)^T = C^T = C


def recover_scipy(L, Z):
    return np.asfortranarray(sl.solve_triangular(L, Z, lower=True, trans="T", check_finite=False))


def _sym_normal(rng, n):
    G = rng.standard_normal((n, n))
    return np.asfortranarray((G + G.T) / 2.0)


def scipy_pencil(cls, n, nrhs_max, seed=0):
    rng = np.random.default_rng({"random": 11000, "ill": 13000}[cls] + 13 * n + seed)
    if cls == "random":
        G = rng.standard_normal((n, n))
        B = G @ G.T / n + np.eye(n)
        cond = 1.0                                   # (cond_2(B) < 10: the bounds stand as they are)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        B = (Q * np.logspace(0.0, -8.0, n)) @ Q.T
        B = (B + B.T) / 2.0
        cond = float(np.linalg.cond(B))
    B = np.asfortranarray(B)
    A = _sym_normal(rng, n)
    L = np.asfortranarray(sl.cholesky(B, lower=True, check_finite=False))
    Z = np.asfortranarray(rng.standard_normal((n, nrhs_max)))
    return {"cls": cls, "n": n, "A": A, "B": B, "L": L, "C": reduce_scipy(A, L), "Z": Z, "X": recover_scipy(L, Z),
            "cond": cond}


def _build(cls, n, nrhs_max):
    p = integer_pencil(n, nrhs_max) if cls == "integer" else scipy_pencil(cls, n, nrhs_max)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                  # computed once, shared, never modified
    return p


@functools.lru_cache(maxsize=8)
def _small(cls, n):
    return _build(cls, n, n + 3)


@functools.lru_cache(maxsize=1)
def _large(cls, n):
    return _build(cls, n, n + 3)


def pencil(cls, n):
    """The case of a class and order with n + 3 right-hand sides: a dict of read-only arrays A, B, L (B = L L^T), C, Z,
    X and the factor `cond` of its bounds.  Cached (one large order at a time)."""
    return _large(cls, n) if n > 2048 else _small(cls, n)


# ------------------------------------------------------------------------------------------------ extended precision
def substitute_longdouble(L, W, trans=False):
    """L^-1 W (or L^-T W) by substitution in numpy.longdouble, a row of the result a step"""
    n = L.shape[0]
    Lq = np.asarray(L, dtype=np.longdouble)
    X = np.array(W, dtype=np.longdouble)
    if not trans:
        for i in range(n):
            X[i] = (X[i] - Lq[i, :i] @ X[:i]) / Lq[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - Lq[i + 1:, i] @ X[i + 1:]) / Lq[i, i]
    return X


def split_t(n):
    """the split of the triangular solves and of the reduction's recursion (ek_chol.hip): the first part, a multiple of
    256 where the order allows it"""
    if n <= 256:
        return 128
    n1 = -(-(n // 2) // 256) * 256
    if n1 >= n:
        n1 -= 256
    return max(n1, 256)
