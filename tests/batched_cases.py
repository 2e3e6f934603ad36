"""A table of hard inputs for the batched solvers (ek_hip_eigenpairs_batched*, ek_hip_eigenpairs_vbatched*): plain
generators, no fixtures.  tests/test_gpu_batched_hard.py runs them on the GPU, tests/test_batched_cases_host.py pins
them on the CPU so that an edit of a generator cannot quietly soften a case.

    make(name, n) -> Case        every name of STANDARD (B is None) and PENCILS, at any order n >= 1
    scaled(case, ka, kb)         A * 2^ka, B * 2^kb: exact, so the truth is 2^(ka - kb) times the truth of `case`

Every case is seeded by its name (zlib.crc32, as tests/test_gpu_fuzz.py::_rng does), so a case is the same bits in every
batch and at every position.  The kinds are those of test_gpu_fuzz.py (_spectrum_case, _panel_case, the pencils of
test_generalized_problem_with_an_ill_conditioned_b_* and test_banded_pencils_*) at batched orders, plus tridiagonal
inputs: every column of the kernel's Householder stage then takes its tau = 0 exit and (d, e) reach the QL stage as
given.

Case.exact holds the eigenvalues where they are known in closed form *for the matrix as stored* (Toeplitz 1-2-1,
Clement, A = B); a spectrum that went through Q diag(w) Q^T is only known to n eps and is left to LAPACK."""
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name family A B exact tridiagonal cond_b spd ka kb")
Case.__doc__ = """A, B (None: standard problem); exact: ascending eigenvalues or None; tridiagonal: A is; cond_b: the
stated condition of B where the case states one; spd: B is meant to be numerically SPD; ka, kb: powers of two applied."""

# A * 2^k: about 1e+-150, 1e+-160, 1e+-200 (the scales of test_extreme_scaling_of_A) and 1e+-301
A_SCALES = (498, -498, 531, -531, 664, -664, 1000, -1000)
B_SCALES = (200, -200)


def rng(name):
    """The generator seeded by a name."""
    return np.random.default_rng(zlib.crc32(name.encode()))


_rng = rng


def _sym(M):
    return np.tril(M) + np.tril(M, -1).T


def _with_spectrum(w, rng):
    n = len(w)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * w) @ Q.T
    return (A + A.T) / 2


def _tridiag(d, e):
    return np.diag(np.asarray(d, dtype=float)) + np.diag(np.asarray(e, dtype=float), 1) + np.diag(np.asarray(e, dtype=float), -1)


def _banded(n, hw, rng):
    M = np.tril(rng.standard_normal((n, n)))
    M = M - np.tril(M, -(hw + 1))
    return M + np.tril(M, -1).T


def _wilkinson(n):
    return np.abs(np.arange(n) - (n - 1) / 2.0)


# --------------------------------------------------------------------------------------------------- spectra
def _spectrum(kind, n, rng):
    if kind == "two_clusters":             # two clusters of width 1e-13
        h = n // 2
        w = np.concatenate([1 + 1e-13 * rng.standard_normal(h), 2 + 1e-13 * rng.standard_normal(n - h)])
    elif kind == "all_equal":
        w = np.full(n, 3.0)
    elif kind == "multiplicity_quarter":   # one eigenvalue of multiplicity n / 4
        m = max(n // 4, 1)
        w = np.concatenate([np.full(m, -1.0), np.linspace(0, 1, n - m)])
    elif kind == "geometric":              # 1 down to 1e-14
        w = np.logspace(0, -14, n)
    elif kind == "pairs":                  # pairs 1e-15 apart
        w = np.repeat(np.linspace(1, 2, (n + 1) // 2), 2)[:n] + 1e-15 * rng.standard_normal(n)
    else:
        raise ValueError(kind)
    return _with_spectrum(w, rng)


def _decoupled_blocks(n, rng):
    blk = np.zeros((n, n))
    h = n // 3
    for a, b in ((0, h), (h, 2 * h), (2 * h, n)):
        M = rng.standard_normal((b - a, b - a))
        blk[a:b, a:b] = M + M.T
    return blk


# --------------------------------------------------------------------------------------------------- tridiagonals
def _tridiagonal(kind, n, rng):
    """(d, e, exact or None)."""
    tag, _, par = kind.partition(":")
    if tag == "toeplitz121":
        k = np.arange(1, n + 1)
        return np.full(n, 2.0), np.full(n - 1, 1.0), np.sort(2.0 - 2.0 * np.cos(k * np.pi / (n + 1)))
    if tag == "clement":                   # zero diagonal: the deflation test |e| <= eps (|d_i| + |d_i+1|) has a zero rhs
        i = np.arange(1, n)
        return np.zeros(n), np.sqrt(i * (n - i).astype(float)), np.arange(-(n - 1), n, 2).astype(float)
    if tag == "wilkinson":
        return _wilkinson(n), np.ones(n - 1), None
    if tag == "glued":                     # W+ of order <= 21, one after the other, glued by `par`
        d, e = [], []
        left = n
        while left > 0:
            b = min(21, left)
            if d:
                e.append([float(par)])
            d.append(_wilkinson(b))
            e.append(np.ones(b - 1))
            left -= b
        return np.concatenate(d), (np.concatenate(e) if n > 1 else np.zeros(0)), None
    if tag in ("graded_down", "graded_up"):
        d = 10.0 ** (-int(par) * np.arange(n) / n)
        if tag == "graded_up":
            d = d[::-1].copy()
        return d, 0.3 * np.sqrt(d[:-1] * d[1:]), None
    if tag in ("ends_equal", "ends_ulp"):  # the flip decision |d[0]| > |d[n-1]| on a tie and an ulp beside it
        rng = _rng("ends")                 # the two cases differ in d[0] alone
        d = rng.uniform(-0.5, 0.5, n)
        d[0] = 1.0
        d[n - 1] = -1.0 if n > 1 else 1.0
        if tag == "ends_ulp":
            d[0] = np.nextafter(1.0, 2.0)
        return d, rng.uniform(0.1, 0.5, n - 1), None
    raise ValueError(kind)


TRIDIAGONALS = ["toeplitz121", "clement", "wilkinson", "glued:1e-8", "glued:1e-14", "graded_down:8", "graded_down:14",
                "graded_up:8", "graded_up:14", "ends_equal", "ends_ulp"]


# --------------------------------------------------------------------------------------------------- dense structure
def _dense(kind, n, rng):
    tag, _, par = kind.partition(":")
    if tag == "graded":                    # D G D with D falling by 10^-k across the matrix
        D = 10.0 ** (-int(par) * np.arange(n) / n)
        return _sym(D[:, None] * rng.standard_normal((n, n)) * D[None, :])
    if tag == "band":
        hw = n // 2 if par == "half" else int(par)
        return _banded(n, hw, rng)
    if tag == "arrowhead":
        A = np.diag(rng.standard_normal(n))
        A[0, :] = A[:, 0] = rng.standard_normal(n)
        return A
    if tag == "lowrank":                   # rank n / 4 + noise
        U = rng.standard_normal((n, max(n // 4, 1)))
        return U @ U.T + float(par) * _sym(rng.standard_normal((n, n)))
    if tag == "pattern":                   # random sparsity pattern
        return _sym(rng.standard_normal((n, n)) * (rng.random((n, n)) < float(par)))
    if tag == "negative_definite":
        G = rng.standard_normal((n, n))
        A = -(G @ G.T + np.eye(n))
        return (A + A.T) / 2
    raise ValueError(kind)


SPECTRA = ["two_clusters", "all_equal", "multiplicity_quarter", "geometric", "pairs"]
DENSE = ["graded:4", "graded:8", "band:1", "band:2", "band:half", "arrowhead", "lowrank:1e-8", "pattern:0.05",
         "negative_definite"]
STANDARD = (SPECTRA + ["decoupled_blocks"] + TRIDIAGONALS + ["neg:" + k for k in TRIDIAGONALS] + DENSE)
PENCILS = ["cond_b:1e6", "cond_b:1e10", "a_equals_b", "band5_band5", "hilbert_b"]
# The Hilbert B is in the table for the failing pivot, from the order at which LAPACK's Cholesky refuses it (14), and at
# orders <= 3 (cond(B) <= 524) as one more ill-conditioned pencil.  At orders 4 .. 13 it still factorises with cond(B)
# from 1.6e4 to 1e18, and the rule for a stated cond(B) has no steady yardstick there: "LAPACK's own" residual and
# orthogonality on a pencil that small are one column of one run (gv and gvd differ from each other by 2.7 x at
# order 7).  Those orders are left out rather than given a wider bound.
HILBERT_LEFT_OUT = range(4, 14)

# The cases that also run multiplied by powers of two.  Their entries stay normal numbers at 2^-1000 and their
# eigenvalues finite at 2^1000 (tests/test_batched_cases_host.py checks both); cond_b:1e6 has eigenvalues up to 1e8 and
# stays below 2^+-664.
SCALED_STANDARD = {"band:half": A_SCALES, "toeplitz121": A_SCALES, "wilkinson": A_SCALES, "two_clusters": A_SCALES,
                   "neg:clement": A_SCALES}
SCALED_PENCILS = {"band5_band5": A_SCALES, "cond_b:1e6": (531, -531, 664, -664)}
B_SCALED_PENCILS = ["band5_band5", "cond_b:1e6"]
# Scale covariance is asked of well-conditioned cases: every stage is homogeneous and nothing in them comes near the
# QL stage's underflow guard.
COVARIANT_STANDARD = ["band:half", "arrowhead", "negative_definite"]
COVARIANT_PENCILS = ["band5_band5"]
COVARIANT_SCALES = (531, -531, 664, -664)


def family(name):
    tag = name.split(":")[0]
    if name.startswith("neg:"):
        return "tridiagonal, negated"
    if name in TRIDIAGONALS:
        return "tridiagonal"
    if name in SPECTRA or name == "decoupled_blocks":
        return "spectrum"
    if name in DENSE:
        return "dense structure"
    if tag == "cond_b" or name == "hilbert_b":
        return "pencil, ill-conditioned B"
    return "pencil"


def make(name, n):
    """The case `name` at order n >= 1 (unscaled)."""
    rng = _rng(name)
    exact, tri, B, cond_b, spd = None, False, None, None, True
    if name in SPECTRA:
        A = _spectrum(name, n, rng)
    elif name == "decoupled_blocks":
        A = _decoupled_blocks(n, rng)
    elif name in TRIDIAGONALS or name.startswith("neg:"):
        neg = name.startswith("neg:")
        d, e, exact = _tridiagonal(name[4:] if neg else name, n, _rng(name[4:] if neg else name))
        A, tri = _tridiag(d, e), True
        if neg:
            A = -A
            exact = None if exact is None else np.sort(-exact)
    elif name in DENSE:
        A = _dense(name, n, rng)
    elif name.startswith("cond_b:"):       # test_generalized_problem_with_an_ill_conditioned_b_at_a_two_stage_order's
        cond_b = float(name.split(":")[1])
        G = rng.standard_normal((n, n))
        A = G + G.T
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        B = (Q * np.logspace(0, -np.log10(cond_b), n)) @ Q.T
        B = (B + B.T) / 2
        if n == 1:
            cond_b = 1.0
    elif name == "a_equals_b":             # every eigenvalue is 1
        B = 0.1 * _banded(n, 8, rng) + 2 * np.eye(n)
        A = B.copy()
        exact = np.ones(n)
    elif name == "band5_band5":            # banded A, banded diagonally dominant B
        A, B = _banded(n, 5, rng), 0.05 * _banded(n, 5, rng) + np.eye(n)
    elif name == "hilbert_b":              # LAPACK's Cholesky refuses it from order 14: the expected outcome is info > 0
        if n in HILBERT_LEFT_OUT:
            raise ValueError("hilbert_b is not part of the table at order %d" % n)
        i = np.arange(n)
        G = rng.standard_normal((n, n))
        A, B = G + G.T, 1.0 / (i[:, None] + i[None, :] + 1.0)
        cond_b = float(np.linalg.cond(B))
        spd = n < 14
    else:
        raise ValueError(name)
    return Case(name, family(name), A, B, exact, tri, cond_b, spd, 0, 0)


def scaled(case, ka, kb=0):
    """A * 2^ka (and B * 2^kb): exact unless an entry leaves the normal range; eigenvalues times 2^(ka - kb)."""
    A = np.ldexp(case.A, ka)
    B = None if case.B is None else np.ldexp(case.B, kb)
    exact = None if case.exact is None else np.ldexp(case.exact, ka - kb)
    name = case.name + "|A*2^%d" % ka + ("|B*2^%d" % kb if kb else "")
    fam = "scaled A" if not kb else ("scaled B" if not ka else "scaled A and B")
    return case._replace(name=name, family=fam, A=A, B=B, exact=exact, ka=ka, kb=kb)


def standard_batch(n):
    """Every standard case at order n and the scaled ones behind them: (case, base) pairs, base the unscaled case."""
    out = []
    for name in STANDARD:
        c = make(name, n)
        out.append((c, c))
    for name, ks in SCALED_STANDARD.items():
        c = make(name, n)
        out += [(scaled(c, k), c) for k in ks]
    return out


def pencil_batch(n):
    out = []
    for name in PENCILS:
        c = make(name, n)
        out.append((c, c))
    for name, ks in SCALED_PENCILS.items():
        c = make(name, n)
        out += [(scaled(c, k), c) for k in ks]
    for name in B_SCALED_PENCILS:
        c = make(name, n)
        out += [(scaled(c, 0, k), c) for k in B_SCALES]
    c = make("band5_band5", n)
    out.append((scaled(c, 600, -600), c))  # L^-1 A L^-T and the eigenvalues themselves overflow: never silently
    return out


def dsytd2_unscaled(A):
    """NumPy restatement of the batched kernel's Householder stage as it was before A was scaled (DSYTD2, lower, the
    column norm a plain sum of squares): (d, e).  Why the scaling exists: at 2^-531 the squares are denormal."""
    C = np.array(A, dtype=float)
    n = C.shape[0]
    d, e = np.zeros(n), np.zeros(max(n - 1, 0))
    for k in range(n - 1):
        x = C[k + 2:, k].copy()
        xn2 = float(np.sum(x * x))
        alpha = C[k + 1, k]
        d[k], e[k] = C[k, k], alpha
        if xn2 == 0.0:
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + xn2), alpha)
        tau = (beta - alpha) / beta
        v = np.concatenate(([1.0], x / (alpha - beta)))
        e[k] = beta
        S = C[k + 1:, k + 1:]
        p = tau * (S @ v)
        w = p - 0.5 * tau * (p @ v) * v
        S -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = C[n - 1, n - 1]
    return d, e
