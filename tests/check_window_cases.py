"""The table behind the tests of the window check (ek_hip_check_window_xbatched*): the orders, the column
counts per order, seeded pairs with SciPy's eigenpairs sliced to a window, the planted errors, the host mirror on the
window's columns, a long-double evaluation of the same quantities, and the tolerance.  Plain functions, no fixtures;
tests/test_check_window_host.py pins the mirror on the CPU, tests/test_gpu_check_window.py runs the kernel against it.

Orders: a ragged K step (n % 16 != 0), one and two row tiles of 128, both sides of EK_HIP_BATCH_NMAX.  Column counts: one
and two column tiles of 64 with a ragged second one, and both sides of every 16-column subtile edge up to 64 (the kernel
issues the matrix instructions of the subtiles that hold a column).

The tolerance is the project's 4 max(n, 8) eps -- absolute for res_ave, res_max and orthogonality, relative for a_norm
and every IPR (tests/test_gpu_check_xbatched.py)."""
import functools

import numpy as np
import scipy.linalg as sl

from eigenkernel_amd import verifier

EPS = 2.220446049250313e-16
ORDERS = (1, 2, 17, 33, 64, 65, 127, 128, 129, 130, 192, 255, 256)
COUNT = 4                                           # seeded problems per order
NAMES = ("a_norm", "res_ave", "res_max", "orthogonality", "ipr")


def columns(n):
    """The column counts of order n, ascending: 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, n / 8, n - 1, n clipped to 1 .. n."""
    raw = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, n // 8, n - 1, n)
    return tuple(sorted({min(max(c, 1), n) for c in raw}))


def _sym(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2.0


def _spd(rng, n, cond=10.0):
    """B = Q diag(d) Q^T with d log-spaced in [1, cond]."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([cond])
    B = (Q * d) @ Q.T
    return (B + B.T) / 2.0


class Case:
    pass


@functools.lru_cache(maxsize=None)
def cases(n, problem):
    """COUNT seeded problems of order n: A, B (None for problem 0) and SciPy's full w and Z.  Read only."""
    rng = np.random.default_rng(35000 + n)
    A = np.stack([_sym(rng, n) for _ in range(COUNT)])
    B = np.stack([_spd(rng, n) for _ in range(COUNT)])
    w, Z = np.zeros((COUNT, n)), np.zeros((COUNT, n, n))
    for b in range(COUNT):
        w[b], Z[b] = sl.eigh(A[b], B[b], lower=True) if problem else sl.eigh(A[b], lower=True)
    c = Case()
    c.n, c.A, c.B, c.w, c.Z = n, A, (B if problem else None), w, Z
    for a in (A, B, w, Z):
        a.setflags(write=False)
    return c


def window(case, b, c):
    """The c pairs in the middle of problem b's spectrum: (w of c values, Z of n x c), copies."""
    first = (case.n - c) // 2
    return case.w[b, first:first + c].copy(), case.Z[b][:, first:first + c].copy()


def planted(w, Z, seed):
    """(w, Z) with three errors: 1e-9 N(0, 1) on every entry of column 0 (residual of that column, and the average), 1e-3
    of the last but one column added to the last (orthogonality and that column's residual; needs two columns), and the
    middle eigenvalue off by 1e-4 (1 + |w|) (res_max).  Every slot of the check becomes non-trivial."""
    rng = np.random.default_rng(seed)
    w, Z = w.copy(), Z.copy()
    c = Z.shape[1]
    Z[:, 0] += 1e-9 * rng.standard_normal(Z.shape[0])
    if c >= 2:
        Z[:, c - 1] += 1e-3 * Z[:, c - 2]
    w[c // 2] += 1e-4 * (1.0 + abs(w[c // 2]))
    return w, Z


@functools.lru_cache(maxsize=None)
def windows(n, problem, c, plant):
    """The window of c pairs of each of the COUNT problems, clean or with the planted errors: ([w], [Z]).  Read only."""
    case = cases(n, problem)
    ws, Zs = [], []
    for b in range(COUNT):
        w, Z = window(case, b, c)
        if plant:
            w, Z = planted(w, Z, 9000 + 131 * n + 7 * c + b)
        w.setflags(write=False)
        Z.setflags(write=False)
        ws.append(w)
        Zs.append(Z)
    return ws, Zs


def mirror(A, B, w, Z):
    """The host mirror on the window's columns: (out of 4, ipr of c)."""
    a_norm, ave, mx = verifier.eval_residual_norm(A, w, Z, B)
    return np.array([a_norm, ave, mx, verifier.eval_orthogonality(Z, B)]), verifier.get_ipratios(Z, B)


@functools.lru_cache(maxsize=None)
def mirrors(n, problem, c, plant):
    case = cases(n, problem)
    ws, Zs = windows(n, problem, c, plant)
    return [mirror(case.A[b], case.B[b] if problem else None, ws[b], Zs[b]) for b in range(COUNT)]


def longdouble(A, B, w, Z):
    """The same quantities with every product and sum in long double."""
    L = np.longdouble
    A, w, Z = A.astype(L), w.astype(L), Z.astype(L)
    S = B.astype(L) @ Z if B is not None else Z
    a_norm = np.sqrt((A * A).sum())
    R = A @ Z - S * w
    norms = np.sqrt((R * R).sum(axis=0))
    G = Z.T @ S
    g = np.diag(G).copy()
    s = 1.0 / np.sqrt(g)
    Gs = G * s[:, None] * s[None, :]
    np.fill_diagonal(Gs, 0.0)
    out = np.array([a_norm, norms.sum() / a_norm / Z.shape[1], norms.max() / a_norm, np.sqrt((Gs * Gs).sum())])
    return out, ((Z * Z) ** 2).sum(axis=0) / g ** 2


def tol(n):
    return 4 * max(n, 8) * EPS


def shares(out, ipr, ref_out, ref_ipr, n):
    """|difference| / tolerance per quantity: a_norm and the IPRs relative, the other three absolute."""
    t = tol(n)
    s = np.abs(np.asarray(out, dtype=np.longdouble) - ref_out) / t
    s[0] /= abs(ref_out[0])
    return np.append(s, (np.abs(np.asarray(ipr, dtype=np.longdouble) - ref_ipr) / np.abs(ref_ipr)).max() / t).astype(float)
