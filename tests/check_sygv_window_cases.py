"""The table behind the tests of the window check of DSYGV's types (ek_hip_check_sygv_window_xbatched*):
tests/check_window_cases.py's orders, column counts, seeded matrices (_sym, _spd with cond 10), planted errors and
tolerance, with the pairs drawn from SciPy's eigh(A, B, type=itype), the host mirror eigenkernel_amd.verifier.*_sygv on
the window's columns, and a long-double evaluation of types 2 and 3.  Plain functions, no fixtures;
tests/test_check_sygv_window_host.py pins the mirror on the CPU, tests/test_gpu_check_sygv_window.py runs the kernel
against it.

The tolerance is the project's 4 max(n, 8) eps -- relative for slot 0 and every IPR, absolute for slots 1 .. 3 --
multiplied by max(1, cond_2(B)) for slot 3 and the IPRs of type 3: two exact factors of B lie cond(B) eps apart
(tests/test_gpu_check_sygv_xbatched.py).  cond_2(B) <= 16 is asserted where the pairs are made."""
import functools

import numpy as np
import scipy.linalg as sl

import check_window_cases as cw
from eigenkernel_amd import verifier

EPS = cw.EPS
ORDERS = cw.ORDERS
COUNT = cw.COUNT
NAMES = ("norm", "res_ave", "res_max", "orthogonality", "ipr")
columns = cw.columns
planted = cw.planted
tol = cw.tol


class Case:
    pass


@functools.lru_cache(maxsize=None)
def cases(n, itype):
    """COUNT seeded pencils of order n, SciPy's full w and Z of the type, cond_2(B) of each.  Read only."""
    rng = np.random.default_rng(36000 + n)
    A = np.stack([cw._sym(rng, n) for _ in range(COUNT)])
    B = np.stack([cw._spd(rng, n) for _ in range(COUNT)])
    w, Z = np.zeros((COUNT, n)), np.zeros((COUNT, n, n))
    for b in range(COUNT):
        w[b], Z[b] = sl.eigh(A[b], B[b], type=itype, lower=True)
    c = Case()
    c.n, c.A, c.B, c.w, c.Z = n, A, B, w, Z
    c.cond = np.array([np.linalg.cond(B[b]) for b in range(COUNT)])
    assert c.cond.max() <= 16.0, c.cond             # small enough for the bounds of type 3 to mean something
    for a in (A, B, w, Z, c.cond):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def window(n, itype, b, c, plant):
    """The c pairs in the middle of problem b's spectrum, clean or with the planted errors: (w of c, Z of n x c).  Read
    only."""
    case = cases(n, itype)
    first = (n - c) // 2
    w, Z = case.w[b, first:first + c].copy(), case.Z[b][:, first:first + c].copy()
    if plant:
        w, Z = planted(w, Z, 9100 + 131 * n + 7 * c + b)
    w.setflags(write=False)
    Z.setflags(write=False)
    return w, Z


def mirror(itype, A, B, w, Z):
    """The host mirror on the window's columns: (out of 4, ipr of c)."""
    norm, ave, mx = verifier.eval_residual_norm_sygv(itype, A, B, w, Z)
    return (np.array([norm, ave, mx, verifier.eval_orthogonality_sygv(itype, Z, B)]),
            verifier.get_ipratios_sygv(itype, Z, B))


@functools.lru_cache(maxsize=None)
def mirrored(n, itype, b, c, plant):
    case = cases(n, itype)
    w, Z = window(n, itype, b, c, plant)
    return mirror(itype, case.A[b], case.B[b], w, Z)


def longdouble(itype, A, B, w, Z):
    """The quantities of types 2 and 3 with every product, sum, factor and solve in long double."""
    assert itype in (2, 3)
    T = np.longdouble
    A, B, w, Z = A.astype(T), B.astype(T), w.astype(T), Z.astype(T)
    n, c = Z.shape
    norm = np.sqrt((A * A).sum()) * np.sqrt((B * B).sum())
    R = (A @ (B @ Z) if itype == 2 else B @ (A @ Z)) - Z * w
    rho = np.sqrt((R * R).sum(axis=0)) / (norm * np.sqrt((Z * Z).sum(axis=0)))
    if itype == 2:
        G = Z.T @ (B @ Z)
    else:
        L = np.tril(B)
        for k in range(n):
            L[k, k] = np.sqrt(L[k, k])
            L[k + 1:, k] /= L[k, k]
            L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
        W = Z.copy()
        for k in range(n):
            W[k] /= L[k, k]
            W[k + 1:] -= np.outer(L[k + 1:, k], W[k])
        G = W.T @ W
    g = np.diag(G).copy()
    s = 1.0 / np.sqrt(g)
    Gs = G * s[:, None] * s[None, :]
    np.fill_diagonal(Gs, 0.0)
    return np.array([norm, rho.sum() / c, rho.max(), np.sqrt((Gs * Gs).sum())]), ((Z * Z) ** 2).sum(axis=0) / g ** 2


def shares(itype, out, ipr, ref_out, ref_ipr, n, cond):
    """|difference| / bound per quantity: slot 0 and the IPRs relative, the other three absolute; slot 3 and the IPRs of
    type 3 with max(1, cond_2(B)) in the bound.  NaN against NaN uses nothing, NaN against a number everything."""
    t = tol(n)
    wide = t * (max(1.0, float(cond)) if itype == 3 else 1.0)

    def share(x, y, bound):
        x, y = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
        both = np.isnan(x) & np.isnan(y)
        with np.errstate(invalid="ignore"):
            s = np.abs(x - y) / bound
        s = np.where(both, 0.0, s)
        return float(np.where(np.isnan(s), np.inf, s).max())

    return np.array([share(out[0], ref_out[0], t * abs(ref_out[0])), share(out[1], ref_out[1], t),
                     share(out[2], ref_out[2], t), share(out[3], ref_out[3], wide),
                     share(ipr, ref_ipr, wide * np.abs(ref_ipr))])
