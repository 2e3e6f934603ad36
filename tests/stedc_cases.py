"""Hard symmetric tridiagonals (d, e) for the divide & conquer stage, shared by tests/test_stedc_cases_host.py (no GPU)
and tests/test_gpu_stedc.py.  Pure numpy: seeded, any order n >= 2.

The classes are chosen for the branches of ek_stedc.hip's merge (deflation fast path, sequential DLAED2 scan with its
state carried over 1024-pole chunks, the all-deflate branch, the even-offset rule of the second product, the sign of the
off-diagonal at a split) rather than for their spectra:

  graded_down      d_i = 10^(-12 i/(n-1)), e_i = 0.5 * 10^(-12 (i+0.5)/(n-1)): twelve decades, large end first
  graded_up        the same reversed
  clement          d = 0, e_i = sqrt((i+1)(n-1-i)): spectrum exactly -(n-1), -(n-3), ..., n-1; at the top merge the two
                   halves share their spectra, so every pole is one of a close pair and is rotated
  legendre         d = 0, e_k = k / sqrt(4k^2 - 1) (Gauss-Legendre's Jacobi matrix): nothing deflates
  laguerre         d_i = 2i+1, e_i = i+1 (Gauss-Laguerre's): tiny-z deflation only
  wilkinson_glued  W_21^+ blocks (d = |j - 10|, e = 1) glued by 1e-7: clusters of hundreds, many rotations
  cluster_eps      d = 1 + eps * randint(0, 8), e = 1e-3 * eps * U(0.5, 1): everything within a few eps
  negative_e       d ~ U(-1, 1), e = -|U(0.1, 1)|
  mixed_sign_e     the same with only every third e negative
  zero_at_splits   random (d, e) with e = 0 exactly at the top split and at the first half's split
  tiny_at_splits   random (d, e) with e = 1e-18 at the top split and -1e-15 at the second half's
  huge / tiny      1e150 / 1e-150 times mixed_sign_e
  large_e          d = 1e-8 * U(-1, 1), e ~ U(0.5, 1): +- pairs
  repeated_blocks  the 1-2-1 matrix cut into identical blocks of 16 (e = 0 after every 16th row): 16 distinct values
  localized        d a random permutation of 0..n-1, e = 1e-3 * U(0.5, 1): eigenvectors are near unit vectors
  one_big          d = 1 except d[n/3] = 1e8, e = 1e-4: one pole sets the scale, the rest is a cluster relative to it

top_merge_counts replays the deflation scan of the top merge (dc_sort_kernel / dc_deflate_kernel) in numpy from the
eigenpairs of the two halves, with the kernel's own tolerance, so that a test can tell which branch a class takes.
"""
import functools
import os

import numpy as np

EPS = 2.220446049250313e-16        # n eps in the bounds
LEAF = 32                          # order up to which the stage solves by implicit QL (no merge)

CLASSES = ("graded_down", "graded_up", "clement", "legendre", "laguerre", "wilkinson_glued", "cluster_eps", "negative_e",
           "mixed_sign_e", "zero_at_splits", "tiny_at_splits", "huge", "tiny", "large_e", "repeated_blocks", "localized",
           "one_big")

# the bounds of tests/test_gpu_path.py::test_stedc_matches_oracle, in units of n eps scale (n eps for the orthogonality)
BOUND_W, BOUND_RES, BOUND_ORTH = 4.0, 32.0, 32.0


# orders at which the oracle's eigenvalues come from a recorded file (tools/stedc_golden.py writes it), not from a fresh run
RECORDED_ORDERS = (1100, 2100)
RECORDED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stedc_oracle_spectra.npz")


@functools.lru_cache(maxsize=None)
def _recorded():
    with np.load(RECORDED_PATH) as f:
        return {k: f[k] for k in f.files}


def recorded_spectrum(name, n):
    """Eigenvalues of class `name` at order n as oracle.stedc computed them (n in RECORDED_ORDERS); a fresh array."""
    return _recorded()["%s_%d" % (name, n)].copy()


def _rng(name, n):
    return np.random.default_rng([CLASSES.index(name), n])


def _mixed(n, rng):
    d = rng.uniform(-1, 1, n)
    e = np.abs(rng.uniform(0.1, 1, n - 1))
    e[2::3] = -e[2::3]
    return d, e


def tridiagonal(name, n):
    """(d, e) of class `name` at order n >= 2 (fresh float64 arrays of n and n - 1 entries)."""
    assert n >= 2
    rng = _rng(name, n)
    i = np.arange(n, dtype=np.float64)
    j = np.arange(n - 1, dtype=np.float64)
    if name in ("graded_down", "graded_up"):
        d = 10.0 ** (-12.0 * i / (n - 1))
        e = 0.5 * 10.0 ** (-12.0 * (j + 0.5) / (n - 1))
        return (d, e) if name == "graded_down" else (d[::-1].copy(), e[::-1].copy())
    if name == "clement":
        return np.zeros(n), np.sqrt((j + 1) * (n - 1 - j))
    if name == "legendre":
        k = j + 1
        return np.zeros(n), k / np.sqrt(4 * k * k - 1)
    if name == "laguerre":
        return 2 * i + 1, j + 1
    if name == "wilkinson_glued":
        d = np.tile(np.abs(np.arange(21.0) - 10.0), n // 21 + 1)[:n]
        e = np.ones(n - 1)
        e[20::21] = 1e-7
        return d, e
    if name == "cluster_eps":
        return 1.0 + EPS * rng.integers(0, 8, n), 1e-3 * EPS * rng.uniform(0.5, 1, n - 1)
    if name == "negative_e":
        return rng.uniform(-1, 1, n), -np.abs(rng.uniform(0.1, 1, n - 1))
    if name == "mixed_sign_e":
        return _mixed(n, rng)
    if name == "zero_at_splits":
        d, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1)
        e[n // 2 - 1] = 0.0
        if (n // 2) // 2 - 1 >= 0:
            e[(n // 2) // 2 - 1] = 0.0
        return d, e
    if name == "tiny_at_splits":
        d, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1)
        s2 = n // 2 + (n - n // 2) // 2 - 1
        if n // 2 - 1 < s2 < n - 1:
            e[s2] = -1e-15
        e[n // 2 - 1] = 1e-18
        return d, e
    if name in ("huge", "tiny"):
        d, e = _mixed(n, rng)
        f = 1e150 if name == "huge" else 1e-150
        return f * d, f * e
    if name == "large_e":
        return 1e-8 * rng.uniform(-1, 1, n), rng.uniform(0.5, 1, n - 1)
    if name == "repeated_blocks":
        e = -np.ones(n - 1)
        e[15::16] = 0.0
        return 2.0 * np.ones(n), e
    if name == "localized":
        return rng.permutation(n).astype(np.float64), 1e-3 * rng.uniform(0.5, 1, n - 1)
    if name == "one_big":
        d = np.ones(n)
        d[n // 3] = 1e8
        return d, 1e-4 * np.ones(n - 1)
    raise ValueError(name)


def exact_spectrum(name, n):
    """The spectrum in closed form (ascending) for the classes that have one, else None."""
    if name == "clement":
        return np.arange(-(n - 1), n, 2, dtype=np.float64)
    if name == "repeated_blocks":
        sizes = [16] * (n // 16) + ([n % 16] if n % 16 else [])
        return np.sort(np.concatenate([2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1)) for m in sizes]))
    return None


def apply_tridiagonal(d, e, Z):
    """T Z for T = tridiag(e, d, e), in O(n cols) (no dense T)."""
    R = d[:, None] * Z
    R[:-1] += e[:, None] * Z[1:]
    R[1:] += e[:, None] * Z[:-1]
    return R


def scale_of(d, e):
    return max(float(np.abs(d).max()), float(np.abs(e).max()) if len(e) else 0.0, 1e-300)


# ------------------------------------------------------------------------------------------------ the selection's ranks
def numroc(n, nb, me, nprocs):
    """NUMROC with the first block on process 0: columns of n that process `me` of `nprocs` owns at block width nb."""
    nblocks = n // nb
    num = (nblocks // nprocs) * nb
    extra = nblocks % nprocs
    if me < extra:
        num += nb
    elif me == extra:
        num += n % nb
    return num


def sel_rank(l, first, nb, npcol, mycol):
    """0-based rank of the eigenpair a selection's column l carries (sel_rank of ek_stedc.hip)."""
    l = np.asarray(l)
    return first + ((l // nb) * npcol + mycol) * nb + l % nb


def is_compact(n, nsel):
    """Whether the stage keeps its bases compact (n x nsel output array) for nsel selected columns."""
    return n > LEAF and 0 <= nsel < n and nsel <= n - n // 2


# ------------------------------------------------------------------------------------------------ the top merge's scan
def split_halves(d, e):
    """The two half problems of the top merge as the stage poses them: (d, e) scaled by max|T|, |e_s| at the split
    (s = n/2 - 1) subtracted from the two diagonal entries next to it.  Returns ((d1, e1), (d2, e2))."""
    n = len(d)
    n1 = n // 2
    nrm = scale_of(d, e)
    ds, es = np.asarray(d, dtype=np.float64) / nrm, np.asarray(e, dtype=np.float64) / nrm
    rho = abs(es[n1 - 1])
    ds[n1 - 1] -= rho
    ds[n1] -= rho
    return (ds[:n1].copy(), es[:n1 - 1].copy()), (ds[n1:].copy(), es[n1:].copy())


def top_merge_counts(d, e, halves, types=False):
    """Replay of the top merge's deflation (dc_sort_kernel, dc_deflate_kernel) from the eigenpairs ((w1, Q1), (w2, Q2))
    of split_halves(d, e): z from the last row of Q1 and the first row of Q2 (its sign flipped when e at the split is
    negative), the poles sorted ascending, the tiny-z test rho |z_i| <= tol and DLAED2's close-pair test
    |(d_i - d_p) z_i z_p| <= tol (z_i^2 + z_p^2) with tol = 8 * 2^-53 * max(max|d|, max|z|), rho = 2 |e_s| / max|T|.
    Returns (deflated, rotations, k); with types=True also (k1, k2, k3), the survivors that are non-zero in the top rows
    only, dense (a rotated pair from both halves) and in the bottom rows only."""
    (w1, Q1), (w2, Q2) = halves
    n = len(d)
    n1 = n // 2
    es = e[n1 - 1] / scale_of(d, e)
    is2 = 0.70710678118654752440
    z = np.concatenate([Q1[-1, :] * is2, (-1.0 if es < 0 else 1.0) * Q2[0, :] * is2])
    poles = np.concatenate([w1, w2])
    order = np.argsort(poles, kind="stable")
    ds, zs, origin = poles[order], z[order], order
    rho = abs(2.0 * es)
    tol = 8.0 * 2.0 ** -53 * max(np.abs(ds).max(), np.abs(zs).max())
    if rho * np.abs(zs).max() <= tol:
        return ((n, 0, 0), (0, 0, 0)) if types else (n, 0, 0)
    ndf = nrot = 0
    cnt = [0, 0, 0, 0]
    have, dp, zp, tp = False, 0.0, 0.0, 0
    for i in range(n):
        zi, di = float(zs[i]), float(ds[i])
        ti = 1 if origin[i] < n1 else 3
        if rho * abs(zi) <= tol:
            ndf += 1
            continue
        if not have:
            have, dp, zp, tp = True, di, zi, ti
            continue
        tau2 = zi * zi + zp * zp
        if abs((di - dp) * zi * zp) <= tol * tau2:
            tau = np.sqrt(tau2)
            c, s = zi / tau, -zp / tau
            nrot += 1
            ndf += 1
            dp, zp, tp = dp * s * s + di * c * c, tau, (ti if tp == ti else 2)
        else:
            cnt[tp] += 1
            dp, zp, tp = di, zi, ti
    if have:
        cnt[tp] += 1
    k = cnt[1] + cnt[2] + cnt[3]
    assert k + ndf == n
    return ((ndf, nrot, k), (cnt[1], cnt[2], cnt[3])) if types else (ndf, nrot, k)
