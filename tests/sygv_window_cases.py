"""Cases and the judge for the window entries of DSYGV's problem types 2 and 3 (ek_hip_sygv_window_batched*,
ek_hip_sygv_window_xbatched*): A B x = l x and B A x = l x, a window of eigenpairs per pencil.  Plain functions, no
fixtures; tests/test_sygv_window_batched_host.py pins them on the CPU against LAPACK's own windowed driver (DSYGVX),
tests/test_gpu_sygv_window_batched.py and tests/test_gpu_sygv_window_xbatched.py run the kernels against them.

The truth is SciPy's full driver of the type, sliced (scipy.linalg.eigh(A, B, type=itype, lower=True)).  The windows, the
'V' bounds and the cluster cuts are those of tests/window_batched_cases.py.

Bounds (none is new): eigenvalues 4 max(n, 8) eps max|w_ref| over the WHOLE reference spectrum; the vectors with the
normalisations of tests/test_gpu_sygv_batched.py::_quantities, against np.eye(m) for the m columns of a window,

  residual       max_j |M z_j - w_j z_j|_2 / (max|A| |B|_2 |z_j|_2),  M = A B (type 2), B A (type 3)       <= 256 n eps
  orthogonality  max|Z^T B Z - I_m| (type 2),  max|(L^-1 Z)^T (L^-1 Z) - I_m| (type 3, B = L L^T)          <= 256 n eps

and for the hard pencils that suite's rule: eigenvalues as above with no cond(B) factor, residual and orthogonality
<= 4 max(LAPACK's full driver's own on the whole pencil, 16 n eps); type 3's orthogonality of a library result is
measured with the factor the library left in dB (held to max|L L^T - B| <= 16 n eps max|B|), LAPACK's with LAPACK's.

Planted clusters: C = batched_cases.make(name, n).A for the five names of window_batched_cases.CLUSTERED, B = M M^T / n
+ I from a seeded normal M (one B per order; cond2(B) 4.5 .. 5.2 at orders 33 .. 256), A = L^-T C L^-1 symmetrised, so that
L^T A L = C: the pencil of types 2 and 3 has C's spectrum, clusters included."""
import ctypes

import numpy as np
import scipy.linalg as sl

import batched_cases as bc
import window_batched_cases as wc

EPS = 2.220446049250313e-16
HARD = ("cond_b:1e6", "cond_b:1e10", "a_equals_b", "band5_band5")
ILL = ("cond_b:1e6", "cond_b:1e10")
_ip = ctypes.POINTER(ctypes.c_int)

_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def pairs(n, batch=8):
    """Seeded random pairs (A symmetric, B SPD with cond 10) of order n, made once: (batch, n, n) each."""
    key = ("pairs", n, batch)
    if key not in _cache:
        rng = np.random.default_rng(77000 + n)
        A, B = [], []
        for _ in range(batch):
            G = rng.standard_normal((n, n))
            A.append((G + G.T) / 2.0)
            Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
            d = np.logspace(0.0, 1.0, n) if n > 1 else np.array([10.0])
            Bm = (Q * d) @ Q.T
            B.append((Bm + Bm.T) / 2.0)
        _cache[key] = _frozen(np.stack(A), np.stack(B))
    return _cache[key]


def planted(name, n):
    """(A, B, C) with L^T A L = C = batched_cases.make(name, n).A, B = L L^T (module docstring), made once."""
    key = ("planted", name, n)
    if key not in _cache:
        C = bc.make(name, n).A
        M = np.random.default_rng(41000 + n).standard_normal((n, n))      # one B per order
        B = M @ M.T / n + np.eye(n)
        B = (B + B.T) / 2.0
        L = np.linalg.cholesky(B)
        X = sl.solve_triangular(L, C, lower=True, trans="T")             # L^-T C
        A = sl.solve_triangular(L, X.T, lower=True, trans="T").T        # (L^-T (L^-T C)^T)^T = L^-T C L^-1
        A = (A + A.T) / 2.0
        _cache[key] = _frozen(A, B, C)
    return _cache[key]


def hard(name, n):
    """(A, B) of a hard pencil of tests/batched_cases.py, made once."""
    key = ("hard", name, n)
    if key not in _cache:
        c = bc.make(name, n)
        _cache[key] = _frozen(np.array(c.A), np.array(c.B))
    return _cache[key]


def reference(key, itype, A, B):
    """scipy.linalg.eigh(A, B, type=itype, lower=True): (w, Z), computed once per (key, itype) and never modified."""
    k = ("ref", key, itype)
    if k not in _cache:
        _cache[k] = _frozen(*sl.eigh(A, B, type=itype, lower=True))
    return _cache[k]


def quantities(itype, A, B, w, Z, L=None):
    """(residual, orthogonality) of the m columns of Z as plain numbers, test_gpu_sygv_batched.py::_quantities with
    np.eye(m).  L: the factor type 3's orthogonality is measured with (None: np.linalg.cholesky(B))."""
    m = Z.shape[1]
    MZ = A @ (B @ Z) if itype == 2 else B @ (A @ Z)
    R = MZ - Z * w
    scale = np.abs(A).max() * np.linalg.norm(B, 2)
    res = (np.linalg.norm(R, axis=0) / (scale * np.linalg.norm(Z, axis=0))).max()
    if itype == 2:
        G = Z.T @ (B @ Z)
    else:
        Y = sl.solve_triangular(np.linalg.cholesky(B) if L is None else L, Z, lower=True)
        G = Y.T @ Y
    return res, np.abs(G - np.eye(m)).max()


def judge(itype, A, B, w_ref, first, w, Z, what, ev_part=1.0, vec_part=1.0, rule=None, L=None):
    """The m = len(w) pairs (w, Z) of type itype against indices first .. first + m - 1 (0-based) of the full reference
    spectrum w_ref; Z None: values only.  ev_part / vec_part: the part of each bound that is allowed.  rule: None, or
    (residual, orthogonality) of LAPACK's full driver on the whole pencil -- the vector bounds are then 4 max(its own,
    16 n eps) instead of 256 n eps.  Returns ([share of the eigenvalue, residual, orthogonality bound], failures)."""
    n, m = A.shape[0], len(w)
    fails = []
    if m == 0:
        return None, fails
    with np.errstate(all="ignore"):
        if not np.all(np.isfinite(w)):
            return None, ["%s: a non-finite eigenvalue" % what]
        if Z is not None and not np.all(np.isfinite(Z)):
            return None, ["%s: a non-finite vector entry" % what]
        if not np.all(np.diff(w) >= 0):
            fails.append("%s: w not ascending" % what)
        tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max() * ev_part
        err = np.abs(w - w_ref[first:first + m]).max()
        shares = [err / tol, None, None]
        if not err <= tol:
            fails.append("%s: eigenvalues, error %.3e > %.3e" % (what, err, tol))
        if Z is not None:
            res, orth = quantities(itype, A, B, w, Z, L)
            if rule is None:
                lim_r = lim_o = 256 * n * EPS * vec_part
            else:
                lim_r, lim_o = (4 * max(x, 16 * n * EPS) * vec_part for x in rule)
            shares[1:] = [res / lim_r, orth / lim_o]
            if not res <= lim_r:
                fails.append("%s: residual %.3e > %.3e" % (what, res, lim_r))
            if not orth <= lim_o:
                fails.append("%s: orthogonality %.3e > %.3e" % (what, orth, lim_o))
    return shares, fails


def worse(worst, shares):
    return worst if not shares else [max(x, y or 0.0) for x, y in zip(worst, shares)]


# ------------------------------------------------------------------------------------------------------ on the GPU
def window_device(lib, entry, first, A, B, jobz, il=None, iu=None, vl=None, vu=None, zcap=None, pad=0, gap=0):
    """A device window entry (`entry`, its argument 1 = `first`: problem or itype) on images with NaN wherever the kernel
    must neither read nor write: tests/test_gpu_window_batched.py::_window_device with the entry as a parameter, and the
    same fields in what it returns (_untouched of that file takes it)."""
    from test_gpu_vbatched import _Dev, _Out
    from test_gpu_window_batched import _image, _pack_lower
    batch, n = A.shape[0], A.shape[1]
    by_value = vl is not None or vu is not None
    if zcap is None:
        zcap = n if by_value else iu - il + 1
    ld = n + pad
    sM, sZ = ld * n + gap, ld * max(zcap, 1) + gap
    o = _Out()
    hA = _pack_lower(A, ld, sM)
    hB = _pack_lower(B, ld, sM) if B is not None else None
    hZ = np.full(max(batch * sZ, 1), np.nan)
    hw = np.full(max(batch * n, 1), np.nan)
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    m = np.full(max(batch, 1), 777, dtype=np.int32)
    with _Dev(lib) as dev:
        dA = dev.up(hA)
        dB = dev.up(hB) if B is not None else None
        dw, dZ = dev.up(hw), dev.up(hZ)
        o.rc = getattr(lib, entry)(first, jobz, 1 if by_value else 0, n, batch, -np.inf if vl is None else vl,
                                   np.inf if vu is None else vu, il or 0, iu or 0, dA, ld, sM, dB, ld, sM,
                                   m.ctypes.data_as(_ip), dw, dZ if jobz else None, ld, zcap, sZ, info.ctypes.data_as(_ip),
                                   None)
        o.info, o.m = info[:batch].copy(), m[:batch].copy()
        o.w = dev.down(dw, hw)[:batch * n].reshape(batch, n)
        o.flatZ = dev.down(dZ, hZ)
        o.flatA = dev.down(dA, hA)
        o.flatB = dev.down(dB, hB) if B is not None else None
    o.Z = np.empty((batch, n, max(zcap, 1)))
    for b in range(batch):
        o.Z[b] = o.flatZ[b * sZ:b * sZ + ld * max(zcap, 1)].reshape(max(zcap, 1), ld)[:, :n].T
    o.A = _image(o.flatA, batch, n, ld, sM)
    o.B = _image(o.flatB, batch, n, ld, sM) if B is not None else None
    o.before = (hA, hB)
    o.ld, o.sM, o.sZ, o.zcap = ld, sM, sZ, zcap
    return o
