"""Inputs, references and bounds of the back-transformation's stage tests (tests/test_ormtr_cases_host.py, no GPU, and
tests/test_gpu_ormtr_stages.py): Z <- Q Z, Q = H(0) H(1) ... H(n-2), H(j) = I - tau_j v_j v_j^T (ek_ormtr.hip).

Reflector classes, each made on the host by DLARFG from seeded random columns (v = 1 at the unit entry, |v_i| <= 1,
1 <= tau <= 2; a column DLARFG finds nothing to annihilate in is the identity: tau = 0 and, here, v = 0):
    random   uniform(-1, 1) columns, the unit entry at row j + 1
    graded   the same, every entry scaled by its own 10**uniform(-12, 0)
    tau0     random with every third reflector the identity
    band     the dense-to-band stage's form: the unit entry at row j + 64, zero from the diagonal down to it, so the
             last 64 reflectors are the identity (no packed form)

The reference is the plain sequential application, one rank-1 update per reflector, H(n-2) first, in numpy.longdouble, on
a sample of at most 8 columns (columns are independent); every column is checked through the projection identity
(Q Z)^T y = Z^T (Q^T y) with three seeded sign vectors y, Q^T y by the same sequential code.

Bounds: elementwise |got - ref| <= n EPS max|ref|; a float64 numpy emulation of the kernels' algorithm (emulate below)
and the plain float64 sequential application stay below 0.012 and 0.016 of it (orders 1100, 1537 and 4200, every class,
widths 7 to 129), which leaves a factor of about 80 for another summation order inside the GEMMs and the K slices.  The
projection is a sum of n entries: n times the elementwise bound."""
import functools

import numpy as np

EPS = 2.220446049250313e-16
KB = 512               # reflectors per compact-WY block (ek_ormtr.hip)
BAND = 64              # half bandwidth of the dense-to-band stage
SPLIT_MIN_ROWS = 4096  # W1 = V_b^T Z is cut along K only from this many rows on
SPLIT_MAX = 16

CLASSES = ("random", "graded", "tau0", "band")
PACKED_CLASSES = ("random", "graded", "tau0")
EDGE_ORDERS = (513, 514, 1024, 1025, 1026, 1537)
SPLIT_ORDERS = (4096, 4097, 4610)
WIDTHS = (1, 7, 129, 2304, None)          # None: n
SAMPLE_COLUMNS = (0, 1, 127, 128, 511, 512)
LD = np.longdouble


def width(n, w):
    return n if w is None else w


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the mirror of ormtr_apply's choice of form
def ormtr_split(ncols_global):
    tiles = (KB // 128) * _ceil_div(ncols_global if ncols_global > 0 else 1, 128)
    s = min(512 // tiles, SPLIT_MAX)
    return s if s >= 2 else 1


def slices(m, smax):
    """(kc, S, klast) of one block whose product runs over m rows: S slices of kc rows, the last of klast"""
    kc = _ceil_div(m, smax)
    kc += kc & 1
    s = _ceil_div(m, kc) if (smax > 1 and m >= SPLIT_MIN_ROWS) else 1
    return kc, s, (m - (s - 1) * kc if s > 1 else m)


def block_forms(n, ncols_global):
    """one record per block of 512 reflectors, the last block first (the order of the sweep)"""
    nrefl = n - 1
    smax = ormtr_split(ncols_global)
    out = []
    for b in range(_ceil_div(max(nrefl, 0), KB) - 1, -1, -1):
        c0 = b * KB
        m = n - c0
        kc, s, klast = slices(m, smax)
        out.append(dict(b=b, c0=c0, kb=min(KB, nrefl - c0), m=m, smax=smax, kc=kc, S=s, klast=klast))
    return out


def slab_widths(ncols, zslab):
    """the widths Path::slab_width yields for ncols columns (ek_solve.hip): the last slabs are narrower"""
    out, c0 = [], 0
    while c0 < ncols:
        left = ncols - c0
        if zslab >= ncols:
            w = left
        elif left > 2 * zslab:
            w = zslab
        elif left > zslab:
            w = min(zslab // 2, left)
        else:
            w = (left + 1) // 2 if left > 512 else left
        out.append(w)
        c0 += w
    return out


# ------------------------------------------------------------------ inputs
_STREAMS = ("reflectors", "packed", "columns", "signs")


def _seed(stream, *key):
    """the seed of one generator: its stream, then the class's index or the integers that name the case"""
    return [_STREAMS.index(stream)] + [CLASSES.index(k) if isinstance(k, str) else int(k) for k in key]


@functools.lru_cache(maxsize=2)
def reflectors(cls, n):
    """(V, tau): V n x n explicit (column j = v_j, zero above the unit entry, column n - 1 zero), tau (n - 1); read-only"""
    assert cls in CLASSES
    rng = np.random.default_rng(_seed("reflectors", cls, n))
    off = BAND if cls == "band" else 1
    X = rng.uniform(-1.0, 1.0, (n, n))
    if cls == "graded":
        X *= 10.0 ** rng.uniform(-12.0, 0.0, (n, n))
    rows = np.arange(n)[:, None]
    unit = np.arange(n)[None, :] + off                       # the row of column j's unit entry
    X = np.asfortranarray(np.where(rows >= unit, X, 0.0))
    ncol = max(n - off, 0)                                   # columns that have a unit row at all
    alpha = np.zeros(n)
    alpha[:ncol] = X[np.arange(off, n), np.arange(ncol)]
    below = np.where(rows > unit, X, 0.0)
    xnorm = np.sqrt((below * below).sum(axis=0))
    beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
    live = xnorm > 0.0
    if cls == "tau0":
        live &= (np.arange(n) % 3 != 2)
    tau = np.where(live, (beta - alpha) / np.where(live, beta, 1.0), 0.0)
    V = below / np.where(live, alpha - beta, 1.0)[None, :] + 0.0       # (+ 0.0: no negative zeros above the unit entry)
    V[:, ~live] = 0.0
    j = np.nonzero(live)[0]
    V[j + off, j] = 1.0
    V = np.asfortranarray(V)
    tau = np.ascontiguousarray(tau[:max(n - 1, 0)])
    assert not live[n - 1:].any()
    V.setflags(write=False)
    tau.setflags(write=False)
    return V, tau


def packed(cls, n, fill=None):
    """the same reflectors in PDSYTRD storage: v_j below the subdiagonal of column j (the unit entry implied), seeded
    random numbers -- or `fill` -- on and above the subdiagonal, which the back-transformation never reads"""
    assert cls in PACKED_CLASSES
    V, tau = reflectors(cls, n)
    rng = np.random.default_rng(_seed("packed", cls, n))
    A = rng.uniform(-1.0, 1.0, (n, n)) if fill is None else np.full((n, n), fill)
    keep = np.tri(n, n, -2, dtype=bool)
    return np.asfortranarray(np.where(keep, V, A)), tau


def unpack(A):
    """explicit V of a PDSYTRD-packed A, as build_v_kernel forms it: 1 on the subdiagonal, A below it, 0 elsewhere"""
    n = A.shape[0]
    V = np.where(np.tri(n, n, -2, dtype=bool), A, 0.0)
    j = np.arange(n - 1)
    V[j + 1, j] = 1.0
    return np.asfortranarray(V)


@functools.lru_cache(maxsize=2)
def columns(n, ncols):
    Z = np.asfortranarray(np.random.default_rng(_seed("columns", n, ncols)).uniform(-1.0, 1.0, (n, ncols)))
    Z.setflags(write=False)
    return Z


def sample_columns(ncols):
    if ncols <= 8:
        return list(range(ncols))
    return sorted({c for c in SAMPLE_COLUMNS + (ncols - 1,) if c < ncols})


# ------------------------------------------------------------------ references
def apply_sequential(V, tau, Z, trans=False, dtype=LD):
    """H(0) ... H(n-2) Z (trans: H(n-2) ... H(0) Z = Q^T Z), one rank-1 update per reflector, in `dtype`"""
    n = V.shape[0]
    W = np.array(Z, dtype=dtype, order="C")
    W = W.reshape(n, -1)
    order = range(n - 1) if trans else range(n - 2, -1, -1)
    for j in order:
        if tau[j] == 0.0:
            continue
        v = V[j + 1:, j].astype(dtype)
        W[j + 1:] -= np.multiply.outer(dtype(tau[j]) * v, v @ W[j + 1:])
    return W


def emulate(V, tau, Z):
    """float64 numpy emulation of ek_ormtr.hip: blocks of 512 reflectors, T by the DLARFT recurrence from the Gram matrix,
    three products per block, the last block first"""
    n = V.shape[0]
    nrefl = n - 1
    W = np.array(Z, dtype=np.float64, order="F")
    for b in range(_ceil_div(max(nrefl, 0), KB) - 1, -1, -1):
        c0 = b * KB
        kb = min(KB, nrefl - c0)
        Vb = V[c0:, c0:c0 + kb]
        G = Vb.T @ Vb
        T = np.zeros((kb, kb))
        for i in range(kb):
            T[i, i] = tau[c0 + i]
            if i:
                T[:i, i] = -tau[c0 + i] * (T[:i, :i] @ G[:i, i])
        W[c0:] -= Vb @ (T @ (Vb.T @ W[c0:]))
    return W


def sign_vectors(n):
    return np.random.default_rng(_seed("signs", n)).choice([-1.0, 1.0], size=(n, 3))


def make_reference(V, tau, Z):
    """what the checks need of one case, all in long double: the sample columns of Q Z, Z^T (Q^T y) for the three sign
    vectors y, and the scale max|ref| of the bounds"""
    n, ncols = Z.shape
    cols = sample_columns(ncols)
    ref = apply_sequential(V, tau, Z[:, cols]) if cols else np.zeros((n, 0), dtype=LD)
    Y = sign_vectors(n)
    q = apply_sequential(V, tau, Y, trans=True)
    ztq = Z.T.astype(LD) @ q
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return dict(n=n, ncols=ncols, cols=cols, ref=ref, Y=Y.astype(LD), ztq=ztq, scale=scale)


@functools.lru_cache(maxsize=8)
def reference(cls, n, ncols):
    """the reference of the case (class, order, width), computed once and shared"""
    V, tau = reflectors(cls, n)
    return make_reference(V, tau, columns(n, ncols))


def bound_elementwise(n, scale):
    return n * EPS * scale


def bound_projection(n, scale):
    return n * bound_elementwise(n, scale)


def errors(got, r):
    """(elementwise error on the sample columns, projection error over all columns) of a result against make_reference"""
    e1 = float(np.abs(got[:, r["cols"]].astype(LD) - r["ref"]).max()) if r["cols"] else 0.0
    e2 = float(np.abs(got.T.astype(LD) @ r["Y"] - r["ztq"]).max()) if r["ncols"] else 0.0
    return e1, e2


def check(got, r, label, fraction=1.0):
    """asserts both bounds (times `fraction`); prints error / bound as the other stage suites do; returns the ratios"""
    n = r["n"]
    e1, e2 = errors(got, r)
    b1, b2 = bound_elementwise(n, r["scale"]), bound_projection(n, r["scale"])
    r1 = e1 / b1 if b1 > 0 else 0.0
    r2 = e2 / b2 if b2 > 0 else 0.0
    print("%s: elementwise %.3e / %.3e = %.4f, projection %.3e / %.3e = %.4f" % (label, e1, b1, r1, e2, b2, r2))
    assert np.isfinite(got).all(), label
    assert e1 <= fraction * b1, (label, e1, b1)
    assert e2 <= fraction * b2, (label, e2, b2)
    return r1, r2
