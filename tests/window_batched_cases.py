"""Windows for the batched window solver (ek_hip_eigenpairs_window_batched*): the table of windows per order, a window
whose two edges cut a cluster, value bounds for RANGE 'V', and a NumPy judge for the m columns of a window.  Plain
functions, no fixtures; tests/test_window_batched_host.py pins them on the CPU against LAPACK's own windowed drivers,
tests/test_gpu_window_batched.py runs the kernel against them.

The truth for eigenvalues is always the full-spectrum reference, sliced (test_gpu_batched_hard.py::_truth): LAPACK's
DSYEVX returned no eigenvalue for all_equal at order 17 with the window (17, 17).

Bounds (none is new): eigenvalues 4 max(n, 8) eps max|w_ref| over the WHOLE reference spectrum; residual c n eps max|A|
and orthogonality c n eps against np.eye(m), c = 64 standard / 256 generalized; for a stated cond(B) the rule of
test_gpu_batched_hard.py::_judge with LAPACK's full driver, on the whole pencil, as "its own"."""
import numpy as np

EPS = 2.220446049250313e-16
CLUSTERED = ("two_clusters", "multiplicity_quarter", "pairs", "glued:1e-14", "all_equal")


def windows(n):
    """[(name, il, iu)], 1-based and inclusive: the whole spectrum, the first, the last, an interior quarter and the
    middle three; windows that coincide at a small order appear once."""
    mid = (n + 1) // 2
    table = [("whole", 1, n), ("first", 1, 1), ("last", n, n),
             ("quarter", n // 4 + 1, max(n // 4 + 1, n // 2)),
             ("middle3", max(1, mid - 1), min(n, mid + 1))]
    out, seen = [], set()
    for name, il, iu in table:
        if (il, iu) not in seen:
            seen.add((il, iu))
            out.append((name, il, iu))
    return out


def clusters(w_ref, rel=1e-10):
    """Runs of the ascending w_ref whose neighbours lie within rel max|w|: [(first, last)], 0-based, inclusive."""
    w = np.asarray(w_ref)
    lim = rel * max(np.abs(w).max(), 1e-300)
    out, a = [], 0
    for i in range(1, len(w) + 1):
        if i == len(w) or w[i] - w[i - 1] > lim:
            out.append((a, i - 1))
            a = i
    return out


def cluster_cut(w_ref):
    """(il, iu), 1-based: from the second member of the first cluster of two or more to the last but one member of the
    last such cluster, so that both edges of the window cut a cluster; None where the spectrum has no such window."""
    big = [c for c in clusters(w_ref) if c[1] > c[0]]
    if not big:
        return None
    il, iu = big[0][0] + 2, big[-1][1]
    return (il, iu) if il <= iu else None


def gap_limit(w_ref):
    n = len(w_ref)
    return 64 * n * EPS * np.abs(w_ref).max()


def value_bounds(refs, il, iu):
    """Bounds (vl, vu) of a half-open window (vl, vu] that holds at least the indices il .. iu of refs[0] (a list of
    ascending reference spectra of one order): midpoints of gaps of refs[0] wider than gap_limit, moved outwards gap by
    gap until every spectrum of refs keeps half its own gap_limit clear of both bounds; -inf / +inf where no gap is
    left.  Returns (vl, vu, [(first, m) per spectrum]): first 0-based."""
    w0 = np.asarray(refs[0])
    n = len(w0)

    def clear(x):
        return all(np.abs(np.asarray(w) - x).min() >= 0.5 * gap_limit(w) for w in refs)

    vl = -np.inf
    for j in range(il - 1, 0, -1):                  # the gap below index j (0-based j): between w0[j - 1] and w0[j]
        x = 0.5 * (w0[j - 1] + w0[j])
        if w0[j] - w0[j - 1] > gap_limit(w0) and clear(x):
            vl = x
            break
    vu = np.inf
    for j in range(iu - 1, n - 1):
        x = 0.5 * (w0[j] + w0[j + 1])
        if w0[j + 1] - w0[j] > gap_limit(w0) and clear(x):
            vu = x
            break
    span = []
    for w in refs:
        w = np.asarray(w)
        first = int((w <= vl).sum())
        span.append((first, int((w <= vu).sum()) - first))
    return vl, vu, span


def quantities(A, B, w, Z):
    """Scaled residual and B-orthogonality of m columns in units of n eps (test_gpu_fuzz.py's `quantities`)."""
    n, m = Z.shape
    Bm = np.eye(n) if B is None else B
    R = A @ Z - (Bm @ Z) * w
    res = (np.abs(R).max(axis=0) / (np.abs(A).max() + np.abs(w) * np.abs(Bm).max())).max() / (n * EPS)
    return res, np.abs(Z.T @ Bm @ Z - np.eye(m)).max() / (n * EPS)


def judge(A, B, cond_b, w_ref, Z_ref, first, w, Z, what, ev_part=1.0, vec_part=1.0):
    """The m = len(w) pairs (w, Z) against indices first .. first + m - 1 (0-based) of the full reference (w_ref, Z_ref)
    of the pencil (A, B); Z None: values only.  ev_part / vec_part: the part of each bound that is allowed (the host test
    holds LAPACK to a half and a quarter); the rule for a stated cond(B) is relative to LAPACK's own and takes no part.
    Returns (shares, failures) as test_gpu_batched_hard.py::_judge does."""
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
        ref = w_ref[first:first + m]
        if cond_b is not None:
            rel = (np.abs(w - ref) / np.maximum(np.abs(ref), 1.0)).max()
            tol = 4 * n * EPS * cond_b
            shares = [rel / tol, None, None]
            if not rel <= tol:
                fails.append("%s: eigenvalues, relative error %.3e > %.3e" % (what, rel, tol))
            if Z is not None:
                res, orth = quantities(A, B, w, Z)
                res_l, orth_l = quantities(A, B, w_ref, Z_ref)        # the full driver on the whole pencil
                lim_r, lim_o = 4 * max(res_l, 16), 4 * max(orth_l, 16)
                shares[1:] = [res / lim_r, orth / lim_o]
                if not res <= lim_r:
                    fails.append("%s: residual %.1f n eps > %.1f (LAPACK's own %.1f)" % (what, res, lim_r, res_l))
                if not orth <= lim_o:
                    fails.append("%s: orthogonality %.1f n eps > %.1f (LAPACK's own %.1f)" % (what, orth, lim_o, orth_l))
            return shares, fails
        tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max() * ev_part
        err = np.abs(w - ref).max()
        shares = [err / tol if tol > 0 else float(err != 0), None, None]
        if not err <= tol:
            fails.append("%s: eigenvalues, error %.3e > %.3e" % (what, err, tol))
        if Z is not None:
            cc = 256 if B is not None else 64
            BZ = B @ Z if B is not None else Z
            res = np.abs(A @ Z - BZ * w).max()
            orth = np.abs(Z.T @ BZ - np.eye(m)).max()
            tol_r, tol_o = cc * n * EPS * np.abs(A).max() * vec_part, cc * n * EPS * vec_part
            shares[1:] = [res / tol_r if tol_r > 0 else float(res != 0), orth / tol_o]
            if not res <= tol_r:
                fails.append("%s: residual %.3e > %.3e" % (what, res, tol_r))
            if not orth <= tol_o:
                fails.append("%s: orthogonality %.3e > %.3e" % (what, orth, tol_o))
    return shares, fails
