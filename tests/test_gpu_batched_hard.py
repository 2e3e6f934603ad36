"""Hard inputs for the batched kernels (ek_hip_eigenpairs_batched_device, ek_hip_eigenpairs_vbatched_device): the table
of tests/batched_cases.py -- clustered and multiple spectra, tridiagonal inputs (Toeplitz, Clement, Wilkinson, glued
Wilkinson, graded both ways, ties of the flip decision, their negatives), graded / banded / arrowhead / low-rank / sparse
/ definite matrices, pencils with cond(B) up to 1e10, A = B, a Hilbert B, and all of it times exact powers of two up to
2^+-1000.  tests/test_gpu_batched.py and tests/test_gpu_vbatched.py check the contract on random matrices; this file
checks the numerics where kernels go wrong.  Every case of one order and problem kind shares one launch.

Nothing here is a new bound:
  eigenvalues      |w - w_ref| <= 4 max(n, 8) eps max|w_ref|, w ascending            (test_gpu_batched.py::_check_problem)
  with vectors     residual <= c n eps max|A|, |Z^T B Z - I| <= c n eps, c = 64 / 256  (the same)
  a stated cond(B) relative error <= 4 n eps cond(B); scaled residual and orthogonality <= 4 max(LAPACK's own on the
                   same pencil, 16) in units of n eps    (test_gpu_fuzz.py::test_generalized_problem_with_an_ill_...)
w_ref is the closed form where batched_cases has one, else LAPACK (scipy.linalg.eigh(A, B, lower=True)) on the
*unscaled* case times the exact 2^k; residuals of scaled cases are evaluated on the descaled quantities.

The Hilbert B runs at orders <= 3, under the rule for a stated cond(B) as it stands, and from order 14, where the
expected outcome is info > 0; batched_cases.HILBERT_LEFT_OUT says why the orders between are not in the table.

No silent failure: every problem ends with info == 0 and all bounds met, or with an info != 0 that is the code
ek_hip_solve_device returns for the same pair (a B that is not numerically SPD), or 100000 + k where L^-1 A L^-T
overflows (A 2^600 with B 2^-600 only).  Every A 2^k and B 2^+-200 case must end with info == 0.

LAPACK's own share of these bounds, against mpmath at 40 digits (a scratch run over every unscaled case of the table at
every order of ORDERS, 370 problems; mpmath is not needed here).  Largest share per family of 4 max(n, 8) eps max|lambda|
-- for a stated cond(B), of 4 n eps cond(B):
  spectrum 0.089 (geometric, n = 3), tridiagonal 0.167 and tridiagonal negated 0.167 (ends_ulp, n = 17),
  dense structure 0.068 (arrowhead, n = 3), pencil 0.118 (A = B at n = 17, where the closed form is used instead),
  cond(B) = 1e6: 0.0026, cond(B) = 1e10: 0.0032, Hilbert at order 3: 0.014
All below a quarter of the bound, so no case had to go.  The closed forms themselves (Toeplitz, Clement, as rounded to
doubles) are within 0.010 of the bound of the 40-digit eigenvalues, and A = B has the eigenvalue 1 n times."""
import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
from test_gpu_vbatched import _batched_device, _same_as_alone, _solve_device, _vbatched

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (3, 17, 30, 32, 33, 64, 65, 100, 128)

_truth_cache = {}


def _truth(base):
    """(w, Z) of the unscaled case by LAPACK, (None, None) where B is not numerically SPD; the closed form replaces w."""
    key = (base.name, base.A.shape[0])
    if key not in _truth_cache:
        try:
            w, Z = sl.eigh(base.A, base.B, lower=True) if base.B is not None else sl.eigh(base.A, lower=True)
        except np.linalg.LinAlgError:
            w, Z = None, None
        if base.exact is not None:
            w = base.exact
        _truth_cache[key] = (w, Z)
    return _truth_cache[key]


def _ill_quantities(A, B, w, Z):
    """Scaled residual and B-orthogonality in units of n eps (test_gpu_fuzz.py's `quantities`)."""
    n = A.shape[0]
    R = A @ Z - (B @ Z) * w
    res = (np.abs(R).max(axis=0) / (np.abs(A).max() + np.abs(w) * np.abs(B).max())).max() / (n * EPS)
    return res, np.abs(Z.T @ B @ Z - np.eye(n)).max() / (n * EPS)


def _judge(lib, c, base, info, w, Z, what):
    """One problem's outcome against the rules of the module docstring.  Returns (shares, failures): the share of each
    bound used (eigenvalues, residual, orthogonality; None where not evaluated) and a list of what went wrong."""
    n = c.A.shape[0]
    k = c.ka - c.kb
    overflow_case = c.ka == 600 and c.kb == -600
    if info != 0:
        if c.spd and not overflow_case:
            return None, ["%s: info = %d where 0 is required (the input has a solution)" % (what, info)]
        ref = _solve_device(lib, c.A, c.B)
        ok = info == ref or (overflow_case and 100000 < info <= 100000 + n + 1)
        return None, [] if ok else ["%s: info = %d, ek_hip_solve_device says %d" % (what, info, ref)]
    with np.errstate(all="ignore"):
        fails = []
        if not np.all(np.isfinite(w)):
            return None, ["%s: info = 0 with a non-finite eigenvalue" % what]
        if Z is not None and not np.all(np.isfinite(Z)):
            return None, ["%s: info = 0 with a non-finite vector entry" % what]
        if not np.all(np.diff(w) >= 0):
            fails.append("%s: w not ascending" % what)
        w_ref, Z_ref = _truth(base)
        if w_ref is None:                           # B not numerically SPD and yet factorised: the big path must agree
            ref = _solve_device(lib, c.A, c.B)
            return None, fails + (["%s: info = 0, ek_hip_solve_device says %d" % (what, ref)] if ref != 0 else [])
        w0 = np.ldexp(w, -k)                        # descaled: exact (a denormal w lost its bits before)
        A0, B0 = base.A, base.B
        Z0 = None if Z is None else np.ldexp(Z, c.kb // 2)      # Z^T B Z = I: Z carries 2^(-kb / 2)
        if c.cond_b is not None:                    # the rule for a stated cond(B)
            rel = (np.abs(w0 - w_ref) / np.maximum(np.abs(w_ref), 1.0)).max()
            tol = 4 * n * EPS * c.cond_b
            shares = [rel / tol, None, None]
            if not rel <= tol:
                fails.append("%s: eigenvalues, relative error %.3e > %.3e" % (what, rel, tol))
            if Z0 is not None:
                res, orth = _ill_quantities(A0, B0, w0, Z0)
                res_l, orth_l = _ill_quantities(A0, B0, w_ref, Z_ref)      # no such case has a closed form: LAPACK's w
                lim_r, lim_o = 4 * max(res_l, 16), 4 * max(orth_l, 16)
                shares[1:] = [res / lim_r, orth / lim_o]
                if not res <= lim_r:
                    fails.append("%s: residual %.1f n eps > %.1f (LAPACK's own %.1f)" % (what, res, lim_r, res_l))
                if not orth <= lim_o:
                    fails.append("%s: orthogonality %.1f n eps > %.1f (LAPACK's own %.1f)" % (what, orth, lim_o, orth_l))
            return shares, fails
        tol = 4 * max(n, 8) * EPS * np.abs(w_ref).max()
        err = np.abs(w0 - w_ref).max()
        shares = [err / tol if tol > 0 else float(err != 0), None, None]
        if not err <= tol:
            fails.append("%s: eigenvalues, error %.3e > %.3e (%.3g of the bound)" % (what, err, tol, err / max(tol, 1e-300)))
        if Z0 is not None:
            cc = 256 if B0 is not None else 64
            BZ = B0 @ Z0 if B0 is not None else Z0
            res = np.abs(A0 @ Z0 - BZ * w0).max()
            orth = np.abs(Z0.T @ BZ - np.eye(n)).max()
            tol_r = cc * n * EPS * np.abs(A0).max()
            shares[1:] = [res / tol_r if tol_r > 0 else float(res != 0), orth / (cc * n * EPS)]
            if not res <= tol_r:
                fails.append("%s: residual %.3e > %.3e" % (what, res, tol_r))
            if not orth <= cc * n * EPS:
                fails.append("%s: orthogonality %.3e > %.3e" % (what, orth, cc * n * EPS))
        return shares, fails


class _Shares:
    """The largest share of each bound per family."""

    def __init__(self):
        self.worst = {}

    def add(self, fam, shares):
        if shares is None:
            return
        cur = self.worst.setdefault(fam, [0.0, 0.0, 0.0])
        for i, s in enumerate(shares):
            if s is not None:
                cur[i] = max(cur[i], float(s))

    def show(self, head):
        for fam in sorted(self.worst):
            print("%s | %-28s share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
                  % ((head, fam) + tuple(self.worst[fam])))


def _tridiagonal_kept(c, A_after, what):
    """H = I throughout: the diagonal and the subdiagonal left in dA are the input's bits."""
    fails = []
    if not np.array_equal(np.diag(A_after).view(np.uint64), np.diag(c.A).view(np.uint64)):
        fails.append("%s: the diagonal left in dA is not the input's" % what)
    if not np.array_equal(np.diag(A_after, -1).view(np.uint64), np.diag(c.A, -1).view(np.uint64)):
        fails.append("%s: the subdiagonal left in dA is not the input's" % what)
    return fails


@pytest.mark.parametrize("jobz", [0, 1])
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", ORDERS)
def test_hard_cases_in_one_batch(hip, n, problem, jobz):
    """Every case of batched_cases (standard: 37 and 40 scaled ones; pencils: 5 and 17 scaled ones) at one order in one
    launch, each held to the rules of the module docstring; tridiagonal inputs leave their (d, e) in dA bit for bit.
    All failures of the batch are reported together."""
    lib = hip.load_library()
    cases = bc.pencil_batch(n) if problem else bc.standard_batch(n)
    A = np.stack([c.A for c, _ in cases])
    B = np.stack([c.B for c, _ in cases]) if problem else None
    o = _batched_device(lib, A, B, jobz)
    assert o.rc == 0, o.rc
    shares, fails = _Shares(), []
    for b, (c, base) in enumerate(cases):
        what = "n=%d problem=%d jobz=%d %s" % (n, problem, jobz, c.name)
        s, f = _judge(lib, c, base, int(o.info[b]), o.w[b], o.Z[b] if jobz else None, what)
        shares.add(c.family, s)
        fails += f
        if not c.spd and o.info[b] <= 0:
            fails.append("%s: info = %d where a pivot of B's Cholesky factorisation should fail" % (what, o.info[b]))
        if c.tridiagonal and o.info[b] == 0:
            fails += _tridiagonal_kept(c, o.A[b], what)
    shares.show("n=%d problem=%d jobz=%d" % (n, problem, jobz))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails)


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", ORDERS)
def test_scale_covariance_to_the_bit(hip, n, problem):
    """Power-of-two scaling is exact and every stage is homogeneous: for well-conditioned cases and k = +-531, +-664,
    w of A 2^k is 2^k times w of A bit for bit, Z is the same bits, and the lower triangle left in dA holds the same
    reflector tails with d and e times 2^k.  Values only gives the same w."""
    lib = hip.load_library()
    names = bc.COVARIANT_PENCILS if problem else bc.COVARIANT_STANDARD
    group = 1 + len(bc.COVARIANT_SCALES)
    cases = []
    for name in names:
        base = bc.make(name, n)
        cases += [base] + [bc.scaled(base, k) for k in bc.COVARIANT_SCALES]
    A = np.stack([c.A for c in cases])
    B = np.stack([c.B for c in cases]) if problem else None
    o = _batched_device(lib, A, B, 1)
    o0 = _batched_device(lib, A, B, 0)
    assert o.rc == 0 and not o.info.any(), (o.rc, o.info)
    assert o0.rc == 0 and not o0.info.any(), (o0.rc, o0.info)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)  # noqa: E731
    band = np.tri(n, n, 0, dtype=bool) & ~np.tri(n, n, -2, dtype=bool)      # diagonal and subdiagonal: d and e
    tails = np.tri(n, n, -2, dtype=bool)
    fails = []
    for g in range(len(names)):
        b0 = g * group
        for j, k in enumerate(bc.COVARIANT_SCALES):
            b = b0 + 1 + j
            what = "n=%d problem=%d %s" % (n, problem, cases[b].name)
            if not np.array_equal(bits(o.w[b]), bits(np.ldexp(o.w[b0], k))):
                fails.append("%s: w is not 2^k times w of the unscaled case" % what)
            if not np.array_equal(bits(o0.w[b]), bits(o.w[b])):
                fails.append("%s: values only gives another w" % what)
            if not np.array_equal(bits(o.Z[b]), bits(o.Z[b0])):
                fails.append("%s: Z differs" % what)
            if not np.array_equal(bits(o.A[b][tails]), bits(o.A[b0][tails])):
                fails.append("%s: reflector tails in dA differ" % what)
            if not np.array_equal(bits(o.A[b][band]), bits(np.ldexp(o.A[b0][band], k))):
                fails.append("%s: d, e in dA are not 2^k times the unscaled case's" % what)
            if problem and not np.array_equal(bits(np.tril(o.B[b])), bits(np.tril(o.B[b0]))):
                fails.append("%s: L in dB differs" % what)
    assert not fails, "\n".join(fails)


def _sweep(problem, batch=512):
    """512 seeded draws: order uniform in 1 .. 128; half of the draws from the cases that also run scaled, with a scale
    drawn from their list (0 included), the other half from the whole table; pencils also draw B 2^+-200.  A Hilbert B
    drawn at an order the table leaves out moves up by 10."""
    rng = bc.rng("sweep%d" % problem)
    names = bc.PENCILS if problem else bc.STANDARD
    table = bc.SCALED_PENCILS if problem else bc.SCALED_STANDARD
    out = []
    for _ in range(batch):
        n = int(rng.integers(1, 129))
        if rng.random() < 0.5:
            name = list(table)[int(rng.integers(len(table)))]
            ks = (0,) + tuple(table[name])
            ka, kb = int(ks[int(rng.integers(len(ks)))]), 0
            if problem and ka == 0 and name in bc.B_SCALED_PENCILS:
                kb = int((0, 200, -200)[int(rng.integers(3))])
        else:
            name, ka, kb = names[int(rng.integers(len(names)))], 0, 0
            if name == "hilbert_b" and n in bc.HILBERT_LEFT_OUT:
                n += 10                             # 14 .. 23: not numerically SPD (no draw is spent on it)
        base = bc.make(name, n)
        out.append((bc.scaled(base, ka, kb) if ka or kb else base, base))
    return out


@pytest.mark.parametrize("problem", [0, 1])
def test_seeded_sweep_through_the_variable_call(hip, problem):
    """One ek_hip_eigenpairs_vbatched_device call of 512 problems drawn from the table (order, case, scale): every
    problem is held to the rules of the module docstring and is bit-identical (w, Z, info, the lower triangles left in
    dA and dB) to the uniform call on that pair alone."""
    lib = hip.load_library()
    cases = _sweep(problem)
    o = _vbatched(lib, [(c.A, c.B) for c, _ in cases], problem, 1)
    assert o.rc == 0, o.rc
    shares, fails = _Shares(), []
    orders, scaled = set(), 0
    for b, (c, base) in enumerate(cases):
        n = c.A.shape[0]
        orders.add(n)
        scaled += bool(c.ka or c.kb)
        what = "sweep problem=%d #%d n=%d %s" % (problem, b, n, c.name)
        s, f = _judge(lib, c, base, int(o.info[b]), o.w[b], o.Z[b], what)
        shares.add(c.family, s)
        fails += f
        if c.tridiagonal and o.info[b] == 0:
            fails += _tridiagonal_kept(c, o.A[b], what)
        try:
            _same_as_alone(lib, ("sweep", problem, b), (c.A, c.B), o, b, problem, 1, what)
        except AssertionError as e:
            fails.append("%s: not the uniform call's bits: %s" % (what, str(e).splitlines()[0]))
    assert len(orders) >= 100 and scaled >= 128, (len(orders), scaled)
    shares.show("sweep problem=%d" % problem)
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:60])
