"""Pins tests/batched_cases.py on the CPU: what tests/test_gpu_batched_hard.py feeds the batched kernels is what its
docstrings say, so that a later edit of a generator cannot quietly soften a case.  No GPU."""
import numpy as np
import pytest

import batched_cases as bc

EPS = 2.220446049250313e-16
ORDERS = (1, 2, 3, 17, 30, 32, 33, 64, 65, 100, 128)
TINY = np.finfo(float).tiny


def _all(n):
    return bc.standard_batch(n) + bc.pencil_batch(n)


@pytest.mark.parametrize("n", ORDERS)
def test_every_case_is_symmetric_and_b_is_spd_where_it_is_meant_to_be(n):
    names = set()
    for c, base in _all(n):
        assert c.name not in names, c.name
        names.add(c.name)
        assert c.A.shape == (n, n) and np.array_equal(c.A, c.A.T), c.name
        assert np.all(np.isfinite(c.A)), c.name
        if c.tridiagonal:
            assert not np.triu(c.A, 2).any(), c.name
        if c.B is None:
            continue
        assert c.B.shape == (n, n) and np.array_equal(c.B, c.B.T), c.name
        if c.spd:
            # smallest eigenvalue well above LAPACK's own error: numerically SPD for any Cholesky
            lam = np.linalg.eigvalsh(base.B)
            assert lam[0] > 64 * n * EPS * lam[-1], (c.name, lam[0], lam[-1])
            np.linalg.cholesky(c.B)
    assert len(names) == len(bc.STANDARD) + len(bc.PENCILS) + 8 * len(bc.SCALED_STANDARD) + 8 + 4 + 4 + 1


def test_the_hilbert_b_is_not_numerically_spd_from_order_14_and_is_left_out_below():
    for n in list(range(14, 34)) + [64, 65, 100, 128]:
        c = bc.make("hilbert_b", n)
        assert not c.spd and c.cond_b > 1e16, n
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(c.B)
    for n in (1, 2, 3):
        c = bc.make("hilbert_b", n)
        assert c.spd and c.cond_b < 1e3 and abs(c.cond_b - np.linalg.cond(c.B)) <= 1e-9 * c.cond_b
    assert list(bc.HILBERT_LEFT_OUT) == list(range(4, 14))
    for n in bc.HILBERT_LEFT_OUT:
        with pytest.raises(ValueError):
            bc.make("hilbert_b", n)


@pytest.mark.parametrize("n", ORDERS)
def test_closed_form_spectra_agree_with_lapack(n):
    """To n eps max|lambda|."""
    import scipy.linalg as sl
    seen = 0
    for c, _ in _all(n):
        if c.exact is None:
            continue
        seen += 1
        assert c.exact.shape == (n,) and np.all(np.diff(c.exact) >= 0), c.name
        w = sl.eigh(c.A, c.B, lower=True, eigvals_only=True) if c.B is not None else np.linalg.eigvalsh(c.A)
        assert np.abs(w - c.exact).max() <= n * EPS * np.abs(c.exact).max(), (c.name, np.abs(w - c.exact).max())
    assert seen == 5 + 2 * 8        # Toeplitz, Clement, their negatives, A = B; Toeplitz and -Clement at eight scales


@pytest.mark.parametrize("n", ORDERS)
def test_power_of_two_scalings_are_exact(n):
    """A 2^k 2^-k gives A back bit for bit, and no entry of a scaled case is denormal or infinite: then the truth of
    the scaled case is exactly 2^(ka - kb) times the truth of the unscaled one.  The largest eigenvalue stays finite,
    except for A 2^600 with B 2^-600, whose eigenvalues (2^1200 times those of the unscaled pencil) overflow."""
    import scipy.linalg as sl
    scaled = [(c, base) for c, base in _all(n) if c.ka or c.kb]
    assert len(scaled) == 8 * len(bc.SCALED_STANDARD) + 8 + 4 + 4 + 1
    for c, base in scaled:
        for M, M0, k in ((c.A, base.A, c.ka), (c.B, base.B, c.kb)):
            if M is None:
                continue
            assert np.array_equal(np.ldexp(M, -k).view(np.uint64), M0.view(np.uint64)), c.name
            nz = np.abs(M[M != 0])
            assert np.all(np.isfinite(M)) and (nz.size == 0 or nz.min() >= TINY), (c.name, nz.min())
        w0 = sl.eigh(base.A, base.B, eigvals_only=True) if base.B is not None else np.linalg.eigvalsh(base.A)
        if c.ka == 600 and c.kb == -600:            # the one case that says so: its eigenvalues are not representable
            assert abs(w0).max() > 2.0 ** -176      # times 2^1200: beyond 2^1024
            continue
        assert np.all(np.isfinite(np.ldexp(w0, c.ka - c.kb))), c.name
        assert np.abs(np.ldexp(w0, c.ka - c.kb)).max() >= TINY or not base.A.any(), c.name


@pytest.mark.parametrize("n", [3, 17, 32, 64, 128])
@pytest.mark.parametrize("name", ["cond_b:1e6", "cond_b:1e10"])
def test_the_stated_condition_of_b_is_what_numpy_reports(name, n):
    c = bc.make(name, n)
    got = np.linalg.cond(c.B)
    assert c.cond_b / 2 <= got <= 2 * c.cond_b, (got, c.cond_b)


def test_tridiagonal_cases_are_what_their_names_say():
    n = 64
    cl = bc.make("clement", n)
    assert not np.diag(cl.A).any() and np.array_equal(cl.exact, np.arange(-63.0, 64.0, 2.0))
    w = bc.make("wilkinson", 21)
    assert np.array_equal(np.diag(w.A), np.abs(np.arange(21) - 10.0)) and np.all(np.diag(w.A, 1) == 1.0)
    for glue in ("1e-8", "1e-14"):
        g = bc.make("glued:" + glue, n)
        e = np.diag(g.A, 1)
        assert np.array_equal(np.flatnonzero(e != 1.0), [20, 41, 62]) and np.all(e[[20, 41, 62]] == float(glue))
    for k in (8, 14):
        dn, up = np.diag(bc.make("graded_down:%d" % k, n).A), np.diag(bc.make("graded_up:%d" % k, n).A)
        assert dn[0] == 1.0 and np.all(np.diff(dn) < 0) and np.array_equal(up, dn[::-1])
        assert 0.5 * 10.0 ** -k < dn[-1] * 10.0 ** (-k / n) < 2 * 10.0 ** -k
    eq, ulp = np.diag(bc.make("ends_equal", n).A), np.diag(bc.make("ends_ulp", n).A)
    assert abs(eq[0]) == abs(eq[-1]) == 1.0
    assert ulp[0] == 1.0 + EPS and abs(ulp[-1]) == 1.0 and np.array_equal(ulp[1:], eq[1:])
    for name in bc.TRIDIAGONALS:
        assert np.array_equal(bc.make("neg:" + name, n).A, -bc.make(name, n).A), name


def test_spectrum_cases_are_what_their_names_say():
    n = 64
    w = np.linalg.eigvalsh(bc.make("two_clusters", n).A)
    assert np.ptp(w[:32]) < 1e-12 and np.ptp(w[32:]) < 1e-12 and abs(w[0] - 1) < 1e-12 and abs(w[-1] - 2) < 1e-12
    assert np.abs(np.linalg.eigvalsh(bc.make("all_equal", n).A) - 3.0).max() < 1e-13
    w = np.linalg.eigvalsh(bc.make("multiplicity_quarter", n).A)
    assert np.abs(w[:16] + 1.0).max() < 1e-13 and w[16] > -1e-13
    w = np.linalg.eigvalsh(bc.make("geometric", n).A)
    assert abs(w[-1] - 1.0) < 1e-13 and abs(w[0]) < 1e-13
    w = np.linalg.eigvalsh(bc.make("pairs", n).A)
    assert np.abs(w[1::2] - w[0::2]).max() < 1e-13 and np.diff(w[0::2]).min() > 1e-3
    blk = bc.make("decoupled_blocks", n).A
    assert not blk[:21, 21:].any() and not blk[21:42, 42:].any() and blk[:21, :21].all()


@pytest.mark.parametrize("n", [30, 64])
def test_unscaled_column_norms_go_wrong_at_2_to_minus_531_and_are_right_at_2_to_minus_498(n):
    """Why the kernel scales A: DSYTD2 with plain sums of squares (bc.dsytd2_unscaled restates the kernel's stage 3 as
    it was).  The eigenvalues of its (d, e), by LAPACK, as a share of the GPU suite's bound 4 n eps max|lambda|: at
    2^-498 (1e-150) the squares are normal numbers; at 2^-531 (1e-160) they are denormal, at 2^-664 zero, and the
    column's tail is dropped without a word.  At 2^531 the sum overflows and (d, e) are not finite."""
    import scipy.linalg as sl
    A = bc.make("band:half", n).A
    w0 = np.linalg.eigvalsh(A)
    bound = 4 * n * EPS * np.abs(w0).max()

    def share(k):
        with np.errstate(all="ignore"):
            d, e = bc.dsytd2_unscaled(np.ldexp(A, k))
        if not (np.all(np.isfinite(d)) and np.all(np.isfinite(e))):
            return np.inf
        # 2^-k is exact on (d, e): LAPACK sees a matrix of norm 1 whatever k
        w = sl.eigvalsh_tridiagonal(np.ldexp(d, -k), np.ldexp(e, -k))
        return np.abs(w - w0).max() / bound

    assert share(0) <= 0.25 and share(-498) <= 0.25 and share(498) <= 0.25
    assert share(-531) > 1e3
    assert share(-664) > 1e3
    assert share(531) == np.inf
