"""The table of tests/verify_cases.py on the host (no GPU): the float64 mirror eigenkernel_amd/verifier.py stays within
HALF of every bound on every case (which licenses the full bound for the kernels in tests/test_gpu_verify.py), the
closed-form expectations agree with the long-double reference, and the judge rejects deliberately wrong verifiers.
The shares and the rejecting cases are printed (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import verify_cases as vc

L = np.longdouble


@functools.lru_cache(maxsize=None)
def _table():
    return vc.table()


@functools.lru_cache(maxsize=None)
def _mirror_shares():
    """The mirror through the judge on the whole table, once: ({(kind, key): (worst share, case)}, failures)."""
    worst, bad = {}, []
    for case in _table():
        fails, shares = vc.judge(case, case.run(vc.mirror))
        bad += ["%s: %s" % (case.name, f) for f in fails if " of the bound " not in f]
        for key, s in shares.items():
            if s >= worst.get((case.kind, key), (-1.0, ""))[0]:
                worst[case.kind, key] = (s, case.name)
    return worst, bad


def test_mirror_has_the_references_finite_and_non_finite_slots():
    assert not _mirror_shares()[1], "\n".join(_mirror_shares()[1][:20])


@pytest.mark.parametrize("key", vc.KEYS)
@pytest.mark.parametrize("kind", ["dense", "exact"])
def test_mirror_stays_within_half_of_every_bound(kind, key):
    """Measured on the host (x86-64, NumPy with OpenBLAS), worst share of the bound per quantity --
    dense:  a_norm 0.004, res_ave 0.002, res_max 0.002, orthogonality 0.002, ipr 0.027;
    exact:  a_norm 0.246, res_ave 0.447, res_max 0.234, orthogonality 0.129, ipr 0.125.
    The closed-form bounds count roundings (n_check eps is 2 * 2^-53 relative at n_check = 1), so half of them is one
    rounding: the mirror takes the square roots and divisions that follow its float64 sums in long double and rounds
    once.  With all of them in float64 (sqrt(x) / sqrt(y): three roundings) it used 0.867 of res_ave's bound, 0.697 of
    res_max's and 0.5000000075 of the criterion's -- the shares the kernels use, which are held to the full bound."""
    share, name = _mirror_shares()[0][kind, key]
    print("mirror, %-5s %-13s worst share of the bound %.3f  (%s)" % (kind, key, share, name))
    assert share <= 0.5, (share, name)


def _as_dense(case):
    """The inputs of a closed-form case under the long-double reference of the dense cases."""
    base = vc.DenseBase(case.n, case.problem, case.A, case.B, case.w, case.Z, None)
    return base.case("reference", case.parts, n_check=case.n_check or None, index1=case.index1,
                     index2=case.index2 or None, n_vec=case.n_vec or None)


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [1, 33, 65, 257])
def test_closed_form_expectations_agree_with_the_long_double_reference(n, problem):
    """Two routes to the same numbers: integer arithmetic and one square root and division per slot, against long-double
    products and sums over all n^2 entries.  They differ by long-double rounding alone: n eps_64 relative."""
    rel = n * float(np.finfo(L).eps) * 8
    for case in vc.exact_cases(n, problem):
        ref = _as_dense(case).ref
        for key, want in case.ref.items():
            want, have = np.atleast_1d(want), np.atleast_1d(ref[key])
            assert np.all(np.abs(want - have) <= rel * np.abs(want)), (case.name, key)
    # the formula of the issue for disjoint pairs: every pair contributes two entries eps / sqrt(1 + eps^2)
    pairs = [(0, 5), (6, 1), (2, 7)]
    Z = np.eye(9)
    for j, k in pairs:
        Z[k, j] += vc.ORTH_EPS
    got = vc.numpy_verifier()(np.zeros((9, 9)), None, np.zeros(9), Z, ("orthogonality",), 0, 1, 9, 0)["orthogonality"]
    want = vc.disjoint_pairs_orthogonality(pairs)
    assert abs(L(got) - want) <= 9 * vc.EPS * want


def test_planted_quantities_stand_far_above_their_bounds():
    """A dropped row or column cannot hide under a bound: every judged reference value of a dense case is at least 1e5
    times its bound (zero stands for itself: the criterion of a single column), and the 1000-fold column is the maximum."""
    for problem in (0, 1):
        for case in vc.extreme_cases(problem) + [c for n in (33, 257) for c in vc.dense_cases(n, problem)]:
            for key, ref in case.ref.items():
                ref, bnd = np.atleast_1d(ref).astype(float), np.atleast_1d(case.bound[key])
                assert np.all((ref >= 1e5 * bnd) | (ref == 0)), (case.name, key, ref.min(), bnd.max())
        for j in vc.POSITIONS:
            base = vc.planted(vc.EXTREME_N, problem, j)
            _, rho, _ = base.rho()
            others = np.delete(rho, j).astype(float)
            assert int(np.argmax(rho)) == j and float(rho[j]) >= 500 * others.max(), (j, float(rho[j]), others.max())


def test_the_judge_accepts_the_plain_verifier_and_rejects_every_flawed_one():
    """On a table of four orders (the closed form also at 1030): the plain NumPy verifier passes every case, and each
    flawed variant is rejected by at least one; the first such case is named."""
    table = vc.table(orders=(33, 65, 257, 1))
    v = vc.numpy_verifier()
    for case in table:
        fails, _ = vc.judge(case, case.run(v))
        assert not fails, (case.name, fails)
    for flaw in vc.FLAWS:
        v = vc.numpy_verifier(flaw)
        # either kind alone rejects it -- but order 1030 exists in closed form only, NaN in dense cases only
        excused = {"dense": vc.FLAWS[8:9], "exact": (vc.FLAWS[2], vc.FLAWS[9])}
        for kind in ("exact", "dense"):
            first = next(((case.name, fails[0]) for case in table if case.kind == kind
                          for fails in [vc.judge(case, case.run(v))[0]] if fails), None)
            assert first or flaw in excused[kind], "no %s case rejects: %s" % (kind, flaw)
            if first:
                print("%-46s rejected by %s -- %s" % (flaw, *first))


def test_the_judge_checks_which_slots_are_finite():
    case = vc.nonfinite_case(0, "w nan", 255)
    got = case.run(vc.mirror)
    assert np.isnan(got["res_ave"]) and np.isnan(got["res_max"]) and np.isfinite(got["orthogonality"])
    assert not vc.judge(case, got)[0]
    clean = vc.clean_case(0).run(vc.mirror)
    fails, _ = vc.judge(case, dict(got, res_max=clean["res_max"]))         # a finite maximum beside a NaN average
    assert len(fails) == 1 and fails[0].startswith("res_max")
    fails, _ = vc.judge(vc.clean_case(0), dict(clean, res_max=np.nan))     # and a NaN where a number belongs
    assert len(fails) == 1 and fails[0].startswith("res_max")
    fails, _ = vc.judge(vc.clean_case(0), {k: x for k, x in clean.items() if k != "ipr"})
    assert fails == ["ipr: missing"]
