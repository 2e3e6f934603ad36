"""GPU suite of the one-problem verifier: ek_hip_residual_device, ek_hip_orthogonality_device, ek_hip_ipratios_device and
the host form ek_hip_check -- the acceptance gate everything else is judged by.  Cases, references, bounds and the judge
are those of tests/verify_cases.py: closed-form cases that are exact in fp64 with bounds counted in ulp,
and seeded dense cases against a long-double reference within forward-error bounds of 4 max(n, 8) eps;
tests/test_verify_cases_host.py shows on the CPU that this judge rejects subtly wrong verifiers.  On top of the numbers:
what must never be read holds NaN, non-finite values in what is read show in exactly the slots of the reference, the
other entry points, repeatability across the shared workspace, and every argument code.  Each test prints the largest
share of the bound it used (pytest -s shows it)."""
import ctypes

import numpy as np
import pytest

from eigenkernel_amd import descriptor as dsc

import test_gpu_sparse as ts
import verify_cases as vc
from test_gpu_batched import _Dev

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e77
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def P(a):
    return a.ctypes.data_as(_dp)


def _padded(M, ld, fill=np.nan):
    """M in a column-major array of ld rows; the rows below M hold `fill`."""
    out = np.full((ld, M.shape[1]), fill, order="F")
    out[:M.shape[0]] = M
    return out


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _bits(got):
    return {k: np.atleast_1d(np.asarray(got[k], dtype=np.float64)).view(np.uint64).tolist() for k in got}


def device_verifier(lib, lda=None, ldb=None, ldz=None):
    """The three device entries as a verifier of verify_cases: uploads what the parts need (NaN in the rows n .. ld - 1),
    asserts the return value 0 and that every input array comes back bit for bit."""
    def v(A, B, w, Z, parts, n_check, index1, index2, n_vec):
        n, problem = A.shape[0], int(B is not None)
        la, lb, lz = lda or max(n, 1), ldb or max(n, 1), ldz or max(n, 1)
        got = {}
        with _Dev(lib) as dev:
            host = {"Z": _padded(Z, lz)}
            if "residual" in parts:
                host["A"], host["w"] = _padded(A, la), np.ascontiguousarray(w)
            if problem:
                host["B"] = _padded(B, lb)
            d = {k: dev.up(a) for k, a in host.items()}
            dB = d["B"] if problem else None
            if "residual" in parts:
                r = [ctypes.c_double(SENTINEL) for _ in range(3)]
                rc = lib.ek_hip_residual_device(problem, n, n_check, d["A"], la, dB, lb, d["w"], d["Z"], lz,
                                                ctypes.byref(r[0]), ctypes.byref(r[1]), ctypes.byref(r[2]))
                assert rc == 0, rc
                got.update(a_norm=r[0].value, res_ave=r[1].value, res_max=r[2].value)
            if "orthogonality" in parts:
                o = ctypes.c_double(SENTINEL)
                rc = lib.ek_hip_orthogonality_device(problem, n, index1, index2, dB, lb, d["Z"], lz, ctypes.byref(o))
                assert rc == 0, rc
                got["orthogonality"] = o.value
            if "ipr" in parts:
                q = np.full(n_vec + 1, SENTINEL)
                rc = lib.ek_hip_ipratios_device(problem, n, n_vec, dB, lb, d["Z"], lz, P(q))
                assert rc == 0, rc
                assert q[n_vec] == SENTINEL
                got["ipr"] = q[:n_vec].copy()
            for k, a in host.items():
                assert _same_bytes(dev.down(d[k], a), a), "the call changed its input " + k
        return got

    return v


def _judge_all(cases, v, label):
    """Every case through v and the judge; prints the worst share per quantity; returns what v gave, by case name."""
    worst, bad, gots = {}, [], {}
    for case in cases:
        got = gots[case.name] = case.run(v)
        fails, shares = vc.judge(case, got)
        bad += ["%s: %s" % (case.name, f) for f in fails]
        for key, s in shares.items():
            worst[key] = max(worst.get(key, 0.0), s)
    print("%s: share of the bound used -- %s" % (label, ", ".join("%s %.3f" % (k, worst[k]) for k in vc.KEYS if k in worst)))
    assert not bad, "\n".join(bad[:20])
    return gots


# ------------------------------------------------------------------------------------------------ the numbers
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", vc.ORDERS + (vc.BIG,))
def test_closed_form_cases(hip, n, problem):
    """Exact data: a_norm and res_max within 2 ulp, res_ave within n_check eps, the criterion within nc eps, every IPR within
    4 ulp -- every n_check, window and n_vec of the order.  Order 1030 with n_check above 1024 is the second trip of
    scale_cols_kernel's column loop."""
    _judge_all(vc.exact_cases(n, problem), device_verifier(hip.load_library()), "closed form n=%d problem=%d" % (n, problem))


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", vc.ORDERS)
def test_dense_cases_against_long_double(hip, n, problem):
    _judge_all(vc.dense_cases(n, problem), device_verifier(hip.load_library()), "dense n=%d problem=%d" % (n, problem))


@pytest.mark.parametrize("problem", [0, 1])
def test_position_of_the_extreme(hip, problem):
    """The 1000-fold column at 0, 63, 64, 255, 256 and n_check - 1 (res_max is that column's rho: every other column lies
    three orders below, the bound ten), the non-orthogonal pair at the corners and at the seam of the window."""
    _judge_all(vc.extreme_cases(problem), device_verifier(hip.load_library()), "extremes problem=%d" % problem)


# ------------------------------------------------------------------------------------------------ what is never read
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [33, 65, 257])
def test_never_looked_at(hip, n, problem):
    """NaN in the strictly upper triangles of A and B, in the rows n .. ld - 1 (lda = n + 3, ldb = n + 5), in w from n_check
    on and in the columns of Z outside the checked range: with ldz = n the bits of the compact call on full symmetric
    matrices; with ldz = n + 7 and NaN in Z's padding rows the same numbers to the bounds."""
    lib = hip.load_library()
    clean = vc.unread_cases(n, problem, dirty=False)
    dirty = vc.unread_cases(n, problem, dirty=True)
    assert all(np.isnan(c.A).any() or n == 1 for c in dirty) and not any(np.isnan(c.Z).any() for c in clean)
    want = _judge_all(clean, device_verifier(lib), "compact n=%d problem=%d" % (n, problem))
    got = _judge_all(dirty, device_verifier(lib, lda=n + 3, ldb=n + 5), "NaN where nothing reads n=%d problem=%d" % (n, problem))
    for c, d in zip(clean, dirty):
        assert _bits(got[d.name]) == _bits(want[c.name]), d.name
    _judge_all(dirty, device_verifier(lib, lda=n + 3, ldb=n + 5, ldz=n + 7), "and ldz = n + 7, n=%d problem=%d" % (n, problem))


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("kind", vc.NONFINITE_KINDS)
def test_non_finite_values_show_in_the_slots_of_the_reference(hip, kind, problem):
    """A NaN or Inf in w[j], a NaN in Z[i, j], a zero column j of Z (j = 0, 255, 256, n_check - 1), A = 0: the calls return
    0, the slots that are not finite are those of the long-double reference (res_max included), and the slots the change
    cannot reach keep the bits of the clean call."""
    v = device_verifier(hip.load_library())
    clean = vc.clean_case(problem)
    want = clean.run(v)
    assert not vc.judge(clean, want)[0]
    for j in (vc.nonfinite_positions() if kind != "a zero" else (0,)):
        case = vc.nonfinite_case(problem, kind, j)
        got = case.run(v)
        fails, _ = vc.judge(case, got)
        assert not fails, (case.name, fails)
        if kind in ("w nan", "w inf"):
            assert not np.isfinite(got["res_ave"]) and not np.isfinite(got["res_max"])
            same = ("a_norm", "orthogonality", "ipr")
        elif kind == "a zero":
            assert got["a_norm"] == 0.0 and not np.isfinite(got["res_ave"]) and not np.isfinite(got["res_max"])
            same = ("orthogonality", "ipr")
        else:
            assert np.isnan(got["orthogonality"]) and np.isnan(got["ipr"][j])
            assert np.isfinite(got["res_max"]) == (kind == "z zero column")
            others = np.arange(case.n_vec) != j
            assert _same_bytes(got["ipr"][others], want["ipr"][others]), case.name
            same = ("a_norm",)
        if kind == "w nan":
            assert np.isnan(got["res_ave"]) and np.isnan(got["res_max"])
        for key in same:
            assert _bits(got)[key] == _bits(want)[key], (case.name, key)


def test_nan_in_w_through_the_other_entry_points(hip):
    """res_max is NaN through ek_hip_check (what = 0), ek_hip_check_sygvx_device (itype = 1) and ek_hip_check_sparse too."""
    lib = hip.load_library()
    case = vc.nonfinite_case(1, "w nan", 255)
    n = case.n
    A, B, Z, w = (np.asfortranarray(x) for x in (vc._sym_lower(case.A), vc._sym_lower(case.B), case.Z, case.w))
    want = case.run(device_verifier(lib))
    assert np.isnan(want["res_max"]) and np.isnan(want["res_ave"])
    desc = dsc.descinit(n, n, n, n, 0, 0, 0, n)
    out = np.full(n, SENTINEL)
    assert lib.ek_hip_check(0, 1, n, n, 1, n, P(A), desc.ctypes.data_as(_ip), P(B), desc.ctypes.data_as(_ip), P(w), P(Z),
                            desc.ctypes.data_as(_ip), P(out)) == 0
    assert np.isnan(out[1]) and np.isnan(out[2]) and _same_bytes(out[:3], np.array([want[k] for k in vc.KEYS[:3]]))
    with _Dev(lib) as dev:
        out4, ipr = np.full(4, SENTINEL), np.full(n, SENTINEL)
        assert lib.ek_hip_check_sygvx_device(1, n, n, dev.up(A), n, dev.up(B), n, dev.up(w), dev.up(Z), n, P(out4), P(ipr)) == 0
    assert np.isnan(out4[1]) and np.isnan(out4[2]) and np.isfinite(out4[3]) and np.isfinite(ipr).all()
    assert _same_bytes(out4, np.array([want[k] for k in vc.KEYS[:4]])) and _same_bytes(ipr, want["ipr"])
    a, b = ts._args(ts.triplets_of(A, 1, keep_zeros=True)), ts._args(ts.triplets_of(B, 2, keep_zeros=True))
    outs = np.full(4, SENTINEL)
    assert lib.ek_hip_check_sparse(1, n, *a[:3], *b[:3], P(w), P(Z), n, n, 1, 0, 0, P(outs), None) == 0
    assert np.isnan(outs[1]) and np.isnan(outs[2]) and np.isfinite(outs[0]) and outs[3] == SENTINEL


@pytest.mark.parametrize("problem", [0, 1])
def test_host_form_with_padded_descriptors(hip, problem):
    """ek_hip_check on host arrays with lld = n + 4 (NaN in the padding rows) gives the bits of the device entries on
    compact arrays, for the three values of what."""
    lib = hip.load_library()
    n = 65
    case = vc.planted(n, problem, 40).case("host form", n_check=33, index1=2, index2=64, n_vec=65)
    want = case.run(device_verifier(lib))
    assert not vc.judge(case, want)[0]
    ld = n + 4
    desc = dsc.descinit(n, n, n, n, 0, 0, 0, ld)
    D = desc.ctypes.data_as(_ip)
    A, Z = _padded(case.A, ld), _padded(case.Z, ld)
    B = _padded(case.B, ld) if problem else None
    pB, dB = (P(B), D) if problem else (None, None)
    out = np.full(n + 1, SENTINEL)
    assert lib.ek_hip_check(0, problem, n, 33, 0, 0, P(A), D, pB, dB, P(case.w.copy()), P(Z), D, P(out)) == 0
    assert _same_bytes(out[:3], np.array([want[k] for k in vc.KEYS[:3]])) and out[3] == SENTINEL
    out[:] = SENTINEL
    assert lib.ek_hip_check(1, problem, n, 0, 2, 64, None, None, pB, dB, None, P(Z), D, P(out)) == 0
    assert _same_bytes(out[:1], np.array([want["orthogonality"]])) and out[1] == SENTINEL
    out[:] = SENTINEL
    assert lib.ek_hip_check(2, problem, n, 65, 0, 0, None, None, pB, dB, None, P(Z), D, P(out)) == 0
    assert _same_bytes(out[:n], want["ipr"]) and out[n] == SENTINEL


def test_repeatable_across_the_shared_workspace(hip):
    """The work array is reused without being cleared and the reductions have a fixed order: an order-65 call gives equal
    bits twice in a row, and before and after calls of order 513 and 1030."""
    v = device_verifier(hip.load_library())
    small = vc.planted(65, 1, 32).case("all parts", n_check=64, index1=2, index2=65, n_vec=65)
    first = _bits(small.run(v))
    assert _bits(small.run(v)) == first
    vc.planted(513, 1, 256).case("all parts").run(v)
    assert _bits(small.run(v)) == first
    for case in (vc.exact_residual_case(vc.BIG, 1, vc.BIG), vc.exact_orth_case(vc.BIG, 1, 1, vc.BIG),
                 vc.exact_ipr_case(vc.BIG, 1, vc.BIG)):
        case.run(v)
    assert _bits(small.run(v)) == first
    assert _bits(small.run(v)) == first


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_codes(hip):
    """Every error code of the three device entries and of ek_hip_check, the first offender deciding; n = 0 and a count of
    0 return 0 and write nothing."""
    lib = hip.load_library()
    n = 4
    r = [ctypes.c_double(SENTINEL) for _ in range(3)]
    R = [ctypes.byref(x) for x in r]
    q = np.full(n, SENTINEL)
    with _Dev(lib) as dev:
        M, w = dev.up(np.eye(n, order="F")), dev.up(np.ones(n))

        def res(problem=1, n_=n, n_check=n, dA=M, lda=n, dB=M, ldb=n, dw=w, dZ=M, ldz=n):
            return lib.ek_hip_residual_device(problem, n_, n_check, dA, lda, dB, ldb, dw, dZ, ldz, *R)

        def orth(problem=1, n_=n, index1=1, index2=n, dB=M, ldb=n, dZ=M, ldz=n):
            return lib.ek_hip_orthogonality_device(problem, n_, index1, index2, dB, ldb, dZ, ldz, R[0])

        def ipr(problem=1, n_=n, n_vec=n, dB=M, ldb=n, dZ=M, ldz=n):
            return lib.ek_hip_ipratios_device(problem, n_, n_vec, dB, ldb, dZ, ldz, P(q))

        assert [res(problem=2), res(problem=-1), res(n_=-1), res(n_check=-1), res(n_check=n + 1), res(dA=None),
                res(lda=n - 1), res(dB=None), res(ldb=n - 1), res(dw=None), res(dZ=None), res(ldz=n - 1)] == \
            [-1, -1, -2, -3, -3, -4, -5, -6, -7, -8, -9, -10]
        assert [res(problem=2, n_=-1), res(n_=-1, n_check=-1), res(n_check=n + 1, dA=None), res(dA=None, lda=0),
                res(dA=None, dB=None), res(lda=0, dB=None), res(dB=None, ldb=0), res(ldb=0, dw=None),
                res(dw=None, dZ=None), res(dZ=None, ldz=0)] == [-1, -2, -3, -4, -4, -5, -6, -7, -8, -9]
        assert all(x.value == SENTINEL for x in r)
        assert res(problem=0, dB=None, ldb=0) == 0 and r[0].value == 2.0         # B and ldb are not looked at for problem 0
        for x in r:
            x.value = SENTINEL
        assert res(n_=0, n_check=0, dA=None, lda=1, dB=None, ldb=1, dw=None, dZ=None, ldz=1) == 0
        assert res(n_=0, n_check=0, lda=0) == -5 and res(n_check=0, dw=None, dZ=None) == 0
        assert all(x.value == SENTINEL for x in r)

        assert [orth(problem=2), orth(n_=-1), orth(n_=0), orth(index1=0), orth(index1=n + 1), orth(index2=0),
                orth(index1=3, index2=2), orth(index2=n + 1), orth(dB=None), orth(ldb=n - 1), orth(dZ=None),
                orth(ldz=n - 1)] == [-1, -2, -3, -3, -3, -4, -4, -4, -5, -6, -7, -8]
        assert [orth(problem=2, n_=-1), orth(n_=-1, index1=0), orth(index1=0, index2=0), orth(index2=0, dB=None),
                orth(dB=None, ldb=0), orth(ldb=0, dZ=None), orth(dZ=None, ldz=0)] == [-1, -2, -3, -4, -5, -6, -7]
        assert r[0].value == SENTINEL
        assert orth(problem=0, dB=None, ldb=0) == 0 and r[0].value == 0.0
        r[0].value = SENTINEL

        assert [ipr(problem=2), ipr(n_=-1), ipr(n_vec=-1), ipr(n_vec=n + 1), ipr(dB=None), ipr(ldb=n - 1), ipr(dZ=None),
                ipr(ldz=n - 1)] == [-1, -2, -3, -3, -4, -5, -6, -7]
        assert [ipr(problem=2, n_=-1), ipr(n_=-1, n_vec=-1), ipr(n_vec=-1, dB=None), ipr(dB=None, ldb=0),
                ipr(ldb=0, dZ=None), ipr(dZ=None, ldz=0)] == [-1, -2, -3, -4, -5, -6]
        assert ipr(n_vec=0, dZ=None) == 0 and ipr(n_=0, n_vec=0, dB=None, ldb=1, dZ=None, ldz=1) == 0
        assert np.all(q == SENTINEL)
        assert ipr(problem=0, dB=None, ldb=0) == 0 and np.array_equal(q, np.ones(n))

    E, one = np.eye(n, order="F"), np.ones(n)
    out = np.full(n, SENTINEL)

    def desc(**kw):
        d = dsc.descinit(n, n, n, n, 0, 0, 0, n)
        for k, x in kw.items():
            d[int(k[1:])] = x
        return d

    def chk(what=0, problem=1, n_=n, n_cols=n, A=E, dA=desc(), B=E, dB=desc(), Z=E, dZ=desc(), out_=out):
        I = lambda d: d.ctypes.data_as(_ip) if d is not None else None
        p = lambda a: P(a) if a is not None else None
        return lib.ek_hip_check(what, problem, n_, n_cols, 1, n, p(A), I(dA), p(B), I(dB), P(one), p(Z), I(dZ), p(out_))

    assert [chk(what=-1), chk(what=3), chk(problem=2), chk(n_=-1), chk(n_cols=-1), chk(n_cols=n + 1), chk(A=None),
            chk(dA=None), chk(B=None), chk(dB=None), chk(Z=None), chk(dZ=None), chk(out_=None)] == \
        [-1, -1, -2, -3, -4, -4, -7, -8, -9, -10, -12, -13, -14]
    assert [chk(dA=desc(_0=2)), chk(dA=desc(_2=n + 1)), chk(dA=desc(_3=n - 1)), chk(dA=desc(_4=0)), chk(dA=desc(_5=2)),
            chk(dA=desc(_6=1)), chk(dA=desc(_7=1)), chk(dA=desc(_8=n - 1))] == [-801, -803, -804, -805, -805, -807, -808, -809]
    assert [chk(dB=desc(_8=n - 1)), chk(dZ=desc(_2=n - 1)), chk(dZ=desc(_8=n - 1))] == [-1009, -1303, -1309]
    assert [chk(what=3, problem=2), chk(n_cols=-1, A=None), chk(A=None, B=None), chk(dA=None, B=None),
            chk(B=None, Z=None), chk(dZ=desc(_8=0), out_=None)] == [-1, -4, -7, -8, -9, -1309]
    assert [chk(what=1, A=None, dA=None), chk(what=2, problem=0, A=None, dA=None, B=None, dB=None)] == [0, 0]
    out[:] = SENTINEL
    d0 = dsc.descinit(0, 0, 1, 1, 0, 0, 0, 1)
    assert chk(n_=0, n_cols=0, dA=d0, dB=d0, dZ=d0) == 0 and np.all(out == SENTINEL)
