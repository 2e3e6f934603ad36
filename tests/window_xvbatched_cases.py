"""Cases for the variable-order window entries (ek_hip_eigenpairs_window_xvbatched*, ek_hip_sygv_window_xvbatched*): mixed
batches over the orders where something changes, a window per problem, and the references they are judged by.  Plain
functions, no fixtures; tests/test_window_xvbatched_host.py pins them on the CPU against SciPy's windowed drivers,
tests/test_gpu_window_xvbatched.py runs the kernels against them.

Everything but the batches is imported: the windows, the 'V' bounds and the judge of tests/window_batched_cases.py, the
pairs, the hard and planted pencils and the judge of tests/sygv_window_cases.py.  No bound is new.

kind: 0 the standard problem, 1 A x = l B x, 2 A B x = l x, 3 B A x = l x (the entries' problem 0 / 1 and itype 2 / 3)."""
import numpy as np
import scipy.linalg as sl

import window_batched_cases as wc
import sygv_window_cases as sc
from window_batched_cases import windows, value_bounds, judge            # noqa: F401  (re-exported)
from sygv_window_cases import pairs, hard, planted                       # noqa: F401

ORDERS = (1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 130, 192, 255, 256)
SMALL_ORDERS = tuple(n for n in ORDERS if n <= 128)
SHUFFLES = (0, 1)
_cache = {}


class Case:
    """One problem of a batch: the pair, its window by index (1-based, inclusive) and the columns Z has beyond it."""

    def __init__(self, key, A, B, il, iu, extra, name):
        self.key, self.A, self.B, self.n = key, A, B, A.shape[0]
        self.il, self.iu, self.extra, self.name = il, iu, extra, name

    @property
    def zcap(self):
        return self.iu - self.il + 1 + self.extra


def problems(orders=ORDERS, per_order=2):
    """Two seeded pairs of every order, each with a window drawn from windows(n) and a zcap that is exact or up to two
    columns larger; made once, in ascending order."""
    key = ("problems", orders, per_order)
    if key not in _cache:
        rng = np.random.default_rng(340034)
        out = []
        for n in orders:
            A, B = pairs(n)
            table = windows(n)
            for k in range(per_order):
                name, il, iu = table[int(rng.integers(len(table)))]
                out.append(Case(("pair", n, k), A[k], B[k], il, iu, int(rng.integers(3)) if k else 0, name))
        _cache[key] = out
    return _cache[key]


def mixed(shuffle, orders=ORDERS, per_order=2):
    """The problems above in a seeded order: neighbours have different orders and different windows."""
    cases = problems(orders, per_order)
    perm = np.random.default_rng(5150 + shuffle).permutation(len(cases))
    return [cases[i] for i in perm]


def spectrum(case, kind):
    """SciPy's full driver on the case, (w, Z), computed once and never modified."""
    k = ("spectrum", case.key, kind)
    if k not in _cache:
        if kind == 0:
            w, Z = sl.eigh(case.A, lower=True)
            w.setflags(write=False)
            Z.setflags(write=False)
            _cache[k] = (w, Z)
        else:
            _cache[k] = sc.reference(case.key, kind, case.A, case.B)
    return _cache[k]


def bounds(case, kind):
    """(vl, vu, first, m): a half-open interval that holds at least the case's index window and lies clear of the reference
    spectrum, and the 0-based first index and the count it determines."""
    w = spectrum(case, kind)[0]
    vl, vu, span = value_bounds([w], case.il, case.iu)
    return vl, vu, span[0][0], span[0][1]


def judge_kind(case, kind, first, w, Z, what, ev_part=1.0, vec_part=1.0, rule=None, L=None):
    """The judge of the kind: window_batched_cases.judge for 0 and 1, sygv_window_cases.judge for 2 and 3."""
    w_ref, Z_ref = spectrum(case, kind)
    if kind in (0, 1):
        return wc.judge(case.A, case.B if kind else None, None, w_ref, Z_ref, first, w, Z, what, ev_part, vec_part)
    return sc.judge(kind, case.A, case.B, w_ref, first, w, Z, what, ev_part, vec_part, rule, L)


def hard_cases():
    """The hard pencils and the planted clusters at the orders on both sides of a class edge, for the variable call: a
    window that cuts a cluster where the spectrum has one, the whole spectrum elsewhere."""
    if "hard" not in _cache:
        out = []
        for n in (33, 128, 129, 256):
            for name in sc.HARD:
                A, B = hard(name, n)
                out.append((Case(("hard", name, n), A, B, 1, n, 0, name), name))
            for name in wc.CLUSTERED:
                A, B, C = planted(name, n)
                cut = wc.cluster_cut(np.linalg.eigvalsh(C))
                il, iu = cut if cut else (1, n)
                out.append((Case(("planted", name, n), A, B, il, iu, 0, name + ":cut"), None))
        _cache["hard"] = out
    return _cache["hard"]
