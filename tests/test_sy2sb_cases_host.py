"""Host side of the stage tests of the dense -> band reduction (no GPU needed): the two hooks ek_hip_debug_sy2sb_stage and
ek_hip_debug_set_sy2sb_flow are declared in the debug header only, exported, bound and wrapped, and the stage entry refuses
bad arguments before any device work; the matrices of tests/sy2sb_cases.py are what they claim to be (the classes meant
for the rescue really have a tall panel CholeskyQR2 cannot take); its closed-form mirror of the panel geometry agrees
with the transcribed loop of sy2sb_lower and with values worked out by hand, order 2113 has the uneven split of the SYMM
it was chosen for and the handover flow one panel of each kind; the float64 emulation spends at most a quarter of every
bound tests/test_gpu_sy2sb_stages.py asserts, for every class at every edge order up to 321 (it prints its shares as
"sy2sb-emulation <class> n=<order> <orthogonality> <similarity> <spectrum>", pytest -s); and the long-double reference
sees an error of 1e-10 planted in one entry of V."""
import ctypes
import os
import re

import numpy as np
import pytest

import sy2sb_cases as sc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ek_hip_debug_sy2sb_stage", "ek_hip_debug_set_sy2sb_flow")


def test_hooks_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    for hook, nargs in zip(HOOKS, (8, 2)):
        assert hook in hooks and hook not in declared
        assert hook in solver.EXPORTED_SYMBOLS
        assert hasattr(raw, hook)
        fn = getattr(lib, hook)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
        assert hook in open(os.path.join(ROOT, "README.md")).read()
    assert callable(solver.sy2sb_stage) and callable(solver.set_sy2sb_flow)


def test_stage_entry_refuses_bad_arguments_before_any_device_work():
    """-k for the k-th argument; none of these calls initialises a device"""
    lib = solver.load_library()
    n = 130
    A, V, tau = np.zeros((n, n), order="F"), np.zeros((n, n), order="F"), np.zeros(n)
    flag = ctypes.c_int(-7)
    P = solver._P

    def call(n=n, A=P(A), lda=n, V=P(V), ldv=n, tau=P(tau), poison=0, flag=ctypes.byref(flag)):
        return lib.ek_hip_debug_sy2sb_stage(n, A, lda, V, ldv, tau, poison, flag)

    assert call(n=0) == -1 and call(n=-3) == -1
    assert call(A=None) == -2
    assert call(lda=n - 1) == -3
    assert call(V=None) == -4
    assert call(ldv=n - 1) == -5
    assert call(tau=None) == -6
    assert call(flag=None) == -8
    assert flag.value == -7 and not A.any() and not V.any() and not tau.any()       # nothing was written


def test_the_flow_hook_returns_zero_and_needs_no_device():
    lib = solver.load_library()
    try:
        for pm, lm in list(sc.FLOWS.values()) + [(-1, 5), (7, -1)]:
            assert lib.ek_hip_debug_set_sy2sb_flow(pm, lm) == 0
    finally:
        assert lib.ek_hip_debug_set_sy2sb_flow(-1, -1) == 0


def test_the_documented_constants():
    """what the mirrors rest on, read from the sources"""
    src = open(os.path.join(ROOT, "eigenkernel_amd", "csrc", "ek_sy2sb.hip")).read()
    assert re.search(r"constexpr int CH = (\d+);", src).group(1) == str(sc.CH)
    assert re.search(r"constexpr int SMALL_MAX = (\d+);", src).group(1) == str(sc.SMALL_MAX)
    assert re.search(r"maxsplit = P > 0 \? 56 : (\d+);", src).group(1) == str(sc.MAXSPLIT)
    assert "m <= 192" not in src and "m > 192" not in src and "any m <= 256" not in src
    common = open(os.path.join(ROOT, "eigenkernel_amd", "csrc", "ek_common.h")).read()
    assert re.search(r"constexpr int kBandW = (\d+);", common).group(1) == str(sc.SB)
    assert (sc.SB, sc.CH, sc.SMALL_MAX, sc.MAXSPLIT) == (64, 64, 127, 16)


@pytest.mark.parametrize("n", [3, 66, 130, 193, 321])
def test_matrices_are_what_they_claim_to_be(n):
    i = np.arange(n)
    dist = np.abs(i[:, None] - i[None, :])
    for cls in sc.CLASSES:
        A = sc.matrix(cls, n)
        assert A.shape == (n, n) and A.flags.f_contiguous and not A.flags.writeable
        assert sc.matrix(cls, n) is A                                   # made once, shared, left unchanged
        assert np.array_equal(A, A.T) and np.isfinite(A).all()
        sc.matrix.cache_clear()
        assert np.array_equal(sc.matrix(cls, n), A)                     # reproducible
    if n < 130:
        return
    far = dist > sc.SB
    assert (sc.matrix("random", n) != 0).all()
    for cls, up in (("graded", False), ("graded_up", True)):
        G = np.abs(np.diag(sc.matrix(cls, n)))
        head, tail = np.median(G[:n // 8]), np.median(G[-(n // 8):])
        assert (tail > 1e8 * head) if up else (head > 1e8 * tail)
    mags = np.abs(sc.matrix("entrywise", n))
    assert (mags < 1e-6).mean() > 0.1 and (mags > 1e-2).mean() > 0.1
    assert 1e79 < np.abs(sc.matrix("big", n)).max() < 1e82 and 1e-81 < np.abs(sc.matrix("tiny", n)).max() < 1e-78
    for cls, w in (("band65", 65), ("band64", 64)):
        W = sc.matrix(cls, n)
        assert not W[dist > w].any() and (W[dist <= w] != 0).all()
    Zc = sc.matrix("zero_columns", n)
    for c in range(n):
        below = Zc[64 * (c // 64 + 1):, c]
        assert (not below.any()) if c % 3 == 2 else (below != 0).all()
    Pc = sc.matrix("parallel_columns", n)
    assert np.allclose(Pc[64:, 5], Pc[64:, 4], rtol=2e-7, atol=0) and not np.array_equal(Pc[64:, 5], Pc[64:, 4])
    Lr = sc.matrix("lowrank_plus_identity", n)
    assert np.linalg.matrix_rank(Lr - np.eye(n), tol=1e-9) == 5
    N = sc.matrix("near_identity", n)
    assert np.abs(N - np.eye(n)).max() < 1e-9 and (N - np.eye(n)).all()
    U = sc.matrix("outlier", n)
    assert U[n // 2, n // 2] == 1e8 and np.abs(U - np.diag(np.diag(U))).max() < 10
    assert (sc.matrix("ones", n) == 1.0).all()
    k = (n - 66) // 64
    for where, r in zip(sc.FAR_WHERE, (64 + 64 * k - 1, 64 + 64 * k, 64 + 64 * k + 1, n - 1)):
        F = sc.matrix("far_entry_" + where, n)
        assert sc.far_row(where, n) == r and k >= 1
        assert F[r, 0] == 1.0 and F[0, r] == 1.0 and far.sum() - 2 == (F[far] == 0).sum()
        # the last non-zero 64-row chunk of the first panel, as panel_kernel<0> counts it
        assert (r - 64) // 64 + 1 == {"before": k, "at": k + 1, "after": k + 1, "last": (n - 65) // 64 + 1}[where]


@pytest.mark.parametrize("n", [193, 321])
def test_the_classes_meant_for_the_rescue_have_a_tall_panel_choleskyqr2_cannot_take(n):
    """the first panel (n - 64 >= 128 rows: the chain) without full column rank, or -- the bands, whose panels are random
    triangles, with one row more (band65) or one far entry more (far_entry_*) -- of a condition far beyond the 1e7 the chain
    is trusted with"""
    for cls in sc.RESCUED_CLASSES + ("band64", "ones"):
        panel = sc.matrix(cls, n)[64:, :64]
        assert panel.shape[0] > sc.SMALL_MAX
        sv = np.linalg.svd(panel, compute_uv=False)
        if cls in ("band64", "band65") + sc.FAR_CLASSES:
            assert sv[-1] == 0 or sv[0] / sv[-1] > 1e8, (cls, sv[0] / sv[-1])   # (its square is beyond 1 / eps: no Cholesky of the Gram matrix)
            below = np.tril(panel, -1)
            if cls == "band65":
                assert not np.tril(panel, -2).any() and np.diag(panel, -1).all()   # upper Hessenberg: row 64 is in the second chunk
            elif cls == "band64":
                assert not below.any() and np.diag(panel).all()
            else:
                r = sc.far_row(cls.rsplit("_", 1)[1], n) - 64
                assert below[r, 0] == 1.0 and np.count_nonzero(below) == 1 and r > 0
                assert not panel[:, 3].any() and sv[-1] <= 1e-14 * sv[0]      # exactly rank deficient
        else:
            rank = int((sv > 1e-12 * max(sv[0], 1.0)).sum())
            expect = {"zero_columns": 64 - 21, "lowrank_plus_identity": 5, "ones": 1}[cls]
            assert rank == expect, (cls, rank)
    sv = np.linalg.svd(sc.matrix("random", n)[64:, :64], compute_uv=False)
    assert sv[0] / sv[-1] < 1e3                                          # (and the plain class is nowhere near)


def test_mirror_against_the_transcribed_loop():
    orders = sorted(set(sc.EDGE_ORDERS + sc.LARGE_ORDERS + tuple(range(1, 1100, 13))))
    flows = list(sc.FLOWS.values()) + [(129, 0), (0, 129), (200, 130), (130, 200), (64, 64), (5120, 5120)]
    for n in orders:
        for pm, lm in flows:
            got = sc.panels(n, pm, lm)
            ref = [{k: v for k, v in q.items() if k != "waited"} for q in sc.walk(n, pm, lm)]
            assert got == ref, (n, pm, lm)


def test_mirror_values_worked_out_by_hand():
    P = sc.panels
    assert P(1) == [] and P(2) == []
    assert [(q["m"], q["kind"], q["chunks"], q["T"]) for q in P(3)] == [(-61, "lds", 0, 0)]
    assert [(q["m"], q["kind"], q["chunks"], q["T"]) for q in P(65)] == [(1, "lds", 1, 0)]
    assert [(q["m"], q["kind"], q["chunks"], q["T"], q["nsplit"], q["tps"]) for q in P(66)] == [(2, "lds", 1, 1, 1, 1)]
    # the boundary between the in-LDS panel and the chain; the chunk and the block-row counts at m = 128 / 129
    assert [(q["m"], q["kind"], q["chunks"], q["T"]) for q in P(191)] == [(127, "lds", 2, 1), (63, "lds", 1, 1)]
    assert [(q["m"], q["kind"], q["chunks"], q["T"]) for q in P(192)] == [(128, "chain", 2, 1), (64, "lds", 1, 1)]
    assert [(q["m"], q["kind"], q["chunks"], q["T"]) for q in P(193)] == [(129, "chain", 3, 2), (65, "lds", 2, 1)]
    # has_next: a second panel from 2 rows on
    assert len(P(129)) == 1 and len(P(130)) == 2 and P(130)[1]["m"] == 2
    assert [q["lookahead"] for q in P(129, 0, 2)] == [False] and [q["lookahead"] for q in P(130, 0, 2)] == [True, False]
    assert [q["pair"] for q in P(129, 1, 0)] == [0] and [q["pair"] for q in P(130, 1, 0)] == [1, 2]
    assert [q["pair"] for q in P(322, 1, 0)] == [1, 2, 1, 2, 0] and [q["pair"] for q in P(258, 1, 0)] == [1, 2, 1, 2]
    # a pair's one update is the second panel's: look-ahead iff a panel follows the pair
    assert [q["lookahead"] for q in P(258, 1, 2)] == [True, True, False, False]
    assert [q["lookahead"] for q in P(322, 1, 2)] == [True, True, True, True, False]
    assert sc.symm_split(2048) == (16, 16, 1) and sc.symm_split(2049) == (17, 9, 2) and sc.symm_split(4096) == (32, 16, 2)
    assert sc.symm_split(4097) == (33, 11, 3)
    assert [sc.chain_panels(n) for n in (191, 192, 255, 256, 449, 513)] == [0, 1, 1, 2, 5, 6]
    # every stage test so far stayed at one tile per split
    assert all(q["tps"] <= 1 for n in sc.EDGE_ORDERS + (1025, 1345) for q in P(n))


def test_order_2113_has_the_uneven_split_it_was_chosen_for():
    q = sc.panels(2113)[0]
    assert (q["m"], q["T"], q["tps"], q["nsplit"]) == (2049, 17, 2, 9)
    assert q["T"] - q["tps"] * (q["nsplit"] - 1) == 1                   # the last split holds one tile
    assert q["chunks"] == 33 and q["m"] - 64 * (q["chunks"] - 1) == 1   # a last chunk of one row
    assert q["m"] - 128 * (q["T"] - 1) == 1                             # a last block row of one row
    assert sc.panels(2112)[0]["tps"] == 1                               # the smallest such order
    assert 2113 in sc.LARGE_ORDERS and (2113, ("random",)) in sc.CASES


@pytest.mark.parametrize("n", [o for o in sc.EDGE_ORDERS + sc.LARGE_ORDERS if o >= sc.HANDOVER_MIN])
def test_the_handover_flow_has_a_panel_of_each_kind(n):
    w = sc.walk(n, *sc.FLOWS["handover"])
    kinds = [(q["pair"] != 0, q["lookahead"]) for q in w if q["m"] >= 2]
    assert kinds[0] == (True, True) and kinds[-1] == (False, False)     # starts in pairs with look-ahead, ends plain
    assert {True, False} <= {k[0] for k in kinds} and {True, False} <= {k[1] for k in kinds}
    # the main stream waits for the second stream's chain at least once, and stops doing so (waited false -> true)
    waits = [q["waited"] for q in w if q["pair"] != 2]
    assert waits[0] is False and True in waits and waits[-1] is False
    assert "handover" in sc.flows_of(n) and "handover" not in sc.flows_of(sc.HANDOVER_MIN - 1)


def test_cases_cover_what_the_module_promises():
    by_order = {}
    for n, classes in sc.CASES:
        by_order.setdefault(n, []).extend(classes)
    assert tuple(sorted(by_order)) == tuple(sorted(sc.EDGE_ORDERS + sc.LARGE_ORDERS))
    for n in sc.EDGE_ORDERS:
        assert sorted(by_order[n]) == sorted(sc.CLASSES)
    for n in sc.LARGE_ORDERS:
        assert tuple(by_order[n]) == ("random", "graded", "band65", "zero_columns")
    assert len(sc.CLASSES) == len(set(sc.CLASSES)) == 18


EMULATED = tuple(c for c in sc.CASES if c[0] <= 321)


@pytest.mark.parametrize("case", EMULATED, ids=sc.case_id)
def test_emulation_spends_at_most_a_quarter_of_every_bound(case):
    n, classes = case
    for cls in classes:
        A = sc.matrix(cls, n)
        Ab, V, tau = sc.emulate(A)
        assert sc.below_band_is_zero(Ab)
        sc.check_structure(V, tau)
        orth, sim, spec = sc.ratios(A, Ab, V, tau, sc.spectrum(cls, n))
        print("sy2sb-emulation %s n=%d %.4f %.4f %.4f" % (cls, n, orth, sim, spec))
        assert max(orth, sim, spec) <= 0.25, (cls, n, orth, sim, spec)


@pytest.mark.parametrize("n", [130, 321, 449])
def test_the_reference_sees_a_planted_error(n):
    """one entry of V off by 1e-10 (the reflector is then no reflector, and Q1^T A Q1 no band): the similarity bound fails,
    on the whole matrix (130, 321) and on the sample columns (449: the entry is in column 37, a sample column's panel)"""
    A = sc.matrix("random", n)
    Ab, V, tau = sc.emulate(A)
    assert max(sc.ratios(A, Ab, V, tau, sc.spectrum("random", n))) <= 0.25
    V = V.copy()
    V[37 + 64 + 5, 37] += 1e-10
    orth, sim, _ = sc.ratios(A, Ab, V, tau)
    assert sim > 1.0, sim
