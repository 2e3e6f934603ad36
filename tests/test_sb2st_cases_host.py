"""Host side of the stage tests of the bulge chasing and of Q2's application (no GPU needed): the stage entry
ek_hip_debug_sb2st_stage is declared in the debug header only, exported, bound, wrapped and refuses bad arguments before
any device work; the bands of tests/sb2st_cases.py are what they claim to be; its mirrors of the geometry give the values
worked out by hand at the edge orders; its float64 emulation of the column-wise scheme spends at most a quarter of every
bound tests/test_gpu_sb2st_stages.py asserts, for every class at every edge order; without the drop rule the
dead_first_column bands break the orthogonality bound (so these inputs can fail); and the two shapes of the wrapped
ticket counter have more passes than the application has workgroups."""
import ctypes
import os
import re

import numpy as np
import pytest

import sb2st_cases as sc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK = "ek_hip_debug_sb2st_stage"


def test_hook_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ek_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ek_hip_debug.h")).read()
    declared = set(re.findall(r"\b(ek_hip_\w+)\s*\(", hdr))
    hooks = set(re.findall(r"\b(ek_hip_\w+)\s*\(", dbg))
    raw = ctypes.CDLL(solver.LIB_PATH)
    lib = solver.load_library()
    assert HOOK in hooks and HOOK not in declared
    assert HOOK in solver.EXPORTED_SYMBOLS
    assert hasattr(raw, HOOK)
    fn = getattr(lib, HOOK)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    assert callable(solver.sb2st_stage)
    assert HOOK in open(os.path.join(ROOT, "README.md")).read()


def test_entry_refuses_bad_arguments_before_any_device_work():
    """-k for the k-th argument; none of these calls initialises a device"""
    lib = solver.load_library()
    n, nc = 130, 5
    kmax = sc.kmax_of(n)
    A = np.zeros((n, n), order="F")
    d, e = np.zeros(n), np.zeros(n)
    V2 = np.zeros((n, n), order="F")
    tau2 = np.zeros((kmax + 1, n - 2), order="F")
    Z = np.zeros((n, nc), order="F")
    ran, flag = ctypes.c_int(-7), ctypes.c_int(-7)
    P = solver._P

    def call(n=n, A=P(A), lda=n, form=0, mode=0, d=P(d), e=P(e), V2=P(V2), ldv2=n, tau2=P(tau2), ldtau=kmax + 1, Z=P(Z),
             ldz=n, ncols=nc):
        return lib.ek_hip_debug_sb2st_stage(n, A, lda, form, mode, d, e, V2, ldv2, tau2, ldtau, Z, ldz, ncols,
                                            ctypes.byref(ran), ctypes.byref(flag))

    assert call(n=0) == -1 and call(n=-3) == -1
    assert call(A=None) == -2
    assert call(lda=n - 1) == -3
    assert call(form=2) == -4 and call(form=-1) == -4
    assert call(mode=3) == -5 and call(mode=-1) == -5
    assert call(d=None) == -6
    assert call(e=None) == -7
    assert call(ldv2=n - 1) == -9
    assert call(ldtau=kmax) == -11
    assert call(Z=None) == -12
    assert call(ldz=n - 1) == -13
    assert call(ncols=-1) == -14
    assert ran.value == -7 and flag.value == -7           # nothing was written


@pytest.mark.parametrize("n", [1, 2, 3, 66, 130, 321])
def test_bands_are_what_they_claim_to_be(n):
    i = np.arange(n)
    dist = np.abs(i[:, None] - i[None, :])
    for cls in sc.CLASSES:
        B = sc.band(cls, n)
        assert B.shape == (n, n) and B.flags.f_contiguous and not B.flags.writeable
        assert sc.band(cls, n) is B                                   # made once, shared, left unchanged
        assert np.array_equal(B, B.T) and np.isfinite(B).all()
        assert not B[dist > sc.SB].any()                              # nothing outside the band
    if n < 66:
        return
    rnd = sc.band("random", n)
    assert (rnd[dist <= sc.SB] != 0).all()
    for cls, up in (("graded", False), ("graded_up", True)):
        G = np.abs(np.diag(sc.band(cls, n)))
        head, tail = np.median(G[:n // 8]), np.median(G[-(n // 8):])
        assert (tail > 1e10 * head) if up else (head > 1e10 * tail)
    mags = np.abs(sc.band("entrywise", n)[dist <= sc.SB])
    assert (mags < 1e-9).mean() > 0.1 and (mags > 1e-3).mean() > 0.1
    assert 1e79 < np.abs(sc.band("big", n)).max() < 1e82 and 1e-81 < np.abs(sc.band("tiny", n)).max() < 1e-78
    for cls, w in (("width5", 5), ("width63", 63)):
        W = sc.band(cls, n)
        assert not W[dist > w].any() and (W[dist <= w] != 0).all()
    O = sc.band("outer_only", n)
    assert not O[(dist != 0) & (dist != sc.SB)].any() and (O[(dist == 0) | (dist == sc.SB)] != 0).all()
    Zc = sc.band("zero_columns", n)
    for c in range(n):
        below = Zc[c + 1:min(c + sc.SB + 1, n), c]
        assert (not below.any()) if c % 3 == 2 else (below != 0).all()
    N = sc.band("near_identity", n)
    assert np.abs(N - np.eye(n)).max() < 1e-9 and (N - np.eye(n))[dist <= sc.SB].all()
    U = sc.band("outlier", n)
    assert U[n // 2, n // 2] == 1e8 and np.abs(U - np.diag(np.diag(U))).max() < 10
    assert (sc.band("ones", n)[dist <= sc.SB] == 1.0).all()
    for cls, amp in zip(sc.DEAD_CLASSES, (1e-158, 1e-160, 1e-161)):
        D = sc.band(cls, n)
        col = D[1:65, 0]
        assert (col >= 0.5 * amp).all() and (col <= amp).all()
        sq = col * col
        assert (sq < 2.3e-308).all() and sq.sum() < sc.DROP_NRM2      # denormal squares (or zero), below the drop rule
        assert (D[1:, 1:] != 0)[dist[1:, 1:] <= sc.SB].all()


def test_geometry_mirrors_at_the_edge_orders():
    """values worked out by hand from ek_sb2st.hip (the loops of chase_kernel, Layout, q2_groups_of_block)"""
    # tasks: (s, k) exists iff s + 1 + 64 k <= n - 2
    assert [sum(1 for _ in sc.tasks(n)) for n in (1, 2, 3, 4)] == [0, 0, 1, 2]
    assert not sc.task_exists(66, 0, 1) and sc.task_exists(67, 0, 1) and not sc.task_exists(67, 1, 1)
    assert not sc.task_exists(130, 0, 2) and sc.task_exists(131, 0, 2) and not sc.task_exists(131, 1, 2)
    assert [sc.tasks_of_sweep(67, s) for s in (0, 1, 64, 65)] == [2, 1, 1, 0]
    assert sum(1 for _ in sc.tasks(130)) == 64 * 2 + 64
    assert [sc.kmax_of(n) for n in (1, 2, 3, 66, 67, 130, 131, 194, 195, 321)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 5]
    assert sc.task_rows(67, 0, 1) == (65, 67) and sc.task_rows(130, 0, 1) == (65, 129) and sc.task_rows(130, 63, 1) == (128, 130)
    assert sc.task_rows(3, 0, 0) == (1, 3) and sc.task_rows(321, 10, 2) == (139, 203)
    # blocks of 32 sweeps: block S = sweeps 32 S - 1 .. 32 S + 30, nS = ceil((nsweeps + 1) / 32): one more from n = 34 + 32 j on
    assert [sc.q2_nS(n) for n in (1, 2, 3, 4, 33, 34, 35, 65, 66, 67, 68)] == [1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert [sc.q2_nS(n) for n in (97, 98, 99, 129, 130, 131, 193, 194, 195, 196, 321)] == [3, 4, 4, 4, 5, 5, 6, 7, 7, 7, 10]
    assert [sc.q2_groups_of_block(131, S) for S in range(6)] == [3, 2, 2, 1, 1, 0]
    assert [sc.q2_groups_of_block(130, S) for S in range(5)] == [2, 2, 2, 1, 1]
    assert [sc.q2_groups_of_block(129, S) for S in range(5)] == [2, 2, 1, 1, 0]
    assert [sc.q2_groups_of_block(n, 0) for n in (1, 2, 3)] == [0, 0, 1]
    for n in sc.EDGE_ORDERS + sc.LARGE_ORDERS:
        # every reflector belongs to exactly one group: sweep s to block (s + 1) // 32
        groups = {((s + 1) // sc.QG, k) for s, k in sc.tasks(n)}
        assert groups == {(S, k) for S in range(sc.q2_nS(n)) for k in range(sc.q2_groups_of_block(n, S))} or n < 3
        assert sc.q2_groups_of_block(n, sc.q2_nS(n)) == 0
    # passes of one application: bundles of NBLK blocks x slabs of 64 columns
    assert sc.q2_passes(321, 321, 3) == (4, 6, 24) and sc.q2_passes(321, 1, 2) == (5, 1, 5) and sc.q2_passes(98, 65, 3) == (2, 2, 4)
    assert sc.q2_passes(97, 97, 3) == (1, 2, 2) and sc.q2_passes(194, 64, 3) == (3, 1, 3) and sc.q2_passes(193, 64, 3) == (2, 1, 2)
    assert sc.q2_default_nblk(8191) == 3 and sc.q2_default_nblk(8192) == 4


def test_the_wrapped_ticket_counter_shapes_have_more_passes_than_workgroups():
    assert sc.q2_passes(1025, 2304, 2) == (16, 36, 576)
    assert sc.q2_passes(1537, 1537, 2) == (24, 25, 600)
    assert 576 > sc.Q2_WORKGROUPS and 600 > sc.Q2_WORKGROUPS
    assert sc.q2_passes(1025, 2304, 3)[2] <= sc.Q2_WORKGROUPS          # (the form they are compared with does not wrap)


def _emulation_ratios(cls, n):
    B = sc.band(cls, n)
    d, e, V2, tau2 = sc.emulate(B)
    dropped = [(0, 0)] if cls in sc.DEAD_CLASSES and n >= 3 else []
    struct = sc.check_structure(V2, tau2, dropped)
    res, orth = sc.chase_ratios(B, d, e, V2, tau2)
    w = min(n, 6)
    Z = sc.z_input(n, w, "scaled")
    zr = sc.z_ratio(sc.emulate_q2(V2, tau2, Z), sc.apply(sc.reflectors(V2, tau2), Z), n)
    return res, orth, zr, struct / 16.0


@pytest.mark.parametrize("case", sc.CHASE_CASES, ids=sc.case_id)
def test_emulation_spends_at_most_a_quarter_of_every_bound(case):
    n, classes = case
    for cls in classes:
        ratios = _emulation_ratios(cls, n)
        assert max(ratios) <= 0.25, (cls, n, ratios)


@pytest.mark.parametrize("cls", sc.DEAD_CLASSES)
def test_without_the_drop_rule_a_dead_first_column_breaks_orthogonality(cls):
    B = sc.band(cls, 130)
    d, e, V2, tau2 = sc.emulate(B, drop_rule=False)
    assert tau2[0, 0] != 0.0
    _, orth = sc.chase_ratios(B, d, e, V2, tau2)
    assert orth > 1e4
    d, e, V2, tau2 = sc.emulate(B)
    assert tau2[0, 0] == 0.0 and d[0] == B[0, 0] and e[0] == B[1, 0]
    assert sc.chase_ratios(B, d, e, V2, tau2)[1] <= 0.25
