"""Host side of the back-transformation's stage tests (no GPU needed): the stage entry ek_hip_debug_ormtr is declared in
the debug header only, exported, bound, wrapped and refuses bad arguments before any device work; the inputs of
tests/test_gpu_ormtr_stages.py are what they claim to be; the long-double reference is orthogonal; a float64 numpy
emulation of the kernels' algorithm spends at most 1/8 of both bounds the GPU file asserts; and the Python mirror of
ormtr_apply's choice of form puts every (order, width) of the lists into the form it was chosen for."""
import ctypes
import os
import re

import numpy as np
import pytest

import ormtr_cases as oc
from eigenkernel_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK = "ek_hip_debug_ormtr"


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
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert callable(solver.debug_ormtr)
    assert HOOK in open(os.path.join(ROOT, "README.md")).read()


def test_entry_refuses_bad_arguments_before_any_device_work():
    """-k for the k-th argument; none of these calls initialises a device"""
    lib = solver.load_library()
    n, nc = 40, 5
    V = np.zeros((n, n), order="F")
    tau = np.zeros(n)
    Z = np.zeros((n, nc), order="F")
    P = solver._P

    def call(n=n, ncols=nc, V=P(V), ldv=n, tau=P(tau), Z=P(Z), ldz=n, ncg=0, slab=0):
        return lib.ek_hip_debug_ormtr(n, ncols, V, ldv, tau, Z, ldz, ncg, slab)

    assert call(n=-1) == -1
    assert call(ncols=-1) == -2
    assert call(V=None) == -3
    assert call(ldv=n - 1) == -4
    assert call(n=0, ldv=0) == -4
    assert call(tau=None) == -5
    assert call(Z=None) == -6
    assert call(ldz=n - 1) == -7


@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("n", [1, 2, 3, 66, 130, 514])
def test_every_generated_reflector_is_a_householder_reflector(cls, n):
    V, tau = oc.reflectors(cls, n)
    assert V.shape == (n, n) and tau.shape == (max(n - 1, 0),) and V.flags.f_contiguous
    off = oc.BAND if cls == "band" else 1
    # zero above the unit entry, the unit entry itself, |v_i| <= 1; column n - 1 is no reflector
    assert not np.triu(V, 1 - off).any()
    assert np.abs(V).max(initial=0.0) <= 1.0 and not V[:, n - 1:].any()
    live = tau != 0.0
    for j in range(n - 1):
        v = V[:, j]
        if live[j]:
            assert v[j + off] == 1.0
            assert 1.0 <= tau[j] <= 2.0
            # (tau and the divisor of v carry the roundings of hypot, a difference and a division each, the divisor
            # twice in v^T v: at most 8 of relative size eps / 2 .. eps on a value of 2)
            assert abs(tau[j] * np.dot(v.astype(oc.LD), v.astype(oc.LD)) - 2.0) <= 16 * oc.EPS
        else:
            assert not v.any()
    dead = set(np.nonzero(~live)[0])
    if cls == "band":
        assert dead == set(range(max(n - 1 - oc.BAND, 0), n - 1))           # the last 64 reflectors
    elif cls == "tau0":
        assert dead == set(range(2, n - 1, 3)) | ({n - 2} if n > 1 else set())
    else:
        assert dead == ({n - 2} if n > 1 else set())                        # DLARFG on a column of one entry
    if cls == "graded" and n >= 66:
        mags = np.abs(V[np.tril_indices(n, -2)])
        assert (mags[mags > 0] < 1e-9).mean() > 0.1 and (mags > 1e-3).mean() > 0.1
    V2, tau2 = oc.reflectors(cls, n)
    assert V2 is V and tau2 is tau and not V.flags.writeable               # made once, shared, left unchanged


@pytest.mark.parametrize("cls", oc.PACKED_CLASSES)
@pytest.mark.parametrize("n", [1, 2, 3, 130, 514])
def test_packed_and_explicit_forms_agree(cls, n):
    """unpacking the PDSYTRD storage as build_v_kernel does returns the explicit V; the packed form implies the unit entry,
    so an identity reflector (tau = 0) shows e_(j+1) there, which tau = 0 takes out of the product"""
    V, tau = oc.reflectors(cls, n)
    A, tau_p = oc.packed(cls, n)
    assert tau_p is tau and A.flags.f_contiguous
    U = oc.unpack(A)
    E = np.array(V)
    j = np.nonzero(tau == 0.0)[0]
    E[j + 1, j] = 1.0
    assert np.array_equal(U, E)
    assert np.array_equal(oc.unpack(oc.packed(cls, n, fill=np.nan)[0]), E)
    if n >= 3:
        assert np.abs(A[~np.tri(n, n, -2, dtype=bool)]).min() > 0.0                           # what is never read is not left zero
    if n == 130:
        Z = oc.columns(n, 5)
        assert np.array_equal(oc.apply_sequential(U, tau, Z), oc.apply_sequential(V, tau, Z))


def test_longdouble_reference_is_orthogonal():
    assert np.finfo(oc.LD).eps < 1.1e-19                                    # an extended format, not a synonym of float64
    n = 130
    for cls in oc.CLASSES:
        V, tau = oc.reflectors(cls, n)
        Q = oc.apply_sequential(V, tau, np.eye(n))
        assert float(np.abs(Q.T @ Q - np.eye(n)).max()) <= 4 * n * oc.EPS, cls
        Qt = oc.apply_sequential(V, tau, np.eye(n), trans=True)
        assert float(np.abs(Qt - Q.T).max()) <= 4 * n * oc.EPS, cls
        assert float(np.abs(Q - np.eye(n)).max()) > 0.5                     # and it is no identity


@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("n,ncols", [(1026, 129), (4097, 7)])
def test_emulation_spends_an_eighth_of_the_bounds(cls, n, ncols):
    """the float64 emulation of the kernels' algorithm, and the plain float64 sequential application, against the
    long-double reference: the reference alone stays well inside what the GPU file asserts"""
    V, tau = oc.reflectors(cls, n)
    Z = oc.columns(n, ncols)
    r = oc.reference(cls, n, ncols)
    assert r["scale"] > 0.1
    oc.check(oc.emulate(V, tau, Z), r, "emulation %s n=%d ncols=%d" % (cls, n, ncols), fraction=0.125)
    seq = np.asarray(oc.apply_sequential(V, tau, Z, dtype=np.float64), dtype=np.float64)
    oc.check(seq, r, "sequential float64 %s n=%d ncols=%d" % (cls, n, ncols), fraction=0.125)
    # the checks do see an error: one reflector left out, and one entry moved by 4 n eps
    tau_bad = np.array(tau)
    tau_bad[n // 2 + int(np.argmax(tau[n // 2:] != 0.0))] = 0.0
    with pytest.raises(AssertionError):
        oc.check(oc.emulate(V, tau_bad, Z), r, "planted: a reflector left out")
    bad = np.array(seq)
    bad[n - 1, ncols - 1] += 4 * oc.bound_elementwise(n, r["scale"])
    with pytest.raises(AssertionError):
        oc.check(bad, r, "planted: one entry of the last sample column")


def test_sample_columns_and_slab_widths():
    assert oc.sample_columns(1) == [0] and oc.sample_columns(7) == list(range(7)) and oc.sample_columns(8) == list(range(8))
    assert oc.sample_columns(129) == [0, 1, 127, 128] and oc.sample_columns(1025) == [0, 1, 127, 128, 511, 512, 1024]
    assert oc.sample_columns(513) == [0, 1, 127, 128, 511, 512]
    # Path::slab_width, zslab = 512: the last slabs are narrower
    assert oc.slab_widths(1000, 512) == [256, 256, 488]
    assert oc.slab_widths(400, 512) == [400] and oc.slab_widths(2304, 512) == [512, 512, 512, 256, 512]
    for nc in range(1, 3000, 7):
        ws = oc.slab_widths(nc, 512)
        assert sum(ws) == nc and min(ws) > 0


def test_mirror_puts_every_case_into_its_form():
    # edge orders: nrefl = 512, 513, 1023, 1024, 1025, 1536 -- full == nblk against a short last block, kb = 1
    kbs = {n: [f["kb"] for f in oc.block_forms(n, n)] for n in oc.EDGE_ORDERS}
    assert kbs == {513: [512], 514: [1, 512], 1024: [511, 512], 1025: [512, 512], 1026: [1, 512, 512],
                   1537: [512, 512, 512]}
    for n in oc.EDGE_ORDERS:
        for w in oc.WIDTHS:
            assert all(f["S"] == 1 for f in oc.block_forms(n, oc.width(n, w)))     # nothing is split below 4096 rows
    # the split of the widths at the split orders
    for n in oc.SPLIT_ORDERS:
        got = [oc.ormtr_split(oc.width(n, w)) for w in oc.WIDTHS]
        assert got[:4] == [16, 16, 16, 7] and got[4] == (4 if n == 4096 else 3)
    f = {n: {w: [b for b in oc.block_forms(n, oc.width(n, w)) if b["S"] > 1] for w in oc.WIDTHS} for n in oc.SPLIT_ORDERS}
    for w in (1, 7, 129, 2304):
        # 4096: equal slices, one batched launch (a split of 16; seven slices are ragged there too); 4097: a ragged last
        # slice; 4610: the two lowest blocks are split
        (b,) = f[4096][w]
        assert b["b"] == 0 and (b["S"] - 1) * b["kc"] + b["klast"] == 4096
        assert (b["klast"] == b["kc"]) == (w != 2304)
        (b,) = f[4097][w]
        assert b["b"] == 0 and 0 < b["klast"] < b["kc"] and (b["S"] - 1) * b["kc"] + b["klast"] == 4097
        assert [b["b"] for b in f[4610][w]] == [1, 0] and [b["m"] for b in f[4610][w]] == [4098, 4610]
    assert [(b["S"], b["kc"], b["klast"]) for b in f[4096][1]] == [(16, 256, 256)]
    assert [(b["S"], b["kc"], b["klast"]) for b in f[4097][1]] == [(16, 258, 227)]
    assert [(b["S"], b["kc"], b["klast"]) for b in f[4097][2304]] == [(7, 586, 581)]
    assert [(b["S"], b["kc"], b["klast"]) for b in f[4610][None]] == [(3, 1366, 1366), (3, 1538, 1534)]
    # the contract test's pairs: widths 75 and 1000 share a split, 129 and 2304 do not
    assert oc.ormtr_split(75) == oc.ormtr_split(1000) == 16 and oc.ormtr_split(129) != oc.ormtr_split(2304)


def test_slices_never_outnumber_the_split():
    """S <= ormtr_split(...) for every m: the partials fit what ormtr_work_bytes reserves; the slices start on even rows,
    cover m exactly and the last one is not empty"""
    splits = sorted({oc.ormtr_split(w) for w in range(1, 20000)})
    assert splits == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16]
    for w in (1, 7, 129, 2304, 4610, 9000):
        assert oc.ormtr_split(w) in splits
    for smax in splits:
        for m in range(4096, 9001):
            kc, s, klast = oc.slices(m, smax)
            assert 1 <= s <= smax, (m, smax)
            assert kc % 2 == 0 or s == 1
            assert (s - 1) * kc + klast == m and 0 < klast <= kc, (m, smax)
    for smax in splits:
        for m in (1, 2, 513, 4095):
            assert oc.slices(m, smax)[1] == 1
