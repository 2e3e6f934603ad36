"""The back-transformation Z <- Q Z (ek_ormtr.hip: ormtr_prepare, ormtr_apply, larft_kernel, build_v_kernel,
sum_partials_kernel) as the whole path reaches it, through ek_hip_debug_ormtr (explicit reflectors, ncols_global, the T
factors formed once and applied in column slabs) and ek_hip_ormtr (PDSYTRD storage).

Inputs, references and bounds are those of tests/ormtr_cases.py: sample columns against the sequential application in
numpy.longdouble to n EPS max|ref|, every column through the projection identity to n times that; each case prints
error / bound.  tests/test_ormtr_cases_host.py shows that a float64 emulation of the algorithm spends at most 1/8 of
either bound.  Where two results are claimed to be the same bits they are compared with numpy.array_equal."""
import struct

import numpy as np
import pytest

import ormtr_cases as oc

pytestmark = pytest.mark.gpu

NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8DEAD0000BEEF))[0]     # a quiet NaN with a payload


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _cases(classes, orders, widths):
    """(class, order, width) with class and order outermost: consecutive cases share the reflectors"""
    return [(c, n, w) for c in classes for n in orders for w in widths(n)]


def _run_both(hip, cls, n, Z, **kw):
    """Q Z through the stage entry and, where the class has a packed form, through ek_hip_ormtr: the same bits"""
    V, tau = oc.reflectors(cls, n)
    got = hip.debug_ormtr(V, tau, Z, **kw)
    if cls in oc.PACKED_CLASSES and Z.shape[1] > 0:
        A, _ = oc.packed(cls, n)
        got2, info = hip.ormtr(A, tau, Z)
        assert info == 0
        assert np.array_equal(got2, got), (cls, n, Z.shape[1])
    return got


EDGE_CASES = _cases(oc.CLASSES, oc.EDGE_ORDERS, lambda n: (1, 7, 129, None))


@pytest.mark.parametrize("cls,n,w", EDGE_CASES)
def test_block_edges(hip, cls, n, w):
    """nrefl = 512, 513, 1023, 1024, 1025, 1536: one, two and three full blocks (the batched Gram GEMM with its table of
    offsets and dims, the batched coupling GEMMs), a short last block, a last block of one reflector, no block short"""
    ncols = oc.width(n, w)
    forms = oc.block_forms(n, ncols)
    assert all(f["S"] == 1 for f in forms)
    got = _run_both(hip, cls, n, oc.columns(n, ncols))
    oc.check(got, oc.reference(cls, n, ncols), "edges %s n=%d ncols=%d blocks=%s" % (cls, n, ncols, [f["kb"] for f in forms]))


SPLIT_CASES = _cases(("random", "band"), oc.SPLIT_ORDERS,
                     lambda n: tuple(w for w in oc.WIDTHS if w is not None or n == 4610))


@pytest.mark.parametrize("cls,n,w", SPLIT_CASES)
def test_split_k(hip, cls, n, w):
    """W1 = V_b^T Z cut along K: equal slices in one batched launch (4096), a ragged last slice in a launch of its own
    (4097), the two lowest blocks both split (4610); sum_partials_kernel with 16, 7 and 3 partials"""
    ncols = oc.width(n, w)
    split = [f for f in oc.block_forms(n, ncols) if f["S"] > 1]
    smax = {1: 16, 7: 16, 129: 16, 2304: 7, None: 3}[w]
    assert oc.ormtr_split(ncols) == smax and all(f["S"] == smax for f in split)
    if n == 4096:
        assert [f["b"] for f in split] == [0] and (split[0]["klast"] == split[0]["kc"]) == (smax == 16)
    elif n == 4097:
        assert [f["b"] for f in split] == [0] and split[0]["klast"] < split[0]["kc"]
    else:
        assert [f["b"] for f in split] == [1, 0]
    got = _run_both(hip, cls, n, oc.columns(n, ncols))
    oc.check(got, oc.reference(cls, n, ncols), "split %s n=%d ncols=%d S=%d kc=%s klast=%s"
             % (cls, n, ncols, smax, [f["kc"] for f in split], [f["klast"] for f in split]))


@pytest.mark.parametrize("cls,n", [("random", 1537), ("band", 1537), ("random", 4097), ("band", 4097)])
def test_a_cells_or_slabs_columns_carry_the_1x1_bits(hip, cls, n):
    """ormtr_apply on some of the columns, told the width of the whole Z, returns the bits of the one call over the whole Z:
    the contract a grid cell's share and a staging slab rest on"""
    nc = 1000
    V, tau = oc.reflectors(cls, n)
    Z = oc.columns(n, nc)
    full = hip.debug_ormtr(V, tau, Z)
    oc.check(full, oc.reference(cls, n, nc), "contract %s n=%d ncols=%d (the one call)" % (cls, n, nc))
    assert np.array_equal(hip.debug_ormtr(V, tau, Z, ncols_global=nc, slab=256), full)
    assert np.array_equal(hip.debug_ormtr(V, tau, Z, slab=75), full)
    assert np.array_equal(hip.debug_ormtr(V, tau, Z[:, 300:375], ncols_global=nc), full[:, 300:375])
    widths = oc.slab_widths(nc, 512)
    assert widths == [256, 256, 488]                                     # Path::slab_width, zslab = 512
    c0 = 0
    for wd in widths:
        assert np.array_equal(hip.debug_ormtr(V, tau, Z[:, c0:c0 + wd], ncols_global=nc), full[:, c0:c0 + wd]), (c0, wd)
        c0 += wd
    if n == 4097:
        # widths 75 and 1000 take the same split, so the above holds with or without ncols_global; 129 columns of 2304
        # do not: without the whole width they are sliced 16 times, not 7, and the bits differ
        wide, part = 2304, 129
        assert oc.ormtr_split(75) == oc.ormtr_split(nc) and oc.ormtr_split(part) != oc.ormtr_split(wide)
        assert any(f["S"] > 1 for f in oc.block_forms(n, wide))
        Z2 = oc.columns(n, wide)
        full2 = hip.debug_ormtr(V, tau, Z2)
        alone = hip.debug_ormtr(V, tau, Z2[:, :part], ncols_global=part)
        told = hip.debug_ormtr(V, tau, Z2[:, :part], ncols_global=wide)
        assert not np.array_equal(alone, full2[:, :part])
        assert np.array_equal(told, full2[:, :part])
        r = oc.make_reference(V, tau, Z2[:, :part])
        oc.check(alone, r, "contract %s n=%d ncols=%d sliced for %d" % (cls, n, part, part))
        oc.check(told, r, "contract %s n=%d ncols=%d sliced for %d" % (cls, n, part, wide))


@pytest.mark.parametrize("cls,n", [("tau0", 1026), ("band", 4097)])
def test_prepare_once_apply_many(hip, cls, n):
    """slabs of two widths against the one call, and the first call again: no state survives in the prepared factors"""
    nc = 300
    V, tau = oc.reflectors(cls, n)
    Z = oc.columns(n, nc)
    first = hip.debug_ormtr(V, tau, Z, slab=128)
    second = hip.debug_ormtr(V, tau, Z, slab=37)
    again = hip.debug_ormtr(V, tau, Z, slab=128)
    assert np.array_equal(first, second) and np.array_equal(first, again)
    assert np.array_equal(first, hip.debug_ormtr(V, tau, Z))
    oc.check(first, oc.reference(cls, n, nc), "slabs %s n=%d ncols=%d" % (cls, n, nc))


def test_reflectors_of_the_one_stage_tridiagonalisation(hip, oracle):
    n, nc = 700, 129
    Ar, d, e, tau, info = hip.sytrd(oracle.synth_matrix(n, 1))
    assert info == 0
    V = oc.unpack(Ar)
    Z = np.asfortranarray(np.random.default_rng(n).uniform(-1, 1, (n, nc)))
    got = hip.debug_ormtr(V, tau, Z)
    got2, info = hip.ormtr(Ar, tau, Z)
    assert info == 0 and np.array_equal(got, got2)
    assert np.count_nonzero(tau) >= n - 2
    oc.check(got, oc.make_reference(V, tau, Z), "sytrd's reflectors n=%d ncols=%d" % (n, nc))


def test_reflectors_of_the_dense_to_band_stage(hip, oracle):
    n, nc = 1100, 129
    _, V, tau, flag = hip.sy2sb(oracle.synth_matrix(n, 1))
    assert flag == 0
    # the band form: column j is zero through row j + 63, which is what the `band` class rests on
    assert not np.triu(V, 1 - oc.BAND).any()
    assert np.count_nonzero(tau[:n - 1]) >= n - 2 - oc.BAND
    Z = np.asfortranarray(np.random.default_rng(n).uniform(-1, 1, (n, nc)))
    got = hip.debug_ormtr(V, tau[:n - 1], Z)
    oc.check(got, oc.make_reference(V, tau[:n - 1], Z), "sy2sb's reflectors n=%d ncols=%d" % (n, nc))


@pytest.mark.parametrize("n", [514, 1025])
@pytest.mark.parametrize("w", [7, None])
def test_never_read_never_written(hip, n, w):
    """ek_hip_ormtr reads A strictly below the subdiagonal only, and neither reads nor writes the padding of local arrays
    whose leading dimension exceeds n"""
    cls, ncols = "random", oc.width(n, w)
    A, tau = oc.packed(cls, n)
    Z = oc.columns(n, ncols)
    clean, info = hip.ormtr(A, tau, Z)
    assert info == 0
    oc.check(clean, oc.reference(cls, n, ncols), "packed %s n=%d ncols=%d" % (cls, n, ncols))
    # NaN on and above the subdiagonal
    An, _ = oc.packed(cls, n, fill=NAN)
    assert np.isnan(An).sum() == n * (n + 1) // 2 + n - 1
    got, info = hip.ormtr(An, tau, Z)
    assert info == 0 and np.array_equal(got, clean)
    # LLD = n + 3, NaN in the padding of A and Z
    lld = n + 3
    Ab = np.full((lld, n), NAN, order="F")
    Zb = np.full((lld, ncols), NAN, order="F")
    Ab[:n] = An
    Zb[:n] = Z
    A_before, Z_before = _bits(Ab).copy(), _bits(Zb).copy()
    t = np.zeros(n)
    t[:n - 1] = tau
    lib = hip.load_library()
    dA, dZ = hip._desc_for(Ab[:n]), hip._desc_for(Zb[:n])
    assert dA[8] == lld and dZ[8] == lld
    assert lib.ek_hip_ormtr(n, ncols, hip._P(Ab), hip._I(dA), hip._P(t), hip._P(Zb), hip._I(dZ)) == 0
    assert np.array_equal(Zb[:n], clean)
    assert np.array_equal(_bits(Zb)[n:], Z_before[n:])                   # the padding returns bit for bit
    assert np.array_equal(_bits(Ab), A_before)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_degenerate_orders(hip, n):
    for cls in oc.CLASSES:
        V, tau = oc.reflectors(cls, n)
        for ncols in (0, 1, 5):
            Z = oc.columns(n, ncols)
            got = _run_both(hip, cls, n, Z)
            assert got.shape == (n, ncols)
            if not tau.any():
                assert np.array_equal(got, Z)                            # n = 1, 2: no reflector that is not the identity
            elif ncols:
                oc.check(got, oc.reference(cls, n, ncols), "degenerate %s n=%d ncols=%d" % (cls, n, ncols))


def test_all_tau_zero_returns_z_bit_for_bit(hip):
    n, nc = 700, 9
    V, _ = oc.reflectors("random", n)
    A, _ = oc.packed("random", n)
    Z = oc.columns(n, nc)
    tau = np.zeros(n - 1)
    assert np.array_equal(_bits(hip.debug_ormtr(V, tau, Z)), _bits(Z))
    got, info = hip.ormtr(A, tau, Z)
    assert info == 0 and np.array_equal(_bits(got), _bits(Z))


@pytest.mark.parametrize("n,j", [(1100, 0), (1100, 600), (1100, 1098), (3, 0)])
def test_one_reflector_only(hip, n, j):
    nc = 9
    cls = "graded" if n > 3 else "random"
    V, tau = oc.reflectors(cls, n)
    if j == n - 2 and n > 3:
        # the last column holds no reflector of more than one entry: H = I - 2 e e^T, a change of sign
        V = np.array(V); V[n - 1, j] = 1.0
        one = np.zeros(n - 1); one[j] = 2.0
    else:
        one = np.zeros(n - 1); one[j] = tau[j]
        assert one[j] != 0.0
    Z = oc.columns(n, nc)
    got = hip.debug_ormtr(V, one, Z)
    oc.check(got, oc.make_reference(V, one, Z), "one reflector n=%d j=%d" % (n, j))
    # H(j) touches rows j + 1 .. n - 1 and nothing else
    assert np.array_equal(got[:j + 1], Z[:j + 1]) and not np.array_equal(got[j + 1:], Z[j + 1:])
