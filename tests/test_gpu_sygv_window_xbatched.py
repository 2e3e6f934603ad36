"""ek_hip_sygv_window_xbatched* on the GPU: the window of eigenpairs of A B x = l x (itype 2) and B A x = l x (itype 3) at
orders 129 .. 256, where the image lies in device memory and the wanted vectors are rows of it.  The nine groups of
tests/test_gpu_sygv_window_batched.py, called as they stand with ek_hip_sygv_xbatched_device as the full call and
ek_hip_debug_window_xbatched_chunk as the chunk hook (a batch of 8 in chunks of 3), and beside them:

  forwarding   the xbatched pair returns the batched pair's bits at orders 1, 33 and 128
  a long batch 608 pencils of order 129 in chunks of 256 with a window of 4 pairs: every problem the bits it has alone
  clusters     the planted-cluster pencils at 129 and 256 (all_equal at 256 with the cluster-cut window is 254 rounds of
               inverse iteration: two copies per launch)
  cost         256 pencils of order 129 and of order 256: <= 0.75 of ek_hip_sygv_xbatched_device of the same type and jobz
               (the gate of the type-1 window call at these orders), <= 1.25 of the type-1 window call

Accuracy runs at 129, 130, 192, 193, 255 and 256 (odd and even, both sides of the half boundary of the pair map),
everything else at 129 and 256.  Largest shares of the bounds used on one MI355X (eigenvalues / residual / orthogonality):
random pairs 0.015 / 0.001 / 0.001, Z3 = B Z2 0.0003, hard pencils 0.010 / 0.003 / 0.239 of the rule, planted clusters
0.010 / 0.007 / 0.001."""
import numpy as np
import pytest

import sygv_window_cases as sw
import test_gpu_sygv_window_batched as base
from test_gpu_sygv_batched import _bits

pytestmark = pytest.mark.gpu
ACCURACY_ORDERS = (129, 130, 192, 193, 255, 256)
ORDERS = (129, 256)
CFG = base.Config("ek_hip_sygv_window_xbatched_device", "ek_hip_eigenpairs_window_xbatched_device",
                  "ek_hip_sygv_xbatched_device", "sygv_window_xbatched", "window_xbatched_chunk")
itypes = pytest.mark.parametrize("itype", [2, 3])


@itypes
@pytest.mark.parametrize("n", ACCURACY_ORDERS)
def test_accuracy_against_scipy(hip, n, itype):
    base.check_accuracy(hip, CFG, n, itype)


@pytest.mark.parametrize("n", ORDERS)
def test_invariants_between_the_types(hip, n):
    base.check_between_the_types(hip, CFG, n)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_images_are_those_of_the_full_call(hip, n, itype):
    base.check_against_the_full_call(hip, CFG, n, itype)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_value_of_an_index_is_the_same_bits_everywhere(hip, n, itype):
    base.check_bits_of_the_values(hip, CFG, n, itype, chunk=3)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_what_is_not_the_calls_is_left_alone(hip, n, itype):
    base.check_left_alone(hip, CFG, n, itype)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_failures_keep_to_their_own_slots(hip, n, itype):
    base.check_failures_keep_to_their_own_slots(hip, CFG, n, itype)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_hard_pencils_under_the_rule(hip, n, itype):
    base.check_hard_pencils(hip, CFG, n, itype)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_planted_clusters(hip, n, itype):
    base.check_planted_clusters(hip, CFG, n, itype)


@itypes
def test_scale_covariance(hip, itype):
    base.check_scale_covariance(hip, CFG, 129, itype)


@itypes
@pytest.mark.parametrize("n", ORDERS)
def test_behind_the_gpus_own_check(hip, n, itype):
    base.check_behind_the_gpu_check(hip, CFG, n, itype)


@itypes
@pytest.mark.parametrize("n", [1, 33, 128])
def test_orders_up_to_128_give_the_batched_pairs_bits(hip, n, itype):
    lib = hip.load_library()
    A, B = sw.pairs(n)
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    for jobz in (0, 1):
        x = sw.window_device(lib, CFG.window, itype, A, B, jobz, il=il, iu=iu, pad=1, gap=3)
        o = sw.window_device(lib, base.CFG.window, itype, A, B, jobz, il=il, iu=iu, pad=1, gap=3)
        assert x.rc == 0 and o.rc == 0 and not o.info.any()
        assert np.array_equal(x.info, o.info) and np.array_equal(x.m, o.m)
        for name in ("w", "flatZ", "flatA", "flatB"):
            assert np.array_equal(_bits(getattr(x, name)), _bits(getattr(o, name))), (jobz, name)
    w, Z, m, info = hip.sygv_window_xbatched(A, B, itype=itype, il=il, iu=iu)
    w0, Z0, m0, info0 = hip.sygv_window_batched(A, B, itype=itype, il=il, iu=iu)
    assert np.array_equal(_bits(w), _bits(w0)) and np.array_equal(_bits(Z), _bits(Z0))
    assert np.array_equal(m, m0) and np.array_equal(info, info0)


@itypes
def test_608_pencils_of_order_129_in_chunks_of_256(hip, itype):
    """Three launches, two seams: every problem has the bits of its pair in a batch of 8."""
    lib = hip.load_library()
    n, batch, il, iu = 129, 608, 60, 63
    A, B = sw.pairs(n)
    ref = sw.window_device(lib, CFG.window, itype, A, B, 1, il=il, iu=iu)
    assert ref.rc == 0 and not ref.info.any()
    idx = (np.arange(batch) * 5) % 8
    before = hip.window_xbatched_chunk(256)
    try:
        o = sw.window_device(lib, CFG.window, itype, A[idx], B[idx], 1, il=il, iu=iu)
    finally:
        hip.window_xbatched_chunk(before)
    assert o.rc == 0 and not o.info.any() and np.all(o.m == 4)
    assert np.array_equal(_bits(o.w[:, :4]), _bits(ref.w[idx, :4]))
    assert np.array_equal(_bits(o.Z), _bits(ref.Z[idx]))
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(_bits(o.A[:, low]), _bits(ref.A[idx][:, low]))
    assert np.array_equal(_bits(o.B[:, low]), _bits(ref.B[idx][:, low]))


@pytest.mark.parametrize("n", ORDERS)
def test_a_window_of_types_2_and_3_costs_what_it_should(hip, n):
    """256 pencils: <= 0.75 of ek_hip_sygv_xbatched_device of the same type and jobz (the gate of
    tests/test_gpu_window_xbatched.py; that call's kernels are the parent's instructions) and <= 1.25 of the type-1
    window call of the same build.  Measured on one MI355X, types 2 / 3: order 129: window / full 0.371 /
    0.372, values / full 0.415 / 0.413, window / type 1's 0.908 / 0.925, values / type 1's 0.918 / 0.913; order 256: 0.364 /
    0.348, 0.422 / 0.422, 0.880 / 0.894, 0.826 / 0.828.  None is within 10 % of its gate."""
    base.check_cost(hip, CFG, n, 256, 0.75)
