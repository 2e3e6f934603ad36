"""ek_hip_eigenpairs_window_xbatched* on the GPU: a window of eigenpairs (RANGE 'I' / 'V') of every problem of a batch at
orders 129 .. 256 -- the kernel class of ek_hip_eigenpairs_xbatched* with Sturm bisection and inverse iteration on the
rows of the image in place of QL.

  accuracy     random standard and generalized batches of 8 against LAPACK's full spectrum, sliced, under
               window_batched_cases.judge; every window of the table, 'I' and 'V', jobz 0 and 1; under 'V' m[b] differs
  hard inputs  every case of tests/batched_cases.py at 129, 193 and 256 in one launch per window; the clustered classes
               again with the window that cuts their clusters; info = 0 or ek_hip_eigenpairs_xbatched_device's code, and
               never 200000 + k
  bits         the value of index k is the same in every window that holds k; a problem gives the same bits alone, at
               positions 0, 7 and last, across a chunk seam (2 and 1 problems a launch) and in both forms; dA and dB are
               ek_hip_eigenpairs_xbatched_device's; at n = 1, 33, 128 the entry gives the old window entry's bits
  untouched    NaN sentinels wherever nothing may be read or written, padded leading dimensions and gaps included
  own slots    a non-SPD B, a NaN in A, a 'V' window wider than zcap and an empty window in one batch
  many         608 problems of order 129 in chunks of 256: more workgroups than the device holds, a ragged last chunk
  speed        device time against ek_hip_eigenpairs_xbatched_device of the same build, 256 pencils of order 129 and of
               order 256: n / 8 pairs with vectors, and all n values without, each <= 0.75 of the full call

The helpers of tests/test_gpu_window_batched.py that do not name an entry are imported; the device call is restated
with the entry as an argument.  References are computed once per (order, kind) and shared."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import window_batched_cases as wc
from test_gpu_vbatched import _Dev, _Out, _pack, _spd, _sym, _unpack
from test_gpu_window_batched import _image, _pack_lower, _untouched, bits

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (129, 130, 192, 193, 255, 256)
HARD = (129, 193, 256)
_ip = ctypes.POINTER(ctypes.c_int)
NEW, OLD = "ek_hip_eigenpairs_window_xbatched_device", "ek_hip_eigenpairs_window_batched_device"


def _window_device(lib, A, B, jobz, il=None, iu=None, vl=None, vu=None, zcap=None, pad=0, gap=0, entry=NEW):
    """tests/test_gpu_window_batched.py's _window_device with the entry as an argument: images with NaN wherever the
    kernel must neither read nor write."""
    batch, n = A.shape[0], A.shape[1]
    by_value = vl is not None or vu is not None
    if zcap is None:
        zcap = n if by_value else iu - il + 1
    ld = n + pad
    sM, sZ = ld * n + gap, ld * max(zcap, 1) + gap
    o = _Out()
    hA = _pack_lower(A, ld, sM)
    hB = _pack_lower(B, ld, sM) if B is not None else None
    hZ = np.full(max(batch * sZ, 1), np.nan)
    hw = np.full(max(batch * n, 1), np.nan)
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    m = np.full(max(batch, 1), 777, dtype=np.int32)
    with _Dev(lib) as dev:
        dA = dev.up(hA)
        dB = dev.up(hB) if B is not None else None
        dw, dZ = dev.up(hw), dev.up(hZ)
        o.rc = getattr(lib, entry)(
            0 if B is None else 1, jobz, 1 if by_value else 0, n, batch, -np.inf if vl is None else vl,
            np.inf if vu is None else vu, il or 0, iu or 0, dA, ld, sM, dB, ld, sM, m.ctypes.data_as(_ip), dw,
            dZ if jobz else None, ld, zcap, sZ, info.ctypes.data_as(_ip), None)
        o.info, o.m = info[:batch].copy(), m[:batch].copy()
        o.w = dev.down(dw, hw)[:batch * n].reshape(batch, n)
        o.flatZ = dev.down(dZ, hZ)
        o.flatA = dev.down(dA, hA)
        o.flatB = dev.down(dB, hB) if B is not None else None
    o.Z = np.empty((batch, n, max(zcap, 1)))
    for b in range(batch):
        o.Z[b] = o.flatZ[b * sZ:b * sZ + ld * max(zcap, 1)].reshape(max(zcap, 1), ld)[:, :n].T
    o.A = _image(o.flatA, batch, n, ld, sM)
    o.B = _image(o.flatB, batch, n, ld, sM) if B is not None else None
    o.before = (hA, hB)
    o.ld, o.sM, o.sZ, o.zcap = ld, sM, sZ, zcap
    return o


def _xbatched_device(lib, A, B, jobz):
    """ek_hip_eigenpairs_xbatched_device on compact device images of A[b], B[b]."""
    batch, n = A.shape[0], A.shape[1]
    hA = _pack(A, n, n * n)
    hB = _pack(B, n, n * n) if B is not None else None
    hZ, hw = np.zeros(max(batch * n * n, 1)), np.zeros(max(batch * n, 1))
    info = np.full(max(batch, 1), 777, dtype=np.int32)
    o = _Out()
    with _Dev(lib) as dev:
        dA = dev.up(hA)
        dB = dev.up(hB) if B is not None else None
        dw, dZ = dev.up(hw), dev.up(hZ)
        o.rc = lib.ek_hip_eigenpairs_xbatched_device(0 if B is None else 1, jobz, n, batch, dA, n, n * n, dB, n, n * n,
                                                     dw, dZ if jobz else None, n, n * n, info.ctypes.data_as(_ip), None)
        o.info = info[:batch].copy()
        o.w = dev.down(dw, hw)[:batch * n].reshape(batch, n)
        o.A = _unpack(dev.down(dA, hA), batch, n, n, n * n)
        o.B = _unpack(dev.down(dB, hB), batch, n, n, n * n) if B is not None else None
    return o


_random_cache, _hard_cache, _full_cache = {}, {}, {}


def _random(n, problem, batch=8):
    key = (n, problem, batch)
    if key not in _random_cache:
        rng = np.random.default_rng(1000 * n + problem)
        A = np.stack([_sym(rng, n) for _ in range(batch)])
        B = np.stack([_spd(rng, n) for _ in range(batch)]) if problem else None
        ref = [sl.eigh(A[b], B[b], lower=True) if problem else sl.eigh(A[b], lower=True) for b in range(batch)]
        for a in (A, B):
            if a is not None:
                a.setflags(write=False)
        _random_cache[key] = (A, B, ref)
    return _random_cache[key]


def _hard(n, problem):
    key = (n, problem)
    if key not in _hard_cache:
        cases = bc.pencil_batch(n) if problem else bc.standard_batch(n)
        refs = {}
        for c, base in cases:
            if base.name not in refs:
                try:
                    w, Z = sl.eigh(base.A, base.B, lower=True) if base.B is not None else sl.eigh(base.A, lower=True)
                except np.linalg.LinAlgError:
                    w, Z = None, None
                refs[base.name] = (base.exact if base.exact is not None and w is not None else w, Z)
        _hard_cache[key] = (cases, refs)
    return _hard_cache[key]


def _full(lib, n, problem):
    key = (n, problem)
    if key not in _full_cache:
        cases, _ = _hard(n, problem)
        A = np.stack([c.A for c, _ in cases])
        B = np.stack([c.B for c, _ in cases]) if problem else None
        _full_cache[key] = _xbatched_device(lib, A, B, 0)
    return _full_cache[key]


# ---------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", ORDERS)
def test_accuracy_on_random_batches(hip, n, problem):
    lib = hip.load_library()
    A, B, ref = _random(n, problem)
    batch = A.shape[0]
    worst, fails = [0.0, 0.0, 0.0], []
    for wname, il, iu in wc.windows(n):
        vl, vu, span = wc.value_bounds([r[0] for r in ref], il, iu)
        for by_value in (False, True):
            for jobz in (0, 1):
                what = "n=%d problem=%d %s %s jobz=%d" % (n, problem, wname, "V" if by_value else "I", jobz)
                o = (_window_device(lib, A, B, jobz, vl=vl, vu=vu, pad=3, gap=5) if by_value
                     else _window_device(lib, A, B, jobz, il=il, iu=iu, pad=3, gap=5))
                assert o.rc == 0 and not o.info.any(), (what, o.rc, o.info)
                _untouched(o, n, what)
                for b in range(batch):
                    first, m = span[b] if by_value else (il - 1, iu - il + 1)
                    assert o.m[b] == m, (what, b, o.m[b], m)
                    s, f = wc.judge(A[b], None if B is None else B[b], None, ref[b][0], ref[b][1], first, o.w[b, :m],
                                    o.Z[b][:, :m] if jobz else None, "%s b=%d" % (what, b))
                    fails += f
                    if s:
                        worst = [max(x, y or 0.0) for x, y in zip(worst, s)]
    vl, vu = 0.5 * (ref[0][0][0] + ref[0][0][1]), 0.5 * (ref[0][0][n // 2] + ref[0][0][n // 2 + 1])
    counts = [int(((r[0] > vl) & (r[0] <= vu)).sum()) for r in ref]
    o = _window_device(lib, A, B, 0, vl=vl, vu=vu)
    assert list(o.m) == counts and len(set(counts)) > 1, (list(o.m), counts)
    print("n=%d problem=%d share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, problem) + tuple(worst)))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------- hard inputs
def _judge_hard(cases, refs, full, o, first_m, what, shares, fails):
    for b, (c, base) in enumerate(cases):
        name = "%s %s" % (what, c.name)
        if o.info[b] != 0 or full.info[b] != 0:
            if o.info[b] != full.info[b]:
                fails.append("%s: info = %d, ek_hip_eigenpairs_xbatched_device says %d" % (name, o.info[b], full.info[b]))
            if o.info[b] != 0 and o.m[b] != 0:
                fails.append("%s: info = %d with m = %d" % (name, o.info[b], o.m[b]))
            continue
        w_ref, Z_ref = refs[base.name]
        if w_ref is None:
            continue                                # B not numerically SPD and yet factorised: the full entry agreed
        first, m = first_m
        if o.m[b] != m:
            fails.append("%s: m = %d, not %d" % (name, o.m[b], m))
            continue
        with np.errstate(all="ignore"):
            w0 = np.ldexp(o.w[b, :m], -(c.ka - c.kb))
            Z0 = np.ldexp(o.Z[b][:, :m], c.kb // 2)
        s, f = wc.judge(base.A, base.B, c.cond_b, w_ref, Z_ref, first, w0, Z0, name)
        fails += f
        if s:
            cur = shares.setdefault(c.family, [0.0, 0.0, 0.0])
            shares[c.family] = [max(x, y or 0.0) for x, y in zip(cur, s)]


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", HARD)
def test_hard_cases_in_one_batch(hip, n, problem):
    lib = hip.load_library()
    cases, refs = _hard(n, problem)
    full = _full(lib, n, problem)
    A = np.stack([c.A for c, _ in cases])
    B = np.stack([c.B for c, _ in cases]) if problem else None
    shares, fails = {}, []
    for wname, il, iu in wc.windows(n):
        o = _window_device(lib, A, B, 1, il=il, iu=iu)
        assert o.rc == 0, o.rc
        assert not np.any(o.info >= 200000), (wname, o.info)
        _judge_hard(cases, refs, full, o, (il - 1, iu - il + 1), "n=%d problem=%d %s" % (n, problem, wname), shares, fails)
    if not problem:
        for b, (c, base) in enumerate(cases):
            if c.name not in wc.CLUSTERED:
                continue
            cut = wc.cluster_cut(refs[base.name][0])
            assert cut is not None, c.name
            o = _window_device(lib, A[b:b + 1], None, 1, il=cut[0], iu=cut[1])
            assert o.rc == 0 and not np.any(o.info >= 200000), (c.name, o.info)
            one = _Out()
            one.info = full.info[b:b + 1]
            _judge_hard(cases[b:b + 1], refs, one, o, (cut[0] - 1, cut[1] - cut[0] + 1),
                        "n=%d cluster cut %d..%d" % ((n,) + cut), shares, fails)
    for fam in sorted(shares):
        print("n=%d problem=%d | %-28s share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
              % ((n, problem, fam) + tuple(shares[fam])))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:60])


# -------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [129, 256])
def test_value_of_an_index_does_not_depend_on_the_window(hip, n, problem):
    lib = hip.load_library()
    A, B, ref = _random(n, problem)
    whole = _window_device(lib, A, B, 0, il=1, iu=n)
    assert whole.rc == 0 and not whole.info.any()
    for wname, il, iu in wc.windows(n):
        vl, vu, span = wc.value_bounds([r[0] for r in ref], il, iu)
        for jobz in (0, 1):
            o = _window_device(lib, A, B, jobz, il=il, iu=iu, zcap=n)
            assert np.array_equal(bits(o.w[:, :iu - il + 1]), bits(whole.w[:, il - 1:iu])), (wname, jobz, "I")
            o = _window_device(lib, A, B, jobz, vl=vl, vu=vu)
            for b, (first, m) in enumerate(span):
                assert o.m[b] == m
                assert np.array_equal(bits(o.w[b, :m]), bits(whole.w[b, first:first + m])), (wname, jobz, "V", b)


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [129, 256])
def test_same_bits_alone_in_any_batch_across_a_seam_and_in_both_forms(hip, n, problem):
    lib = hip.load_library()
    A, B, _ = _random(n, problem)
    il, iu = n // 4 + 1, n // 4 + 12
    m = iu - il + 1
    alone = _window_device(lib, A[:1], None if B is None else B[:1], 1, il=il, iu=iu)
    assert alone.rc == 0 and alone.info[0] == 0 and alone.m[0] == m
    full = _xbatched_device(lib, A[:1], None if B is None else B[:1], 1)
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(bits(alone.A[0][low]), bits(full.A[0][low])), "dA is not ek_hip_eigenpairs_xbatched_device's"
    if problem:
        assert np.array_equal(bits(alone.B[0][low]), bits(full.B[0][low])), "dB is not ek_hip_eigenpairs_xbatched_device's"
    lim = 4 * n * EPS * np.abs(full.w[0]).max()
    assert np.abs(alone.w[0, :m] - full.w[0, il - 1:iu]).max() <= lim

    def same(o, b, what):
        assert o.rc == 0 and o.info[b] == 0 and o.m[b] == m, what
        assert np.array_equal(bits(o.w[b, :m]), bits(alone.w[0, :m])), what + ": w"
        assert np.array_equal(bits(o.Z[b][:, :m]), bits(alone.Z[0][:, :m])), what + ": Z"
        assert np.array_equal(bits(o.A[b][low]), bits(alone.A[0][low])), what + ": dA"
        if problem:
            assert np.array_equal(bits(o.B[b][low]), bits(alone.B[0][low])), what + ": dB"

    batch = 9
    idx = np.arange(batch) % (A.shape[0] - 1) + 1
    for pos in (0, 7, batch - 1):
        idx[pos] = 0
    for chunk in (0, 2, 1):
        before = hip.window_xbatched_chunk(chunk)
        try:
            o = _window_device(lib, A[idx], None if B is None else B[idx], 1, il=il, iu=iu, pad=1, gap=2)
        finally:
            hip.window_xbatched_chunk(before)
        for pos in (0, 7, batch - 1):
            same(o, pos, "chunk %d position %d" % (chunk, pos))
    w, Z, mm, info = hip.eigenpairs_window_xbatched(A[:2], None if B is None else B[:2], il=il, iu=iu)
    assert info[0] == 0 and mm[0] == m
    assert np.array_equal(bits(w[0, :m]), bits(alone.w[0, :m])), "host form: w"
    assert np.array_equal(bits(Z[0][:, :m]), bits(alone.Z[0][:, :m])), "host form: Z"
    assert not w[0, m:].any(), "host form: w written behind m"


@pytest.mark.parametrize("n", [1, 33, 128])
def test_small_orders_give_the_old_entry_its_bits(hip, n):
    lib = hip.load_library()
    rng = np.random.default_rng(n)
    A = np.stack([_sym(rng, n) for _ in range(3)])
    B = np.stack([_spd(rng, n) for _ in range(3)])
    il, iu = (n + 3) // 4, max((n + 3) // 4, n // 2)
    for kw in (dict(il=il, iu=iu), dict(vl=-0.25, vu=np.inf)):
        new = _window_device(lib, A, B, 1, pad=2, gap=3, **kw)
        old = _window_device(lib, A, B, 1, pad=2, gap=3, entry=OLD, **kw)
        assert new.rc == 0 and old.rc == 0
        assert np.array_equal(new.m, old.m) and np.array_equal(new.info, old.info)
        for x, y in ((new.w, old.w), (new.flatZ, old.flatZ), (new.flatA, old.flatA), (new.flatB, old.flatB)):
            assert np.array_equal(bits(x), bits(y))


# --------------------------------------------------------------------------------------------------------- own slots
@pytest.mark.parametrize("n", [129, 200])
def test_failures_keep_to_their_own_slots(hip, n):
    lib = hip.load_library()
    A, B, ref = _random(n, 1, batch=5)
    idx = np.arange(9) % 5
    A9, B9 = A[idx].copy(), B[idx].copy()
    w0 = ref[0][0]
    vl, vu = 0.5 * (w0[n // 4 - 1] + w0[n // 4]), 0.5 * (w0[n // 2 - 1] + w0[n // 2])
    zcap = max(int(((r[0] > vl) & (r[0] <= vu)).sum()) for r in ref) + 1
    clean = _window_device(lib, A9, B9, 1, vl=vl, vu=vu, zcap=zcap, pad=1, gap=3)
    assert clean.rc == 0 and not clean.info.any() and clean.m.min() > 0
    B9[1] = B9[1] - 3.0 * np.eye(n)                 # not SPD
    A9[3, n // 2, 0] = np.nan                       # lower triangle
    A9[5] = 1e-6 * A9[5] + 0.5 * (vl + vu) * B9[5]  # every eigenvalue in the middle of (vl, vu]: wider than zcap
    A9[7] = A9[7] + 100.0 * B9[7]                   # the spectrum moves up by 100: an empty window
    inside = int(((sl.eigh(A9[5], B9[5], eigvals_only=True) > vl) & (sl.eigh(A9[5], B9[5], eigvals_only=True) <= vu)).sum())
    assert inside > zcap
    o = _window_device(lib, A9, B9, 1, vl=vl, vu=vu, zcap=zcap, pad=1, gap=3)
    assert o.rc == 0
    assert o.info[1] > 0 and o.m[1] == 0
    assert o.info[3] == -5 and o.m[3] == 0
    assert o.info[5] == -20 and o.m[5] == inside
    assert o.info[7] == 0 and o.m[7] == 0
    for b in (1, 3, 5, 7):
        assert np.all(np.isnan(o.w[b])) and np.all(np.isnan(o.Z[b])), b
    _untouched(o, n, "planted")
    for b in (0, 2, 4, 6, 8):
        assert o.info[b] == 0 and o.m[b] == clean.m[b]
        assert np.array_equal(bits(o.w[b, :o.m[b]]), bits(clean.w[b, :o.m[b]])), b
        assert np.array_equal(bits(o.Z[b][:, :o.m[b]]), bits(clean.Z[b][:, :o.m[b]])), b


# --------------------------------------------------------------------------------------------------- many workgroups
def test_more_workgroups_than_the_device_holds_and_a_ragged_chunk(hip):
    lib = hip.load_library()
    n, batch = 129, 608
    A, B, ref = _random(n, 1)
    idx = np.arange(batch) % A.shape[0]
    il, iu = 5, 8
    before = hip.window_xbatched_chunk(256)
    try:
        o = _window_device(lib, A[idx], B[idx], 1, il=il, iu=iu)
    finally:
        hip.window_xbatched_chunk(before)
    assert o.rc == 0 and not o.info.any() and np.all(o.m == 4)
    fails = []
    for b in range(A.shape[0]):
        s, f = wc.judge(A[b], B[b], None, ref[b][0], ref[b][1], il - 1, o.w[b, :4], o.Z[b][:, :4], "b=%d" % b)
        fails += f
    assert not fails, "\n".join(fails)
    for b in range(batch):
        assert np.array_equal(bits(o.w[b, :4]), bits(o.w[idx[b], :4])), b
        assert np.array_equal(bits(o.Z[b]), bits(o.Z[idx[b]])), b


# ------------------------------------------------------------------------------------------------------------- speed
def _speed(lib, n, batch):
    """Device seconds, best of 3, the kinds alternated in one process, inputs refreshed outside the clock."""
    rng = np.random.default_rng(n)
    A = np.stack([_sym(rng, n) for _ in range(8)])[np.arange(batch) % 8]
    B = np.stack([_spd(rng, n) for _ in range(8)])[np.arange(batch) % 8]
    hA = np.ascontiguousarray(A.transpose(0, 2, 1)).ravel()
    hB = np.ascontiguousarray(B.transpose(0, 2, 1)).ravel()
    info = np.zeros(batch, dtype=np.int32)
    m = np.zeros(batch, dtype=np.int32)
    sec = ctypes.c_double(0.0)
    best = {}
    with _Dev(lib) as dev:
        dA, dB = dev.up(hA), dev.up(hB)
        dw, dZ = dev.up(np.zeros(batch * n)), dev.up(np.zeros(batch * n * n))
        ipp, mp = info.ctypes.data_as(_ip), m.ctypes.data_as(_ip)

        def full(jobz):
            return lib.ek_hip_eigenpairs_xbatched_device(1, jobz, n, batch, dA, n, n * n, dB, n, n * n, dw,
                                                         dZ if jobz else None, n, n * n, ipp, ctypes.byref(sec))

        def window(jobz, iu):
            return lib.ek_hip_eigenpairs_window_xbatched_device(1, jobz, 0, n, batch, 0.0, 0.0, 1, iu, dA, n, n * n, dB,
                                                                n, n * n, mp, dw, dZ if jobz else None, n, n, n * n, ipp,
                                                                ctypes.byref(sec))

        kinds = {"full1": lambda: full(1), "full0": lambda: full(0), "window": lambda: window(1, n // 8),
                 "values": lambda: window(0, n)}
        for rep in range(4):                        # the first round warms up
            for name, fn in kinds.items():
                dev.put(dA, hA)
                dev.put(dB, hB)
                assert fn() == 0 and not info.any(), (name, info[info != 0][:4])
                if rep:
                    best[name] = min(best.get(name, np.inf), sec.value)
    return best


@pytest.mark.parametrize("n", [129, 256])
def test_a_window_costs_at_most_three_quarters_of_the_full_call(hip, n):
    lib = hip.load_library()
    t = _speed(lib, n, 256)
    r1, r0 = t["window"] / t["full1"], t["values"] / t["full0"]
    print("n=%d batch=256 ms: full with vectors %.3f, window of n/8 with vectors %.3f (%.3f); full values %.3f, all values "
          "by bisection %.3f (%.3f)" % (n, 1e3 * t["full1"], 1e3 * t["window"], r1, 1e3 * t["full0"], 1e3 * t["values"],
                                        r0))
    assert r1 <= 0.75, r1
    assert r0 <= 0.75, r0
