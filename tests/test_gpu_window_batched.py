"""ek_hip_eigenpairs_window_batched* on the GPU: a window of eigenpairs (RANGE 'I' / 'V') of every problem of a batch by
Sturm bisection and inverse iteration, orders 1 .. 128.

  accuracy     random standard and generalized batches against LAPACK under the suite's bounds (tests/
               window_batched_cases.py::judge), every window of the table, jobz 0 and 1, 'I' and 'V'; under 'V' m[b]
               differs from problem to problem
  hard inputs  STANDARD, PENCILS, the scaled cases and the Hilbert rule of tests/batched_cases.py, every case of an order
               in one launch, judged on the window's columns; the clustered classes also with a window whose edges cut
               a cluster.  Every case ends with info = 0 or the code ek_hip_eigenpairs_batched_device gives
  bits         the value of index k is the same in every window that holds k, for both ranges and both jobz; a problem
               gives the same bits alone, at positions 0, 7 and last of batches of 8 and 300, across a chunk seam, in host
               and device form; dA and dB are left as ek_hip_eigenpairs_batched_device leaves them; its w agrees to the
               bound
  untouched    NaN in the strictly upper triangles, rows n..ld-1, the gaps, dw[b, m[b]:] and Z's columns from m[b] on
  own slots    a non-SPD B, a NaN in A, a 'V' window wider than zcap and an empty window in one batch: their neighbours
               keep their bits
  speed        device time against ek_hip_eigenpairs_batched_device of the same build: a window of n / 8 pairs with
               vectors and all n values without must take <= 0.6 of it (512 pencils of order 128, 1024 of order 64)

The truth is the full-spectrum reference, sliced.  References are computed once per (order, kind) and shared."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
import window_batched_cases as wc
from test_gpu_vbatched import _Dev, _Out, _batched_device, _spd, _sym

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16
ORDERS = (1, 2, 3, 17, 30, 32, 33, 64, 65, 100, 128)
_ip = ctypes.POINTER(ctypes.c_int)
bits = lambda x: np.ascontiguousarray(x).view(np.uint64)  # noqa: E731


def _pack_lower(M, ld, stride):
    """Lower triangles only, column-major with leading dimension ld, a problem every `stride` doubles; NaN everywhere
    else: the strictly upper triangles, the rows n..ld-1 and the gaps."""
    batch, n = M.shape[0], M.shape[1]
    flat = np.full(max(batch * stride, 1), np.nan)
    low = np.tril(np.ones((n, n), dtype=bool))
    for b in range(batch):
        img = flat[b * stride:b * stride + ld * n].reshape(n, ld)      # img[j, i] = element (i, j)
        img[:, :n][low.T] = M[b].T[low.T]
    return flat


def _image(flat, batch, n, ld, stride):
    """(batch, n, n) with element (i, j) of problem b at [b, i, j]."""
    out = np.empty((batch, n, n))
    for b in range(batch):
        out[b] = flat[b * stride:b * stride + ld * n].reshape(n, ld)[:, :n].T
    return out


def _window_device(lib, A, B, jobz, il=None, iu=None, vl=None, vu=None, zcap=None, pad=0, gap=0):
    """The device entry on images with NaN wherever the kernel must neither read nor write.  Returns rc, m, info, w
    (batch, n), Z (batch, n, zcap), the images of A and B after the call and the flat buffers before and after."""
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
        o.rc = lib.ek_hip_eigenpairs_window_batched_device(
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


def _untouched(o, n, what):
    """NaN survives wherever the call must not write, and was never read into a result (info = 0 comes with finite w, Z)."""
    batch = len(o.m)
    low = np.tril(np.ones((n, n), dtype=bool))
    for flat, before in ((o.flatA, o.before[0]), (o.flatB, o.before[1])):
        if flat is None:
            continue
        keep = np.ones(flat.shape, dtype=bool)
        for b in range(batch):
            keep[b * o.sM:b * o.sM + o.ld * n].reshape(n, o.ld)[:, :n][low.T] = False
        assert np.array_equal(bits(flat[keep]), bits(before[keep])), what + ": written outside a lower triangle"
    for b in range(batch):
        mb = int(o.m[b]) if o.info[b] == 0 else 0
        assert np.all(np.isnan(o.w[b, mb:])), what + ": w[%d] written behind m = %d" % (b, mb)
        if o.info[b] == 0:
            assert np.all(np.isfinite(o.w[b, :mb])), what
    zb = np.ones(o.flatZ.shape, dtype=bool)
    for b in range(batch):
        mb = int(o.m[b]) if o.info[b] == 0 else 0
        cols = zb[b * o.sZ:b * o.sZ + o.ld * max(o.zcap, 1)].reshape(max(o.zcap, 1), o.ld)
        cols[:mb, :n] = False
    assert np.all(np.isnan(o.flatZ[zb])), what + ": Z written outside columns 0 .. m - 1"


# ------------------------------------------------------------------------------------------------- shared references
_random_cache = {}


def _random(n, problem, batch=5):
    """A seeded random batch of order n and its full LAPACK reference, made once."""
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


_hard_cache = {}


def _hard(n, problem):
    """The hard batch of an order, its references (None where LAPACK refuses B) and the existing entry's outcome."""
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


_full_cache = {}


def _full(lib, n, problem, jobz=1):
    """ek_hip_eigenpairs_batched_device on the hard batch, once."""
    key = (n, problem, jobz)
    if key not in _full_cache:
        cases, _ = _hard(n, problem)
        A = np.stack([c.A for c, _ in cases])
        B = np.stack([c.B for c, _ in cases]) if problem else None
        _full_cache[key] = _batched_device(lib, A, B, jobz)
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
    if n >= 17:
        vl, vu = 0.5 * (ref[0][0][0] + ref[0][0][1]), 0.5 * (ref[0][0][n // 2] + ref[0][0][n // 2 + 1])
        counts = [int(((r[0] > vl) & (r[0] <= vu)).sum()) for r in ref]
        o = _window_device(lib, A, B, 0, vl=vl, vu=vu)
        assert list(o.m) == counts and len(set(counts)) > 1, (list(o.m), counts)
    print("n=%d problem=%d share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
          % ((n, problem) + tuple(worst)))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------- hard inputs
def _judge_hard(n, problem, cases, refs, full, o, first_of, what, shares, fails):
    for b, (c, base) in enumerate(cases):
        name = "%s %s" % (what, c.name)
        if o.info[b] != 0 or full.info[b] != 0:
            if o.info[b] != 0 and c.spd and not (c.ka == 600 and c.kb == -600):
                fails.append("%s: info = %d where 0 is required (the input has a solution)" % (name, o.info[b]))
            if o.info[b] != full.info[b]:
                fails.append("%s: info = %d, ek_hip_eigenpairs_batched_device says %d" % (name, o.info[b], full.info[b]))
            if o.info[b] != 0 and o.m[b] != 0:
                fails.append("%s: info = %d with m = %d" % (name, o.info[b], o.m[b]))
            continue
        w_ref, Z_ref = refs[base.name]
        if w_ref is None:
            continue                                # B not numerically SPD and yet factorised: the existing entry agreed
        first, m = first_of(b)
        if o.m[b] != m:
            fails.append("%s: m = %d, not %d" % (name, o.m[b], m))
            continue
        k = c.ka - c.kb
        with np.errstate(all="ignore"):
            w0 = np.ldexp(o.w[b, :m], -k)
            Z0 = np.ldexp(o.Z[b][:, :m], c.kb // 2)
        s, f = wc.judge(base.A, base.B, c.cond_b, w_ref, Z_ref, first, w0, Z0, name)
        fails += f
        if s:
            cur = shares.setdefault(c.family, [0.0, 0.0, 0.0])
            shares[c.family] = [max(x, y or 0.0) for x, y in zip(cur, s)]


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [n for n in ORDERS if n >= 3])
def test_hard_cases_in_one_batch(hip, n, problem):
    """Every case of the table at one order in one launch per window, held to the rules of window_batched_cases.judge on
    the window's columns; the clustered classes again, each with the window that cuts its clusters."""
    lib = hip.load_library()
    cases, refs = _hard(n, problem)
    full = _full(lib, n, problem)
    A = np.stack([c.A for c, _ in cases])
    B = np.stack([c.B for c, _ in cases]) if problem else None
    shares, fails = {}, []
    for wname, il, iu in wc.windows(n):
        o = _window_device(lib, A, B, 1, il=il, iu=iu)
        assert o.rc == 0, o.rc
        what = "n=%d problem=%d %s" % (n, problem, wname)
        _judge_hard(n, problem, cases, refs, full, o, lambda b: (il - 1, iu - il + 1), what, shares, fails)
        assert not np.any(o.info >= 200000), (what, o.info)
        if wname == "whole":                        # the existing entry's w, to the bound
            for b, (c, base) in enumerate(cases):
                if o.info[b] == 0 and full.info[b] == 0:
                    lim = 4 * max(n, 8) * EPS * np.abs(full.w[b]).max()
                    if c.cond_b is None and not np.abs(o.w[b] - full.w[b]).max() <= lim:
                        fails.append("%s %s: w differs from the existing entry's by more than the bound" % (what, c.name))
    if not problem:
        for b, (c, base) in enumerate(cases):
            if c.name not in wc.CLUSTERED:
                continue
            cut = wc.cluster_cut(refs[base.name][0])
            if cut is None:
                continue
            o = _window_device(lib, A[b:b + 1], None, 1, il=cut[0], iu=cut[1])
            assert o.rc == 0, o.rc
            _judge_hard(n, problem, cases[b:b + 1], refs, _one(full, b), o, lambda _: (cut[0] - 1, cut[1] - cut[0] + 1),
                        "n=%d cluster cut %d..%d" % ((n,) + cut), shares, fails)
    for fam in sorted(shares):
        print("n=%d problem=%d | %-28s share of the bound used: eigenvalues %.3f residual %.3f orthogonality %.3f"
              % ((n, problem, fam) + tuple(shares[fam])))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:60])


def _one(full, b):
    o = _Out()
    o.info, o.w = full.info[b:b + 1], full.w[b:b + 1]
    return o


@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [17, 64, 128])
def test_hard_cases_by_value_and_values_only(hip, n, problem):
    """The unscaled table under 'V' (bounds from each window of a case that has the gaps; the counts differ from case to
    case) and with jobz = 0: the counts are LAPACK's, and the values are those of the index form, bit for bit."""
    lib = hip.load_library()
    cases, refs = _hard(n, problem)
    # a stated cond(B) is left out: its eigenvalues are known to 4 n eps cond(B), which is wider than the gap that keeps
    # a count unambiguous
    keep = [b for b, (c, base) in enumerate(cases) if c.ka == 0 and c.kb == 0 and c.cond_b is None]
    lead = "band5_band5" if problem else "toeplitz121"              # the bounds come from a spectrum with gaps
    keep.sort(key=lambda b: cases[b][0].name != lead)
    A = np.stack([cases[b][0].A for b in keep])
    B = np.stack([cases[b][0].B for b in keep]) if problem else None
    spectra = [refs[cases[b][1].name][0] for b in keep]
    whole = _window_device(lib, A, B, 0, il=1, iu=n)
    assert whole.rc == 0 and not whole.info.any()
    for wname, il, iu in wc.windows(n):
        vl, vu, span = wc.value_bounds(spectra, il, iu)
        for jobz in (0, 1):
            o = _window_device(lib, A, B, jobz, vl=vl, vu=vu)
            assert o.rc == 0 and not o.info.any(), (wname, o.info)
            for i, (first, m) in enumerate(span):
                assert o.m[i] == m, (wname, cases[keep[i]][0].name, o.m[i], m)
                assert np.array_equal(bits(o.w[i, :m]), bits(whole.w[i, first:first + m])), (wname, cases[keep[i]][0].name)


# -------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("problem", [0, 1])
@pytest.mark.parametrize("n", [3, 33, 100, 128])
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
@pytest.mark.parametrize("n", [17, 128])
def test_same_bits_alone_in_any_batch_across_a_seam_and_in_both_forms(hip, n, problem):
    """One pair alone, at positions 0, 7 and last of batches of 8 and 300 (the rest filled with other pairs), with a chunk
    of 5 problems per launch (seams in front of position 7 and all over the batch of 300), and through the host entry:
    m, info, w and Z are the same bits, and so are the images left in dA and dB -- which are those
    ek_hip_eigenpairs_batched_device leaves."""
    lib = hip.load_library()
    A, B, _ = _random(n, problem)
    il, iu = n // 4 + 1, max(n // 4 + 1, n // 2)
    m = iu - il + 1
    alone = _window_device(lib, A[:1], None if B is None else B[:1], 1, il=il, iu=iu)
    assert alone.rc == 0 and alone.info[0] == 0 and alone.m[0] == m
    full = _batched_device(lib, A[:1], None if B is None else B[:1], 1)
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(bits(alone.A[0][low]), bits(full.A[0][low])), "dA is not the existing entry's image"
    if problem:
        assert np.array_equal(bits(alone.B[0][low]), bits(full.B[0][low])), "dB is not the existing entry's image"
    lim = 4 * max(n, 8) * EPS * np.abs(full.w[0]).max()
    assert np.abs(alone.w[0, :m] - full.w[0, il - 1:iu]).max() <= lim

    def same(o, b, what):
        assert o.rc == 0 and o.info[b] == 0 and o.m[b] == m, what
        assert np.array_equal(bits(o.w[b, :m]), bits(alone.w[0, :m])), what + ": w"
        assert np.array_equal(bits(o.Z[b][:, :m]), bits(alone.Z[0][:, :m])), what + ": Z"
        assert np.array_equal(bits(o.A[b][low]), bits(alone.A[0][low])), what + ": dA"
        if problem:
            assert np.array_equal(bits(o.B[b][low]), bits(alone.B[0][low])), what + ": dB"

    for batch in (8, 300):
        for chunk in (0, 5):
            idx = np.arange(batch) % (A.shape[0] - 1) + 1
            for pos in (0, 7, batch - 1):
                idx[pos] = 0
            before = hip.window_batched_chunk(chunk)
            try:
                o = _window_device(lib, A[idx], None if B is None else B[idx], 1, il=il, iu=iu, pad=1, gap=2)
            finally:
                hip.window_batched_chunk(before)
            for pos in (0, 7, batch - 1):
                same(o, pos, "batch %d chunk %d position %d" % (batch, chunk, pos))
    w, Z, mm, info = hip.eigenpairs_window_batched(A[:2], None if B is None else B[:2], il=il, iu=iu)
    assert info[0] == 0 and mm[0] == m
    assert np.array_equal(bits(w[0, :m]), bits(alone.w[0, :m])), "host form: w"
    assert np.array_equal(bits(Z[0][:, :m]), bits(alone.Z[0][:, :m])), "host form: Z"
    assert not w[0, m:].any(), "host form: w written behind m"


# --------------------------------------------------------------------------------------------------------- own slots
@pytest.mark.parametrize("n", [17, 100])
def test_failures_keep_to_their_own_slots(hip, n):
    """A non-SPD B, a NaN in A, a 'V' window wider than zcap and an empty window planted in one batch: each gets its code
    and its m, writes nothing of w or Z, and its neighbours keep the bits they have without the planted problems."""
    lib = hip.load_library()
    A, B, ref = _random(n, 1, batch=5)
    idx = np.arange(9) % 5
    A9, B9 = A[idx].copy(), B[idx].copy()
    w0 = ref[0][0]
    vl, vu = 0.5 * (w0[n // 4 - 1] + w0[n // 4]), 0.5 * (w0[n // 2 - 1] + w0[n // 2])
    zcap = max(int(((r[0] > vl) & (r[0] <= vu)).sum()) for r in ref) + 1
    clean = _window_device(lib, A9, B9, 1, vl=vl, vu=vu, zcap=zcap)
    assert clean.rc == 0 and not clean.info.any() and clean.m.min() > 0
    B9[1] = B9[1] - 3.0 * np.eye(n)                 # not SPD
    A9[3, n // 2, 0] = np.nan                       # lower triangle
    A9[5] = 1e-6 * A9[5] + 0.5 * (vl + vu) * B9[5]  # every eigenvalue in the middle of (vl, vu]: wider than zcap
    A9[7] = A9[7] + 100.0 * B9[7]                   # the spectrum moves up by 100: an empty window
    assert ((sl.eigh(A9[5], B9[5], eigvals_only=True) > vl) & (sl.eigh(A9[5], B9[5], eigvals_only=True) <= vu)).sum() > zcap
    o = _window_device(lib, A9, B9, 1, vl=vl, vu=vu, zcap=zcap)
    assert o.rc == 0
    assert o.info[1] > 0 and o.m[1] == 0
    assert o.info[3] == -5 and o.m[3] == 0
    assert o.info[5] == -20 and o.m[5] > zcap
    assert o.m[5] == ((sl.eigh(A9[5], B9[5], eigvals_only=True) > vl) & (sl.eigh(A9[5], B9[5], eigvals_only=True) <= vu)).sum()
    assert o.info[7] == 0 and o.m[7] == 0
    for b in (1, 3, 5, 7):
        assert np.all(np.isnan(o.w[b])) and np.all(np.isnan(o.Z[b])), b
    _untouched(o, n, "planted")
    for b in (0, 2, 4, 6, 8):
        assert o.info[b] == 0 and o.m[b] == clean.m[b]
        assert np.array_equal(bits(o.w[b, :o.m[b]]), bits(clean.w[b, :o.m[b]])), b
        assert np.array_equal(bits(o.Z[b][:, :o.m[b]]), bits(clean.Z[b][:, :o.m[b]])), b


# ------------------------------------------------------------------------------------------------------------- speed
def _speed(lib, n, batch):
    """Device seconds, best of 3, the kinds alternated in one process, inputs refreshed outside the clock (every call
    works in place): the existing entry with and without vectors, a window of n / 8 pairs with vectors, all n values."""
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
            return lib.ek_hip_eigenpairs_batched_device(1, jobz, n, batch, dA, n, n * n, dB, n, n * n, dw,
                                                        dZ if jobz else None, n, n * n, ipp, ctypes.byref(sec))

        def window(jobz, iu):
            return lib.ek_hip_eigenpairs_window_batched_device(1, jobz, 0, n, batch, 0.0, 0.0, 1, iu, dA, n, n * n, dB, n,
                                                               n * n, mp, dw, dZ if jobz else None, n, n, n * n, ipp,
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


@pytest.mark.parametrize("n,batch", [(128, 512), (64, 1024)])
def test_a_window_costs_at_most_six_tenths_of_the_full_call(hip, n, batch):
    lib = hip.load_library()
    t = _speed(lib, n, batch)
    r1, r0 = t["window"] / t["full1"], t["values"] / t["full0"]
    print("n=%d batch=%d ms: full with vectors %.3f, window of n/8 with vectors %.3f (%.3f); full values %.3f, all values "
          "by bisection %.3f (%.3f)" % (n, batch, 1e3 * t["full1"], 1e3 * t["window"], r1, 1e3 * t["full0"],
                                        1e3 * t["values"], r0))
    assert r1 <= 0.6, r1
    assert r0 <= 0.6, r0
