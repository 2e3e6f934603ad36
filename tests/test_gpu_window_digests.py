"""Bit identity of the batched window entries with the build before their host side became one driver:
tests/golden/window_digests.txt holds one sha256 per call, written by tools/window_digests.py on a build of that parent
commit, and every one must be reproduced.

A digest covers the returned info and m and the whole allocations of w, Z, A and B as they come back.  Leading dimensions
are n + 1, a problem's stride is padded by 3 and w by 2 words (the variable call: a gap of 3 words behind every piece), with
NaN in everything that is not a problem's own, so a store outside a problem changes a digest too.  Every case runs in the
device-pointer form and in the host-pointer form ("<label> host": what comes back in the caller's arrays).  Inputs are
seeded by name (batched_cases.rng).  The cases are the smallest that reach every branch of the host driver:
  uniform  orders 3, 33, 65, 128 (the window_batched entries) and 129, 200 (window_xbatched): five problems with both chunk
           hooks at 2, so three launches at offsets 0, 2, 4; the index window 2 .. n - 1 (1 .. 1 at order 3, a spare
           column in Z) and a value window that contains the middle third of every spectrum (zcap = n); with and without
           vectors; the standard problem (eigenpairs entry) and types 1 and 3 (sygv entry)
  variable one call over orders 0, 1, 31, 64, 65, 128, 129, 256, 33, 200 with a window per problem, by index and by value,
           the standard problem and type 3: under the default budget with a stream per class, with a budget of one byte
           (a problem per launch) and on one stream -- the three must give the same line
  failing  one batch of order 65, type 1, by value: a good pair, a NaN in A (info -5), a B whose second pivot fails
           (info 2) and a pair with more eigenvalues in the window than zcap columns (info -20, m the count)
A value window's edges are the LAPACK eigenvalues rounded outwards to eighths, so they do not move with LAPACK's last bits."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import scipy.linalg as sl

import batched_cases as bc
from test_gpu_vbatched import _Dev, _spd, _sym, _view

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_digests.txt")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
UNIFORM_ORDERS = (3, 33, 65, 128, 129, 200)
XV_ORDERS = (0, 1, 31, 64, 65, 128, 129, 256, 33, 200)
# (tag, entry family, first argument, type of the pencil for the reference: 0 the standard problem)
KINDS = [("standard", "eigenpairs", 0, 0), ("type1", "sygv", 1, 1), ("type3", "sygv", 3, 3)]
# (tag, ek_hip_debug_window_xvbatched_budget, ek_hip_debug_vbatched_streams)
WAYS = [("default", 0, 3), ("a problem per launch", 1, 3), ("one stream", 0, 1)]
_made = {}                                              # inputs and windows, made once and never modified


def _spectrum(A, B, itype):
    return sl.eigvalsh(A, B, type=itype) if itype else sl.eigvalsh(A)


def _middle(spectra):
    """(vl, vu] around the middle third of every spectrum, on eighths."""
    lo = min(w[len(w) // 3] for w in spectra)
    hi = max(w[min(len(w) - 1, 2 * len(w) // 3)] for w in spectra)
    return float(np.floor(lo * 8.0) / 8.0 - 0.125), float(np.ceil(hi * 8.0) / 8.0 + 0.125)


def _index(n):
    il = 2 if n >= 3 else 1
    return il, max(il, n - 1)


def _pairs(tag, orders):
    if (tag, orders) not in _made:
        rng = bc.rng("window digest %s" % tag)
        _made[(tag, orders)] = [(_sym(rng, n), _spd(rng, n)) for n in orders]
    return _made[(tag, orders)]


def _hooks(lib, chunk=0, budget=0, streams=3):
    lib.ek_hip_debug_window_batched_chunk(chunk)
    lib.ek_hip_debug_window_xbatched_chunk(chunk)
    lib.ek_hip_debug_window_xvbatched_budget(budget)
    lib.ek_hip_debug_vbatched_streams(streams)


def _pack(mats, n, ld, stride):
    flat = np.full(len(mats) * stride, np.nan)
    _view(flat, len(mats), n, ld, stride)[...] = np.stack(mats).transpose(0, 2, 1)
    return flat


def _uniform(lib, host, family, first, jobz, pairs, window, zcap, chunk):
    """One uniform call; window: (il, iu) or (vl, vu) as floats.  Returns info, m and the allocations of w, Z, A, B."""
    n, batch = pairs[0][0].shape[0], len(pairs)
    withB = family == "sygv" or first == 1
    by_value = isinstance(window[0], float)
    ld = n + 1
    sM, sZ = ld * n + 3, ld * max(zcap, 1) + 3
    hA = _pack([A for A, _ in pairs], n, ld, sM)
    hB = _pack([B for _, B in pairs], n, ld, sM) if withB else np.full(1, np.nan)
    hZ, hw = np.full(batch * sZ, np.nan), np.full(batch * n + 2, np.nan)
    info, m = np.full(batch, 777, dtype=np.int32), np.full(batch, 777, dtype=np.int32)
    vl, vu = window if by_value else (0.0, 0.0)
    il, iu = (0, 0) if by_value else window
    fn = getattr(lib, "ek_hip_%s_window_%sbatched%s" % (family, "x" if n > 128 else "", "" if host else "_device"))

    def call(pA, pB, pw, pZ):
        rc = fn(first, jobz, 1 if by_value else 0, n, batch, vl, vu, il, iu, pA, ld, sM, pB if withB else None, ld, sM,
                m.ctypes.data_as(_ip), pw, pZ if jobz else None, ld, zcap, sZ, info.ctypes.data_as(_ip), None)
        assert rc == 0, rc

    try:
        _hooks(lib, chunk=chunk)
        if host:
            call(*(x.ctypes.data_as(_dp) for x in (hA, hB, hw, hZ)))
            return info, m, hw, hZ, hA, hB
        with _Dev(lib) as dev:
            dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
            call(dA, dB, dw, dZ)
            return info, m, dev.down(dw, hw), dev.down(dZ, hZ), dev.down(dA, hA), dev.down(dB, hB)
    finally:
        _hooks(lib)


def _variable(lib, host, family, first, jobz, pairs, windows, zcaps, budget=0, streams=3):
    """One variable call on an arena per array kind, ld = n + 1 and three words behind every piece."""
    batch = len(pairs)
    withB = family == "sygv" or first == 1
    by_value = isinstance(windows[0][0], float)
    n = np.array([A.shape[0] for A, _ in pairs], dtype=np.int32)
    ld = (n + 1).astype(np.int32)
    zcap = np.array(zcaps, dtype=np.int32)
    lo = np.array([w[0] for w in windows], dtype=np.float64 if by_value else np.int32)
    hi = np.array([w[1] for w in windows], dtype=np.float64 if by_value else np.int32)
    offm = np.concatenate([[0], np.cumsum(ld.astype(np.int64) * n + 3)])
    offw = np.concatenate([[0], np.cumsum(n.astype(np.int64) + 3)])
    offz = np.concatenate([[0], np.cumsum(ld.astype(np.int64) * np.maximum(zcap, 1) + 3)])
    hA, hB = np.full(offm[-1], np.nan), np.full(offm[-1] if withB else 1, np.nan)
    hw, hZ = np.full(offw[-1], np.nan), np.full(offz[-1], np.nan)
    for b, (A, B) in enumerate(pairs):
        for flat, M in ((hA, A), (hB, B)) if withB else ((hA, A),):
            flat[offm[b]:offm[b] + ld[b] * n[b]].reshape(n[b], ld[b])[:, :n[b]] = M.T
    info, m = np.full(batch, 777, dtype=np.int32), np.full(batch, 777, dtype=np.int32)
    fn = getattr(lib, "ek_hip_%s_window_xvbatched%s" % (family, "" if host else "_device"))

    def table(base, off):
        return (ctypes.c_void_p * batch)(*[base + int(off[b]) * 8 for b in range(batch)])

    def call(pA, pB, pw, pZ):
        I = lambda a: a.ctypes.data_as(_ip)             # noqa: E731
        D = lambda a: a.ctypes.data_as(_dp)             # noqa: E731
        rc = fn(first, jobz, 1 if by_value else 0, batch, I(n), D(lo) if by_value else None, D(hi) if by_value else None,
                None if by_value else I(lo), None if by_value else I(hi), table(pA, offm), I(ld),
                table(pB, offm) if withB else None, I(ld), I(m), table(pw, offw), table(pZ, offz) if jobz else None, I(ld),
                I(zcap), I(info), None)
        assert rc == 0, rc

    try:
        _hooks(lib, budget=budget, streams=streams)
        if host:
            call(hA.ctypes.data, hB.ctypes.data, hw.ctypes.data, hZ.ctypes.data)
            return info, m, hw, hZ, hA, hB
        with _Dev(lib) as dev:
            dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
            call(dA.value, dB.value, dw.value, dZ.value)
            return info, m, dev.down(dw, hw), dev.down(dZ, hZ), dev.down(dA, hA), dev.down(dB, hB)
    finally:
        _hooks(lib)


def _failing():
    """(pairs, window, zcap): good, NaN in A, second pivot of B not positive, more eigenvalues in the window than zcap."""
    if "failing" not in _made:
        n = 65
        rng = bc.rng("window digest failing")
        pairs = [(_sym(rng, n), _spd(rng, n)) for _ in range(4)]
        window = _middle([_spectrum(*pairs[0], 1)])
        zcap = int(((_spectrum(*pairs[0], 1) > window[0]) & (_spectrum(*pairs[0], 1) <= window[1])).sum())
        pairs[1][0][n - 1, 2] = np.nan
        pairs[2][1][1, 1] = -3.0
        pairs[3] = (pairs[3][0] * 2.0 ** -10, pairs[3][1])   # the whole spectrum inside the window
        assert 0 < zcap < n
        _made["failing"] = (pairs, window, zcap)
    return _made["failing"]


def digest_cases():
    """(label, variable, thunk): thunk(lib, host, **way) returns (info, m, flat allocations ...); way: budget, streams, for
    the variable cases only."""
    out = []
    for n in UNIFORM_ORDERS:
        pairs = _pairs("uniform n=%d" % n, (n,) * 5)
        for tag, family, first, itype in KINDS:
            by_value = _middle([_spectrum(A, B, itype) for A, B in pairs])
            for wtag, window, zcap in (("index", _index(n), _index(n)[1] - _index(n)[0] + 2), ("value", by_value, n)):
                for jobz in (1, 0):
                    out.append(("uniform n=%d %s %s%s" % (n, tag, wtag, "" if jobz else " values"), False,
                                lambda lib, host, f=family, a=first, j=jobz, p=pairs, w=window, z=zcap:
                                _uniform(lib, host, f, a, j, p, w, z, 2)))
    pairs = [p if p[0].shape[0] else (np.zeros((0, 0)), np.zeros((0, 0))) for p in _pairs("variable", XV_ORDERS)]
    for tag, family, first, itype in (KINDS[0], KINDS[2]):
        index = [_index(n) if n else (0, 0) for n in XV_ORDERS]
        value = [_middle([_spectrum(A, B, itype)]) if A.shape[0] else (0.0, 1.0) for A, B in pairs]
        for wtag, windows, zcaps in (("index", index, [iu - il + 1 + b % 2 for b, (il, iu) in enumerate(index)]),
                                     ("value", value, list(XV_ORDERS))):
            out.append(("variable %s %s" % (tag, wtag), True,
                        lambda lib, host, f=family, a=first, w=windows, z=zcaps, **way:
                        _variable(lib, host, f, a, 1, pairs, w, z, **way)))
    out.append(("failing n=65", False,
                lambda lib, host: _uniform(lib, host, "sygv", 1, 1, _failing()[0], _failing()[1], _failing()[2], 0)))
    return out


def digest_of(lib, case, host=False, **way):
    info, m, *flats = case[2](lib, host, **way)
    h = hashlib.sha256(info.tobytes() + m.tobytes())
    for f in flats:
        h.update(np.ascontiguousarray(f).tobytes())
    return h.hexdigest()


def read_digests(path=DIGESTS):
    out = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            label, _, digest = line.rstrip("\n").rpartition("  ")
            out[label] = digest
    return out


def test_every_window_digest_of_the_parent_is_reproduced(hip):
    lib = hip.load_library()
    want = read_digests()
    cases = digest_cases()
    assert sorted(want) == sorted([c[0] for c in cases] + [c[0] + " host" for c in cases])
    differ = [c[0] + tail for c in cases for host, tail in ((False, ""), (True, " host"))
              if digest_of(lib, c, host) != want[c[0] + tail]]
    assert not differ, differ


def test_a_variable_call_gives_one_line_however_it_is_launched(hip):
    """The default budget on a stream per class, a problem per launch, and one stream: the fixture's line three times."""
    lib = hip.load_library()
    want = read_digests()
    for case in digest_cases():
        if case[1]:
            got = [digest_of(lib, case, budget=budget, streams=streams) for _, budget, streams in WAYS]
            assert got == [want[case[0]]] * len(WAYS), (case[0], got)


def test_what_the_failing_batch_reports(hip):
    """What the digest of the failing batch stands for: each failure in its own slot, and a failed problem's w and Z (and
    everything between the problems) still the NaN they were."""
    pairs, window, zcap = _failing()
    n, ld = 65, 66
    info, m, w, Z, _, _ = _uniform(hip.load_library(), False, "sygv", 1, 1, pairs, window, zcap, 0)
    assert list(info) == [0, -5, 2, -20] and m[0] == zcap and m[1] == 0 and m[2] == 0 and m[3] == n, (info, m)
    assert np.all(np.isfinite(w[:zcap])) and np.all(np.isnan(w[zcap:]))
    sZ = ld * zcap + 3
    assert np.all(np.isfinite(Z[:sZ - 3].reshape(zcap, ld)[:, :n])) and np.all(np.isnan(Z[:sZ - 3].reshape(zcap, ld)[:, n:]))
    assert np.all(np.isnan(Z[sZ - 3:]))
