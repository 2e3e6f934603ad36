"""Bit identity of the batched checks that run on the matrix cores (the full checks above order 128 and the window checks
of every order) with the build before their four units took their tiles, loaders, products and kernel bodies from
ek_batched_check_x.h: tests/golden/check_digests.txt holds one sha256 per call, written by
tools/check_digests.py on a build of that parent commit, and every one must be reproduced.  The file is never
regenerated from the tree under test.

A digest covers the whole allocations of out and ipr as they come back.  They start as NaN, so every word that is not a
problem's own output (behind the last problem, an IPR row from m[b] on, the row of a skipped problem) is in the digest as
the NaN it was.  Inputs are seeded by name (batched_cases.rng); leading dimensions, zcap and a problem's stride are padded,
the padding holds NaN.  A uniform call holds three problems and takes the device form unless its label says host.  The
cases are the smallest at which each shared piece can go wrong:
  full      n = 129 (one ragged strip in the second row tile), 145 (the strip edge 128 + 16 + 1), 200, 256 (no ragged
            edge): problem 0 and 1, itype 2 and 3, each with and without ipr
  window    n = 1, 17, 64, 65, 129, 256 with every m of 1, 16, 17, 48, 49, 64, 65, 128, 129, n that fits, three a call:
            nsub 1 .. 4, the second column tile, the second row tile of the Gram pass, every class of type 3's factor split
            (n <= 64, <= 128, above) and of its solve split (c <= 16, 32, 64, 128, above); one call per kind with an m = 0
            problem and a skipped problem between live ones
  host      one call per kernel class
  pivot     type 3, full and window, n = 129: a B whose pivot fails at column 2 between two good pencils
  table     the variable entries over the orders 0, 1, 64, 65, 129, 256 (the window entries twice over them, with other m,
            zeros among them); orders up to 128 of the two full entries run the kernels of the classes below"""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import batched_cases as bc
from test_gpu_vbatched import _Dev, _spd, _sym

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "check_digests.txt")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
FULL_ORDERS = (129, 145, 200, 256)
WINDOW_ORDERS = (1, 17, 64, 65, 129, 256)
COLUMNS = (1, 16, 17, 48, 49, 64, 65, 128, 129)
TABLE_ORDERS = (0, 1, 64, 65, 129, 256)
TABLE_M = ((0, 1, 48, 65, 129, 256), (0, 0, 16, 17, 64, 128))
KINDS = (0, 1, 2, 3)                                # problem 0, problem 1, itype 2, itype 3
GROUPS = ("full", "window", "edge", "table")


@functools.lru_cache(maxsize=None)
def _problems(n, count=3, bad=-1):
    """`count` problems (A, B, w, Z) of order n, read only; bad: the problem whose B fails at the second pivot."""
    rng = bc.rng("check digest n=%d" % n)
    out = []
    for b in range(count):
        A, B = _sym(rng, n), _spd(rng, n)
        w, Z = rng.standard_normal(n), rng.standard_normal((n, n))
        if b == bad:
            B[1, 1] = -3.0
        out.append((A, B, w, Z))
    return out


def _image(M, ld, cols):
    """An n x cols matrix as a column-major image with leading dimension ld and two words behind it, NaN in the padding."""
    flat = np.full(ld * cols + 2, np.nan)
    flat[:ld * cols].reshape(cols, ld)[:M.shape[1], :M.shape[0]] = M.T
    return flat


def _entry(lib, kind, window, variable, host):
    name = "ek_hip_check_%s%sx%sbatched%s" % ("sygv_" if kind > 1 else "", "window_" if window else "",
                                               "v" if variable else "", "" if host else "_device")
    return getattr(lib, name)


def _uniform(lib, kind, n, m=None, ipr=True, host=False, info=None, bad=-1):
    """One uniform call on the problems of order n (as many as m has, three without m); m: the window entry.  Returns the
    allocations of out and ipr."""
    batch = 3 if m is None else len(m)
    probs = _problems(n, batch, bad)
    lda, ldb, ldz = n + 1, n + 2, n + 3
    zcap = n if m is None else max(m) + 1
    hA = np.concatenate([_image(p[0], lda, n) for p in probs])
    hB = np.concatenate([_image(p[1], ldb, n) for p in probs])
    hZ = np.concatenate([_image(p[3][:, :(n if m is None else m[b])], ldz, zcap) for b, p in enumerate(probs)])
    hw = np.full(batch * n, np.nan)
    for b, p in enumerate(probs):
        k = n if m is None else m[b]
        hw[b * n:b * n + k] = p[2][:k]
    out, q = np.full(batch * 4 + 2, np.nan), np.full(batch * n + 3, np.nan)
    iarr = None if info is None else np.asarray(info, dtype=np.int32)
    marr = None if m is None else np.asarray(m, dtype=np.int32)
    fn = _entry(lib, kind, m is not None, False, host)

    def call(A, B, w, Z):
        head = (kind, n, batch, A, lda, lda * n + 2, B if kind else None, ldb, ldb * n + 2)
        mid = (w, Z, ldz) if m is None else (marr.ctypes.data_as(_ip), w, Z, ldz, zcap)
        return fn(*head, *mid, ldz * zcap + 2, None if iarr is None else iarr.ctypes.data_as(_ip),
                  out.ctypes.data_as(_dp), q.ctypes.data_as(_dp) if ipr else None, None)

    if host:
        rc = call(*[x.ctypes.data_as(_dp) for x in (hA, hB, hw, hZ)])
    else:
        with _Dev(lib) as dev:
            rc = call(*[dev.up(x) for x in (hA, hB, hw, hZ)])
    assert rc == 0, rc
    return out, q


def _table(lib, kind, window):
    """One variable call, device form: the full entries over TABLE_ORDERS, the window entries twice over them with the
    columns of TABLE_M; problem 3 of the second round is skipped."""
    rounds = TABLE_M if window else (TABLE_ORDERS,)
    n = np.array(TABLE_ORDERS * len(rounds), dtype=np.int32)
    m = np.array([c for r in rounds for c in r], dtype=np.int32)
    batch = len(n)
    probs = [_problems(int(k), 2)[b // len(TABLE_ORDERS)] if k else None for b, k in enumerate(n)]
    lda, ldb, ldz = (np.maximum(n + x, 1).astype(np.int32) for x in (1, 2, 3))
    zcap = (m + 1).astype(np.int32)
    info = np.zeros(batch, dtype=np.int32)
    if window:
        info[len(TABLE_ORDERS) + 3] = 5
    out = np.full(batch * 4 + 2, np.nan)
    q = [np.full(int(k) + 2, np.nan) for k in n]
    qt = (ctypes.c_void_p * batch)(*[x.ctypes.data for x in q])
    I = lambda a: a.ctypes.data_as(_ip)                 # noqa: E731
    with _Dev(lib) as dev:
        def table(images):
            return (ctypes.c_void_p * batch)(*[dev.up(x).value if x is not None else None for x in images])

        tA = table([p and _image(p[0], lda[b], n[b]) for b, p in enumerate(probs)])
        tB = table([p and _image(p[1], ldb[b], n[b]) for b, p in enumerate(probs)]) if kind else None
        tw = table([p and np.concatenate([p[2][:m[b]], np.full(n[b] - m[b] + 1, np.nan)]) for b, p in enumerate(probs)])
        tZ = table([p and _image(p[3][:, :m[b]], ldz[b], zcap[b]) for b, p in enumerate(probs)])
        mid = (I(m), tw, tZ, I(ldz), I(zcap)) if window else (tw, tZ, I(ldz))
        rc = _entry(lib, kind, window, True, False)(kind, batch, I(n), tA, I(lda), tB, I(ldb), *mid, I(info),
                                                    out.ctypes.data_as(_dp), qt, None)
    assert rc == 0, rc
    return [out] + q


def _columns(n):
    """The column counts of order n, three a call (the last call filled up from the front)."""
    cols = sorted(set(min(c, n) for c in COLUMNS + (n,)))
    cols += (cols * 3)[:-len(cols) % 3]
    return [tuple(cols[k:k + 3]) for k in range(0, len(cols), 3)]


def digest_cases():
    """(label, group, thunk): the thunk takes the library and returns the allocations to digest."""
    out = []
    for n in FULL_ORDERS:
        for kind in KINDS:
            for ipr in (True, False):
                out.append(("full n=%d kind=%d%s" % (n, kind, "" if ipr else " no ipr"), "full",
                            lambda lib, n=n, k=kind, i=ipr: _uniform(lib, k, n, ipr=i)))
    for n in WINDOW_ORDERS:
        for kind in KINDS:
            for m in _columns(n):
                out.append(("window n=%d kind=%d m=%d,%d,%d" % ((n, kind) + m), "window",
                            lambda lib, n=n, k=kind, m=m: _uniform(lib, k, n, m)))
    for kind in KINDS:
        out.append(("window n=129 kind=%d empty and skipped" % kind, "edge",
                    lambda lib, k=kind: _uniform(lib, k, 129, (17, 0, 65, 129, 1), info=(0, 0, 0, 1, 0))))
        out.append(("host full n=145 kind=%d" % kind, "edge", lambda lib, k=kind: _uniform(lib, k, 145, host=True)))
        out.append(("host window n=129 kind=%d" % kind, "edge",
                    lambda lib, k=kind: _uniform(lib, k, 129, (17, 65, 129), host=True)))
    out.append(("pivot full n=129", "edge", lambda lib: _uniform(lib, 3, 129, bad=1)))
    out.append(("pivot window n=129", "edge", lambda lib: _uniform(lib, 3, 129, (17, 65, 129), bad=1)))
    for kind in KINDS:
        out.append(("table full kind=%d" % kind, "table", lambda lib, k=kind: _table(lib, k, False)))
        out.append(("table window kind=%d" % kind, "table", lambda lib, k=kind: _table(lib, k, True)))
    return out


def digest_of(lib, case):
    h = hashlib.sha256()
    for f in case[2](lib):
        h.update(np.ascontiguousarray(f).tobytes())
    return h.hexdigest()


def read_digests(path=DIGESTS):
    out = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            label, _, digest = line.rstrip("\n").rpartition("  ")
            out[label] = digest
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_every_digest_of_the_parent_is_reproduced(hip, group):
    lib = hip.load_library()
    want = read_digests()
    cases = digest_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    cases = [c for c in cases if c[1] == group]
    assert cases
    differ = [c[0] for c in cases if digest_of(lib, c) != want[c[0]]]
    assert not differ, differ


def test_the_pivot_case_is_what_it_says(hip):
    """What the two pivot digests stand for: the failed pencil reports NaN in slot 3 and in its IPRs, its residual slots
    stand, and its neighbours are whole."""
    for m in (None, (17, 65, 129)):
        out, q = _uniform(hip.load_library(), 3, 129, m, bad=1)
        out, q = out[:12].reshape(3, 4), q[:3 * 129].reshape(3, 129)
        assert np.all(np.isfinite(out[[0, 2]])) and np.all(np.isfinite(out[1, :3])) and np.isnan(out[1, 3])
        for b, k in enumerate(m or (129,) * 3):
            assert np.all(np.isfinite(q[b, :k]) == (b != 1)) and np.all(np.isnan(q[b, k:]))
