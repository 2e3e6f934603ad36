"""Bit identity of the batched solver with the build before its two kernels took block_reduce, stage 0 and the rank sort
from ek_batched_stages.h: tests/golden/batched_digests.txt holds one sha256 per call, written by
tools/batched_digests.py on a build of that parent commit, and every one must be reproduced.  Stage 3 and the QL loop
still stand in both kernels; the digests are what a later attempt to share them has to keep.

A digest covers the returned info and the whole allocations of w, Z, A and B as they come back.  Leading dimensions are
n + 1 and a problem's stride is padded, with NaN in everything that is not a problem's own, so a store outside a problem
changes a digest too.  Inputs are seeded by name (batched_cases.rng); a uniform call holds three problems.  The cases are
the smallest at which each block that the kernels have in common (the scan of A, DSYTD2, QL with its flip and its
underflow split, the rank sort, the strided axpy and dot) can go wrong:
  orders 1, 2, 3, 31, 33, 64, 65, 128 (ek_hip_eigenpairs_batched_device, ek_hip_sygv_batched_device) and 129, 200, 256 (the
      xbatched entries): problem 0 with and without vectors, type 1 with and without, types 2 and 3 with vectors
  orders 33, 128, 200, from batched_cases: tridiagonal inputs (every tau = 0 exit), graded ones that take the flip, and A
      times 2^664 and 2^-664 (the scaling of stage 0), standard and generalized
  orders 65 and 200: a good pair between a NaN in A (info -5), a B whose pivot fails at column 2 and a pencil whose
      eigenvalues overflow; the failed problems' w and Z come back as they were
  one variable call over orders 0, 1, 31, 64, 65, 128, 129, 256, for problem 0 and for type 3"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import batched_cases as bc
import test_gpu_xvbatched as xv
from test_gpu_vbatched import _Dev, _spd, _sym, _view

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batched_digests.txt")
_ip = ctypes.POINTER(ctypes.c_int)
SMALL, LARGE = (1, 2, 3, 31, 33, 64, 65, 128), (129, 200, 256)
HARD_ORDERS = (33, 128, 200)
FAIL_ORDERS = (65, 200)
XV_ORDERS = (0, 1, 31, 64, 65, 128, 129, 256)
# (tag, entry family, first argument, jobz)
KINDS = [("standard", "eigenpairs", 0, 1), ("standard values", "eigenpairs", 0, 0), ("type1", "eigenpairs", 1, 1),
         ("type1 values", "eigenpairs", 1, 0), ("type2", "sygv", 2, 1), ("type3", "sygv", 3, 1)]


def _pack(mats, n, ld, stride):
    flat = np.full(len(mats) * stride, np.nan)
    _view(flat, len(mats), n, ld, stride)[...] = np.stack(mats).transpose(0, 2, 1)
    return flat


def _uniform(lib, family, first, jobz, pairs):
    """One uniform call on the pairs (B is None: the standard problem), ld = n + 1, stride = ld n + 3, two words behind
    the last w; the entry for orders up to 256 above order 128.  Returns info and the allocations of w, Z, A, B after."""
    n, batch = pairs[0][0].shape[0], len(pairs)
    withB = family == "sygv" or first == 1
    ld, stride = n + 1, (n + 1) * n + 3
    hA = _pack([A for A, _ in pairs], n, ld, stride)
    hB = _pack([B for _, B in pairs], n, ld, stride) if withB else np.full(1, np.nan)
    hZ, hw = np.full(batch * stride, np.nan), np.full(batch * n + 2, np.nan)
    info = np.full(batch, 777, dtype=np.int32)
    fn = getattr(lib, "ek_hip_%s_%sbatched_device" % (family, "x" if n > 128 else ""))
    with _Dev(lib) as dev:
        dA, dB, dw, dZ = dev.up(hA), dev.up(hB), dev.up(hw), dev.up(hZ)
        rc = fn(first, jobz, n, batch, dA, ld, stride, dB if withB else None, ld, stride, dw, dZ if jobz else None, ld,
                stride, info.ctypes.data_as(_ip), None)
        assert rc == 0, rc
        return info, dev.down(dw, hw), dev.down(dZ, hZ), dev.down(dA, hA), dev.down(dB, hB)


def _sha(info, *flats):
    h = hashlib.sha256(info.tobytes())
    for f in flats:
        if f is not None:
            h.update(np.ascontiguousarray(f).tobytes())
    return h.hexdigest()


def _random_pairs(n):
    rng = bc.rng("digest random n=%d" % n)
    return [(_sym(rng, n), _spd(rng, n)) for _ in range(3)]


def _hard(n):
    """(tag, first, pairs): every tau = 0 exit, the flip, and the two directions of stage 0's scaling."""
    def std(*cases):
        return [(c.A, None) for c in cases]

    band, toe = bc.make("band:half", n), bc.make("toeplitz121", n)
    b5, cb = bc.make("band5_band5", n), bc.make("cond_b:1e6", n)
    pencils = [bc.scaled(b5, 664), bc.scaled(b5, -664), bc.scaled(cb, 664)]
    return [("tridiagonal", 0, std(toe, bc.make("neg:clement", n), bc.make("glued:1e-14", n))),
            ("flip", 0, std(bc.make("graded_down:14", n), bc.make("graded:8", n), bc.make("ends_ulp", n))),
            ("scaled", 0, std(bc.scaled(band, 664), bc.scaled(band, -664), bc.scaled(toe, -664))),
            ("scaled pencils", 1, [(c.A, c.B) for c in pencils])]


def _failing(n):
    """A good pair, a NaN in A, a B whose second pivot is not positive, a pencil whose eigenvalues overflow."""
    rng = bc.rng("digest failing n=%d" % n)
    pairs = [(_sym(rng, n), _spd(rng, n)) for _ in range(3)]
    pairs[1][0][n - 1, 2] = np.nan
    pairs[2][1][1, 1] = -3.0
    c = bc.scaled(bc.make("band5_band5", n), 600, -600)
    return pairs + [(c.A, c.B)]


def digest_cases():
    """(label, thunk): the thunk takes the library and returns (info, flat allocations ...)."""
    out = []
    for n in SMALL + LARGE:
        for tag, family, first, jobz in KINDS:
            out.append(("uniform n=%d %s" % (n, tag),
                        lambda lib, n=n, f=family, a=first, j=jobz: _uniform(lib, f, a, j, _random_pairs(n))))
    for n in HARD_ORDERS:
        for tag, first, pairs in _hard(n):
            out.append(("hard n=%d %s" % (n, tag), lambda lib, a=first, p=pairs: _uniform(lib, "eigenpairs", a, 1, p)))
    for n in FAIL_ORDERS:
        out.append(("failing n=%d" % n, lambda lib, n=n: _uniform(lib, "eigenpairs", 1, 1, _failing(n))))
    for tag, kind, first in (("standard", "eig", 0), ("type3", "sygv", 3)):
        def variable(lib, kind=kind, first=first):
            rng = bc.rng("digest variable")
            pairs = [(_sym(rng, n), _spd(rng, n)) if n else (np.zeros((0, 0)), np.zeros((0, 0))) for n in XV_ORDERS]
            o = xv._xv(lib, pairs, kind, first, 1, pad=1)
            assert o.rc == 0, o.rc
            return o.info, o.wflat, o.Zflat, o.Aflat, o.Bflat
        out.append(("variable %s" % tag, variable))
    return out


def digest_of(lib, case):
    return _sha(*case[1](lib))


def read_digests(path=DIGESTS):
    out = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            label, _, digest = line.rstrip("\n").rpartition("  ")
            out[label] = digest
    return out


def test_every_digest_of_the_parent_is_reproduced(hip):
    lib = hip.load_library()
    want = read_digests()
    cases = digest_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    differ = [c[0] for c in cases if digest_of(lib, c) != want[c[0]]]
    assert not differ, differ


@pytest.mark.parametrize("n", FAIL_ORDERS)
def test_failed_problems_leave_their_slots_alone(hip, n):
    """What the digests of the failing batches stand for: the three kinds of failure are reported as such, and the w and
    Z of a failed problem (and everything between the problems) are still the NaN they were."""
    info, w, Z, _, _ = _uniform(hip.load_library(), "eigenpairs", 1, 1, _failing(n))
    assert info[0] == 0 and info[1] == -5 and info[2] == 2 and info[3] > 100000, info
    ld, stride = n + 1, (n + 1) * n + 3
    assert np.all(np.isfinite(w[:n])) and np.all(np.isnan(w[n:]))
    assert np.all(np.isfinite(_view(Z, 1, n, ld, stride))) and np.all(np.isnan(Z[stride:]))
    gaps = np.ones(stride, dtype=bool)
    _view(gaps, 1, n, ld, stride)[...] = False
    assert np.all(np.isnan(Z[:stride][gaps]))
