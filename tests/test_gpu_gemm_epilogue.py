"""The epilogue of gemm_small_kernel, gemm_kernel and gemm_kernel_w8 (ek_gemm.hip): C <- alpha acc + beta C in batches.

A whole tile (m0 + T <= M and n0 + T <= N after the `dims` table) takes a path without predicates, an edge tile one with
exact masks; with beta != 0 both fetch their C values a batch at a time (the VEC small kernel: in front of the K loop).
The shapes are the smallest at which these paths differ, one launch each through ek_hip_debug_gemm_desc:

    whole        T x T                                  the fast path alone
    ragged       (T + 1) x (T - 3), odd ldc             column-edge and corner tile
    ragged-2x2   (T + 1) x (T + 5), odd ldc             whole, row-edge, column-edge and corner tile in one launch
    lower-3x2    (2 T + 1) x (T + 5), lower_only        the same four kinds on the compact grid
    batch        2 entries by strideC, dims (T, T, K) and (T - 31, T - 3, K - 3): the decision is taken after `dims`
    lower-2x2    2 T x 2 T, lower_only as launched 2 (one product) and 1 (a batch of 2): the diagonal tiles whole, the
                 upper tile bit for bit what it was

K: 4, 20, 36 (small kernel), 16, 20 (8 waves), 516 (4 waves: K > 512 is what takes beta != 0 there).  The 128-tilings are
reached as tests/gemm_cases.py does: lower_only, or (ragged-2x2) a batch of 64 that brings the tile count to 256.  Every
launch asserts the variant the hook reports: kernel, VEC or scalar (odd lda), lower_only as launched.

The reference is exact, as in test_gpu_gemm.py: operands integers in [-7, 7], C in [-1000, 1000], alpha in {1, -1, 2, -0.5},
beta in {1, -2, 0.5}; C lies inside a NaN-filled allocation that must come back untouched outside the product.  With
beta = 0 C holds NaN and +-Inf beforehand and the result is still exact (gemm() gives the 8-wave kernel no such product:
its shapes then run on the 4-wave kernel, with K = 20).

Bit identity: tests/golden/gemm_epilogue_digests.txt holds the sha256 of C's allocation for one uniform(-1, 1) product
per kernel and transposition (alpha = -1, beta = 1; the shapes above and one of 3 x 3 tiles), written by
tools/gemm_epilogue_digests.py on a build of the commit before the batched epilogue.  Every element is still
fma(beta, c, alpha * acc) over the same K order, so every digest must be reproduced."""
import ctypes
import hashlib
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu

KS = {gc.SMALL: (4, 20, 36), gc.W8: (16, 20), gc.W4: (516,)}
BETAS = (1.0, -2.0, 0.5)
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_epilogue_digests.txt")

Shape = namedtuple("Shape", "name m n batch lower dims odd_ldc share_ab mode")


def shapes(kern, with_3x3=False):
    """The launches of one kernel; T = 64 for the small kernel (lower_only there needs small_tiles), else 128."""
    T = 64 if kern == gc.SMALL else 128
    big = kern != gc.SMALL
    S = [
        Shape("whole", T, T, 1, int(big), False, False, False, 2 if big else 0),
        Shape("ragged", T + 1, T - 3, 1, int(big), False, True, False, 2 if big else 0),
        Shape("ragged-2x2", T + 1, T + 5, 64 if big else 1, 0, False, True, big, 0),
        Shape("lower-3x2", 2 * T + 1, T + 5, 1, 1, False, False, False, 2),
        Shape("batch", T, T, 2, int(big), True, False, False, 1 if big else 0),
        Shape("lower-2x2-mode2", 2 * T, 2 * T, 1, 1, False, False, False, 2),
        Shape("lower-2x2-mode1", 2 * T, 2 * T, 2, 1, False, False, False, 1),
    ]
    if with_3x3:
        S.append(Shape("lower-3x3", 3 * T, 3 * T, 1, 1, False, False, False, 2))
    return T, S


def entry_dims(sh, k, e, T):
    if sh.dims and e == 1:
        return T - 31, T - 3, max(k - 3, 1)
    return sh.m, sh.n, k


class _Device:
    """Device arrays through the library's own allocator; freed on exit."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)

    def put(self, a):
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), a.nbytes) == 0
        self.ptrs.append(p)
        assert self.lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def get(self, p, like):
        out = np.empty_like(like)
        assert self.lib.ek_hip_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out


def _view(buf, op, e, rows, cols):
    off = gc.entry_offset(op, e)
    return buf[off:off + op.ld * cols].reshape(cols, op.ld)[:, :rows].T


def layout(sh, ta, tb, k, scalar):
    """(A, B, C) as gemm_cases.layout() lays them out; scalar: an odd lda switches VEC off; sh.odd_ldc: an odd ldc."""
    ra, ca = (k, sh.m) if ta else (sh.m, k)
    rb, cb = (sh.n, k) if tb else (k, sh.n)
    A = gc._operand(ra, ca, scalar, False, sh.batch, "", 33, sh.share_ab)
    B = gc._operand(rb, cb, False, False, sh.batch, "", 33, sh.share_ab)
    C = gc._operand(sh.m, sh.n, sh.odd_ldc, False, sh.batch, "", 2, False)
    return A, B, C


def splitmix(seed, count):
    """count doubles in [-1, 1) from the splitmix64 sequence: the same bits whatever generator numpy ships."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -52) - 1.0


def launch(lib, kern, sh, T, ta, tb, k, alpha, beta, scalar, hA, hB, hC):
    """One launch on host images; returns C's allocation afterwards.  Asserts the variant."""
    A, B, C = layout(sh, ta, tb, k, scalar)
    dims = None
    if sh.dims:
        dims = np.array([entry_dims(sh, k, e, T) for e in range(sh.batch)], dtype=np.int32).ravel()
    v = np.full(8, -7, dtype=np.int32)
    with _Device(lib) as dev:
        dA, dB, dC = dev.put(hA), dev.put(hB), dev.put(hC)
        rc = lib.ek_hip_debug_gemm_desc(
            ta, tb, sh.m, sh.n, k, alpha, beta, ctypes.c_void_p(dA.value + 8 * A.front), A.ld, A.stride,
            ctypes.c_void_p(dB.value + 8 * B.front), B.ld, B.stride, ctypes.c_void_p(dC.value + 8 * C.front), C.ld, C.stride,
            sh.batch, sh.lower, 0, int(kern == gc.SMALL and sh.lower), 0, None,
            None if dims is None else dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            v.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        if rc <= -1000:
            pytest.exit("the GPU reported an error (%d) in %r: nothing more is launched on it" % (rc, sh), returncode=3)
        assert rc == 0, (rc, sh)
        got = dev.get(dC, hC)
    expect = (gc.W4 if (kern == gc.W8 and beta == 0.0) else kern, int(not scalar), sh.mode)
    assert (int(v[0]), int(v[1]), int(v[2])) == expect, (sh, ta, tb, k, beta, scalar, v[:4], expect)
    return got


def _run(lib, kern, sh, T, ta, tb, k, alpha, beta, scalar):
    rng = np.random.default_rng(zlib.crc32(repr((kern, sh, ta, tb, k, alpha, beta, scalar)).encode()))
    A, B, C = layout(sh, ta, tb, k, scalar)
    hA, hB, hC = np.full(A.total, np.nan), np.full(B.total, np.nan), np.full(C.total, np.nan)
    written = np.zeros(C.total, dtype=bool)
    refs = []
    ra, ca = (k, sh.m) if ta else (sh.m, k)
    rb, cb = (sh.n, k) if tb else (k, sh.n)
    Ae = Be = prod = None
    for e in range(sh.batch):
        m, n, ke = entry_dims(sh, k, e, T)
        if Ae is None or not sh.share_ab:
            Ae = rng.integers(-7, 8, (ra, ca)).astype(np.float64)
            Be = rng.integers(-7, 8, (rb, cb)).astype(np.float64)
            _view(hA, A, e, ra, ca)[...] = Ae
            _view(hB, B, e, rb, cb)[...] = Be
        opA = (Ae.T if ta else Ae)[:m, :ke]
        opB = (Be.T if tb else Be)[:ke, :n]
        # the host M x N of every entry holds integers (beta != 0) or NaN and +-Inf (beta = 0); a `dims` entry defines
        # its leading m x n only, the rest of the host shape must come back as it was
        if beta != 0.0:
            C0 = rng.integers(-1000, 1001, (sh.m, sh.n))
            Cin = C0.astype(np.float64)
        else:
            C0 = None
            Cin = np.tile([np.nan, np.inf, -np.inf], sh.m * sh.n // 3 + 1)[:sh.m * sh.n].reshape(sh.m, sh.n)
        inside = (np.arange(sh.m)[:, None] < m) & (np.arange(sh.n)[None, :] < n)
        upper = np.zeros((sh.m, sh.n), dtype=bool)
        if sh.lower:
            # a tile strictly above the diagonal is not referenced: NaN sentinels on every other entry of it
            upper = (np.arange(sh.n)[None, :] // T) > (np.arange(sh.m)[:, None] // T)
            Cin[upper & ((np.arange(sh.m)[:, None] + np.arange(sh.n)[None, :]) % 2 == 0)] = np.nan
        _view(hC, C, e, sh.m, sh.n)[...] = Cin
        # the float64 product is exact: every partial sum is an integer of at most 49 K
        if prod is None or not sh.share_ab:
            prod = (opA @ opB).astype(np.int64)
        twice = int(2 * alpha) * prod
        if beta != 0.0:
            twice += int(2 * beta) * C0[:m, :n]
        refs.append((twice / 2.0, (inside & ~upper)[:m, :n]))
        _view(written, C, e, sh.m, sh.n)[...] = inside & ~upper
    got = launch(lib, kern, sh, T, ta, tb, k, alpha, beta, scalar, hA, hB, hC)
    same = (got.view(np.uint64) == hC.view(np.uint64)) | written
    assert same.all(), (sh, ta, tb, k, int((~same).sum()), "entries outside the product changed; first at", int(np.argmin(same)))
    for e, (ref, defined) in enumerate(refs):
        g = _view(got, C, e, ref.shape[0], ref.shape[1])
        good = (g == ref) | ~defined
        if not good.all():
            bad = ~good
            raise AssertionError((sh, ta, tb, k, alpha, beta, scalar, "entry", e, int(bad.sum()), "of", good.size,
                                  "entries differ; first (row, column)", tuple(int(x[0]) for x in np.nonzero(bad)),
                                  g[bad][:4], ref[bad][:4]))


def _names(kern):
    return [sh.name for sh in shapes(kern)[1]]


def _sweep(lib, kern, name, betas, ks=None):
    """Every K, transpose, VEC and scalar of one shape; alpha and beta in rotation over the launches."""
    T, S = shapes(kern)
    sh = next(s for s in S if s.name == name)
    i = 0
    for k in ks or KS[kern]:
        for ta, tb in gc.TRANS:
            for scalar in (False, True):
                _run(lib, kern, sh, T, ta, tb, k, gc.ALPHAS[i % 4], betas[(i // 4 + i) % len(betas)], scalar)
                i += 1


@pytest.mark.parametrize("name", _names(gc.SMALL))
def test_small_kernel_epilogue(hip, name):
    """gemm_small_kernel, K = 4, 20, 36: VEC fetches the C tile in front of the K loop, scalar as one batch behind it."""
    _sweep(hip.load_library(), gc.SMALL, name, BETAS)


@pytest.mark.parametrize("name", _names(gc.W8))
def test_eight_wave_kernel_epilogue(hip, name):
    """gemm_kernel_w8, K = 16 and 20: two batches of 16 doubles per lane."""
    _sweep(hip.load_library(), gc.W8, name, BETAS)


@pytest.mark.parametrize("name", _names(gc.W4))
def test_four_wave_kernel_epilogue(hip, name):
    """gemm_kernel, K = 516: four batches of 16 doubles per lane."""
    _sweep(hip.load_library(), gc.W4, name, BETAS)


@pytest.mark.parametrize("kern", (gc.SMALL, gc.W8, gc.W4), ids=("small", "8-wave-shapes", "4-wave"))
def test_beta_zero_never_reads_c(hip, kern):
    """The same shapes with beta = 0 over NaN and +-Inf: exact, at the largest K of each kernel.  The 8-wave shapes
    (K = 20) run on the 4-wave kernel."""
    for name in _names(kern):
        _sweep(hip.load_library(), kern, name, (0.0,), KS[kern][-1:])


# ------------------------------------------------------------------------------------------- bit identity with the parent
def digest_cases():
    """(label, kern, shape, T, ta, tb, k): one per kernel, transposition and shape (VEC), the largest K of the kernel."""
    out = []
    for kern in (gc.SMALL, gc.W8, gc.W4):
        T, S = shapes(kern, with_3x3=True)
        for sh in S:
            for ta, tb in gc.TRANS:
                k = KS[kern][-1]
                out.append(("%s %s %d%d K=%d" % (gc.KERNEL_NAMES[kern], sh.name, ta, tb, k), kern, sh, T, ta, tb, k))
    return out


def digest_of(lib, case):
    """sha256 of C's allocation after C <- C - op(A) op(B) on splitmix data (the NaN padding included)."""
    label, kern, sh, T, ta, tb, k = case
    seed = zlib.crc32(label.encode())
    A, B, C = layout(sh, ta, tb, k, False)
    hA, hB, hC = np.full(A.total, np.nan), np.full(B.total, np.nan), np.full(C.total, np.nan)
    ra, ca = (k, sh.m) if ta else (sh.m, k)
    rb, cb = (sh.n, k) if tb else (k, sh.n)
    for e in range(1 if sh.share_ab else sh.batch):
        _view(hA, A, e, ra, ca)[...] = splitmix(seed + 3 * e, ra * ca).reshape(ra, ca)
        _view(hB, B, e, rb, cb)[...] = splitmix(seed + 3 * e + 1, rb * cb).reshape(rb, cb)
    for e in range(sh.batch):
        _view(hC, C, e, sh.m, sh.n)[...] = splitmix(seed + 3 * e + 2, sh.m * sh.n).reshape(sh.m, sh.n)
    got = launch(lib, kern, sh, T, ta, tb, k, -1.0, 1.0, False, hA, hB, hC)
    return hashlib.sha256(got.tobytes()).hexdigest()


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
