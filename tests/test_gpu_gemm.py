"""Every fp64 GEMM variant (ek_gemm.hip), dispatch path and tile map, one launch at a time through ek_hip_debug_gemm_desc.

The products are the table of tests/gemm_cases.py (tests/test_gemm_host.py confirms its dispatch without a GPU).  Each
launch asserts the variant the hook reports -- kernel, VEC or scalar, lower_only as launched -- so a later change of a
threshold cannot quietly move a case to another kernel; the last test asserts that all of them were reached.

Set-up.  Every operand and C lie strictly inside a larger allocation whose remainder is NaN (rows M .. ld - 1 of every
column, a margin in front of the base and one behind the last column, the gaps of a batch).  A read of the padding is
inside the allocation but poisons the result; after the call everything of C's allocation that the product does not
define must come back bit for bit.

The reference is exact.  Operands are integers in [-7, 7], C integers in [-1000, 1000], alpha in {1, -1, 2, -0.5}, beta in
{0, 1, -2, 0.5}, K <= 640: every product, partial sum and scaled value is an integer or a half integer below 2^16, exactly
representable whatever the order of summation and whatever is fused, so the kernel must EQUAL the int64 result.  Where
beta = 0, C holds NaN and +-Inf beforehand.  One uniform(-1, 1) product per kernel is held to 4 K eps against long double
(the bound of test_gpu_blocks.py::test_dgemm_matches_numpy)."""
import ctypes
import zlib

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu
EPS = 2.220446049250313e-16

_LAUNCHED = set()        # variants the hook reported, over the module
_RAN = set()             # keys of the table that ran


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
    """Entry e of an operand inside its allocation `buf`, as a rows x cols (column-major) view."""
    off = gc.entry_offset(op, e)
    return buf[off:off + op.ld * cols].reshape(cols, op.ld)[:, :rows].T


def _operands(c, rng, e, ra, ca, rb, cb):
    if c.data == "uniform":
        return rng.uniform(-1, 1, (ra, ca)), rng.uniform(-1, 1, (rb, cb))
    if c.data == "identity":
        return np.eye(ra, ca), np.arange(rb * cb, dtype=np.float64).reshape(rb, cb)
    return (rng.integers(-7, 8, (ra, ca)).astype(np.float64), rng.integers(-7, 8, (rb, cb)).astype(np.float64))


def _exact_product(X, Y):
    """X Y of integer matrices as int64.  Small ones by numpy's integer product; the others by the float64 BLAS, which is
    the same numbers: every partial sum is an integer of at most 49 K, far below 2^53, so no rounding takes place."""
    if X.shape[0] * X.shape[1] * Y.shape[1] <= 1 << 18:
        return X.astype(np.int64) @ Y.astype(np.int64)
    return (X @ Y).astype(np.int64)


def _run(lib, c):
    """One launch of a case: builds the images, launches, checks the variant, the result and everything around it."""
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    A, B, C = gc.layout(c)
    hA = np.full(A.total, np.nan)
    hB = hA if c.gram else np.full(B.total, np.nan)
    hC = np.full(C.total, np.nan)
    written = np.zeros(C.total, dtype=bool)
    refs = []                # per entry: the reference and the mask of the tiles lower_only leaves alone (or None)
    tile = 64 if c.small_tiles else 128
    Ae = Be = None
    for e in range(c.batch):
        m, n, k = gc.entry_dims(c, e)
        ra, ca = (k, m) if c.ta else (m, k)
        rb, cb = (n, k) if c.tb else (k, n)
        if Ae is None or not c.share_ab:
            Ae, Be = _operands(c, rng, e, ra, ca, rb, cb)
            if c.gram:
                Be = Ae
            _view(hA, A, e, ra, ca)[...] = Ae
            if not c.gram:
                _view(hB, B, e, rb, cb)[...] = Be
        opA = Ae.T if c.ta else Ae
        opB = Be.T if c.tb else Be
        # C beforehand: integers; NaN and +-Inf where beta = 0 must ignore it
        if c.data == "uniform":
            C0 = rng.uniform(-1, 1, (m, n))
            Cin = C0.copy()
        elif c.beta != 0.0:
            C0 = rng.integers(-1000, 1001, (m, n))
            Cin = C0.astype(np.float64)
        else:
            C0 = None
            Cin = np.tile([np.nan, np.inf, -np.inf], m * n // 3 + 1)[:m * n].reshape(m, n)
        # lower_only: a tile strictly above the diagonal is not referenced -- NaN sentinels on every other entry of it
        # (beta * NaN would hide a visit on its own; the integers between them would not)
        upper = None
        if c.lower:
            upper = (np.arange(n)[None, :] // tile) > (np.arange(m)[:, None] // tile)
            Cin[upper & ((np.arange(m)[:, None] + np.arange(n)[None, :]) % 2 == 0)] = np.nan
        _view(hC, C, e, m, n)[...] = Cin
        if c.data == "uniform":
            ref = c.alpha * (opA.astype(np.longdouble) @ opB.astype(np.longdouble)) + c.beta * C0.astype(np.longdouble)
            ref = ref.astype(np.float64)
        else:
            twice = int(2 * c.alpha) * _exact_product(opA, opB)
            if c.beta != 0.0:
                twice += int(2 * c.beta) * C0
            ref = twice / 2.0
        refs.append((ref, upper))
        _view(written, C, e, m, n)[...] = True if upper is None else ~upper
    with _Device(lib) as dev:
        dA = dev.put(hA)
        dB = dA if c.gram else dev.put(hB)
        dC = dev.put(hC)
        rc, v = gc.call(lib, True, c, dA.value, dB.value, dC.value)
        if rc <= -1000:
            pytest.exit("the GPU reported an error (%d) in %r: nothing more is launched on it" % (rc, c), returncode=3)
        assert rc == 0, (rc, c)
        got = dev.get(dC, hC)
    assert (int(v[0]), int(v[1]), int(v[2])) == c.expect, (c, v)
    _LAUNCHED.add((int(v[0]), c.ta, c.tb, int(v[1]), int(v[2])))
    # the remainder of the allocation, and the tiles lower_only leaves alone: bit for bit
    same = (got.view(np.uint64) == hC.view(np.uint64)) | written
    assert same.all(), (c, int((~same).sum()), "entries outside the product changed; first at", int(np.argmin(same)))
    for e, (ref, upper) in enumerate(refs):
        g = _view(got, C, e, ref.shape[0], ref.shape[1])
        if c.data == "uniform":
            err = np.abs(g - ref) if upper is None else np.where(upper, 0.0, np.abs(g - ref))
            tol = 4 * c.k * EPS
            assert np.all(np.isfinite(err)) and err.max(initial=0) <= tol, (c, e, err.max(initial=0), tol)
            continue
        good = (g == ref) if upper is None else ((g == ref) | upper)
        if not good.all():
            bad = ~good
            raise AssertionError((c, "entry", e, int(bad.sum()), "of", good.size, "entries differ; first (row, column)",
                                  tuple(int(x[0]) for x in np.nonzero(bad)), g[bad][:4], ref[bad][:4]))


def _keys(prefix):
    return [k for k in gc.KEYS if k.startswith(prefix)]


def _run_key(hip, key):
    lib = hip.load_library()
    cases = [c for c in gc.CASES if c.key == key]
    assert cases
    for c in cases:
        _run(lib, c)
    _RAN.add(key)


@pytest.mark.parametrize("key", _keys("small-"))
def test_small_kernel_every_transpose_vec_and_scalar(hip, key):
    """gemm_small_kernel (64 x 64 x 32): four transposes x {VEC, odd lda, odd ldb, base 8 mod 16}, every alpha and beta;
    K = 0 is C <- beta C."""
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("w4-"))
def test_four_wave_kernel_every_transpose_vec_and_scalar(hip, key):
    """gemm_kernel: 16 x 16 ragged tiles with beta = 0 over a C of NaN and Inf, a lower_only product with K > 512 and
    beta = 1, a batch of 64 by strides."""
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("w8-"))
def test_eight_wave_kernel_every_transpose_vec_and_scalar(hip, key):
    """gemm_kernel_w8: the same shapes with beta != 0 and K in {1, 15, 16, 17, 512}."""
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("rankk-"))
def test_rank_k_kernel_every_stage_count_vec_and_scalar(hip, key):
    """gemm_rankk_kernel: K in {32, 33, 64, 100, 128, 256} (one to eight stages of 32, ragged last stage), lower_only,
    beta = 1 and beta = 0 over NaN; an odd leading dimension makes its own run-time test take the scalar fetch."""
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("lower-"))
def test_lower_only_writes_the_tiles_on_and_below_the_diagonal_once(hip, key):
    """The contract: a tile with n0 > m0 + T - 1 (T = 128, or 64 with small_tiles) is untouched bit for bit, every other
    tile holds the full product -- once: beta = 1.  Compact grids square and tall, the whole grid where N is wider than M
    in tiles and for a batch."""
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("modes-"))
def test_every_instantiation_in_both_lower_only_grids(hip, key):
    _run_key(hip, key)


@pytest.mark.parametrize("key", _keys("tables-"))
def test_batches_by_offset_and_dimension_tables(hip, key):
    """The D&C and ORMTR forms: strides 0, offsets into shared buffers, per-entry dims below the host's; even offsets with
    the promise (VEC) and odd ones without (scalar); below and above 256 tiles.  Outside each entry's M x N every byte of
    C is unchanged, an entry with K = 0 and beta = 0 writes zeros; the Gram products V^T V read A and B at one pointer."""
    _run_key(hip, key)


def test_asymmetric_identity_on_the_128_tilings(hip):
    """A = I, B = arange on the 4-wave, 8-wave and rank-k kernels (256 entries of one tile): a transposed store shows."""
    _run_key(hip, "asymmetry")


def test_uniform_products_against_long_double(hip):
    """One per kernel, |alpha|, |beta| <= 1: |C - ref| <= 4 K eps -- exact on integers is not enough."""
    _run_key(hip, "uniform")


def test_beta_zero_ignores_nan_and_inf_in_c_on_every_kernel_that_takes_it(hip):
    """The small, 4-wave and rank-k kernels; gemm() never gives the 8-wave kernel a product with beta = 0."""
    lib = hip.load_library()
    assert not [c for c in gc.CASES if c.expect[0] == gc.W8 and c.beta == 0.0]
    for kern in (gc.SMALL, gc.W4, gc.RANKK):
        c = min((c for c in gc.CASES if c.expect[0] == kern and c.beta == 0.0 and c.data == "int" and c.k > 0),
                key=lambda c: c.m * c.n * c.batch)
        _run(lib, c)


def test_every_instantiation_was_launched(hip):
    """The table states every instantiation in every lower_only mode (no GPU needed for that); when the whole module ran,
    the hook has reported every one of them as launched."""
    assert {gc.variant_of(c) for c in gc.CASES} == gc.all_variants()
    assert _LAUNCHED <= gc.all_variants()
    if _RAN == set(gc.KEYS):
        assert _LAUNCHED == gc.all_variants(), sorted(gc.all_variants() - _LAUNCHED)
