"""The dense -> band reduction (ek_sy2sb.hip: the panel chain, the in-LDS panel, the rescue, the SYMM with its split K, W,
the corrections of a pair, the trailing updates) as a stage, through ek_hip_debug_sy2sb_stage, in every flow of
sy2sb_lower: ek_hip_debug_set_sy2sb_flow forces pairs, the look-ahead on the second stream, both, and the hand-over from
the look-ahead flow to the plain one in mid-stage, at orders of a few hundred.  Inputs, the mirrors of the geometry, the
long-double references and the bounds are those of tests/sy2sb_cases.py.

Every test prints its figures as "sy2sb-ratio <check> n=<order> <class> <flow> <error / bound>" (pytest -s); the
identities also print the rescue count ("sy2sb-rescued n=<order> <class> <flow> <count> of <chain panels>").

Measured on an MI355X, error / bound, the worst over every order and flow with (order), and the most panels one call
sent to the rescue:

    class                    orthogonality   similarity    spectrum      rescued
    random                   0.002 (191)     0.001 (128)   0.048 (130)   0
    graded                   0.002 (256)     0.000         0.017 (127)   0
    graded_up                0.002 (131)     0.003 (128)   0.022 (130)   0
    entrywise                0.002 (127)     0.001 (129)   0.046 (67)    0
    big                      0.002 (129)     0.001 (129)   0.055 (127)   0
    tiny                     0.002 (129)     0.001 (129)   0.078 (130)   0
    band65                   0.002 (128)     0.000 (127)   0.059 (192)   22 (order 2113)
    band64                   0             0             0             6
    zero_columns             0.002 (131)     0.001 (127)   0.041 (193)   1
    parallel_columns         0.002 (191)     0.001 (128)   0.047 (128)   1
    lowrank_plus_identity    0.002 (130)     0.002 (129)   0.008 (127)   1
    near_identity            0.002 (129)     0.002 (129)   0.033 (128)   0
    outlier                  0.002 (256)     0.003 (129)   0.020 (192)   0
    ones                     0.001 (193)     0.026 (193)   0.068 (193)   6
    far_entry_before         0.005 (321)     0.001 (255)   0.039 (131)   3
    far_entry_at             0.006 (321)     0.001 (321)   0.046 (191)   3
    far_entry_after          0.004 (321)     0.001 (255)   0.050 (131)   3
    far_entry_last           0.005 (320)     0.001 (320)   0.087 (67)    3

The spectra of the pairs and handover bands against the plain one: at most 0.032 of 4 n eps max|w|.  The worst of all:
orthogonality 0.006, similarity 0.026, spectrum 0.087 -- the level of the float64 emulation of tests/sy2sb_cases.py
(0.002 / 0.002 / 0.057), except where the rescue's reflectors of a rank-deficient panel cost a few units more.  Every bit
contract held in every case: the first panel the same in every flow; the look-ahead changing no bit (see
test_flows_agree); two calls equal; NaN above the diagonal of A and in the workspace changing nothing.  No kernel had to
be changed, and lookahead_min = 2 stayed as it is (see the cases module)."""
import hashlib
import os

import numpy as np
import pytest

import sy2sb_cases as sc

pytestmark = pytest.mark.gpu

NAN = np.frombuffer(np.uint64(0x7FF8DEADBEEF1234).tobytes(), dtype=np.float64)[0]     # a NaN with a payload
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _flow_back_at_the_switches(hip):
    yield
    hip.set_sy2sb_flow(-1, -1)


def _run(hip, A, flow, poison=False):
    """(Ab, V, tau, flag) of the stage in the named flow; the hook is back at the switches afterwards"""
    hip.set_sy2sb_flow(*sc.FLOWS[flow])
    try:
        return hip.sy2sb_stage(A, poison=poison)
    finally:
        hip.set_sy2sb_flow(-1, -1)


def _bits(x, y):
    """equal bit for bit (NaN payloads and the sign of zero included)"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def _same(a, b, lower_only=False):
    """band (the whole returned matrix unless lower_only), V, tau and flag agree bit for bit"""
    A0, A1 = (np.tril(a[0]), np.tril(b[0])) if lower_only else (a[0], b[0])
    assert _bits(A0, A1), "band"
    assert _bits(a[1], b[1]), "V"
    assert _bits(a[2], b[2]), "tau"
    assert a[3] == b[3], ("flag", a[3], b[3])


def _report(check, n, cls, flow, value):
    print("sy2sb-ratio %s n=%d %s %s %.4f" % (check, n, cls, flow, value))


def _check_identities(A, out, cls, flow, seen):
    """flag, nothing below the band, structure, the three residuals, the rescue count.  seen: residuals by the digest of the
    output (flows that agree bit for bit share the long-double work)"""
    n = A.shape[0]
    Ab, V, tau, flag = out
    assert flag & 0xff == 0, (cls, n, flow, flag)
    assert np.isfinite(Ab).all()
    assert sc.below_band_is_zero(Ab), (cls, n, flow)
    sc.check_structure(V, tau)
    key = hashlib.sha256(np.tril(Ab).tobytes() + V.tobytes() + tau.tobytes()).digest()
    if key not in seen:
        seen[key] = sc.ratios(A, Ab, V, tau, sc.spectrum(cls, n) if n <= sc.SPECTRUM_MAX else None)
    orth, sim, spec = seen[key]
    _report("orthogonality", n, cls, flow, orth)
    _report("similarity", n, cls, flow, sim)
    if spec is not None:
        _report("spectrum", n, cls, flow, spec)
    rescued = flag >> 8
    print("sy2sb-rescued n=%d %s %s %d of %d chain panels" % (n, cls, flow, rescued, sc.chain_panels(n)))
    assert orth <= 1.0 and sim <= 1.0 and (spec is None or spec <= 1.0), (cls, n, flow, orth, sim, spec)
    assert rescued <= sc.chain_panels(n), (cls, n, flow, rescued)
    if cls == "random":
        assert rescued == 0, (n, flow, rescued)
    if cls in sc.RESCUED_CLASSES and n >= 193:
        assert rescued >= 1, (cls, n, flow)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_identities_in_every_flow(hip, case):
    """every class at the orders where the geometry changes (the in-LDS panel against the chain at m = 127 / 128, the chunk
    and block-row counts at m = 128 / 129, has_next at m - 64 = 2, ...), four classes at 1025 and at 2113 (two tiles per
    split of the SYMM, an uneven last split, a last chunk and block row of one row), in every flow"""
    n, classes = case
    for cls in classes:
        A = sc.matrix(cls, n)
        seen = {}
        for flow in sc.flows_of(n):
            _check_identities(A, _run(hip, A, flow), cls, flow, seen)


FLOW_CASES = tuple((n, c) for n in (130, 193, 257, 321, 449, 513, 1025) for c in sc.LARGE_CLASSES) \
    + tuple((n, c) for n in (258, 449) for c in ("parallel_columns", "lowrank_plus_identity", "far_entry_at", "ones"))


@pytest.mark.parametrize("n,cls", FLOW_CASES, ids=lambda v: str(v))
def test_flows_agree(hip, n, cls):
    """One input in every flow.  The first panel is factored before anything is pending: V[:, :64] and tau[:64] carry the
    same bits everywhere.  The look-ahead changes no bit of anything: the 64-tiling (gemm_small_kernel) and the staged
    rank-k kernel (gemm_rankk_kernel) both start every element's accumulator at zero and add K in ascending groups of four
    (one v_mfma_f64_16x16x4 per group, K = 128 or 256 in whole stages of 32 in both), as the one-launch update of the
    plain flow does on the same 64-tiling; alpha = -1 and beta = 1 make the epilogue C - acc in any contraction; and every
    element of the lower triangle is updated once -- so `lookahead` equals `plain` and `both` equals `pairs` bit for bit,
    band, V, tau and flag.  Pairs do change the arithmetic (DLATRD's corrections, a rank-256 update): their band agrees
    with the plain one in its spectrum, within 4 n eps max|w|."""
    A = sc.matrix(cls, n)
    w_ref = sc.spectrum(cls, n)
    out = {flow: _run(hip, A, flow) for flow in sc.flows_of(n)}
    for flow, r in out.items():
        assert r[3] & 0xff == 0
        assert _bits(r[1][:, :sc.SB], out["plain"][1][:, :sc.SB]) and _bits(r[2][:sc.SB], out["plain"][2][:sc.SB]), flow
    _same(out["lookahead"], out["plain"], lower_only=True)
    _same(out["both"], out["pairs"], lower_only=True)
    for flow in out:
        if flow in ("pairs", "handover"):
            r = sc.spectra_ratio(out[flow][0], out["plain"][0], w_ref)
            _report("spectrum_against_plain", n, cls, flow, r)
            assert r <= 1.0, (flow, r)


@pytest.mark.parametrize("flow", ["both", "handover"])
@pytest.mark.parametrize("n", [449, 513, 1025])
def test_two_calls_give_the_same_bits(hip, n, flow):
    """the second stream factors the next panel beside the update, out of double-buffered operand images, and the main
    stream takes it up behind an event: an ordering mistake would show as a difference between calls"""
    for cls in ("random", "band65"):
        A = sc.matrix(cls, n)
        first = _run(hip, A, flow)
        for _ in range(2):
            _same(_run(hip, A, flow), first)


@pytest.mark.parametrize("flow", ["plain", "both"])
@pytest.mark.parametrize("n", [130, 257, 449])
def test_only_the_lower_triangle_is_read(hip, n, flow):
    """the strict upper triangle of A holds a NaN: the lower band, V, tau and the flag are those of the clean call (what
    comes back above the diagonal is not looked at)"""
    for cls in ("random", "band65"):
        A = sc.matrix(cls, n)
        clean = _run(hip, A, flow)
        Ap = np.array(A, order="F")
        Ap[np.triu_indices(n, 1)] = NAN
        assert np.isnan(Ap).sum() == n * (n - 1) // 2
        _same(_run(hip, Ap, flow), clean, lower_only=True)


@pytest.mark.parametrize("flow", ["plain", "both"])
@pytest.mark.parametrize("cls", ["random", "band65"])
@pytest.mark.parametrize("n", [129, 193, 321, 513])
def test_nothing_is_read_from_the_workspace_before_it_is_written(hip, n, cls, flow):
    """the stage's own workspace filled with a NaN on entry: the same bits as from a zeroed one"""
    A = sc.matrix(cls, n)
    clean = _run(hip, A, flow)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    _same(_run(hip, A, flow, poison=True), clean)
    _same(_run(hip, A, flow), clean)                        # (and the workspace the poisoned call left changes nothing)


def _sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def test_the_hook_is_back_at_the_switches(hip, oracle, monkeypatch):
    """After everything above (this test is the module's last): without the hook's help the stage gives the bits of the
    anchor lines "sy2sb n=449" of tests/golden/path_anchor_digests.txt (written before the hook existed) -- the plain
    one with no switch set, the pairs one through EK_SY2SB_PAIR_MIN, which the hook would override if it were still
    set -- and the hook's own `plain` / `lookahead` and `pairs` / `both` give the same two sets of bits."""
    want = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "path_anchor_digests.txt")):
        if line.startswith("sy2sb n=449 "):
            label = "pairs" if " pairs " in line else "plain"
            want[label] = dict(kv.split("=") for kv in line.split() if kv.startswith(("band=", "reflectors=", "tau=", "flag=")))
    assert set(want) == {"plain", "pairs"}
    A = oracle.synth_matrix(449, 1)

    def digests(out):
        return {"band": _sha(out[0]), "reflectors": _sha(out[1]), "tau": _sha(out[2]), "flag": "%d" % out[3]}

    monkeypatch.delenv("EK_SY2SB_PAIR_MIN", raising=False)
    assert digests(hip.sy2sb(A)) == want["plain"]
    assert digests(hip.sy2sb_stage(A)) == want["plain"]
    monkeypatch.setenv("EK_SY2SB_PAIR_MIN", "1")
    assert digests(hip.sy2sb(A)) == want["pairs"]
    for flow, label in (("plain", "plain"), ("pairs", "pairs")):
        assert digests(_run(hip, A, flow)) == want[label], flow      # (the hook overrides the switch, both ways)
    monkeypatch.delenv("EK_SY2SB_PAIR_MIN", raising=False)
    for flow, label in (("lookahead", "plain"), ("both", "pairs")):
        d, w = digests(_run(hip, A, flow)), want[label]
        assert (d["reflectors"], d["tau"], d["flag"]) == (w["reflectors"], w["tau"], w["flag"]), flow
    assert digests(hip.sy2sb(A)) == want["plain"]
