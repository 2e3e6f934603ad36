"""The bulge chasing and the application of Q2 (ek_sb2st.hip: chase_pos_kernel, chase_kernel, q2_tfactor_kernel,
q2_apply_nb_kernel) as a stage, through ek_hip_debug_sb2st_stage: the reflectors and tau as the stage leaves them, either
chase kernel on demand with the kernel that really ran reported, and the workspace form of the hook (form 0) or of a
whole-path solve (form 1).  Inputs, the long-double references and the bounds are those of tests/sb2st_cases.py; the
chase is judged from the exported reflectors (residual of the two-sided application, orthogonality of their product,
every reflector a Householder reflector), Q2's application against the sequential application of the same reflectors.

Measured on an MI355X, error / bound, the worst of each check with (order) -- every test prints its figures as
"sb2st-ratio <check> n=<order> <class> <ratio>" (pytest -s):

    class                       residual      orthogonality   |tau v'v - 2| / 16 eps   Z (Q2 against the reference)
    random                      0.056 (34)    0.133 (35)      0.218 (1025)             0.148 (34)
    graded                      0.035 (33)    0.125 (35)      0.187 (1025)             0.177 (67)
    graded_up                   0.041 (33)    0.135 (33)      0.196 (195)
    entrywise                   0.062 (34)    0.149 (33)      0.167 (321)
    big                         0.058 (33)    0.140 (34)      0.209 (321)
    tiny                        0.057 (33)    0.154 (35)      0.175 (193)
    width5                      0.053 (33)    0.127 (35)      0.192 (1025)
    width63                     0.056 (35)    0.131 (35)      0.181 (321)
    outer_only                  0.018 (97)    0.082 (196)     0.188 (194)              0.062 (98)
    zero_columns                0.055 (33)    0.140 (34)      0.240 (1025)             0.141 (34)
    near_identity               0.074 (34)    0.148 (34)      0.177 (129)
    outlier                     0.062 (34)    0.152 (33)      0.187 (321)
    ones                        0.044 (4)     0.109 (97)      0.194 (194)
    dead_first_column_1e-158    0.061 (33)    0.157 (33)      0.174 (193)
    dead_first_column_1e-160    0.062 (33)    0.138 (33)      0.195 (321)
    dead_first_column_1e-161    0.058 (34)    0.158 (34)      0.180 (196)

    Z in the whole path's workspace form 0.046 (130); with a wrapped ticket counter 0.015 (1025), 0.012 (1537); on more
    columns than the workspace has progress words 0.057 (98), 0.027 (321).

The worst of all: residual 0.074, orthogonality 0.158 (0.32 of m eps), Z 0.177, |tau v'v - 2| 3.8 eps -- what the float64
emulation of tests/sb2st_cases.py loses on the CPU, within a few hundredths.  Every bit contract (the two chase kernels,
the two workspace forms, 2, 3 and 4 blocks per pass, column pieces, NaN where nothing is read) held in every case.
"""
import numpy as np
import pytest

import sb2st_cases as sc

pytestmark = pytest.mark.gpu

SAMPLE = (0, 15, 16, 63, 64)


def _bits(x, y):
    """equal bit for bit (NaN payloads and the sign of zero included)"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def _same_stage(a, b, keys=("d", "e", "V2", "tau2", "Z")):
    for key in keys:
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
        else:
            assert _bits(a[key], b[key]), key


def _report(check, n, cls, value):
    print("sb2st-ratio %s n=%d %s %.4f" % (check, n, cls, value))


def _dropped(cls, n):
    return [(0, 0)] if cls in sc.DEAD_CLASSES and n >= 3 else []


def _check_chase(r, B, cls):
    """flag, finite d and e, the structure of the reflectors, residual and orthogonality: returns the three ratios"""
    n = B.shape[0]
    assert r["flag"] == 0
    assert np.isfinite(r["d"]).all() and np.isfinite(r["e"]).all()
    struct = sc.check_structure(r["V2"], r["tau2"], _dropped(cls, n))
    res, orth = sc.chase_ratios(B, r["d"], r["e"], r["V2"], r["tau2"])
    _report("residual", n, cls, res)
    _report("orthogonality", n, cls, orth)
    _report("tau_vtv_of_16eps", n, cls, struct / 16.0)
    assert res <= 1.0 and orth <= 1.0, (cls, n, res, orth)
    return res, orth, struct


@pytest.mark.parametrize("case", sc.CHASE_CASES, ids=sc.case_id)
def test_chase_at_the_edges_of_the_geometry(hip, case):
    """every class at the degenerate orders, at n - 1 = 0 (mod 32) (a block of 32 sweeps more), n - 3 = 0 (mod 64) (a task
    more per sweep), three blocks of sweeps per bundle, and their neighbours; four classes at 513 and 1025"""
    n, classes = case
    for cls in classes:
        B = sc.band(cls, n)
        r = hip.sb2st_stage(B)
        _check_chase(r, B, cls)
        if n < 3:
            assert r["ran"] == 0 and np.array_equal(r["d"], np.diag(B)) and np.array_equal(r["e"], np.diag(B, -1))
        else:
            assert r["ran"] in (2, 3)              # the default: positions in registers (3: the census gave up, sweeps redid it)


def _both_kernels(hip, B):
    r1 = hip.sb2st_stage(B, chase_mode=1)
    r2 = hip.sb2st_stage(B, chase_mode=2)
    assert r1["flag"] == 0 and r2["flag"] == 0
    assert r1["ran"] == 1
    if r2["ran"] == 1:
        pytest.skip("this chip does not hold the %d positions of order %d at once: the position kernel was not launched"
                    % ((B.shape[0] - 3) // 64 + 1, B.shape[0]))
    assert r2["ran"] == 2
    return r1, r2


@pytest.mark.parametrize("cls", ["random", "width5", "zero_columns", "outer_only"])
@pytest.mark.parametrize("n", [3, 4, 66, 67, 131, 193, 777, 1500, 4200])
def test_both_chase_kernels_run_and_give_the_same_bits(hip, n, cls):
    """chase_mode 1 and 2 through sb2st_lower's own argument (the switch EK_SB2ST_CHASE is read once per process): the control
    words say which kernel ran; d, e, every reflector and every tau agree bit for bit.  width5, zero_columns and outer_only
    send identity reflectors (tau = 0) and dropped columns through the position kernel's mail lines."""
    r1, r2 = _both_kernels(hip, sc.band(cls, n))
    _same_stage(r1, r2)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cls", sc.DEAD_CLASSES)
def test_drop_rule_on_a_first_column_with_denormal_squares(hip, cls, mode):
    """B[1:65, 0] around 1e-158 .. 1e-161: the squared norm is denormal (at 1e-161: nine significant bits); reflector (0, 0)
    must be the identity, or Q2 is not orthogonal in the third digit (tests/test_sb2st_cases_host.py shows that)"""
    n = 130
    B = sc.band(cls, n)
    r = hip.sb2st_stage(B, chase_mode=mode)
    if mode == 2 and r["ran"] == 1:
        pytest.skip("this chip does not hold the positions of order %d at once" % n)
    assert r["ran"] == mode
    assert r["tau2"][0, 0] == 0.0 and r["d"][0] == B[0, 0]
    assert r["V2"][1, 0] == 1.0 and not r["V2"][2:65, 0].any()
    _check_chase(r, B, cls)
    if mode == 2:
        _same_stage(hip.sb2st_stage(B, chase_mode=1), r)


@pytest.mark.parametrize("ncols", [17, None])
@pytest.mark.parametrize("n", [130, 321, 1025])
def test_whole_path_workspace_form_gives_the_bits_of_the_hook_form(hip, n, ncols):
    """form 1 is what Path does: pack_band into sb2st_band(work, n) of the workspace without records (other offsets of the
    progress words and of the records' offsets), band_packed = true, the records in a lent array"""
    ncols = n if ncols is None else ncols
    B, Z = sc.band("random", n), sc.z_input(n, ncols, "random")
    r0 = hip.sb2st_stage(B, Z, form=0)
    r1 = hip.sb2st_stage(B, Z, form=1)
    assert r0["flag"] == 0 and r1["flag"] == 0 and r0["ran"] == r1["ran"]
    _same_stage(r0, r1)
    d, e, Zh, f = hip.sb2st(B, Z)                                    # the older hook: the same stage
    assert f == 0 and _bits(d, r0["d"]) and _bits(e, r0["e"]) and _bits(Zh, r0["Z"])
    cols = [c for c in SAMPLE + (ncols - 1,) if c < ncols]
    zr = sc.z_ratio(r1["Z"][:, cols], sc.apply(sc.reflectors(r1["V2"], r1["tau2"]), Z[:, cols]), n)
    _report("z_form1", n, "random", zr)
    assert zr <= 1.0


@pytest.mark.parametrize("cls", ["random", "graded", "zero_columns", "outer_only"])
@pytest.mark.parametrize("n", [34, 67, 98, 131, 194, 321])
def test_q2_on_general_columns_against_the_reference(hip, monkeypatch, n, cls):
    """widths round a 16-column tile and a 64-column slab, random columns and columns scaled by 1e+100 / 1e-100; the default
    number of blocks per pass against the long-double application of the same reflectors on sample columns, and 2, 3 and 4
    blocks per pass equal to it bit for bit"""
    B = sc.band(cls, n)
    worst = 0.0
    refl = None
    for w in (1, 15, 16, 17, 63, 64, 65, 129, n):
        for kind in ("random", "scaled"):
            Z = sc.z_input(n, w, kind)
            monkeypatch.delenv("EK_Q2_NBLK", raising=False)
            r = hip.sb2st_stage(B, Z, reflectors=refl is None)
            assert r["flag"] == 0 and r["Z"].shape == (n, w)
            if refl is None:
                refl = sc.reflectors(r["V2"], r["tau2"])
            cols = sorted(set(c for c in SAMPLE + (w - 1,) if c < w))
            worst = max(worst, sc.z_ratio(r["Z"][:, cols], sc.apply(refl, Z[:, cols]), n))
            for nblk in ("2", "3", "4"):
                monkeypatch.setenv("EK_Q2_NBLK", nblk)
                rb = hip.sb2st_stage(B, Z, reflectors=False)
                assert rb["flag"] == 0 and _bits(rb["Z"], r["Z"]), (w, kind, nblk)
    _report("z", n, cls, worst)
    assert worst <= 1.0


@pytest.mark.parametrize("n,ncols", [(1025, 2304), (1537, 1537)])
def test_q2_with_a_wrapped_ticket_counter(hip, monkeypatch, n, ncols):
    """two blocks per pass make 576 and 600 passes for the 512 workgroups: every workgroup comes back to the ticket counter, as
    in every solve of production size"""
    assert sc.q2_passes(n, ncols, 2)[2] > sc.Q2_WORKGROUPS >= sc.q2_passes(n, ncols, 3)[2]
    B, Z = sc.band("random", n), sc.z_input(n, ncols, "random")
    monkeypatch.setenv("EK_Q2_NBLK", "2")
    r2 = hip.sb2st_stage(B, Z)
    monkeypatch.setenv("EK_Q2_NBLK", "3")
    r3 = hip.sb2st_stage(B, Z, reflectors=False)
    assert r2["flag"] == 0 and r3["flag"] == 0
    assert _bits(r2["Z"], r3["Z"])
    cols = sc.sample_columns(ncols)
    zr = sc.z_ratio(r2["Z"][:, cols], sc.apply(sc.reflectors(r2["V2"], r2["tau2"]), Z[:, cols]), n)
    _report("z_wrapped", n, "random", zr)
    assert zr <= 1.0


@pytest.mark.parametrize("n,ncols,nblk", [(321, 1000, 2), (98, 2304, 3), (98, 2304, 2)])
def test_q2_on_more_columns_than_the_workspace_has_progress_words(hip, monkeypatch, n, ncols, nblk):
    """The workspace holds a progress word per pass for ncols <= n; 80 passes at (321, 1000) and 72 at (98, 2304) are more
    than its 64 words: such a call goes in pieces of whole slabs (before, its words ran over the records' offsets)"""
    B, Z = sc.band("random", n), sc.z_input(n, ncols, "random")
    monkeypatch.setenv("EK_Q2_NBLK", str(nblk))
    assert sc.q2_passes(n, ncols, nblk)[2] > 64
    r = hip.sb2st_stage(B, Z)
    assert r["flag"] == 0
    cols = sc.sample_columns(ncols)
    zr = sc.z_ratio(r["Z"][:, cols], sc.apply(sc.reflectors(r["V2"], r["tau2"]), Z[:, cols]), n)
    _report("z_many_columns", n, "random", zr)
    assert zr <= 1.0
    tail = hip.sb2st_stage(B, Z[:, ncols - 200:], reflectors=False)
    assert _bits(tail["Z"], r["Z"][:, ncols - 200:])


def test_q2_columns_are_independent(hip):
    """a call on Z[:, c0:c0+w] carries the bits of the one call; a NaN column and an Inf column leave every other column alone"""
    n = 321
    B, Z = sc.band("random", n), sc.z_input(n, n, "random")
    full = hip.sb2st_stage(B, Z, reflectors=False)
    assert full["flag"] == 0
    for c0 in (0, 1, 16, 37, 64):
        for w in (1, 17, 64, 100):
            part = hip.sb2st_stage(B, Z[:, c0:c0 + w], reflectors=False)
            assert part["flag"] == 0 and _bits(part["Z"], full["Z"][:, c0:c0 + w]), (c0, w)
    Zp = np.array(Z, order="F")
    Zp[:, 5] = np.nan
    Zp[:, 70] = np.inf
    Zp[17, 200] = -np.inf
    bad = hip.sb2st_stage(B, Zp, reflectors=False)
    keep = [c for c in range(n) if c not in (5, 70, 200)]
    assert _bits(bad["Z"][:, keep], full["Z"][:, keep])
    assert np.isnan(bad["Z"][:, 5]).all() and not np.isfinite(bad["Z"][:, 70]).any()
    assert _bits(bad["d"], full["d"]) and _bits(bad["e"], full["e"])


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", [130, 321])
def test_what_the_stage_never_reads(hip, n, form):
    """NaN above the diagonal of A, below its 64th sub-diagonal and in the padding of every host array (three more rows
    than needed in lda, ldv2, ldtau and ldz): every output keeps its bits"""
    B, Z = sc.band("random", n), sc.z_input(n, 17, "random")
    clean = hip.sb2st_stage(B, Z, form=form)
    i = np.arange(n)
    A = np.array(B, order="F")
    A[(i[:, None] < i[None, :]) | (i[:, None] - i[None, :] > sc.SB)] = np.nan
    assert np.isnan(A).sum() == n * n - sum(min(sc.SB + 1, n - c) for c in range(n))
    r = hip.sb2st_stage(A, Z, form=form, pad=3)
    assert r["flag"] == 0 and clean["flag"] == 0 and r["ran"] == clean["ran"]
    _same_stage(clean, r)
