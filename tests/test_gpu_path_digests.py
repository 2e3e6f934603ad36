"""Bit identity of the one-problem path with two earlier builds: tests/golden/path_anchor_digests.txt holds, per case,
the first 16 hex digits of the SHA-256 of every output, written by tools/path_digests.py, and every one must be
reproduced.  Its first 30 lines (down to "sygst_team n=449 team=3") were written on the build before csrc/ek_switch.h
("Run-time switches"); the lines after them on the build before the whole-path driver became a Path of stages
("The Path"), which reproduced the first 30 byte for byte.  (The band -> tridiagonal stage on its own has
tests/golden/q2_anchor_digests.txt.)

Inputs are the synthetic generator's (oracle.synth_matrix: A = seed 1, B = seed 2); nothing is stored but digests.  The
cases are the smallest orders at which each branch that a removed switch reached is taken by default:
  whole solves, standard and generalized: n = 130 (one-stage tridiagonalisation: the symv launch), n = 600 (two stages,
      chase_pos_kernel then chase_kernel<8>, Q2 with 3 blocks), n = 600 with the panels in pairs and with the chase's
      sweeps through memory, n = 5200 (look-ahead and pairs by default; generalized: sygst's folded update and the
      Cholesky's outer blocks of 4); standard only: n = 8320 (above the 8192 of the staged trailing update, Q2 with 4
      blocks, the placement probes; all of w, 256 columns of Z)
  eigenvalues only and an index window at n = 600
  stages: potrf and sygst types 1 to 3 at n = 300 and 4097, sytrd at 257, sy2sb at 449 with pairs forced and not, the
      one-GPU rehearsals of sy2sb, sytrd, potrf and sygst with a team of 3 at n = 449
and, for every way through the whole-path driver (130: one stage, 600: two stages, 640: a multiple of 128):
  the device entry on arrays it aliases (n = 640, ld = 640), with EK_HIP_ALIAS=0, and on arrays it copies (600, ld 603)
  grid cells on one GPU without a communicator: every cell of 2 x 2 (generalized 600, standard 130), the *_select arm on
      1 x 3 (640, 77 columns), ek_hip_solve_device_grid for cell (1,0) of 2 x 2; distributed inputs through the host hook
  a communicator of one rank with EK_HIP_DIST_MIN_RANKS=1 (the `dist` arm of every stage)
  value windows at n = 600: pairs, values only, an empty interval, a zcap one short of m (-18, w and Z untouched)
  sygvx types 2 and 3 at n = 600: index window, full range, values only (type 2); the *_select arm on 1 x 1
  the band short cut taken and switched off, A scaled by 1e200 and 1e-200, a repeated bulge chasing
  the staging pipeline at n = 600 (EK_HIP_PIPE_MIN=256), also with local arrays of 603 rows
A case whose switch is read once per process (EK_SB2ST_CHASE) runs in a process of its own, through the tool."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "tests", "golden", "path_anchor_digests.txt")
TOOL = os.path.join(ROOT, "tools", "path_digests.py")


def _sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def _solve(generalized, n, zcols=None):
    def run(hip, oracle):
        A = oracle.synth_matrix(n, 1)
        B = oracle.synth_matrix(n, 2) if generalized else None
        ep, _ = hip.eigen_solver("general_hip" if generalized else "hip", A, B)
        Z = ep.Vectors if zcols is None else ep.Vectors[:, :zcols]
        return [("w", _sha(ep.values)), ("Z", _sha(Z))]
    return run


def _values(generalized, n):
    def run(hip, oracle):
        A = oracle.synth_matrix(n, 1)
        B = oracle.synth_matrix(n, 2) if generalized else None
        return [("w", _sha(hip.eigenvalues(A, B)))]
    return run


def _window(generalized, n, il, iu):
    def run(hip, oracle):
        A = oracle.synth_matrix(n, 1)
        B = oracle.synth_matrix(n, 2) if generalized else None
        w, Z, first = hip.eigenpairs(A, B, il=il, iu=iu)
        return [("w", _sha(w)), ("Z", _sha(Z)), ("first", "%d" % first)]
    return run


def _potrf(n):
    def run(hip, oracle):
        L, info = hip.potrf(oracle.synth_matrix(n, 2))
        return [("factor", _sha(L)), ("info", "%d" % info)]
    return run


def _sygst(n, ibtype):
    def run(hip, oracle):
        L, info = hip.potrf(oracle.synth_matrix(n, 2))
        assert info == 0
        C, info = hip.sygst_ibtype(oracle.synth_matrix(n, 1), L, ibtype)
        return [("reduced", _sha(C)), ("info", "%d" % info)]
    return run


def _sytrd(n, team=None):
    def run(hip, oracle):
        A = oracle.synth_matrix(n, 1)
        out = hip.sytrd(A) if team is None else hip.sytrd_team(A, team)
        Ar, d, e, tau, info = out[:5]
        return [("reflectors", _sha(Ar)), ("d", _sha(d)), ("e", _sha(e)), ("tau", _sha(tau)), ("info", "%d" % info)] + \
               ([] if team is None else [("mismatch", "%d" % out[5])])
    return run


def _sy2sb(n, team=None):
    def run(hip, oracle):
        A = oracle.synth_matrix(n, 1)
        out = hip.sy2sb(A) if team is None else hip.sy2sb_team(A, team)
        Ab, V, tau, flag = out[:4]
        return [("band", _sha(Ab)), ("reflectors", _sha(V)), ("tau", _sha(tau)), ("flag", "%d" % flag)] + \
               ([] if team is None else [("mismatch", "%d" % out[4])])
    return run


def _potrf_team(n, team):
    def run(hip, oracle):
        L, info, mismatch = hip.potrf_team(oracle.synth_matrix(n, 2), team)
        return [("factor", _sha(L)), ("info", "%d" % info), ("mismatch", "%d" % mismatch)]
    return run


def _sygst_team(n, team):
    def run(hip, oracle):
        L, info = hip.potrf(oracle.synth_matrix(n, 2))
        assert info == 0
        C, info = hip.sygst_team(oracle.synth_matrix(n, 1), np.tril(L), team)
        return [("reduced", _sha(C)), ("info", "%d" % info)]
    return run


# ------------------------------------------------------------------ the cases behind every way through the Path
def _pair(generalized, n):
    from oracle import ek_oracle
    return ek_oracle.synth_matrix(n, 1), (ek_oracle.synth_matrix(n, 2) if generalized else None)


class _Dev:
    """Device arrays of one call through a *_device entry: up(M) -> pointer, down(p, like) -> host copy."""
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def up(self, M):
        import ctypes
        M = np.asfortranarray(M)
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), M.nbytes) == 0
        self.ptrs.append(p)
        assert self.lib.ek_hip_memcpy_h2d(p, M.ctypes.data_as(ctypes.c_void_p), M.nbytes) == 0
        return p

    def down(self, p, shape):
        import ctypes
        M = np.zeros(shape, order="F")
        assert self.lib.ek_hip_memcpy_d2h(M.ctypes.data_as(ctypes.c_void_p), p, M.nbytes) == 0
        return M

    def free(self):
        for p in self.ptrs:
            self.lib.ek_hip_free(p)


def _rows(M, ld):
    out = np.zeros((ld, M.shape[1]), order="F")
    out[:M.shape[0]] = M
    return out


def _device(n, ld, cell=None, problem=1, nb=32):
    """ek_hip_solve_device (cell None) or ek_hip_solve_device_grid for cell = (nprow, npcol, myrow, mycol): w, Z and what
    is left in A and B, every array whole (with its ld - n rows of padding)."""
    def run(hip, oracle):
        lib = hip.load_library()
        A, B = _pair(problem == 1, n)
        dev = _Dev(lib)
        try:
            dA = dev.up(_rows(A, ld)); dB = dev.up(_rows(B, ld)) if problem == 1 else None
            dw = dev.up(np.zeros(n))
            if cell is None:
                zshape = (ld, n)
                dZ = dev.up(np.zeros(zshape))
                info = lib.ek_hip_solve_device(problem, n, n, dA, ld, dB, ld, dw, dZ, ld, None, 0)
            else:
                from eigenkernel_amd import descriptor as d
                zshape = (max(1, d.numroc(n, nb, cell[2], 0, cell[0])), max(1, d.numroc(n, nb, cell[3], 0, cell[1])))
                dZ = dev.up(np.zeros(zshape))
                info = lib.ek_hip_solve_device_grid(problem, n, n, dA, ld, dB, ld, dw, dZ, zshape[0], nb, *cell, None, 0)
            out = [("info", "%d" % info), ("w", _sha(dev.down(dw, (n,)))), ("Z", _sha(dev.down(dZ, zshape))),
                   ("A", _sha(dev.down(dA, (ld, n))))]
            return out + ([("B", _sha(dev.down(dB, (ld, n))))] if problem == 1 else [])
        finally:
            dev.free()
    return run


def _grid(name, n, grid, n_vec=None, inputs="replicated"):
    """Every cell of the grid in turn, as its rank would call: Z_loc and w per cell (distributed inputs, through the
    host hook: Z_loc, A_loc and B_loc)."""
    def run(hip, oracle):
        from eigenkernel_amd import descriptor as d
        from test_host_logic import virtual_allgatherv
        generalized = name.startswith("general_")
        A, B = _pair(generalized, n)
        nprow, npcol = grid
        out = []
        if inputs == "distributed":
            nbu = int(d.setup_distributed_matrix(n, n, nprow, npcol, 0, 0, block_size=32)[0][d.BLOCK_ROW_])
            hook = virtual_allgatherv([A, B] if generalized else [A], nbu, nprow, npcol)
            hip.set_allgatherv(hook)
        try:
            for rank in range(nprow * npcol):
                _, _, myrow, mycol = d.make_process_grid(rank, nprow * npcol, nprow, npcol)
                proc = hip.Process(rank, nprow * npcol, 0, nprow, npcol, myrow, mycol)
                tag = "%d%d" % (myrow, mycol)
                if inputs == "distributed":
                    hook.state["rank"] = rank
                    ep, _ = hip.eigen_solver(name, A, B, n_vec=n_vec, block_size=32, proc=proc, inputs="distributed")
                    out += [("Z" + tag, _sha(ep.Vectors)), ("A" + tag, _sha(ep.A_loc))]
                    out += [("B" + tag, _sha(ep.B_loc))] if generalized else []
                else:
                    ep, _ = hip.eigen_solver(name, A, B, n_vec=n_vec, block_size=32, proc=proc)
                    out += [("Z" + tag, _sha(ep.Vectors)), ("w" + tag, _sha(ep.values))]
        finally:
            if inputs == "distributed":
                hip.set_allgatherv(None)
        return out
    return run


def _comm_of_one(problem, n):
    """A communicator of one rank attached, a 1 x 1 grid cell: with EK_HIP_DIST_MIN_RANKS=1 the `dist` arm of every stage."""
    def run(hip, oracle):
        hip.comm_init(hip.comm_unique_id(), 1, 0)
        try:
            return _device(n, n, cell=(1, 1, 0, 0), problem=problem, nb=64)(hip, oracle)
        finally:
            hip.comm_destroy()
    return run


def _sig6(x):
    return float("%.6g" % x)


def _value_window(generalized, n, kind):
    """(vl, vu] from midpoints between eigenvalues 17 / 18 and 210 / 211 (6 significant digits): kind "pairs", "values",
    "empty" (an interval between eigenvalues 17 and 18), "short" (zcap = m - 1 through the C entry: -18, m and ifirst
    come back, w and Z keep the caller's fill)."""
    def run(hip, oracle):
        import ctypes
        A, B = _pair(generalized, n)
        w = hip.eigenvalues(A, B)
        vl, vu = _sig6(0.5 * (w[16] + w[17])), _sig6(0.5 * (w[209] + w[210]))
        if kind == "empty":
            vl, vu = w[16] + (w[17] - w[16]) / 3, w[16] + 2 * (w[17] - w[16]) / 3
        if kind != "short":
            ww, Z, first = hip.eigenpairs(A, B, vl=vl, vu=vu, vectors=kind != "values")
            return [("m", "%d" % len(ww)), ("first", "%d" % first), ("w", _sha(ww))] + \
                   ([("Z", _sha(Z))] if Z is not None else [])
        m = int(np.count_nonzero((w > vl) & (w <= vu)))
        Af, Bf = np.asfortranarray(A), (np.asfortranarray(B) if generalized else None)
        wf, Zf = np.full(n, 7.5), np.full((n, m - 1), 7.5, order="F")
        mo, fo = ctypes.c_int(0), ctypes.c_int(0)
        info = hip.load_library().ek_hip_eigenpairs(1 if generalized else 0, 1, 1, n, ctypes.c_double(vl),
                                                    ctypes.c_double(vu), 1, n, hip._P(Af), n,
                                                    hip._P(Bf) if generalized else None, n, ctypes.byref(mo),
                                                    ctypes.byref(fo), hip._P(wf), hip._P(Zf), n, m - 1, None, 0)
        return [("info", "%d" % info), ("m", "%d" % mo.value), ("first", "%d" % fo.value),
                ("w_untouched", "%d" % bool((wf == 7.5).all())), ("Z_untouched", "%d" % bool((Zf == 7.5).all()))]
    return run


def _sygvx(n, itype, il=None, iu=None, vectors=True):
    def run(hip, oracle):
        A, B = _pair(True, n)
        w, Z, first = hip.sygvx(A, B, itype=itype, il=il, iu=iu, vectors=vectors)
        return [("w", _sha(w)), ("first", "%d" % first)] + ([("Z", _sha(Z))] if vectors else [])
    return run


def _select(n, n_vec):
    def run(hip, oracle):
        A, B = _pair(True, n)
        ep, _ = hip.eigen_solver("general_hip_select", A, B, n_vec=n_vec)
        return [("w", _sha(ep.values)), ("Z", _sha(ep.Vectors))]
    return run


def _standard(n, change, before=None):
    """A standard solve of change(A); before(lib) runs first; the band short cut's mark (last_solve_stats()[3]) is added."""
    def run(hip, oracle):
        A = change(_pair(False, n)[0])
        if before:
            before(hip.load_library())
        ep, _ = hip.eigen_solver("hip", A)
        return [("w", _sha(ep.values)), ("Z", _sha(ep.Vectors)), ("band", "%d" % hip.last_solve_stats()[3])]
    return run


def _band64(A):
    i = np.arange(A.shape[0])
    return np.where(np.abs(i[:, None] - i[None, :]) <= 64, A, 0.0)


def _host_lld(n, lld):
    """ek_hip_solve on the 1 x 1 grid with local arrays of lld rows: w, Z and what is left in A and B."""
    def run(hip, oracle):
        from eigenkernel_amd import descriptor as d
        A, B = _pair(True, n)
        desc = d.descinit(n, n, 64, 64, 0, 0, 0, lld)
        Al, Bl, Zl, w = _rows(A, lld), _rows(B, lld), np.zeros((lld, n), order="F"), np.zeros(n)
        info = hip.load_library().ek_hip_solve(1, n, n, hip._P(Al), hip._I(desc), hip._P(Bl), hip._I(desc), hip._P(w),
                                               hip._P(Zl), hip._I(desc), 1, 1, 0, 0, None, 0)
        return [("info", "%d" % info), ("w", _sha(w)), ("Z", _sha(Zl)), ("A", _sha(Al)), ("B", _sha(Bl))]
    return run


PAIRS = {"EK_SY2SB_PAIR_MIN": "1"}
SWEEPS = {"EK_SB2ST_CHASE": "1"}
# (label, switches set for it, thunk, runs in a process of its own)
CASES = []
for _g, _tag in ((False, "standard"), (True, "generalized")):
    CASES += [("solve %s n=130" % _tag, {}, _solve(_g, 130), False),
              ("solve %s n=600" % _tag, {}, _solve(_g, 600), False),
              ("solve %s n=600 pairs" % _tag, PAIRS, _solve(_g, 600), False),
              ("solve %s n=600 sweeps" % _tag, SWEEPS, _solve(_g, 600), True),
              ("values %s n=600" % _tag, {}, _values(_g, 600), False),
              ("window %s n=600 il=17 iu=210" % _tag, {}, _window(_g, 600, 17, 210), False)]
CASES += [("solve standard n=5200", {}, _solve(False, 5200), False),
          ("solve generalized n=5200", {}, _solve(True, 5200), False),
          ("solve standard n=8320 Z(:,0:256)", {}, _solve(False, 8320, 256), False)]
for _n in (300, 4097):
    CASES += [("potrf n=%d" % _n, {}, _potrf(_n), False)]
    CASES += [("sygst type %d n=%d" % (_t, _n), {}, _sygst(_n, _t), False) for _t in (1, 2, 3)]
CASES += [("sytrd n=257", {}, _sytrd(257), False),
          ("sy2sb n=449", {}, _sy2sb(449), False),
          ("sy2sb n=449 pairs", PAIRS, _sy2sb(449), False),
          ("sy2sb_team n=449 team=3", {}, _sy2sb(449, 3), False),
          ("sytrd_team n=449 team=3", {}, _sytrd(449, 3), False),
          ("potrf_team n=449 team=3", {}, _potrf_team(449, 3), False),
          ("sygst_team n=449 team=3", {}, _sygst_team(449, 3), False)]
PIPE = {"EK_HIP_PIPE_MIN": "256"}
CASES += [("device generalized n=640 ld=640", {}, _device(640, 640), False),
          ("device generalized n=640 ld=640 copied", {"EK_HIP_ALIAS": "0"}, _device(640, 640), False),
          ("device generalized n=600 ld=603", {}, _device(600, 603), False),
          ("grid 2x2 generalized n=600", {}, _grid("general_hip", 600, (2, 2)), False),
          ("grid 2x2 standard n=130", {}, _grid("hip", 130, (2, 2)), False),
          ("grid 1x3 select n=640 n_vec=77", {}, _grid("general_hip_select", 640, (1, 3), 77), False),
          ("device_grid 2x2 cell (1,0) generalized n=600", {}, _device(600, 600, cell=(2, 2, 1, 0)), False),
          ("hook 2x2 generalized n=600", {}, _grid("general_hip", 600, (2, 2), inputs="distributed"), False),
          ("communicator of one generalized n=600", {"EK_HIP_DIST_MIN_RANKS": "1"}, _comm_of_one(1, 600), False),
          ("communicator of one standard n=130", {"EK_HIP_DIST_MIN_RANKS": "1"}, _comm_of_one(0, 130), False)]
for _g, _tag in ((False, "standard"), (True, "generalized")):
    CASES += [("value window %s n=600 %s" % (_tag, _k), {}, _value_window(_g, 600, _k), False)
              for _k in ("pairs", "values", "empty", "short")]
for _t in (2, 3):
    CASES += [("sygvx type %d n=600 il=17 iu=210" % _t, {}, _sygvx(600, _t, 17, 210), False),
              ("sygvx type %d n=600" % _t, {}, _sygvx(600, _t), False)]
CASES += [("sygvx type 2 n=600 values", {}, _sygvx(600, 2, vectors=False), False),
          ("select generalized n=640 n_vec=64", {}, _select(640, 64), False),
          ("band input n=600", {}, _standard(600, _band64), False),
          ("band input n=600 no short cut", {"EK_HIP_BAND_INPUT": "0"}, _standard(600, _band64), False),
          ("scaled up standard n=130", {}, _standard(130, lambda A: A * 1e200), False),
          ("scaled down standard n=130", {}, _standard(130, lambda A: A * 1e-200), False),
          ("chase repeated standard n=600", {}, _standard(600, lambda A: A, lambda lib: lib.ek_hip_debug_fail_next_chase(1)), False),
          ("pipeline standard n=600", PIPE, _solve(False, 600), False),
          ("pipeline generalized n=600", PIPE, _solve(True, 600), False),
          ("pipeline generalized n=600 lld=603", PIPE, _host_lld(600, 603), False)]
LABELS = [c[0] for c in CASES]


def line_of(case, hip, oracle):
    """The case's line of the file: label, switches, key=digest ... (two spaces between the three fields)."""
    label, env, run, _ = case
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        out = run(hip, oracle)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    switches = " ".join("%s=%s" % kv for kv in sorted(env.items())) or "-"
    return "%s  %s  %s" % (label, switches, " ".join("%s=%s" % kv for kv in out))


def read_digests(path=DIGESTS):
    out = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            out[line.split("  ")[0]] = line.rstrip("\n")
    return out


def test_the_file_holds_every_case_but_the_dropped_ones():
    """At most two cases may be missing (those whose two runs on the parent differed; DESIGN.md names them)."""
    have = set(read_digests())
    assert have <= set(LABELS)
    assert len(set(LABELS) - have) <= 2, sorted(set(LABELS) - have)


@pytest.mark.parametrize("label", LABELS)
def test_every_digest_of_the_parent_is_reproduced(hip, oracle, label):
    want = read_digests()
    if label not in want:
        return                                                 # (dropped on the parent: see the test above)
    case = CASES[LABELS.index(label)]
    if case[3]:
        got = subprocess.run([sys.executable, TOOL, "--only", label], stdout=subprocess.PIPE, check=True,
                             universal_newlines=True).stdout.strip()
    else:
        got = line_of(case, hip, oracle)
    print(got)
    assert got == want[label]
