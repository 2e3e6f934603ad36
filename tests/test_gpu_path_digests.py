"""Bit identity of the one-problem path with the build before csrc/ek_switch.h ("Run-time switches"):
tests/golden/path_anchor_digests.txt holds, per case, the first 16 hex digits of the SHA-256 of every output, written by
tools/path_digests.py on a build of that parent commit, and every one must be reproduced.  (The band -> tridiagonal
stage on its own has tests/golden/q2_anchor_digests.txt.)

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
