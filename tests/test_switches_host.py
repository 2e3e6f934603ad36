"""The library's run-time switches (eigenkernel_amd/csrc/ek_switch.h): one reader of the environment, one list of names in
the code and in the two documents a host reads, and the table's rules for unset, numeric, empty and non-numeric values and
for the moment of reading, checked by a stand-alone program under the host sanitizers.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eigenkernel_amd", "csrc")
NAME = re.compile(r"\bEK_[A-Z0-9]+_[A-Z0-9_]+\b")
READ = {"kOnce": "once", "kEachCall": "each call", "kOnceAndEachCall": "once and each call"}
# the switches this table replaced: experiments decided long ago (DESIGN.md says where each measurement is recorded)
REMOVED = ["EK_SYGST_FOLD", "EK_POTRF_OB", "EK_SB2ST_XCDMAP", "EK_SB2ST_TRACE", "EK_SB2ST_PROF", "EK_SB2ST_WAVES",
           "EK_SB2ST_VERBOSE", "EK_Q2_EXTRA", "EK_Q2_WGS", "EK_SY2SB_PROF", "EK_SY2SB_STAGED_MAX", "EK_GEMM_VEC",
           "EK_GEMM_W8", "EK_GEMM_RANKK", "EK_SYMV_WGS", "EK_SYMV_G", "EK_SYTRD_MAXCOLS", "EK_HIP_LDPAD"]
SOURCE = (".hip", ".h", ".py", ".c", ".cpp", ".f90", ".sh", ".md", ".txt", "Makefile")


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _table():
    """{name: read policy} from the rows of kSwitches."""
    rows = re.findall(r'\{"(EK_[A-Z0-9_]+)",\s*[^,]+,\s*(k\w+)\}', _read(os.path.join(CSRC, "ek_switch.h")))
    assert len(rows) == 20 and len(set(r[0] for r in rows)) == 20, rows
    return {name: READ[read] for name, read in rows}


def _listed(text):
    """{name: read policy} from a document's list: one switch per line, `name | default | read | meaning`."""
    out = {}
    for line in text.splitlines():
        cells = [c.strip(" `*") for c in line.split("|")]
        names = [c for c in cells if NAME.fullmatch(c)]
        if names:
            assert len(names) == 1 and names[0] not in out, line
            out[names[0]] = cells[cells.index(names[0]) + 2]
    return out


def test_one_unit_reads_the_environment():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")) and f != "ek_switch.h":
            assert "getenv" not in _read(os.path.join(CSRC, f)), f
    assert "getenv" in _read(os.path.join(CSRC, "ek_switch.h"))


def test_the_documents_list_the_table():
    table = _table()
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text[text.index("## 7. Environment switches"):text.index("**Which HIP runtime")]
    assert _listed(section) == table
    header = _read(os.path.join(ROOT, "include", "ek_hip.h"))
    assert _listed(header[header.index("Run-time switches"):]) == table


def test_the_removed_switches_are_gone():
    found = []
    tops = [os.path.join(ROOT, d) for d in ("eigenkernel_amd", "include", "tests", "tools", "host")]
    files = [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "INTEGRATION.md")]
    for top in tops:
        for d, _, fs in os.walk(top):
            files += [os.path.join(d, f) for f in fs if f.endswith(SOURCE)]
    for path in files:
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = _read(path)
        found += [(os.path.relpath(path, ROOT), n) for n in REMOVED if re.search(r"\b%s\b" % n, text)]
    assert not found, found


def test_the_table_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "switch_probe")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "switch_probe.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0 and run.stdout.strip() == "switch probe ok", (run.returncode, run.stdout, run.stderr)
