"""The environment switches of libmpdx.so have ONE source, csrc/switches.hpp: nothing else in the library reads the environment, the
table lists exactly the known names, INTEGRATION.md documents every row with the same default and timing, every MPDX_* variable the
tests and tools set is accounted for, and the parse kinds do what the scattered getenv sites they replaced did (checked on the host:
the header is plain C++17).  No GPU."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mpd_public_amd" / "csrc"

NAMES = """BWD_DBG DEBUG DEBUG_FUSE DEBUG_TRAIN FUSED FUSED_MASK GEO GUIDE_DENSE KSPLIT
   LDS_CAP_KB MERGE_DOWN3 NO_MERGE NO_MERGE_UP NO_MID2 NO_MID3 PAIR
   STATIC_PROGRAMS TARGET_WGS TILE TIME_TAIL_SPLIT
   TRAIN_BWD_PROG TRAIN_BWD_PROG_MAX_B TRAIN_DEFERRED
   TRAIN_GN_FUSE TRAIN_REDUCE_JOIN TRAIN_RESTREAM_RIDE
   TRAIN_WGRAD_LATE TRAIN_WGRAD_MULTI WGRAD_LATE_DIV WGRAD_PROG_MUL WS WSN
   WSN_MIN_B WSP WSP_MIN_B WS_NS""".split()

ROW = re.compile(r'^\s*X\(\s*(\w+),\s*"(MPDX_\w+)",\s*(\w+),\s*([^,]+?),\s*(\w+),\s*"(.*)"\)\s*\\?$')
DOC_WORD = {"false": "unset", "nullptr": "unset", "kUnset": "unset", "true": "on"}   # a default as INTEGRATION.md writes it


def table():
    """name -> (accessor, kind, default, timing, description), scanned from the X-macro list."""
    text = (CSRC / "switches.hpp").read_text()
    body = text[text.index("#define MPDX_SWITCHES(X)"):text.index("// clang-format on")]
    rows = [m.groups() for m in map(ROW.match, body.splitlines()) if m]
    assert len(rows) == len(re.findall(r"^\s*X\(", body, re.M)), "a row of MPDX_SWITCHES does not scan"
    assert len({r[1] for r in rows}) == len(rows), "a switch is declared twice"
    return {name: (fn, kind, dflt.strip(), timing, doc) for fn, name, kind, dflt, timing, doc in rows}


def doc_section():
    text = (ROOT / "INTEGRATION.md").read_text()
    start = text.index("Environment switches of libmpdx.so")
    return text[start:text.index("\n## ", start)]


def test_getenv_only_in_switches_hpp():
    hits = [f"{p.name}:{i + 1}" for p in sorted(CSRC.iterdir()) if p.name != "switches.hpp"
            for i, line in enumerate(p.read_text(errors="replace").splitlines()) if "getenv" in line]
    assert not hits, hits


def test_table_is_the_known_set():
    t = table()
    assert sorted(t) == sorted("MPDX_" + n for n in NAMES) and len(t) == 36
    for name, (fn, kind, dflt, timing, doc) in t.items():
        assert fn == name[len("MPDX_"):].lower(), (name, fn)
        assert kind in ("PRESENT", "ON", "INT", "UINT", "STR") and timing in ("ONCE", "LIVE") and doc.strip(), name
        assert {"PRESENT": dflt == "false", "ON": dflt == "true", "STR": dflt == "nullptr"}.get(kind, True), (name, kind, dflt)


def test_every_row_is_documented_and_vice_versa():
    t = table()
    doc = {}
    for line in doc_section().splitlines():
        m = re.match(r"^\| `(MPDX_\w+)` \| (\w+) \| ([^|]+?) \| (once|live) \| (.+) \|$", line)
        if m:
            assert m.group(1) not in doc, m.group(1)
            doc[m.group(1)] = m.groups()[1:]
    assert sorted(doc) == sorted(t), sorted(set(doc) ^ set(t))
    for name, (fn, kind, dflt, timing, text) in t.items():
        want = (kind.lower(), DOC_WORD.get(dflt, dflt.rstrip("u")), timing.lower())
        assert doc[name][:3] == want, (name, doc[name][:3], want)


def test_every_variable_the_tests_and_tools_set_is_accounted_for():
    """An MPDX_* word in tests/, tools/*.py, tools/*.sh is a switch of the table, a Python-side variable the document lists with
    its reader, or a compile-time definition the document's closing line names."""
    sec = doc_section()
    py_side = sec[sec.index("Not the library's"):]
    known = set(table()) | set(re.findall(r"`(MPDX_\w+)`", py_side))
    files = sorted((ROOT / "tests").glob("*.py")) + sorted((ROOT / "tools").glob("*.py")) + sorted((ROOT / "tools").glob("*.sh"))
    used = {}
    for p in files:
        if p.name == Path(__file__).name:
            continue
        for w in re.findall(r"\bMPDX_[A-Z][A-Z0-9_]*[A-Z0-9]\b", p.read_text(errors="replace")):
            used.setdefault(w, p.name)
    used = {w: f for w, f in used.items() if not w.startswith("MPDX_E_") and not w.startswith("MPDX_ROBOT_") and not w.startswith("MPDX_FIELD_")}   # constants of include/mpdx.h
    assert len(used) >= 25
    unknown = {w: f for w, f in used.items() if w not in known}
    assert not unknown, unknown
    for w in ("MPDX_LIB", "MPDX_GATHER", "MPDX_TRAIN_GRAPH", "MPDX_TORCH_DATALOADER", "MPDX_BUILD_DEFS", "MPDX_TEST_THREADS", "MPDX_BENCH_TABLE",
              "MPDX_DEV_HOOKS", "MPDX_LOOP_ABLATION", "MPDX_GPMP_STAMPS", "MPDX_BWD_PAD4"):
        assert w in known and w not in table(), w


PROBE = r"""
#include "switches.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    using namespace mpdx;
    if (argc > 1) {   // timing: read, change the environment, read again
        const int once0 = sw::ksplit(), live0 = sw::ws();
        setenv("MPDX_KSPLIT", "1", 1); setenv("MPDX_WS", "2", 1);
        printf("once %d %d live %d %d\n", once0, sw::ksplit(), live0, sw::ws());
        return 0;
    }
    const char* tile = sw::tile();
    printf("no_merge %d pair %d ksplit %d fused_mask %u tile %s\n", (int)sw::no_merge(), (int)sw::pair(), sw::ksplit(), sw::fused_mask(), tile ? tile : "(null)");
    printf("target_wgs %d lds_cap_kb %d wsn_min_b %d wsp_min_b %d bwd_prog_max_b %d\n", sw::target_wgs(), sw::lds_cap_kb(), sw::wsn_min_b(),
           sw::wsp_min_b(), sw::train_bwd_prog_max_b());
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("switches")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", f"-I{CSRC}", "-o", str(d / "probe"), str(d / "probe.cpp")], check=True)

    def run(env, *args):
        base = {k: v for k, v in os.environ.items() if not k.startswith("MPDX_")}
        out = subprocess.run([str(d / "probe"), *args], env={**base, **env}, capture_output=True, text=True, check=True).stdout
        words = out.split()
        return dict(zip(words[::2], words[1::2])) if not args else out.strip()
    return run


def test_parse_kinds_on_the_host(probe):
    unset = probe({})
    assert unset["no_merge"] == "0" and unset["pair"] == "1" and unset["ksplit"] == "-1" and unset["fused_mask"] == str(0xffffffff) and unset["tile"] == "(null)"
    assert (unset["target_wgs"], unset["lds_cap_kb"], unset["wsn_min_b"], unset["wsp_min_b"], unset["bwd_prog_max_b"]) == \
        ("160", "96", "512", "512", "512")
    assert probe({"MPDX_NO_MERGE": "0"})["no_merge"] == "1"      # present: any value counts as set
    assert probe({"MPDX_NO_MERGE": ""})["no_merge"] == "1"
    for off in ("0", "", "x"):                                   # on: off when atoi of the value is 0 - "" and "x" too
        assert probe({"MPDX_PAIR": off})["pair"] == "0", off
    assert probe({"MPDX_PAIR": "1"})["pair"] == "1"
    assert probe({"MPDX_KSPLIT": "0"})["ksplit"] == "0" and probe({"MPDX_KSPLIT": "1"})["ksplit"] == "1"
    assert probe({"MPDX_FUSED_MASK": "0x5"})["fused_mask"] == "5" and probe({"MPDX_FUSED_MASK": "6"})["fused_mask"] == "6"
    assert probe({"MPDX_TILE": "32x64"})["tile"] == "32x64"
    assert probe({"MPDX_TARGET_WGS": "200", "MPDX_LDS_CAP_KB": "64"})["target_wgs"] == "200"


def test_once_keeps_its_first_value_and_live_follows(probe):
    assert probe({}, "timing") == "once -1 -1 live 1 2"
    assert probe({"MPDX_KSPLIT": "0", "MPDX_WS": "0"}, "timing") == "once 0 0 live 0 2"
