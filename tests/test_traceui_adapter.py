"""The reference-side binding of INTEGRATION.md §2: include/rtx_traceui.h's
adapter (TraceUI flags -> RtxRenderParams) is compiled against the
UNMODIFIED reference header ui/TraceUI.h (tests/native/
traceui_adapter_check.cpp: explicit instantiation + accessor signature
asserts), and for every parity-case flag set it yields the RtxRenderParams
that RenderOptions.from_cli (the Python mirror the GPU tests use) yields.

Where the reference's sources are present the checker is compiled and run,
and its rows must equal the record under tests/golden/ref_pins/
(tools/make_ref_pins.py).  Where they are absent the recorded rows stand in
for the compiled checker's, and hold only for the very adapter sources they
were recorded from (tests/ref_pins.py: adapter_sources_sha)."""
import os
import subprocess

import pytest

import ref_pins as rp
from cases import CASES
from conftest import ROOT

REF_UI = os.path.join(rp.REF_SRC, "ui")

EXTRA_FLAGS = [
    "-w 1920 -r 5 -O r -A 4", "-w 1024 -r 5 -O r -A 4", "-w 1920 -r 5 -O d -A 2.5 -B 16 -C 0.05",
    "-w 3840 -r 5 -O a -A 8", "-w 64 -O j -A 3", "-w 32 -O c -A 0.25 -O s -A 7", "-O g -O o -r 2",
    "-O a -A 5 -B 0.125", "-O d -A 0.5 -B 0 -C 0.2",
]


def flag_sets():
    return sorted({c[2] for c in CASES} | set(EXTRA_FLAGS))


def checker_command(exe):
    return ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", f"-I{REF_UI}", f"-I{ROOT}/include", "-o", exe,
            os.path.join(ROOT, "tests", "native", "traceui_adapter_check.cpp")]


def checker_rows(exe):
    """flag set -> the checker's row for it (buffer 97 + k wide, 61 + k high)"""
    fs = flag_sets()
    lines = [f"{97 + k} {61 + k} {f}" for k, f in enumerate(fs)]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = out.stdout.strip().splitlines()
    assert len(rows) == len(fs)
    return dict(zip(fs, rows))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the compiled checker, or None where only the record is there"""
    if not os.path.isdir(REF_UI):
        return None
    exe = str(tmp_path_factory.mktemp("adapter") / "traceui_adapter_check")
    subprocess.run(checker_command(exe), check=True)
    return exe


def test_adapter_matches_python_mirror(pkg, checker):
    rec = rp.pins()["traceui"]
    if checker is not None:
        rows = checker_rows(checker)
        assert rec["rows"] == rows  # the record is the compiled checker's answer
        assert rec["sources_sha256"] == rp.adapter_sources_sha()
    else:
        assert rec["sources_sha256"] == rp.adapter_sources_sha(), "the adapter changed since its rows were recorded"
        rows = rec["rows"]
    assert sorted(rows) == flag_sets()
    names = ["width", "height", "depth", "aa_mode", "aa_samples", "dof", "dof_div", "anaglyph", "ss_res",
             "overlapping", "aa_thresh", "aterm_thresh", "dof_fd", "dof_apsz", "tile", "shard", "nshards", "packed"]
    for k, flags in enumerate(flag_sets()):
        row = rows[flags]
        assert row != "ERROR", flags
        vals = row.split()
        p = pkg.RenderOptions.from_cli(flags.split()).params(61 + k)
        for name, v in zip(names, vals):
            want = getattr(p, name)
            if name == "width":  # the C++ side was given the buffer width, as traceImage(w, h) is
                want = 97 + k
            got = float(v) if isinstance(want, float) else int(v)
            assert got == want, (flags, name, got, want)
