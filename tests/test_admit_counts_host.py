"""The out_counts of the admission family on the CPU: csrc/admit_counts.h compiled by g++ into one stand-alone program
(tests/hostcheck/admit_counts_check.cpp) that carries hand-written count vectors for all eight forms -- the empty batch, everything shed,
nothing shed, a mix, a copy served, a copy behind a non-zero leader, a copy that names another amount, amounts null, and a replay tail
that did not run (tc[0] != mv).  The same program runs once more under ASan + UBSan.  The eight lengths are held to the ACT_*_COUNTS
macros of include/act_mi355x.h and to the binding's name tuples."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
# the program's name of a form -> (the header's macro, the binding's tuple)
FORMS = {"admit": ("ACT_ADMIT_COUNTS", "ADMIT_COUNTS"), "admit_unique": ("ACT_ADMIT_UNIQUE_COUNTS", "ADMIT_UNIQUE_COUNTS"),
         "return": ("ACT_REDEEM_RETURN_COUNTS", "REDEEM_RETURN_COUNTS"), "return_unique": ("ACT_REDEEM_RETURN_UNIQUE_COUNTS", "REDEEM_RETURN_UNIQUE_COUNTS"),
         "admit_replay": ("ACT_ADMIT_REPLAY_COUNTS", "ADMIT_REPLAY_COUNTS"), "admit_replay_unique": ("ACT_ADMIT_REPLAY_UNIQUE_COUNTS", "ADMIT_REPLAY_UNIQUE_COUNTS"),
         "return_replay": ("ACT_RETURN_REPLAY_COUNTS", "RETURN_REPLAY_COUNTS"),
         "return_replay_unique": ("ACT_RETURN_REPLAY_UNIQUE_COUNTS", "RETURN_REPLAY_UNIQUE_COUNTS")}


def build_check(out, sanitize=False):
    src = os.path.join(ROOT, "tests", "hostcheck", "admit_counts_check.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src], check=True)
    return out


def lengths(stdout):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^LEN (\w+) (\d+)$", stdout, flags=re.M)}


def test_hand_written_counts_and_the_eight_lengths(tmp_path):
    exe = build_check(str(tmp_path / "admit_counts_check"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ADMIT COUNTS CHECK: 0 failures" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    hdr = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    macros = {name: int(v) for name, v in re.findall(r"^#define (ACT_\w+_COUNTS) (\d+)$", hdr, flags=re.M)}
    from act_amd import capi
    got = lengths(r.stdout)
    assert set(got) == set(FORMS)
    for form, (macro, names) in FORMS.items():
        assert got[form] == macros[macro] == len(getattr(capi, names)), form


def test_the_same_under_asan_ubsan(tmp_path):
    """a stand-alone program linked with the sanitizers: every input array and every count vector in a heap block of exactly its size"""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this toolchain links no sanitizer runtime")
    exe = build_check(str(tmp_path / "admit_counts_check_asan"), sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ADMIT COUNTS CHECK: 0 failures" in r.stdout, (r.stdout[-3000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


def test_the_counts_are_written_once():
    """the header is plain C++ in the library's dependencies, and the engine holds no count length and no counting loop of its own"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "admit_counts.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1).split()
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    hdr = strip(open(os.path.join(CSRC, "admit_counts.h")).read())
    assert "hip" not in hdr.lower()
    for f in ("admit_impl.inc", "admit_replay_impl.inc", "copies_impl.inc"):
        src = strip(open(os.path.join(CSRC, f)).read())
        assert not re.search(r"ACT_\w+_COUNTS", src.replace("ACT_REPLAY_COUNTS", "")), f      # (ACT_REPLAY_COUNTS: the replay tail's own array)
        assert "admit_counts_of" not in src and "admit_replay_counts_of" not in src, f
    assert "admit_counts(" in strip(open(os.path.join(CSRC, "admit_impl.inc")).read())
