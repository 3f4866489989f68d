"""The settle window of the host reader's road on the CPU: csrc/wire_window.h (the gather plan, the parse step, the lane-patch plan)
over csrc/cbor_reader.h, compiled by g++ into one stand-alone program (tests/hostcheck/wire_window_check.cpp) whose copier is memcpy
out of a "device" buffer of exactly the batch's size.  The program carries the gather and patch cases itself; the parse step runs over
a short corpus of IssuanceRequest spellings (the corpus of tests/test_issue_wire_read_host.py, thinned) with the code the Python model
of from_cbor gives each.  The same program runs once more under ASan + UBSan."""
import os
import re
import struct
import subprocess

import pytest

import pymodel as m
from conftest import ROOT
from test_issue_wire_read_host import CSRC, L, T, corpus  # noqa: F401  (corpus: the module's fixture)


def build_check(out, sanitize=False):
    src = os.path.join(ROOT, "tests", "hostcheck", "wire_window_check.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def short_corpus(corpus):  # noqa: F811
    """every message of the other sections, every seventh prefix: (message, the model's code)"""
    msgs = [msg for sec, msg in corpus if sec != "prefix"] + [msg for sec, msg in corpus if sec == "prefix"][::7]
    out = [(msg, m.cbor_decode(T, msg, L)[0]) for msg in msgs]
    assert {c for _, c in out} == {0, 1, 2, 3} and 40 < len(out) < 400
    return out


def _write(short_corpus, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", L))
        for msg, code in short_corpus:
            f.write(struct.pack("<I", len(msg))); f.write(msg); f.write(bytes([code]))


def test_gather_patch_and_parse(short_corpus, tmp_path):
    exe = build_check(str(tmp_path / "wire_window_check"))
    _write(short_corpus, str(tmp_path / "corpus.bin"))
    r = subprocess.run([exe, str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WIRE WINDOW CHECK: 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "parsed %d messages" % len(short_corpus) in r.stdout


def test_the_same_under_asan_ubsan(short_corpus, tmp_path):
    """a stand-alone program linked with the sanitizers: the "device" bytes, the gathered bytes and every patched array in a heap block
    of exactly its size"""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this toolchain links no sanitizer runtime")
    exe = build_check(str(tmp_path / "wire_window_check_asan"), sanitize=True)
    _write(short_corpus, str(tmp_path / "corpus.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "corpus.bin")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "WIRE WINDOW CHECK: 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


def test_the_window_exists_once():
    """the header is plain C++ beside cbor_reader.h and is in the library's dependencies; the three settles go through it"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wire_window.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1).split()
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    hdr = strip(open(os.path.join(CSRC, "wire_window.h")).read())
    assert '#include "cbor_reader.h"' in hdr and "hip" not in hdr.lower()
    src = {f: strip(open(os.path.join(CSRC, f)).read()) for f in ("cbor_impl.inc", "admit_impl.inc", "issue_wire_impl.inc")}
    assert '#include "wire_window.h"' in src["cbor_impl.inc"]
    assert all(s.count("wire_window_read(") >= 1 for s in src.values())
    assert sum(s.count("cbor_read_message(") for s in src.values()) == 1      # act_cbor_decode_batch's, inside its chunk
    assert "ADMIT_READ_WINDOW" not in src["admit_impl.inc"] and sum(s.count("constexpr size_t WIRE_SETTLE_WINDOW") for s in src.values()) == 0
    assert not any("CBOR_ERR_PARSE ?" in s for s in src.values())             # one spelling of code -> status: act::cbor_code_status
