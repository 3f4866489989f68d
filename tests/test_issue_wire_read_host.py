"""The issuance side of the device wire reader on the CPU: what a chunk of act_issue_cbor_batch does with one IssuanceRequest message
under ACT_WIRE_READER_DEVICE -- flag lane, plain pass, validating pass, take-up with scalar reduction, status override
(csrc/issue_wire_lanes.h over csrc/cbor_lanes.h) -- against the host road it replaces (cbor_read_message, the ordering of
cbor_settle_codes, decode_scalar), both compiled by g++ into one stand-alone program (tests/hostcheck/issue_wire_read_check.cpp) that
compares flag, status and all 128 record bytes, and against the Python model of from_cbor.  The same program runs once more under
ASan + UBSan with every message in a heap block of exactly its size."""
import os
import re
import struct
import subprocess

import pytest

import pymodel as m
from conftest import ROOT
from test_cbor import _variants
from test_cbor_read_host import BAD_PT, record

CSRC = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
L = 8                                  # (an IssuanceRequest does not depend on L)
WIRE = {0: 0, 1: 254, 2: 253, 3: 255}  # from_cbor's result as a lane status
T = "IssuanceRequest"


def build_check(out, sanitize=False):
    src = os.path.join(ROOT, "tests", "hostcheck", "issue_wire_read_check.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src], check=True)
    return out


def _template():
    """the canonical message and the offsets of its four payloads, found by encoding a record of four distinct marker fields"""
    marks = [bytes([0xC1 + i]) * 32 for i in range(4)]
    enc = m.cbor_encode(T, b"".join(marks), L)
    offs = [enc.index(x) for x in marks]
    assert len(enc) == 141 and offs == sorted(offs)
    return enc, offs


def _ents(rec):
    return [(key, b"\x58\x20" + rec[32 * i:32 * i + 32]) for i, (key, _, _) in enumerate(m.CBOR_TYPES[T])]


def _body(es):
    return b"".join(m._cbor_head(0, k) + v for k, v in es)


@pytest.fixture(scope="module")
def corpus():
    """(section, message)"""
    rec = record(T, L)
    enc = m.cbor_encode(T, rec, L)
    es = _ents(rec)
    indef = b"\xbf" + _body(es) + b"\xff"
    c = [("variants", v) for v, _ in _variants(T, rec, L)]
    c += [("canonical", enc), ("trailing", enc + b"\x00")]
    for f in (1, 2, 3):                                      # every scalar field unreduced, in a canonical message and in a respelled one
        for big in (m.ELL + 1, 2**256 - 1):
            r2 = rec[:32 * f] + big.to_bytes(32, "little") + rec[32 * f + 32:]
            c += [("unreduced", m.cbor_encode(T, r2, L)), ("unreduced", b"\xbf" + _body(_ents(r2)) + b"\xff")]
    bad_k = BAD_PT + rec[32:]
    c += [("bad-k", m.cbor_encode(T, bad_k, L)), ("bad-k", b"\xbf" + _body(_ents(bad_k)) + b"\xff"), ("bad-k", m._cbor_head(5, 4) + _body(_ents(bad_k)[::-1]))]
    dup = m._cbor_head(0, es[0][0]) + b"\x58\x20" + BAD_PT    # an invalid point that a duplicate key keeps out of the record
    c += [("hidden", m._cbor_head(5, 5) + dup + _body(es)), ("hidden", b"\xbf" + dup + _body(es) + b"\xff"),
          ("hidden", m._cbor_head(5, 5) + m._cbor_head(0, es[0][0]) + es[0][1] + _body(_ents(bad_k)))]      # ... and the other way round: the last one wins
    c += [("prefix", enc[:i]) for i in range(len(enc))] + [("prefix", indef[:i]) for i in range(len(indef))]
    return c


def _write(corpus, path):
    tmpl, offs = _template()
    with open(path, "wb") as f:
        f.write(struct.pack("<II", L, len(tmpl))); f.write(tmpl); f.write(struct.pack("<4I", *offs))
        for _, msg in corpus:
            f.write(struct.pack("<I", len(msg))); f.write(msg)


def _read(corpus, path):
    blob = open(path, "rb").read()
    assert len(blob) == 136 * len(corpus)
    keys = ("spec_flag", "lane_flag", "spec_status", "lane_status", "mismatch", "plain", "code", "info")
    return [dict(zip(keys, blob[136 * i:136 * i + 8]), rec=blob[136 * i + 8:136 * i + 136]) for i in range(len(corpus))]


@pytest.fixture(scope="module")
def results(corpus, tmp_path_factory):
    d = tmp_path_factory.mktemp("issue_wire_read")
    exe = build_check(str(d / "issue_wire_read_check"))
    _write(corpus, str(d / "corpus.bin"))
    r = subprocess.run([exe, str(d / "corpus.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1) and "ISSUE WIRE READ CHECK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    return _read(corpus, str(d / "out.bin")), r


def test_the_corpus_holds_every_class(corpus, results):
    """the classification is the specification's alone: a corpus of nothing but parse errors would show nothing"""
    res, _ = results
    classes = {
        "canonical": [r for r in res if r["spec_flag"] == 0],
        "respelled and accepted": [r for r in res if r["spec_flag"] == 0x80 and r["spec_status"] == 0],
        "CBOR_ERR_PARSE": [r for r in res if r["code"] == 1],
        "CBOR_ERR_STRUCTURE": [r for r in res if r["code"] == 2],
        # the plain pass decodes no point: on the plain road an invalid value is a message that reads (code 0, no validating pass
        # wanted) and whose K the take-up then fails to decode -- canonical or respelled
        "CBOR_ERR_VALUE from the plain road": [r for r in res if r["code"] == 0 and r["spec_status"] == 255],
        "CBOR_ERR_VALUE that only the validating pass finds": [r for r in res if r["plain"] != 3 and r["code"] == 3],
    }
    assert all(classes.values()), {k: len(v) for k, v in classes.items()}
    assert any(r["spec_flag"] == 0x80 for r in classes["CBOR_ERR_VALUE from the plain road"]) and any(r["spec_flag"] == 0 for r in classes["CBOR_ERR_VALUE from the plain road"])
    assert any(r["info"] & 1 for r in res) and any(r["info"] & 2 for r in res)      # irregular messages and points in front of a fault occur
    sec = lambda name: [r for (s, _), r in zip(corpus, res) if s == name]
    assert {r["spec_status"] for r in sec("unreduced")} == {0} and {r["spec_flag"] for r in sec("unreduced")} == {0, 0x80}
    assert {r["spec_status"] for r in sec("hidden")} == {255} and {r["spec_status"] for r in sec("bad-k")} == {255}
    assert [r["spec_flag"] for r in sec("canonical") + sec("trailing")] == [0, 0] and {r["spec_status"] for r in sec("prefix")} == {254}


def test_device_road_equals_the_host_road(corpus, results):
    res, run = results
    bad = [(i, corpus[i][0], r, corpus[i][1][:24].hex()) for i, r in enumerate(res)
           if r["mismatch"] or r["spec_flag"] != r["lane_flag"] or r["spec_status"] != r["lane_status"]]
    assert not bad and run.returncode == 0 and "0 mismatches" in run.stdout, (bad[:10], run.stderr[-2000:])


def test_unreduced_scalars_come_out_reduced(corpus, results):
    res, _ = results
    seen = 0
    for (sec, msg), r in zip(corpus, res):
        if sec != "unreduced":
            continue
        fields = [int.from_bytes(r["rec"][32 * f:32 * f + 32], "little") for f in (1, 2, 3)]
        assert all(v < m.ELL for v in fields) and (1 in fields or (2**256 - 1) % m.ELL in fields), msg[:8].hex()
        seen += 1
    assert seen == 12


def test_corpus_against_the_model(corpus, results):
    res, _ = results
    seen = set()
    for (sec, msg), r in zip(corpus, res):
        es, er = m.cbor_decode(T, msg, L)
        assert (r["lane_status"], r["rec"]) == (WIRE[es], er), (sec, r, es, msg[:24].hex())
        seen.add(es)
    assert seen == {0, 1, 2, 3}


def test_the_header_is_in_both_libraries():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hdrs = re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1).split()
    assert {"issue_wire_lanes.h", "cbor_lanes.h", "cbor_reader.h"} <= set(hdrs)
    assert '#include "issue_wire_lanes.h"' in open(os.path.join(CSRC, "k_sign.hip")).read()
    lanes = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "issue_wire_lanes.h")).read())
    assert "std::vector" not in lanes and "__device__" not in lanes      # plain ACT_HD bodies: what g++ compiles is what the kernels run


def test_whole_corpus_under_asan_ubsan(corpus, tmp_path):
    """a stand-alone program linked with the sanitizers: every message and record in a heap block of exactly its size"""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this toolchain links no sanitizer runtime")
    exe = build_check(str(tmp_path / "issue_wire_read_check_asan"), sanitize=True)
    _write(corpus, str(tmp_path / "corpus.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
