"""Runs inside a subprocess started by tests/test_admission_host.py with libasan preloaded: every check of tests/admission_cases.py
over the AddressSanitizer + UBSan build of tests/hostcheck/admit_check.cpp.  Any report aborts the process."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import admission_cases as ad  # noqa: E402
from test_cbor import _variants  # noqa: E402

if __name__ == "__main__":
    ac = C.CDLL(sys.argv[1])
    with open(os.path.join(ROOT, "tests", "golden", "lifecycle_L128.json")) as f:
        g = json.load(f)
    records = [bytes.fromhex(c["proof"]) for c in g["cases"][:2]]
    ad.check_all_lane_bodies(ac, records, 128, lambda rec: _variants("SpendProof", rec, 128))
    print("ADMISSION SANITIZERS CLEAN")
