"""Runs inside a subprocess started by tests/test_copies_host.py with libasan preloaded: every check of tests/copies_cases.py over the
AddressSanitizer + UBSan build of tests/hostcheck/copy_check.cpp.  Any report aborts the process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import copies_cases as cp  # noqa: E402

if __name__ == "__main__":
    cc = cp.load_copy_check(sys.argv[1])
    cp.check_all_lane_bodies(cc)
    print("COPIES SANITIZERS CLEAN")
