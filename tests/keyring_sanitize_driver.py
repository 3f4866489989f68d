"""Runs inside a subprocess started by tests/test_keyring_host.py with libasan preloaded: the ring lane bodies and the incremental
hash of the AddressSanitizer + UBSan build of tests/hostcheck/keyring_check.cpp over the lane mix (L = 3 and 64) and every transcript
length.  Any report aborts the process."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from oracle_c import Oracle, build  # noqa: E402
import keyring_cases as kr  # noqa: E402

if __name__ == "__main__":
    build()
    o = Oracle()
    kc = C.CDLL(sys.argv[1])
    h = o.params_new("bench-org", "bench-service", "bench-env", "2024-01-01")
    kr.check_lane_bodies(kc, o, h, Ls=(3, 64))
    kr.check_incremental_hash(kc, o)
    print("KEYRING SANITIZERS CLEAN")
