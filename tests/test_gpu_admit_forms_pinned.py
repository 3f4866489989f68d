"""The admission family held to a recorded run of the commit its refactor started from: tests/admit_forms_cases.py's matrix -- every
act_redeem_(cbor_)*_batch entry point of the family, host and device memory, the empty batch, one lane, 70 valid lanes (nothing shed),
70 shed lanes, and a 300-lane mix of everything a screen, a copy stage and a tail tell apart; wire with offsets, without them where
every message is canonical, and the mix under both wire readers -- replayed against the built library and compared field by field with
tests/golden/admit_forms_L8.json: rc, statuses, out_key, replay marks and counts verbatim (with the guard bytes around them), SHA-256
of the output allocation and of each set's sorted (key, epoch) pairs.  Every call runs under a time limit of its own."""
import json
import os
import subprocess

import pytest

import admit_forms_cases as fc
from conftest import GOLDEN, ROOT
from test_gpu_replay import step

pytestmark = pytest.mark.gpu

_state = {}


def fixture_cases():
    if "want" not in _state:
        with open(os.path.join(GOLDEN, "admit_forms_L8.json")) as f:
            _state["fixture"] = json.load(f)
        _state["want"] = fc.unpack(_state["fixture"])
    return _state["fixture"], _state["want"]


def rig(engine_factory, tmp_path_factory):
    if "rig" not in _state:
        from act_amd import capi
        with step(120, "tokens, proofs and the sets every case starts from"):
            _state["rig"] = fc.Rig(capi, str(tmp_path_factory.mktemp("admit_forms")), make_engine=engine_factory)
    return _state["rig"]


def test_the_fixture_was_recorded_from_another_commit():
    fixture, want = fixture_cases()
    assert (fixture["L"], fixture["max_batch"]) == (fc.L, fc.MAX_BATCH) and len(fixture["recorded_from"]) == 40
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if r.returncode == 0:                                           # (an exported tree has no history to ask)
        assert r.stdout.strip() != fixture["recorded_from"], "the fixture must come from the parent's library, never from the one under test"
    assert len(want) == 270 and len(json.dumps(fixture)) < 200_000


@pytest.mark.parametrize("form,wire,mem", fc.matrix())
def test_every_form_answers_as_recorded(engine_factory, tmp_path_factory, form, wire, mem):
    _, want = fixture_cases()
    r = rig(engine_factory, tmp_path_factory)
    cases = fc.variants(r, form, wire, mem)
    assert cases and all(cid in want for cid, *_ in cases)
    for cid, name, offsets_given, reader in cases:
        with step(60, cid):
            got = fc.run_case(r, form, wire, mem, name, offsets_given, reader)
        for field in ("rc", "counts", "status", "out_key", "replayed", "out_sha256", "set_sha256", "receipts_sha256"):
            assert got[field] == want[cid][field], (cid, field, got[field], want[cid][field])
    assert r.eng.secret_residue() == 0
