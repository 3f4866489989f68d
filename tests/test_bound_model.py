"""Request binding: the big-integer model of the bound form (tests/bound_cases.py) against its committed fixture, and the
properties of the construction that need no engine."""
import json
import os

import pymodel as pm

import bound_cases as bc
from conftest import GOLDEN


def test_the_fixture_is_what_the_model_makes():
    with open(os.path.join(GOLDEN, "bound_spend.json")) as f:
        want = json.load(f)
    assert bc.fixture() == want


def test_the_wrapper_appends_one_item_to_spend_transcripts_only():
    c = bc.case(bc.FIXTURE_L, "bound-fixture")
    params, items = c["params"], [bytes([i]) * 32 for i in range(4)]
    plain = pm.transcript_challenge(params, b"spend", items)
    with bc.bound(c["bind"]):
        assert pm.transcript_challenge(params, b"spend", items) == pm.sc_from_wide(pm.blake3(pm.transcript_preimage(params, b"spend", items) + bc.lp(c["bind"]), 64))
        assert pm.transcript_challenge(params, b"refund", items) == pm.sc_from_wide(pm.blake3(pm.transcript_preimage(params, b"refund", items), 64))
    assert pm.transcript_challenge(params, b"spend", items) == plain != 0
    assert len(bc.lp(c["bind"])) == 40 and bc.lp(c["bind"])[:8] == bytes(7) + b"\x20"


def test_bound_and_unbound_proofs_of_one_token_differ_only_behind_the_challenge():
    """same token, charge and rng bytes: every commitment (k, s, A', B_bar, Com_j) is the same, the challenge and every response differ;
    another binding, the all-zero one included, is another challenge"""
    c = bc.case(bc.FIXTURE_L, "bound-fixture")
    L = c["L"]
    a, b = c["proof_rec"], c["plain_rec"]
    head = 32 * (4 + L)
    assert a[:head] == b[:head] and a[head:head + 32] != b[head:head + 32]
    proof = c["proof"]
    for other in (bytes(32), bytes([c["bind"][0] ^ 1]) + c["bind"][1:]):
        with bc.bound(other):
            assert pm.spend_verify_challenge(c["sk"].x, c["params"], proof)[0] != proof.gamma
    with bc.bound(bytes(32)):      # an unbound proof is not a proof under the all-zero binding
        plain = pm.parse_spend_proof(b, L)
        assert pm.spend_verify_challenge(c["sk"].x, c["params"], plain)[0] != plain.gamma
    assert pm.spend_verify_challenge(c["sk"].x, c["params"], plain)[0] == plain.gamma
