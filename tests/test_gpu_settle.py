"""Settle on the GPU: act_redeem_settle_batch / act_redeem_cbor_settle_batch through the C ABI, behind the reserve calls
of tests/test_gpu_reserve.py (whose helpers and World this file uses: L = 8, s = 3, two proofs per nullifier).  Reserve + settle is held
to act_redeem_(cbor_)return_replay_batch on fresh sets, byte for byte, and to the model record of tests/refund_return_cases.py under the
nonces of tests/return_replay_cases.py; the receipts to the three keys of tests/reserve_cases.py.  Then retries, the pin, the bounds,
the failures, the client at L = 128 and the Python layer.  Both transcript modes with both memory kinds, records and wire, a ring of two
keys with epochs.  Every step runs under a time limit of its own.

One place where the two-phase road cannot be the one-phase call: a lane whose t exceeds s is ACT_STATUS_RETURN_TOO_BIG in both, but
reserve, which never sees t, has recorded its nullifier -- the reservation stays open until it is settled with an amount that fits.
The comparison below says so lane by lane, and then settles those lanes with t = s on both roads."""
import pytest

import reserve_cases as rc
from conftest import ELL, scb
from test_gpu_refund_return import records_of
from test_gpu_refund_return import world as world128
from test_gpu_replay import CREDIT, L, NONCE_KEY, SPEND, _pairs, call_replay, setup, step
from test_gpu_reserve import MODES, call_reserve, call_settle, kbytes, kprimes, model_receipts
from test_gpu_return_replay import amounts, call_rr, model_record, restored, snapshot

pytestmark = pytest.mark.gpu

S = SPEND


def reserved(eng, mem, ns, rs, ring, w, toks, epochs=None):
    """tokens reserved (variant 0) -> (records, key indices)"""
    got = call_reserve(eng, mem, ns, rs, ring, recs=[w.proof(t) for t in toks], key_epochs=epochs)
    assert got[0] == bytes(len(toks))
    return got[1], got[2]


# ---- 2. reserve + settle is the one-phase call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("n", [6, 65])
def test_reserve_and_settle_is_the_return_replay_call(engine_factory, bench_params, mode, mem, wire, n):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [41, 42]
    ts = amounts(n)                                                 # 1, s - 1, s cycling
    charges = [S + 1 if t % 9 == 4 else S for t in range(n)]       # every ninth lane is shed at the wrong price
    for t in range(2, n, 13):
        ts[t] = S + 1                                               # ... and a few name too much
    shed = {t: 250 if charges[t] != S else 249 for t in range(n) if charges[t] != S or ts[t] > S}
    big = [t for t in shed if shed[t] == 249]
    assert 250 in shed.values() and big
    recs = [w.proof(t) for t in range(n)]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    ns1, rs1 = capi.NullifierSet(1000), capi.NullifierSet(1000)
    spent, receipts = set(), set()
    with step(60, "reserve, settle, and the one-phase call on fresh sets"):
        res = call_reserve(eng, mem, ns, rs, ring, charges=charges, key_epochs=epochs, **kw)
        two = call_settle(eng, mem, rs, ring, [r if r else bytes(96) for r in res[1]], res[2], ts, key_epochs=epochs, wire=wire)
        one = call_rr(eng, mem, ns1, rs1, ring, charges=charges, returned=ts, key_epochs=epochs, **kw)
    assert list(one[0]) == [shed.get(t, 0) for t in range(n)]
    # a lane reserve shed at the wrong price has no reservation: ACT_STATUS_NOT_RESERVED where the one-phase call says WRONG_CHARGE
    assert list(two[0]) == [248 if shed.get(t) == 250 else shed.get(t, 0) for t in range(n)] and two[2] == bytes(n)
    assert two[4] == one[5]                                         # every output byte: records, or type 10 messages
    assert records_of(eng, wire, two[4], n) == records_of(eng, wire, one[5], n)      # (wire: decoded, and canonical)
    assert list(res[2]) == [255 if shed.get(t) == 250 else w.owner[t] for t in range(n)]
    assert [res[2][t] for t in range(n) if t not in shed] == [one[2][t] for t in range(n) if t not in shed]
    assert two[3] == dict(lanes=n, not_reserved=sum(1 for v in shed.values() if v == 250), return_too_big=len(big), settled=n - len(shed), settled_again=0, other_amount=0,
                          unanswered=0)
    # the nullifier set: the one-phase call's, and the reservations that are still open
    open_k = sorted((rc.rp.reduced(kbytes(w, t)), epochs[w.owner[t]]) for t in big)
    assert _pairs(ns) == sorted(_pairs(ns1) + open_k)
    # the receipts: the model's three keys per settled lane and tag_res alone per open reservation, under the matched key's epoch
    lanes = [rc.ar.Lane(w.k[t], (t, 0), 0, w.owner[t], S) for t in range(n)]
    mres = rc.reserve(lanes, spent, receipts, charges)
    mst, mbefore, mc = rc.settle([r if r else (0, (0, 0), 0) for r in mres[4]], list(res[2]), ts, receipts, 2)
    assert (mst, mbefore, mc) == (list(two[0]), list(two[2]), two[3])
    assert _pairs(rs) == model_receipts(eng, w, receipts, epochs) and len(rs) == 3 * (n - len(shed)) + len(big)
    if n == 6:
        with step(120, "the model's records"):
            got = records_of(eng, wire, two[4], n)
            for t in range(n):
                if t not in shed:
                    assert got[160 * t:160 * t + 160] == model_record(eng, w, bench_params, t, ts[t], w.owner[t]), (t, ts[t])
    with step(60, "the open reservations settled with t = s, and the same lanes through the one-phase call"):
        two2 = call_settle(eng, mem, rs, ring, [res[1][t] for t in big], [res[2][t] for t in big], [S] * len(big), key_epochs=epochs, wire=wire)
        one2 = call_rr(eng, mem, ns1, rs1, ring, returned=[S] * len(big), key_epochs=epochs, **(dict(msgs=[kw["msgs"][t] for t in big]) if wire else dict(recs=[recs[t] for t in big])))
        assert two2[0] == one2[0] == bytes(len(big)) and two2[4] == one2[5] and _pairs(ns) == _pairs(ns1)
    for x in (ns, rs, ns1, rs1):
        x.close()
    assert eng.secret_residue() == 0


# ---- 3. retries ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_settled_again_gives_the_same_bytes_and_the_one_phase_call_serves_the_client(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring, epochs = 6, w.keys, [41, 42]
    ts = amounts(n)
    recs = [w.proof(t) for t in range(n)]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "reserve; before settlement the one-phase calls answer 3 and both sets stay as they were"):
        res, kidx = reserved(eng, mem, ns, rs, ring, w, range(n), epochs)
        before = (_pairs(ns), _pairs(rs))
        got = call_rr(eng, mem, ns, rs, ring, recs=recs, returned=ts, key_epochs=epochs)
        assert got[0] == bytes([3]) * n and got[2] == b"\xff" * n and got[4]["foreign_spend"] == n and (_pairs(ns), _pairs(rs)) == before
        assert call_replay(eng, mem, ns, rs, ring, recs=recs, key_epochs=epochs)[0] == bytes([3]) * n and (_pairs(ns), _pairs(rs)) == before
    with step(60, "settle, and settle again"):
        first = call_settle(eng, mem, rs, ring, res, kidx, ts, key_epochs=epochs, wire=wire)
        assert first[0] == bytes(n) and first[2] == bytes(n) and first[3]["settled"] == n
        settled = _pairs(rs)
        again = call_settle(eng, mem, rs, ring, res, kidx, ts, key_epochs=epochs, wire=wire)
        assert again[0] == bytes(n) and again[2] == b"\1" * n and again[4] == first[4] and again[3]["settled_again"] == n and _pairs(rs) == settled
    with step(90, "a second context, the receipts restored from a snapshot"):
        snaps = snapshot(ns, rs, tmp_path, "settled")
        eng2 = engine_factory(bench_params, L, max_batch=2048, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
        ns2, rs2 = restored(capi, snaps)
        other = call_settle(eng2, mem, rs2, ring, res, kidx, ts, key_epochs=epochs, wire=wire)
        assert other[0] == bytes(n) and other[2] == b"\1" * n and other[4] == first[4] and _pairs(rs2) == settled
        ns2.close(); rs2.close()
        assert eng2.secret_residue() == 0
    with step(60, "after settlement: the one-phase call serves the same t and refuses another"):
        kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
        served = call_rr(eng, mem, ns, rs, ring, returned=ts, key_epochs=epochs, **kw)
        assert served[0] == bytes(n) and served[3] == b"\1" * n and served[5] == first[4]
        other_t = call_rr(eng, mem, ns, rs, ring, returned=amounts(n, 1), key_epochs=epochs, **kw)
        assert other_t[0] == bytes([3]) * n and (_pairs(ns), _pairs(rs)) == (before[0], settled)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 4. the pin and the bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_the_marker_pins_the_amount(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring = w.keys
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    t1 = [2, 0, 1, S]
    with step(60, "four reservations settled with t1"):
        res, kidx = reserved(eng, mem, ns, rs, ring, w, range(5))
        first = call_settle(eng, mem, rs, ring, res[:4], kidx[:4], t1, wire=wire)
        assert first[0] == bytes(4)
    before = (_pairs(ns), _pairs(rs))
    with step(60, "another amount: 247 and unchanged sets, 0 against non-zero and non-zero against 0 included"):
        got = call_settle(eng, mem, rs, ring, res[:4], kidx[:4], [0, 1, 2, S - 1], wire=wire)
        assert got[0] == bytes([247]) * 4 and got[1] == [b""] * 4 and got[2] == bytes(4) and got[3] == dict(dict.fromkeys(rc.SETTLE_COUNTS, 0), lanes=4, other_amount=4)
        got = call_settle(eng, mem, rs, ring, res[:1], kidx[:1], None, wire=wire)      # no amounts at all names 0
        assert got[0] == bytes([247]) and (_pairs(ns), _pairs(rs)) == before
    with step(60, "t1 + l is t1"):
        got = call_settle(eng, mem, rs, ring, res[:4], kidx[:4], [t + ELL for t in t1], wire=wire)
        assert got[0] == bytes(4) and got[2] == b"\1" * 4 and got[4] == first[4] and (_pairs(ns), _pairs(rs)) == before
    with step(60, "inside one batch: [R t1, R t1, R t2]"):
        got = call_settle(eng, mem, rs, ring, [res[4]] * 3, [kidx[4]] * 3, [2, 2, 1], wire=wire)
        assert list(got[0]) == [0, 0, 247] and list(got[2]) == [0, 1, 0] and got[1][0] == got[1][1] and got[1][2] == b""
        assert (got[3]["settled"], got[3]["settled_again"], got[3]["other_amount"]) == (1, 1, 1) and len(rs) == 5 + 2 * 5
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mode,mem", MODES)
def test_the_bounds_and_what_is_not_a_reservation(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [101, 102]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "reservations; token 9 recorded by the replay call"):
        res, kidx = reserved(eng, mem, ns, rs, ring, w, range(8), epochs)
        assert call_replay(eng, mem, ns, rs, ring, recs=[w.proof(9)], key_epochs=epochs)[0] == b"\0"
    before = _pairs(rs)
    with step(60, "t = s + 1, 2^200 + 1, s + l: 249 / 249 / accepted, and the 249 lanes leave no trace"):
        got = call_settle(eng, mem, rs, ring, res[:3], kidx[:3], [S + 1, (1 << 200) + 1, S + ELL], key_epochs=epochs)
        assert list(got[0]) == [249, 249, 0] and got[3]["return_too_big"] == 2 and got[1][:2] == [b"", b""]
        kp = kprimes(eng, w)
        assert _pairs(rs) == sorted(before + [(rc.marker(kbytes(w, 2), kp[0][2]), epochs[0]), (rc.tag(kbytes(w, 2), kp[0][2], S), epochs[0])])
    before = _pairs(rs)
    with step(60, "248 with nothing recorded: a flipped bit of k, K' or s; another ring index out of range; a one-phase spend"):
        def flipped(r, at):
            b = bytearray(r); b[at] ^= 1
            return bytes(b)
        foreign = rc.record(kbytes(w, 9), kp[0][9], S)             # what a record of token 9 would be: its spend holds no reservation tag
        batch = [flipped(res[3], 0), flipped(res[3], 40), flipped(res[3], 64), res[3], res[3], foreign]
        got = call_settle(eng, mem, rs, ring, batch, [kidx[3]] * 3 + [255, 2, w.owner[9]], [1] * 6, key_epochs=epochs)
        assert got[0] == bytes([248]) * 6 and got[1] == [b""] * 6 and got[3] == dict(dict.fromkeys(rc.SETTLE_COUNTS, 0), lanes=6, not_reserved=6) and _pairs(rs) == before
        # a flipped s above t is not a smaller bound either: s - 1 is another reservation
        assert call_settle(eng, mem, rs, ring, [res[3][:64] + scb(S - 1)], [kidx[3]], [1], key_epochs=epochs)[0] == bytes([248]) and _pairs(rs) == before
    with step(60, "an epoch retired on the receipts takes its reservations with it"):
        gone = rs.retire_epoch(102)
        assert gone == sum(1 for t in list(range(8)) + [9] if w.owner[t] == 1)
        left = _pairs(rs)
        got = call_settle(eng, mem, rs, ring, res[4:8], kidx[4:8], [1] * 4, key_epochs=[101, 103])
        assert list(got[0]) == [0 if w.owner[t] == 0 else 248 for t in range(4, 8)]
        assert len(rs) == len(left) + 2 * sum(1 for t in range(4, 8) if w.owner[t] == 0)
        assert call_settle(eng, mem, rs, ring, res[4:8], kidx[4:8], [1] * 4, key_epochs=epochs, want_rc=1)[0] == bytes([99]) * 4      # the retired epoch itself: refused as a whole
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 5. failures ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_whole_call_refusals_and_a_failed_signature_step(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 5, w.keys
    ts = amounts(n)
    ns, small = capi.NullifierSet(1000), capi.NullifierSet(500)     # 1024 slots: room for 512 keys
    with step(60, "receipts without room for 2 n, and a NULL nonce_key"):
        res, kidx = reserved(eng, mem, ns, small, ring, w, range(n))
        filler = b"".join(scb(1000 + i) for i in range(512 - n - 2 * n + 1))
        assert small.check_and_insert(filler) == bytes(len(filler) // 32) and len(small) == 512 - 2 * n + 1
        got = call_settle(eng, mem, small, ring, res, kidx, ts, want_rc=1)
        assert got[0] == bytes([99]) * n and len(small) == 512 - 2 * n + 1 and got[3]["lanes"] == 0 and b"receipts" in eng.lib.act_last_error(eng.ctx)
        got = call_settle(eng, mem, small, ring, res[:1], kidx[:1], ts[:1], nonce_key=None, want_rc=1)
        assert got[0] == bytes([99]) and len(small) == 512 - 2 * n + 1
    rs = capi.NullifierSet(1000)
    ns2 = capi.NullifierSet(1000)
    with step(60, "the signature step fails behind the recorded marker and amount tag"):
        res, kidx = reserved(eng, mem, ns2, rs, ring, w, range(n))
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        got = call_settle(eng, mem, rs, ring, res, kidx, ts, want_rc=2)
        assert got[0] == bytes([251]) * n and got[1] == [b""] * n and len(rs) == 3 * n and got[3]["unanswered"] == n
        assert eng.secret_residue() == 0
    with step(60, "the same call again is served with the bytes of an undisturbed run; other amounts are not"):
        assert call_settle(eng, mem, rs, ring, res, kidx, amounts(n, 1))[0] == bytes([247]) * n
        got = call_settle(eng, mem, rs, ring, res, kidx, ts)
        assert got[0] == bytes(n) and got[2] == b"\1" * n
        fresh_ns, fresh_rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
        assert call_rr(eng, mem, fresh_ns, fresh_rs, ring, recs=[w.proof(t) for t in range(n)], returned=ts)[5] == got[4]
        fresh_ns.close(); fresh_rs.close()
    for x in (ns, ns2, small, rs):
        x.close()
    assert eng.secret_residue() == 0


def test_a_moved_sign_key_signs_every_lane_and_is_the_one_phase_calls_bytes(engine_factory, bench_params):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    n, ring, ts = 4, w.keys, [1, 2, 3, 0]
    ns, rs, ns1, rs1 = (capi.NullifierSet(1000) for _ in range(4))
    with step(60, "sign_key = 0 on both roads"):
        res, kidx = reserved(eng, "host", ns, rs, ring, w, range(n))
        two = call_settle(eng, "host", rs, ring, res, kidx, ts, sign_key=0)
        one = call_rr(eng, "host", ns1, rs1, ring, recs=[w.proof(t) for t in range(n)], returned=ts, sign_key=0)
        assert two[0] == bytes(n) and two[4] == one[5] and list(kidx) == [w.owner[t] for t in range(n)] and _pairs(ns) == _pairs(ns1)
    for x in (ns, rs, ns1, rs1):
        x.close()
    assert eng.secret_residue() == 0


# ---- 6. the client --------------------------------------------------------------------------------------------------------------------------------
def test_the_client_accepts_a_settled_and_a_resettled_record_at_full_range_width(engine_factory, bench_params):
    from act_amd import capi
    eng = engine_factory(bench_params, 128, max_batch=16, transcript=capi.TRANSCRIPT_HOST)
    n = 3
    with step(240, "tokens and proofs"):
        w = world128(eng, "rr-128", n, 128)
    ts = [w.s[0], 1, 2]
    blob, ring = b"".join(w.proofs), [w.keys[1], w.keys[0]]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(120, "reserved, settled, settled again"):
        tt = b"".join(scb(t) for t in ts)
        st, res, ok, rep, c = eng.redeem_reserve(ns, rs, ring, blob, charges=b"".join(scb(s) for s in w.s))
        assert st == bytes(n) and rep == bytes(n) and c["fresh"] == n and [res[96 * i + 64:96 * i + 96] for i in range(n)] == [scb(s) for s in w.s]
        st, out, sb, c = eng.redeem_settle(rs, ring, res, ok, NONCE_KEY, tt, sign_key=1)
        assert st == bytes(n) and sb == bytes(n) and c["settled"] == n
        st2, out2, sb2, c2 = eng.redeem_settle(rs, ring, res, ok, NONCE_KEY, tt, sign_key=1)
        assert st2 == bytes(n) and sb2 == b"\1" * n and out2 == out and c2["settled_again"] == n
    with step(120, "client"):
        pre = b"".join(w.prer)
        for o in (out, out2):
            cst, tok = eng.refund_to_credit_token_return(pre, blob, o, w.keys[0][32:])
            assert cst == bytes(n) and [tok[160 * i + 128:160 * i + 160] for i in range(n)] == [scb(CREDIT - w.s[i] + ts[i]) for i in range(n)]
        ost, _ = eng.refund_to_credit_token(pre, blob, b"".join(out[160 * i:160 * i + 128] for i in range(n)), w.keys[0][32:])
        assert ost == bytes([4]) * n                                # the plain client call refuses the first 128 bytes when t != 0
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 7. the Python layer ----------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_gives_what_the_capi_calls_give(engine_factory, bench_params):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, "host")
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    toks, ts = [0, 1, 2, 3], [1, S, S + 1, 2]
    with step(120, "api and capi on sets with the same history"):
        dbs = [(api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)) for _ in range(2)]
        proofs = [api.SpendProof(w.proof(t), L) for t in toks]
        blob = b"".join(w.proof(t) for t in toks)
        res, rep = ring.reserve_batch(params, dbs[0][0], dbs[0][1], proofs, charges=[S, S, S, S + 1])
        st, rec, ok, crep, c = eng.redeem_reserve(dbs[1][0].set, dbs[1][1].set, w.keys, blob, key_epochs=[11, 12], charges=scb(S) * 3 + scb(S + 1))
        assert list(st) == [0, 0, 0, 250] and [r.code if isinstance(r, api.Error) else 0 for r in res] == list(st) and rep == [False] * 4 and ring.last_reserve_counts == c
        good = [r for r in res if isinstance(r, api.Reservation)]
        assert [r.record for r in good] == [rec[96 * i:96 * i + 96] for i in range(3)] and [r.key for r in good] == list(ok[:3])
        for r in good:
            back = api.Reservation.from_bytes(r.to_bytes())
            assert len(r.to_bytes()) == 97 and (back.record, back.key) == (r.record, r.key) and back.nullifier() == r.record[:32] and back.charge() == S
        out, before = ring.settle_batch(params, dbs[0][1], good, ts[:3], NONCE_KEY)
        st, raw, sb, c = eng.redeem_settle(dbs[1][1].set, w.keys, rec[:96 * 3], ok[:3], NONCE_KEY, b"".join(scb(t) for t in ts[:3]), key_epochs=[11, 12])
        assert list(st) == [0, 0, 249] and [r.code if isinstance(r, api.Error) else 0 for r in out] == list(st) and before == [False] * 3 and ring.last_settle_counts == c
        assert [r.record for r in out if isinstance(r, api.RefundReturn)] == [raw[160 * i:160 * i + 160] for i in range(2)]
        # the retry, the wire forms and the one-key wrappers
        res2, rep2 = ring.reserve_cbor_batch(params, dbs[0][0], dbs[0][1], [p.to_cbor(params) for p in proofs[:3]], L)
        assert [r.record for r in res2] == [r.record for r in good] and rep2 == [True] * 3
        msgs, before = ring.settle_batch(params, dbs[0][1], good[:2], ts[:2], NONCE_KEY, cbor=True)
        assert before == [True, True] and [api.RefundReturn.from_cbor(x, params).record for x in msgs] == [raw[:160], raw[160:320]]
        one = api.PrivateKey(w.keys[0])
        d0, d1 = api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)
        r1, p1 = one.reserve_batch(params, d0, d1, proofs[:1])
        o1, b1 = one.settle_batch(params, d1, r1, [1], NONCE_KEY)
        assert p1 == [False] and b1 == [False] and o1[0].record == raw[:160]
