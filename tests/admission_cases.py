"""Shared by the admission tests (tests/test_admission_host.py, tests/test_gpu_admission.py, tools/admission_probe.py): the loop of
act_redeem_admit_batch as a model over labels (what a lane IS by construction: which token it spends, whether its proof was
tampered with, what the wire reader says about its spelling) and a Python set; the fixed lane mix of the feature with HAND-WRITTEN
expectations, so that the model is not its own judge; the seeded lane plans of the density runs; and the host build of the
admission lane bodies (tests/hostcheck/admit_check.cpp).  Not a test module."""
import ctypes as C
import os
import random
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = 2**252 + 27742317777372353535851937790883648493
KEY_NONE = 255
WRONG_CHARGE, DOUBLE_SPEND = 250, 3
COUNTS = ("lanes", "wire_rejected", "wrong_charge", "spent_before", "verified", "rejected_by_verification", "double_spend_after", "accepted")

# k: the nullifier (any hashable; reduced scalar on the GPU side), s: the charge the proof carries, verdict: what verification says about
# the proof (0 / 6 / 7 / 255) by construction, key: the ring index it verifies under, wire: the wire reader's code for the message (0 =
# well-shaped; 253 / 254 / 255)
Lane = namedtuple("Lane", "k s verdict key wire", defaults=(0, 0))


def model(lanes, spent, charges=None):
    """The loop of the header, in lane order.  `spent`: the set as the call finds it (not modified).  -> (statuses, out_key, counts,
    recorded: [(k, key index)] in the order of recording)"""
    before = frozenset(spent)
    now = set(before)
    st, ok, rec = [], [], []
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = len(lanes)
    for i, ln in enumerate(lanes):
        if ln.wire:                                                    # 1. the message fails structurally
            st.append(ln.wire); ok.append(KEY_NONE); c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:     # 2. not the expected charge
            st.append(WRONG_CHARGE); ok.append(KEY_NONE); c["wrong_charge"] += 1; continue
        if ln.k in before:                                             # 3. spent when the call looks it up: not verified
            st.append(DOUBLE_SPEND); ok.append(KEY_NONE); c["spent_before"] += 1; continue
        c["verified"] += 1                                             # 4. the redeem call
        if ln.verdict:
            st.append(ln.verdict); ok.append(KEY_NONE); c["rejected_by_verification"] += 1; continue
        ok.append(ln.key)
        if ln.k in now:
            st.append(DOUBLE_SPEND); c["double_spend_after"] += 1; continue
        now.add(ln.k); rec.append((ln.k, ln.key))
        st.append(0); c["accepted"] += 1
    return st, ok, c, rec


def plain_model(lanes, spent):
    """act_redeem_(cbor_)keyring_epochs_batch on the same lanes: verify, THEN look up and record"""
    now = set(spent)
    st = []
    for ln in lanes:
        if ln.wire or ln.verdict:
            st.append(ln.wire or ln.verdict); continue
        if ln.k in now:
            st.append(DOUBLE_SPEND); continue
        now.add(ln.k); st.append(0)
    return st


# ---- the fixed lane mix (the table of the feature), hand-written ------------------------------------------------------------------------
# (name, token, verdict by construction, charge is the expected one, wire code, spelled canonically).  Tokens "sp*" are recorded before
# the call.  The last four lanes exist in the wire form only.
FIXED_MIX = [
    ("fresh valid",                          "t0",  0,   True,  0,   True),
    ("replay of a recorded nullifier",       "sp0", 0,   True,  0,   True),
    ("spent, tampered proof",                "sp1", 7,   True,  0,   True),
    ("spent, undecodable A'",                "sp2", 255, True,  0,   True),
    ("fresh, tampered",                      "t1",  7,   True,  0,   True),
    ("fresh valid, wrong charge",            "t2",  0,   False, 0,   True),
    ("spent, wrong charge",                  "sp3", 0,   False, 0,   True),
    ("shared fresh nullifier, tampered",     "t3",  7,   True,  0,   True),
    ("shared fresh nullifier, valid",        "t3",  0,   True,  0,   True),
    ("shared fresh nullifier, valid (1st)",  "t4",  0,   True,  0,   True),
    ("shared fresh nullifier, valid (2nd)",  "t4",  0,   True,  0,   True),
    ("A' = identity",                        "t5",  6,   True,  0,   True),
    ("wire: respelled replay",               "sp0", 0,   True,  0,   False),
    ("wire: truncated message",              "t6",  0,   True,  254, False),
    ("wire: mis-shaped message",             "t7",  0,   True,  253, False),
    ("wire: spent, invalid point in front of a structural fault", "sp4", 0, True, 255, False),
]
N_RECORD_LANES = 12
# what the admission calls answer, what the plain redeem calls answer on the same lanes, and the counts -- written down by hand from the
# issue's table, not computed
FIXED_EXPECT = [0, 3, 3, 3, 7, 250, 250, 7, 0, 0, 3, 6, 3, 254, 253, 255]
FIXED_EXPECT_PLAIN = [0, 3, 7, 255, 7, 0, 3, 7, 0, 0, 3, 6, 3, 254, 253, 255]
FIXED_COUNTS_RECORDS = dict(lanes=12, wire_rejected=0, wrong_charge=2, spent_before=3, verified=7, rejected_by_verification=3, double_spend_after=1, accepted=3)
FIXED_COUNTS_WIRE = dict(lanes=16, wire_rejected=3, wrong_charge=2, spent_before=4, verified=7, rejected_by_verification=3, double_spend_after=1, accepted=3)
FIXED_SPENT = ("sp0", "sp1", "sp2", "sp3", "sp4")
SPEND, EXPECTED_WRONG = 2, 3        # every proof of the mix spends 2; a "wrong charge" lane is asked for 3


def fixed_lanes(wire):
    """-> (lanes, charges) of the fixed mix over token NAMES"""
    mix = FIXED_MIX if wire else FIXED_MIX[:N_RECORD_LANES]
    lanes = [Lane(tok, SPEND, verdict, 0, code) for _, tok, verdict, _, code, _ in mix]
    charges = [SPEND if right else EXPECTED_WRONG for _, _, _, right, _, _ in mix]
    return lanes, charges


def check_model_on_fixed_mix():
    for wire in (False, True):
        lanes, charges = fixed_lanes(wire)
        n = len(lanes)
        st, ok, counts, rec = model(lanes, set(FIXED_SPENT), charges)
        assert st == FIXED_EXPECT[:n], (wire, st)
        assert counts == (FIXED_COUNTS_WIRE if wire else FIXED_COUNTS_RECORDS), (wire, counts)
        assert [k for k, _ in rec] == ["t0", "t3", "t4"] and [ok[i] for i in (0, 8, 9, 10)] == [0, 0, 0, 0] and ok.count(KEY_NONE) == n - 4
        assert counts["verified"] == counts["lanes"] - counts["wire_rejected"] - counts["wrong_charge"] - counts["spent_before"]
        # without charges the two wrong-charge lanes are an honest spend and a replay
        st2, _, c2, rec2 = model(lanes, set(FIXED_SPENT), None)
        assert [st2[5], st2[6]] == [0, 3] and c2["wrong_charge"] == 0 and c2["spent_before"] == counts["spent_before"] + 1 and len(rec2) == 4
        assert plain_model(lanes, set(FIXED_SPENT)) == FIXED_EXPECT_PLAIN[:n]
        # the two orders differ only where the nullifier was in the set before the call, and there admission says 3
        assert all(a == b or (lanes[i].k in FIXED_SPENT and a == 3) for i, (a, b) in enumerate(zip(st2, plain_model(lanes, set(FIXED_SPENT)))))


# ---- the density runs: n = 2 * 4096 + 17 lanes, a seeded fraction of them shed --------------------------------------------------------
DENSITY_N = 2 * 4096 + 17
DENSITIES = ((0, 1), (1, 8), (1, 2), (7, 8), (1, 1))
# chosen on the CPU (tests/test_admission_host.py asserts it): with these seeds every mixed density puts at least 1/16 of the lanes into
# each category.  At 7/8 the survivors are one lane in eight, so accepted and rejected-by-verification can only both reach 1/16 when
# the seed sheds slightly fewer than 7/8 and every survivor belongs to a (tampered, valid) pair.
DENSITY_SEEDS = {(0, 1): 1, (1, 8): 1, (1, 2): 1, (7, 8): 2, (1, 1): 1, (3, 4): 1}
EXTRA_DENSITIES = ((3, 4),)      # the general lane cycle at a high shed fraction; no category bound is asserted for it

# a lane of a plan: the token it spends, which of the token's two proofs (0 / 1: same nullifier, different rng), tampered or not, and
# whether the token is recorded before the call / the lane is asked the wrong charge
PlanLane = namedtuple("PlanLane", "token variant tampered spent wrong")


def density_plan(n, num, den, seed, with_charges):
    r = random.Random(seed * 1000003 + num * 101 + den)
    shed = [r.random() * den < num for _ in range(n)]
    plan, tok, flip = [None] * n, 0, 0
    live = [i for i in range(n) if not shed[i]]
    for i in range(n):
        if shed[i]:
            wrong = with_charges and flip % 2 == 1
            plan[i] = PlanLane(tok, 0, False, not wrong, wrong); tok += 1; flip += 1
    # 7/8 is special-cased: with one lane in eight surviving, accepted and rejected-by-verification can only both reach 1/16 of the
    # lanes when EVERY survivor belongs to a (tampered, valid) pair, so that run holds no lone valid or lone tampered survivor and no
    # (valid, valid) pair; those shapes are covered at 1/8 and 1/2 and by the run at 3/4 below, which asserts no category sizes
    cycle = ("tv",) if (num, den) == (7, 8) else ("tv", "vv", "v", "t")
    j, c = 0, 0
    while j < len(live):
        kind = cycle[c % len(cycle)]; c += 1
        if len(kind) == 2 and j + 1 < len(live):
            plan[live[j]] = PlanLane(tok, 0, kind[0] == "t", False, False)
            plan[live[j + 1]] = PlanLane(tok, 1, False, False, False)
            j += 2
        else:
            plan[live[j]] = PlanLane(tok, 0, kind == "t", False, False); j += 1
        tok += 1
    return plan, tok


def plan_lanes(plan, spend=SPEND, nullifier=lambda t: t):
    """-> (model lanes, charges, spent set) of a plan"""
    lanes = [Lane(nullifier(p.token), spend, 7 if p.tampered else 0, 0, 0) for p in plan]
    charges = [spend + 1 if p.wrong else spend for p in plan]
    spent = {nullifier(p.token) for p in plan if p.spent}
    return lanes, charges, spent


def plan_categories(plan, with_charges):
    """lanes per category of the feature's density check, from the MODEL's output"""
    lanes, charges, spent = plan_lanes(plan)
    st, _, c, _ = model(lanes, spent, charges if with_charges else None)
    multi = {}
    for p in plan:
        if not p.spent and not p.wrong:
            multi[p.token] = multi.get(p.token, 0) + 1
    cats = dict(accepted=c["accepted"], spent_before=c["spent_before"], rejected_by_verification=c["rejected_by_verification"],
                in_batch_duplicate=sum(1 for p in plan if multi.get(p.token, 0) > 1))
    if with_charges:
        cats["wrong_charge"] = c["wrong_charge"]
    return cats, st, c


def plan_is_mixed_enough(n, num, den, seed):
    for with_charges in (False, True):
        plan, _ = density_plan(n, num, den, seed, with_charges)
        cats, _, _ = plan_categories(plan, with_charges)
        if any(16 * v < n for v in cats.values()):
            return False
    return True


def find_seed(n, num, den, limit=4000):
    for seed in range(1, limit):
        if plan_is_mixed_enough(n, num, den, seed):
            return seed
    raise AssertionError("no seed below %d gives every category 1/16 of the lanes at %d/%d" % (limit, num, den))


def density_seed(num, den):
    return DENSITY_SEEDS[(num, den)]


# ---- wire spellings ----------------------------------------------------------------------------------------------------------------------
def spend_entries(rec, L):
    """[(key, encoded value)] of a SpendProof record, as SpendProof::to_cbor orders them (tests/test_cbor.py _variants)"""
    import pymodel as m
    bstr = lambda b: b"\x58\x20" + b
    f = [rec[i:i + 32] for i in range(0, len(rec), 32)]
    ents, i = [], 0
    for key, kind, shape in m.CBOR_TYPES["SpendProof"]:
        if shape == 0:
            ents.append((key, bstr(f[i]))); i += 1
        elif shape == 1:
            ents.append((key, m._cbor_head(4, L) + b"".join(bstr(x) for x in f[i:i + L]))); i += L
        else:
            ents.append((key, m._cbor_head(4, L) + b"".join(b"\x82" + bstr(f[i + 2 * j]) + bstr(f[i + 2 * j + 1]) for j in range(L)))); i += 2 * L
    return ents


def wire_map(ents, extra=0):
    import pymodel as m
    return m._cbor_head(5, len(ents) + extra) + b"".join(m._cbor_head(0, k) + v for k, v in ents)


def respelled(rec, L):
    """a legal spelling that is not the canonical one: the keys in reverse order"""
    return wire_map(spend_entries(rec, L)[::-1])


def invalid_point_then_fault(rec, L):
    """A' is not a Ristretto encoding and, BEHIND it in wire order, a scalar is a 31-byte string: from_cbor reports the point"""
    ents = spend_entries(rec, L)
    ents[2] = (ents[2][0], b"\x58\x20" + b"\x01" + bytes(31))
    ents[5] = (ents[5][0], b"\x58\x1f" + bytes(31))
    return wire_map(ents)


def layout(L):
    """(template, payload offsets) of the canonical SpendProof message: the codec's cbor_layout, rebuilt from the model's encoder"""
    import pymodel as m
    nf = 14 + 4 * L
    tmpl = m.cbor_encode("SpendProof", bytes(32 * nf), L)
    probe = m.cbor_encode("SpendProof", b"".join(bytes([1 + f % 250]) * 32 for f in range(nf)), L)
    offs, i = [], 0
    while i < len(tmpl):
        if tmpl[i:i + 2] == b"\x58\x20" and probe[i + 2:i + 34] == bytes([1 + len(offs) % 250]) * 32:
            offs.append(i + 2); i += 34
        else:
            i += 1
    assert len(offs) == nf, (len(offs), nf)
    return tmpl, offs


# ---- host build of the lane bodies -------------------------------------------------------------------------------------------------------
def build_admit_check(out, sanitize=False):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "admit_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src], check=True)
    return out


def _u32(n):
    return (C.c_uint32 * max(1, n))()


def host_compact(ac, pre: bytes):
    n = len(pre)
    nb = (n + 255) // 256
    blk, idx, pos = _u32(nb), _u32(n), _u32(n)
    ac.hc_admit_compact.restype = C.c_uint32
    total = ac.hc_admit_compact(pre, n, blk, idx, pos)
    return total, list(idx[:total]), list(pos[:n])


SHED_PATTERNS = ("none", "all", "alternating", "random")
COMPACT_NS = (0, 1, 63, 64, 65, 255, 257, 4 * 256 + 3, 70000)      # 70000: more workgroups (274) than the scanning workgroup has threads


def shed_pattern(name, n, seed=5):
    r = random.Random(seed * 7919 + n)
    codes = (3, 250, 253, 254, 255)
    if name == "none":
        return bytes(n)
    if name == "all":
        return bytes(codes[i % 5] for i in range(n))
    if name == "alternating":
        return bytes(0 if i % 2 else 3 for i in range(n))
    return bytes(0 if r.random() < 0.4 else codes[r.randrange(5)] for _ in range(n))


def check_compaction(ac):
    """stability: the survivors' order is lane order; pos is the inverse; every n and shed pattern of the feature"""
    for n in COMPACT_NS:
        for pat in SHED_PATTERNS:
            pre = shed_pattern(pat, n)
            total, idx, pos = host_compact(ac, pre)
            want = [i for i in range(n) if pre[i] == 0]
            assert total == len(want) and idx == want, (n, pat)
            inv = {lane: j for j, lane in enumerate(want)}
            assert pos == [inv.get(i, 0xFFFFFFFF) for i in range(n)], (n, pat)


def check_gather_scatter(ac, window=96):
    """rows, messages and the scatter against plain Python slicing; the survivors cross a gather window (`window` survivors at a time,
    as the engine takes ADMIT_WINDOW_BATCHES * max_batch) and the rows are not multiples of 16 bytes"""
    r = random.Random(77)
    for n in (0, 1, 63, 64, 65, 255, 257, 3 * window + 5):
        for pat in SHED_PATTERNS:
            pre = shed_pattern(pat, n, seed=9)
            total, idx, pos = host_compact(ac, pre)
            for row in (32, 128, 141, 17):
                src = bytes(r.randrange(256) for _ in range(n * row)) + b"\0"
                got = b""
                for w0 in range(0, total, window):
                    w = min(window, total - w0)
                    dst = C.create_string_buffer(w * row + 1)
                    ac.hc_admit_rows(dst, src, (C.c_uint32 * w)(*idx[w0:w0 + w]), w, C.c_uint64(row))
                    assert dst.raw[w * row:] == b"\0", "wrote past the window"
                    got += dst.raw[:w * row]
                assert got == b"".join(src[i * row:(i + 1) * row] for i in idx), (n, pat, row)
            # messages of uneven length
            lens = [r.randrange(0, 70) for _ in range(n)]
            offs = [0]
            for ln in lens:
                offs.append(offs[-1] + ln)
            blob = bytes(r.randrange(256) for _ in range(offs[-1])) + b"\0"
            for w0 in range(0, total, window):
                w = min(window, total - w0)
                sel = idx[w0:w0 + w]
                dst_off = [0]
                for i in sel:
                    dst_off.append(dst_off[-1] + lens[i])
                longest = max(lens[i] for i in sel)
                dst = C.create_string_buffer(dst_off[-1] + 1)
                ac.hc_admit_msgs(dst, (C.c_uint64 * (w + 1))(*dst_off), blob, (C.c_uint64 * w)(*[offs[i] for i in sel]), w, (longest + 15) // 16)
                assert dst.raw == b"".join(blob[offs[i]:offs[i + 1]] for i in sel) + b"\0", (n, pat, w0)
            # the answers back to their lanes
            for ob in (128, 141):
                cst = bytes(r.choice((0, 3, 7, 6, 255)) for _ in range(total)) + b"\0"
                ckey = bytes(r.randrange(4) for _ in range(total)) + b"\0"
                cout = bytes(r.randrange(1, 256) for _ in range(total * ob)) + b"\0"
                st = C.create_string_buffer(b"\x77" * (n + 1)); okey = C.create_string_buffer(b"\x77" * (n + 1)); out = C.create_string_buffer(b"\x77" * (n * ob + 1))
                ac.hc_admit_scatter(n, C.c_uint64(ob), (C.c_uint32 * max(1, n))(*pos), pre + b"\0", cst, ckey, cout, st, okey, out)
                assert st.raw[n:n + 1] == b"\x77" and okey.raw[n:n + 1] == b"\x77" and out.raw[n * ob:n * ob + 1] == b"\x77"
                for i in range(n):
                    j = pos[i]
                    if j == 0xFFFFFFFF:
                        assert (st.raw[i], okey.raw[i], out.raw[i * ob:(i + 1) * ob]) == (pre[i], KEY_NONE, bytes(ob)), (n, pat, i)
                    else:
                        assert (st.raw[i], okey.raw[i], out.raw[i * ob:(i + 1) * ob]) == (cst[j], ckey[j], cout[j * ob:(j + 1) * ob]), (n, pat, i)


def check_decision(ac):
    """the decision function against the model's order, and the probe is only made for a lane that passed the charge check"""
    probed = C.c_int(0)
    for code in (0, 253, 254, 255):
        for given in (0, 1):
            for equal in (0, 1):
                for found in (0, 1):
                    got = ac.hc_admit_decide(code, given, equal, found, C.byref(probed))
                    ln = Lane("k", 5, 0, 0, code)
                    st, _, _, _ = model([ln], {"k"} if found else set(), [5 if equal else 6] if given else None)
                    want = st[0] if st[0] in (250, 3, 253, 254, 255) else 0
                    assert got == want, (code, given, equal, found, got, want)
                    assert probed.value == int(code == 0 and not (given and not equal)), (code, given, equal, found)


def check_screen(ac):
    """admit_screen_lane over a table built with the set's slot function, against the model: keys spelled k and k + l, charges spelled
    s and s + l, strides of a record and of the compact side array"""
    r = random.Random(31)
    salt = bytes(range(16, 32))
    cap = 1024
    for n in (0, 1, 63, 64, 65, 255, 257):
        for pat in SHED_PATTERNS:
            tk, ts = _u32(cap * 8), _u32(cap)
            pool = [r.randrange(ELL) for _ in range(max(1, n))]
            want_pre = shed_pattern(pat, n, seed=3)
            spent, ks, charge, code = set(), [], [], []
            lanes, charges = [], []
            for i in range(n):
                k = pool[i]; s = r.randrange(1, 1000)
                w = want_pre[i]
                c_i, cd = s, 0
                if w == 3:
                    spent.add(k)
                elif w == 250:
                    c_i = s + 1
                elif w:
                    cd = w
                spell = lambda v: v + ELL if r.random() < 0.3 and v + ELL < 2**256 else v
                ks.append(spell(k).to_bytes(32, "little") + spell(s).to_bytes(32, "little"))
                charge.append(spell(c_i).to_bytes(32, "little")); code.append(cd)
                lanes.append(Lane(k, s, 0, 0, cd)); charges.append(c_i)
            for k in spent:
                assert ac.hc_admit_table_insert(tk, ts, cap, salt, k.to_bytes(32, "little"), 7) == 1
            st, _, _, _ = model(lanes, spent, charges)
            for stride in (64, 96):
                blob = b"".join(x + bytes(stride - 64) for x in ks) + b"\0"
                pre = C.create_string_buffer(b"\x55" * (n + 1)); kred = C.create_string_buffer(32 * n + 1)
                ac.hc_admit_screen(n, stride, blob, b"".join(charge) + b"\0", bytes(code) + b"\0", tk, ts, cap, salt, pre, kred)
                assert pre.raw[n:n + 1] == b"\x55"
                assert list(pre.raw[:n]) == [x if x in (250, 3, 253, 254, 255) else 0 for x in st] == list(want_pre), (n, pat, stride)
                for i in range(n):
                    assert kred.raw[32 * i:32 * i + 32] == (bytes(32) if code[i] else lanes[i].k.to_bytes(32, "little")), (n, pat, i)
            # no charges: a wrong-charge lane is an ordinary fresh lane
            pre = C.create_string_buffer(n + 1); kred = C.create_string_buffer(32 * n + 1)
            ac.hc_admit_screen(n, 64, b"".join(ks) + b"\0", None, None, tk, ts, cap, salt, pre, kred)
            assert list(pre.raw[:n]) == [3 if ln.k in spent else 0 for ln in lanes]


def check_framing(ac, records, L, variants):
    """admit_wire_piece against the template: a message is canonical iff its first msg_len bytes are the template around 32-byte
    payloads; the k and s payloads of a canonical message are the record's fields 0 and 1 (the model's decoder agrees, mod l).
    `variants(rec)` -> messages (tests/test_cbor.py _variants)"""
    import pymodel as m
    tmpl, offs = layout(L)
    ml, nf = len(tmpl), len(offs)
    pay = set()
    for o in offs:
        pay.update(range(o, o + 32))
    frame = [i for i in range(ml) if i not in pay]
    msgs = []
    for rec in records:
        msgs += [v for v, _ in variants(rec)] + [respelled(rec, L), invalid_point_then_fault(rec, L)]
    n = len(msgs)
    off = [0]
    for v in msgs:
        off.append(off[-1] + len(v))
    blob = b"".join(msgs) + b"\0"
    ks = C.create_string_buffer(64 * n + 1); flags = C.create_string_buffer((n + 3) // 4 * 4 + 1)
    ac.hc_admit_wire(n, nf, ml, blob, (C.c_uint64 * (n + 1))(*off), tmpl, (C.c_uint32 * nf)(*offs), ks, flags)
    canon = 0
    for i, v in enumerate(msgs):
        want = len(v) >= ml and all(v[j] == tmpl[j] for j in frame)
        assert (flags.raw[i] == 0) == want, (i, v[:16].hex())
        if want:
            canon += 1
            assert ks.raw[64 * i:64 * i + 64] == v[offs[0]:offs[0] + 32] + v[offs[1]:offs[1] + 32]
            code, rec = m.cbor_decode("SpendProof", v, L)
            if code == 0:
                red = lambda b: (int.from_bytes(b, "little") % ELL).to_bytes(32, "little")
                assert rec[:64] == red(ks.raw[64 * i:64 * i + 32]) + red(ks.raw[64 * i + 32:64 * i + 64]), i
    assert 0 < canon < n and flags.raw[(n + 3) // 4 * 4:] == b"\0"
    # fixed-size messages without offsets: the same answers for a batch of canonical messages with one byte of framing changed
    good = [m.cbor_encode("SpendProof", rec, L) for rec in records]
    bad = bytearray(good[0]); bad[offs[3] - 2] ^= 1
    batch = good + [bytes(bad)]
    ks2 = C.create_string_buffer(64 * len(batch) + 1); fl2 = C.create_string_buffer((len(batch) + 3) // 4 * 4 + 1)
    ac.hc_admit_wire(len(batch), nf, ml, b"".join(batch) + b"\0", None, tmpl, (C.c_uint32 * nf)(*offs), ks2, fl2)
    assert list(fl2.raw[:len(batch)]) == [0] * len(good) + [0x80]
    for i, rec in enumerate(records):
        assert ks2.raw[64 * i:64 * i + 64] == rec[:64]


def check_patch(ac):
    r = random.Random(41)
    n = 300
    ks = bytearray(r.randrange(256) for _ in range(64 * n))
    which = sorted(r.sample(range(n), 70))
    patch = bytes(r.randrange(256) for _ in range(64 * len(which)))
    buf = C.create_string_buffer(bytes(ks) + b"\x99")
    ac.hc_admit_patch(buf, (C.c_uint32 * len(which))(*which), patch + b"\0", len(which))
    for t, i in enumerate(which):
        ks[64 * i:64 * i + 64] = patch[64 * t:64 * t + 64]
    assert buf.raw[:64 * n + 1] == bytes(ks) + b"\x99"


def check_all_lane_bodies(ac, records=None, L=None, variants=None):
    check_decision(ac)
    check_screen(ac)
    check_compaction(ac)
    check_gather_scatter(ac)
    check_patch(ac)
    if records:
        check_framing(ac, records, L, variants)
