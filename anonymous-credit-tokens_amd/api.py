"""Host-side mirror of the reference crate's public interface (/root/reference/src/lib.rs) over the
C ABI: same type names, method names, argument meaning and error behaviour, with `*_batch`
siblings that take lists.  Every method is one (batched) call into the HIP engine; nothing here
computes curve or scalar arithmetic.  Values are held as the raw records of include/act_mi355x.h.

    params = Params.new("org", "svc", "prod", "2024-01-15")                 # src/lib.rs:291
    sk = PrivateKey.random(OsRng())                                            # :188
    pre = PreIssuance.random(rng); req = pre.request(params, rng)              # :432, :463
    resp = sk.issue(params, req, 20, rng)                                      # :621  (raises Error)
    tok = pre.to_credit_token(params, sk.public(), req, resp)                  # :528
    proof, prerefund = tok.prove_spend(params, 5, rng)                         # :972
    refund = sk.refund(params, proof, rng)                                     # :781  (raises Error)
    tok2 = prerefund.to_credit_token(params, proof, refund, sk.public())       # :1217
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

from . import capi

L = 128  # src/lib.rs:116

_ELL = 2**252 + 27742317777372353535851937790883648493


class Error(Exception):
    """Mirror of `enum Error` (src/lib.rs:102-112); `code` = 1 + discriminant, 255 = undecodable point."""
    NAMES = {1: "InvalidIssuanceRequestProof", 2: "InvalidIssuanceResponseProof", 3: "DoubleSpendError",
             4: "InvalidRefundProof", 5: "InvalidRefundResponseProof", 6: "IdentityPointError",
             7: "InvalidClientSpendProof", 8: "AmountTooBigError", 9: "ScalarOutOfRangeError", 255: "UndecodablePoint",
             250: "WrongCharge", 249: "ReturnTooBig"}      # 250: the admission calls only; 249: the return calls only (not variants of the crate's enum)

    def __init__(self, code: int):
        super().__init__(self.NAMES.get(code, f"status {code}"))
        self.code = code
        self.name = self.NAMES.get(code, str(code))


class CborError(Exception):
    """Mirror of `enum CborError` (src/cbor.rs:30-37): Ciborium (malformed CBOR), InvalidStructure, InvalidValue."""
    NAMES = {1: "Ciborium", 2: "InvalidStructure", 3: "InvalidValue"}

    def __init__(self, code: int):
        super().__init__(self.NAMES.get(code, f"status {code}"))
        self.code = code
        self.name = self.NAMES.get(code, str(code))


class _Cbor:
    """to_cbor / from_cbor of the crate's wire and state types (src/cbor.rs:94-695) through the batch codec of the engine:
    deterministic RFC 8949 encoding with integer keys; from_cbor accepts what ciborium accepts, reduces scalars mod l and rejects
    points that are not canonical Ristretto encodings."""
    CBOR_TYPE = None

    def to_cbor(self, params: "Params" = None) -> bytes:
        nbits = getattr(self, "nbits", L)
        return _codec_engine(params, nbits).cbor_encode(self.CBOR_TYPE, self.record)[0]

    @classmethod
    def from_cbor(cls, data: bytes, params: "Params" = None, nbits: int = L):
        st, rec = _codec_engine(params, nbits).cbor_decode(cls.CBOR_TYPE, [bytes(data)])
        if st[0]:
            raise CborError(st[0])
        return cls(rec, nbits) if cls.CBOR_TYPE == "SpendProof" else cls(rec)


def _codec_engine(params, nbits):
    # the codec does not depend on the Params; any context of the right range width will do
    return (params or Params.new("act", "keygen", "default", "1970-01-01")).engine(nbits)


class OsRng:
    """CryptoRngCore stand-in backed by os.urandom."""

    def fill_bytes(self, n: int) -> bytes:
        return os.urandom(n)


class ByteStreamRng:
    """Deterministic CryptoRngCore stand-in replaying a byte string (tests; parity runs)."""

    def __init__(self, data: bytes):
        self.data, self.pos = bytes(data), 0

    def fill_bytes(self, n: int) -> bytes:
        if self.pos + n > len(self.data):
            raise ValueError("rng stream exhausted")
        out = self.data[self.pos:self.pos + n]
        self.pos += n
        return out

    def peek(self, n: int) -> bytes:
        return self.data[self.pos:self.pos + n].ljust(n, b"\0")

    def advance(self, n: int):
        self.pos += n


def _wire_error(status: int):
    """lane status of a wire-level call -> the error the crate's two calls would have produced"""
    return CborError({254: 1, 253: 2, 255: 3}[status]) if status in (253, 254, 255) else Error(status)


def _draw_signed(rng, n_lanes: int, run):
    """The wire-level calls take the generator itself (ACT_RNG_CALLBACK): the library draws 128 bytes per lane it SIGNS, once, after
    every verdict is known.  `rng.fill_bytes(k)` is called with exactly that many bytes."""
    import ctypes as C

    cb = capi.rng_trampoline(rng.fill_bytes)          # an exception in fill_bytes, or a short read, fails the call: nothing is signed
    src = capi.RngSource(cb, None)
    holder = type("Src", (), {"ptr": C.addressof(src), "keep": (cb, src)})()
    return run(_CallbackRng(holder), capi.RNG_CALLBACK)


class _CallbackRng(capi.ReplayRng):
    """adapter: a capi.ReplayRng-shaped object (what capi._rng_arg accepts) around an arbitrary act_rng_source"""

    def __init__(self, holder):
        self._holder = holder

    @property
    def ptr(self):
        return self._holder.ptr


def scalar(v) -> bytes:
    """Scalar::from(u128) / canonical 32-byte little-endian scalar."""
    if isinstance(v, (bytes, bytearray)):
        assert len(v) == 32
        return bytes(v)
    return (int(v) % _ELL).to_bytes(32, "little")


def scalar_to_u128(s: bytes):
    """src/lib.rs:146-153: Some(value) iff the high 16 bytes are zero."""
    return int.from_bytes(s[:16], "little") if not any(s[16:]) else None


def _check_then_sign(rng, check, sign):
    """issue / refund draw e, alpha only AFTER the checks have passed (src/lib.rs:638-643, 842-846): a rejected item leaves the caller's
    generator untouched.  So: `check()` -> (statuses, whatever the signature needs); exactly 128 bytes per ACCEPTED lane are drawn, in
    lane order, with ONE fill_bytes call; `sign(state, statuses, bytes)` -> (statuses, records).  Two library calls, the crate's contract
    for ANY generator (round 5 drew 128 bytes per lane up front unless the generator could peek)."""
    st, state = check()
    accepted = sum(1 for s in st if s == 0)
    drawn = rng.fill_bytes(128 * accepted) if accepted else b""
    if len(drawn) != 128 * accepted:
        raise ValueError("generator returned %d bytes, %d asked" % (len(drawn), 128 * accepted))
    return sign(state, st, drawn + b"\0")          # (+ one byte: never an empty buffer at the C boundary)


class Params:
    _engines: dict = {}

    def __init__(self, h: bytes, device: int = 0):
        self.h, self.device = bytes(h), device

    @staticmethod
    def new(organization: str, service: str, deployment_id: str, version: str, device: int = 0) -> "Params":
        return Params(capi.params_new(organization, service, deployment_id, version, device), device)

    @staticmethod
    def random(rng, device: int = 0) -> "Params":
        return Params(capi.params_random(rng.fill_bytes(192), device), device)

    def engine(self, nbits: int = L) -> capi.Engine:
        key = (self.h, nbits, self.device)
        if key not in Params._engines:
            mode = capi.TRANSCRIPT_DEVICE if os.environ.get("ACT_TRANSCRIPT", "host") == "device" else capi.TRANSCRIPT_HOST
            Params._engines[key] = capi.Engine(self.h, nbits, self.device, transcript=mode)
        return Params._engines[key]

    def __eq__(self, other):
        # the reference compares self.h3 with other.h2 (src/lib.rs:233); mirrored, quirk included
        return self.h[0:32] == other.h[0:32] and self.h[32:64] == other.h[32:64] and self.h[64:96] == other.h[32:64]

    def __ne__(self, other):
        return not self.__eq__(other)


class PublicKey(_Cbor):
    CBOR_TYPE = "PublicKey"

    def __init__(self, w: bytes):
        self.w = bytes(w)
        self.record = self.w


class PrivateKey(_Cbor):
    CBOR_TYPE = "PrivateKey"

    def __init__(self, record: bytes):
        assert len(record) == 64
        self.record = bytes(record)

    @staticmethod
    def random(rng, params: Params = None) -> "PrivateKey":
        params = params or Params.new("act", "keygen", "default", "1970-01-01")
        return PrivateKey(params.engine().private_key_random(rng.fill_bytes(64)))

    def public(self) -> PublicKey:
        return PublicKey(self.record[32:])

    def issue(self, params: Params, request: "IssuanceRequest", c, rng) -> "IssuanceResponse":
        return self.issue_batch(params, [request], [c], rng)[0]

    def issue_batch(self, params: Params, requests: Sequence["IssuanceRequest"], cs: Sequence, rng) -> List["IssuanceResponse"]:
        e = params.engine()
        req = b"".join(r.record for r in requests); cc = b"".join(scalar(c) for c in cs)
        st, out = _check_then_sign(rng, lambda: (e.issue_check(req), None),
                                   lambda _s, st, rb: e.issue_sign(self.record, req, cc, st, rb, capi.RNG_SEQUENTIAL))
        res = [IssuanceResponse(out[160 * i:160 * i + 160]) if st[i] == 0 else Error(st[i]) for i in range(len(requests))]
        if len(res) == 1 and isinstance(res[0], Error):
            raise res[0]
        return res

    def refund(self, params: Params, spend_proof: "SpendProof", rng) -> "Refund":
        return self.refund_batch(params, [spend_proof], rng)[0]

    def refund_batch(self, params: Params, proofs: Sequence["SpendProof"], rng) -> List["Refund"]:
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        st, out = _check_then_sign(rng, lambda: e.verify_spend(self.record, pb, True),
                                   lambda kp, st, rb: e.refund_sign(self.record, kp, st, rb, capi.RNG_SEQUENTIAL))
        res = [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))]
        if len(res) == 1 and isinstance(res[0], Error):
            raise res[0]
        return res

    def redeem_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng) -> List["Refund"]:
        """The server loop of examples/act.rs:62-73 as one call: verify, look the nullifier up, record it, sign.  Entry i is a
        Refund, or Error (DoubleSpendError for a nullifier already recorded / spent by an earlier accepted proof of the batch)."""
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        st, out = _draw_signed(rng, len(proofs), lambda src, mode: e.redeem(db.set, self.record, pb, src, mode))      # the generator itself: drawn once, after the nullifier step, for the lanes that are signed
        return [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))]

    # ---- wire bytes in, wire bytes out (rust/src/mi355x.rs refund_cbor_batch / redeem_cbor_batch) ----------
    def refund_cbor_batch(self, params: Params, msgs: Sequence[bytes], rng, nbits: int = L) -> list:
        """`[SpendProof::from_cbor(m).and_then(|p| self.refund(params, &p, rng)).map(to_cbor) for m in msgs]` as one call: entry i is
        the CBOR Refund message, a CborError (from_cbor's) or an Error (refund's); `rng` is drawn for the accepted messages only, in
        message order, after all verdicts (src/lib.rs:842-852)."""
        e = params.engine(nbits)
        st, out = _draw_signed(rng, len(msgs), lambda src, mode: e.refund_cbor(self.record, list(msgs), src, mode))
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))]

    def issue_cbor_batch(self, params: Params, msgs: Sequence[bytes], cs: Sequence, rng) -> list:
        """`[IssuanceRequest::from_cbor(m).and_then(|r| self.issue(params, &r, c, rng)).map(to_cbor) for m, c in zip(msgs, cs)]` as one
        call: entry i is the CBOR IssuanceResponse message, a CborError (from_cbor's) or an Error (issue's); `rng` is drawn for the
        accepted messages only, in message order, after all verdicts (src/lib.rs:638-643)."""
        e = params.engine()
        cc = b"".join(scalar(c) for c in cs)
        st, out = _draw_signed(rng, len(msgs), lambda src, mode: e.issue_cbor(self.record, list(msgs), cc, src, mode))
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))]

    def redeem_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L) -> list:
        """The server loop of examples/act.rs:62-73 on wire bytes: from_cbor, refund's checks, the nullifier store (DoubleSpendError),
        the signature, to_cbor."""
        e = params.engine(nbits)
        st, out = _draw_signed(rng, len(msgs), lambda src, mode: e.redeem_cbor(db.set, self.record, list(msgs), src, mode))
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))]

    # ---- admission before verification: the expected charge and the spent nullifiers first ------------------
    def redeem_admit_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng, charges: Sequence = None, unique: bool = False) -> List["Refund"]:
        """redeem_batch with the admission stage in front: entry i is a Refund, Error 250 (WrongCharge: proof i does not spend
        charges[i]; nothing was recorded, the token can still be redeemed at the right price) or the Errors of redeem_batch -- a
        nullifier that is already recorded is answered DoubleSpendError WITHOUT the proof being verified.  unique=True: a proof with
        the bytes of an earlier proof of the batch is not verified either (act_redeem_admit_unique_batch); the same entries."""
        res, _ = Keyring([self]).redeem_admit_batch(params, db, proofs, rng, charges=charges, unique=unique)
        return res

    def redeem_admit_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L, charges: Sequence = None, unique: bool = False) -> list:
        res, _ = Keyring([self]).redeem_admit_cbor_batch(params, db, msgs, rng, nbits, charges=charges, unique=unique)
        return res

    # ---- partial refunds: the issuer returns t <= s unused credits with the Refund --------------------------
    def refund_return(self, params: Params, spend_proof: "SpendProof", t, rng) -> "RefundReturn":
        """refund, returning t of the s credits the proof spends: the client's next token holds c - s + t.  Error 249 (ReturnTooBig)
        when t > s -- checked HERE, against the proof's own s, because the sign-only call underneath does not see s; like every
        rejection it leaves the generator untouched."""
        e = params.engine(spend_proof.nbits)
        tt = scalar(t)

        def check():
            st, kp = e.verify_spend(self.record, spend_proof.record, True)
            if st[0] == 0 and int.from_bytes(tt, "little") > int.from_bytes(scalar(int.from_bytes(spend_proof.charge(), "little")), "little"):
                st = bytes([capi.STATUS_RETURN_TOO_BIG])
            return st, kp
        st, out = _check_then_sign(rng, check, lambda kp, st, rb: e.refund_sign_return_keyring([self.record], bytes(1), kp, st, rb, tt, capi.RNG_SEQUENTIAL))
        if st[0]:
            raise Error(st[0])
        return RefundReturn(out)

    def redeem_return_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng, returned: Sequence = None, charges: Sequence = None,
                            unique: bool = False) -> List["RefundReturn"]:
        """redeem_admit_batch with the amounts the issuer returns (Keyring.redeem_return_batch): entry i is a RefundReturn or an Error"""
        res, _ = Keyring([self]).redeem_return_batch(params, db, proofs, rng, returned=returned, charges=charges, unique=unique)
        return res

    def redeem_return_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L, returned: Sequence = None, charges: Sequence = None,
                                 unique: bool = False) -> list:
        res, _ = Keyring([self]).redeem_return_cbor_batch(params, db, msgs, rng, nbits, returned=returned, charges=charges, unique=unique)
        return res

    # ---- replayable redemption: a retried SpendProof gets its Refund again ----------------------------------
    def redeem_replay_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], nonce_key: bytes,
                            admit: bool = False, charges: Sequence = None, unique: bool = False, returned: Sequence = None, binds: Sequence = None) -> Tuple[list, list]:
        """redeem_batch without a generator: the nonces are derived from `nonce_key` (32 secret bytes the issuer keeps), this key, the
        nullifier and K', and `receipts` (a second NullifierDb) remembers which K' a nullifier was spent for -- a proof that is sent
        again gets the same Refund, byte for byte, instead of DoubleSpendError.  admit / charges / unique / returned / binds: Keyring.redeem_replay_batch.  -> (results, replayed flags)"""
        res, _, replayed = Keyring([self]).redeem_replay_batch(params, db, receipts, proofs, nonce_key, admit=admit, charges=charges, unique=unique, returned=returned,
                                                               binds=binds)
        return res, replayed

    def redeem_replay_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nonce_key: bytes, nbits: int = L,
                                 admit: bool = False, charges: Sequence = None, unique: bool = False, returned: Sequence = None, binds: Sequence = None) -> Tuple[list, list]:
        res, _, replayed = Keyring([self]).redeem_replay_cbor_batch(params, db, receipts, msgs, nonce_key, nbits, admit=admit, charges=charges, unique=unique,
                                                                    returned=returned, binds=binds)
        return res, replayed

    def redeem_return_replay_unique_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], nonce_key: bytes,
                                          returned: Sequence = None, charges: Sequence = None) -> Tuple[list, list]:
        """Keyring.redeem_return_replay_unique_batch with this key alone.  -> (results, replayed flags)"""
        res, _, replayed = Keyring([self]).redeem_return_replay_unique_batch(params, db, receipts, proofs, nonce_key, returned=returned, charges=charges)
        return res, replayed

    def redeem_return_replay_unique_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nonce_key: bytes, nbits: int = L,
                                               returned: Sequence = None, charges: Sequence = None) -> Tuple[list, list]:
        res, _, replayed = Keyring([self]).redeem_return_replay_unique_cbor_batch(params, db, receipts, msgs, nonce_key, nbits, returned=returned, charges=charges)
        return res, replayed

    # ---- reserve and settle: record a spend now, sign its partial refund later -----------------------------------
    def reserve_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], charges: Sequence = None,
                      binds: Sequence = None) -> Tuple[list, list]:
        """Keyring.reserve_batch with this key alone.  -> (results: a Reservation or an Error per proof, replayed flags)"""
        return Keyring([self]).reserve_batch(params, db, receipts, proofs, charges=charges, binds=binds)

    def reserve_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nbits: int = L, charges: Sequence = None,
                           binds: Sequence = None) -> Tuple[list, list]:
        return Keyring([self]).reserve_cbor_batch(params, db, receipts, msgs, nbits, charges=charges, binds=binds)

    def settle_batch(self, params: Params, receipts: "NullifierDb", reservations: Sequence["Reservation"], returned: Sequence, nonce_key: bytes, nbits: int = L,
                     cbor: bool = False) -> Tuple[list, list]:
        """Keyring.settle_batch with this key alone.  -> (results, settled-before flags)"""
        return Keyring([self]).settle_batch(params, receipts, reservations, returned, nonce_key, nbits=nbits, cbor=cbor)

    def verify_spend_batch(self, params: Params, proofs: Sequence["SpendProof"], binds: Sequence = None) -> bytes:
        """binds (one 32-byte request binding per proof): Keyring.verify_spend_batch with this key alone -- a ring of one key is the
        bound one-key call"""
        nbits = proofs[0].nbits if proofs else L
        if binds is not None:
            return Keyring([self]).verify_spend_batch(params, proofs, binds=binds)[0]
        return params.engine(nbits).verify_spend(self.record, b"".join(p.record for p in proofs))


class Keyring:
    """Key rotation: an ordered ring of up to four issuer keys (the caller's order of preference -- usually newest first) that one
    batch is verified and refunded against.  A SpendProof names no key; every method returns what the PrivateKey method of the same
    name returns PLUS, per proof, the ring index it verified under (None where no ring key accepts it).  `sign_with=None` signs every
    refund with the key its proof matched; `sign_with=i` signs every accepted lane with ring key i, which moves the client onto that
    key with its next token (the client then calls to_credit_token with `ring.public(i)`).  The nullifier database is shared by all
    keys; `Params` must be the ones every ring key issued under.  `epochs` (one per key, 0 .. 2^24 - 1: the caller's stable name for
    each key): redeem_batch / redeem_cbor_batch record every accepted nullifier under the epoch of the key its proof matched, so that
    NullifierDb.retire can drop a key's nullifiers once the key has left every ring for good."""

    def __init__(self, keys: Sequence[PrivateKey], epochs: Sequence[int] = None):
        if not 1 <= len(keys) <= capi.KEYRING_MAX:
            raise ValueError("a key ring holds 1 .. %d keys" % capi.KEYRING_MAX)
        if epochs is not None and len(epochs) != len(keys):
            raise ValueError("epochs: one per ring key")
        self.keys = list(keys)
        self.epochs = list(epochs) if epochs is not None else None

    def public(self, i: int) -> PublicKey:
        return self.keys[i].public()

    def _records(self):
        return [k.record for k in self.keys]

    def _sign_key(self, sign_with):
        if sign_with is None:
            return capi.SIGN_MATCHED
        if not 0 <= sign_with < len(self.keys):
            raise ValueError("sign_with is not a ring index")
        return sign_with

    @staticmethod
    def _indices(st, ok):
        return [ok[i] if ok[i] != capi.KEY_NONE else None for i in range(len(st))]

    @staticmethod
    def _binds(binds, n):
        """request bindings (INTEGRATION.md "request binding"): one 32-byte value per lane -> n * 32 bytes"""
        if len(binds) != n or any(len(b) != 32 for b in binds):
            raise ValueError("binds: one 32-byte request binding per proof")
        return b"".join(bytes(b) for b in binds)

    def verify_spend_batch(self, params: Params, proofs: Sequence["SpendProof"], binds: Sequence = None) -> Tuple[bytes, list]:
        """binds (one 32-byte request binding per proof; act_verify_spend_keyring_bound_batch): proof i verifies only if it was made
        with binds[i] (CreditToken.prove_spend(..., bind=)); a proof made without a binding does not verify under any"""
        nbits = proofs[0].nbits if proofs else L
        if binds is not None:
            st, ok = params.engine(nbits).verify_spend_keyring(self._records(), b"".join(p.record for p in proofs), bind=self._binds(binds, len(proofs)))
        else:
            st, ok = params.engine(nbits).verify_spend_keyring(self._records(), b"".join(p.record for p in proofs))
        return st, self._indices(st, ok)

    def refund_batch(self, params: Params, proofs: Sequence["SpendProof"], rng, sign_with=None) -> Tuple[list, list]:
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        sk = self._sign_key(sign_with)
        matched = []

        def check():
            st, ok, kp = e.verify_spend_keyring(self._records(), pb, True)
            matched.append(ok)
            return st, (kp, ok if sk < 0 else bytes([sk]) * len(st))
        st, out = _check_then_sign(rng, check, lambda s, st, rb: e.refund_sign_keyring(self._records(), s[1], s[0], st, rb, capi.RNG_SEQUENTIAL))
        res = [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))]
        return res, self._indices(st, matched[0] if matched else b"")

    def redeem_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng, sign_with=None) -> Tuple[list, list]:
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        st, out, ok = _draw_signed(rng, len(proofs), lambda src, mode: e.redeem_keyring(db.set, self._records(), pb, src, mode, self._sign_key(sign_with), key_epochs=self.epochs))
        return [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok)

    def redeem_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L, sign_with=None) -> Tuple[list, list]:
        e = params.engine(nbits)
        st, out, ok = _draw_signed(rng, len(msgs), lambda src, mode: e.redeem_cbor_keyring(db.set, self._records(), list(msgs), src, mode, self._sign_key(sign_with), key_epochs=self.epochs))
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok)

    def redeem_admit_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng, sign_with=None, charges: Sequence = None, unique: bool = False) -> Tuple[list, list]:
        """redeem_batch behind the admission stage (act_redeem_admit_batch): `charges` (optional, one per proof) is what each request
        costs -- a proof whose s differs is answered Error 250 and is neither looked up, verified nor recorded; a proof whose nullifier
        the database already holds is answered DoubleSpendError without being verified.  `self.last_admit_counts`: the call's counts.
        unique=True (act_redeem_admit_unique_batch): byte-identical proofs of the batch are verified once; the results are the same
        and the counts gain "copies"."""
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        st, out, ok, self.last_admit_counts = _draw_signed(rng, len(proofs), lambda src, mode: e.redeem_admit(
            db.set, self._records(), pb, src, mode, self._sign_key(sign_with), charges=cc, key_epochs=self.epochs, unique=unique))
        return [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok)

    def redeem_admit_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L, sign_with=None, charges: Sequence = None, unique: bool = False) -> Tuple[list, list]:
        e = params.engine(nbits)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        st, out, ok, self.last_admit_counts = _draw_signed(rng, len(msgs), lambda src, mode: e.redeem_cbor_admit(
            db.set, self._records(), list(msgs), src, mode, self._sign_key(sign_with), charges=cc, key_epochs=self.epochs, unique=unique))
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok)

    def redeem_return_batch(self, params: Params, db: "NullifierDb", proofs: Sequence["SpendProof"], rng, returned: Sequence = None, charges: Sequence = None,
                            sign_with=None, unique: bool = False) -> Tuple[list, list]:
        """The reserve-then-return server step (act_redeem_return_batch): redeem_admit_batch, and every accepted proof is refunded
        with returned[i] of the s_i credits it spends -- entry i is a RefundReturn whose client ends with c - s_i + returned[i].
        returned[i] > s_i is Error 249: not looked up, not verified, not recorded, not signed.  `self.last_admit_counts`: the call's
        counts (capi.REDEEM_RETURN_COUNTS), also kept as `self.last_return_counts`.  unique=True (act_redeem_return_unique_batch): a
        proof with the bytes of an earlier proof of the batch is not verified, WHATEVER its returned amount -- the first one is the one
        that is signed, over its own amount, and the others are DoubleSpendError as they are without unique; the results are the same
        and the counts gain "copies" (capi.REDEEM_RETURN_UNIQUE_COUNTS, ten names).  The retry-safe form of this call is redeem_replay_batch(..., returned=)."""
        nbits = proofs[0].nbits if proofs else L
        e = params.engine(nbits)
        pb = b"".join(p.record for p in proofs)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        tt = b"".join(scalar(t) for t in returned) if returned is not None else None
        st, out, ok, self.last_admit_counts = _draw_signed(rng, len(proofs), lambda src, mode: e.redeem_return(
            db.set, self._records(), pb, src, mode, self._sign_key(sign_with), charges=cc, returned=tt, key_epochs=self.epochs, unique=unique))
        self.last_return_counts = self.last_admit_counts
        return [RefundReturn(out[160 * i:160 * i + 160]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok)

    def redeem_return_cbor_batch(self, params: Params, db: "NullifierDb", msgs: Sequence[bytes], rng, nbits: int = L, returned: Sequence = None,
                                 charges: Sequence = None, sign_with=None, unique: bool = False) -> Tuple[list, list]:
        """the same on wire bytes (act_redeem_cbor_return_batch; unique=True: act_redeem_cbor_return_unique_batch, a copy has the same
        length and the same bytes as an earlier message): entry i is a CBOR RefundReturn message, a CborError or an Error"""
        e = params.engine(nbits)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        tt = b"".join(scalar(t) for t in returned) if returned is not None else None
        st, out, ok, self.last_admit_counts = _draw_signed(rng, len(msgs), lambda src, mode: e.redeem_cbor_return(
            db.set, self._records(), list(msgs), src, mode, self._sign_key(sign_with), charges=cc, returned=tt, key_epochs=self.epochs, unique=unique))
        self.last_return_counts = self.last_admit_counts
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok)

    def redeem_replay_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], nonce_key: bytes, sign_with=None,
                            admit: bool = False, charges: Sequence = None, unique: bool = False, returned: Sequence = None, binds: Sequence = None) -> Tuple[list, list, list]:
        """redeem_batch made retry-safe (act_redeem_replay_batch): no generator -- the nonces are derived from `nonce_key`, the key a
        lane is signed with, the nullifier and K' -- and `receipts`, a second NullifierDb, records for which K' every nullifier was
        spent.  A proof that is sent again (same ring key to sign with, same nonce_key) gets the same Refund, byte for byte; another
        proof for the same nullifier is DoubleSpendError as before.  Retire an epoch on both databases.
        admit=True (act_redeem_admit_replay_batch): the admission screen in front -- `charges` (optional, one per proof; Error 250 for
        a proof whose s differs) and the spent nullifiers first: a proof whose nullifier is spent and whose receipt is not its own is
        DoubleSpendError WITHOUT being verified, a retry is verified and served.  Accepted lanes, refunds and both databases end as
        without it; the counts are capi.ADMIT_REPLAY_COUNTS.
        unique=True (with admit=True; act_redeem_admit_replay_unique_batch): byte-identical proofs of the batch are verified and signed
        once and the copies get the same Refund; the results are the same and the counts gain "copies" and "copies_served".
        returned (one amount per proof; act_redeem_return_replay_batch; implies admit=True): the reserve-then-return step made
        retry-safe -- entry i is a RefundReturn over returned[i]; returned[i] > s_i is Error 249.  The receipt PINS the amount: a proof
        sent again with the same amount gets the same RefundReturn, with another amount DoubleSpendError -- derive the amount from the
        request, or remember it.  The counts are capi.RETURN_REPLAY_COUNTS.  Not with unique=True (ValueError): that form is a method
        of its own, redeem_return_replay_unique_batch.
        binds (one 32-byte request binding per proof; with admit=True; act_redeem_return_replay_bound_batch): proof i is verified under
        binds[i] -- a proof made with another binding, or with none, is Error 7 and nothing is recorded or signed for it; the binding
        enters neither the receipt nor the nonces, so a retry under the same binding gets the same bytes.  Entry i is a RefundReturn
        (over 0 where `returned` is None).  Not with unique=True (ValueError): the bound calls have no unique form.
        -> (results, matched ring indices, replayed flags); `self.last_replay_counts`: the call's counts."""
        nbits = proofs[0].nbits if proofs else L
        if returned is not None and unique:
            raise ValueError("a copy may name another amount than its leader: the unique form with returned amounts is redeem_return_replay_unique_batch")
        if binds is not None:
            if unique:
                raise ValueError("request binding: the bound calls have no unique form")
            if not admit and returned is None:
                raise ValueError("request binding: the bound redeem call is an admission call: admit=True")
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            tt = b"".join(scalar(t) for t in returned) if returned is not None else None
            st, out, ok, rep, self.last_replay_counts = params.engine(nbits).redeem_return_replay(
                db.set, receipts.set, self._records(), b"".join(p.record for p in proofs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc,
                returned=tt, bind=self._binds(binds, len(proofs)))
            return [RefundReturn(out[160 * i:160 * i + 160]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok), [bool(r) for r in rep]
        admit = admit or returned is not None
        if charges is not None and not admit:
            raise ValueError("charges are compared by the admission screen: admit=True")
        if unique and not admit:
            raise ValueError("copies are found behind the admission screen: admit=True")
        e, pb = params.engine(nbits), b"".join(p.record for p in proofs)
        if returned is not None:
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            tt = b"".join(scalar(t) for t in returned)
            st, out, ok, rep, self.last_replay_counts = e.redeem_return_replay(
                db.set, receipts.set, self._records(), pb, nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, returned=tt)
            return [RefundReturn(out[160 * i:160 * i + 160]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok), [bool(r) for r in rep]
        if admit:
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            st, out, ok, rep, self.last_replay_counts = e.redeem_admit_replay(
                db.set, receipts.set, self._records(), pb, nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, unique=unique)
        else:
            st, out, ok, rep, self.last_replay_counts = e.redeem_replay(db.set, receipts.set, self._records(), pb, nonce_key, self._sign_key(sign_with), key_epochs=self.epochs)
        return [Refund(out[128 * i:128 * i + 128]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok), [bool(r) for r in rep]

    def redeem_replay_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nonce_key: bytes, nbits: int = L,
                                 sign_with=None, admit: bool = False, charges: Sequence = None, unique: bool = False, returned: Sequence = None,
                                 binds: Sequence = None) -> Tuple[list, list, list]:
        """the same on wire bytes (act_redeem_cbor_replay_batch; admit=True: act_redeem_cbor_admit_replay_batch): a retry may be another
        CBOR spelling of the same proof.  unique=True (with admit=True): act_redeem_cbor_admit_replay_unique_batch -- a copy is a message
        of the same length and the same bytes; another spelling is verified on its own.  returned: act_redeem_cbor_return_replay_batch --
        entry i is a CBOR RefundReturn message (implies admit=True; not with unique=True: redeem_return_replay_unique_cbor_batch).
        binds: as in redeem_replay_batch (act_redeem_cbor_return_replay_bound_batch); entry i is a CBOR RefundReturn message"""
        if returned is not None and unique:
            raise ValueError("a copy may name another amount than its leader: the unique form with returned amounts is redeem_return_replay_unique_cbor_batch")
        if binds is not None:
            if unique:
                raise ValueError("request binding: the bound calls have no unique form")
            if not admit and returned is None:
                raise ValueError("request binding: the bound redeem call is an admission call: admit=True")
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            tt = b"".join(scalar(t) for t in returned) if returned is not None else None
            st, out, ok, rep, self.last_replay_counts = params.engine(nbits).redeem_cbor_return_replay(
                db.set, receipts.set, self._records(), list(msgs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, returned=tt,
                bind=self._binds(binds, len(msgs)))
            return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok), [bool(r) for r in rep]
        admit = admit or returned is not None
        if charges is not None and not admit:
            raise ValueError("charges are compared by the admission screen: admit=True")
        if unique and not admit:
            raise ValueError("copies are found behind the admission screen: admit=True")
        e = params.engine(nbits)
        if returned is not None:
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            tt = b"".join(scalar(t) for t in returned)
            st, out, ok, rep, self.last_replay_counts = e.redeem_cbor_return_replay(
                db.set, receipts.set, self._records(), list(msgs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, returned=tt)
        elif admit:
            cc = b"".join(scalar(c) for c in charges) if charges is not None else None
            st, out, ok, rep, self.last_replay_counts = e.redeem_cbor_admit_replay(
                db.set, receipts.set, self._records(), list(msgs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, unique=unique)
        else:
            st, out, ok, rep, self.last_replay_counts = e.redeem_cbor_replay(db.set, receipts.set, self._records(), list(msgs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs)
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok), [bool(r) for r in rep]

    def redeem_return_replay_unique_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], nonce_key: bytes,
                                          returned: Sequence = None, sign_with=None, charges: Sequence = None) -> Tuple[list, list, list]:
        """redeem_replay_batch(..., returned=) with byte-identical proofs of the batch verified and signed once
        (act_redeem_return_replay_unique_batch).  A proof with the bytes of an earlier proof that passed the screen is a copy WHATEVER
        amount it names; behind the call it is answered from its leader: the leader's RefundReturn, byte for byte, if it names the
        leader's amount and the leader was accepted; DoubleSpendError if it names another amount (the receipt pins the leader's); the
        leader's error otherwise.  Results, matched keys, replayed flags and both databases are those of redeem_replay_batch(...,
        returned=) on the same batch; the counts are capi.RETURN_REPLAY_UNIQUE_COUNTS (fifteen names: "copies", "copies_served",
        "copies_other_amount" behind the twelve).  returned=None: every amount is 0.
        -> (results, matched ring indices, replayed flags); `self.last_replay_counts`: the call's counts."""
        nbits = proofs[0].nbits if proofs else L
        e, pb = params.engine(nbits), b"".join(p.record for p in proofs)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        tt = b"".join(scalar(t) for t in returned) if returned is not None else None
        st, out, ok, rep, self.last_replay_counts = e.redeem_return_replay(
            db.set, receipts.set, self._records(), pb, nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, returned=tt, unique=True)
        return [RefundReturn(out[160 * i:160 * i + 160]) if st[i] == 0 else Error(st[i]) for i in range(len(proofs))], self._indices(st, ok), [bool(r) for r in rep]

    def redeem_return_replay_unique_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nonce_key: bytes, nbits: int = L,
                                               returned: Sequence = None, sign_with=None, charges: Sequence = None) -> Tuple[list, list, list]:
        """the same on wire bytes (act_redeem_cbor_return_replay_unique_batch): a copy is a message of the same length and the same
        bytes; another spelling is verified on its own.  Entry i is a CBOR RefundReturn message or an Error."""
        e = params.engine(nbits)
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        tt = b"".join(scalar(t) for t in returned) if returned is not None else None
        st, out, ok, rep, self.last_replay_counts = e.redeem_cbor_return_replay(
            db.set, receipts.set, self._records(), list(msgs), nonce_key, self._sign_key(sign_with), key_epochs=self.epochs, charges=cc, returned=tt, unique=True)
        return [out[i] if st[i] == 0 else _wire_error(st[i]) for i in range(len(msgs))], self._indices(st, ok), [bool(r) for r in rep]


    # ---- reserve and settle (include/act_mi355x.h "reserve and settle") -------------------------------------------
    def _reservations(self, st, out, ok, rep):
        res = [Reservation(out[96 * i:96 * i + 96], ok[i]) if st[i] == 0 else Error(st[i]) for i in range(len(st))]
        return res, [bool(r) for r in rep]

    def reserve_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", proofs: Sequence["SpendProof"], charges: Sequence = None,
                      binds: Sequence = None) -> Tuple[list, list]:
        """The first half of the metered-service step (act_redeem_reserve_batch): redeem_replay_batch(..., admit=True) WITHOUT the
        signature.  Every proof is screened (`charges`, optional: Error 250 where s differs; a spent nullifier that is not this proof's
        own reservation: DoubleSpendError, unverified), verified and RECORDED as spent, and entry i is a Reservation -- what the service
        keeps beside the job until it knows what the work cost.  No nonce_key, no generator: nothing is signed.  A proof that is sent
        again gets the same Reservation and replayed[i] = True: the job for it exists already -- never start a second one.
        binds (one 32-byte request binding per proof; act_redeem_reserve_bound_batch): proof i is verified under binds[i]; a recorded
        reservation's proof sent again beside ANOTHER request is Error 7, not a replay.
        -> (results, replayed flags); `self.last_reserve_counts`: the call's counts (capi.RESERVE_COUNTS)."""
        nbits = proofs[0].nbits if proofs else L
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        kw = dict(bind=self._binds(binds, len(proofs))) if binds is not None else {}
        st, out, ok, rep, self.last_reserve_counts = params.engine(nbits).redeem_reserve(db.set, receipts.set, self._records(), b"".join(p.record for p in proofs),
                                                                                        key_epochs=self.epochs, charges=cc, **kw)
        return self._reservations(st, out, ok, rep)

    def reserve_cbor_batch(self, params: Params, db: "NullifierDb", receipts: "NullifierDb", msgs: Sequence[bytes], nbits: int = L, charges: Sequence = None,
                           binds: Sequence = None) -> Tuple[list, list]:
        """the same on CBOR SpendProof messages (act_redeem_cbor_reserve_batch): a retry may be another spelling of the same proof.  Entry i
        is a Reservation, a CborError or an Error -- the reservation has no wire type, it never goes to a client.  binds: as in
        reserve_batch (act_redeem_cbor_reserve_bound_batch)"""
        cc = b"".join(scalar(c) for c in charges) if charges is not None else None
        kw = dict(bind=self._binds(binds, len(msgs))) if binds is not None else {}
        st, out, ok, rep, self.last_reserve_counts = params.engine(nbits).redeem_cbor_reserve(db.set, receipts.set, self._records(), list(msgs), key_epochs=self.epochs, charges=cc,
                                                                                             **kw)
        res, replayed = self._reservations(st, out, ok, rep)
        return [r if st[i] == 0 else _wire_error(st[i]) for i, r in enumerate(res)], replayed

    def settle_batch(self, params: Params, receipts: "NullifierDb", reservations: Sequence["Reservation"], returned: Sequence, nonce_key: bytes, nbits: int = L,
                     sign_with=None, cbor: bool = False) -> Tuple[list, list]:
        """The second half (act_redeem_settle_batch): the work behind reservations[i] cost s_i - returned[i].  The reservation is looked
        up in `receipts` (Error 248: not reserved -- altered, recorded by a one-phase call, or its epoch retired), the amount is bound
        (returned[i] > s_i: Error 249) and PINNED, and entry i is the RefundReturn over returned[i], signed with nonces derived from
        `nonce_key`.  Settling a reservation again with the same amount gives the same bytes (settled_before[i] = True); with another
        amount Error 247.  After settlement a client that resends its SpendProof is served by redeem_replay_batch(..., returned=).
        returned=None: every amount is 0.  cbor=True (act_redeem_cbor_settle_batch): entry i is a CBOR RefundReturn message.
        -> (results, settled-before flags); `self.last_settle_counts`: the call's counts (capi.SETTLE_COUNTS)."""
        tt = b"".join(scalar(t) for t in returned) if returned is not None else None
        st, out, before, self.last_settle_counts = params.engine(nbits).redeem_settle(
            receipts.set, self._records(), b"".join(r.record for r in reservations), bytes(r.key for r in reservations), nonce_key, tt, self._sign_key(sign_with),
            key_epochs=self.epochs, cbor=cbor)
        n = len(reservations)
        res = [(out[i] if cbor else RefundReturn(out[160 * i:160 * i + 160])) if st[i] == 0 else Error(st[i]) for i in range(n)]
        return res, [bool(b) for b in before]


class PreIssuance(_Cbor):
    CBOR_TYPE = "PreIssuance"

    def __init__(self, record: bytes):
        assert len(record) == 64
        self.record = bytes(record)   # r | k

    @staticmethod
    def random(rng, params: Params = None) -> "PreIssuance":
        params = params or Params.new("act", "keygen", "default", "1970-01-01")
        return PreIssuance(params.engine().pre_issuance_random(rng.fill_bytes(128)))

    def request(self, params: Params, rng) -> "IssuanceRequest":
        return IssuanceRequest(params.engine().request(self.record, rng.fill_bytes(128)))

    def to_credit_token(self, params: Params, public: PublicKey, request: "IssuanceRequest", response: "IssuanceResponse") -> "CreditToken":
        st, out = params.engine().issuance_to_credit_token(self.record, public.w, request.record, response.record)
        if st[0]:
            raise Error(st[0])
        return CreditToken(out)

    def to_credit_token_ring(self, params: Params, publics: Sequence[PublicKey], request: "IssuanceRequest", response: "IssuanceResponse") -> Tuple["CreditToken", int]:
        """to_credit_token against the issuer's published keys (1 .. 4, in the caller's order of preference) while it rotates them:
        -> (token, index of the first ring key the response verifies under); the one-key error when none does."""
        st, out, ok = params.engine().issuance_to_credit_token_ring(self.record, [p.w for p in publics], request.record, response.record)
        if st[0]:
            raise Error(st[0])
        return CreditToken(out), ok[0]


class IssuanceRequest(_Cbor):
    CBOR_TYPE = "IssuanceRequest"

    def __init__(self, record: bytes):
        assert len(record) == 128
        self.record = bytes(record)   # K | gamma | k_bar | r_bar


class IssuanceResponse(_Cbor):
    CBOR_TYPE = "IssuanceResponse"

    def __init__(self, record: bytes):
        assert len(record) == 160
        self.record = bytes(record)   # A | e | gamma | z | c


class CreditToken(_Cbor):
    CBOR_TYPE = "CreditToken"

    def __init__(self, record: bytes):
        assert len(record) == 160
        self.record = bytes(record)   # a | e | k | r | c

    def nullifier(self) -> bytes:
        return self.record[64:96]

    def credits(self) -> bytes:
        return self.record[128:160]

    def prove_spend(self, params: Params, s, rng, nbits: int = L, bind: bytes = None) -> Tuple["SpendProof", "PreRefund"]:
        """bind (32 bytes, typically a hash of the request this spend pays for; act_prove_spend_bound_batch): the bytes enter the
        proof's challenge, and the issuer verifies it under the same bytes (binds= of the Keyring / PrivateKey calls).  A bound proof
        is not a crate SpendProof: the crate's refund and every call here without its binding reject it."""
        e = params.engine(nbits)
        if bind is not None and len(bind) != 32:
            raise ValueError("bind: 32 bytes")
        kw = dict(bind=bytes(bind)) if bind is not None else {}
        st, proof, pre = e.prove_spend(self.record, scalar(s), rng.fill_bytes(e.prove_rng_bytes), **kw)
        if st[0]:
            raise Error(st[0])
        return SpendProof(proof, nbits), PreRefund(pre)

    def __eq__(self, other):
        return self.record == other.record


class SpendProof(_Cbor):
    CBOR_TYPE = "SpendProof"

    def __init__(self, record: bytes, nbits: int = L):
        assert len(record) == 32 * (14 + 4 * nbits)
        self.record, self.nbits = bytes(record), nbits

    def nullifier(self) -> bytes:
        return self.record[0:32]

    def charge(self) -> bytes:
        return self.record[32:64]


class PreRefund(_Cbor):
    CBOR_TYPE = "PreRefund"

    def __init__(self, record: bytes):
        assert len(record) == 96
        self.record = bytes(record)   # r | k | m

    def to_credit_token(self, params: Params, spend_proof: SpendProof, refund: "Refund", public_key: PublicKey) -> CreditToken:
        st, out = params.engine(spend_proof.nbits).refund_to_credit_token(self.record, spend_proof.record, refund.record, public_key.w)
        if st[0]:
            raise Error(st[0])
        return CreditToken(out)

    def to_credit_token_return(self, params: Params, spend_proof: SpendProof, refund_return: "RefundReturn", public_key: PublicKey) -> CreditToken:
        """to_credit_token over a RefundReturn: the proof is checked over X_A = g + K' + t h1 and the token holds m + t.  Error 4 when
        the proof fails (also when t was altered on the way), Error 8 (AmountTooBigError) for a validly signed t > s."""
        st, out = params.engine(spend_proof.nbits).refund_to_credit_token_return(self.record, spend_proof.record, refund_return.record, public_key.w)
        if st[0]:
            raise Error(st[0])
        return CreditToken(out)

    def to_credit_token_return_ring(self, params: Params, spend_proof: SpendProof, refund_return: "RefundReturn", publics: Sequence[PublicKey]) -> Tuple[CreditToken, int]:
        """to_credit_token_return against the issuer's published keys (act_refund_to_credit_token_return_keyring_batch): a RefundReturn
        names no key either, and Keyring.redeem_return_batch(sign_with=i) signs with any ring key.  -> (token holding m + t, index of the
        first ring key the record verifies under); Error 4 when no ring key does, Error 8 for a t > s that a ring key validly signed."""
        st, out, ok = params.engine(spend_proof.nbits).refund_to_credit_token_return_ring(self.record, spend_proof.record, refund_return.record, [p.w for p in publics])
        if st[0]:
            raise Error(st[0])
        return CreditToken(out), ok[0]

    def to_credit_token_ring(self, params: Params, spend_proof: SpendProof, refund: "Refund", publics: Sequence[PublicKey]) -> Tuple[CreditToken, int]:
        """to_credit_token against the issuer's published keys: a Refund names no key, and Keyring.refund_batch(sign_with=i) moves a
        client onto key i without telling it.  -> (token, index of the first ring key the refund verifies under)."""
        st, out, ok = params.engine(spend_proof.nbits).refund_to_credit_token_ring(self.record, spend_proof.record, refund.record, [p.w for p in publics])
        if st[0]:
            raise Error(st[0])
        return CreditToken(out), ok[0]


class Refund(_Cbor):
    CBOR_TYPE = "Refund"

    def __init__(self, record: bytes):
        assert len(record) == 128
        self.record = bytes(record)   # A* | e | gamma | z

    def __eq__(self, other):
        return self.record == other.record


class RefundReturn(_Cbor):
    """A Refund that returns t of the spent credits (include/act_mi355x.h, "partial refunds"): signed over X_A = g + K' + t h1."""
    CBOR_TYPE = "RefundReturn"

    def __init__(self, record: bytes):
        assert len(record) == 160
        self.record = bytes(record)   # A* | e | gamma | z | t

    def returned(self) -> bytes:
        return self.record[128:160]

    def __eq__(self, other):
        return self.record == other.record


class Reservation:
    """What reserve hands back for an accepted proof and the service keeps until it settles (include/act_mi355x.h "reserve and settle"):
    the 96 public bytes k^ | enc(K') | s^ and the ring index the proof matched.  It has no CBOR type: it never goes to a client.
    to_bytes / from_bytes: 97 bytes for the service's own storage, beside the job -- and, once known, the amount."""

    def __init__(self, record: bytes, key: int):
        assert len(record) == 96 and 0 <= key < 256
        self.record, self.key = bytes(record), int(key)

    def nullifier(self) -> bytes:
        return self.record[:32]

    def charge(self) -> int:
        return int.from_bytes(self.record[64:96], "little")

    def to_bytes(self) -> bytes:
        return self.record + bytes([self.key])

    @classmethod
    def from_bytes(cls, data: bytes) -> "Reservation":
        if len(data) != 97:
            raise ValueError("a stored reservation is 97 bytes")
        return cls(data[:96], data[96])

    def __eq__(self, other):
        return (self.record, self.key) == (other.record, other.key)


class NullifierDb:
    """The double-spend database the crate leaves to the caller (src/lib.rs:741-745; `NullifierDb` of src/tests.rs:29-50), as a
    hash set in the GPU's memory.  The tests' `if is_spent(k) { reject } else { record_spent(k) }` pair is one atomic call here,
    `spend(k)` (there is no read-only query: a look-up that does not record is how double spends slip through concurrent
    callers); whole batches go through PrivateKey.redeem_batch.  Keys are compared as scalars (k and k + l are one nullifier)."""

    def __init__(self, capacity: int = 1 << 20, device: int = 0):
        self.set = capi.NullifierSet(capacity, device)

    def spend(self, nullifier: bytes, epoch: int = 0) -> bool:
        """record `nullifier` (under `epoch`, the name of the issuer key its token was issued under; 0 = untagged); True if it was
        fresh, False if it had been spent before under any epoch (DoubleSpendError)"""
        return self.set.check_and_insert(bytes(nullifier), epochs=[epoch] if epoch else None)[0] == 0

    def spend_batch(self, nullifiers: Sequence[bytes], epoch: int = 0) -> List[bool]:
        """the same for a list, with the meaning of the loop in list order (a repeat inside the list is a double spend)"""
        if not nullifiers:
            return []
        return [b == 0 for b in self.set.check_and_insert(b"".join(bytes(k) for k in nullifiers), epochs=[epoch] if epoch else None)]

    def epoch_len(self, epoch: int) -> int:
        """how many nullifiers are recorded under `epoch`"""
        return self.set.epoch_len(epoch)

    def retire(self, epoch: int) -> int:
        """Remove every nullifier recorded under `epoch` and refuse the epoch from then on (also across save / restore); returns how
        many were removed.  ONLY once the epoch's key has been removed from every ring of every server that shares this database and
        will never be put back: from then on no proof under that key verifies, so its nullifiers are never consulted again.
        Retiring earlier re-enables double spends of that key's tokens."""
        return self.set.retire_epoch(epoch)

    def retired(self) -> List[int]:
        return self.set.retired_epochs()

    def reserve(self, capacity: int):
        """grow so that `capacity` nullifiers fit; the recorded ones are kept (rehashed on the GPU)"""
        self.set.reserve(capacity)

    def save(self, path: str) -> int:
        """snapshot of every recorded nullifier (nullifier_snapshot.py); returns how many were saved.  A point-in-time copy:
        what is recorded after it is lost in a crash unless the caller logs it ("restart and growth")."""
        return self.set.save(path)

    @classmethod
    def restore(cls, path: str, capacity: int = 1 << 20, device: int = 0) -> "NullifierDb":
        """a database holding the snapshot's nullifiers (the file is validated as a whole before anything is recorded)"""
        db = cls.__new__(cls)
        db.set = capi.NullifierSet.restore(path, capacity=capacity, device=device)
        return db

    def __len__(self):
        return len(self.set)
