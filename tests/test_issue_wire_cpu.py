"""Issuance on wire bytes, without a GPU: the six entry points are declared in the header with the agreed prototypes, bound by the
ctypes binding, exported by the built library, and declared by the Rust binding (its node forms, with the header's arity), which also
offers the batch, blob and one-message forms."""
import os
import re

from conftest import ROOT
from test_abi_prototypes import parse_header, parse_rust_externs

NAMES = ("act_issue_check_cbor_batch", "act_issue_sign_cbor_batch", "act_issue_cbor_batch",
         "act_node_issue_check_cbor_batch", "act_node_issue_sign_cbor_batch", "act_node_issue_cbor_batch")
PROTOS = {
    "act_issue_check_cbor_batch": ["act_ctx *ctx", "size_t n", "int mem", "const uint8_t *cbor", "const uint64_t *offsets", "uint8_t *status",
                                   "uint8_t *out_req"],
    "act_issue_sign_cbor_batch": ["act_ctx *ctx", "size_t n", "int mem", "const uint8_t sk[64]", "const uint8_t *req", "const uint8_t *c",
                                  "const uint8_t *status_in", "const uint8_t *rng", "int rng_mode", "uint8_t *out_resp_cbor", "uint8_t *status"],
    "act_issue_cbor_batch": ["act_ctx *ctx", "size_t n", "int mem", "const uint8_t sk[64]", "const uint8_t *cbor", "const uint64_t *offsets",
                             "const uint8_t *c", "const uint8_t *rng", "int rng_mode", "uint8_t *out_resp_cbor", "uint8_t *status"],
}


def _norm(p):
    return re.sub(r"\s+", " ", p).strip()


def test_header_declares_the_six_prototypes():
    protos = parse_header()
    for name in NAMES:
        assert name in protos, name
        assert protos[name][0] == "int", name
    for name, want in PROTOS.items():
        assert [_norm(p) for p in protos[name][1]] == want, name
        node = protos[name.replace("act_", "act_node_", 1)][1]
        # the node forms: the node handle instead of the context, no `mem`, the rest as the single-GPU form
        assert [_norm(p) for p in node] == ["act_node *node"] + want[1:2] + want[3:], name


def test_binding_and_library_carry_them():
    from act_amd import capi
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("issue_cbor", "issue_check_cbor", "issue_sign_cbor", "issue_cbor_ptr"):
        assert callable(getattr(capi.Engine, method, None)), method
    assert callable(getattr(capi.Node, "issue_cbor", None))
    from act_amd.api import PrivateKey
    assert callable(getattr(PrivateKey, "issue_cbor_batch", None))


def test_rust_extern_block_declares_the_node_forms():
    protos = parse_header()
    fns = parse_rust_externs()
    for name in NAMES[3:]:
        assert name in fns, name
        assert len(fns[name][0]) == len(protos[name][1]), name


def test_rust_binding_offers_issue_cbor():
    src = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    assert re.search(r"pub fn issue_cbor_batch\s*\(&self, params: &Params, msgs: &\[&\[u8\]\], amounts: &\[Scalar\]", src)
    assert re.search(r"pub fn issue_cbor_blob\s*\(&self, params: &Params, blob: &\[u8\], offsets: &\[u64\], amounts: &\[Scalar\]", src)
    predrawn = src[src.index("pub mod predrawn"):]
    assert re.search(r"pub fn issue_cbor\s*\(sk: &PrivateKey, params: &Params, msg: &\[u8\], c: Scalar, nonces: &\[u8; 128\]\)", predrawn)
    # above the kept single-call signatures (tests/test_rust_sources.py reads those from their marker on)
    kept = src.index("impl PreIssuance {\n    pub fn request(&self")
    assert src.index("pub fn issue_cbor_batch") < kept and src.index("pub fn issue_cbor_blob") < kept
    assert "const ISSUANCE_RESPONSE_CBOR_BYTES: usize = 176;" in src
