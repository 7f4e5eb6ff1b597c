"""Host side of bls.verify_signature_sets_each (no GPU): the per-set host
rules short-circuit before the native library is touched, and the header
declares the two per-set entries."""
import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_each_empty_list():
    from lighthouse_amd import bls

    assert bls.verify_signature_sets_each([]) == []


def test_each_host_rules_do_not_touch_native(monkeypatch):
    """Sets with an empty signature or no keys are False on the host; a list
    of nothing else never loads the library or creates a context."""
    from lighthouse_amd import _native, bls

    def boom(*a, **kw):
        raise AssertionError("native library touched")

    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "default_ctx", boom)
    pk = bls.PublicKey.from_uncompressed(bytes(96))
    sig = bls.Signature.from_compressed(bytes([0xC0]) + bytes(95))
    sets = [
        bls.SignatureSet(bls.Signature.empty(), [pk], bytes(32)),
        bls.SignatureSet(sig, [], bytes(32)),
        bls.SignatureSet(bls.Signature.empty(), [], bytes(32)),
    ]
    assert bls.verify_signature_sets_each(sets) == [False, False, False]


def test_header_declares_each_entries():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in ("m3x_bls_verify_each", "m3x_bls_verify_each_dev"):
        assert sym in declared, sym
