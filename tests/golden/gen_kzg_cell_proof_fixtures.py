#!/usr/bin/env python3
"""Generator for the PeerDAS cell-proof fixture.

  gen_kzg_cell_proof_fixtures.py <trusted_setup.json>
      writes tests/golden/ceremony_g1_monomial.bin: the 4096 compressed
      points of the ceremony file's g1_monomial list, 48 bytes each, in the
      file's own order (196608 bytes): entry j is [tau^j]G1.

<trusted_setup.json> is the ceremony file the reference ships at
common/eth2_network_config/built_in_network_configs/trusted_setup.json; it
is read at generation time only. The first 65 points are the ones
gen_kzg_cell_fixtures.py recorded in kzg_cell_fixtures.json, which
tests/test_kzg_cell_proofs_ref.py checks."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
N = 4096


def main(setup_path):
    import json

    ts = json.loads(Path(setup_path).read_text())
    pts = [bytes.fromhex(s[2:] if s.startswith("0x") else s)
           for s in ts["g1_monomial"]]
    assert len(pts) == N and all(len(p) == 48 for p in pts)
    # compressed, not infinity
    assert all(p[0] & 0x80 and not p[0] & 0x40 for p in pts)
    (HERE / "ceremony_g1_monomial.bin").write_bytes(b"".join(pts))
    print("wrote ceremony_g1_monomial.bin")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
