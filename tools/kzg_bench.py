#!/usr/bin/env python3
"""Stand-alone timing of KZG blob proof batch verification (not bench.py).

For n = 1, 6 and 192 blobs: end-to-end verify_blob_kzg_proof_batch time
over device-resident inputs (host clock around calls that end in a stream
synchronise; min / median / max over --reps after --warmup) -> blobs/s, and
in a separate pass the per-kernel HIP-event times (with timing on, each
kernel is synchronised, so the stream overlap is off and the kernel times
do not sum to the end-to-end time). Prints one JSON line per n.

Inputs are three distinct seed-derived blobs cycled to n, with commitments
and proofs made under the insecure test setup of
tests/golden/kzg_fixtures.json (CPU oracle: test infrastructure). Needs a
GPU; there is no fallback. No CPU KZG implementation exists in this tree,
so no CPU ratio is computed.

--prove times the producing half instead, by the same method, for n = 1 and
6: blob_to_kzg_commitment and compute_blob_kzg_proof over device-resident
inputs and outputs, under the known-tau test setup ([L_i(tau)]G1 from the
CPU oracle). It first reports the one-time Lagrange load (validation +
table build), and beside each producing result it prints the kzg_mults
kernel time of a verification run of the same n in the same process: the
per-lane 255-step chain the MSM kernels (kzgp_msm + kzgp_finish) are
measured against.

--cells times the PeerDAS cell functions, by the same method: compute_cells
for n = 1 and 6 blobs (device-resident blobs and cells), and
verify_cell_proof_batch for n = 6 cells (one column of a 6-blob block), 128
(every column of one blob) and 768 (6 blobs x 128 columns) from host buffers
(the call has no device-resident form), under the known-tau test setup.
Inputs, the reference cells and the proofs [q_c(tau)]G1 are prepared once.

--recover times recover_all_cells, by the same method, for n = 1 and 6 blobs
over device-resident known cells and outputs, with two patterns of 64 known
cells: cells 0..63 missing, and 64 random cells missing. The output is
compared with the reference cells once, before timing. No setup is needed.

--cellproofs times compute_cells_and_kzg_proofs, by the same method, for
n = 1 and 6 blobs over device-resident blobs, cells and proofs, under the
known-tau test setup (g1_monomial[j] = [tau^j]G1 from the CPU oracle). It
first reports the one-time g1_monomial load (validation + table build) and
the table's device footprint. Beside each result it prints, from the same
process, compute_cells of the same n and the kzg_mults kernel time of a blob
verification of the same n: stage 2 (kzgc_proof_dft) is a serial chain of
such multiplications and is stated as a multiple of it. The first blob's 128
proofs are compared with [q_c(tau)]G1 from the oracle once, before timing."""
import argparse
import ctypes
import hashlib
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))


def make_triples(g2_seed):
    import gen_bls_fixtures as G
    import kzg_ref as K

    subprocess.run(["make", "-s", "-C", str(REPO / "oracle")], check=True)
    oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))
    tau = int.from_bytes(hashlib.sha256(g2_seed.encode()).digest(), "big") % K.R

    def g1_mul(k):
        k %= K.R
        if k == 0:
            return K.G1_POINT_AT_INFINITY
        out = ctypes.create_string_buffer(96)
        assert oracle.m3x_oracle_bls_g1_mul(
            G.g1_uncompressed(G.G1G), k.to_bytes(32, "big"), out) == 0
        raw = out.raw
        return G.g1_compress(
            (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")))

    out = []
    for i in range(3):
        blob = K.blob_from_seed(b"kzg-bench-%d" % i)
        poly = K.blob_to_polynomial(blob)
        p_tau = K.poly_eval_at_secret(poly, tau)
        c = g1_mul(p_tau)
        z = K.compute_challenge(blob, c)
        y = K.evaluate_polynomial_in_evaluation_form(poly, z)
        q_tau = (p_tau - y) * pow((tau - z) % K.R, -1, K.R) % K.R
        out.append((blob, c, g1_mul(q_tau)))
    return out


def make_lagrange(g2_seed):
    """[L_k(tau)]G1 compressed, in trusted-setup file order."""
    import gen_bls_fixtures as G
    import kzg_prover_ref as P
    import kzg_ref as K

    oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))
    tau = int.from_bytes(hashlib.sha256(g2_seed.encode()).digest(), "big") % K.R
    gen = G.g1_uncompressed(G.G1G)
    out = []
    for s in P.lagrange_scalars_file_order(tau):
        buf = ctypes.create_string_buffer(96)
        assert oracle.m3x_oracle_bls_g1_mul(gen, s.to_bytes(32, "big"), buf) == 0
        raw = buf.raw
        out.append(G.g1_compress(
            (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big"))))
    return b"".join(out)


def timed(ctx, run, reps, warmup):
    """(host-clock times of `reps` calls, per-kernel ms from a separate
    pass with event timing on) - the verify mode's method."""
    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    ctx.timing_enable(True)
    kreps = max(3, reps // 4)
    for _ in range(kreps):
        run()
    kernels = {
        name: round(ms / kreps, 4)
        for name, (ms, launches) in ctx.kernel_times().items()
        if name.startswith("kzg") and launches
    }
    ctx.timing_enable(False)
    return times, kernels


def prove_main(args, fx, triples, ctx, kzg):
    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])
    lagrange = make_lagrange(fx["test_setup"]["tau_seed"])
    t0 = time.perf_counter()
    k = kzg.Kzg(g2_tau, lagrange, ctx=ctx)
    load_ms = (time.perf_counter() - t0) * 1e3
    table_bytes = 64 * 4096 * 8 * 96
    print(json.dumps({
        "setup_load_ms": round(load_ms, 2),
        "table_bytes": table_bytes,
        "table_MB": round(table_bytes / 1e6, 1),
    }), flush=True)
    for n in [int(s) for s in args.sizes.split(",")]:
        ts = [triples[i % 3] for i in range(n)]
        blobs_d = ctx.upload(b"".join(t[0] for t in ts))
        cs_d = ctx.upload(b"".join(t[1] for t in ts))
        ps_d = ctx.upload(b"".join(t[2] for t in ts))
        out_d = ctx.alloc(48 * n)
        want_c = b"".join(t[1] for t in ts)
        want_p = b"".join(t[2] for t in ts)

        def check(want):
            got = ctypes.create_string_buffer(48 * n)
            assert ctx._lib.m3x_d2h(ctx.handle, got, out_d, 48 * n) == 0
            assert got.raw == want, "producer output differs from the oracle's"

        def verify():
            assert k.verify_blob_kzg_proof_batch_dev(blobs_d, cs_d, ps_d, n) is True

        _, vk = timed(ctx, verify, max(4, args.reps // 4), 1)
        for what, run, want in (
            ("blob_to_kzg_commitment",
             lambda: k.blob_to_kzg_commitment_batch_dev(blobs_d, n, out_d), want_c),
            ("compute_blob_kzg_proof",
             lambda: k.compute_blob_kzg_proof_batch_dev(blobs_d, cs_d, n, out_d), want_p),
        ):
            times, kernels = timed(ctx, run, args.reps, args.warmup)
            check(want)
            med = statistics.median(times)
            msm = kernels.get("kzgp_msm", 0.0) + kernels.get("kzgp_finish", 0.0)
            print(json.dumps({
                "call": what,
                "n_blobs": n,
                "reps": args.reps,
                "ms_min": round(min(times) * 1e3, 4),
                "ms_median": round(med * 1e3, 4),
                "ms_max": round(max(times) * 1e3, 4),
                "blobs_per_s_median": round(n / med, 2),
                "kernel_ms_serialised": kernels,
                "msm_kernels_ms": round(msm, 4),
                "verify_kzg_mults_ms": vk.get("kzg_mults"),
            }), flush=True)
        for p in (blobs_d, cs_d, ps_d, out_d):
            ctx.free(p)
    k.close()


def cells_main(args, fx, ctx, kzg):
    import gen_bls_fixtures as G
    import kzg_cells_ref as C
    import kzg_ref as K

    cfx = json.loads(
        (REPO / "tests" / "golden" / "kzg_cell_fixtures.json").read_text())
    subprocess.run(["make", "-s", "-C", str(REPO / "oracle")], check=True)
    oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))
    seed = fx["test_setup"]["tau_seed"]
    tau = int.from_bytes(hashlib.sha256(seed.encode()).digest(), "big") % K.R
    gen = G.g1_uncompressed(G.G1G)

    def g1_mul(k):
        k %= K.R
        if k == 0:
            return K.G1_POINT_AT_INFINITY
        out = ctypes.create_string_buffer(96)
        assert oracle.m3x_oracle_bls_g1_mul(gen, k.to_bytes(32, "big"), out) == 0
        raw = out.raw
        return G.g1_compress(
            (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")))

    mono = b"".join(g1_mul(pow(tau, j, K.R)) for j in range(64))
    k = kzg.Kzg.with_cell_setup(
        bytes.fromhex(fx["test_setup"]["g2_tau"]),
        (mono, bytes.fromhex(cfx["test_setup"]["g2_tau64"])), ctx=ctx)
    # six distinct blobs: reference cells, commitment, all 128 proofs
    blobs, ref_cells, commitments, proofs = [], [], [], []
    for i in range(6):
        blob = K.blob_from_seed(b"kzg-cells-bench-%d" % i)
        coef = C.blob_coefficients(blob)
        blobs.append(blob)
        ref_cells.append(
            [C.cell_to_bytes(c) for c in C.cells_from_coefficients(coef)])
        commitments.append(g1_mul(C.poly_eval(coef, tau)))
        proofs.append([
            g1_mul(C.poly_eval(C.cell_quotient(coef, c), tau))
            for c in range(128)
        ])

    def report(call, n, unit, times, kernels):
        med = statistics.median(times)
        print(json.dumps({
            "call": call,
            "n_" + unit: n,
            "reps": args.reps,
            "ms_min": round(min(times) * 1e3, 4),
            "ms_median": round(med * 1e3, 4),
            "ms_max": round(max(times) * 1e3, 4),
            unit + "_per_s_median": round(n / med, 2),
            "kernel_ms_serialised": kernels,
        }), flush=True)

    for n in (1, 6):
        blobs_d = ctx.upload(b"".join(blobs[:n]))
        out_d = ctx.alloc(n * 128 * 2048)
        run = lambda: k.compute_cells_batch_dev(blobs_d, n, out_d)  # noqa: E731
        times, kernels = timed(ctx, run, args.reps, args.warmup)
        got = ctypes.create_string_buffer(n * 128 * 2048)
        assert ctx._lib.m3x_d2h(ctx.handle, got, out_d, len(got)) == 0
        assert got.raw == b"".join(b"".join(c) for c in ref_cells[:n]), \
            "cells differ from the reference"
        report("compute_cells", n, "blobs", times, kernels)
        ctx.free(blobs_d)
        ctx.free(out_d)

    shapes = {
        6: [(row, 70) for row in range(6)],
        128: [(0, col) for col in range(128)],
        768: [(row, col) for col in range(128) for row in range(6)],
    }
    for n, coords in shapes.items():
        cells = [ref_cells[r][c] for r, c in coords]
        prs = [proofs[r][c] for r, c in coords]
        m = max(r for r, _ in coords) + 1
        cs = commitments[:m]

        def run():
            assert k.verify_cell_proof_batch(cells, prs, coords, cs) is True

        times, kernels = timed(ctx, run, args.reps, args.warmup)
        report("verify_cell_proof_batch", n, "cells", times, kernels)
    k.close()


def recover_main(args, ctx, kzg):
    import random

    import kzg_cells_ref as C
    import kzg_ref as K

    k = kzg.Kzg(bytes.fromhex(json.loads(
        (REPO / "tests" / "golden" / "kzg_fixtures.json").read_text()
    )["test_setup"]["g2_tau"]), ctx=ctx)
    ref_cells = []
    for i in range(6):
        coef = C.blob_coefficients(K.blob_from_seed(b"kzg-recover-bench-%d" % i))
        ref_cells.append(
            [C.cell_to_bytes(c) for c in C.cells_from_coefficients(coef)])
    patterns = {
        "first_half_missing": list(range(64, 128)),
        "random_64_missing": sorted(random.Random(1).sample(range(128), 64)),
    }
    for name, ids in patterns.items():
        for n in (1, 6):
            cells_d = ctx.upload(b"".join(
                b"".join(ref_cells[b][c] for c in ids) for b in range(n)))
            out_d = ctx.alloc(n * 128 * 2048)
            run = lambda: k.recover_all_cells_batch_dev(ids, cells_d, n, out_d)  # noqa: E731
            run()
            got = ctypes.create_string_buffer(n * 128 * 2048)
            assert ctx._lib.m3x_d2h(ctx.handle, got, out_d, len(got)) == 0
            assert got.raw == b"".join(b"".join(c) for c in ref_cells[:n]), \
                "recovered cells differ from the reference"
            times, kernels = timed(ctx, run, args.reps, args.warmup)
            med = statistics.median(times)
            print(json.dumps({
                "call": "recover_all_cells",
                "pattern": name,
                "n_blobs": n,
                "known_cells": len(ids),
                "reps": args.reps,
                "ms_min": round(min(times) * 1e3, 4),
                "ms_median": round(med * 1e3, 4),
                "ms_max": round(max(times) * 1e3, 4),
                "blobs_per_s_median": round(n / med, 2),
                "kernel_ms_serialised": kernels,
            }), flush=True)
            ctx.free(cells_d)
            ctx.free(out_d)
    k.close()


def cellproofs_main(args, fx, triples, ctx, kzg):
    import gen_bls_fixtures as G
    import kzg_cells_ref as C
    import kzg_ref as K

    oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))
    seed = fx["test_setup"]["tau_seed"]
    tau = int.from_bytes(hashlib.sha256(seed.encode()).digest(), "big") % K.R
    gen = G.g1_uncompressed(G.G1G)

    def g1_mul(k):
        k %= K.R
        if k == 0:
            return K.G1_POINT_AT_INFINITY
        out = ctypes.create_string_buffer(96)
        assert oracle.m3x_oracle_bls_g1_mul(gen, k.to_bytes(32, "big"), out) == 0
        raw = out.raw
        return G.g1_compress(
            (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")))

    mono, t = [], 1
    for _ in range(K.FIELD_ELEMENTS_PER_BLOB):
        mono.append(g1_mul(t))
        t = t * tau % K.R
    mono = b"".join(mono)
    k = kzg.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]), ctx=ctx)
    t0 = time.perf_counter()
    k.load_g1_monomial(mono)
    load_ms = (time.perf_counter() - t0) * 1e3
    table_bytes = 64 * 4096 * 8 * 96
    print(json.dumps({
        "setup_load_ms": round(load_ms, 2),
        "table_bytes": table_bytes,
        "table_MB": round(table_bytes / 1e6, 1),
    }), flush=True)
    coef = C.blob_coefficients(triples[0][0])
    want0 = b"".join(
        g1_mul(C.poly_eval(C.cell_quotient(coef, c), tau)) for c in range(128))
    for n in (1, 6):
        ts = [triples[i % 3] for i in range(n)]
        blobs_d = ctx.upload(b"".join(t[0] for t in ts))
        cs_d = ctx.upload(b"".join(t[1] for t in ts))
        ps_d = ctx.upload(b"".join(t[2] for t in ts))
        cells_d = ctx.alloc(n * 128 * 2048)
        proofs_d = ctx.alloc(n * 128 * 48)

        def verify():
            assert k.verify_blob_kzg_proof_batch_dev(blobs_d, cs_d, ps_d, n) is True

        _, vk = timed(ctx, verify, max(4, args.reps // 4), 1)
        ctimes, _ = timed(
            ctx, lambda: k.compute_cells_batch_dev(blobs_d, n, cells_d),
            args.reps, args.warmup)
        run = lambda: k.compute_cells_and_kzg_proofs_batch_dev(  # noqa: E731
            blobs_d, n, cells_d, proofs_d)
        run()
        got = ctypes.create_string_buffer(n * 128 * 48)
        assert ctx._lib.m3x_d2h(ctx.handle, got, proofs_d, len(got)) == 0
        assert got.raw[: 128 * 48] == want0, "proofs differ from the oracle's"
        times, kernels = timed(ctx, run, args.reps, args.warmup)
        med = statistics.median(times)
        mults = vk.get("kzg_mults")
        dft = kernels.get("kzgc_proof_dft")
        print(json.dumps({
            "call": "compute_cells_and_kzg_proofs",
            "n_blobs": n,
            "reps": args.reps,
            "ms_min": round(min(times) * 1e3, 4),
            "ms_median": round(med * 1e3, 4),
            "ms_max": round(max(times) * 1e3, 4),
            "blobs_per_s_median": round(n / med, 2),
            "kernel_ms_serialised": kernels,
            "stage1_ms": kernels.get("kzgc_toeplitz"),
            "stage2_ms": dft,
            "verify_kzg_mults_ms": mults,
            "stage2_over_kzg_mults": round(dft / mults, 2) if dft and mults else None,
            "compute_cells_ms_median": round(statistics.median(ctimes) * 1e3, 4),
        }), flush=True)
        for p in (blobs_d, cs_d, ps_d, cells_d, proofs_d):
            ctx.free(p)
    k.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prove", action="store_true",
                    help="time commitment and blob-proof computation instead")
    ap.add_argument("--cells", action="store_true",
                    help="time compute_cells and cell-proof batch verification")
    ap.add_argument("--recover", action="store_true",
                    help="time recover_all_cells")
    ap.add_argument("--cellproofs", action="store_true",
                    help="time compute_cells_and_kzg_proofs")
    args = ap.parse_args()
    if args.sizes is None:
        args.sizes = "1,6" if args.prove else "1,6,192"

    from lighthouse_amd import _native, kzg

    fx = json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())
    if args.recover:
        return recover_main(args, _native.default_ctx(), kzg)
    if args.cells:
        return cells_main(args, fx, _native.default_ctx(), kzg)
    triples = make_triples(fx["test_setup"]["tau_seed"])
    ctx = _native.default_ctx()
    if args.prove:
        return prove_main(args, fx, triples, ctx, kzg)
    if args.cellproofs:
        return cellproofs_main(args, fx, triples, ctx, kzg)
    k = kzg.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]), ctx=ctx)
    for n in [int(s) for s in args.sizes.split(",")]:
        ts = [triples[i % 3] for i in range(n)]
        blobs_d = ctx.upload(b"".join(t[0] for t in ts))
        cs_d = ctx.upload(b"".join(t[1] for t in ts))
        ps_d = ctx.upload(b"".join(t[2] for t in ts))
        run = lambda: k.verify_blob_kzg_proof_batch_dev(blobs_d, cs_d, ps_d, n)  # noqa: E731
        for _ in range(args.warmup):
            assert run() is True
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ok = run()
            times.append(time.perf_counter() - t0)
            assert ok is True
        ctx.timing_enable(True)
        kreps = max(3, args.reps // 4)
        for _ in range(kreps):
            assert run() is True
        kernels = {
            name: round(ms / kreps, 4)
            for name, (ms, launches) in ctx.kernel_times().items()
            if name.startswith("kzg_") and launches
        }
        ctx.timing_enable(False)
        for p in (blobs_d, cs_d, ps_d):
            ctx.free(p)
        med = statistics.median(times)
        print(json.dumps({
            "n_blobs": n,
            "reps": args.reps,
            "ms_min": round(min(times) * 1e3, 4),
            "ms_median": round(med * 1e3, 4),
            "ms_max": round(max(times) * 1e3, 4),
            "blobs_per_s_median": round(n / med, 2),
            "kernel_ms_serialised": kernels,
        }), flush=True)
    k.close()


if __name__ == "__main__":
    main()
