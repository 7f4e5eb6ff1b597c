#!/usr/bin/env python3
"""Stand-alone timing of the gossip batch-false fallback (not bench.py):
n per-set verdicts by (a) n sequential m3x_bls_verify_sets(n = 1, r = 1)
calls on one context, the method before m3x_bls_verify_each existed, and
(b) one m3x_bls_verify_each call.

For n = 1, 8, 64 and 192 valid k = 1 sets with one tampered message: host
clock around calls that end in a stream synchronise, (a) and (b)
alternating within each repetition, median over --reps after --warmup; then,
in a separate pass with event timing on, the per-set pairing kernel's time
(timing slot 20) for (b). Both methods' verdicts are checked (False at the
tampered index only) before anything is timed.

Every n runs in a child process of its own under a time limit, and the
script ends at the first child that fails or runs out of time. Writes the
rows to --out as JSON and prints them. Needs a GPU; there is no fallback.
The CPU oracle (test infrastructure) only makes the keys and signatures."""
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

K_BLS_EACH = 20
STEP_LIMIT_S = 240


def workload(n):
    subprocess.run(["make", "-s", "-C", str(REPO / "oracle")], check=True)
    oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))
    sks = ctypes.create_string_buffer(32 * n)
    pks = ctypes.create_string_buffer(96 * n)
    oracle.m3x_oracle_bls_keypool(ctypes.c_uint64(n), sks, pks)
    msgs = b"".join(hashlib.sha256(b"each-bench-%d" % i).digest() for i in range(n))
    sigs = ctypes.create_string_buffer(96 * n)
    assert oracle.m3x_oracle_bls_sign_batch(ctypes.c_uint64(n), sks.raw, msgs, sigs) == 0
    bad = n // 2
    msgs = bytearray(msgs)
    msgs[32 * bad : 32 * (bad + 1)] = hashlib.sha256(b"tampered").digest()
    return bytes(msgs), sigs.raw, pks.raw, bad


def one(n, reps, warmup):
    from lighthouse_amd import _native

    msgs, sigs, pks, bad = workload(n)
    ctx = _native.default_ctx()
    lib = ctx._lib
    one_off = (ctypes.c_uint32 * 2)(0, 1)
    one_rand = (ctypes.c_uint64 * 1)(1)
    offs = (ctypes.c_uint32 * (n + 1))(*range(n + 1))
    verdicts = (ctypes.c_int32 * n)()

    def loop():
        return [
            lib.m3x_bls_verify_sets(
                ctx.handle, msgs[32 * i : 32 * (i + 1)], sigs[96 * i : 96 * (i + 1)],
                pks[96 * i : 96 * (i + 1)], one_off, one_rand, 1)
            for i in range(n)
        ]

    def each():
        assert lib.m3x_bls_verify_each(ctx.handle, msgs, sigs, pks, offs, n, verdicts) == 0
        return list(verdicts)

    want = [0 if i == bad else 1 for i in range(n)]
    for _ in range(warmup):
        assert loop() == want
        assert each() == want
    t_loop, t_each = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        loop()
        t1 = time.perf_counter()
        each()
        t2 = time.perf_counter()
        t_loop.append(t1 - t0)
        t_each.append(t2 - t1)
    ctx.timing_enable(True)
    for _ in range(reps):
        each()
    ms, cnt = ctypes.c_double(), ctypes.c_uint64()
    assert lib.m3x_kernel_ms(ctx.handle, K_BLS_EACH, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert cnt.value == reps
    ctx.timing_enable(False)
    med_loop = statistics.median(t_loop) * 1e3
    med_each = statistics.median(t_each) * 1e3
    return {
        "n_sets": n,
        "reps": reps,
        "loop_ms_median": round(med_loop, 4),
        "loop_ms_min": round(min(t_loop) * 1e3, 4),
        "loop_ms_max": round(max(t_loop) * 1e3, 4),
        "each_ms_median": round(med_each, 4),
        "each_ms_min": round(min(t_each) * 1e3, 4),
        "each_ms_max": round(max(t_each) * 1e3, 4),
        "each_pairing_kernel_ms": round(ms.value / reps, 4),
        "loop_over_each": round(med_loop / med_each, 2),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="1,8,64,192")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(REPO / "profiles" / "bls_each_bench.json"))
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        print(json.dumps(one(args.one, args.reps, args.warmup)), flush=True)
        return
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        # a fresh child per size: its own time limit, and a failure ends the
        # script before anything else is started on the GPU
        p = subprocess.run(
            [sys.executable, str(Path(__file__).resolve()), "--one", str(n), "--reps", str(args.reps),
             "--warmup", str(args.warmup)],
            capture_output=True, text=True, timeout=STEP_LIMIT_S,
        )
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"n = {n}: exit status {p.returncode}")
        row = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    Path(args.out).write_text(json.dumps(
        {"method": "host clock, median; (a) loop of n single-set batch calls, "
                   "(b) one per-set call; kernel time from HIP events",
         "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
