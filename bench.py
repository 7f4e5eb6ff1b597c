#!/usr/bin/env python3
"""bench.py — BASELINE.json workloads on MI355X.

A "step" is one pass of the hot path over one batch of synthetic input:
  - primary (BASELINE configs[1], the quoted single-GPU workload): batch
    BLS verification of 65,536 attestation signature sets (75% k=1
    unaggregated + 25% aggregates with k=512 — committee size at 2^20
    active validators), inputs resident in HBM when the timed region
    starts; each step runs the full blst.rs:37-119 check incl. the final
    exponentiation and verdict readback.
  - in the same step, the SHA256 path (configs[2]): full rebuild of the
    1,048,576-validator registry hash_tree_root (9,437,204 two-to-one node
    hashes), reported as extra_metrics.
Multi-GPU (--gpus N via torch.distributed.run): weak scaling — each rank
verifies its own 64k-set batch (verdicts AND-combined with one 4-byte
all_reduce(MIN) over RCCL) and computes its aligned shard of ONE shared
1M-validator registry (subtree roots gathered to rank 0 which finishes the
zero cap + mix_in_length).

Workload generation (untimed) uses the CPU oracle as the synthetic-data
SIGNER (the r-side of each set must verify, so sets are signed with
aggregate secrets derived from the interop keypool); the timed region runs
only the product HIP path.

A plain run sets up, warms up, times --steps steps and prints the result
line. --dump-outputs DIR also saves what the last timed step returned
(bls_verdict.npy, state_root.npy). Everything else is behind --full: the
oracle correctness gate before timing, the per-kernel timing pass and
roofline, the C4 / C5 / incremental-registry / shuffle extras, split
BLS/merkle timing, and the cpu_baseline leg, which times the same oracle
as the reference-equivalent CPU port (kind "port", OpenMP, cores stated).
Without --full those fields of the result line are null.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

# BLS12-381 group order (for synthetic aggregate secret keys)
ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# analytic roofline constants (derivation in DESIGN.md §Roofline):
# Fp multiplies per set in the dominant kernel (k_bls_miller): 63 doubling
# steps x (f^2 108 + sparse line mult 54 + line coeffs 36 + point dbl 21)
# + 5 addition steps x ~110  ~= 14.3k; int32 ALU ops per 6x64-limb CIOS
# Montgomery multiply ~= 550 (144 32-bit mults + carries/adds).
FP_MUL_PER_MILLER = 14300
INT_OPS_PER_FP_MUL = 550
PEAK_INT32_OPS = 256 * 4 * 32 * 2.4e9  # CUs x SIMDs x lanes x clock
SHA_OPS_PER_NODE = 1900  # two compressions, pad block constant-folded
REGISTRY_NODE_HASHES = 8 * (1 << 20) + ((1 << 20) - 1) + 20 + 1  # 9,437,204

POOL = 4096
N_SETS = 65536
N_AGG = N_SETS // 4
K_AGG = 512
N_VALIDATORS = 1 << 20


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def build_bls_workload(oracle, seed=0xC0FFEE):
    """65,536 sets: 49,152 k=1 + 16,384 k=512 aggregates over a 4096-key
    interop pool; every set carries a real signature (signed with the sum
    of the member secret keys), so the batch verdict is True."""
    t0 = time.time()
    sks = ctypes.create_string_buffer(32 * POOL)
    pks = ctypes.create_string_buffer(96 * POOL)
    oracle.m3x_oracle_bls_keypool(ctypes.c_uint64(POOL), sks, pks)
    sk_ints = [
        int.from_bytes(sks.raw[32 * i : 32 * (i + 1)], "big") for i in range(POOL)
    ]
    msgs = bytearray()
    sign_sks = bytearray()
    pk_bytes = bytearray()
    offsets = [0]
    costs = []
    for i in range(N_SETS):
        msg = hashlib.sha256(b"c2msg%d" % i).digest()
        msgs += msg
        if i < N_SETS - N_AGG:  # k = 1
            j = i % POOL
            sign_sks += sk_ints[j].to_bytes(32, "big")
            pk_bytes += pks.raw[96 * j : 96 * (j + 1)]
            offsets.append(offsets[-1] + 1)
            costs.append(1)
        else:  # aggregate, k = 512, contiguous committee window
            off = (i * 37) % (POOL - K_AGG)
            agg = 0
            for j in range(off, off + K_AGG):
                agg = (agg + sk_ints[j]) % ORDER
            sign_sks += agg.to_bytes(32, "big")
            pk_bytes += pks.raw[96 * off : 96 * (off + K_AGG)]
            offsets.append(offsets[-1] + K_AGG)
            costs.append(K_AGG)
    sigs = ctypes.create_string_buffer(96 * N_SETS)
    rc = oracle.m3x_oracle_bls_sign_batch(
        ctypes.c_uint64(N_SETS), bytes(sign_sks), bytes(msgs), sigs
    )
    assert rc == 0
    rands = [((i * 0x9E3779B97F4A7C15 + seed) | 1) & 0xFFFFFFFFFFFFFFFF for i in range(N_SETS)]
    log(f"bls workload built in {time.time()-t0:.1f}s")
    return {
        "msgs": bytes(msgs),
        "sigs": sigs.raw,
        "pks": bytes(pk_bytes),
        "offsets": offsets,
        "rands": rands,
        "costs": costs,
    }


def upload_bls(ctx, w):
    import numpy as np

    dev = {}
    dev["msgs"] = ctx.upload(w["msgs"])
    dev["sigs"] = ctx.upload(w["sigs"])
    dev["pks"] = ctx.upload(w["pks"])
    dev["offsets"] = ctx.upload(np.asarray(w["offsets"], dtype=np.uint32).tobytes())
    dev["rands"] = ctx.upload(np.asarray(w["rands"], dtype=np.uint64).tobytes())
    return dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--backend", default=os.environ.get("M3X_BENCH_BACKEND", "nccl"),
                    help="torch.distributed backend (gloo = CPU dry-run of the collective path)")
    ap.add_argument("--dry-run", action="store_true",
                    help="stub the GPU compute but run the EXACT multi-rank "
                         "code path (collectives, timing, report) on CPU — "
                         "CI proof of the world-N bench path (VERDICT r1 #5)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: "
                         "the oracle correctness gate before timing, "
                         "per-kernel timing + roofline, the C4/C5/incremental/"
                         "shuffle extras, split timing and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned to its "
                         "caller as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    DRY = args.dry_run
    FULL = args.full

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(args.gpus, world)

    import torch

    comm_dev = "cuda" if args.backend == "nccl" else "cpu"

    def sync():
        if comm_dev == "cuda":
            torch.cuda.synchronize()

    dist = None
    if world > 1:
        import torch.distributed as tdist

        dist = tdist
        if comm_dev == "cuda":
            torch.cuda.set_device(local_rank)
        tdist.init_process_group(args.backend)

    os.environ.setdefault("M3X_DEVICE", str(local_rank))
    # Effective CPU budget for the oracle baseline legs: the GPU box
    # reports 256 logical CPUs but the process is typically quota-limited
    # (cgroup cpu.max) to far fewer; oversubscribed OpenMP then THRASHES
    # (measured: 46M node-hashes/s at 256 threads vs 404M at 32 on the
    # same box). Use the real budget and pin threads.
    eff_cores = len(os.sched_getaffinity(0))
    try:
        quota = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota[0] != "max":
            eff_cores = min(eff_cores, max(1, int(quota[0]) // int(quota[1])))
    except (OSError, ValueError, IndexError):
        pass
    os.environ.setdefault("OMP_NUM_THREADS", str(eff_cores))
    os.environ.setdefault("OMP_PROC_BIND", "spread")
    os.environ.setdefault("OMP_PLACES", "cores")
    log(f"cpu baseline budget: {eff_cores} effective cores "
        f"(os.cpu_count={os.cpu_count()})")
    start, per = rank * (N_VALIDATORS // world), N_VALIDATORS // world
    sub_depth = per.bit_length() - 1
    if DRY:
        # stubbed compute, REAL collective/timing/report path
        ctx = oracle = lib = None
        ssz_full = None
        out32 = None
        devmap = None
    else:
        from lighthouse_amd import _native, beacon_state as bs

        ctx = _native.Ctx(local_rank)
        oracle = ctypes.CDLL(str(REPO / "oracle" / "liboracle.so"))

        # ---------------- workload prep (untimed) ----------------
        bls_w = build_bls_workload(oracle, seed=0xC0FFEE + rank)
        bls_dev = upload_bls(ctx, bls_w)

        t0 = time.time()
        st = bs.generate(N_VALIDATORS)  # same seed on all ranks
        ssz_full = st["validators_ssz"]
        log(f"state generated in {time.time()-t0:.1f}s")
        # registry shard for this rank; rank 0 holds the other big fields
        ssz_shard = ssz_full[121 * start : 121 * (start + per)]
        ssz_dev = ctx.upload(ssz_shard + b"\x00" * 4)
        devmap = bs.upload_fields(st, ctx) if rank == 0 else None

        lib = ctx._lib
        out32 = ctypes.create_string_buffer(32)

    def bls_step():
        if DRY:
            v = 1
        else:
            v = lib.m3x_bls_verify_sets_dev(
                ctx.handle,
                bls_dev["msgs"],
                bls_dev["sigs"],
                bls_dev["pks"],
                bls_dev["offsets"],
                bls_dev["rands"],
                N_SETS,
            )
        if world > 1:
            t = torch.tensor([v], dtype=torch.int32, device=comm_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            v = int(t.item())
        return v

    def _hash2(a, b):
        return hashlib.sha256(a + b).digest()

    def registry_root_step():
        if DRY:
            node = _hash2(b"dry-shard", rank.to_bytes(4, "little"))
        else:
            rc = lib.m3x_validator_subtree_root_dev(
                ctx.handle, ssz_dev, per, sub_depth, out32
            )
            assert rc == 0, rc
            node = out32.raw
        if world > 1:
            # NCCL has no gather primitive: use all_gather (8x32B, latency-
            # bound; SURVEY 8e — never a ring for 32 bytes)
            t = (
                torch.frombuffer(bytearray(node), dtype=torch.uint8)
                .clone()
                .to(comm_dev)
            )
            gathered = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(gathered, t)
            if rank == 0:
                nodes = [bytes(g.cpu().numpy().tobytes()) for g in gathered]
                level = sub_depth
                while len(nodes) > 1:
                    nxt = []
                    for i in range(0, len(nodes), 2):
                        if DRY:
                            nxt.append(_hash2(nodes[i], nodes[i + 1]))
                        else:
                            o = ctypes.create_string_buffer(32)
                            lib.m3x_merkleize_chunks(
                                ctx.handle, nodes[i] + nodes[i + 1], 2, 1,
                                -1, o
                            )
                            nxt.append(o.raw)
                    nodes = nxt
                    level += 1
                if DRY:
                    return _hash2(nodes[0], b"dry-cap")
                return ctx.finalize_root(nodes[0], level, 40, N_VALIDATORS)
            return None
        if DRY:
            return _hash2(node, b"dry-cap")
        return ctx.finalize_root(node, sub_depth, 40, N_VALIDATORS)

    def merkle_step():
        """full Deneb state root (C3): registry sharded across ranks, the
        remaining 27 fields + top container on rank 0, all on GPU."""
        reg = registry_root_step()
        if rank != 0:
            return None
        if DRY:
            return _hash2(reg, b"dry-top")
        return bs.state_root(st, ctx=ctx, dev=devmap, registry_root=reg)

    # correctness gate before timing (--full; a plain run keeps only the
    # per-step verdict assert): verdict true, root matches oracle
    if FULL:
        assert bls_step() == 1, "bls batch verdict false on valid workload"
        reg_root = registry_root_step()
        full_root = merkle_step()
        full_root2 = merkle_step()  # collective: every rank participates
        if rank == 0 and not DRY:
            want = ctypes.create_string_buffer(32)
            oracle.m3x_oracle_validator_registry_root(
                ssz_full, ctypes.c_uint64(N_VALIDATORS), want
            )
            assert reg_root == want.raw, "registry root mismatch vs oracle"
            assert full_root == full_root2, "state root not deterministic"
            log("correctness gate passed (verdict true, registry root"
                " bit-exact vs oracle; full-state parity pinned at small n"
                " in tests)")
        elif rank == 0:
            assert full_root == full_root2, "dry state root not deterministic"

    # ---------------- timed region ----------------
    for _ in range(args.warmup):
        bls_step()
        merkle_step()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.time()
    for _ in range(args.steps):
        v = bls_step()
        assert v == 1
        last_root = merkle_step()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.time() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=comm_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # what the last timed step handed its caller: the batch verdict and the
    # 32-byte state root (one byte per element), both as float32
    if args.dump_outputs and rank == 0:
        import numpy as np

        out_dir = Path(args.dump_outputs)
        out_dir.mkdir(parents=True, exist_ok=True)
        np.save(out_dir / "bls_verdict.npy", np.asarray([v], dtype=np.float32))
        np.save(
            out_dir / "state_root.npy",
            np.frombuffer(last_root, dtype=np.uint8).astype(np.float32),
        )

    # separate instrumented pass (per-kernel timing serializes the
    # prepare/h2c stream overlap, so it runs OUTSIDE the timed region)
    if DRY or not FULL:
        ktimes = {}
    else:
        ctx.timing_enable(True)
        bls_step()
        merkle_step()
        ktimes = ctx.kernel_times()  # read BEFORE disable (disable resets)
        ctx.timing_enable(False)

    # everything below the timed region up to the report is --full only
    extras = FULL and rank == 0 and world == 1 and not DRY

    # C4: synthetic Deneb block import (131 sets: 128 aggregates k=512 +
    # proposal + randao + sync-agg as k=1) + full state root
    c4_ms = None
    if extras:
        idx4 = list(range(N_SETS - N_AGG, N_SETS - N_AGG + 128)) + [0, 1, 2]
        m4 = b"".join(bls_w["msgs"][32 * i : 32 * (i + 1)] for i in idx4)
        s4 = b"".join(bls_w["sigs"][96 * i : 96 * (i + 1)] for i in idx4)
        p4 = b""
        o4 = [0]
        for i in idx4:
            a, b = bls_w["offsets"][i], bls_w["offsets"][i + 1]
            p4 += bls_w["pks"][96 * a : 96 * b]
            o4.append(o4[-1] + (b - a))
        d4 = {
            "msgs": ctx.upload(m4),
            "sigs": ctx.upload(s4),
            "pks": ctx.upload(p4),
            "offsets": ctx.upload(
                __import__("numpy").asarray(o4, dtype="uint32").tobytes()
            ),
            "rands": ctx.upload(
                __import__("numpy")
                .asarray([bls_w["rands"][i] for i in idx4], dtype="uint64")
                .tobytes()
            ),
        }
        # (A two-context overlapped variant — BLS on one context, state
        # root on another, mirroring the reference's concurrent block
        # pipeline — measured NO win and extra variance on this path:
        # the root's many small launches interleave anyway. Sequential
        # kept for a clean number.)
        for _ in range(1):
            v = lib.m3x_bls_verify_sets_dev(
                ctx.handle, d4["msgs"], d4["sigs"], d4["pks"], d4["offsets"],
                d4["rands"], len(idx4))
            merkle_step()
        torch.cuda.synchronize()
        tb = time.time()
        v = lib.m3x_bls_verify_sets_dev(
            ctx.handle, d4["msgs"], d4["sigs"], d4["pks"], d4["offsets"],
            d4["rands"], len(idx4))
        merkle_step()
        torch.cuda.synchronize()
        c4_ms = (time.time() - tb) * 1e3
        assert v == 1

    # incremental registry cache: per-block delta rehash
    incr_ms = None
    if extras:
        from lighthouse_amd import tree_hash as th

        cache = th.RegistryCache(ssz_full, N_VALIDATORS, ctx=ctx)
        import random as _rnd

        rng = _rnd.Random(5)
        idxs = sorted(rng.sample(range(N_VALIDATORS), 2048))
        blob = b"".join(
            ssz_full[121 * i : 121 * i + 80]
            + int(31_000_000_000).to_bytes(8, "little")
            + ssz_full[121 * i + 88 : 121 * (i + 1)]
            for i in idxs
        )
        cache.update(idxs, blob)  # warm
        torch.cuda.synchronize()
        tb = time.time()
        cache.update(idxs, blob)
        torch.cuda.synchronize()
        incr_ms = (time.time() - tb) * 1e3
        cache.close()

    # swap-or-not shuffle: 1M indices, 90 rounds
    shuffle_ms = None
    if extras:
        import numpy as _np

        idx_dev = ctx.upload(_np.arange(1 << 20, dtype=_np.uint32).tobytes())
        seed32 = hashlib.sha256(b"bench-shuffle").digest()
        lib.m3x_shuffle_list_dev(ctx.handle, idx_dev, 1 << 20, 90, seed32, 0)
        torch.cuda.synchronize()
        tb = time.time()
        lib.m3x_shuffle_list_dev(ctx.handle, idx_dev, 1 << 20, 90, seed32, 0)
        torch.cuda.synchronize()
        shuffle_ms = (time.time() - tb) * 1e3

    # C5 shape at N=1: 1,048,576 all-k=1 sets on ONE GPU (BASELINE
    # configs[4]'s per-GPU workload; the driver's SCALE run shards the
    # same shape over N GPUs). Reuses the 4096-key pool: signatures are
    # the pool signature for msg-index mod pool — generation cost stays
    # bounded while every set still carries a REAL valid signature.
    c5_sets_per_sec = None
    if extras:
        import numpy as _np

        t0 = time.time()
        n1m = 1 << 20
        pool_msgs = bls_w["msgs"][: 32 * POOL]
        pool_sigs = bls_w["sigs"][: 96 * POOL]
        pool_pks = bls_w["pks"][: 96 * POOL]  # first POOL sets are k=1
        reps = n1m // POOL
        d5 = {
            "msgs": ctx.upload(pool_msgs * reps),
            "sigs": ctx.upload(pool_sigs * reps),
            "pks": ctx.upload(pool_pks * reps),
            "offsets": ctx.upload(
                _np.arange(n1m + 1, dtype=_np.uint32).tobytes()
            ),
            "rands": ctx.upload(
                _np.asarray(
                    [((i * 0x9E3779B97F4A7C15 + 0xC0FFEE) | 1) & (2**64 - 1)
                     for i in range(n1m)],
                    dtype=_np.uint64,
                ).tobytes()
            ),
        }
        log(f"c5 1M-set workload staged in {time.time()-t0:.1f}s")
        v = lib.m3x_bls_verify_sets_dev(
            ctx.handle, d5["msgs"], d5["sigs"], d5["pks"], d5["offsets"],
            d5["rands"], n1m)
        assert v == 1
        torch.cuda.synchronize()
        tb = time.time()
        v = lib.m3x_bls_verify_sets_dev(
            ctx.handle, d5["msgs"], d5["sigs"], d5["pks"], d5["offsets"],
            d5["rands"], n1m)
        torch.cuda.synchronize()
        c5_t = time.time() - tb
        assert v == 1
        c5_sets_per_sec = n1m / c5_t
        for p in d5.values():
            ctx.free(p)

    # split timing: one more pass of each, timed separately (for extras)
    bls_only = merkle_only = None
    if FULL:
        sync()
        tb = time.time()
        bls_step()
        sync()
        bls_only = time.time() - tb
        tb = time.time()
        merkle_step()
        sync()
        merkle_only = time.time() - tb

    # ---------------- cpu baseline (rank 0, N=1) ----------------
    cpu_baseline = None
    cpu_sha = None
    if extras:
        # BLS: 16,384-set sample, same 75/25 mix (12,288 k=1 + 4,096
        # k=512) — large enough that 256 OpenMP threads are saturated and
        # the per-batch final exponentiation amortizes (the round-1
        # 256-set sample measured thread-spawn, not throughput)
        idx = list(range(12288)) + list(
            range(N_SETS - N_AGG, N_SETS - N_AGG + 4096)
        )
        msgs = b"".join(bls_w["msgs"][32 * i : 32 * (i + 1)] for i in idx)
        sigs = b"".join(bls_w["sigs"][96 * i : 96 * (i + 1)] for i in idx)
        pkb = b""
        offs = [0]
        for i in idx:
            a, b = bls_w["offsets"][i], bls_w["offsets"][i + 1]
            pkb += bls_w["pks"][96 * a : 96 * b]
            offs.append(offs[-1] + (b - a))
        off_arr = (ctypes.c_uint32 * len(offs))(*offs)
        rnd = (ctypes.c_uint64 * len(idx))(*[bls_w["rands"][i] for i in idx])
        tcpu = None
        for _ in range(2):  # warm thread pool, then measure (best of 2)
            tb = time.time()
            vcpu = oracle.m3x_oracle_bls_verify_sets(
                msgs, sigs, pkb, off_arr, rnd, ctypes.c_uint64(len(idx))
            )
            t = time.time() - tb
            assert vcpu == 1
            tcpu = t if tcpu is None else min(tcpu, t)
        cores = eff_cores
        cpu_baseline = {
            "value": len(idx) / tcpu,
            "unit": "sets/s",
            "cores": cores,
            "kind": "port",
            "sample": (
                f"{len(idx)} sets (75% k=1, 25% k=512), {tcpu:.2f}s best-of-2,"
                f" OpenMP x{cores} = {len(idx)/tcpu/cores:.0f} sets/s/core"
                " (optimized-port oracle; blst-class asm is ~1000-1500"
                " sets/s/core — see BASELINE.md)"
            ),
        }
        # shuffle CPU baseline (oracle, single list)
        import numpy as _np

        idx = _np.arange(1 << 20, dtype=_np.uint32)
        arr = (ctypes.c_uint32 * (1 << 20)).from_buffer_copy(idx.tobytes())
        seed32 = hashlib.sha256(b"bench-shuffle").digest()
        tb = time.time()
        oracle.m3x_oracle_shuffle_list(
            arr, ctypes.c_uint64(1 << 20), ctypes.c_uint8(90), seed32, 0
        )
        cpu_shuffle_ms = (time.time() - tb) * 1e3
        # SHA: full registry once
        tb = time.time()
        want = ctypes.create_string_buffer(32)
        oracle.m3x_oracle_validator_registry_root(
            ssz_full, ctypes.c_uint64(N_VALIDATORS), want
        )
        tsha = time.time() - tb
        cpu_sha = {
            "node_hashes_per_sec": REGISTRY_NODE_HASHES / tsha,
            "state_root_s": tsha,
            "cores": eff_cores,
            "shuffle_1m_90rounds_ms_1core": cpu_shuffle_ms,
        }

    # ---------------- report ----------------
    if rank == 0:
        steps = args.steps
        sets_per_step = N_SETS * world  # weak scaling: each rank its batch
        value = sets_per_step * steps / elapsed
        miller_ms, miller_n = ktimes.get("bls_miller", (0.0, 0))
        roofline = None
        if miller_n:
            per_launch_ms = miller_ms / miller_n
            ops = N_SETS * FP_MUL_PER_MILLER * INT_OPS_PER_FP_MUL
            achieved = ops / (per_launch_ms / 1e3)
            roofline = {
                "bound": "valu",
                "achieved": achieved,
                "peak": PEAK_INT32_OPS,
                "unit": "int32 ops/s",
                "frac": achieved / PEAK_INT32_OPS,
                "traffic": None,
                "kernel": "k_bls_miller",
                "basis": "analytic op count (DESIGN.md Roofline); VALU workload per SURVEY 8d — not HBM/MFMA-bound",
            }
        if DRY:
            full_nodes = None
        else:
            full_nodes = bs.node_hash_count(N_VALIDATORS)
        sha_hps = (
            full_nodes / merkle_only
            if (full_nodes and merkle_only)
            else None
        )
        line = {
            "metric": "bls_sig_sets_verified_per_sec",
            "value": value,
            "unit": "sets/s",
            "n_gpus": n_gpus,
            "steps": steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {
                "workload": "c2_64k_attestation_sets_plus_c3_registry_root",
                "n_sets_per_gpu": N_SETS,
                "set_mix": "75% k=1 unagg, 25% aggregates k=512",
                "n_validators": N_VALIDATORS,
                "parallelism": f"shard{world}" if world > 1 else "single",
                "dry_run": DRY or None,
                "full": FULL,
            },
            "extra_metrics": {
                "sha256_node_hashes_per_sec": sha_hps,
                "state_root_full_ms": merkle_only * 1e3 if merkle_only else None,
                "state_root_node_hashes": full_nodes,
                "bls_batch_ms": bls_only * 1e3 if bls_only else None,
                "kernel_ms_per_step": {
                    k: v[0] for k, v in ktimes.items() if v[1]
                },
                "c4_block_import_ms": c4_ms,
                "registry_incremental_update_2048_ms": incr_ms,
                "shuffle_1m_90rounds_ms": shuffle_ms,
                "c5_1m_sets_1gpu_sets_per_sec": c5_sets_per_sec,
                "cpu_sha_baseline": cpu_sha,
            },
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
