"""SHA-256 and RIPEMD-160 batch rates through the device-resident entry points (gsv_sha256_batch_dev,
gsv_ripemd160_batch_dev) on one explicit stream, timed with HIP events (warmup 2, 10 steps, medians), one
process, one GPU, no counters:

    2^20 messages of 32, 64, 128 and 1,024 bytes, 2^16 messages of 4 KiB

Messages are random bytes of one length, back to back from a 256-byte-aligned start.  Per shape and hash:
hashes/s, compressions/s ((len + 72) // 64 a message), GB/s of message bytes, and the fraction of the VALU
floor: compressions/s over PEAK_LANE_OPS / the VALU instructions of one compression, counted in the built
code object (the straight-line block of each kernel's loop that holds the rounds; DESIGN 3.4d has the
count and the arithmetic).  In the same run k_keccak256 hashes the same bytes, with its fraction of its own
floor (bench.py's figures: 4,320 VALU instructions a permutation, 4,198 for a message's last), and
afterwards hashlib.sha256 hashes a share of each shape on 16 threads (it holds the interpreter lock for
messages under 2 KiB, so those shapes are one core's rate).  The first 32 rows of every launch are checked
against hashlib / tests/ripemd160_model.py.

The GPU work runs in ONE child process under its own time limit; the parent only starts it and times the CPU
side.  GPU box, repo root:
    python tools/hash_sweep.py [--out profiles/hash/sweep.json]
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 10
GPU_TIME_LIMIT_S = 300
SHAPES = [(1 << 20, 32), (1 << 20, 64), (1 << 20, 128), (1 << 20, 1024), (1 << 16, 4096)]
PEAK_LANE_OPS = 256 * 4 * 64 * 0.5 * 2.4e9  # full-rate 32-bit VALU lane-ops/s (bench.py PEAK_LANE_OPS)
# VALU instructions of the block that holds one compression's rounds, gfx950 build of csrc/hash_md.hip
VALU_PER_COMPRESSION = {"sha256": 1406, "ripemd160": 939}
KECCAK_FLOOR, KECCAK_DIGEST_FLOOR = 24 * 180, 23 * 180 + 58


def worker():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import gsv
    import ripemd160_model as M

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
        ev[0].record(s)
        for i in range(STEPS):
            fn()
            ev[i + 1].record(s)
        s.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(STEPS))
        return {"median_ms": round(ms[STEPS // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1,
           "peak_lane_ops_per_s": PEAK_LANE_OPS, "valu_per_compression": VALU_PER_COMPRESSION, "shapes": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(256160)
    for n, ln in SHAPES:
        data = torch.randint(0, 256, (n * ln + 16,), dtype=torch.uint8, device=dev, generator=gen)
        off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * ln).contiguous()
        rows = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        head = data[:32 * ln].cpu().numpy().tobytes()
        msgs = [head[i * ln:(i + 1) * ln] for i in range(32)]
        torch.cuda.synchronize()
        comps = n * ((ln + 72) // 64)
        shape = {"n": n, "len": ln, "compressions": comps}
        for kind, call, want in (("sha256", ctx.sha256_batch_dev, lambda m: hashlib.sha256(m).digest()),
                                 ("ripemd160", ctx.ripemd160_batch_dev, M.precompile_row)):
            r = timed(lambda: call(data, off, rows, stream=s))
            got = rows[:32].cpu().numpy()
            assert all(got[i].tobytes() == want(msgs[i]) for i in range(32)), (kind, n, ln)
            t = r["median_ms"] * 1e-3
            r.update({"hashes_per_s": round(n / t), "compressions_per_s": round(comps / t),
                      "gb_per_s": round(n * ln / t / 1e9, 2),
                      "fraction_of_valu_floor": round(comps / t * VALU_PER_COMPRESSION[kind] / PEAK_LANE_OPS, 4)})
            shape[kind] = r
        perms = n * (ln // 136 + 1)
        floor = (KECCAK_FLOOR * (perms - n) + KECCAK_DIGEST_FLOOR * n) / perms
        r = timed(lambda: ctx.keccak256_batch_dev(data, off, rows, stream=s))
        t = r["median_ms"] * 1e-3
        r.update({"hashes_per_s": round(n / t), "permutations_per_s": round(perms / t), "gb_per_s": round(n * ln / t / 1e9, 2),
                  "valu_floor_per_permutation": round(floor, 1),
                  "fraction_of_valu_floor": round(perms / t * floor / PEAK_LANE_OPS, 4)})
        shape["keccak256"] = r
        for kind in ("sha256", "ripemd160"):
            shape[kind]["fraction_over_keccak_fraction"] = round(
                shape[kind]["fraction_of_valu_floor"] / r["fraction_of_valu_floor"], 3)
        out["shapes"]["%dx%d" % (n, ln)] = shape
        del data, off, rows
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("HASH_SWEEP " + json.dumps(out), flush=True)


def cpu_side(threads=16):
    """hashlib.sha256 over a share of each shape's messages on `threads` threads: hashes/s = messages / wall time"""
    from concurrent.futures import ThreadPoolExecutor
    out = {"what": "hashlib.sha256, one call a message", "threads": threads}

    def run(msgs):
        for m in msgs:
            hashlib.sha256(m).digest()

    for n, ln in SHAPES:
        per = max(64, min(1 << 13, (64 << 20) // (ln * threads)))
        blob = os.urandom(per * ln)
        parts = [[blob[i * ln:(i + 1) * ln] for i in range(per)] for _ in range(threads)]
        with ThreadPoolExecutor(threads) as pool:
            t0 = time.perf_counter()
            list(pool.map(run, parts))
            dt = time.perf_counter() - t0
        out["%dx%d" % (n, ln)] = {"messages": per * threads, "hashes_per_s": round(per * threads / dt),
                                  "gb_per_s": round(per * threads * ln / dt / 1e9, 3)}
    return out


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"hash_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("HASH_SWEEP ")][-1]
    out = json.loads(line[len("HASH_SWEEP "):])
    out["cpu"] = cpu_side()
    for k, v in out["shapes"].items():
        v["sha256"]["gpu_over_cpu"] = round(v["sha256"]["hashes_per_s"] / out["cpu"][k]["hashes_per_s"], 1)
    out["not_measured"] = "PMC counters, traces, more than one GPU"
    txt = json.dumps(out, indent=1)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
