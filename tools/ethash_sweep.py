"""hashimotoLight batch rates through the device-resident entry point (gsv_ethash_light_batch_dev) at epoch 0
(16,776,896-byte cache, 1,073,739,904-byte dataset): batches of 2^10 to 2^18 headers on one explicit stream,
timed with HIP events (warmup 1, 5 steps, medians), one process, one GPU, ONE box, no counters collected.

Per batch size: headers/s and the fraction of the two floors of DESIGN 3.4e.
  VALU floor    the VALU instructions of one header, counted in the built code object (both lanes of its pair),
                v_mul_lo_u32 / v_mul_hi_u32 weighted by the rate tools/microbench_int.hip measured
                (0.42 of the full rate), over the chip's full-rate lane-ops/s
  gather floor  32,896 cache rows of 64 bytes per header over the Infinity-Cache gather rate of
                uniformly random rows (8.6 TB/s: measured on 1,152-byte rows, not on 64-byte ones)
The first 16 rows of the first batch are checked against tests/golden/ethash.json.  The CPU figure is not
measured here: the reference's libethash took 3.0 ms per header on one core of the CPU machine it was built
on (gcc -O2), 5,300 headers/s if 16 threads scaled perfectly; that machine is not the GPU box's host.

The GPU work runs in ONE child process under its own time limit.  GPU box, repo root:
    python tools/ethash_sweep.py [--out profiles/ethash/sweep.json]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 1, 5
GPU_TIME_LIMIT_S = 420
BATCHES = [1 << k for k in range(10, 19)]
PEAK_LANE_OPS = 256 * 4 * 64 * 0.5 * 2.4e9  # full-rate 32-bit VALU lane-ops/s (bench.py PEAK_LANE_OPS)
MUL_RATE = 0.42                             # v_mul_lo_u32 over the full rate (profiles/r02/microbench_int.txt)
# VALU instructions in the gfx950 build of csrc/ethash.hip (DESIGN 3.4e has the count): a Keccak-f round, one
# parent round of generateDatasetItem (of which multiplies), the rest of one dataset item and its use
ROUND_VALU, PARENT_VALU, PARENT_MULS, ITEM_REST_VALU = 180, 42, 19, 123
ITEM_SLOTS = 2 * 24 * ROUND_VALU + 256 * (PARENT_VALU - PARENT_MULS + PARENT_MULS / MUL_RATE) + ITEM_REST_VALU
HEADER_SLOTS = 2 * (64 * ITEM_SLOTS + 24 * ROUND_VALU + 23 * ROUND_VALU + 58)  # two lanes; seed + closing hash
ROWS_PER_HEADER = 64 * 2 * 257
GATHER_BYTES_PER_S = 8.6e12
CPU_HEADERS_PER_S_16_THREADS = 16 / 3.0e-3


def worker():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import numpy as np
    import torch

    import gsv
    from gsv import ethash as E

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    with open(os.path.join(ROOT, "tests", "golden", "ethash.json")) as f:
        rows = json.load(f)["light"]["0"]
    cache = torch.from_numpy(E.generateCache(E.cacheSize(0), E.seedHash(0))).to(dev)
    size = E.datasetSize(0)
    nmax = BATCHES[-1]
    rng = np.random.default_rng(0xE7)
    h = rng.integers(0, 256, (nmax, 32), dtype=np.uint8)
    nn = rng.integers(0, 2**63, nmax, dtype=np.int64)
    for k, r in enumerate(rows):
        h[k] = np.frombuffer(bytes.fromhex(r["hash"]), np.uint8)
        nn[k] = np.array([r["nonce"]], np.uint64).view(np.int64)[0]
    d_h, d_n = torch.from_numpy(h).to(dev), torch.from_numpy(nn).to(dev)
    d_mix = torch.empty((nmax, 32), dtype=torch.uint8, device=dev)
    d_res = torch.empty((nmax, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1,
           "boxes": 1, "epoch": 0, "cache_bytes": int(cache.numel()), "dataset_bytes": size,
           "valu_slots_per_header": round(HEADER_SLOTS), "gather_bytes_per_header": ROWS_PER_HEADER * 64,
           "valu_floor_headers_per_s": round(PEAK_LANE_OPS / HEADER_SLOTS),
           "gather_floor_headers_per_s": round(GATHER_BYTES_PER_S / (ROWS_PER_HEADER * 64)), "batches": {}}
    for n in BATCHES:
        def fn():
            ctx.ethash_light_batch_dev(cache, size, d_h, d_n, d_mix, d_res, stream=s, n=n)
        for _ in range(WARMUP):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
        ev[0].record(s)
        for i in range(STEPS):
            fn()
            ev[i + 1].record(s)
        s.synchronize()
        if n == BATCHES[0]:
            got_m, got_r = d_mix[:16].cpu().numpy(), d_res[:16].cpu().numpy()
            for k, r in enumerate(rows):
                assert got_m[k].tobytes().hex() == r["mix"] and got_r[k].tobytes().hex() == r["result"], k
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(STEPS))
        t = ms[STEPS // 2] * 1e-3
        out["batches"][str(n)] = {
            "median_ms": round(ms[STEPS // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "headers_per_s": round(n / t),
            "fraction_of_valu_floor": round(n / t * HEADER_SLOTS / PEAK_LANE_OPS, 4),
            "fraction_of_gather_floor": round(n / t * ROWS_PER_HEADER * 64 / GATHER_BYTES_PER_S, 4),
            "over_cpu_16_threads_if_perfect": round(n / t / CPU_HEADERS_PER_S_16_THREADS, 1)}
        print("ETHASH_STEP", n, out["batches"][str(n)], flush=True)
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ETHASH_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ethash_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ETHASH_SWEEP ")][-1]
    out = json.loads(line[len("ETHASH_SWEEP "):])
    out["cpu"] = {"what": "the reference's libethash, gcc -O2, one hashimotoLight at epoch 0 on one core",
                  "ms_per_header": 3.0, "headers_per_s_16_threads_if_perfect": round(CPU_HEADERS_PER_S_16_THREADS),
                  "where": "measured on the CPU machine the library was built on, not on the GPU box's host"}
    out["gather_rate_note"] = "8.6 TB/s is the rate of uniformly random 1,152-byte rows from the Infinity Cache; " \
                              "64-byte rows are not measured apart from this sweep"
    out["not_measured"] = "one box only; no PMC counters, no traces, one GPU"
    txt = json.dumps(out, indent=1)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
