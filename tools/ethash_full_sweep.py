"""The sealing half of ethash at epoch 0 (16,776,896-byte cache, 1,073,739,904-byte dataset) through the
device-resident entry points, on one explicit stream, timed with HIP events, one process, one GPU, ONE box, no
counters collected:

  generation    the whole dataset by gsv_ethash_dataset_items_dev (k_ethash_items), warmup 1, 3 steps
  full          gsv_ethash_full_batch_dev over 2^16 .. 2^22 (hash, nonce) items, warmup 1, 5 steps, medians
  search        gsv_ethash_search_dev over 2^22 nonces of one header (memset + search + finish), at a
                difficulty nobody meets and at one every 2^16th nonce meets
  light         gsv_ethash_light_batch_dev over the first 2^16 of the same items, in the same run

Per batch: nonces/s and the fraction of the two floors of DESIGN 3.4f.
  gather floor  64 pages of 128 bytes per nonce, uniformly random lines of a table four times the Infinity
                Cache, over 5.5-5.8 TB/s: the guide's rate for random whole rows read into registers, measured
                on 1,152- and 2,304-byte rows, NOT on 128-byte ones
  VALU floor    the VALU instructions of one nonce counted in the built code object (eight lanes of the access
                loop, one lane of the two permutations), multiplies weighted by the rate
                tools/microbench_int.hip measured (0.42 of the full rate)
The first 16 rows of the first batch are checked against tests/golden/ethash.json, and the light kernel's rows
against the full kernel's.

The GPU work runs in ONE child process under ONE time limit, as tools/ethash_sweep.py does: the steps share the
dataset, the stream and the context (one process), so they are not separate commands with a limit each; a step
that faults or hangs ends the child, and nothing is started after it.  GPU box, repo root:
    python tools/ethash_full_sweep.py [--out profiles/ethash/full_sweep.json]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, GEN_STEPS = 1, 5, 3
GPU_TIME_LIMIT_S = 300
BATCHES = [1 << k for k in range(16, 23)]
LIGHT_N = 1 << 16
SEARCH_SPAN = 1 << 22
PEAK_LANE_OPS = 256 * 4 * 64 * 0.5 * 2.4e9  # full-rate 32-bit VALU lane-ops/s (bench.py PEAK_LANE_OPS)
MUL_RATE = 0.42                             # v_mul_lo_u32 over the full rate (profiles/r02/microbench_int.txt)
# per nonce, from the gfx950 build of csrc/ethash.hip (DESIGN 3.4f has the count)
ACCESS_VALU, ACCESS_MULS = 18.4, 7.1        # one access of one lane: the 128-access block is 2,357 VALU, 908 multiplies
KECCAK_VALU = 24 * 201 + 24 * 181 + 120     # seed permutation, closing permutation, state set-up and stores
NONCE_SLOTS = 8 * 64 * (ACCESS_VALU - ACCESS_MULS + ACCESS_MULS / MUL_RATE) + KECCAK_VALU
NONCE_BYTES = 64 * 128
GATHER_LOW, GATHER_HIGH = 5.5e12, 5.8e12
LIGHT_ITEMS_PER_S_PRIOR = 292e6             # 2.28 M headers/s x 128 items


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
    items = size // 64
    dataset = torch.empty(size, dtype=torch.uint8, device=dev)
    assert dataset.data_ptr() % 128 == 0
    torch.cuda.synchronize()

    def median(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record(s)
        for i in range(steps):
            fn()
            ev[i + 1].record(s)
        s.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
        return ms[steps // 2], ms[0], ms[-1]

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1,
           "boxes": 1, "epoch": 0, "cache_bytes": int(cache.numel()), "dataset_bytes": size,
           "timing": "HIP events on one stream, one process, no counters collected",
           "valu_slots_per_nonce": round(NONCE_SLOTS), "gather_bytes_per_nonce": NONCE_BYTES,
           "valu_floor_nonces_per_s": round(PEAK_LANE_OPS / NONCE_SLOTS),
           "gather_floor_nonces_per_s": [round(GATHER_LOW / NONCE_BYTES), round(GATHER_HIGH / NONCE_BYTES)],
           "full": {}}

    med, lo, hi = median(lambda: ctx.ethash_dataset_items_dev(cache, 0, items, dataset, stream=s), GEN_STEPS, WARMUP)
    out["generation"] = {"items": items, "steps": GEN_STEPS, "median_ms": round(med, 3), "min_ms": round(lo, 3),
                         "max_ms": round(hi, 3), "items_per_s": round(items / (med * 1e-3)),
                         "expected_ms_from_the_light_kernels_item_rate": round(items / LIGHT_ITEMS_PER_S_PRIOR * 1e3, 1)}
    print("ETHASH_FULL_STEP generation", out["generation"], flush=True)

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

    def rate(n, med, lo, hi):
        per_s = n / (med * 1e-3)
        return {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "nonces_per_s": round(per_s),
                "fraction_of_gather_floor": [round(per_s * NONCE_BYTES / GATHER_HIGH, 4),
                                             round(per_s * NONCE_BYTES / GATHER_LOW, 4)],
                "fraction_of_valu_floor": round(per_s * NONCE_SLOTS / PEAK_LANE_OPS, 4),
                "gathered_bytes_per_s": round(per_s * NONCE_BYTES)}

    for n in BATCHES:
        med, lo, hi = median(lambda: ctx.ethash_full_batch_dev(dataset, d_h, d_n, d_mix, d_res, stream=s, n=n), STEPS,
                             WARMUP)
        if n == BATCHES[0]:
            got_m, got_r = d_mix[:16].cpu().numpy(), d_res[:16].cpu().numpy()
            for k, r in enumerate(rows):
                assert got_m[k].tobytes().hex() == r["mix"] and got_r[k].tobytes().hex() == r["result"], k
        out["full"][str(n)] = rate(n, med, lo, hi)
        print("ETHASH_FULL_STEP full", n, out["full"][str(n)], flush=True)
    full_m, full_r = d_mix[:LIGHT_N].clone(), d_res[:LIGHT_N].clone()

    # the light kernel over the same items, in the same run
    med, lo, hi = median(lambda: ctx.ethash_light_batch_dev(cache, size, d_h, d_n, d_mix, d_res, stream=s, n=LIGHT_N),
                         STEPS, WARMUP)
    assert torch.equal(d_mix[:LIGHT_N], full_m) and torch.equal(d_res[:LIGHT_N], full_r)
    light_per_s = LIGHT_N / (med * 1e-3)
    out["light"] = {"items": LIGHT_N, "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                    "headers_per_s": round(light_per_s)}
    out["full_over_light_at_65536"] = round(out["full"][str(LIGHT_N)]["nonces_per_s"] / light_per_s, 1)
    print("ETHASH_FULL_STEP light", out["light"], out["full_over_light_at_65536"], flush=True)

    # the search: one header, 2^22 nonces
    out["search"] = {}
    s_off = torch.zeros(1, dtype=torch.int32, device=dev)
    s_non = torch.zeros(1, dtype=torch.int64, device=dev)
    s_fnd = torch.zeros(1, dtype=torch.uint8, device=dev)
    for name, difficulty in (("no_winner", 1 << 200), ("one_in_65536", 1 << 16)):
        d_d = torch.from_numpy(np.frombuffer(difficulty.to_bytes(32, "big"), np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        med, lo, hi = median(lambda: ctx.ethash_search_dev(dataset, d_h[:1], d_d, d_n[:1], SEARCH_SPAN, s_off, s_non,
                                                           d_mix[:1], d_res[:1], s_fnd, stream=s, n=1), STEPS, WARMUP)
        out["search"][name] = dict(rate(SEARCH_SPAN, med, lo, hi), span=SEARCH_SPAN, found=int(s_fnd.cpu()[0]),
                                   offset=int(s_off.cpu().numpy().view(np.uint32)[0]))
        print("ETHASH_FULL_STEP search", name, out["search"][name], flush=True)
    assert out["search"]["no_winner"]["found"] == 0 and out["search"]["one_in_65536"]["found"] == 1
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ETHASH_FULL_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ethash_full_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ETHASH_FULL_SWEEP ")][-1]
    out = json.loads(line[len("ETHASH_FULL_SWEEP "):])
    out["gather_rate_note"] = "5.5-5.8 TB/s is the rate of uniformly random 1,152- and 2,304-byte rows read into " \
                              "registers from a table far larger than the Infinity Cache; 128-byte rows are not " \
                              "measured apart from this sweep"
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
