"""Ethash.VerifyHeaders through the device-resident entry points (gsv_block_header_rules_dev,
gsv_ethash_verify_seal_batch_dev, gsv_block_header_merge_dev), on one explicit stream, timed with HIP events, one
process, one GPU, ONE box, no counters collected:

  kernels   k_block_header, k_block_header_rules and k_block_header_merge alone at 2,048 headers (what
            eth/downloader hands VerifyHeaders at a time) and at 2^18: the context's per-kernel timers (events
            around each launch), mean over the steps
  chain     rules -> seal -> merge at 2,048 headers with every seal checked, and with one seal in 100
            (fsHeaderCheckFrequency: the seal kernel runs over the first 21 headers' rows, as a caller that
            compacts would), medians over the steps
  seal      gsv_ethash_verify_seal_batch_dev alone over the same 2,048 rows, in the same run

The figure: the whole chain over the seal kernel alone with every seal checked, and the new kernels' share of the
chain.  The headers are a valid chain built with tests/block_header_model.py behind block 0 (epoch 0: the real
16,776,896-byte cache), with made-up seals: the seal kernel does the same work whatever its verdict.  The 2^18
batch is that chain 128 times over (the seams have no ancestor).  Every status is checked against the model.

The GPU work runs in ONE child process under ONE time limit, as tools/ethash_full_sweep.py does; a step that
faults or hangs ends the child, and nothing is started after it.  GPU box, repo root:
    python tools/block_header_sweep.py [--out profiles/headers/sweep.json]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 20
GPU_TIME_LIMIT_S = 300
N, BIG = 2048, 1 << 18


def worker():
    sys.path[:0] = [os.path.join(ROOT, "geth-sharding_amd"), os.path.join(ROOT, "tests"), ROOT]
    import numpy as np
    import torch

    import block_header_cases as C
    import block_header_model as B
    import gsv
    from gsv import _lib
    from gsv import ethash as E
    from gsv import params as P

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)

    parent = B.new_header(Difficulty=1 << 34, Number=0, GasLimit=8000000, Time=1500000000, Extra=b"sweep")
    pb = B.encode_header(parent)
    blobs, prev, prev_blob = [], parent, pb
    rng = np.random.default_rng(0x5EED)
    for k in range(N):
        h = C.child(C.TEST_CONFIG, prev, prev_blob, dt=1 + int(rng.integers(0, 30)), salt=k,
                    Extra=rng.bytes(int(rng.integers(0, 33))), MixDigest=rng.bytes(32), Nonce=rng.bytes(8),
                    Bloom=rng.bytes(256), TxHash=rng.bytes(32), ReceiptHash=rng.bytes(32))
        blobs.append(B.encode_header(h))
        prev, prev_blob = h, blobs[-1]
    now = prev["Time"]
    want, _ = B.verify_headers(C.TEST_CONFIG, blobs, pb, now)
    assert want == [0] * N

    def tensors(n, reps):
        flat = np.frombuffer(b"".join(blobs) * reps + bytes(8), np.uint8)
        lens = np.array([len(b) for b in blobs] * reps, np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        t = {"rlp": torch.from_numpy(flat.copy()).to(dev), "off": torch.from_numpy(off.view(np.int64)).to(dev),
             "parent": torch.from_numpy(np.frombuffer(pb, np.uint8).copy()).to(dev),
             "work": torch.empty(gsv.block_header_work_bytes(n), dtype=torch.uint8, device=dev),
             "nonce": torch.empty(n, dtype=torch.int64, device=dev)}
        for k in ("hnn", "mix", "diff"):
            t[k] = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        for k in ("pre", "post", "seal", "status"):
            t[k] = torch.zeros(n, dtype=torch.uint8, device=dev)
        return t, int(flat.size - 8)

    def rules(t, n):
        ctx.block_header_rules_dev(P.TestChainConfig, t["rlp"], t["off"], n, t["parent"], now, t["work"], t["hnn"],
                                   t["nonce"], t["mix"], t["diff"], t["pre"], t["post"], stream=s)

    def median(fn):
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

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1, "boxes": 1,
           "timing": "HIP events on one stream, one process, no counters collected", "kernels": {}}

    # the three new kernels alone: the context's timers around each launch
    for n, reps in ((N, 1), (BIG, BIG // N)):
        t, nbytes = tensors(n, reps)
        torch.cuda.synchronize()
        for _ in range(WARMUP):
            rules(t, n)
            ctx.block_header_merge_dev(t["pre"], None, None, t["post"], t["status"], n=n, stream=s)
        s.synchronize()
        ctx.set_timing(True)
        ctx.reset_timing()
        for _ in range(STEPS):
            rules(t, n)
            ctx.block_header_merge_dev(t["pre"], None, None, t["post"], t["status"], n=n, stream=s)
        s.synchronize()
        row = {"rlp_bytes": nbytes}
        for name, kid in (("k_block_header", _lib.K_BLOCK_HEADER), ("k_block_header_rules", _lib.K_BLOCK_RULES),
                          ("k_block_header_merge", _lib.K_BLOCK_MERGE)):
            ms, launches = ctx.kernel_time(kid)
            assert launches == STEPS
            row[name] = {"mean_ms": round(ms / launches, 4), "headers_per_s": round(n / (ms / launches * 1e-3))}
        ctx.set_timing(False)
        ctx.reset_timing()
        st = t["status"].cpu().numpy()
        seams = np.arange(n) % N == 0
        seams[0] = False
        assert (st[~seams] == 0).all() and (st[seams] == _lib.ST_UNKNOWN_ANCESTOR).all()
        out["kernels"][str(n)] = row
        print("HEADER_SWEEP_STEP kernels", n, row, flush=True)
        del t

    # the chain at 2,048 headers over the real epoch-0 cache
    cache = torch.from_numpy(E.generateCache(E.cacheSize(0), E.seedHash(0))).to(dev)
    size = E.datasetSize(0)
    t, _ = tensors(N, 1)
    few = (N + 99) // 100
    seals = torch.zeros(N, dtype=torch.uint8, device=dev)
    seals[:few] = 1
    torch.cuda.synchronize()

    def seal(m):
        ctx.ethash_verify_seal_batch_dev(cache, size, t["hnn"], t["nonce"], t["mix"], t["diff"], t["seal"], stream=s, n=m)

    def chain_all():
        rules(t, N)
        seal(N)
        ctx.block_header_merge_dev(t["pre"], t["seal"], None, t["post"], t["status"], n=N, stream=s)

    def chain_few():
        rules(t, N)
        seal(few)
        ctx.block_header_merge_dev(t["pre"], t["seal"], seals, t["post"], t["status"], n=N, stream=s)

    out["chain_all_seals"] = median(chain_all)
    assert (t["status"].cpu().numpy() == _lib.ST_INVALID_MIX_DIGEST).all()  # made-up seals
    out["seal_alone"] = median(lambda: seal(N))
    out["chain_one_seal_in_100"] = dict(median(chain_few), sealed=few)
    st = t["status"].cpu().numpy()
    assert (st[:few] == _lib.ST_INVALID_MIX_DIGEST).all() and (st[few:] == 0).all()
    new_ms = sum(out["kernels"][str(N)][k]["mean_ms"] for k in ("k_block_header", "k_block_header_rules",
                                                                "k_block_header_merge"))
    out["headers"] = N
    out["chain_over_seal_alone"] = round(out["chain_all_seals"]["median_ms"] / out["seal_alone"]["median_ms"], 4)
    out["new_kernels_ms"] = round(new_ms, 4)
    out["new_kernels_share_of_chain"] = round(new_ms / out["chain_all_seals"]["median_ms"], 4)
    out["chain_all_seals"]["headers_per_s"] = round(N / (out["chain_all_seals"]["median_ms"] * 1e-3))
    out["chain_one_seal_in_100"]["headers_per_s"] = round(N / (out["chain_one_seal_in_100"]["median_ms"] * 1e-3))
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("HEADER_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"block_header_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("HEADER_SWEEP ")][-1]
    out = json.loads(line[len("HEADER_SWEEP "):])
    out["not_measured"] = "one box only; no PMC counters, no traces, one GPU; the host form's copies and its host-side " \
                          "cache generation; real seals (the seal kernel's work does not depend on its verdict)"
    txt = json.dumps(out, indent=1)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
