"""The producer side measured through the device-resident entry points, at 100 collations of 8,192
transactions (a 100 MiB body) and at 13 (a rank's share at 8 GPUs), all readings taken in one run:

    (a) serialize      gsv_blob_serialize_batch_dev alone: time and GB/s counted as source bytes read plus
                       body bytes written, beside a device-to-device copy of the same body bytes on the same
                       stream (torch Tensor.copy_, a hipMemcpyAsync): the yardstick, not a datasheet figure
    (b) chunk_root     gsv_chunk_root_batch_dev alone on the same bodies; with --parent-lib PATH also
                       through that other build of libgsv.so (GSV_LIB_PATH) in child processes of their own,
                       before and after this tree's, for the same-box comparison with the parent commit
    (c) proposer       gsv_proposer_create_collations_dev: one step at a time (depth 1) and with consecutive
                       steps on 4 streams at pipeline depth 4, the depth the notary leg of bench.py uses
        sign           gsv_ecdsa_sign_batch_dev on n hashes alone (the fourth part of the step)

The inputs are made on the device: gsv_notary_synth_dev bodies go through gsv_blob_deserialize_batch_dev,
and the blobs it finds are compacted with torch into the blob array the serializer reads.  Every run checks
that serializing them gives the synthetic bodies back byte for byte and that the proposer step's roots are
the chunk-root leg's.  Legs (a), (b), sign and depth-1 (c) are timed with HIP events on one
gsv_stream_create stream (warmup 3, 20 steps; median / min / max), (a) and the copy as replays of a graph
captured from the call (_timed_graph says why); depth-4 (c) by the wall clock over 40 steps.  Writes profiles/proposer/sweep.json (--out PATH for another place) and prints the same JSON line.
Each GPU step runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/proposer_sweep.py [--parent-lib PATH]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, PIPE_STEPS = 3, 20, 40
SIZES = (100, 13)
TXS = 8192
DEPTH = 4
GPU_TIME_LIMIT_S = 240


def _setup():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import torch

    import gsv

    ctx = gsv.default_context()
    return torch, gsv, ctx, torch.device("cuda", ctx.device)


def _timed(torch, s, fn):
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


def _timed_graph(torch, s, fn):
    """fn captured once into a HIP graph, the replays timed: a *_dev call compares its host tables with the
    prepared shape's on every call (6.5 MB of offsets at 819,200 blobs), which a 0.1 ms kernel timed between
    events on the stream would show as GPU idle time; a replay has no host side"""
    fn()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()

    def replay():
        with torch.cuda.stream(s):
            g.replay()
    r = _timed(torch, s, replay)
    del g
    return r


def chunk_worker():
    """leg (b) alone, on the synthetic bodies (what the serializer reproduces): any build of the library"""
    import numpy as np
    torch, gsv, ctx, dev = _setup()
    (s,) = ctx.pipeline_streams(1)
    out = {}
    for n in SIZES:
        bodies = torch.empty((n * TXS * 128,), dtype=torch.uint8, device=dev)
        ctx.notary_synth_dev(777, 0, n, TXS, bodies, None, None, stream=s)
        off = np.arange(n + 1, dtype=np.uint64) * TXS * 128
        roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        ctx.chunk_root_prepare(off)
        s.synchronize()
        out["n_%d" % n] = _timed(torch, s, lambda: ctx.chunk_root_batch_dev(bodies, off, roots, stream=s, prepare=False))
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("PROPOSER_SWEEP " + json.dumps(out), flush=True)


def worker():
    import numpy as np
    torch, gsv, ctx, dev = _setup()
    (s,) = ctx.pipeline_streams(1)

    def u8(*shape):
        return torch.empty(shape, dtype=torch.uint8, device=dev)

    out = {"warmup": WARMUP, "steps": STEPS, "pipeline_steps": PIPE_STEPS, "pipeline_depth": DEPTH,
           "device": torch.cuda.get_device_name(ctx.device)}
    for n in SIZES:
        # ---- inputs, on the device: synthetic bodies -> Deserialize -> the compact blob array
        body_bytes = n * TXS * 128
        synth = u8(body_bytes)
        ctx.notary_synth_dev(777, 0, n, TXS, synth, None, None, stream=s)
        h_off = np.arange(n + 1, dtype=np.uint64) * TXS * 128
        doff = gsv.blob_data_layout(h_off)
        nb = torch.empty((n,), dtype=torch.int32, device=dev)
        start = torch.empty((n, TXS), dtype=torch.int32, device=dev)
        ln = torch.empty((n, TXS), dtype=torch.int32, device=dev)
        sk, data = u8(n, TXS), u8(int(doff[-1]))
        ctx.blob_deserialize_batch_dev(synth, h_off, TXS, nb, start, ln, sk, data, stream=s)
        s.synchronize()
        assert int(nb.min()) == TXS and int(nb.max()) == TXS and int(sk.max()) == 0
        with torch.cuda.stream(s):
            lens = ln.view(-1).to(torch.int64)
            src = start.view(-1).to(torch.int64) + torch.from_numpy(doff[:-1].astype(np.int64)).to(dev).repeat_interleave(TXS)
            ends = torch.cumsum(lens, 0)
            total = int(ends[-1])
            idx = torch.arange(total, device=dev) + (src - (ends - lens)).repeat_interleave(lens)
            blobs = data[idx].contiguous()
            del idx
        s.synchronize()
        blob_off = np.zeros(n * TXS + 1, np.uint64)
        blob_off[1:] = ends.cpu().numpy()
        list_off = np.arange(n + 1, dtype=np.uint64) * TXS
        body_off = gsv.blob_serialized_size(blob_off, list_off)
        assert list(body_off) == list(h_off)
        bodies, copy_dst = u8(body_bytes), u8(body_bytes)
        g = torch.Generator(device=dev).manual_seed(5)
        sid = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        per = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        prop = torch.randint(0, 256, (n, 20), dtype=torch.uint8, device=dev, generator=g)
        key = torch.randint(1, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        key[:, 0] = 0x7F  # below the group order
        roots_b = u8(n, 32)
        ctx.blob_serialize_prepare(blob_off, list_off)
        ctx.chunk_root_prepare(body_off)
        ctx.set_pipeline_depth(DEPTH)
        ctx.proposer_prepare(blob_off, list_off)
        ctx.set_pipeline_depth(1)
        pouts = [(u8(body_bytes), u8(n, 32), u8(n, 32), u8(n, 65), u8(n)) for _ in range(DEPTH)]
        sig_alone, st_alone = u8(n, 65), u8(n)
        torch.cuda.synchronize()

        def copy():
            with torch.cuda.stream(s):
                copy_dst.copy_(synth)

        def proposer(k, st):
            b, r, h, sg, stt = pouts[k]
            ctx.proposer_create_collations_dev(blobs, blob_off, list_off, sid, per, prop, key, b, r, h, sg, stt,
                                               stream=st, prepare=False)
        r = {"collations": n, "txs_per_collation": TXS, "body_bytes": body_bytes, "blob_bytes": total}
        for rnd in ("", "_2"):  # two interleaved rounds: the A/A spread of each leg
            r["serialize" + rnd] = _timed_graph(torch, s, lambda: ctx.blob_serialize_batch_dev(
                blobs, blob_off, list_off, bodies, None, stream=s, prepare=False))
            r["copy_dtod" + rnd] = _timed_graph(torch, s, copy)
            r["chunk_root" + rnd] = _timed(torch, s, lambda: ctx.chunk_root_batch_dev(
                bodies, body_off, roots_b, stream=s, prepare=False))
            r["sign" + rnd] = _timed(torch, s, lambda: ctx.ecdsa_sign_batch_dev(pouts[0][2], key, sig_alone, st_alone,
                                                                               stream=s))
            r["proposer_depth1" + rnd] = _timed(torch, s, lambda: proposer(0, s))
        # the round trip: the serializer gives the synthetic bodies back, the step's roots are leg (b)'s
        assert torch.equal(bodies, synth), "Serialize(Deserialize(body)) differs from the body"
        assert torch.equal(pouts[0][0], synth) and torch.equal(pouts[0][1], roots_b)
        assert int(pouts[0][4].max()) == 0 and torch.equal(pouts[0][3], sig_alone)
        # depth-4 pipeline by the wall clock (as tools/notary_sweep.py)
        ss = ctx.pipeline_streams(DEPTH)
        for rnd in ("", "_2"):
            for i in range(DEPTH):
                proposer(i, ss[i])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(PIPE_STEPS):
                proposer(i % DEPTH, ss[i % DEPTH])
            torch.cuda.synchronize()
            r["proposer_depth%d_ms_per_step%s" % (DEPTH, rnd)] = round((time.perf_counter() - t0) / PIPE_STEPS * 1e3, 4)
        ctx.destroy_streams(ss)
        for k in range(DEPTH):
            assert torch.equal(pouts[k][1], roots_b) and torch.equal(pouts[k][3], sig_alone)
        best = lambda leg: min(r[leg]["median_ms"], r[leg + "_2"]["median_ms"])  # noqa: E731
        moved = total + body_bytes
        r["serialize_gb_per_s"] = round(moved / (best("serialize") * 1e-3) / 1e9, 1)
        r["copy_dtod_gb_per_s"] = round(2 * body_bytes / (best("copy_dtod") * 1e-3) / 1e9, 1)
        r["serialize_rate_over_copy_rate"] = round(r["serialize_gb_per_s"] / r["copy_dtod_gb_per_s"], 3)
        r["sum_of_parts_ms"] = round(best("serialize") + best("chunk_root") + best("sign"), 4)
        d4 = min(r["proposer_depth%d_ms_per_step" % DEPTH], r["proposer_depth%d_ms_per_step_2" % DEPTH])
        r["proposer_depth%d_over_sum_of_parts" % DEPTH] = round(d4 / r["sum_of_parts_ms"], 4)
        r["proposer_depth1_over_sum_of_parts"] = round(best("proposer_depth1") / r["sum_of_parts_ms"], 4)
        r["collations_per_s_depth%d" % DEPTH] = round(n / (d4 * 1e-3))
        out["n_%d" % n] = r
        del blobs, bodies, copy_dst, synth, data, pouts
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("PROPOSER_SWEEP " + json.dumps(out), flush=True)


def _child(flag, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), flag],
                       stdout=subprocess.PIPE, text=True, env=env)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"proposer_sweep: the GPU step {flag} ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROPOSER_SWEEP ")][-1]
    return json.loads(line[len("PROPOSER_SWEEP "):])


def main():
    if "--worker" in sys.argv:
        return worker()
    if "--chunk-worker" in sys.argv:
        return chunk_worker()
    dest = os.path.join(ROOT, "profiles", "proposer", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    parent = None
    if "--parent-lib" in sys.argv:
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent-lib") + 1])
    penv = dict(os.environ, GSV_LIB_PATH=parent) if parent else None
    before = _child("--chunk-worker", penv) if parent else None
    out = _child("--worker")
    out["chunk_root_this_tree_alone"] = _child("--chunk-worker")
    if parent:
        out["chunk_root_parent_build"] = {"before": before, "after": _child("--chunk-worker", penv)}
        for n in SIZES:
            k = "n_%d" % n
            p = min(before[k]["median_ms"], out["chunk_root_parent_build"]["after"][k]["median_ms"])
            t = out["chunk_root_this_tree_alone"][k]["median_ms"]  # like with like: the same child, the same bodies
            out[k]["chunk_root_this_tree_over_parent"] = round(t / p, 4)
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
