"""bn256ScalarMul / bn256Add batch rates through the device-resident entry points
(gsv_bn256_scalar_mul_batch_dev, gsv_bn256_add_batch_dev): the GLV multiplication against the
bit-serial form (GSV_BN_G1_BITSERIAL=1), interleaved in one process on one explicit stream, timed with
HIP events: warmup 3, 20 steps, n = 2^20 (mul, add) and n = 8,192 (mul).  The inputs are made on the
device (P_i = s_i G by the multiplication itself, scalars uniform over 256 bits); every run checks the
statuses and that both forms return the same bytes.  Prints one JSON line.

The GPU work runs in ONE child process under its own time limit (`timeout -k 10`); the parent only
starts it and, with --cpu, times the oracle's CPU restatement of the multiplication
(oracle.bn256_g1_mul looped on 16 threads; the Go reference itself is not built here).  GPU box, repo root:
    python tools/bn_g1_sweep.py [--cpu] > profiles/g1/sweep.json
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 20
N_BIG, N_SMALL = 1 << 20, 8192
GPU_TIME_LIMIT_S = 240
# v_mad_u64_u32 per item: the instrumented build's counts over 65,536 uniform 256-bit scalars
# (tools/count_ops.py, profiles/g1/opcount.json): F_p products x (81 + 81 for the Montgomery reduction)
MADS = {"mul_glv": 317113.5, "mul_bitserial": 520404.4, "add": 4536.0}
PEAK_MADS = 39.32e12  # v_mad_u64_u32 per second, the VALU peak of README.md / DESIGN.md


def worker():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import numpy as np
    import torch

    import gsv

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    rng = np.random.default_rng(2026)

    def scalars(n):
        return torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)

    def timed(fn, variant=None):
        if variant:
            os.environ["GSV_BN_G1_BITSERIAL"] = "1"
        try:
            for _ in range(WARMUP):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
            ev[0].record(s)
            for i in range(STEPS):
                fn()
                ev[i + 1].record(s)
            s.synchronize()
        finally:
            os.environ.pop("GSV_BN_G1_BITSERIAL", None)
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(STEPS))
        return {"median_ms": round(ms[STEPS // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device)}
    for n in (N_BIG, N_SMALL):
        g = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        g[:, 31] = 1
        g[:, 63] = 2
        rec = torch.cat([g, scalars(n)], dim=1).contiguous()
        pts = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        st = torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.bn256_scalar_mul_batch_dev(rec, pts, st, stream=s)
        s.synchronize()
        assert int(st.max()) == 0
        rec = torch.cat([pts, scalars(n)], dim=1).contiguous()
        o1, o2 = torch.empty_like(pts), torch.empty_like(pts)
        torch.cuda.synchronize()
        r = {"n": n}
        r["glv"] = timed(lambda: ctx.bn256_scalar_mul_batch_dev(rec, o1, st, stream=s))
        assert int(st.max()) == 0
        r["bitserial"] = timed(lambda: ctx.bn256_scalar_mul_batch_dev(rec, o2, st, stream=s), "bitserial")
        assert int(st.max()) == 0 and torch.equal(o1, o2), "the two forms differ"
        # a second interleaved round: A, B, A, B in one process
        r["glv_2"] = timed(lambda: ctx.bn256_scalar_mul_batch_dev(rec, o1, st, stream=s))
        r["bitserial_2"] = timed(lambda: ctx.bn256_scalar_mul_batch_dev(rec, o2, st, stream=s), "bitserial")
        t_glv = min(r["glv"]["median_ms"], r["glv_2"]["median_ms"]) * 1e-3
        t_bs = min(r["bitserial"]["median_ms"], r["bitserial_2"]["median_ms"]) * 1e-3
        r["glv_items_per_s"] = round(n / t_glv)
        r["bitserial_items_per_s"] = round(n / t_bs)
        r["time_ratio_glv_over_bitserial"] = round(t_glv / t_bs, 4)
        r["mad_ratio_glv_over_bitserial"] = round(MADS["mul_glv"] / MADS["mul_bitserial"], 4)
        r["glv_mad_fraction_of_peak"] = round(MADS["mul_glv"] * n / t_glv / PEAK_MADS, 4)
        r["bitserial_mad_fraction_of_peak"] = round(MADS["mul_bitserial"] * n / t_bs / PEAK_MADS, 4)
        out["mul_%d" % n] = r
        if n == N_BIG:
            arec = torch.cat([pts, torch.roll(pts, 1, 0)], dim=1).contiguous()
            torch.cuda.synchronize()
            a = {"n": n}
            a.update(timed(lambda: ctx.bn256_add_batch_dev(arec, o1, st, stream=s)))
            assert int(st.max()) == 0
            a["items_per_s"] = round(n / (a["median_ms"] * 1e-3))
            a["mad_fraction_of_peak"] = round(MADS["add"] * n / (a["median_ms"] * 1e-3) / PEAK_MADS, 4)
            out["add_%d" % n] = a
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("BN_G1_SWEEP " + json.dumps(out), flush=True)


def cpu_restatement(threads=16, per_thread=1500):
    """oracle.bn256_g1_mul on `threads` threads (the C call releases the GIL)"""
    import random
    import threading
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    rng = random.Random(5)
    pts = [O.bn256_g1_mul(rng.getrandbits(250)) for _ in range(64)]
    ks = [rng.getrandbits(256) for _ in range(per_thread)]

    def run():
        for i, k in enumerate(ks):
            O.bn256_g1_mul(k, pts[i & 63])

    ts = [threading.Thread(target=run) for _ in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    return {"what": "oracle.bn256_g1_mul (the CPU restatement, not the Go reference)", "threads": threads,
            "items": threads * per_thread, "items_per_s": round(threads * per_thread / dt)}


def main():
    if "--worker" in sys.argv:
        return worker()
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"bn_g1_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("BN_G1_SWEEP ")][-1]
    out = json.loads(line[len("BN_G1_SWEEP "):])
    if "--cpu" in sys.argv:
        out["cpu"] = cpu_restatement()
        out["gpu_over_cpu_mul"] = round(out["mul_%d" % N_BIG]["glv_items_per_s"] / out["cpu"]["items_per_s"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
