"""ScalarMult and ECDH against verification and recovery, through the device-resident entry points
(gsv_secp256k1_scalar_mul_batch_dev, gsv_ecdh_batch_dev, gsv_ecdsa_verify_batch_dev,
gsv_ecrecover_batch_dev): five legs interleaved in one process on one explicit stream, timed with HIP
events (warmup 3, 20 steps; median / min / max), at n = 8,192 and n = 2^20.  Every leg is run twice in the
run (A, B, C, D, E, A, B, C, D, E), so the A/A spread of each is visible beside the ratios.

    scalar_mul            k_ecdh writing X || Y
    ecdh_x                k_ecdh writing the shared X alone (no Y product)
    ecdh_keys             k_ecdh writing the ECIES keys Ke || Km alone (two SHA-256 compressions more)
    verify_uncompressed   k_ecverify on 65-byte keys, the yardstick: the same ladder plus the comb, the
                          final add and an inversion mod n, minus k_ecdh's constant-time inversion mod p
    recover               k_ecrecover with its key and address outputs, as bench.py times it

The inputs are made on the device by gsv_synth_sign_dev: its public keys are the points, its message
hashes the scalars (a hash is >= n with probability 2^-128).  Every run checks that all items succeed,
that the three k_ecdh legs agree on X, and that the keys of the first 64 items are hashlib's.

CPU baseline: the reference's secp256k1_ext_scalar_mul (the reference build the tests compare against),
16,384 multiplications over 16 threads (ctypes releases the GIL), run in the parent before the GPU step.

Writes profiles/ecdh/sweep.json (--out PATH for another place) and prints the same JSON line.  The GPU
work runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/ecdh_sweep.py
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 20
SIZES = (8192, 1 << 20)
GPU_TIME_LIMIT_S = 240
LEGS = ("scalar_mul", "ecdh_x", "ecdh_keys", "verify_uncompressed", "recover")
CPU_ITEMS, CPU_THREADS = 16384, 16


def worker():
    import hashlib

    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import torch

    import gsv

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

    def u8(*shape):
        return torch.empty(shape, dtype=torch.uint8, device=dev)

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device)}
    for n in SIZES:
        msg, sig65, pub = u8(n, 32), u8(n, 65), u8(n, 65)
        torch.cuda.synchronize()
        ctx.synth_sign_dev(11 + n, msg, sig65, pub, None, stream=s)
        with torch.cuda.stream(s):
            sig64 = sig65[:, :64].contiguous()
            pts = pub[:, 1:].contiguous()
            len65 = torch.full((n,), 65, dtype=torch.uint8, device=dev)
        xy, st_m = u8(n, 64), u8(n)
        shared, st_x = u8(n, 32), u8(n)
        keys, st_k = u8(n, 48), u8(n)
        ok_u, st_r = u8(n), u8(n)
        rpub, raddr = u8(n, 65), u8(n, 20)
        s.synchronize()
        fns = {
            "scalar_mul": lambda: ctx.secp256k1_scalar_mul_batch_dev(pts, msg, xy, st_m, stream=s),
            "ecdh_x": lambda: ctx.ecdh_batch_dev(pts, msg, shared, None, st_x, stream=s),
            "ecdh_keys": lambda: ctx.ecdh_batch_dev(pts, msg, None, keys, st_k, stream=s),
            "verify_uncompressed": lambda: ctx.ecdsa_verify_batch_dev(msg, sig64, pub, len65, ok_u, stream=s),
            "recover": lambda: ctx.ecrecover_batch_dev(msg, sig65, rpub, raddr, st_r, stream=s),
        }
        r = {"n": n}
        for rnd in ("", "_2"):  # two interleaved rounds
            for leg in LEGS:
                r[leg + rnd] = timed(fns[leg])
        assert int(st_m.max()) == 0 and int(st_x.max()) == 0 and int(st_k.max()) == 0, "an item failed"
        assert torch.equal(xy[:, :32], shared), "scalar_mul and ecdh disagree on X"
        assert int(ok_u.min()) == 1 and int(st_r.max()) == 0 and torch.equal(rpub, pub)
        hx, hk = shared[:64].cpu().numpy(), keys[:64].cpu().numpy()
        for i in range(64):
            k = hashlib.sha256(b"\x00\x00\x00\x01" + bytes(hx[i])).digest()
            assert bytes(hk[i]) == k[:16] + hashlib.sha256(k[16:]).digest(), "derived keys differ from hashlib's"
        t = {leg: min(r[leg]["median_ms"], r[leg + "_2"]["median_ms"]) * 1e-3 for leg in LEGS}
        for leg in LEGS:
            r[leg + "_ns_per_item"] = round(t[leg] / n * 1e9, 3)
            r[leg + "_items_per_s"] = round(n / t[leg])
            a, b = r[leg]["median_ms"], r[leg + "_2"]["median_ms"]
            r[leg + "_aa_spread"] = round(abs(a - b) / min(a, b), 4)
        for leg in ("scalar_mul", "ecdh_x", "ecdh_keys"):
            r["ratio_%s_over_verify_uncompressed" % leg] = round(t[leg] / t["verify_uncompressed"], 4)
            r["ratio_%s_over_recover" % leg] = round(t[leg] / t["recover"], 4)
        out["n_%d" % n] = r
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ECDH_SWEEP " + json.dumps(out), flush=True)


def cpu_baseline():
    """the reference's secp256k1_ext_scalar_mul over CPU_THREADS threads, or a note that its build is absent"""
    import ctypes
    import random
    import threading

    sys.path.insert(0, ROOT)
    from oracle import oracle as O

    R = O.ref()
    if R is None:
        return {"note": "none: the reference build oracle/_ref is not here"}
    rng = random.Random(2024)
    g = bytes.fromhex("79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798"
                      "483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8")
    n_order = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    bufs, ks = [], []
    for _ in range(CPU_ITEMS):  # the points: the reference's own multiples of G
        b = ctypes.create_string_buffer(g, 64)
        assert R.secp256k1_ext_scalar_mul(None, b, rng.randrange(1, n_order).to_bytes(32, "big")) == 1
        bufs.append(b)
        ks.append(ctypes.create_string_buffer(rng.randrange(1, n_order).to_bytes(32, "big"), 32))
    bad = []

    def work(t):
        for i in range(t, CPU_ITEMS, CPU_THREADS):
            if R.secp256k1_ext_scalar_mul(None, bufs[i], ks[i]) != 1:
                bad.append(i)

    th = [threading.Thread(target=work, args=(t,)) for t in range(CPU_THREADS)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    assert not bad
    return {"what": "secp256k1_ext_scalar_mul of the reference build through ctypes", "items": CPU_ITEMS,
            "threads": CPU_THREADS, "cpus": os.cpu_count(), "seconds": round(dt, 4),
            "items_per_s": round(CPU_ITEMS / dt), "ns_per_item": round(dt / CPU_ITEMS * 1e9, 1)}


def main():
    if "--worker" in sys.argv:
        return worker()
    dest = os.path.join(ROOT, "profiles", "ecdh", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    cpu = cpu_baseline()
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ecdh_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ECDH_SWEEP ")][-1]
    out = json.loads(line[len("ECDH_SWEEP "):])
    out["cpu_baseline"] = cpu
    for n in SIZES:
        if "items_per_s" in cpu:
            out["n_%d" % n]["scalar_mul_speedup_over_cpu_baseline"] = round(
                out["n_%d" % n]["scalar_mul_items_per_s"] / cpu["items_per_s"], 1)
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
