"""crypto.Sign and public-key derivation through the device-resident entry points
(gsv_ecdsa_sign_batch_dev, gsv_pubkey_create_batch_dev) against the synthetic signer
(gsv_synth_sign_dev) as the yardstick: three legs interleaved in one process on one explicit stream,
timed with HIP events (warmup 3, 20 steps), at n = 2^10, 2^16 and 2^20:

    sign           k_ecsign: 16 SHA-256 compressions (the RFC 6979 nonce), one comb multiplication, one
                   inversion mod p, one constant-time inversion mod n
    pubkey_create  k_pubkey_create with its address output: one comb multiplication, one inversion mod p,
                   one Keccak permutation
    synth_sign     k_synth_sign with its key and address outputs: three Keccak derivations, TWO comb
                   multiplications, two inversions mod p, the same inversion mod n, one more Keccak

Keys and messages are random bytes made on the device (a key of 0 or >= n has probability 2^-128).  Every
run checks that all items sign, that recovery of the signatures returns pubkey_create's keys, and that the
addresses agree.  The CPU baseline is the reference's own signer (gsvref_sign of the reference build,
when it is there) on 16 host threads over 2^16 items.  Writes profiles/sign/sweep.json (--out PATH for
another place) with the per-item times, signatures/s and the ratio to synth_sign, and prints the same
JSON line.

The GPU work runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/ecsign_sweep.py
"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 20
SIZES = (1 << 10, 1 << 16, 1 << 20)
GPU_TIME_LIMIT_S = 240
LEGS = ("sign", "pubkey_create", "synth_sign")
CPU_THREADS, CPU_ITEMS = 16, 1 << 16


def worker():
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(6979)
    for n in SIZES:
        with torch.cuda.stream(s):
            key = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
            msg = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        sig, st = u8(n, 65), u8(n)
        pub, addr, pst = u8(n, 65), u8(n, 20), u8(n)
        ymsg, ysig, ypub, yaddr = u8(n, 32), u8(n, 65), u8(n, 65), u8(n, 20)
        rpub, raddr, rst = u8(n, 65), u8(n, 20), u8(n)
        s.synchronize()
        fns = {
            "sign": lambda: ctx.ecdsa_sign_batch_dev(msg, key, sig, st, stream=s),
            "pubkey_create": lambda: ctx.pubkey_create_batch_dev(key, pub, addr, pst, stream=s),
            "synth_sign": lambda: ctx.synth_sign_dev(7 + n, ymsg, ysig, ypub, yaddr, stream=s),
        }
        r = {"n": n}
        for rnd in ("", "_2"):  # two interleaved rounds: A, B, C, A, B, C
            for leg in LEGS:
                r[leg + rnd] = timed(fns[leg])
        ctx.ecrecover_batch_dev(msg, sig, rpub, raddr, rst, stream=s)
        s.synchronize()
        assert int(st.max()) == 0 and int(pst.max()) == 0, "a random key did not sign"
        assert int(rst.max()) == 0 and torch.equal(rpub, pub) and torch.equal(raddr, addr), \
            "recovery of a signature did not return the signer's key"
        t = {leg: min(r[leg]["median_ms"], r[leg + "_2"]["median_ms"]) * 1e-3 for leg in LEGS}
        for leg in LEGS:
            r[leg + "_ns_per_item"] = round(t[leg] / n * 1e9, 3)
            r[leg + "_items_per_s"] = round(n / t[leg])
        r["ratio_sign_over_synth_sign"] = round(t["sign"] / t["synth_sign"], 4)
        r["ratio_pubkey_create_over_synth_sign"] = round(t["pubkey_create"] / t["synth_sign"], 4)
        out["n_%d" % n] = r
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ECSIGN_SWEEP " + json.dumps(out), flush=True)


def cpu_baseline():
    """the reference's signer on CPU_THREADS host threads (ctypes releases the GIL around each call)"""
    sys.path.insert(0, ROOT)
    from concurrent.futures import ThreadPoolExecutor

    from oracle import oracle as O
    R = O.ref()
    if R is None:
        return {"cpu_baseline": "none: the reference build (make -C oracle ref) is not here"}
    rnd = os.urandom(64 * CPU_ITEMS)
    keys = [b"\x01" + rnd[64 * i + 1:64 * i + 32] for i in range(CPU_ITEMS)]  # below n: top byte 01
    msgs = [rnd[64 * i + 32:64 * i + 64] for i in range(CPU_ITEMS)]

    def work(t):
        sig = ctypes.create_string_buffer(65)
        ok = 0
        for i in range(t, CPU_ITEMS, CPU_THREADS):
            ok += R.gsvref_sign(sig, msgs[i], keys[i])
        return ok

    work(0)  # warm: context tables, page faults
    t0 = time.perf_counter()
    with ThreadPoolExecutor(CPU_THREADS) as ex:
        done = sum(ex.map(work, range(CPU_THREADS)))
    dt = time.perf_counter() - t0
    assert done == CPU_ITEMS
    return {"cpu_baseline": {"what": "gsvref_sign (the reference's libsecp256k1, RFC 6979 nonce)",
                             "threads": CPU_THREADS, "host_cpus": os.cpu_count(), "n": CPU_ITEMS,
                             "seconds": round(dt, 4), "items_per_s": round(CPU_ITEMS / dt)}}


def main():
    if "--worker" in sys.argv:
        return worker()
    dest = os.path.join(ROOT, "profiles", "sign", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ecsign_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ECSIGN_SWEEP ")][-1]
    out = json.loads(line[len("ECSIGN_SWEEP "):])
    out.update(cpu_baseline())
    base = out["cpu_baseline"]
    if isinstance(base, dict):
        big = out["n_%d" % SIZES[-1]]
        out["gpu_over_cpu_threads"] = round(big["sign_items_per_s"] / base["items_per_s"], 1)
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
