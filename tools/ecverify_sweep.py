"""ECDSA verification with a known key against public-key recovery on the same signatures, through the
device-resident entry points (gsv_ecdsa_verify_batch_dev, gsv_ecrecover_batch_dev): three legs
interleaved in one process on one explicit stream, timed with HIP events (warmup 3, 20 steps), at
n = 8,192 and n = 2^20:

    verify_uncompressed   65-byte keys (04 || X || Y): no square root
    verify_compressed     33-byte keys (02|03 || X): one square root per item in the key parse
    recover               k_ecrecover with its key and address outputs, as bench.py times it
    recover_pub_only      the same kernel without the address (no Keccak), for information

The inputs are made on the device by gsv_synth_sign_dev: msg32, the first 64 bytes of each sig65 row
repacked, and pub65 (the compressed rows are cut from it on the device).  Every run checks that all
items verify and recover.  Writes profiles/verify/sweep.json (--out PATH for another place) with the
per-item times and the two verify / recover ratios, and prints the same JSON line.

No CPU baseline of the reference's verify is given: the reference build the tests compare against
exports recovery, signing and key derivation only, not secp256k1_ext_ecdsa_verify.

The GPU work runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/ecverify_sweep.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 20
SIZES = (8192, 1 << 20)
GPU_TIME_LIMIT_S = 240
LEGS = ("verify_uncompressed", "verify_compressed", "recover", "recover_pub_only")


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

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device),
           "cpu_baseline": "none: the reference build used by the tests does not export its verify"}
    for n in SIZES:
        msg, sig65, pub = u8(n, 32), u8(n, 65), u8(n, 65)
        torch.cuda.synchronize()
        ctx.synth_sign_dev(7 + n, msg, sig65, pub, None, stream=s)
        with torch.cuda.stream(s):
            sig64 = sig65[:, :64].contiguous()
            comp = torch.zeros((n, 65), dtype=torch.uint8, device=dev)
            comp[:, 0] = (pub[:, 64] & 1) | 2
            comp[:, 1:33] = pub[:, 1:33]
            len65 = torch.full((n,), 65, dtype=torch.uint8, device=dev)
            len33 = torch.full((n,), 33, dtype=torch.uint8, device=dev)
        ok_u, ok_c, st = u8(n), u8(n), u8(n)
        rpub, raddr = u8(n, 65), u8(n, 20)
        s.synchronize()
        fns = {
            "verify_uncompressed": lambda: ctx.ecdsa_verify_batch_dev(msg, sig64, pub, len65, ok_u, stream=s),
            "verify_compressed": lambda: ctx.ecdsa_verify_batch_dev(msg, sig64, comp, len33, ok_c, stream=s),
            "recover": lambda: ctx.ecrecover_batch_dev(msg, sig65, rpub, raddr, st, stream=s),
            "recover_pub_only": lambda: ctx.ecrecover_batch_dev(msg, sig65, rpub, None, st, stream=s),
        }
        r = {"n": n}
        for rnd in ("", "_2"):  # two interleaved rounds: A, B, C, D, A, B, C, D
            for leg in LEGS:
                r[leg + rnd] = timed(fns[leg])
        assert int(ok_u.min()) == 1 and int(ok_c.min()) == 1, "a valid signature did not verify"
        assert int(st.max()) == 0 and torch.equal(rpub, pub), "recovery did not return the signer's key"
        t = {leg: min(r[leg]["median_ms"], r[leg + "_2"]["median_ms"]) * 1e-3 for leg in LEGS}
        for leg in LEGS:
            r[leg + "_ns_per_item"] = round(t[leg] / n * 1e9, 3)
            r[leg + "_items_per_s"] = round(n / t[leg])
        r["ratio_verify_uncompressed_over_recover"] = round(t["verify_uncompressed"] / t["recover"], 4)
        r["ratio_verify_compressed_over_recover"] = round(t["verify_compressed"] / t["recover"], 4)
        r["ratio_verify_uncompressed_over_recover_pub_only"] = round(t["verify_uncompressed"] / t["recover_pub_only"], 4)
        out["n_%d" % n] = r
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ECVERIFY_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    dest = os.path.join(ROOT, "profiles", "verify", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ecverify_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ECVERIFY_SWEEP ")][-1]
    out = json.loads(line[len("ECVERIFY_SWEEP "):])
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
