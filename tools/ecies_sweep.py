"""ecies.Decrypt and Encrypt beside the key agreement alone, through the device-resident entry points
(gsv_ecies_decrypt_batch_dev, gsv_ecies_encrypt_batch_dev, gsv_ecdh_batch_dev with keys only: what the
library could do before the message half existed, and therefore the baseline), on one explicit stream from
gsv_stream_create, timed with HIP events (warmup 2, 8 steps; median / min / max), at n = 2^14, 2^17 and
2^20.  Every leg is run twice in the run (A, B, C, D, E, A, B, C, D, E), so the A/A spread of each is
visible beside the ratios.

    ecdh_keys        k_ecdh writing Ke || Km alone
    decrypt_194      Decrypt of 307-byte packets (the shape of RLPx's Auth1: a 194-byte message)
    encrypt_194      Encrypt of 194-byte messages
    decrypt_4096     Decrypt of 4 KiB messages
    encrypt_4096     Encrypt of 4 KiB messages

After the event-timed rounds each ECIES leg runs three more times with the context's kernel timing on:
gsv_ctx_kernel_time then gives the symmetric kernel's own time (GSV_K_ECIES) and the time of the
launches before it (GSV_K_ECRECOVER: the checks or eph G, and the ladder) apart.

The inputs are made on the device: random secret keys, their public keys by gsv_pubkey_create_batch_dev,
random ephemeral keys, IVs and messages; the ciphertexts Decrypt is timed on are Encrypt's.  Every run
checks that all items succeed, that Decrypt returns the messages Encrypt was given, and that the Python
model (tests/ecies_model.py) opens the first three ciphertexts of each shape to the same bytes.

Writes profiles/ecies/sweep.json (--out PATH for another place) and prints the same JSON line.  The GPU
work runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/ecies_sweep.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 8
SIZES = (1 << 14, 1 << 17, 1 << 20)
MSG_LENS = (194, 4096)
GPU_TIME_LIMIT_S = 420
OVERHEAD = 113


def worker():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import ecies_model as M
    import gsv
    from gsv import _lib

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

    def rnd(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device)}
    torch.manual_seed(20)
    for n in SIZES:
        with torch.cuda.stream(s):
            sk, eph, iv = rnd(n, 32), rnd(n, 32), rnd(n, 16)
            sk[:, 0] &= 0x7F  # below n for certain
            eph[:, 0] &= 0x7F
        pub65, st_p = u8(n, 65), u8(n)
        ctx.pubkey_create_batch_dev(sk, pub65, None, st_p, stream=s)
        with torch.cuda.stream(s):
            pub = pub65[:, 1:].contiguous()
        keys, st_k = u8(n, 48), u8(n)
        fns = {"ecdh_keys": lambda: ctx.ecdh_batch_dev(pub, eph, None, keys, st_k, stream=s)}
        shapes = {}
        for L in MSG_LENS:
            with torch.cuda.stream(s):
                msg = rnd(n * L)
                moff = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
                coff = torch.arange(n + 1, device=dev, dtype=torch.int64) * (L + OVERHEAD)
            ct, back = u8(n * (L + OVERHEAD)), u8(n * (L + OVERHEAD))
            st_e, st_d = u8(n), u8(n)
            mlen = torch.empty(n, dtype=torch.int32, device=dev)
            w_e, w_d = u8(gsv.ecies_work_bytes(n, True)), u8(gsv.ecies_work_bytes(n, False))
            shapes[L] = (msg, ct, back, st_e, st_d, mlen)
            fns["encrypt_%d" % L] = (lambda msg=msg, moff=moff, ct=ct, st_e=st_e, w_e=w_e:
                                     ctx.ecies_encrypt_batch_dev(msg, moff, pub, eph, iv, None, None, ct, st_e, w_e, stream=s))
            fns["decrypt_%d" % L] = (lambda ct=ct, coff=coff, back=back, mlen=mlen, st_d=st_d, w_d=w_d:
                                     ctx.ecies_decrypt_batch_dev(ct, coff, sk, None, None, back, mlen, st_d, w_d, stream=s))
            fns["encrypt_%d" % L]()  # the ciphertexts Decrypt is timed on
        s.synchronize()
        legs = ["ecdh_keys"] + ["%s_%d" % (d, L) for L in MSG_LENS for d in ("decrypt", "encrypt")]
        r = {"n": n}
        for tag in ("", "_2"):  # two interleaved rounds
            for leg in legs:
                r[leg + tag] = timed(fns[leg])
        # the kernels' own times
        ctx.set_timing(True)
        for leg in legs[1:]:
            ctx.reset_timing()
            for _ in range(3):
                fns[leg]()
            s.synchronize()
            sym_ms, k = ctx.kernel_time(_lib.K_ECIES)
            lad_ms, _ = ctx.kernel_time(_lib.K_ECRECOVER)
            assert k == 3
            r[leg + "_symmetric_kernel_ms"] = round(sym_ms / 3, 4)
            r[leg + "_launches_before_it_ms"] = round(lad_ms / 3, 4)
            r[leg + "_symmetric_over_ladder_side"] = round(sym_ms / lad_ms, 4)
        ctx.set_timing(False)
        ctx.reset_timing()
        # every item succeeded, Decrypt returns Encrypt's input, the model opens a sample
        assert int(st_p.max()) == 0 and int(st_k.max()) == 0, "a key failed"
        sk_h = sk[:3].cpu().numpy()
        for L in MSG_LENS:
            msg, ct, back, st_e, st_d, mlen = shapes[L]
            assert int(st_e.max()) == 0 and int(st_d.max()) == 0, "an item failed"
            assert int(mlen.min()) == L == int(mlen.max())
            assert torch.equal(back.view(n, L + OVERHEAD)[:, :L], msg.view(n, L)), "Decrypt(Encrypt(m)) != m"
            assert int(back.view(n, L + OVERHEAD)[:, L:].max()) == 0, "a slot's tail is not zero"
            ct_h, msg_h = ct.view(n, L + OVERHEAD)[:3].cpu().numpy(), msg.view(n, L)[:3].cpu().numpy()
            for i in range(3):
                assert M.decrypt(bytes(ct_h[i]), bytes(sk_h[i])) == (0, bytes(msg_h[i])), "the model disagrees"
        base = min(r["ecdh_keys"]["median_ms"], r["ecdh_keys_2"]["median_ms"])
        for leg in legs:
            a, b = r[leg]["median_ms"], r[leg + "_2"]["median_ms"]
            t = min(a, b) * 1e-3
            r[leg + "_ns_per_item"] = round(t / n * 1e9, 3)
            r[leg + "_items_per_s"] = round(n / t)
            r[leg + "_aa_spread"] = round(abs(a - b) / min(a, b), 4)
            if leg != "ecdh_keys":
                r["ratio_%s_over_ecdh_keys" % leg] = round(min(a, b) / base, 4)
                L = int(leg.split("_")[1])
                r[leg + "_message_bytes_per_s"] = round(n * L / t)
        out["n_%d" % n] = r
        del fns, shapes
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("ECIES_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    dest = os.path.join(ROOT, "profiles", "ecies", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"ecies_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ECIES_SWEEP ")][-1]
    out = json.loads(line[len("ECIES_SWEEP "):])
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
