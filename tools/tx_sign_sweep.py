"""types.SignTx through the device-resident entry point (gsv_tx_sign_batch_dev) on the notary benchmark's
transaction shape: the synthetic collations' transactions (gsv_notary_synth_dev: EIP-155, chain id 1,
102-104 bytes of RLP each) unpacked from their blobs on the device and signed again with fresh random keys,
at n = 2^20 and n = 8,192, device-resident, one explicit stream, HIP events (warmup 3, 20 steps).

    whole call     the three launches of gsv_tx_sign_batch_dev, events around the call
    k_tx_sighash   its own events inside the call (gsv_ctx_kernel_time, GSV_K_TX_SIGHASH)
    k_ecsign       likewise (GSV_K_ECRECOVER)
    k_tx_seal      likewise (GSV_K_TX_SEAL)
    ecsign alone   gsv_ecdsa_sign_batch_dev over the same hashes and keys in the same run: the yardstick, what
                   the library could do before this call existed

The per-launch times come from a second pass with the context's timing on (it brackets every launch with
events, which costs the whole call a little: the whole-call figure is taken with timing off).  Legs are
interleaved in two rounds.  Every run checks that all items sign and, for the first 512, that
gsv_tx_sender_batch returns the address of the signing key.  No counters: one box, one run.  Writes
profiles/txsign/sweep.json (--out PATH for another place) and prints the same JSON line.

The GPU work runs in ONE child process under its own time limit (`timeout -k 10`).  GPU box, repo root:
    python tools/tx_sign_sweep.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 20
SIZES = (1 << 20, 8192)
PER_SHARD = 8192
GPU_TIME_LIMIT_S = 300
CHECKED = 512


def worker():
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import numpy as np
    import torch

    import gsv
    from gsv import _lib

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    G = _lib.tx_sign_growth(1)

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

    def per_launch(fn):
        """ms per launch of each kernel id over STEPS calls with the context's timing on"""
        ctx.set_timing(True)
        try:
            fn()
            s.synchronize()
            ctx.reset_timing()
            for _ in range(STEPS):
                fn()
            s.synchronize()
            out = {}
            for name, kid in (("k_tx_sighash", _lib.K_TX_SIGHASH), ("k_ecsign", _lib.K_ECRECOVER),
                              ("k_tx_seal", _lib.K_TX_SEAL)):
                ms, launches = ctx.kernel_time(kid)
                assert launches == STEPS, (name, launches)
                out[name + "_ms"] = round(ms / launches, 4)
            return out
        finally:
            ctx.set_timing(False)
            ctx.reset_timing()

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device),
           "workload": "gsv_notary_synth_dev transactions (EIP-155, chain id 1), signed again with random keys",
           "yardstick": "gsv_ecdsa_sign_batch_dev (k_ecsign alone) over the same hashes and keys, same run",
           "counters": "none: one box, HIP events only"}
    gen = torch.Generator(device=dev)
    gen.manual_seed(155)
    for n in SIZES:
        shards = n // PER_SHARD
        bodies = torch.zeros((n * 128,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.notary_synth_dev(2024, 0, shards, PER_SHARD, bodies, stream=s)
        s.synchronize()
        with torch.cuda.stream(s):
            # the blob codec undone: four chunks per transaction, 31 data bytes behind each indicator; the
            # last indicator is the terminal length
            c = bodies.view(n, 4, 32)
            lens = 93 + (c[:, 3, 0] & 0x1F).to(torch.int64)
            data = c[:, :, 1:].reshape(n, 124)
            keep = torch.arange(124, device=dev)[None, :] < lens[:, None]
            rlp = torch.cat([data[keep], torch.zeros(8, dtype=torch.uint8, device=dev)])
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            off[1:] = torch.cumsum(lens, 0)
            key = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
            key[:, 0] = 1  # below the group order, never 0
        s.synchronize()
        total = int(off[n])
        sig_out = torch.zeros(total + n * G, dtype=torch.uint8, device=dev)
        olen = torch.zeros(n, dtype=torch.int32, device=dev)
        h = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        st = torch.zeros(n, dtype=torch.uint8, device=dev)
        work = torch.zeros(gsv.tx_sign_work_bytes(n), dtype=torch.uint8, device=dev)
        msg = work[16 * n:48 * n].view(n, 32)  # the hashes k_tx_sighash leaves in the work area
        ysig = torch.zeros((n, 65), dtype=torch.uint8, device=dev)
        yst = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fns = {
            "whole_call": lambda: ctx.tx_sign_batch_dev(rlp, off, key, 1, _lib.SIGNER_EIP155, sig_out, olen, h, st, work,
                                                        stream=s),
            "ecsign_alone": lambda: ctx.ecdsa_sign_batch_dev(msg, key, ysig, yst, stream=s),
        }
        lmin, lmax = int(lens.min()), int(lens.max())
        r = {"n": n, "tx_bytes_min": lmin, "tx_bytes_max": lmax}
        for rnd in ("", "_2"):  # two interleaved rounds
            for leg in fns:
                r[leg + rnd] = timed(fns[leg])
        r["per_launch"] = per_launch(fns["whole_call"])
        s.synchronize()
        assert int(st.max()) == 0 and int(yst.max()) == 0, "an item did not sign"
        assert torch.equal(ysig, work[48 * n:113 * n].view(n, 65)), "the two signature runs differ"
        # the first CHECKED outputs through types.Sender
        k = min(CHECKED, n)
        o, ln, o_h = off[:k + 1].cpu().numpy(), olen[:k].cpu().numpy(), sig_out[:int(off[k]) + k * G].cpu().numpy()
        signed = [o_h[int(o[i]) + i * G:int(o[i]) + i * G + int(ln[i])].tobytes() for i in range(k)]
        _, addr, _ = ctx.pubkey_create_batch(key[:k].cpu().numpy(), want_addr=True)
        got, sst = ctx.tx_sender_batch(signed, 1, _lib.SIGNER_EIP155)
        assert (sst == 0).all() and (got == addr).all(), "types.Sender did not return the signing key's address"
        t = {leg: min(r[leg]["median_ms"], r[leg + "_2"]["median_ms"]) for leg in fns}
        r["whole_call_ms"], r["ecsign_alone_ms"] = t["whole_call"], t["ecsign_alone"]
        r["signed_txs_per_s"] = round(n / (t["whole_call"] * 1e-3))
        r["ecsign_alone_sigs_per_s"] = round(n / (t["ecsign_alone"] * 1e-3))
        r["ratio_whole_call_over_ecsign_alone"] = round(t["whole_call"] / t["ecsign_alone"], 4)
        pl = r["per_launch"]
        r["new_kernels_over_k_ecsign"] = round((pl["k_tx_sighash_ms"] + pl["k_tx_seal_ms"]) / pl["k_ecsign_ms"], 4)
        out["n_%d" % n] = r
        del bodies, rlp, sig_out, work
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("TX_SIGN_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    dest = os.path.join(ROOT, "profiles", "txsign", "sweep.json")
    if "--out" in sys.argv:
        dest = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    p = subprocess.run(["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__),
                        "--worker"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"tx_sign_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("TX_SIGN_SWEEP ")][-1]
    out = json.loads(line[len("TX_SIGN_SWEEP "):])
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
