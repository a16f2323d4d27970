"""The receipt half of ValidateState through the device-resident entry points (gsv_receipts_bloom_dev,
gsv_derive_sha_batch_dev, gsv_receipts_check_dev), on one explicit stream, timed with HIP events, one process, one
GPU, ONE box, no counters collected and no trace made:

  1. spread   2,048 lists x 100 receipts x 2 logs x 3 topics (1,638,400 bloom items): the bloom part (scan, bloom,
              lists) as a whole, median over the steps, and each kernel by the context's per-kernel timers
  2. floor    the same number of items as 32-byte messages through k_keccak256, in the same run: one digest
              permutation per item is the floor for k_receipt_bloom; the ratio k_receipt_bloom / k_keccak256
  3. packed   the same items with all 200 logs of a list in ONE receipt: the ratio to (1) of the bloom kernel and of
              the bloom part (one lane per item, not per receipt, is there to keep it near 1)
  4. whole    gsv_receipts_verify_batch from host memory (copies included, wall clock) against the bloom part
              alone plus gsv_derive_sha_batch_dev alone plus the check, all on the device

Both shapes hold the same addresses and topics list by list, so their list blooms must be equal; four lists are
also checked against tests/receipt_model.py.  The GPU work runs in ONE child process under ONE time limit; a step
that faults or hangs ends the child, and nothing is started after it.  GPU box, repo root:
    python tools/receipt_sweep.py [--out profiles/receipts/sweep.json]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 20
GPU_TIME_LIMIT_S = 420
LISTS, RECEIPTS, LOGS, TOPICS = 2048, 100, 2, 3


def shape(items, receipts_per_list, logs_per_receipt):
    """items: (lists, logs per list, 20 + 32 TOPICS) random bytes, address || topics per log.  Every receipt has
    the same length: one template, the items' bytes written over their places.  Returns (flat, voff, list_off,
    the receipt's length)."""
    import numpy as np

    import receipt_model as R
    one = (bytes([0xAA]) * 20, [bytes([0xBB]) * 32] * TOPICS, bytes(36))
    blob = R.encode_receipt(R.new_receipt(gas=21000, logs=[one] * logs_per_receipt, bloom=bytes(256)))
    t = np.frombuffer(blob, np.uint8)
    # the logs are the receipt's tail, each log the same bytes: list head, 0x94 + address, list head, 0xa0 + topic ...
    enc = R.encode_log(one)
    topics_len = 33 * TOPICS
    topics_head = len(R.T.enc_list(bytes(topics_len))) - topics_len
    log_head = len(enc) - (21 + topics_head + topics_len + len(R.T.enc_string(one[2])))
    first = len(blob) - logs_per_receipt * len(enc)
    pos = []
    for j in range(logs_per_receipt):
        a = first + j * len(enc) + log_head + 1
        pos.append((a, [a + 20 + topics_head + 33 * k + 1 for k in range(TOPICS)]))
    assert all(blob[a:a + 20] == one[0] and all(blob[tp:tp + 32] == one[1][0] for tp in tps) for a, tps in pos)
    n = items.shape[0] * receipts_per_list
    flat = np.tile(t, (n, 1))
    view = items.reshape(n, logs_per_receipt, 20 + 32 * TOPICS)
    for j, (a, tps) in enumerate(pos):
        flat[:, a:a + 20] = view[:, j, :20]
        for k, tp in enumerate(tps):
            flat[:, tp:tp + 32] = view[:, j, 20 + 32 * k:52 + 32 * k]
    voff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(len(blob)))
    list_off = (np.arange(items.shape[0] + 1, dtype=np.uint64) * np.uint64(receipts_per_list))
    return flat.reshape(-1), voff, list_off, len(blob)


def worker():
    sys.path[:0] = [os.path.join(ROOT, "geth-sharding_amd"), os.path.join(ROOT, "tests"), ROOT]
    import ctypes

    import numpy as np
    import torch

    import gsv
    import receipt_model as R
    from gsv import _lib

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    rng = np.random.default_rng(0x5EED)
    per_list = RECEIPTS * LOGS
    items = rng.integers(0, 256, (LISTS, per_list, 20 + 32 * TOPICS), dtype=np.uint8)  # address || topics per log

    def tensors(flat, voff, list_off):
        n, nl = voff.size - 1, list_off.size - 1
        t = {"vals": torch.from_numpy(np.concatenate([flat, np.zeros(16, np.uint8)])).to(dev),
             "voff": torch.from_numpy(voff.view(np.int64)).to(dev),
             "loff": torch.from_numpy(list_off.view(np.int64)).to(dev),
             "work": torch.empty(gsv.receipts_work_bytes(n, flat.size), dtype=torch.uint8, device=dev),
             "rst": torch.zeros(n, dtype=torch.uint8, device=dev),
             "bloom": torch.zeros((nl, 256), dtype=torch.uint8, device=dev),
             "root": torch.zeros((nl, 32), dtype=torch.uint8, device=dev),
             "gas": torch.zeros(nl, dtype=torch.int64, device=dev),
             "lst": torch.zeros(nl, dtype=torch.uint8, device=dev), "st": torch.zeros(nl, dtype=torch.uint8, device=dev)}
        return t, n, nl, int(flat.size)

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

    n_items = LISTS * per_list * (1 + TOPICS)
    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1, "boxes": 1,
           "timing": "HIP events on one stream, one process, no counters collected, no trace made",
           "lists": LISTS, "bloom_items": n_items}
    blooms = {}
    for name, rpl, lpr in (("spread", RECEIPTS, LOGS), ("packed", 1, per_list)):
        flat, voff, list_off, rlen = shape(items, rpl, lpr)
        t, n, nl, nbytes = tensors(flat, voff, list_off)
        torch.cuda.synchronize()

        def bloom_part():
            ctx.receipts_bloom_dev(t["vals"], t["voff"], n, t["loff"], nl, nbytes, t["work"], t["rst"], None, t["bloom"],
                                   t["gas"], t["lst"], stream=s)

        row = {"receipts": n, "receipt_bytes": rlen, "rlp_bytes": nbytes, "slots": nbytes // 21 + 1,
               "bloom_part": median(bloom_part)}
        ctx.set_timing(True)
        ctx.reset_timing()
        for _ in range(STEPS):
            bloom_part()
        s.synchronize()
        for kname, kid in (("k_receipt_scan", _lib.K_RECEIPT_SCAN), ("k_receipt_bloom", _lib.K_RECEIPT_BLOOM),
                           ("k_receipt_lists", _lib.K_RECEIPT_LISTS)):
            ms, launches = ctx.kernel_time(kid)
            assert launches == STEPS
            row[kname] = {"mean_ms": round(ms / launches, 4)}
        ctx.set_timing(False)
        ctx.reset_timing()
        row["k_receipt_bloom"]["items_per_s"] = round(n_items / (row["k_receipt_bloom"]["mean_ms"] * 1e-3))
        assert not t["rst"].cpu().numpy().any() and not t["lst"].cpu().numpy().any()
        blooms[name] = t["bloom"].cpu().numpy()
        out[name] = row
        print("RECEIPT_SWEEP_STEP", name, row, flush=True)
        if name == "spread":
            # 4. the whole of it: the device chain's parts, then the host form from host memory
            ctx.derive_sha_prepare(voff, list_off)

            def derive():
                ctx.derive_sha_batch_dev(t["vals"], voff, list_off, t["root"], stream=s, prepare=False)

            def check():
                ctx.receipts_check_dev(t["lst"], t["bloom"], t["root"], t["gas"], None, None, None, nl, t["st"], stream=s)

            def chain():
                bloom_part()
                derive()
                check()

            whole = {"derive_sha_alone": median(derive), "check_alone": median(check), "device_chain": median(chain)}
            L = _lib.load()
            st = np.zeros(nl, np.uint8)
            hb = np.zeros((nl, 256), np.uint8)
            hr = np.zeros((nl, 32), np.uint8)
            p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
            hflat = np.concatenate([flat, np.zeros(16, np.uint8)])
            wall = []
            for _ in range(WARMUP + 5):
                t0 = time.perf_counter()
                rc = L.gsv_receipts_verify_batch(ctx.handle, p(hflat), p(voff), p(list_off), nl, None, None, None, None,
                                                 p(hb), p(hr), None, p(st))
                wall.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            wall = sorted(wall[WARMUP:])
            whole["host_form_wall_ms"] = {"median_ms": round(wall[len(wall) // 2], 3), "min_ms": round(wall[0], 3),
                                          "runs": len(wall)}
            assert not st.any() and (hb == blooms["spread"]).all() and (hr == t["root"].cpu().numpy()).all()
            whole["bloom_part_plus_derive_ms"] = round(row["bloom_part"]["median_ms"] +
                                                       whole["derive_sha_alone"]["median_ms"], 4)
            whole["device_chain_over_parts"] = round(whole["device_chain"]["median_ms"] /
                                                     (whole["bloom_part_plus_derive_ms"] +
                                                      whole["check_alone"]["median_ms"]), 4)
            out["whole"] = whole
            print("RECEIPT_SWEEP_STEP whole", whole, flush=True)
            # four lists against the model
            for k in (0, 1, LISTS // 2, LISTS - 1):
                want = 0
                for row_k in items[k]:
                    want |= R.bloom9(row_k[:20].tobytes())
                    for x in range(TOPICS):
                        want |= R.bloom9(row_k[20 + 32 * x:52 + 32 * x].tobytes())
                assert blooms["spread"][k].tobytes() == R.to_bloom(want), k
        del t
    assert (blooms["spread"] == blooms["packed"]).all()

    # 2. the floor: the same number of 32-byte messages through k_keccak256
    msgs = torch.from_numpy(rng.integers(0, 256, n_items * 32 + 16, dtype=np.uint8)).to(dev)
    moff = torch.arange(0, (n_items + 1) * 32, 32, dtype=torch.int64, device=dev)
    mout = torch.empty((n_items, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out["k_keccak256_32B"] = median(lambda: ctx.keccak256_batch_dev(msgs, moff, mout, stream=s))
    out["k_keccak256_32B"]["items_per_s"] = round(n_items / (out["k_keccak256_32B"]["median_ms"] * 1e-3))
    out["bloom_kernel_over_keccak"] = round(out["spread"]["k_receipt_bloom"]["mean_ms"] /
                                            out["k_keccak256_32B"]["median_ms"], 4)
    out["packed_over_spread_bloom_kernel"] = round(out["packed"]["k_receipt_bloom"]["mean_ms"] /
                                                   out["spread"]["k_receipt_bloom"]["mean_ms"], 4)
    out["packed_over_spread_bloom_part"] = round(out["packed"]["bloom_part"]["median_ms"] /
                                                 out["spread"]["bloom_part"]["median_ms"], 4)
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("RECEIPT_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"receipt_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RECEIPT_SWEEP ")][-1]
    out = json.loads(line[len("RECEIPT_SWEEP "):])
    out["not_measured"] = "one box only; no PMC counters, no traces, one GPU; receipts with a per-receipt bloom row " \
                          "asked for; lists that hold a failed receipt"
    txt = json.dumps(out, indent=1)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
