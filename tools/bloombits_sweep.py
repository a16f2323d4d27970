"""The bloombits family through its device-resident entry points, on one explicit stream, timed with HIP events, one
process, one GPU, ONE box, no counters collected and no trace made:

  1. generator  256 sections of 4,096 blooms (256 MiB in, 256 MiB out: past the Infinity Cache) against a
                device-to-device copy of 256 MiB in the same run; the ratio of the two rates of bytes moved
  2. compress   the 524,288 vectors of 512 bytes of that table (blooms of bit density 1/50), and decompress of its
                output, beside the generator's time; how many vectors came out empty, raw and encoded
  3. matcher    1,024 queries of three rules by two clauses over 1,221 sections of 4,096 (5 M blocks): the match launch
                and the three launches of blocks_dev; time per query and the rate of row bytes read (18 rows of 512
                bytes per query and section; the rows of bits that several queries share stay in cache), over blooms
                of bit density 1/4 so that the queries have matches to expand

Section 0 of the table is checked against tests/bloombits_model.py, and one query's blocks against the blooms.  The
GPU work runs in ONE child process under ONE time limit; a step that faults or hangs ends the child, and nothing is
started after it.  GPU box, repo root:
    python tools/bloombits_sweep.py [--out profiles/bloombits/sweep.json]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 10
GPU_TIME_LIMIT_S = 420
S, GEN_SECTIONS = 4096, 256
QUERIES, RULES, CLAUSES, MATCH_SECTIONS = 1024, 3, 2, 1221


def worker():
    sys.path[:0] = [os.path.join(ROOT, "geth-sharding_amd"), os.path.join(ROOT, "tests"), ROOT]
    import numpy as np
    import torch

    import bloombits_model as M
    import gsv

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    rb = S // 8

    def median(fn, steps=STEPS):
        for _ in range(WARMUP):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record(s)
        for i in range(steps):
            fn()
            ev[i + 1].record(s)
        s.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
        return {"median_ms": round(ms[steps // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    def sparse_blooms(n, seed, dense=False):
        """n blooms of bit density about 1/50: the AND of six random bytes' bits is 1/64, plus a second draw; dense:
        1/4, so that three rules of two clauses of three bits still leave some blocks of 5 M"""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        a = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev, generator=g)
        if dense:
            return a & torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev, generator=g)
        for _ in range(5):
            a &= torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev, generator=g)
        b = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev, generator=g)
        for _ in range(7):
            b &= torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev, generator=g)
        return a | b

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device), "gpus": 1, "boxes": 1,
           "timing": "HIP events on one stream, one process, no counters collected, no trace made", "section_size": S}

    # 1. generator against a copy
    n_gen = GEN_SECTIONS * S
    blooms = sparse_blooms(n_gen, 1)
    table = torch.empty(GEN_SECTIONS * 2048 * rb, dtype=torch.uint8, device=dev)
    spare = torch.empty_like(table)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gen = median(lambda: ctx.bloombits_generate_dev(blooms, GEN_SECTIONS, S, table, stream=s))
        cp = median(lambda: spare.copy_(blooms.view(-1)))
    moved = 2 * blooms.numel()
    gen.update(sections=GEN_SECTIONS, bytes_in=blooms.numel(), bytes_out=table.numel(),
               GB_per_s=round(moved / gen["median_ms"] / 1e6, 1))
    cp.update(bytes=blooms.numel(), GB_per_s=round(moved / cp["median_ms"] / 1e6, 1))
    out["generator"], out["copy_d2d"] = gen, cp
    out["generator_over_copy_rate"] = round(gen["GB_per_s"] / cp["GB_per_s"], 4)
    want = M.generate_sections_np(blooms[:S].cpu().numpy(), S)
    assert (table[:2048 * rb].cpu().numpy().reshape(1, 2048, rb) == want).all()
    print("BLOOMBITS_SWEEP_STEP generator", gen, cp, flush=True)

    # 2. the codec over that table
    n_vec = GEN_SECTIONS * 2048
    slots = torch.empty(n_vec * rb, dtype=torch.uint8, device=dev)
    lens = torch.zeros(n_vec, dtype=torch.int32, device=dev)
    comp = median(lambda: ctx.bitset_compress_batch_dev(table, n_vec, rb, slots, lens, stream=s))
    ln = lens.cpu().numpy()
    comp.update(vectors=n_vec, vector_bytes=rb, empty=int((ln == 0).sum()), raw=int((ln == rb).sum()),
                encoded=int(((ln > 0) & (ln < rb)).sum()), compressed_bytes=int(ln.sum()),
                over_generator=round(comp["median_ms"] / gen["median_ms"], 3))
    for k in (0, 1, 2047, n_vec - 1):
        assert slots[k * rb:k * rb + int(ln[k])].cpu().numpy().tobytes() == \
            M.compress_bytes(table[k * rb:(k + 1) * rb].cpu().numpy().tobytes()), k
    # decompress takes an offset table: item k = its slot's first ln[k] bytes
    starts = torch.arange(0, n_vec, dtype=torch.int64, device=dev) * rb
    packed_off = torch.zeros(n_vec + 1, dtype=torch.int64, device=dev)
    packed_off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    packed = torch.empty(int(ln.sum()) + 8, dtype=torch.uint8, device=dev)
    idx = torch.repeat_interleave(starts - packed_off[:-1], lens.to(torch.int64)) + \
        torch.arange(0, int(ln.sum()), dtype=torch.int64, device=dev)
    packed[:int(ln.sum())] = slots[idx]
    del idx
    back = torch.empty(n_vec * rb, dtype=torch.uint8, device=dev)
    st = torch.zeros(n_vec, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dec = median(lambda: ctx.bitset_decompress_batch_dev(packed, packed_off, n_vec, rb, back, st, stream=s))
    assert not st.any().item() and torch.equal(back, table)
    dec["over_generator"] = round(dec["median_ms"] / gen["median_ms"], 3)
    out["compress"], out["decompress"] = comp, dec
    print("BLOOMBITS_SWEEP_STEP codec", comp, dec, flush=True)
    del slots, back, packed, spare, table, blooms

    # 3. the matcher
    ns = MATCH_SECTIONS
    blooms = sparse_blooms(ns * S, 2, dense=True)
    table = torch.empty(ns * 2048 * rb, dtype=torch.uint8, device=dev)
    ctx.bloombits_generate_dev(blooms, ns, S, table, stream=s)
    rng = np.random.default_rng(3)
    n_rules, n_clauses = QUERIES * RULES, QUERIES * RULES * CLAUSES
    cl = rng.integers(0, 2048, (n_clauses, 3), dtype=np.uint16)
    clauses = torch.from_numpy(cl.view(np.int16)).to(dev)
    rule_off = torch.arange(0, n_clauses + 1, CLAUSES, dtype=torch.int32, device=dev)
    query_off = torch.arange(0, n_rules + 1, RULES, dtype=torch.int32, device=dev)
    begin = torch.zeros(QUERIES, dtype=torch.int64, device=dev)
    end = torch.full((QUERIES,), ns * S - 1, dtype=torch.int64, device=dev)
    match = torch.empty(QUERIES * ns * rb, dtype=torch.uint8, device=dev)
    count = torch.zeros(QUERIES * ns, dtype=torch.int32, device=dev)
    block_off = torch.zeros(QUERIES + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def do_match():
        ctx.bloombits_match_dev(table, S, 0, ns, clauses, n_clauses, rule_off, n_rules, query_off, QUERIES, begin, end,
                                match, count, stream=s)
    m = median(do_match, 5)
    total = int(count.to(torch.int64).sum().item())
    blocks = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    b = median(lambda: ctx.bloombits_blocks_dev(match, count, S, 0, ns, QUERIES, block_off, blocks, total, stream=s), 5)
    row_bytes_read = QUERIES * ns * RULES * CLAUSES * 3 * rb
    m.update(queries=QUERIES, sections=ns, blocks=ns * S, us_per_query=round(m["median_ms"] * 1e3 / QUERIES, 3),
             row_bytes_read=row_bytes_read, row_GB_per_s=round(row_bytes_read / m["median_ms"] / 1e6, 1),
             table_bytes=table.numel(), match_bytes=match.numel(), matches=total)
    b.update(block_numbers=total, us_per_query=round(b["median_ms"] * 1e3 / QUERIES, 3))
    out["match"], out["blocks"] = m, b
    # one query against the blooms themselves
    q = 0
    bo = block_off.cpu().numpy()
    assert bo[-1] == total
    got = blocks[bo[q]:bo[q + 1]].cpu().numpy()
    hb = blooms.cpu().numpy()
    ok = np.ones(ns * S, bool)
    for r in range(RULES):
        anyc = np.zeros(ns * S, bool)
        for c in range(CLAUSES):
            v = np.ones(ns * S, bool)
            for bit in cl[(q * RULES + r) * CLAUSES + c]:
                v &= (hb[:, 255 - int(bit) // 8] >> (int(bit) % 8)) & 1 == 1
            anyc |= v
        ok &= anyc
    assert got.tolist() == np.flatnonzero(ok).tolist()
    print("BLOOMBITS_SWEEP_STEP matcher", m, b, flush=True)
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("BLOOMBITS_SWEEP " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"bloombits_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("BLOOMBITS_SWEEP ")][-1]
    out = json.loads(line[len("BLOOMBITS_SWEEP "):])
    out["not_measured"] = "one box only; no PMC counters, no traces, one GPU; section sizes other than 4,096; the " \
                          "host forms (copies included); tables at odd addresses (the byte-wise paths)"
    txt = json.dumps(out, indent=1)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
