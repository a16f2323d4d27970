"""modexp precompile batch rates through the device-resident entry point (gsv_modexp_batch_dev) on one explicit
stream, timed with HIP events (warmup 2, 10 steps), one process, no counters:

    (32, 32, 32)      random 256-bit exponents, 2^20 rows
    (256, 3, 256)     e = 65537 (the RSA shape), 2^17 rows
    (128, 128, 128)   random 1024-bit exponents, 2^16 rows
    (1024, 3, 1024)   e = 65537 (nagydani-5 pow0x10001's shape), 2^16 rows

Moduli are random, odd, with the top bit set; bases random.  Per shape: rows/s, the 32x32 products a row needs
by the algorithm (its own bits) and the products its wave issues (a wave multiplies where ANY of its 64 lanes has
the bit set), the issued products' fraction of the v_mad_u64_u32 peak, and setup's share: the time of the same rows
with e = 1 (setup, base conversion, final conversion, load and store; no step of the walk) over the shape's time.
The first 48 rows of every shape are checked against Python's pow.

The GPU work runs in ONE child process under its own time limit; the parent only starts it and, with --cpu,
times Python's pow (the model; not the reference's big.Int.Exp) on 16 processes over rows of the same shapes.
--only32 runs the first shape alone (the A/B of the exponent walk: run once per library, GSV_LIB_PATH).
GPU box, repo root:
    python tools/modexp_sweep.py [--cpu] [--only32]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 2, 10
GPU_TIME_LIMIT_S = 300
PEAK_MADS = 39.32e12  # v_mad_u64_u32 per second, the VALU peak of README.md / DESIGN.md
SHAPES = [((32, 32, 32), 1 << 20, "random"), ((256, 3, 256), 1 << 17, "f4"), ((128, 128, 128), 1 << 16, "random"),
          ((1024, 3, 1024), 1 << 16, "f4")]


def limbs_of(ml):
    L = 8
    while 4 * L < ml:
        L *= 2
    return L


def rows_of(rng, n, shape, kind):
    """(n, bl + el + ml) uint8 rows and the exponents' bits as an (n, 8 el) array, most significant first"""
    import numpy as np
    bl, el, ml = shape
    rows = rng.integers(0, 256, (n, bl + el + ml), dtype=np.uint8)
    if kind == "f4":
        rows[:, bl:bl + el] = np.frombuffer((65537).to_bytes(el, "big"), np.uint8)
    elif kind == "one":
        rows[:, bl:bl + el] = np.frombuffer((1).to_bytes(el, "big"), np.uint8)
    else:
        rows[:, bl] |= 0x80
    rows[:, bl + el] |= 0x80
    rows[:, -1] |= 1
    return rows, np.unpackbits(rows[:, bl:bl + el], axis=1)


def products(shape, bits):
    """32x32 products per row: by its own exponent, and as its wave issues them.  A Montgomery product is
    2 L^2 of them; log2(L) squarings make R^2, one product converts the base (three per further L-limb piece),
    one converts back."""
    import numpy as np
    bl, el, ml = shape
    L = limbs_of(ml)
    pieces = max(1, -(-bl // (4 * L)))
    fixed = (L.bit_length() - 1) + 1 + 3 * (pieces - 1) + 1
    n, nb = bits.shape
    top = nb - bits.argmax(axis=1)  # bit length (every exponent here is non-zero)
    own = (top - 1) + (bits.sum(axis=1) - 1)
    w = bits[: n // 64 * 64].reshape(n // 64, 64, nb)
    wtop = nb - w.any(axis=1).argmax(axis=1)
    issued = (wtop - 1) + (w.any(axis=1).sum(axis=1) - 1)
    return {"limbs": L, "products_per_montgomery": 2 * L * L,
            "products_per_row": round(float((own.mean() + fixed) * 2 * L * L), 1),
            "products_issued_per_row": round(float((issued.mean() + fixed) * 2 * L * L), 1)}


def worker(only32):
    sys.path.insert(0, os.path.join(ROOT, "geth-sharding_amd"))
    import numpy as np
    import torch

    import gsv

    ctx = gsv.default_context()
    dev = torch.device("cuda", ctx.device)
    (s,) = ctx.pipeline_streams(1)
    rng = np.random.default_rng(198)

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

    out = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(ctx.device),
           "library": os.environ.get("GSV_LIB_PATH", "in-tree"), "shapes": {}}
    for shape, n, kind in SHAPES[:1] if only32 else SHAPES:
        bl, el, ml = shape
        rows, bits = rows_of(rng, n, shape, kind)
        rows1, _ = rows_of(rng, n, shape, "one")
        d_in, d_in1 = torch.from_numpy(rows).to(dev), torch.from_numpy(rows1).to(dev)
        d_out = torch.empty((n, ml), dtype=torch.uint8, device=dev)
        wb = gsv.modexp_work_bytes(n, bl, el, ml)
        d_work = torch.empty((wb,), dtype=torch.uint8, device=dev) if wb else None
        torch.cuda.synchronize()
        r = {"n": n, "work_bytes": wb}
        r.update(timed(lambda: ctx.modexp_batch_dev(d_in, bl, el, ml, d_out, d_work, stream=s)))
        got = d_out[:48].cpu().numpy()
        for i in range(48):
            b, e, m = (int.from_bytes(rows[i, a:z].tobytes(), "big") for a, z in
                       ((0, bl), (bl, bl + el), (bl + el, bl + el + ml)))
            assert got[i].tobytes() == pow(b, e, m).to_bytes(ml, "big"), (shape, i)
        r["setup_only"] = timed(lambda: ctx.modexp_batch_dev(d_in1, bl, el, ml, d_out, d_work, stream=s))
        t = r["median_ms"] * 1e-3
        r["rows_per_s"] = round(n / t)
        r.update(products(shape, bits))
        r["issued_fraction_of_peak"] = round(r["products_issued_per_row"] * n / t / PEAK_MADS, 4)
        r["setup_share_of_time"] = round(r["setup_only"]["median_ms"] / r["median_ms"], 4)
        out["shapes"]["%d/%d/%d" % shape] = r
        del d_in, d_in1, d_out, d_work
    torch.cuda.synchronize()
    ctx.destroy_streams([s])
    print("MODEXP_SWEEP " + json.dumps(out), flush=True)


def _pow_rows(args):
    shape, kind, count, seed = args
    import numpy as np
    bl, el, ml = shape
    rows, _ = rows_of(np.random.default_rng(seed), count, shape, kind)
    ops = [tuple(int.from_bytes(r[a:z].tobytes(), "big") for a, z in ((0, bl), (bl, bl + el), (bl + el, bl + el + ml)))
           for r in rows]
    t0 = time.perf_counter()
    for b, e, m in ops:
        pow(b, e, m)
    return time.perf_counter() - t0


def cpu_model(procs=16):
    """Python's pow on `procs` processes: rows/s = rows / the slowest process's time"""
    import multiprocessing as mp
    out = {"what": "Python's pow(b, e, m) (the model, not the reference's big.Int.Exp)", "processes": procs}
    with mp.Pool(procs) as pool:
        for shape, _, kind in SHAPES:
            count = 4000 if shape[2] <= 32 else 400
            dts = pool.map(_pow_rows, [(shape, kind, count, 7 + i) for i in range(procs)])
            out["%d/%d/%d" % shape] = {"rows": procs * count, "rows_per_s": round(procs * count / max(dts))}
    return out


def main():
    if "--worker" in sys.argv:
        return worker("--only32" in sys.argv)
    cmd = ["timeout", "-k", "10", str(GPU_TIME_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    if "--only32" in sys.argv:
        cmd.append("--only32")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.exit(f"modexp_sweep: the GPU step ended with status {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MODEXP_SWEEP ")][-1]
    out = json.loads(line[len("MODEXP_SWEEP "):])
    if "--cpu" in sys.argv:
        out["cpu"] = cpu_model()
        for k, v in out["shapes"].items():
            v["gpu_over_cpu_model"] = round(v["rows_per_s"] / out["cpu"][k]["rows_per_s"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
