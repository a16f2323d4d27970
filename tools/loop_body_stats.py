"""Per basic block of one kernel in a hipcc -S gfx950 assembly file: instructions, 64-bit multiply-adds
(v_mad_u64_u32 / v_mad_i64_i32), 64-bit shifts, other instructions, scratch stores / loads.  Blocks
below --min instructions are left out; the ladder's doubling and mixed-add bodies are the blocks of
about 870 and 1,600 instructions that repeat.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S ecrecover.hip -o ecrecover.s
    python tools/loop_body_stats.py ecrecover.s k_ecrecover [--min 400]
"""
import re
import sys


def main(path, kernel, floor):
    s = open(path).read()
    m = re.search(r"^(\S*" + re.escape(kernel) + r"E\S*):\s+; @", s, re.M)
    body = s[m.end():s.find("; -- End function", m.end())]
    blocks, name, cur = [], "entry", []
    for l in body.split("\n"):
        lab = re.match(r"^(\.LBB\S+):", l)
        if lab:
            blocks.append((name, cur))
            name, cur = lab.group(1), []
        elif l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;"):
            cur.append(l.split()[0])
    blocks.append((name, cur))
    tot = [0, 0, 0]
    for name, ops in blocks:
        mad = sum(o in ("v_mad_u64_u32", "v_mad_i64_i32") for o in ops)
        smad = sum(o == "v_mad_i64_i32" for o in ops)
        sh = sum(o in ("v_lshrrev_b64", "v_lshlrev_b64", "v_ashrrev_i64") for o in ops)
        tot = [tot[0] + len(ops), tot[1] + mad, tot[2] + sh]
        if len(ops) >= floor:
            print(f"{name:12s} inst={len(ops):5d} mad64={mad:5d} (signed {smad:3d}) shift64={sh:4d} "
                  f"other={len(ops) - mad - sh:5d} scratch_st={sum('scratch_store' in o for o in ops):3d} "
                  f"scratch_ld={sum('scratch_load' in o for o in ops):3d}")
    print(f"kernel       inst={tot[0]:5d} mad64={tot[1]:5d} shift64={tot[2]:4d}")


if __name__ == "__main__":
    a = sys.argv[1:]
    floor = int(a[a.index("--min") + 1]) if "--min" in a else 400
    main(a[0], a[1], floor)
