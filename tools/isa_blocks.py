"""The straight-line pieces of one kernel in a gfx950 -S listing (compile only, no GPU):

    hipcc <build flags> --cuda-device-only -S -o new.s shippingenv_amd/csrc/shipenv.hip
    python tools/isa_blocks.py new.s _ZN12_GLOBAL__N_115step_seq_kernelILb1EEEvNS_8StepArgsEil [first_line last_line]

A piece starts at a label or after a branch. Per piece: the listing line, the label ("+" after a
branch), instructions, VALU, of them the ~8-cycle ones (v_mad_u64_u32, the f64 conversions and
compares), LDS reads, SALU, then scratch / buffer accesses and v_readlane / v_writelane
(`bad`, which a step loop must not have), and the branch that ends the piece. Used to count what
a wave executes on each path through step_seq_kernel's state-only loop
(profiles/seq_guard/isa.json)."""
import re
import sys

SLOW = re.compile(r"^v_(mad_u64_u32|cvt_f64_\w+|cvt_\w+_f64|cmp_\w+_f64)")  # ~8 cycles per wave-instruction


def pieces(path, name):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    new = lambda label, line: {"label": label, "line": line + 1, "n": 0, "valu": 0, "slow": 0, "ds": 0,  # noqa: E731
                               "salu": 0, "bad": 0, "br": []}
    out, cur = [], new("entry", start)
    for i in range(start + 1, end):
        s = lines[i].split(";", 1)[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            out.append(cur)
            cur = new(m.group(1), i)
            continue
        if not s or s.startswith("."):
            continue
        op = s.split()[0]
        cur["n"] += 1
        if op.startswith("v_"):
            cur["valu"] += 1
            cur["slow"] += bool(SLOW.match(op))
            cur["bad"] += "readlane" in op or "writelane" in op
        elif op.startswith("ds_"):
            cur["ds"] += "read" in op or "load" in op
        elif op.startswith(("scratch_", "buffer_")):
            cur["bad"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
            if "branch" in op:
                cur["br"].append(op.replace("s_cbranch_", "").replace("s_branch", "jmp") + ">" + s.split()[-1])
                out.append(cur)
                cur = new("+", i + 1)
    out.append(cur)
    return [p for p in out if p["n"]]


if __name__ == "__main__":
    lo, hi = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, 1 << 60)
    for p in pieces(sys.argv[1], sys.argv[2]):
        if lo <= p["line"] <= hi:
            print(f"{p['line']:6d} {p['label']:12s} n={p['n']:4d} valu={p['valu']:4d} slow={p['slow']:3d} "
                  f"ds={p['ds']:2d} salu={p['salu']:3d} bad={p['bad']} {' '.join(p['br'])}")
