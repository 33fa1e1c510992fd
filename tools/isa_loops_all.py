"""Spill traffic of a kernel by loop, nested loops included, and outside its time loops -- the sibling of tools/isa_loop_check.py, which
lists only INNERMOST loops and so misses a time loop whose steps contain a small backward branch of their own (the replayed pair of
solve_fused_kernel<.., RPL>: its unrolled steps leave through an operand test).
   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 -DRAT_PART=<bit> -S --cuda-device-only -o part.s kernels.hip
   python tools/isa_loops_all.py [--summary] part.s <substring of the mangled kernel name> [...]
A loop is a label some later branch jumps back to (several back edges to one label: the widest).  Every loop that contains f64 MFMAs is
listed with the columns of isa_loop_check.py.  A "time loop" is a listed loop with no listed loop inside it; the others ("outer": the
persistent kernel's phase loop, a loop around unrolled steps) are shown with the number of time loops they contain and are not summed.
Spill registers are the VGPRs some v_writelane of the kernel targets; a v_readlane FROM one of them is an SGPR reload.  The last table row
is what lies OUTSIDE every time loop -- the phase prologues and the glue: their spill stores and reloads.  --summary: one row per kernel
(to compare every instantiation of a template between two trees)."""
import re
import sys


def instructions(lines):
    return [l for l in lines if re.match(r"^\s+[a-z]", l) and not l.lstrip().startswith(";")]


def counts(seg, spill_regs):
    """(instructions, f64 MFMAs, scratch instructions, v_writelane, SGPR reloads) of a list of assembly lines"""
    seg = instructions(seg)
    rl = sum(1 for l in seg for m in [re.match(r"\s*v_readlane_b32 s\d+, (v\d+),", l)] if m and m.group(1) in spill_regs)
    return (len(seg), sum("v_mfma_f64" in l for l in seg), sum("scratch_" in l for l in seg), sum("v_writelane" in l for l in seg), rl)


def kernel_loops(body):
    """[(first line, last line)] of every backward-branch loop of a kernel body, one per header label"""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    ends = {}
    for i, l in enumerate(body):
        m = re.match(r"\s*s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            a = labels[m.group(1)]
            ends[a] = max(ends.get(a, i), i)
    return sorted(ends.items())


def report(src, pat, summary=False, out=sys.stdout):
    starts = [i for i, l in enumerate(src) if re.match(r"^_Z\w+:", l)]
    for s in starts:
        name = src[s].split(":")[0]
        if pat not in name:
            continue
        e = next(i for i in range(s, len(src)) if "s_endpgm" in src[i])
        body = src[s:e + 1]
        spill_regs = {m.group(1) for l in body for m in [re.match(r"\s*v_writelane_b32 (v\d+),", l)] if m}
        whole = counts(body, spill_regs)
        listed = [(lp, counts(body[lp[0]:lp[1] + 1], spill_regs)) for lp in kernel_loops(body)]
        listed = [(lp, c) for lp, c in listed if c[1] > 0]
        inside = {lp: sum(1 for o, _ in listed if o != lp and lp[0] <= o[0] and o[1] <= lp[1]) for lp, _ in listed}
        # block placement lets two time loops share lines without one holding the other: the totals count every line once
        in_time = set()
        for lp, _ in listed:
            if inside[lp] == 0:
                in_time.update(range(lp[0], lp[1] + 1))
        tot = counts([l for i, l in enumerate(body) if i in in_time], spill_regs)
        rest = [a - b for a, b in zip(whole, tot)]
        if summary:
            print(f"| `{name}` | {len(spill_regs)} | {whole[2]} | {whole[3]} | {sum(1 for lp, _ in listed if inside[lp] == 0)} | {tot[1]} | {tot[3]} | {tot[4]} | "
                  f"{rest[3]} | {rest[4]} |", file=out)
            continue
        print(f"## `{name}`: {len(body)} lines, {len(spill_regs)} SGPR-spill VGPRs {sorted(spill_regs)}, {whole[2]} scratch instructions, "
              f"{whole[3]} v_writelane in the whole kernel\n", file=out)
        print("| loop (lines) | kind | instructions | f64 MFMAs | scratch ld/st | v_writelane | SGPR reloads (v_readlane from a spill VGPR) |", file=out)
        print("|---|---|---|---|---|---|---|", file=out)
        for lp, c in listed:
            time_loops = sum(1 for o, _ in listed if o != lp and lp[0] <= o[0] and o[1] <= lp[1] and inside[o] == 0)
            kind = "time loop" if inside[lp] == 0 else f"outer ({time_loops} time loops inside)"
            print(f"| {lp[0]}-{lp[1]} | {kind} | {c[0]} | {c[1]} | {c[2]} | {c[3]} | {c[4]} |", file=out)
        print(f"| every time loop, each line once | | {tot[0]} | {tot[1]} | {tot[2]} | {tot[3]} | {tot[4]} |", file=out)
        print(f"| outside every time loop | prologues, glue | {rest[0]} | {rest[1]} | {rest[2]} | {rest[3]} | {rest[4]} |", file=out)
        print(f"\nTime loops in total: {tot[2]} scratch instructions, {tot[3]} v_writelane, {tot[4]} SGPR reloads.  "
              f"Outside them: {rest[2]} scratch instructions, {rest[3]} v_writelane, {rest[4]} SGPR reloads.\n", file=out)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--summary"]
    brief = "--summary" in sys.argv[1:]
    text = open(args[0]).read().split("\n")
    if brief:
        print("| kernel | SGPR-spill VGPRs | scratch instructions | v_writelane | time loops | f64 MFMAs in them | v_writelane in them | SGPR reloads in them | "
              "v_writelane outside | SGPR reloads outside |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    for p in args[1:]:
        report(text, p, brief)
