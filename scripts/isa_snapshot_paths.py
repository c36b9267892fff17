#!/usr/bin/env python
"""What a wave of wfa_tile2_kernel issues OUTSIDE its step loop, from the compiler's assembly (hipcc -S --cuda-device-only with the build's flags
for wfa_tile2.hip): per instantiation

  * registers and scratch (the kernel's metadata), global_load_dwordx2 / global_store_dwordx2 / global_store_dword counts;
  * the lean load: the straight-line block that holds the 32 unmasked row loads (no exec-mask region), label to branch;
  * the general load: from the first exec-mask region that guards a row load to the end of the last one before the first s_barrier -- a full
    wave falls through every s_cbranch_execz there, so every instruction of the range is on its path (the lean block, where the compiler put it
    inside that range, is left out);
  * the lean store: the straight-line blocks of unmasked 8-byte row stores (one per copy of write_rows the compiler kept apart);
  * the general store: everything behind the step loop but the lean blocks -- the pending row's extension, five copies of write_rows (T mod 5),
    the short-last-block path and the maxima's epilogue together, with the stores among it; a wave runs ONE copy, about a fifth of it;
  * the step loop (the longest outermost loop of the kernel, header to back edge, and the rare paths laid out behind it), all paths (static): the ten-step body with its rare branches.
    `isa_hot_path.py` prices the common path of one step; its figures move between the steps of a body with the scheduler's choices (the
    barriers are no scheduling boundaries for register moves), so two trees are compared over the whole body.

Counts are of ordinary instructions only (a line that begins with a mnemonic).
usage: isa_snapshot_paths.py tile2.s [more.s ...]"""
import re
import sys

INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def functions(lines):
    out, name, start = [], None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN3wfm16wfa_tile2_kernelI\w+?EEEv\w+):", l)
        if m:
            name, start = m.group(1), i
        elif name and l.startswith(".Lfunc_end"):  # (a kernel holds several s_endpgm: one per early exit)
            out.append((name, start, i))
            name = None
    return out


def short(name):
    m = re.match(r"_ZN3wfm16wfa_tile2_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)EEE", name)
    return "<%s,%s,%s,%s>" % (m.group(1), *("true" if m.group(k) == "1" else "false" for k in (2, 3, 4)))


def op(l):
    m = INSTR.match(l)
    return m.group(1) if m else None


def n_instr(body, a, b, skip=()):
    return sum(1 for i in range(a, b) if op(body[i]) and not any(x <= i < y for x, y in skip))


def blocks(body):
    """straight-line blocks: [begin, end) split at labels and behind branches"""
    cuts = {0, len(body)}
    for i, l in enumerate(body):
        if LABEL.match(l):
            cuts.add(i)
        o = op(l)
        if o and (o.startswith("s_cbranch") or o == "s_branch"):
            cuts.add(i + 1)
    c = sorted(cuts)
    return list(zip(c, c[1:]))


def metadata(lines, name):
    i = next(k for k, l in enumerate(lines) if l.strip() == ".name:           " + name or (l.strip().startswith(".name:") and l.split()[-1] == name))
    md = {}
    for l in lines[max(0, i - 40):i + 40]:
        m = re.match(r"\s+\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", l)
        if m:
            md[m.group(1)] = int(m.group(2))
    return md


def report(path):
    lines = open(path).read().split("\n")
    print("==", path)
    for name, a, b in functions(lines):
        body = lines[a:b]
        ops = [op(l) for l in body]
        labels = {LABEL.match(l).group(1): i for i, l in enumerate(body) if LABEL.match(l)}
        headers = {i for i, l in enumerate(body) if LABEL.match(l) and "Loop Header: Depth=1" in l}
        jumps = [(i, labels[m.group(1)]) for i, l in enumerate(body) for m in [re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)] if m and m.group(1) in labels]
        # the step loop: the outermost loop with the longest span, header to its last back edge; the rare paths the compiler laid out behind it
        # (blocks that jump back into it) belong to it
        _, loop_h, loop_e = max((i - t, t, i) for i, t in jumps if t in headers and t < i)
        loop_x = max([loop_e] + [i for i, t in jumps if i > loop_e and loop_h <= t <= loop_e])
        md = metadata(lines, name)
        print(f"{short(name)}: vgpr {md.get('vgpr_count')} scratch {md.get('private_segment_fixed_size')} vgpr spills {md.get('vgpr_spill_count')}"
              f" | global_load_dwordx2 {ops.count('global_load_dwordx2')} global_store_dwordx2 {ops.count('global_store_dwordx2')} global_store_dword {ops.count('global_store_dword')}")
        bl = blocks(body)
        # the snapshot load ends where the smallest live offset goes to LDS (ds_min), before the loop; the store begins behind the loop
        first_bar = min([loop_h] + [i for i, o in enumerate(ops) if o and o.startswith("ds_min")])
        last_bar = loop_x + 1
        lean_ld = [(x, y) for x, y in bl if y <= first_bar and ops[x:y].count("global_load_dwordx2") >= 28]
        lean_st = [(x, y) for x, y in bl if x >= last_bar and ops[x:y].count("global_store_dwordx2") >= 20]
        # the general load: exec-mask regions (s_and_saveexec_b64 ... global_load_dwordx2 within a few lines) before the first barrier
        masked = [i for i in range(first_bar) if ops[i] == "global_load_dwordx2" and not any(x <= i < y for x, y in lean_ld)
                  and any(ops[j] == "s_and_saveexec_b64" for j in range(max(0, i - 14), i))]
        if masked:
            g0 = max(j for j in range(masked[0]) if ops[j] == "s_and_saveexec_b64")
            g1 = next(j for j in range(masked[-1], first_bar) if ops[j] == "s_or_b64" and "exec" in body[j]) + 1
            n = n_instr(body, g0, g1, lean_ld)
            sc = sum(1 for i in range(g0, g1) if ops[i] and ops[i].startswith("s_") and not any(x <= i < y for x, y in lean_ld))
            print(f"   general load: {n} instructions ({sc} scalar) around {len(masked)} masked loads; v_writelane {ops[g0:g1].count('v_writelane_b32')}"
                  f" v_readlane {ops[g0:g1].count('v_readlane_b32')}")
        for x, y in lean_ld:
            print(f"   lean load:    {n_instr(body, x, y)} instructions around {ops[x:y].count('global_load_dwordx2')} loads")
        if not lean_ld:
            print("   lean load:    none")
        if short(name).split(",")[1] != "true":  # (the P2 form's 32 steps are laid out differently: its conditions are the registers above)
            print(f"   step loop, all paths: {n_instr(body, loop_h, loop_x + 1)} instructions, {ops[loop_h:loop_x + 1].count('s_barrier')} s_barrier")
        if short(name).split(",")[1] == "true":
            continue  # P2: no output snapshot
        tail = n_instr(body, last_bar, len(body), lean_st)
        st1 = sum(1 for i in range(last_bar, len(body)) if ops[i] == "global_store_dword")
        st2 = sum(1 for i in range(last_bar, len(body)) if ops[i] == "global_store_dwordx2" and not any(x <= i < y for x, y in lean_st))
        print(f"   general store and epilogue (all five copies): {tail} instructions around {st1} 4-byte and {st2} 8-byte stores")
        for x, y in lean_st:
            print(f"   lean store:   {n_instr(body, x, y)} instructions around {ops[x:y].count('global_store_dwordx2')} 8-byte stores")
        if not lean_st:
            print("   lean store:   none")


for p in sys.argv[1:]:
    report(p)
