"""Read the gfx950 listing of the fp32 conv1 kernels: registers and the waits of their MFMA loops.

    python scripts/diag/conv1_listing.py [LISTING.s] [--full]

Without a listing it compiles ops/csrc/f32_kernels.hip to one with the flags of ops/build.py
(``--cuda-device-only -S``, as scripts/diag/gemm_listing_diff.py's header shows; CPU only, about
a minute and a half).  For ``f32_conv1_fwd_x3_k<false>``, ``<true>`` and
``f32_conv1_wgrad_x3_k<1>``, ``<2>`` it prints VGPRs, AGPRs, scratch, LDS and occupancy, then every
``s_waitcnt`` (and barrier) of the basic blocks that hold MFMAs and of the block in front of each run of
them (the preheader; and the blocks before it, back to the previous MFMA block, that load or wait on
vmcnt), with what was issued since the previous wait:

    <line> <block> s_waitcnt vmcnt(0)      | vm 13 lds 0 st 0 mfma 0

vm = global / buffer loads, lds = ds_read*, st = ds_write* + global stores, mfma = v_mfma*.
``--full`` adds one line per ds_read / global load / first MFMA of a run, to see the issue order.
A reading aid for profiles/conv1_overlap.md: it asserts nothing.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ["f32_conv1_fwd_x3_kILb0E", "f32_conv1_fwd_x3_kILb1E", "f32_conv1_wgrad_x3_kILi1E", "f32_conv1_wgrad_x3_kILi2E"]


def compile_listing(out):
    sys.path.insert(0, ROOT)
    from apex_amd.ops import build as b

    cmd = [b._hipcc(), *b.HIP_FLAGS, "-x", "hip", *b._py_includes(), "--cuda-device-only", "-S",
           str(b.CSRC / "f32_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def function(lines, tag):
    """(symbol, first line number, body lines, {descriptor / comment facts}) of the kernel whose symbol holds tag"""
    start = next(i for i, ln in enumerate(lines) if tag in ln and re.match(r"^_Z\w+:", ln))
    sym = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    facts = {}
    for ln in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize|TotalNumVgprs):\s*(\d+)", ln.strip())
        if m:
            facts[m.group(1)] = int(m.group(2))
    return sym, start, lines[start:end], facts


def blocks(body):
    """[(label, [(offset, instruction)])] in text order"""
    out, cur = [], ("entry", [])
    for off, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append(cur)
            cur = (m.group(1), [])
            continue
        s = ln.split(";")[0].strip()
        if s and not s.startswith("."):
            cur[1].append((off, s))
            if s.startswith(("s_cbranch", "s_branch")):  # the fall-through is a block of its own
                out.append(cur)
                cur = (cur[0].rstrip("+") + "+", [])
    out.append(cur)
    return out


def kind(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "vm"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "lds"
    if op.startswith(("ds_write", "ds_store", "global_store", "buffer_store", "flat_store")):
        return "st"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    return None


def report(lines, tag, full):
    sym, start, body, facts = function(lines, tag)
    print(f"== {tag}  ({sym})")
    print("   " + "  ".join(f"{k} {v}" for k, v in facts.items()))
    bl = blocks(body)
    has = [any(kind(i) == "mfma" for _, i in b[1]) for b in bl]
    show = [h or (k + 1 < len(bl) and has[k + 1]) for k, h in enumerate(has)]
    # ... and, in front of every preheader, the blocks back to the previous MFMA block (at most 40:
    # the forward's next-sample prefetch is issued there): a wait anywhere between those loads and the
    # loop counts.  Of these only the blocks that load or wait are printed.
    quiet = set()
    for k in [k for k in range(len(bl)) if show[k] and not has[k]]:
        for j in range(k - 1, max(k - 40, -1), -1):
            if has[j]:
                break
            if any(kind(i) == "vm" or i.startswith("s_waitcnt vmcnt") for _, i in bl[j][1]):
                show[j] = True
                quiet.add(j)
    n = {"vm": 0, "lds": 0, "st": 0, "mfma": 0, "smem": 0}
    for k, (label, ins) in enumerate(bl):
        if not show[k]:
            continue
        role = "loop" if has[k] else ("before" if k in quiet else "preheader")
        print(f"   -- {label} ({role}, {sum(kind(i) == 'mfma' for _, i in ins)} MFMA)")
        for key in n:
            n[key] = 0
        prev = None
        for off, i in ins:
            kd = kind(i)
            if i.startswith(("s_waitcnt", "s_barrier")):
                since = " ".join(f"{key} {v}" for key, v in n.items() if key != "smem" or v)
                print(f"   {start + off + 1:7d} {label:10s} {i:34s} | {since}")
                for key in n:
                    n[key] = 0
            elif kd:
                n[kd] += 1
                if full and (kd in ("vm", "lds") or (kd == "mfma" and prev != "mfma")):
                    print(f"   {start + off + 1:7d} {label:10s}     {i[:60]}")
            if kd:
                prev = kd
        print(f"           {label:10s} (end of block)                     | "
              + " ".join(f"{key} {v}" for key, v in n.items() if key != "smem" or v))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    full = "--full" in sys.argv
    if args:
        path = args[0]
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="conv1_listing_"), "f32_kernels.s")
        compile_listing(path)
        print("listing:", path)
    lines = open(path).read().split("\n")
    for tag in KERNELS:
        report(lines, tag, full)


if __name__ == "__main__":
    main()
