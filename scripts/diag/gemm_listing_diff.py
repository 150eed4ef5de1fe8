"""Pair the fp32 GEMM kernels of two device listings of f32_kernels.hip and compare them.

    hipcc <ops/build.py HIP_FLAGS> -x hip <includes> --cuda-device-only -S f32_kernels.hip -o X.s
    python scripts/diag/gemm_listing_diff.py OLD.s NEW.s

A kernel is keyed by (gemm_k | gemm2_k, policies, form, XB, EP), read off its mangled name: the
older listing carries the prefetch depth after the form, and only depth 1 has a counterpart in
the newer one, which has no depth.  For each pair the function's text
and every .amdhsa_ line must be equal once the kernel's own symbol is replaced (assembler
comments dropped, local labels renumbered by order of appearance, blanks collapsed: they follow
the symbol's length and the function's position in the file).  Prints the
counts, the kernels that differ and the kernels without a counterpart; exits 1 on a difference.
"""
import re
import sys

OLD = re.compile(r"_ZN4apex12_GLOBAL__N_1\d(gemm2?_k)I(.+E)Li(\d)ELi(\d)ELb([01])ELi(\d)EEEv")
NEW = re.compile(r"_ZN4apex12_GLOBAL__N_1\d(gemm2?_k)I(.+E)Li(\d)ELb([01])ELi(\d)EEEv")


def key(sym):
    m = OLD.match(sym)
    if m:
        k, pol, form, depth, xb, ep = m.groups()
        return (k, pol, form, xb, ep) if depth == "1" else None
    m = NEW.match(sym)
    if m:
        return m.groups()
    return None


def kernels(path):
    """{key: (symbol, text + descriptor lines with the symbol replaced)}, and the count of GEMM kernels"""
    lines = open(path).read().split("\n")
    out, n = {}, 0
    for i, ln in enumerate(lines):
        if not ln.startswith("\t.amdhsa_kernel "):
            continue
        sym = ln.split()[1]
        if "gemm_k" not in sym and "gemm2_k" not in sym:
            continue
        n += 1
        k = key(sym)
        if k is None:
            continue
        j = i
        while not lines[j].startswith(sym + ":"):
            j -= 1
        body = []
        for t in lines[j:]:
            if t.startswith(".Lfunc_end"):
                break
            body.append(t)
        e = i
        while not lines[e].startswith("\t.end_amdhsa_kernel"):
            e += 1
        body += [t for t in lines[i:e] if ".amdhsa_" in t]
        # local labels are numbered through the file: compare them by order of appearance
        text = "\n".join(body).replace(sym, "<kernel>")
        labels = {}
        text = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), text)
        # (comments name basic blocks by the function's number in the file)
        out[k] = (sym, re.sub(r"[ \t]+", " ", re.sub(r"[ \t]*;.*", "", text)))
    return out, n


def main():
    (old, n_old), (new, n_new) = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k][1] != new[k][1]]
    print(f"GEMM kernels: {n_old} -> {n_new}; surviving in the old listing {len(old)}, paired {len(both)}, "
          f"identical {len(both) - len(differ)}, new only {len(set(new) - set(old))}")
    for k in differ:
        print("differs:", new[k][0])
    for k in sorted(set(old) - set(new)):
        print("no counterpart:", old[k][0])
    sys.exit(1 if differ or set(old) - set(new) else 0)


if __name__ == "__main__":
    main()
