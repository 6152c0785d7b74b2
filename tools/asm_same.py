"""Compares the kernels of two device assembly files (hipcc -O3 -S --cuda-device-only).

    python tools/asm_same.py parent.s this.s [name-filter]

Per kernel of the first file whose demangled name holds the filter: the instruction streams are
compared line by line after removing comments and the function number of local labels
(.LBB<n>_<m>, which moves when kernels are added in between).  Kernels are matched by their
demangled name without the parameter list (namespace, template name and template arguments), so a
template that gains a trailing parameter pack, empty in the existing instantiations, still pairs
up: its mangled names change, its argument lists and so its kernel-argument offsets do not.
Prints the kernels that differ or are missing, the kernels only the second file has, and the counts.
"""
import re
import subprocess
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
                continue
            t = line.split(";", 1)[0].strip()
            if t and not t.startswith(".p2align"):
                cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    names = sorted(out)
    dem = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    by_dem = {}
    for n, d in zip(names, dem):
        assert d not in by_dem, f"two kernels of {path} demangle to {d}"
        by_dem[d] = [t.replace(n, "@self") for t in out[n]]  # (the directives after s_endpgm name the kernel)
    return by_dem


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    filt = sys.argv[3] if len(sys.argv) > 3 else "k_vol_"
    same = diff = 0
    for n in sorted(a):
        if filt not in n:
            continue
        if n not in b:
            print("MISSING  ", n)
            diff += 1
        elif a[n] != b[n]:
            k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            print("DIFFERS  ", n, "at instruction", k)
            diff += 1
        else:
            same += 1
    new = [n for n in sorted(b) if n not in a and filt in n]
    print(f"{same} kernels of the first file identical in the second ({sum(len(a[n]) for n in a if filt in n)} "
          f"lines compared), {diff} different or missing, {len(new)} new")
    for n in new:
        print("NEW      ", n)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
