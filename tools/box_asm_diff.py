#!/usr/bin/env python3
"""Compare the device code of one source file between two commits, kernel by kernel.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Igamesmanmpi_amd/csrc -S --cuda-device-only \\
        gamesmanmpi_amd/csrc/dense_box.hip -o new.s          (and the same in a checkout of the parent)
    python tools/box_asm_diff.py parent.s new.s [--rename OLD=NEW ...]

Per kernel: the instruction streams compared line by line (comments, directives, labels' numbering
aside and blank lines dropped), the instruction count, .amdhsa_next_free_vgpr and the scratch size.
--rename maps a parent kernel's demangled name to its name here (a new template parameter).
"""
import argparse
import re
import subprocess


def kernels(path):
    text = open(path).read()
    out = {}
    # a kernel's code runs from its label to its .amdhsa_kernel descriptor
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        name, body, desc = m.group(1), m.group(2), m.group(3)
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            # a local label carries the function's number in the file, which moves with the order of emission
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        sc = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
        out[name] = (ins, vg, int(sc.group(1)) if sc else 0)
    return out


def demangle(names):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    ren = dict(r.split("=", 1) for r in a.rename)
    ko, kn = kernels(a.parent), kernels(a.new)
    do, dn = demangle(list(ko)), demangle(list(kn))
    old = {ren.get(do[k], do[k]): v for k, v in ko.items()}
    new = {dn[k]: v for k, v in kn.items()}
    same = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o and n:
            tag = "identical" if o[0] == n[0] else "CHANGED"
            same += tag == "identical"
            print("%-9s %-52s instructions %5d -> %5d  next_free_vgpr %d -> %d  scratch %d -> %d" %
                  (tag, name, len(o[0]), len(n[0]), o[1], n[1], o[2], n[2]))
        elif n:
            print("%-9s %-52s instructions     - -> %5d  next_free_vgpr - -> %d  scratch - -> %d" %
                  ("new", name, len(n[0]), n[1], n[2]))
        else:
            print("%-9s %-52s instructions %5d ->     -" % ("removed", name, len(o[0])))
    print("\n%d kernels of the parent, %d identical" % (len(old), same))


if __name__ == "__main__":
    main()
