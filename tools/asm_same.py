#!/usr/bin/env python3
"""Which kernels of two device listings (hipcc --cuda-device-only -S, e.g. tools/kres.sh -> /tmp/asm/k/all.s) are the SAME code:
function by function, comments and directives dropped, block labels renumbered in order of appearance.  Prints the functions that
differ (demangled) and the count of those that do not.  usage: asm_same.py a.s b.s"""
import re
import subprocess
import sys


def functions(path):
    out, name, body, labels = {}, None, None, None
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        l = l.split(";")[0].strip()
        if not l or (l.startswith(".") and not l.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), f"L{len(labels)}"), l))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    differ = sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))
    names = subprocess.run(["c++filt"], input="\n".join(differ), capture_output=True, text=True).stdout.split("\n") if differ else []
    print(f"{len(a)} / {len(b)} functions; same listing: {len(a.keys() & b.keys()) - sum(k in a and k in b for k in differ)}; differ: {len(differ)}")
    for k, n in zip(differ, names):
        print(f"  {n.split('(')[0]}   {len(a.get(k, []))} -> {len(b.get(k, []))} instructions")


if __name__ == "__main__":
    main()
