"""Do two builds of a kernel file give the same code for the kernels both have?  Compiles nothing itself: takes two assembly listings,

    hipcc --offload-arch=gfx950 -O3 -std=c++17 [-ffp-contract=off for neighbor.hip] -S --cuda-device-only -o old.s <old file>.hip
    hipcc ...                                                                                       -o new.s <new file>.hip
    python tools/dense_isa_compare.py old.s new.s [--ignore-kernarg-offsets]

and compares kernel by kernel the instruction text up to s_endpgm, with comments dropped and local labels renumbered.  A kernel that
gained a template parameter is matched by its name with the new parameter's `ILb0E` instantiation (the dense form of a kernel with a
counted sibling).  --ignore-kernarg-offsets also masks the literal offsets of scalar loads from the kernel-argument segment (a dense
instantiation whose argument list grew in the middle).  Exit status 1 when a common kernel differs."""
import re
import sys


def kernels(path, mask_kernarg):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)s_endpgm", open(path).read(), flags=re.S | re.M):
        body = "\n".join(l.split(";")[0].rstrip() for l in m.group(2).splitlines())
        body = re.sub(r"\.LBB\d+_", "LBB_", body)
        if mask_kernarg:
            body = re.sub(r"(s_load_dword\w*\s+s\[?[\d:]+\]?, s\[0:1\], )0x[0-9a-f]+", r"\1OFF", body)
            body = "\n".join(sorted(body.splitlines()))             # loads of shifted arguments may be reordered
        out[m.group(1)] = body
    return out


def base(name):
    """_Z<len><name>... -> <name> (template arguments and parameter types dropped); a nested name (_ZN...: a kernel in a namespace)
    is its own base and is matched by its full name only"""
    m = re.match(r"_Z(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


old_s, new_s = sys.argv[1], sys.argv[2]
mask = "--ignore-kernarg-offsets" in sys.argv
old, new = kernels(old_s, mask), kernels(new_s, mask)
bad = 0
for name, body in old.items():
    dense = "_Z%d%sILb0E" % (len(base(name)), base(name))
    cand = [n for n in new if n == name] or [n for n in new if n.startswith(dense)]
    if not cand:
        print("only in old:", name)
        continue
    same = any(new[c] == body for c in cand)
    bad += not same
    print("%-5s %s" % ("same" if same else "DIFF", name))
for name in new:
    if name not in old and not any(base(name) == base(o) for o in old):
        print("new:  ", name)
sys.exit(1 if bad else 0)
