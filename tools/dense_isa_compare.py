"""Do two builds of a kernel file give the same code for the kernels both have?  Compiles nothing itself: takes two assembly listings,

    hipcc --offload-arch=gfx950 -O3 -std=c++17 [-ffp-contract=off for neighbor.hip] -S --cuda-device-only -o old.s <old file>.hip
    hipcc ...                                                                                       -o new.s <new file>.hip
    python tools/dense_isa_compare.py old.s new.s [--ignore-kernarg-offsets] [--rename REGEX=REPL ...] [--resources old.txt new.txt]

and compares kernel by kernel the instruction text up to s_endpgm, with comments and assembler directives dropped, local labels
renumbered and the kernel's own symbol masked.  A kernel that gained a template parameter is matched by its name with the new
parameter's `ILb0E` instantiation (the dense form of a kernel with a counted sibling); --rename maps the DEMANGLED name of an old kernel
(without `void` and the parameter list) to the new kernel that took its place, e.g. 'knn_counted_kernel<(\\d+)>=knn_kernel<\\1, false, true>'.
--ignore-kernarg-offsets also masks the literal offsets of scalar loads from the kernel-argument segment (an instantiation whose
argument list was reordered or grew in the middle).  --resources: the two compilers' stderr under
`-Rpass-analysis=kernel-resource-usage`; prints (VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, waves/SIMD) old -> new per kernel and
counts a figure that grew (occupancy: fell) like a DIFF.  Exit status 1 when a common kernel differs."""
import re
import subprocess
import sys

RES = (r"VGPRs", r"AGPRs", r"SGPRs", r"LDS Size \[bytes/block\]", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]")


def kernels(path, mask_kernarg):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)s_endpgm", open(path).read(), flags=re.S | re.M):
        lines = [l.split(";")[0].rstrip() for l in m.group(2).splitlines()]
        lines = [l for l in lines if l.strip() and not l.strip().startswith(".") or re.match(r"\.LBB\d+_\d+:", l.strip())]
        body = re.sub(r"\.LBB\d+_", "LBB_", "\n".join(lines)).replace(m.group(1), "SELF")
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


def demangled(names):
    """mangled -> 'kernel<args>'"""
    if not names:
        return {}
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, out)}


def resources(path):
    out = {}
    for m in re.finditer(r"Function Name: (\S+).*?(?=Function Name:|\Z)", open(path).read(), flags=re.S):
        out[m.group(1)] = tuple(int(re.search(k + r": (\d+)", m.group(0)).group(1)) for k in RES)
    return out


argv = sys.argv[1:]
old_s, new_s = argv[0], argv[1]
mask = "--ignore-kernarg-offsets" in argv
renames = [argv[i + 1].split("=", 1) for i, a in enumerate(argv) if a == "--rename"]
res = [resources(argv[argv.index("--resources") + k]) for k in (1, 2)] if "--resources" in argv else None
old, new = kernels(old_s, mask), kernels(new_s, mask)
plain_old, plain_new = demangled(list(old)), demangled(list(new))
bad = 0
taken = set()
for name, body in old.items():
    dense = "_Z%d%sILb0E" % (len(base(name)), base(name))
    want = plain_old[name]
    for pat, rep in renames:
        want = re.sub("^" + pat, rep, want)
    cand = [n for n in new if n == name] or [n for n in new if renames and plain_new[n] == want] or [n for n in new if n.startswith(dense)]
    if not cand:
        print("only in old:", plain_old[name])
        continue
    same = [c for c in cand if new[c] == body]
    hit = (same or cand)[0]
    taken.add(hit)
    note = ""
    if res:
        a, b = res[0][name], res[1][hit]
        grew = any(y > x for x, y in zip(a[:5], b[:5])) or b[5] < a[5]
        note = "  %s -> %s%s" % (a, b, "  GREW" if grew else "")
        bad += grew
    bad += not same
    label = plain_old[name] if plain_new[hit] == plain_old[name] else "%s -> %s" % (plain_old[name], plain_new[hit])
    print("%-5s %-100s %5d lines%s" % ("same" if same else "DIFF", label, len(body.splitlines()), note))
for name in new:
    if name not in taken and name not in old and not any(base(name) == base(o) for o in old):
        print("new:  ", plain_new[name])
sys.exit(1 if bad else 0)
