#!/usr/bin/env python3
"""Diff of two builds' device code, kernel by kernel:  kernel_asm_diff.py OLD NEW

OLD / NEW: a directory of `hipcc --cuda-device-only -S` output (*.s), or a csrc directory (*.hip), whose translation
units -- the .hip files no other .hip file includes -- are compiled to assembly first.  A kernel's text is what stands
between its label and .Lfunc_end, comments and blank lines dropped, the numbers of function-local labels (.LBB<n>_,
.Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_, .LCPI<n>_) renumbered in order of appearance; its .amdhsa_* descriptor block
(registers, LDS, scratch) is compared on its own.  Prints the kernels that differ or exist on one side only (exit
status 1 if there is any), and those whose number of copies changed, which count only if some copy differs from the
others.  Which file a kernel sits in does not matter."""
import concurrent.futures, glob, os, re, subprocess, sys, tempfile

FLAGS = "-O3 -std=c++17 -fPIC -Wall -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form=1 --offload-arch=gfx950".split()
LABEL = re.compile(r"\.(LBB|Lfunc_end|Ltmp|LJTI|LCPI)(\d+)")


def assembly(path):
    if glob.glob(os.path.join(path, "*.s")):
        return sorted(glob.glob(os.path.join(path, "*.s")))
    hips = sorted(glob.glob(os.path.join(path, "*.hip")))
    included = set(re.findall(r'#include "([^"]+\.hip)"', "".join(open(h).read() for h in hips)))
    out = tempfile.mkdtemp(prefix="kasm_")
    jobs = [(h, os.path.join(out, os.path.basename(h)[:-4] + ".s")) for h in hips if os.path.basename(h) not in included]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda j: subprocess.check_call([hipcc, *FLAGS, "--cuda-device-only", "-S", "-o", j[1], j[0]]), jobs))
    return [j[1] for j in jobs]


def kernels(files):
    """name -> list of (code, descriptor), one entry per definition"""
    found = {}
    for f in files:
        text = open(f).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
            body = text[text.index("\n%s:" % name):]
            body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).end()]
            lines = [l.split(";")[0].rstrip() for l in body.splitlines()]
            seen = {}
            lines = [LABEL.sub(lambda m: ".%s%d" % (m.group(1), seen.setdefault(m.group(0), len(seen))), l) for l in lines if l.strip()]
            desc = [l for l in lines if l.lstrip().startswith(".amdhsa_")]
            found.setdefault(name, []).append(([l for l in lines if l not in desc], desc))
    return found


def main(old, new):
    a, b = kernels(assembly(old)), kernels(assembly(new))
    bad = shared = 0
    for name in sorted(set(a) | set(b)):
        na, nb = len(a.get(name, ())), len(b.get(name, ()))
        why = ["only in %s" % s for s, n in (("old", na), ("new", nb)) if not n]
        if not why and na != nb:     # a template that fewer or more units instantiate: fine if every copy is the same
            same = all(k == a[name][0] for k in a[name] + b[name])
            print("%s: %d copies in old, %d in new, %s" % (name, na, nb, "all texts and descriptors identical" if same else "and they differ"))
            bad += not same
        elif not why:                # (a template two units instantiate exists once per unit, on both sides)
            shared += na > 1
            pairs = list(zip(sorted(a[name]), sorted(b[name])))
            why = [what + " differs" for i, what in enumerate(("code", "descriptor")) if any(p[i] != q[i] for p, q in pairs)]
        for w in why: print("%s: %s" % (name, w))
        bad += bool(why)
    print("%d kernels in old, %d in new (%d of them in more than one unit on both sides), %d to look at" % (len(a), len(b), shared, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
