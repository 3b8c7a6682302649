"""Per-kernel text diff of two device-assembly listings (hipcc --cuda-device-only -S of one source from two trees):
IDENT where a kernel's instruction stream is the same text (comments and the function's index in basic-block labels
aside), else DIFF with both VGPR counts, instruction counts, scratch sizes and spill counts.  A refactor that must not move a kernel checks it with this.

  python tools/asm_identity.py OLD.s NEW.s [OLDNAME=NEWNAME ...]

A kernel that the refactor renamed is matched by naming the pair: the old listing's OLDNAME is compared as NEWNAME.
"""
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{demangled name: (body lines, {resource: value})} of every .amdhsa_kernel in the listing."""
    lines = open(path).read().splitlines()
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    out = {}
    for sym in names:
        a = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        # (basic-block labels carry the function's index in the listing, which moves with the order of instantiation)
        # (... and the directives inside the body name the kernel itself, which a rename changes)
        body = [re.sub(r"BB\d+_", "BB_", l).replace(sym, "<kernel>") for l in lines[a + 1:b] if "__hip_cuid" not in l]
        res_spills = sum("Spill" in l for l in body)
        body = [l for l in (re.sub(r"\s*;.*$", "", l) for l in body) if l]  # no comments
        tail = "\n".join(lines[b:b + 40])
        res = {k: int(re.search(r"; %s: (\d+)" % k, tail).group(1)) for k in ("NumVgprs", "ScratchSize")}
        res["spills"] = res_spills
        res["insts"] = sum(bool(re.match(r"\s+[a-z]\w+", l)) and not l.lstrip().startswith(".") for l in body)
        out[sym] = (body, res)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return out
    dem = subprocess.run([filt], input="\n".join(out), capture_output=True, text=True)
    return {d: out[s] for d, s in zip(dem.stdout.splitlines(), out)}


if __name__ == "__main__":
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for pair in sys.argv[3:]:  # OLD=NEW: the old listing's kernels whose name contains OLD are compared as NEW
        a, b = pair.split("=")
        old = {k.replace(a, b): v for k, v in old.items()}
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("ONLY-%s %s" % ("OLD" if name in old else "NEW", name))
        elif old[name][0] == new[name][0]:
            print("IDENT %s" % name)
        else:
            print("DIFF  %s\n      old %s\n      new %s" % (name, old[name][1], new[name][1]))
