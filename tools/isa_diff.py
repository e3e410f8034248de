"""Per-function comparison of two device assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S output).

Basic-block label numbers (.LBB12_3 and kin) and comments are numbered / written per translation unit, so they are
normalised away; everything else of a function's body must match line for line.  Prints every parent function that
differs or is missing, then the counts and the functions that are new.
usage: python tools/isa_diff.py parent.s branch.s   (names are mangled: pipe through c++filt to read them)"""
import re
import sys


def functions(path):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            if cur:
                out[cur] = body
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        line = re.sub(r"\.(LBB|Ltmp|LJTI|LCPI)\d+_", r".\1F_", line)
        line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_endF", line)
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n"))
        if line:
            body.append(line)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = diff = 0
    for k in sorted(a):
        if k not in b:
            print("MISSING in branch:", k)
            diff += 1
        elif a[k] != b[k]:
            print("DIFFERS:", k)
            diff += 1
        else:
            same += 1
    new = sorted(set(b) - set(a))
    print("parent functions %d, identical %d, differing/missing %d, new in branch %d" % (len(a), same, diff, len(new)))
    for k in new:
        print("NEW:", k)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
