"""Per-kernel comparison of two sets of gfx950 listings (fhe-regex_amd: make asm).
Usage: python tools/isa_diff.py OLD NEW   (each a .s file or a directory of them)
A kernel is `identical`, `identical-through-loop` (the first difference lies after the
closing branch of its longest backward branch, the step loop of tools/isa_loop.py) or
`DIFFERS`; the resource figures (SGPRs, VGPRs, scratch, occupancy) are printed for both."""
import glob
import os
import re
import sys

DROP = re.compile(r"^\s*(\.loc|\.file|\.ident|\.cfi\w*)\b|^\.Ltmp\w*:")
RES = ("TotalNumSgprs", "TotalNumVgprs", "ScratchSize", "Occupancy")


def kernels(path):
    out = {}
    files = sorted(glob.glob(os.path.join(path, "*gfx950.s"))) if os.path.isdir(path) else [path]
    for f in files:
        lines = open(f).read().split("\n")
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M):
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            body, ids = [], {}
            for l in lines[start:end]:
                l = l.split(";")[0].rstrip()
                if not l or DROP.match(l):
                    continue
                body.append(re.sub(r"\.LBB\w+", lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l))
            tail = "\n".join(lines[end:end + 40])
            res = tuple(int(re.search(r"; %s: (\d+)" % k, tail).group(1)) for k in RES)
            out[name] = (body, res)
    return out


def loop_end(body):
    labels = {l[:-1]: i for i, l in enumerate(body) if re.match(r"^\.L\d+:$", l)}
    best = (0, -1)
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.L\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            best = max(best, (i - labels[m.group(1)], i))
    return best[1]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-22s %s" % ("ONLY-OLD" if name in old else "ONLY-NEW", name))
            bad += 1
            continue
        (a, ra), (b, rb) = old[name], new[name]
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        if first is None:
            verdict = "identical"
        elif first > loop_end(a) >= 0 and loop_end(a) == loop_end(b):
            verdict = "identical-through-loop"
        else:
            verdict = "DIFFERS@%d(loop-end %d)" % (first, loop_end(a))
        if ra != rb or verdict.startswith("DIFFERS"):
            bad += 1
        print("%-22s %s  %s -> %s%s" % (verdict, name, ra, rb, "" if ra == rb else "  RESOURCES CHANGED"))
    sys.exit(1 if bad else 0)


main()
