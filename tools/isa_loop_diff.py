"""Step loops of two sets of gfx950 listings (fhe-regex_amd: make asm), kernel by kernel: whether
the multiset of f64 instructions is the same, the LDS reads and waits in front of the loop's first
f64 instruction (the digits), and every opcode whose count changed.
Usage: python tools/isa_loop_diff.py OLD_DIR NEW_DIR [name-substring]   (exit 1: an f64 multiset differs)"""
import collections
import glob
import os
import re
import sys


def kernels(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*gfx950.s"))):
        lines = open(f).read().split("\n")
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M):
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            out[name] = lines[start:end]
    return out


def step_loop(body):
    """instructions of the longest backward branch's span"""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_(?:c)?branch\w*\s+(\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and (best is None or i - labels[m.group(1)] > best[1] - best[0]):
            best = (labels[m.group(1)], i)
    if best is None:
        return []
    out = []
    for l in body[best[0]:best[1] + 1]:
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    return out


def head(ins):
    first = next((i for i, x in enumerate(ins) if "f64" in x.split()[0]), len(ins))
    return first, [x for x in ins[:first] if x.startswith("ds_read")], [x for x in ins[:first] if x.startswith("s_waitcnt")]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    bad = 0
    for name in sorted(set(old) & set(new)):
        if pat not in name:
            continue
        a, b = step_loop(old[name]), step_loop(new[name])
        if not a or not b:
            continue
        ca, cb = (collections.Counter(x.split()[0] for x in v) for v in (a, b))
        fa, fb = ({k: v for k, v in c.items() if "f64" in k} for c in (ca, cb))
        same = fa == fb
        bad += not same
        (ia, ra, wa), (ib, rb, wb) = head(a), head(b)
        print(name)
        print("  loop: %d -> %d instructions; f64: %d -> %d, multiset %s" % (len(a), len(b), sum(fa.values()), sum(fb.values()),
                                                                            "the same" if same else "DIFFERENT"))
        print("  before the first f64 instruction (at %d -> %d): ds_read %d -> %d, s_waitcnt %s -> %s" % (ia, ib, len(ra), len(rb), wa, wb))
        changed = {k: (ca.get(k, 0), cb.get(k, 0)) for k in sorted(set(ca) | set(cb)) if ca.get(k, 0) != cb.get(k, 0)}
        print("  counts changed: %s" % (", ".join("%s %d -> %d" % (k, x, y) for k, (x, y) in changed.items()) or "none"))
    sys.exit(1 if bad else 0)


main()
