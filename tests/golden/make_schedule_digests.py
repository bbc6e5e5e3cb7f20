"""Generates tests/golden/schedule_digests.json: the SHA-256 of the host-only match
schedule (fheregex.schedule_match, no device) of a fixed corpus of cases.  The digest
covers the bytes of every fr_job (unused entries are zero), level_off and every
part's (out_gate, out_w, out_const), so it pins the lowered program and its schedule
gate for gate and in order; a case that raises stores the exception's class name.
tests/test_host.py::test_schedule_digests recomputes the digests and compares them: a
refactor of the parser, the recorders, the lowering or the scheduler must leave the
file as it is.

The corpus: the BASELINE configs (/^abc$/ x 3, /abc/ x 64 and 256, /^[a-z]+$/ x 256,
/the/i x 1024), /^[a-z0-9]+$/ x 256 under GRAMMAR_EXT, config 5's pattern x 64 under
ENGINE_MERGED, and the patterns of engine_vectors, readme_vectors, fuzz_scale and
fuzz_boundary at their own content lengths; each crossed with the three lowerings,
max_parts in {1, 2, 4, 16} and multi_value in {0, 1}, the first seven also with the
start range [L/4, L/2).  The cases themselves are stored, not seeds: one row per
(pattern, length, start range, engine, grammar) with the crossed axes named once, and per
row its distinct digests and each case's index into them (many cases of a row share a
schedule: a faithful lowering has one part whatever max_parts says).

Regenerate only when a change is meant to alter schedules, with the library of the
revision that defines them (FHEREGEX_LIB selects it), from the repo root:
    python3 tests/golden/make_schedule_digests.py
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "fhe-regex_amd")]
import fheregex as F  # noqa: E402

OUT = os.path.join(HERE, "schedule_digests.json")
CONFIG5 = "/^a{2,8}(bc|de)+[^xyz]$/"
# (pattern, n_chars, engine, grammar): these also get a proper sub-range of starts
NAMED = [("/^abc$/", 3, F.ENGINE_AUTO, F.GRAMMAR_REFERENCE),
         ("/abc/", 64, F.ENGINE_AUTO, F.GRAMMAR_REFERENCE),
         ("/abc/", 256, F.ENGINE_AUTO, F.GRAMMAR_REFERENCE),
         ("/^[a-z]+$/", 256, F.ENGINE_AUTO, F.GRAMMAR_REFERENCE),
         ("/the/i", 1024, F.ENGINE_AUTO, F.GRAMMAR_REFERENCE),
         ("/^[a-z0-9]+$/", 256, F.ENGINE_AUTO, F.GRAMMAR_EXT),
         (CONFIG5, 64, F.ENGINE_MERGED, F.GRAMMAR_REFERENCE)]
LOWERINGS = (F.LOWER_FAITHFUL, F.LOWER_THRESHOLD, F.LOWER_FAITHFUL_TREE)
MAX_PARTS = (1, 2, 4, 16)
MULTI_VALUE = (0, 1)
FIELDS = ("pattern", "n_chars", "lo", "hi", "engine", "grammar", "lowering", "max_parts", "multi_value")


def _load(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


def sources():
    """(pattern, n_chars, lo, hi, engine, grammar), deduplicated, in a fixed order"""
    named = [(p, n, e, g, True) for p, n, e, g in NAMED]
    vectors = _load("engine_vectors.json") + _load("readme_vectors.json")["cases"] + \
        _load("fuzz_scale.json")["cases"] + _load("fuzz_boundary.json")["cases"]
    named += [(v["pattern"], len(v["content"]), F.ENGINE_AUTO, F.GRAMMAR_REFERENCE, False) for v in vectors]
    out = []
    for pattern, n, engine, grammar, sub in named:
        for lo, hi in [(0, n)] + ([(n // 4, n // 2)] if sub else []):
            if (pattern, n, lo, hi, engine, grammar) not in out:
                out.append((pattern, n, lo, hi, engine, grammar))
    return out


def cases_of(source):
    """a source's cases, tuples in the order of FIELDS: lowering x max_parts x multi_value"""
    pattern, n, lo, hi, engine, grammar = source
    return [(pattern, n, lo, hi, engine, grammar, lowering, parts, mv)
            for lowering in LOWERINGS for parts in MAX_PARTS for mv in MULTI_VALUE]


def digest(case):
    """SHA-256 of the case's schedule, or the class name of the exception it raises"""
    pattern, n, lo, hi, engine, grammar, lowering, parts, mv = case
    try:
        S = F.schedule_match(n, pattern, lo, hi, lowering=lowering, engine=engine, grammar=grammar,
                             multi_value=bool(mv), max_parts=parts)
    except Exception as e:  # noqa: BLE001  (whatever it raises is the case's record)
        return type(e).__name__
    h = hashlib.sha256()
    for j in S.jobs:
        h.update(ctypes.string_at(ctypes.addressof(j), ctypes.sizeof(j)))
    h.update(struct.pack(f"<{len(S.level_off)}I", *S.level_off))
    for p in S.parts:
        h.update(struct.pack("<3i", *p))
    return h.hexdigest()


def digests(cases):
    """digest() of each case; the recordings are independent and the library releases the GIL,
    so they run on a thread pool (eight workers at most: the largest recordings hold ~1 GB each)"""
    from concurrent.futures import ThreadPoolExecutor
    F.lib()
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(digest, cases))


def main():
    src = sources()
    got = digests([c for s in src for c in cases_of(s)])
    k = len(cases_of(src[0]))
    with open(OUT, "w") as f:
        f.write('{"generator": "tests/golden/make_schedule_digests.py",\n')
        f.write(' "fields": %s,\n' % json.dumps(FIELDS))
        f.write(' "lowering": %s, "max_parts": %s, "multi_value": %s,\n'
                % (json.dumps(LOWERINGS), json.dumps(MAX_PARTS), json.dumps(MULTI_VALUE)))
        f.write(' "sources_are": "pattern, n_chars, lo, hi, engine, grammar, the distinct digests of the '
                'source, and per case (lowering x max_parts x multi_value, the last fastest) its digest\'s index",\n')
        f.write(' "sources": [\n')
        rows = []
        for i, s in enumerate(src):
            ds = got[k * i:k * (i + 1)]
            distinct = sorted(set(ds), key=ds.index)
            rows.append("  " + json.dumps(list(s) + [distinct, [distinct.index(d) for d in ds]]))
        f.write(",\n".join(rows))
        f.write("\n ]}\n")
    print(f"{len(src)} sources, {len(got)} cases -> {OUT}")


def load():
    """the stored cases and their digests: [(case tuple, digest)]"""
    with open(OUT) as f:
        doc = json.load(f)
    assert (doc["fields"], doc["lowering"], doc["max_parts"], doc["multi_value"]) == \
        (list(FIELDS), list(LOWERINGS), list(MAX_PARTS), list(MULTI_VALUE))
    out = []
    for row in doc["sources"]:
        cs = cases_of(tuple(row[:6]))
        assert len(row[7]) == len(cs)
        out += [(c, row[6][i]) for c, i in zip(cs, row[7])]
    return out


if __name__ == "__main__":
    main()
