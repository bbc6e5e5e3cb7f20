"""Generates tests/golden/wire_digests.json: the seven wire blobs (include/fheregex.h), byte
for byte, and which damaged blobs their checkers accept.

Host-only contexts (no device), fixed integer seeds, at the FFT points (1, 2048) and (2, 1024)
and, for the formats every ring carries, at the RNS point (1, 2048).  Per point and blob:

- its length, its header in hex and the BLAKE2b-256 of the whole blob;
- the acceptance matrix of the entry that checks it (FORMATS below): for every header byte, the
  blob with bit 0 and with bit 7 of that byte flipped, and the blob at the lengths 0, header
  only, exact - 1, exact + 1 and exact + 8 (the added bytes zero).  Each cell is the call's
  return code and, when refused, its message, so a refactor keeps the codes and the texts.
  The mask key's 32 bytes are free bits: the key formats, whose accepted blob is expanded in
  full at seconds apiece, flip its first byte only; the others flip all of them.

FRPKRES1 appears once (fr_pack_bools_blob), FRCPRES1 twice: fr_pack_bools_compact's blob and
fr_compress_packed's go through two writers.  The FFT-only formats are recorded at the RNS
point as the refusal of their size or encrypt call.

tests/test_wire_golden.py recomputes all of it and compares for equality: a refactor of the
wire layer must leave the file as it is.  Regenerate only when a format is meant to change,
with the library of the revision that defines it, from the repo root:
    python3 tests/golden/make_wire_digests.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "fhe-regex_amd")]
import fheregex as F  # noqa: E402

OUT = os.path.join(HERE, "wire_digests.json")
POINTS = [(1, 2048, F.RING_FFT), (2, 1024, F.RING_FFT), (1, 2048, F.RING_RNS)]
SEED_CLIENT, SEED_SERVER, SEED_PACKING, SEED_CONTENT, SEED_NEEDLE = 7, 11, 13, 17, 19
CONTENT = "wire layer"
NEEDLE = "a?c"
BITS = (0, 7)
# blob name -> (header bytes, mask key's offset or None, a key format, the checking entry)
FORMATS = {
    "FRCSKEY1": (72, 40, True, "fr_load_server_key_compact"),
    "FRCCTXT1": (64, 32, False, "fr_expand_compact_content"),
    "FRPKKEY1": (48, None, True, "fr_load_packing_key"),
    "FRCPKEY1": (96, 56, True, "fr_load_packing_key_compact"),
    "FRPKRES1": (24, None, False, "fr_decrypt_packed"),
    "FRCPRES1": (32, None, False, "fr_expand_packed_compact"),
    "FRCPRES1/compress": (32, None, False, "fr_expand_packed_compact"),
    "FRNEEDL1": (64, 24, False, "fr_expand_needle"),
}


def point_id(point):
    k, N, ring = point
    return f"k{k}n{N}" + ("" if ring == F.RING_FFT else "rns")


def context(point):
    k, N, ring = point
    return F.Context(device=-1, params=F.default_params(k=k, N=N, ring=ring))


def u8(blob):
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy() if not isinstance(blob, np.ndarray) else blob.copy()


def refusal(fn):
    """the [code, message] of the FheRegexError fn() raises"""
    try:
        fn()
    except F.FheRegexError as e:
        return [e.code, str(e)]
    raise AssertionError("accepted")


def blobs(point, client):
    """name -> uint8 array, or the [code, message] of the refusal, on a context holding the keys"""
    fft = point[2] == F.RING_FFT
    out = {}
    if fft:
        client.gen_server_key(SEED_SERVER, compact=True)
        out["FRCSKEY1"] = u8(client.export_server_key_compact())
    else:
        out["FRCSKEY1"] = refusal(client.server_key_compact_size)
    out["FRCCTXT1"] = u8(client.encrypt_str_compact(CONTENT, seed=SEED_CONTENT))
    client.gen_packing_key(SEED_PACKING)
    out["FRPKKEY1"] = client.export_packing_key()
    # trivial booleans are the handles a host-only context has: the words do not depend on the key
    zero = client.or_many([])
    one = client.not_(zero)
    hs = [one, zero, one, one, zero]
    out["FRPKRES1"] = u8(client.pack_bools(hs))
    out["FRCPRES1"] = u8(client.pack_bools_compact(hs))
    W = (point[0] + 1) * point[1]
    words = (np.arange(1, W + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    out["FRCPRES1/compress"] = u8(client.compress_packed(words, 33))
    client.gen_packing_key(SEED_PACKING, compact=True)
    out["FRCPKEY1"] = client.export_packing_key_compact()
    masks = F.needle_masks(NEEDLE, any_char="?")
    if fft:
        out["FRNEEDL1"] = u8(client.encrypt_needle(masks, seed=SEED_NEEDLE))
    else:
        out["FRNEEDL1"] = refusal(lambda: client.encrypt_needle(masks, seed=SEED_NEEDLE))
    return out


class Checker:
    """the entry that checks a format, on a keyless server context (fr_decrypt_packed, which
    needs the client's key for the bits, as the size query that stops after the check)"""

    def __init__(self, point, client):
        self.server = context(point)
        self.client = client
        self.n = C.c_size_t()
        self.words = np.zeros(2 * 64 * (point[0] + 1) * point[1], dtype=np.uint64)  # a needle's at most

    def __call__(self, entry, buf, length):
        L, p, n = F.lib(), C.cast(buf.ctypes.data, C.c_char_p), C.byref(self.n)
        h = self.server.h
        if entry == "fr_expand_compact_content":
            rc = L.fr_expand_compact_content(h, p, length, F._p(self.words), len(self.words), n)
        elif entry == "fr_expand_needle":
            rc = L.fr_expand_needle(h, p, length, F._p(self.words), len(self.words), n)
        elif entry == "fr_expand_packed_compact":
            rc = L.fr_expand_packed_compact(h, p, length, F._p(self.words), n)
        elif entry == "fr_decrypt_packed":
            rc = L.fr_decrypt_packed(self.client.h, p, length, None, n)
        else:
            rc = getattr(L, entry)(h, p, length)
        return rc if rc == F.FR_OK else [rc, L.fr_last_error().decode()]


def acceptance(name, blob, check):
    """{"flips": [[offset, bit, result]], "lengths": [[length, result]]}, result 0 or [code, message]"""
    header, mk, is_key, entry = FORMATS[name]
    exact = len(blob)
    buf = np.concatenate([blob, np.zeros(8, dtype=np.uint8)])  # room for exact + 8
    assert check(entry, buf, exact) == F.FR_OK, name
    flips = []
    for off in range(header):
        in_mask_key = mk is not None and mk <= off < mk + 32
        for bit in BITS:
            if in_mask_key and is_key and (off, bit) != (mk, BITS[0]):
                continue
            buf[off] ^= 1 << bit
            flips.append([off, bit, check(entry, buf, exact)])
            buf[off] ^= 1 << bit
    lengths = [[n, check(entry, buf, n)] for n in (0, header, exact - 1, exact + 1, exact + 8)]
    assert np.array_equal(buf[:exact], blob)
    return {"flips": flips, "lengths": lengths}


def record(point):
    """the stored entry of one point"""
    client = context(point)
    client.gen_client_key(SEED_CLIENT)
    check = Checker(point, client)
    rec = {}
    for name, blob in blobs(point, client).items():
        if isinstance(blob, list):
            rec[name] = {"refused": blob}
            continue
        header = FORMATS[name][0]
        rec[name] = {"length": len(blob), "header": bytes(blob[:header]).hex(),
                     "blake2b": hashlib.blake2b(blob, digest_size=32).hexdigest(),
                     "entry": FORMATS[name][3], **acceptance(name, blob, check)}
    return rec


def load():
    """the stored points, every result index replaced by its result"""
    with open(OUT) as f:
        doc = json.load(f)
    res = doc["results"]
    for rec in doc["points"].values():
        for b in rec.values():
            for key in ("flips", "lengths"):
                if key in b:
                    b[key] = [row[:-1] + [res[row[-1]]] for row in b[key]]
    return doc["points"]


def main():
    points = {point_id(p): record(p) for p in POINTS}
    results = []  # the distinct cells (0 or [code, message]); the matrices hold indices into them
    for rec in points.values():
        for b in rec.values():
            for key in ("flips", "lengths"):
                for row in b.get(key, []):
                    if row[-1] not in results:
                        results.append(row[-1])
                    row[-1] = results.index(row[-1])
    with open(OUT, "w") as f:
        f.write('{"generator": "tests/golden/make_wire_digests.py",\n')
        f.write(' "seeds": %s,\n' % json.dumps({"client": SEED_CLIENT, "server": SEED_SERVER, "packing": SEED_PACKING,
                                               "content": SEED_CONTENT, "needle": SEED_NEEDLE}))
        f.write(' "cells_are": "flips: [header offset, bit, result], lengths: [length, result]; a result is an '
                'index into results: 0 (accepted) or [code, message]",\n')
        f.write(' "results": [\n%s\n ],\n' % ",\n".join("  " + json.dumps(r) for r in results))
        f.write(' "points": {\n')
        f.write(",\n".join('  %s: {\n%s\n  }' % (json.dumps(pid), ",\n".join(
            "   %s: %s" % (json.dumps(name), json.dumps(b)) for name, b in rec.items())) for pid, rec in points.items()))
        f.write("\n }}\n")
    print(f"{len(POINTS)} points -> {OUT}")


if __name__ == "__main__":
    main()
