"""The compact packed result on host-only contexts: sizes, the rounding rule, decryption and
the error the rounding adds, affine and constant inputs, the wire checks and the reply framing.

A packed boolean is never bootstrapped again, so only the client's rounding at 2^58 sees its
error.  Every sent coefficient travels as v = ((x + 2^47) >> 48) mod 2^16 and is installed as
v << 48: a uniform error of std 2^48 / sqrt(12) per coefficient, reaching the phase through the
body coefficient and the h set bits of the key, so the rounding adds std sqrt((h + 1) / 12) 2^48
(2^51.2 at h = 1024).  The std bound below is that figure with 10% for the sampling spread of a
std over >= 1,024 coefficients (about 2.2% at one sigma); the bound on the largest total error,
2^54, is four bits under the threshold.

Measured on the host at n = N (seeds below): the added std is 2^50.79 at (1, 2048) and 2^51.00
at (2, 1024) against bounds of 2^51.35; the largest total error over n = 1, 33, N is 2^52.70.
"""
import struct

import numpy as np
import pytest

import fheregex as F
from pack_oracle import round16  # the rule, restated: ((x + 2^47) >> 48) mod 2^16

POINTS = [(1, 2048), (2, 1024)]
POINT_IDS = ["k1n2048", "k2n1024"]
PSEED = 0x9AC4
DELTA_LOG = 59


def host(point, key_blob):
    k, N = point
    ctx = F.Context(device=-1, params=F.default_params(k=k, N=N))
    if k == 1:
        ctx.load_client_key(key_blob)
    else:
        ctx.gen_client_key(7)
    return ctx


def weight(ctx):
    """the big key's weight from the bincode client key: u64 length, then the words"""
    blob = ctx.serialize_client_key()
    (n,) = struct.unpack_from("<Q", blob, 0)
    return int(np.frombuffer(blob, dtype="<u8", count=n, offset=8).sum())


def signed(x):
    return np.asarray(x, dtype=np.uint64).astype(np.int64)


class Keyed:
    """a client context with the host-generated packing key, and the packs the tests share:
    n fresh encryptions through pack_lwes, computed once per n and never changed"""

    def __init__(self, point, key_blob):
        self.k, self.N = point
        self.ctx = host(point, key_blob)
        self.ctx.gen_packing_key(PSEED)
        self._packs = {}

    def pack(self, n):
        if n not in self._packs:
            bits = np.random.default_rng(300 + n).integers(0, 2, n).astype(np.uint8)
            lwes = self.ctx.encrypt_blocks(bits, seed=77).reshape(n, -1)
            words = self.ctx.pack_lwes(lwes)
            words.setflags(write=False)
            self._packs[n] = (bits, words)
        return self._packs[n]


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def keyed(request, key_blob):
    return Keyed(request.param, key_blob)


def header(k, N, n, magic=b"FRCPRES1", bits=16, reserved=0):
    return magic + struct.pack("<iiQII", k, N, n, bits, reserved)


def test_sizes(keyed):
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    for n in (1, 256, N):
        assert ctx.packed_compact_size(n) == 32 + 2 * (k * N + n)
    if (k, N) == (1, 2048):
        assert [ctx.packed_compact_size(n) for n in (1, 256, 2048)] == [4130, 4640, 8224]
    for n in (0, N + 1):
        with pytest.raises(F.FheRegexError) as e:
            ctx.packed_compact_size(n)
        assert e.value.code == F.ERR_INVALID


@pytest.mark.parametrize("n", [1, 33, "N"])
def test_rounding_rule(keyed, n):
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    n = N if n == "N" else n
    _, words = keyed.pack(n)
    blob = ctx.compress_packed(words, n)
    assert len(blob) == 32 + 2 * (k * N + n) and blob[:32] == header(k, N, n)
    sent = k * N + n
    assert np.array_equal(np.frombuffer(blob, dtype="<u2", offset=32), round16(words[:sent]))
    back, got_n = ctx.expand_packed_compact(blob)
    assert got_n == n and len(back) == (k + 1) * N
    assert np.array_equal(back[:sent], round16(words[:sent]).astype(np.uint64) << np.uint64(48))
    assert not back[sent:].any()
    # the rule at its edges: a word just under a half rounds down, a half up, the top wraps to 0
    edge = np.zeros((k + 1) * N, dtype=np.uint64)
    edge[:4] = [(1 << 47) - 1, 1 << 47, (0xFFFF << 48) + (1 << 47), (0xFFFF << 48) + (1 << 47) - 1]
    assert list(np.frombuffer(ctx.compress_packed(edge, 1), dtype="<u2", offset=32)[:4]) == [0, 1, 0, 0xFFFF]


@pytest.mark.parametrize("n", [1, 33, "N"])
def test_decrypt_and_added_error(keyed, n):
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    n = N if n == "N" else n
    bits, words = keyed.pack(n)
    blob = ctx.compress_packed(words, n)
    assert ctx.decrypt_packed_compact(blob) == list(bits)
    expanded, _ = ctx.expand_packed_compact(blob)
    # the first n coefficients of the body were sent; the phase of a used coefficient sees the
    # body's own rounding and the masks' through the key
    ph_full, ph_comp = ctx.packed_phase(words), ctx.packed_phase(expanded)
    added = signed(ph_comp - ph_full)[:n]
    total = signed(ph_comp)[:n] - (bits.astype(np.int64) << DELTA_LOG)
    h = weight(ctx)
    assert k * N // 4 < h < 3 * k * N // 4
    model = np.sqrt((h + 1) / 12.0) * 2.0 ** 48
    std = float(np.sqrt(np.mean(added.astype(np.float64) ** 2)))
    worst = int(np.abs(total).max())
    print(f"(k, N) = ({k}, {N}), n = {n}, h = {h}: added std 2^{np.log2(max(std, 1)):.2f} "
          f"(model 2^{np.log2(model):.2f}), largest total error 2^{np.log2(max(worst, 1)):.2f}")
    if n == N:
        assert std < 1.1 * model
        assert std > 0.5 * model  # (the rounding is really there)
    assert worst < 2 ** 54


def test_affine_and_constant_inputs(keyed):
    """1 - x packs to the negated bit, a constant to itself, its LWE unread"""
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    bits = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    lwes = ctx.encrypt_blocks(bits, seed=5).reshape(5, -1)
    w = [1, -1, -1, 0, 0]
    off = [0, 2, 2, 2, 0]  # units of Delta / 2
    words = ctx.pack_lwes(lwes, w, off)
    assert ctx.decrypt_packed_compact(ctx.compress_packed(words, 5)) == [1, 1, 0, 1, 0]
    # constants alone: a zero mask, and bodies that are exact in 16 bits
    only = ctx.pack_lwes(None, [0, 0, 0], [2, 0, 2], n=3)
    blob = ctx.compress_packed(only, 3)
    vals = np.frombuffer(blob, dtype="<u2", offset=32)
    assert not vals[:k * N].any() and list(vals[k * N:]) == [1 << (DELTA_LOG - 48), 0, 1 << (DELTA_LOG - 48)]
    assert np.array_equal(ctx.expand_packed_compact(blob)[0], only)
    # a trivial boolean handle is such a constant (the only handle a host-only context has)
    one, zero = ctx.not_(ctx.or_many([])), ctx.or_many([])
    assert ctx.pack_bools_compact([one, zero, one]) == blob
    assert ctx.decrypt_packed_compact(ctx.pack_bools_compact([one])) == [1]
    with pytest.raises(F.FheRegexError) as e:
        ctx.pack_bools_compact([ctx.trivial(5)])  # a radix handle
    assert e.value.code == F.ERR_INVALID
    keyless = F.Context(device=-1, params=F.default_params(k=k, N=N))  # no packing key
    with pytest.raises(F.FheRegexError) as e:
        keyless.pack_bools_compact([keyless.or_many([])])
    assert e.value.code == F.ERR_INVALID and "packing key" in str(e.value)


def test_wire_refusals(keyed):
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    bits, words = keyed.pack(33)
    blob = ctx.compress_packed(words, 33)
    body = blob[32:]
    assert ctx.decrypt_packed_compact(blob) == list(bits)
    ok, oN = (2, 1024) if k == 1 else (1, 2048)
    full = b"FRPKRES1" + struct.pack("<iiQ", k, N, 33) + words.tobytes()
    bad = {
        "truncated": blob[:-1],
        "appended": blob + b"\0",
        "header only": blob[:31],
        "magic": b"FRCPRES2" + blob[8:],
        "full magic, compact body": b"FRPKRES1" + blob[8:],
        "other point": header(ok, oN, 33) + body,
        "other point, its own length": header(ok, oN, 33) + bytes(2 * (ok * oN + 33)),
        "n = 0": header(k, N, 0) + body,
        "n = 0, its own length": header(k, N, 0) + bytes(2 * k * N),
        "n = N + 1": header(k, N, N + 1) + body,
        "n = N + 1, its own length": header(k, N, N + 1) + bytes(2 * (k * N + N + 1)),
        "n = 34, this length": header(k, N, 34) + body,
        "bits 15": header(k, N, 33, bits=15) + body,
        "bits 32": header(k, N, 33, bits=32) + body,
        "reserved": header(k, N, 33, reserved=1) + body,
        "a full blob": full,
    }
    for name, b in bad.items():
        for call in (ctx.decrypt_packed_compact, ctx.expand_packed_compact):
            with pytest.raises(F.FheRegexError) as e:
                call(b)
            assert e.value.code == F.ERR_INVALID, name
    # ... and the full form's decryption keeps refusing the compact blob
    assert ctx.decrypt_packed(full) == list(bits)
    with pytest.raises(F.FheRegexError) as e:
        ctx.decrypt_packed(blob)
    assert e.value.code == F.ERR_INVALID
    # no client key: the blob is checked first, then the key is missed
    server = F.Context(device=-1, params=F.default_params(k=k, N=N))
    with pytest.raises(F.FheRegexError) as e:
        server.decrypt_packed_compact(blob)
    assert e.value.code == F.ERR_NO_KEY
    assert np.array_equal(server.expand_packed_compact(blob)[0], ctx.expand_packed_compact(blob)[0])
    with pytest.raises(ValueError):
        ctx.compress_packed(words[:-1], 33)
    for n in (0, N + 1):
        with pytest.raises(F.FheRegexError) as e:
            ctx.compress_packed(words, n)
        assert e.value.code == F.ERR_INVALID


def test_reply_framing(keyed):
    """ClientKey.decrypt_starts tells the two reply forms apart by their first word"""
    k, N, ctx = keyed.k, keyed.N, keyed.ctx
    ck = F.ClientKey(ctx)
    (b1, w1), (b2, w2) = keyed.pack(N), keyed.pack(33)
    c1, c2 = ctx.compress_packed(w1, N), ctx.compress_packed(w2, 33)
    want = [j for j in range(N) if b1[j]] + [N + j for j in range(33) if b2[j]]
    assert any(o >= N for o in want)
    reply = struct.pack("<II", 0xFFFFFFFF, 2) + c1 + c2
    assert ck.decrypt_starts(reply) == want
    assert ck.decrypt_starts(struct.pack("<II", 0xFFFFFFFF, 1) + c2) == [j for j in range(33) if b2[j]]
    assert ck.decrypt_starts(struct.pack("<II", 0xFFFFFFFF, 0)) == []  # an empty content
    # a chunk whose header or body overruns the reply, a missing chunk, bytes left over
    for bad in (reply[:-1], reply[:8 + len(c1) + 31], struct.pack("<II", 0xFFFFFFFF, 3) + c1 + c2, reply + b"\0",
                struct.pack("<I", 0xFFFFFFFF), struct.pack("<II", 0xFFFFFFFF, 1) + header(k, N, N) + c2[32:]):
        with pytest.raises(ValueError):
            ck.decrypt_starts(bad)
    # a chunk that is delimited but is no compact blob is the library's to refuse
    with pytest.raises(F.FheRegexError):
        ck.decrypt_starts(struct.pack("<II", 0xFFFFFFFF, 1) + header(k, N, 33, bits=15) + c2[32:])
    # the full form's framing decodes through the same call
    full = [b"FRPKRES1" + struct.pack("<iiQ", k, N, len(b)) + w.tobytes() for b, w in ((b1, w1), (b2, w2))]
    assert ck.decrypt_starts(struct.pack("<I", 2) + full[0] + full[1]) == want
    assert ck.decrypt_starts(struct.pack("<I", 0)) == []
