"""The compact reply on the device, both FFT points and one pack on the RNS ring.

k_pack_compress against the host's compress_packed, byte for byte, at the sizes where its
tail changes (kN + n a multiple of its eight values per store or not); fr_match_starts_packed
against fr_match_starts + fr_pack_bools_blob (+ compress_packed) in both reply forms, its plan
shared with fr_match_starts, without a handle or an arena slot, and on lanes; the error of a
compact reply of real bootstrap outputs; and a keyless server answering in the compact form.

The bound on that error is derived, not tuned: the worst bootstrap output of DESIGN §7, 2^52.2,
plus the worst rounding measured on the host (tests/test_compact_reply.py), 2^52.7, is under
2^53.5; 2^55 leaves a bit and a half and is three bits under the threshold 2^58.  Measured on
an MI355X for the 16 starts of /abc/ below: 2^52.64 at (1, 2048), 2^52.09 at (2, 1024).
"""
import numpy as np
import pytest

import fheregex as F
from test_packed_results_gpu import POINT_IDS, POINTS, PSEED, Pair, make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def pair(request, key_blob):
    """as tests/test_packed_results_gpu.py's: a host client and a device context with the same
    client key and packing key"""
    p = Pair(request.param, key_blob)
    yield p
    # every slot the tests took has been returned (the cached plans give theirs back first)
    p.dev.set_plan_cache(0)
    st = p.dev.arena_stats()
    assert st["slots"] == st["free_slots"], st
    assert p.dev.handle_count() == 0
    p.dev.close()


CONTENT = "xabcabx".ljust(16, "x")
K = bytes((29 * i + 5) & 0xFF for i in range(32))   # the keyless server's packing key
KS = bytes((37 * i + 11) & 0xFF for i in range(32))  # ... and its server key
DELTA_LOG = 59


def starts_of(content, pattern):
    return [s for s, v in enumerate(F.plain_match_starts(content, pattern)[1]) if v]


@pytest.fixture(scope="module")
def chars(pair):
    hs = pair.dev.upload_radix(pair.host.encrypt_str(CONTENT, seed=8))
    yield hs
    for h in hs:
        pair.dev.release(h)


def in_use(dev):
    st = dev.arena_stats()
    return st["slots"] - st["free_slots"]


@pytest.mark.parametrize("n", [1, 3, 33, "N"])
def test_device_compress_equals_host(pair, n):
    """n = 1: one boolean; 3: a body tail shorter than one store, with a negated handle and a
    trivial constant; 33: one row tile plus one; N: the full body, no tail"""
    dev, host = pair.dev, pair.host
    n = pair.N if n == "N" else n
    bits = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    up = dev.upload_bool(host.encrypt_blocks(bits, seed=13).reshape(n, -1))
    handles, want_bits, owned = list(up), [int(b) for b in bits], list(up)
    if n == 3:
        zero = dev.or_many([])
        owned.append(zero)
        handles[1] = dev.not_(up[1])  # 1 - x
        handles[2] = dev.not_(zero)   # the trivial constant 1
        want_bits[1:] = [1 - want_bits[1], 1]
    got = dev.pack_bools_compact(handles)
    want = host.compress_packed(dev.pack_bools_words(handles), n)
    assert len(got) == dev.packed_compact_size(n) == 32 + 2 * (host.params.k * pair.N + n)
    assert got == want, (n, sum(a != b for a, b in zip(got, want)))
    assert host.decrypt_packed_compact(got) == want_bits
    for h in set(handles + owned):
        dev.release(h)


@pytest.mark.parametrize("pattern", ["/abc/", "/^abc/"])
def test_match_starts_packed_equals_two_steps(pair, chars, pattern):
    """/abc/: affine outputs over the plan's gates and two constant starts at the end;
    /^abc/: every start past the first a constant"""
    dev, host = pair.dev, pair.host
    hs = dev.match_starts(chars, pattern)
    two_full = dev.pack_bools(hs)
    two_compact = host.compress_packed(dev.pack_bools_words(hs), len(hs))
    for h in hs:
        dev.release(h)
    assert dev.match_starts_packed(chars, pattern, compact=False) == two_full
    got = dev.match_starts_packed(chars, pattern, compact=True)
    assert got == two_compact
    want = F.plain_match_starts(CONTENT, pattern)[1]
    assert host.decrypt_packed_compact(got) == want == host.decrypt_packed(two_full)
    assert starts_of(CONTENT, pattern) == ([1] if pattern == "/abc/" else [])
    # a sub-range of starts is the slice
    assert host.decrypt_packed_compact(dev.match_starts_packed(chars, pattern, 1, 6)) == want[1:6]


def test_plan_is_cached_and_shared_with_match_starts(pair, chars):
    dev = pair.dev
    a, st_a = dev.match_starts_packed(chars, "/bca/", stats=True)
    b, st_b = dev.match_starts_packed(chars, "/bca/", stats=True)
    assert (st_a.plan_cached, st_b.plan_cached) == (0, 1) and a == b and st_b.pbs == st_a.pbs > 0
    hs, st_c = dev.match_starts(chars, "/bca/", stats=True)  # one plan serves both calls
    assert st_c.plan_cached == 1
    for h in hs:
        dev.release(h)
    full, st_d = dev.match_starts_packed(chars, "/bca/", compact=False, stats=True)
    assert st_d.plan_cached == 1 and full[:8] == b"FRPKRES1" and a[:8] == b"FRCPRES1"


def test_no_slots_and_no_handles(pair, chars):
    dev = pair.dev
    dev.match_starts_packed(chars, "/abc/")  # the plan is cached from here
    before = (in_use(dev), dev.handle_count())
    blob, st = dev.match_starts_packed(chars, "/abc/", stats=True)
    assert st.plan_cached == 1
    assert (in_use(dev), dev.handle_count()) == before
    # the two-step path holds a handle per start, and a slot per start that is no constant
    hs = dev.match_starts(chars, "/abc/")
    during = (in_use(dev), dev.handle_count())
    assert during[1] == before[1] + 16 and during[0] >= before[0] + 14
    for h in hs:
        dev.release(h)
    assert (in_use(dev), dev.handle_count()) == before


def test_lanes(pair, chars):
    """four packed matches of two patterns round-robin over three lanes, an asynchronous
    has_match between them: the bytes of the same calls on a context without lanes"""
    dev, host = pair.dev, pair.host
    patterns = ["/abc/", "/ab/", "/abc/", "/ab/"]
    serial = [dev.match_starts_packed(chars, p) for p in patterns]
    dev.set_lanes(3)
    dev.set_async(True)
    flags = []
    try:
        got = []
        for p in patterns:
            got.append(dev.match_starts_packed(chars, p))
            flags.append(dev.has_match(chars, "/bc/")[0])  # enqueued, not waited for
        assert got == serial
        assert host.decrypt_packed_compact(got[1]) == F.plain_match_starts(CONTENT, "/ab/")[1]
        assert [host.decrypt_radix(dev.download_radix(h)) for h in flags] == [1, 1, 1, 1]
    finally:
        dev.set_lanes(1)
        for h in flags:
            dev.release(h)


def test_error_of_real_bootstrap_outputs(pair, chars):
    dev, host = pair.dev, pair.host
    blob = dev.match_starts_packed(chars, "/abc/")
    words, n = host.expand_packed_compact(blob)
    assert n == 16
    want = np.array(F.plain_match_starts(CONTENT, "/abc/")[1], dtype=np.int64) << DELTA_LOG
    err = host.packed_phase(words).astype(np.int64)[:n] - want
    worst = int(np.abs(err).max())
    print(f"(k, N) = ({host.params.k}, {pair.N}): largest distance of a used coefficient from its bit "
          f"2^{np.log2(max(worst, 1)):.2f}")
    assert worst < 2 ** 55


def test_keyless_server_replies_compact(pair, key_blob):
    """the server holds a compact server key, a compact packing key and compact content, and
    nothing of the client's"""
    host = pair.host
    k, N = host.params.k, pair.N
    gen = make((F.RING_FFT, k, N), key_blob, 0)
    gen.gen_server_key(KS, compact=True)
    gen.gen_packing_key(K, compact=True)
    server = F.Context(device=0, params=F.default_params(k=k, N=N))
    server.load_server_key_compact(gen.export_server_key_compact())
    server.load_packing_key_compact(gen.export_packing_key_compact())
    gen.close()
    with pytest.raises(F.FheRegexError):
        server.serialize_client_key()
    ck, sk = F.ClientKey(host), F.ServerKey(server)
    hs = sk.upload_str(ck.encrypt_str_compact(CONTENT, seed=3))
    reply = sk.match_starts(hs, "/abc/", compact=True)
    assert len(reply) == 8 + 32 + 2 * (k * N + 16)
    assert ck.decrypt_starts(reply) == [1]
    assert ck.decrypt_starts(sk.match_starts(hs, "/abc/")) == [1]  # the default form, as before
    assert sk.match_starts([], "/abc/", compact=True) == b"\xff\xff\xff\xff\0\0\0\0"
    assert ck.decrypt_starts(sk.match_starts([], "/abc/", compact=True)) == []
    for h in hs:
        server.release(h)
    if (k, N) == (2, 1024):  # two chunks: N + 8 characters, a match in each
        text = list("x" * (N + 8))
        text[5:8] = text[N + 2:N + 5] = "abc"
        text = "".join(text)
        hs = sk.upload_str(ck.encrypt_str_compact(text, seed=4))
        reply = sk.match_starts(hs, "/abc/", compact=True)
        assert len(reply) == 8 + (32 + 2 * (k * N + N)) + (32 + 2 * (k * N + 8))
        assert ck.decrypt_starts(reply) == [5, N + 2]
        for h in hs:
            server.release(h)
    # without a packing key the call refuses before anything is launched
    bare = make((F.RING_FFT, k, N), key_blob, 0)
    bare.gen_server_key(KS)
    with pytest.raises(F.FheRegexError) as e:
        bare.match_starts_packed(bare.upload_radix(host.encrypt_str("ab", seed=1)), "/a/")
    assert e.value.code == F.ERR_INVALID and "packing key" in str(e.value)
    assert bare.plan_cache_stats()["misses"] == 0
    bare.close()
    server.set_plan_cache(0)
    st = server.arena_stats()
    assert st["slots"] == st["free_slots"], st
    server.close()


def test_rns_point_packs_compact_and_decrypts(key_blob):
    point = (F.RING_RNS, 1, 2048)
    host, dev = make(point, key_blob, -1), make(point, key_blob, 0)
    dev.gen_packing_key(PSEED)
    bits = [1, 0, 0, 1, 1, 0, 1]
    hs = dev.upload_bool(host.encrypt_blocks(bits, seed=5).reshape(len(bits), -1))
    blob = dev.pack_bools_compact(hs)
    assert len(blob) == 32 + 2 * (2048 + 7)
    assert blob == host.compress_packed(dev.pack_bools_words(hs), len(bits))
    assert host.decrypt_packed_compact(blob) == bits
    for h in hs:
        dev.release(h)
    st = dev.arena_stats()
    assert st["slots"] == st["free_slots"], st
    dev.close()
