"""Compact content on the device: k_expand_blocks rebuilds every mask word of a blob in fresh
arena slots (both FFT points and the RNS ring), word for word the host expansion.

Covers: block and string blobs, a ChaCha counter above 32 bits, slots taken from a
fragmented free list, an upload that grows (and so moves) the arena before and after other
content is resident, matches on expanded content (the words of the same LWEs uploaded the
ordinary way), ordering against asynchronous matches on four lanes, and a server that holds
neither a client key nor a full-size key.  Server keys are generated on the device from a
seed.
"""
import ctypes as C

import numpy as np
import pytest

import fheregex as F
import regex_oracle as ro

K = bytes((41 * i + 7) & 0xFF for i in range(32))
SEED = 42
POINTS = [(F.RING_FFT, 1, 2048), (F.RING_FFT, 2, 1024), (F.RING_RNS, 1, 2048)]
POINT_IDS = ["fft", "fft-k2n1024", "rns"]
FFT_POINTS, FFT_IDS = POINTS[:2], POINT_IDS[:2]

pytestmark = pytest.mark.gpu


def make(point, key_blob, device, server_key=False):
    ring, k, N = point
    ctx = F.Context(device=device, params=F.default_params(k=k, N=N, ring=ring))
    if key_blob is not None:
        ctx.load_client_key(key_blob)
    if server_key:
        ctx.gen_server_key(SEED)
    return ctx


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def pair(request, key_blob):
    """(host client, device context without any key) at every point"""
    return make(request.param, key_blob, -1), make(request.param, None, 0)


@pytest.fixture(scope="module", params=FFT_POINTS, ids=FFT_IDS)
def keyed(request, key_blob):
    """(host client, device context with a device-generated server key)"""
    return make(request.param, key_blob, -1), make(request.param, key_blob, 0, server_key=True)


def text(rng, n, planted):
    s = "".join(chr(c) for c in rng.integers(0x20, 0x7F, n)).replace("a", "x")
    return s[:5] + "abc" + s[8:] if planted else s


def test_words(pair):
    client, dev = pair
    for nb in (1, 3, 5):
        for first in (0, 2 ** 33 + 5):
            blob = client.encrypt_blocks_compact([(3 * q + nb) % 16 for q in range(nb)], K, first)
            want = client.expand_compact_content(blob)
            hs = dev.upload_compact_blocks(blob)
            assert len(hs) == nb
            for q, h in enumerate(hs):
                assert np.array_equal(dev.download_radix(h)[0], want[q]), (nb, first, q)
    for s in ("Q", "0123abc789abcdef"):
        blob = client.encrypt_str_compact(s, K)
        want = client.expand_compact_content(blob).reshape(len(s), 4, -1)
        hs = dev.upload_compact_str(blob)
        assert len(hs) == len(s)
        for i, h in enumerate(hs):
            assert np.array_equal(dev.download_radix(h), want[i]), (s, i)
    assert dev.upload_compact_str(client.encrypt_str_compact("", K)) == []
    # refused before a slot or a handle is taken: a block blob through the string entry, a
    # bad magic, cap one short -- the next upload gets the handles the last one gave back
    probe = client.encrypt_blocks_compact([1, 2, 3], K)
    before = dev.upload_compact_blocks(probe)
    for h in before:
        dev.release(h)
    for bad in (probe, b"FRCCTXT2" + blob[8:]):
        with pytest.raises(F.FheRegexError) as e:
            dev.upload_compact_str(bad)
        assert e.value.code == F.ERR_INVALID
    n, out = C.c_size_t(), (C.c_uint32 * 16)()
    assert F.lib().fr_upload_compact_str(dev.h, blob, len(blob), out, 15, C.byref(n)) == F.ERR_INVALID
    assert n.value == 16
    assert F.lib().fr_upload_compact_blocks(dev.h, probe, len(probe), out, 2, C.byref(n)) == F.ERR_INVALID
    assert sorted(dev.upload_compact_blocks(probe)) == sorted(before)


def test_fragmented_slots(pair):
    client, dev = pair
    first = client.encrypt_str("ABCDEFGH", seed=3)
    hs = dev.upload_radix(first)
    for i in (1, 3, 6):
        dev.release(hs[i])
    blob = client.encrypt_str_compact("fresh", K)
    want = client.expand_compact_content(blob).reshape(5, 4, -1)
    new = dev.upload_compact_str(blob)
    for i, h in enumerate(new):
        assert np.array_equal(dev.download_radix(h), want[i]), i
    for i in (0, 2, 4, 5, 7):
        assert np.array_equal(dev.download_radix(hs[i]), first[i]), i


def test_arena_growth(pair):
    """the first upload of a fresh context needs 1,200 slots against the arena's first 1,024;
    a second one crosses 2,048 with content resident: the slots are allocated (and the arena
    moved) before the kernel's arena pointer is read"""
    client, _ = pair
    p = client.params
    dev = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
    rng = np.random.default_rng(7)
    a, b = text(rng, 300, False), text(rng, 220, False)
    blob_a, blob_b = client.encrypt_str_compact(a, K), client.encrypt_str_compact(b, bytes(reversed(K)))
    ha = dev.upload_compact_str(blob_a)  # 1,200 slots
    hb = dev.upload_compact_str(blob_b)  # 2,080 slots in all
    for blob, hs in ((blob_a, ha), (blob_b, hb)):
        want = client.expand_compact_content(blob).reshape(len(hs), 4, -1)
        got = np.stack([dev.download_radix(h) for h in hs])
        assert np.array_equal(got, want)
    dev.close()


def test_match(keyed):
    client, dev = keyed
    rng = np.random.default_rng(12)
    for planted in (True, False):
        s = text(rng, 16, planted)
        exp = ro.has_match(s, "/abc/").result
        assert exp == int(planted)
        blob = client.encrypt_str_compact(s, K)
        out, st = dev.has_match(dev.upload_compact_str(blob), "/abc/")
        words = dev.download_radix(out)
        assert client.decrypt_radix(words) == exp, (planted, s)
        assert st.blind_rotations > 0
        # the same LWEs uploaded the ordinary way: the same arithmetic, the same words
        full = client.expand_compact_content(blob).reshape(16, 4, -1)
        o2, _ = dev.has_match(dev.upload_radix(full), "/abc/")
        assert np.array_equal(dev.download_radix(o2), words)


def test_ordering_on_lanes(keyed):
    client, dev = keyed
    rng = np.random.default_rng(13)
    texts = [text(rng, 16, i % 2 == 0) for i in range(10)]
    blobs = [client.encrypt_str_compact(s, bytes([i + 1]) * 32) for i, s in enumerate(texts)]
    serial = []
    for blob in blobs:  # one stream, a download after every match
        o, _ = dev.has_match(dev.upload_radix(client.expand_compact_content(blob).reshape(16, 4, -1)), "/abc/")
        serial.append(dev.download_radix(o))
    for i, s in enumerate(texts):
        assert client.decrypt_radix(serial[i]) == ro.has_match(s, "/abc/").result
    dev.set_lanes(4)
    dev.set_async(True)
    try:
        outs = []
        for blob in blobs[:8]:  # nothing waits for the device in between
            o, _ = dev.has_match(dev.upload_compact_str(blob), "/abc/")
            outs.append(o)
        for i, o in enumerate(outs):
            assert np.array_equal(dev.download_radix(o), serial[i]), i
        # an upload while a match is queued, then a match on it
        q, _ = dev.has_match(dev.upload_compact_str(blobs[8]), "/abc/")
        h9 = dev.upload_compact_str(blobs[9])
        o9, _ = dev.has_match(h9, "/abc/")
        assert np.array_equal(dev.download_radix(o9), serial[9])
        assert np.array_equal(dev.download_radix(q), serial[8])
    finally:
        dev.set_lanes(1)


def test_server_without_a_client_key(keyed):
    """the server holds a compact server key and compact content: neither a client key nor
    a full-size object ever reaches it"""
    client, dev = keyed
    p = client.params
    gen = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
    gen.load_client_key(client.serialize_client_key())
    gen.set_keygen(F.KEYGEN_DEVICE)
    gen.gen_server_key(K, compact=True)
    server = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
    server.load_server_key_compact(gen.export_server_key_compact())
    gen.close()
    with pytest.raises(F.FheRegexError):
        server.serialize_client_key()
    sk = F.ServerKey(server)
    for planted in (True, False):
        s = text(np.random.default_rng(14), 16, planted)
        hs = sk.upload_str(F.ClientKey(client).encrypt_str_compact(s))  # OS randomness
        out = F.has_match(sk, hs, "/abc/")
        assert client.decrypt_radix(server.download_radix(out)) == int(planted) == ro.has_match(s, "/abc/").result
    server.close()
