"""The compact packing key on the device, both FFT points and one load on the RNS ring.

Generation: k_gen_pksk<N, COMPACT> under the public mask key, with the 40-bit rounding in its
epilogue, gives the host generator's key word for word.  Expansion: k_expand_rows over
STREAM_PKSK_MASK and the blob's two planes rebuilds every mask word and every body word, the
byte limbs follow; the export read back from the device equals the client's key, and
k_gather_planes40 gives the blob back.  Use: a keyless server that loaded a compact server key
and a compact packing key packs to the words of the host keyswitch over the same rows, and
answers match_starts.  The key has one size per point, so the packs are kept small.
"""
import numpy as np
import pytest

import fheregex as F
import regex_oracle as ro
from test_packed_results_gpu import mixed_inputs

K = bytes((29 * i + 5) & 0xFF for i in range(32))   # packing key
KS = bytes((37 * i + 11) & 0xFF for i in range(32))  # server key
POINTS = [(1, 2048), (2, 1024)]
SIZES = {(1, 2048): 62_914_656, (2, 1024): 31_457_376}

pytestmark = pytest.mark.gpu


class Setup:
    """the host client: client key, the compact-generated packing key and both its blobs"""

    def __init__(self, point, key_blob):
        self.point = point
        self.k, self.N = point
        self.p = F.default_params(k=self.k, N=self.N)
        self.key_blob = key_blob
        self.client = F.Context(device=-1, params=self.p)
        self.client.load_client_key(key_blob)
        self.client.gen_packing_key(K, compact=True)
        self.blob = self.client.export_packing_key_compact()
        self.full = self.client.export_packing_key()
        self.rows = np.frombuffer(self.full, dtype="<u8", offset=48).reshape(3 * self.k * self.N, (self.k + 1) * self.N)

    def device(self, client_key=False):
        ctx = F.Context(device=0, params=self.p)
        if client_key:
            ctx.load_client_key(self.key_blob)
        return ctx


@pytest.fixture(scope="module", params=POINTS, ids=["fft", "fft-k2n1024"])
def setup(request, key_blob):
    return Setup(request.param, key_blob)


@pytest.fixture(scope="module")
def server(setup):
    """a device context without a client key that loaded a compact server key and the compact
    packing key, both from the host client's blobs"""
    setup.client.gen_server_key(KS, compact=True)
    ctx = setup.device()
    ctx.load_server_key_compact(setup.client.export_server_key_compact())
    ctx.load_packing_key_compact(setup.blob)
    yield ctx
    ctx.set_plan_cache(0)
    st = ctx.arena_stats()
    assert st["slots"] == st["free_slots"], st
    ctx.close()


class Pair:
    def __init__(self, host, dev):
        self.host, self.dev = host, dev


def test_device_generation_equals_host(setup):
    ctx = setup.device(client_key=True)
    ctx.set_keygen(F.KEYGEN_DEVICE)
    ctx.gen_packing_key(K, compact=True)
    blob = ctx.export_packing_key_compact()
    assert len(blob) == ctx.packing_key_compact_size() == SIZES[setup.point]
    assert np.array_equal(blob, setup.blob)
    assert np.array_equal(ctx.export_packing_key(), setup.full)
    # the standard instantiation next to it: the standard key, and no compact export
    ctx.gen_packing_key(K)
    W = (setup.k + 1) * setup.N
    got = np.frombuffer(ctx.export_packing_key(), dtype="<u8", offset=48).reshape(-1, W)
    for r in (0, len(got) // 2 + 1, len(got) - 1):
        assert np.array_equal(got[r], setup.client.gen_packing_rows(K, r, r + 1)[0]), r
    with pytest.raises(F.FheRegexError) as e:
        ctx.export_packing_key_compact()
    assert e.value.code == F.ERR_INVALID
    ctx.close()


def test_device_expansion_equals_client_key(setup, server):
    assert np.array_equal(server.export_packing_key(), setup.full)  # read back from the device's rows
    assert np.array_equal(server.export_packing_key_compact(), setup.blob)
    k, N = setup.point
    # the last mask column, the first body column and both ends, through the GEMM's operand
    for col in (0, k * N - 1, k * N, (k + 1) * N - 1):
        assert np.array_equal(server.dev_packing_limb_column(col), setup.rows[:, col]), col
    with pytest.raises(F.FheRegexError):
        server.serialize_client_key()


@pytest.mark.parametrize("n", [1, 33])
def test_pack_on_expanded_key_equals_host(setup, server, n):
    pair = Pair(setup.client, server)
    handles, lwes, owned = mixed_inputs(pair, n, np.random.default_rng(n))
    got = server.pack_bools_words(handles)
    want = setup.client.pack_lwes(lwes)  # the host keyswitch over the client's (rounded) rows
    assert np.array_equal(got, want), (n, int((got != want).sum()))
    bits = setup.client.decrypt_packed(server.pack_bools(handles))
    assert bits == [setup.client.decode_block(lwes[j]) & 1 for j in range(n)]
    for h in set(handles + owned):
        server.release(h)


def test_end_to_end_with_compact_everything(setup, server):
    ck, sk = F.ClientKey(setup.client), F.ServerKey(server)
    rng = np.random.default_rng(12)
    s = "".join(chr(c) for c in rng.integers(0x20, 0x7F, 16)).replace("a", "x")
    s = s[:5] + "abc" + s[8:]
    want = [i for i in range(16) if ro.has_match(s, "/abc/", i, i + 1).result]
    assert want == [5]
    hs = sk.upload_str(ck.encrypt_str_compact(s, seed=3))
    reply = sk.match_starts(hs, "/abc/")
    assert len(reply) == 4 + server.packed_result_size(16)
    assert ck.decrypt_starts(reply) == want
    for h in hs:
        server.release(h)


def test_replacement(setup):
    """a full key over a compact one and the reverse: each leaves a key that packs to the
    host's words, and only the compact install exports compact"""
    ctx = setup.device()
    up = setup.client.encrypt_blocks([1, 0, 1, 1, 0], seed=21).reshape(5, -1)
    want = setup.client.pack_lwes(up)
    hs = ctx.upload_bool(up)
    ctx.load_packing_key_compact(setup.blob)
    assert np.array_equal(ctx.pack_bools_words(hs), want)
    ctx.load_packing_key(setup.full)
    assert np.array_equal(ctx.pack_bools_words(hs), want)
    with pytest.raises(F.FheRegexError) as e:
        ctx.export_packing_key_compact()
    assert e.value.code == F.ERR_INVALID and "not generated in compact form" in str(e.value)
    assert np.array_equal(ctx.export_packing_key(), setup.full)
    ctx.load_packing_key_compact(setup.blob)
    assert np.array_equal(ctx.pack_bools_words(hs), want)
    assert np.array_equal(ctx.export_packing_key_compact(), setup.blob)
    # a refused blob leaves that key working
    bad = setup.blob.copy()
    bad[48] = 32
    with pytest.raises(F.FheRegexError):
        ctx.load_packing_key_compact(bad)
    with pytest.raises(F.FheRegexError):
        ctx.load_packing_key_compact(setup.blob[:-1])
    assert np.array_equal(ctx.pack_bools_words(hs), want)
    assert setup.client.decrypt_packed(ctx.pack_bools(hs)) == [1, 0, 1, 1, 0]
    # the stage times of a profiled load are all there
    ctx.set_profiling(1)
    ctx.load_packing_key_compact(setup.blob)
    ms = ctx.packing_key_load_timers()
    assert len(ms) == 3 and all(t > 0 for t in ms), ms
    ctx.close()


def test_rns_point_loads_packs_and_decrypts(key_blob):
    p = F.default_params(k=1, N=2048, ring=F.RING_RNS)
    host = F.Context(device=-1, params=p)
    host.load_client_key(key_blob)
    host.gen_packing_key(K, compact=True)
    blob = host.export_packing_key_compact()
    assert len(blob) == SIZES[(1, 2048)]
    dev = F.Context(device=0, params=p)
    dev.load_packing_key_compact(blob)
    hs = dev.upload_bool(host.encrypt_blocks([1], seed=5).reshape(1, -1))
    assert host.decrypt_packed(dev.pack_bools(hs)) == [1]
    assert np.array_equal(dev.export_packing_key_compact(), blob)
    for h in hs:
        dev.release(h)
    st = dev.arena_stats()
    assert st["slots"] == st["free_slots"], st
    dev.close()
