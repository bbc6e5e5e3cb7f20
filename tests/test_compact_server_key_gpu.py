"""The compact server key on the device, both FFT points.

Generation: k_gen_ksk and k_gen_bsk<N, COMPACT> under the public mask key give the host
generator's key word for word.  Expansion: k_expand_ksk / k_expand_bsk<N> rebuild every
mask word from the mask key around the uploaded bodies; the export read back from the
device equals the client's, which covers the ChaCha block straddles of all 10,240 KSK
rows.  Use: a keyless server that loaded the blob matches /abc/ to the words of a context
that generated the key itself and of one that took the expanded key through
fr_load_server_key.  The key has one size per point, so only the match is kept small.
"""
import numpy as np
import pytest

import fheregex as F
import regex_oracle as ro

K = bytes((37 * i + 11) & 0xFF for i in range(32))
POINTS = [(1, 2048), (2, 1024)]

pytestmark = pytest.mark.gpu


class Setup:
    def __init__(self, point, key_blob):
        k, N = point
        self.p = F.default_params(k=k, N=N)
        self.client = F.Context(device=-1, params=self.p)  # host: client key, generation, encryption
        self.client.load_client_key(key_blob)
        self.client.gen_server_key(K, compact=True)
        self.blob = self.client.export_server_key_compact()
        self.ksk, self.bsk = self.client.export_server_key()
        self.key_blob = key_blob


@pytest.fixture(scope="module", params=POINTS, ids=["fft", "fft-k2n1024"])
def setup(request, key_blob):
    return Setup(request.param, key_blob)


@pytest.fixture(scope="module")
def generated(setup):
    """a device context that generated the compact key itself"""
    ctx = F.Context(device=0, params=setup.p)
    ctx.load_client_key(setup.key_blob)
    ctx.set_keygen(F.KEYGEN_DEVICE)
    ctx.gen_server_key(K, compact=True)
    return ctx


@pytest.fixture(scope="module")
def server(setup):
    """a device context without a client key that loaded the host client's blob"""
    ctx = F.Context(device=0, params=setup.p)
    ctx.load_server_key_compact(setup.blob)
    return ctx


def test_device_generation_equals_host(setup, generated):
    ksk, bsk = generated.export_server_key()
    assert np.array_equal(ksk, setup.ksk)
    assert np.array_equal(bsk, setup.bsk)
    assert generated.export_server_key_compact() == setup.blob


def test_device_expansion_equals_client_export(setup, server):
    ksk, bsk = server.export_server_key()  # read back from the device's torus keys
    assert np.array_equal(ksk, setup.ksk)
    assert np.array_equal(bsk, setup.bsk)
    assert server.export_server_key_compact() == setup.blob
    with pytest.raises(F.FheRegexError):
        server.serialize_client_key()


def test_match_on_expanded_key(setup, server, generated):
    full = F.Context(device=0, params=setup.p)  # the expanded key through fr_load_server_key
    full.load_server_key(setup.ksk, setup.bsk)
    rng = np.random.default_rng(11)
    for planted in (True, False):
        s = "".join(chr(c) for c in rng.integers(0x20, 0x7F, 16))
        s = s[:6] + "abc" + s[9:] if planted else s.replace("a", "x")
        exp = ro.has_match(s, "/abc/").result
        assert exp == int(planted)
        ct = setup.client.encrypt_str(s, seed=5)
        out, st = server.has_match(server.upload_radix(ct), "/abc/")
        words = server.download_radix(out)
        assert setup.client.decrypt_radix(words) == exp, (planted, s)
        assert st.blind_rotations > 0
        for other in (generated, full):
            o, _ = other.has_match(other.upload_radix(ct), "/abc/")
            assert np.array_equal(other.download_radix(o), words)
    # one direct blind rotation of 3 LWEs, word-identical across the three contexts
    lwes = setup.client.encrypt_blocks([9, 0, 14], seed=2)
    luts = [[(7 * m + 3 + i) % 16 for m in range(16)] for i in range(3)]
    ks = server.dev_keyswitch(lwes)
    ref = server.dev_blind_rotate(ks, luts)
    for i, v in enumerate((9, 0, 14)):
        assert setup.client.decode_block(ref[i]) == luts[i][v]
    for other in (generated, full):
        assert np.array_equal(other.dev_keyswitch(lwes), ks)
        assert np.array_equal(other.dev_blind_rotate(ks, luts), ref)


def test_replacement_while_a_match_is_queued(setup, server):
    """the same blob installed while a match is still queued (calls are asynchronous): the
    device drains before the old key's buffers go, and the queued match reads the old key"""
    ct = setup.client.encrypt_str("0123abc789abcdef", seed=6)
    out, _ = server.has_match(server.upload_radix(ct), "/abc/")
    words = server.download_radix(out)
    assert setup.client.decrypt_radix(words) == 1
    queued, _ = server.has_match(server.upload_radix(ct), "/abc/")
    server.load_server_key_compact(setup.blob)
    assert np.array_equal(server.download_radix(queued), words)
    again, _ = server.has_match(server.upload_radix(ct), "/abc/")  # and the new key is the same key
    assert np.array_equal(server.download_radix(again), words)
