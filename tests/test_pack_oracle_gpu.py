"""The reply path on the device against oracle/pack_oracle.py, and the LWE keyswitch against the
oracle's under crafted keys: directed operands (tests/gadget_edges.py) in every launch shape,
word for word, at both FFT points.  No expected word comes from the product's host code.

Packing keyswitch, per (point, key) with the key real, saturating or mixed:
  n = 1, 33     k_ks_mfma<1, 1> with two K slices meeting in atomics (the DPP epilogue)
  n = 97        k_ks_glds, the whole K = 6144 in one accumulator, padded to 128 rows (the LDS
                epilogue); with the saturating key and the all-low row every i32 limb sum is
                64 * 128 * 6144 = 50,331,648, the bound common.h states
  n = 33 under FR_PK_SPLIT=1 in a fresh context: the same K in k_ks_mfma<1, 1>
  k_pack_rotate_sum, k_pack_map_sum (1x3, 3x33-gaps, 33x65; full and compact), k_pack_compress
  with kN + n no multiple of 8 (n = 6, 9: the last thread's overlapping, 2-byte-aligned store),
  k_ksk_limbs' carry chain through dev_packing_limb_column.
LWE keyswitch, per point, a private Oracle whose ksk is overwritten with the key the device loads:
  count = 1 (8 K slices), 97 (k_ks_glds, 5 slices; FR_KS_SPLIT=1: all 10240 k in one
  accumulator, limb sums 4 * 128 * 10240 = 5,242,880 under the saturating key), 97 under
  FR_KS_LDS=0 (k_ks_mfma<4, 1>), 33 under FR_KS_MFMA=0 (the VALU kernel) and under FR_KS_DIG16=0
  (the byte-store digit pass).

Wall time of the module on an MI355X: 10.4 s (72 tests, none above 0.9 s; a crafted packing key
is one 201 MB upload per module-scoped context).
"""
import struct

import numpy as np
import pytest

import fheregex as F
import gadget_edges as ge
import oracle_ffi as of
import pack_oracle as po
import test_compact_reply as tcr
import test_packed_results_gpu as tpg
import test_scan_clear_gpu as sc

pytestmark = pytest.mark.gpu

U = np.uint64
SEED, PSEED = tpg.SEED, tpg.PSEED
POINTS = {"fft": (F.RING_FFT, 1, 2048), "fft-k2n1024": (F.RING_FFT, 2, 1024)}
KINDS = ["real", "saturating", "mixed"]
RIGS = [(pid, kind) for pid in POINTS for kind in KINDS]


def closed_clean(dev):
    """every slot the tests took has been returned; the context is closed whether or not"""
    try:
        dev.set_plan_cache(0)
        st = dev.arena_stats()
    finally:
        dev.close()
    assert st["slots"] == st["free_slots"], st


class Rig:
    """a device context holding the packing key `kind` (generated on the device, or a crafted one
    behind the generated key's header), its wire blob and the restatement's Key of the same rows"""

    def __init__(self, pid, kind, key_blob):
        _, self.k, self.N = POINTS[pid]
        k, N = self.k, self.N
        self.big, self.W = k * N, (k + 1) * N
        self.dev = tpg.make(POINTS[pid], key_blob, 0)
        self.dev.gen_packing_key(PSEED)
        self.blob = self.dev.export_packing_key()
        if kind != "real":
            self.blob = ge.packing_blob(self.blob[:48], ge.crafted_key(kind, 3 * self.big, self.W))
            self.dev.load_packing_key(self.blob)
        self.key = po.Key(np.frombuffer(self.blob, dtype="<u8", offset=48), k, N)
        self.point = POINTS[pid]


@pytest.fixture(scope="module", params=RIGS, ids=["%s-%s" % r for r in RIGS])
def rig(request, key_blob):
    r = Rig(*request.param, key_blob)
    yield r
    closed_clean(r.dev)


def upload(dev, lwes):
    """handles of the rows, row 2 behind a NOT (w = -1, off = 2) where there is one; the
    weights and offsets the handles stand for; everything to release"""
    n = len(lwes)
    handles = dev.upload_bool(lwes)
    owned, w, off = list(handles), [1] * n, [0] * n
    if n >= 3:
        handles[2] = dev.not_(handles[2])
        owned.append(handles[2])
        w[2], off[2] = -1, 2
    return handles, owned, w, off


def pack_words(dev, lwes):
    handles, owned, w, off = upload(dev, lwes)
    try:
        return dev.pack_bools_words(handles), w, off
    finally:
        for h in owned:
            dev.release(h)


def differing(got, want):
    bad = np.flatnonzero(got != want)
    return len(bad), [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:4]]


# ------------------------------------------------------------------ the packing keyswitch
@pytest.mark.parametrize("which", ["one", "tile_plus_one", "four_row_tiles"])
def test_pack_of_edge_rows(rig, which):
    """all-low and the catalogue row first, an edge row last, one handle negated"""
    n = {"one": 1, "tile_plus_one": 33, "four_row_tiles": 97}[which]
    # 97: three whole row tiles and one real row ahead of 31 padding rows in the fourth
    assert (n >= tpg.mr4_min()) == (which == "four_row_tiles") and n % 32 in (1, n)
    names, lwes = ge.lwe_rows(7, 3, rig.big, n, 100 + n)
    assert names[0] == "all-low" and (n < 4 or (names[1], names[-1]) == ("catalogue", "ends"))
    got, w, off = pack_words(rig.dev, lwes)
    want = po.pack(rig.key, lwes, w, off)
    assert np.array_equal(got, want), differing(got, want)


def test_pack_in_one_slice_of_the_one_row_tile_shape(rig, monkeypatch):
    """FR_PK_SPLIT=1 in a fresh context: n = 33 keeps K = 6144 in one accumulator of k_ks_mfma<1, 1>"""
    monkeypatch.setenv("FR_PK_SPLIT", "1")
    ring, k, N = rig.point
    dev = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
    dev.load_packing_key(rig.blob)
    _, lwes = ge.lwe_rows(7, 3, rig.big, 33, 133)
    try:
        got, w, off = pack_words(dev, lwes)
    finally:
        closed_clean(dev)
    want = po.pack(rig.key, lwes, w, off)
    assert np.array_equal(got, want), differing(got, want)


def test_limb_columns_recombine(rig):
    """k_ksk_limbs' balanced carry chain on the crafted words (a carry through all eight bytes)"""
    rows = rig.key.rows
    for col in (0, 1, 2, 3, 5, 7, rig.N - 1, rig.N, rig.W - 1, 1234):
        assert np.array_equal(rig.dev.dev_packing_limb_column(col), rows[:, col]), col


@pytest.mark.parametrize("shape", ["1x3", "3x33-gaps", "33x65"])
def test_mapped_pack_of_edge_rows(rig, shape):
    k, N, dev = rig.k, rig.N, rig.dev
    R, map_ = sc.shapes(N)[shape]
    n = len(map_)
    _, lwes = ge.lwe_rows(7, 3, rig.big, R, 200 + R)
    handles, owned, w, off = upload(dev, lwes)
    try:
        full = dev.dev_pack_mapped(handles, map_)
        compact = dev.dev_pack_mapped(handles, map_, compact=True)
    finally:
        for h in owned:
            dev.release(h)
    want = po.pack_mapped(rig.key, lwes, map_, w, off)
    assert full[:24] == b"FRPKRES1" + struct.pack("<iiQ", k, N, n) and len(full) == 24 + 8 * rig.W
    got = np.frombuffer(full, dtype="<u8", offset=24)
    assert np.array_equal(got, want), differing(got, want)
    assert compact[:32] == tcr.header(k, N, n) and len(compact) == 32 + 2 * (rig.big + n)
    assert np.array_equal(np.frombuffer(compact, dtype="<u2", offset=32), po.round16(want[:rig.big + n]))


@pytest.mark.parametrize("n", [6, 9])
def test_compress_at_the_rounding_edges(rig, n):
    """trivial rows whose bodies are the rounding's edges; kN + n is no multiple of 8"""
    k, N, dev = rig.k, rig.N, rig.dev
    assert (rig.big + n) % 8
    lwes, vals = ge.trivial_rows(rig.big, n)
    want = po.pack(rig.key, lwes)
    assert not want[:rig.big].any() and np.array_equal(want[rig.big:rig.big + n], lwes[:, -1])
    handles = dev.upload_bool(lwes)
    try:
        blobs = [dev.pack_bools_compact(handles), dev.dev_pack_mapped(handles, list(range(n)), compact=True)]
        # ... and behind a real pack, every sent coefficient
        _, edge = ge.lwe_rows(7, 3, rig.big, n, 300 + n)
        more = dev.upload_bool(edge)
        handles += more
        edge_blob = dev.pack_bools_compact(more)
    finally:
        for h in handles:
            dev.release(h)
    for blob in blobs:
        assert blob[:32] == tcr.header(k, N, n) and len(blob) == 32 + 2 * (rig.big + n)
        sent = np.frombuffer(blob, dtype="<u2", offset=32)
        assert np.array_equal(sent, po.round16(want[:rig.big + n]))
        assert list(sent[rig.big:]) == vals
    sent = np.frombuffer(edge_blob, dtype="<u2", offset=32)
    assert np.array_equal(sent, po.round16(po.pack(rig.key, edge)[:rig.big + n]))


# ------------------------------------------------------------------ the LWE keyswitch
_SERVER, _ORACLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def released():
    """the exported server keys and the private oracles live no longer than this module"""
    yield
    _SERVER.clear()
    _ORACLE.clear()


def server_key(pid, key_blob):
    """(ksk, bsk) a device context generated and exported, once per point"""
    if pid not in _SERVER:
        donor = tpg.make(POINTS[pid], key_blob, 0)
        donor.gen_server_key(SEED)
        _SERVER[pid] = donor.export_server_key()
        donor.close()
    return _SERVER[pid]


def private_oracle(pid, fixture_key):
    """an Oracle of this module's own (the shared oracle_k1 is never modified); its ksk is
    overwritten with whatever key the device holds"""
    if pid not in _ORACLE:
        _, k, N = POINTS[pid]
        _ORACLE[pid] = of.Oracle(fixture_key, SEED, k=k, N=N, with_bsk=False, ring=of.RING_FFT)
    return _ORACLE[pid]


KS_CASES = {
    "one": ({}, 1),                               # k_ks_mfma<1, 1>, 8 K slices
    "glds": ({}, 97),                             # k_ks_glds, 5 K slices
    "glds-one-slice": ({"FR_KS_SPLIT": "1"}, 97),  # all 10240 k in one accumulator
    "mr4-registers": ({"FR_KS_LDS": "0"}, 97),    # k_ks_mfma<4, 1>
    "valu": ({"FR_KS_MFMA": "0"}, 33),            # k_lincomb_keyswitch
    "byte-digits": ({"FR_KS_DIG16": "0"}, 33),    # k_ks_digits
}


@pytest.mark.parametrize("case", list(KS_CASES))
@pytest.mark.parametrize("pid", list(POINTS))
def test_keyswitch_under_crafted_keys(pid, case, key_blob, fixture_key, monkeypatch):
    env, count = KS_CASES[case]
    assert (count >= tpg.mr4_min()) == (count == 97)
    ring, k, N = POINTS[pid]
    real_ksk, bsk = server_key(pid, key_blob)
    O = private_oracle(pid, fixture_key)
    assert O.ksk.shape == real_ksk.shape == (k * N * 5 * (O.n + 1),)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    dev = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
    _, lwes = ge.lwe_rows(3, 5, k * N, count, 400 + count)
    kinds = KINDS if not env else KINDS[1:]  # the real key in the default shapes: count 1 and 97
    try:
        for kind in kinds:
            ksk = real_ksk if kind == "real" else ge.crafted_key(kind, k * N * 5, O.n + 1).reshape(-1)
            dev.load_server_key(ksk, bsk)
            O.ksk[:] = ksk
            got, want = dev.dev_keyswitch(lwes), O.keyswitch(lwes)
            assert got.shape == want.shape == (count, O.n + 1)
            assert np.array_equal(got, want), (kind, differing(got.reshape(-1), want.reshape(-1)))
    finally:
        closed_clean(dev)
