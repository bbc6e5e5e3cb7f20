"""The seven wire blobs against tests/golden/wire_digests.json, on host-only contexts.

The file was recorded by tests/golden/make_wire_digests.py (which also defines what is recorded)
with the library of the commit before the wire layer got a file of its own.  Per point --
(1, 2048) and (2, 1024) on the FFT ring, (1, 2048) on the RNS ring -- and per blob it holds the
length, the header bytes, the BLAKE2b-256 of the whole blob, and the return code and message of
the checking entry for every header byte with bit 0 and bit 7 flipped (the key formats: one byte
of the free mask key only) and for the lengths 0, header, exact - 1, exact + 1, exact + 8.  All
of it is recomputed here and compared for equality; one context per point serves the module.

The header layouts themselves are restated independently, with struct.pack, in
test_compact_server_key.py, test_compact_content.py, test_packed_results.py,
test_compact_packing_key.py, test_compact_reply.py and test_private_needle.py.
"""
import importlib.util
import os

import pytest

from conftest import GOLDEN

spec = importlib.util.spec_from_file_location("make_wire_digests", os.path.join(GOLDEN, "make_wire_digests.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def stored():
    return gen.load()


@pytest.fixture(scope="module", params=gen.POINTS, ids=gen.point_id)
def point(request, stored):
    """(the point's stored record, the record of this build)"""
    return stored[gen.point_id(request.param)], gen.record(request.param)


def test_file_holds_every_point_and_format(stored):
    assert list(stored) == [gen.point_id(p) for p in gen.POINTS]
    for rec in stored.values():
        assert sorted(rec) == sorted(gen.FORMATS)


@pytest.mark.parametrize("name", list(gen.FORMATS))
def test_blob_and_acceptance(point, name):
    want, got = point[0][name], point[1][name]
    assert sorted(got) == sorted(want)
    for field in ("refused", "length", "header", "entry", "blake2b", "lengths"):
        assert got.get(field) == want.get(field), (name, field)
    if "flips" in want:
        assert len(got["flips"]) == len(want["flips"])
        bad = [(g, w) for g, w in zip(got["flips"], want["flips"]) if g != w]
        assert not bad, f"{name}: {len(bad)} of {len(want['flips'])} flipped headers answer differently, first: {bad[0]}"
