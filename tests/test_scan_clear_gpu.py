"""Scan of a long clear text on the device: the mapped rotate-sum (k_pack_map_sum, through
fr_dev_pack_mapped) word for word against the host restatement, fr_scan_clear_starts byte for byte
against fr_find_clear_starts and the packs of its handles, fr_scan_clear against the plain search
and, output by output, against Oracle.run_schedule on the scan's schedule; the plan cache, lanes,
ownership, the noise of a reply whose starts all read one row, and the refusals.

Contexts are tests/test_private_needle_gpu.py's end-to-end ones (server, packing and client key
in one context per point) and tests/test_gate_programs.py's.

The noise bound is tests/test_compact_reply_gpu.py's 2^55 for a compact reply of real bootstrap
outputs (worst bootstrap output 2^52.2 plus worst rounding 2^52.7, a bit and a half of margin):
DESIGN §7 charges a mapped pack of n starts what it charges a pack of n rows, so the same bound
is asked of 255 starts that read one row."""
import ctypes as C
import struct

import numpy as np
import pytest

import fheregex as F
import test_gate_programs as tg
import test_private_needle_gpu as pn
from test_find_clear import extract_sum
from test_find_clear_gpu import HIGH

pytestmark = pytest.mark.gpu

U = np.uint64
PIDS = ["k1n2048", "k2n1024"]
REP = b"abcab" * 8 + b"xyz"  # 43 bytes, few distinct windows
DELTA_LOG = 59


def in_use(c):
    st = c.arena_stats()
    return st["slots"] - st["free_slots"]


def full_blob(c, words, n):
    return b"FRPKRES1" + struct.pack("<iiQ", c.params.k, c.params.N, n) + words.tobytes()


def plain_starts(text, masks):
    return [p for p, v in enumerate(F.plain_find_clear(text, masks)[0]) if v]


# ------------------------------------------------------------------ the kernel, word for word
def rows_of(c, R, seed):
    """R boolean handles and the (lwes, w, off) they stand for: uploaded encryptions, and for
    R >= 3 a negated handle (row 1) and a trivial constant 1 (row 2)"""
    bits = np.random.default_rng(seed).integers(0, 2, R).astype(np.uint8)
    lwes = c.encrypt_blocks(bits, seed=seed).reshape(R, -1)
    up = c.upload_bool(lwes)
    handles, owned, w, off = list(up), list(up), [1] * R, [0] * R
    if R >= 3:
        zero = c.or_many([])
        handles[1], handles[2] = c.not_(up[1]), c.not_(zero)
        owned += [zero, handles[1], handles[2]]
        w[1], off[1] = -1, 2
        w[2], off[2] = 0, 2
    return handles, owned, lwes, w, off


def shapes(N):
    rng = np.random.default_rng(9)
    wide = [int(v) for v in rng.integers(0, 5, N)]
    wide[:5], wide[N - 1] = [0, 1, 2, 3, 4], 4  # every row read, the last start mapped
    return {
        "1x1": (1, [0]),
        "1x3": (1, [0, 0, 0]),
        "2x33": (2, [j % 2 for j in range(33)]),
        "3x33-gaps": (3, [(-1 if j % 5 == 3 else j % 3) for j in range(33)]),
        "5xN": (5, wide),
        # two slices of 32 starts and a third of one; class 16 is starts 31 and 32, one in each slice
        "33x65": (33, [(j + 1) // 2 for j in range(65)]),
        "identity": (33, list(range(33))),
    }


@pytest.mark.parametrize("shape", ["1x1", "1x3", "2x33", "3x33-gaps", "5xN", "33x65", "identity"])
@pytest.mark.parametrize("pid", PIDS)
def test_pack_mapped_words(key_blob, pid, shape):
    c = pn.e2e(key_blob, pid)[0]
    R, map_ = shapes(c.params.N)[shape]
    n = len(map_)
    handles, owned, lwes, w, off = rows_of(c, R, 100 + R)
    try:
        want = c.pack_lwes_mapped(lwes, map_, w, off)
        got = c.dev_pack_mapped(handles, map_)
        assert got == full_blob(c, want, n), np.flatnonzero(np.frombuffer(got[24:], dtype=U) != want)[:8]
        assert c.dev_pack_mapped(handles, map_, compact=True) == c.compress_packed(want, n)
        if shape == "identity":
            assert got == c.pack_bools(handles)
            assert c.dev_pack_mapped(handles, map_, compact=True) == c.pack_bools_compact(handles)
        bits = c.decrypt_packed(got)
        row_bits = [c.decrypt_radix(c.download_radix(h)) for h in handles]
        assert bits == [row_bits[r] if r >= 0 else 0 for r in map_]
    finally:
        for h in set(owned):
            c.release(h)


def test_pack_mapped_refusals(key_blob):
    c = pn.e2e(key_blob, "k1n2048")[0]
    handles, owned, _, _, _ = rows_of(c, 3, 7)
    N = c.params.N
    before = c.device_timers(), c.arena_stats()
    for hs, map_ in ((handles, [0, 1, 3]), (handles, [0, 1, 1]), (handles, [0, 1, -1]), (handles, [0, 1]),
                     (handles[:1], [0] * (N + 1)), ([], [0]), (handles, [])):
        with pytest.raises(F.FheRegexError):
            c.dev_pack_mapped(hs, map_)
    assert (c.device_timers(), c.arena_stats()) == before
    for h in set(owned):
        c.release(h)


# ------------------------------------------------------------------ byte identity with the existing path
NEEDLES = {REP: {1: b"a", 3: b"cab", 9: b"abcababca"}, HIGH: {1: b"\xe9", 3: b"\xe9\x80\xe9", 9: HIGH[3:12]}}


@pytest.mark.parametrize("m", [1, 3, 9])
@pytest.mark.parametrize("text", [REP, HIGH], ids=["rep", "high"])
@pytest.mark.parametrize("pid", PIDS)
def test_scan_starts_is_find_clear_starts_byte_for_byte(key_blob, pid, text, m):
    """equal windows give equal LWEs word for word (exact extract-sums, deterministic bootstraps
    in every launch shape) and the pack is linear: both reply forms, byte for byte"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    s = NEEDLES[text][m]
    masks = F.needle_masks(s)
    nd = sk.upload_needle(c.encrypt_needle(masks, seed=90 + m))
    handles = c.handle_count()
    try:
        for compact in (False, True):
            got, want = sk.scan_clear_starts(text, nd, compact), sk.find_clear_starts(text, nd, compact)
            assert len(got) == len(want)
            assert got == want, (pid, m, compact, [i for i in range(len(got)) if got[i] != want[i]][:8])
            assert ck.decrypt_starts(got) == plain_starts(text, masks) != []
        cls, D, Dpad, _ = F.window_classes(text, m)
        assert c.scan_classes() == (D, Dpad) and D <= len(text) - m + 1
        assert text != REP or D < len(text) - m + 1  # (the 43-byte text: starts share windows at every m)
        assert c.handle_count() == handles
    finally:
        nd.close()


@pytest.mark.parametrize("compact", [False, True])
def test_two_chunks(key_blob, compact):
    """(2, 1024): N + 40 bytes of a 7-byte period; the second chunk has 40 starts and few rows"""
    c, ck, sk, _, _ = pn.e2e(key_blob, "k2n1024")
    N = c.params.N
    text = (b"abcdefg" * (N // 7 + 8))[:N + 40]
    masks = F.needle_masks(b"cde")
    nd = sk.upload_needle(c.encrypt_needle(masks, seed=95))
    try:
        blobs, st = c.scan_clear_starts(text, nd, compact=compact, stats=True)
        assert c.scan_classes() == (7, 64) and st.blind_rotations == st.pbs == 64 and st.levels == 1
        got = sk.scan_clear_starts(text, nd, compact)
        assert got[-len(blobs):] == blobs
        assert got == sk.find_clear_starts(text, nd, compact)
        want = plain_starts(text, masks)
        assert ck.decrypt_starts(got) == want and want[0] == 2 and want[-1] >= N and len(want) == len(text) // 7
    finally:
        nd.close()


# ------------------------------------------------------------------ the boolean
SCAN_CASES = [(REP, b"xyz", False, None, 1), (REP, b"abd", False, None, 0), (b"ab", b"abc", False, None, 0),
              (REP, b"b?a", False, "?", 1), (REP, b"CAB", True, None, 1), (HIGH, b"\x00\xff", False, None, 1)]


@pytest.mark.parametrize("pid", PIDS)
def test_scan_clear_boolean(key_blob, pid):
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    for text, s, ic, wc, want in SCAN_CASES:
        masks = F.needle_masks(s, ic, wc)
        assert F.plain_scan_clear(text, masks)[1] == F.plain_find_clear(text, masks)[1] == want
        nd = sk.upload_needle(c.encrypt_needle(masks, seed=97))
        try:
            out, st = c.scan_clear(text, nd)
            D, Dpad = c.scan_classes()
            assert (D, Dpad) == F.window_classes(text, len(s))[1:3]
            S = F.schedule_scan_clear(Dpad, len(s))
            assert st.pbs == st.blind_rotations == len(S.jobs) and st.levels == len(S.level_off) - 1
            assert ck.decrypt(out) == want, (text, s)
            ref = sk.find_clear(text, nd)
            assert ck.decrypt(ref) == want
            c.release(out), c.release(ref)
            # the replies of these needles too (a needle longer than the text: every chunk written on
            # the host), and of an empty text: no chunk
            for t in (text, b""):
                for compact in (False, True):
                    assert sk.scan_clear_starts(t, nd, compact) == sk.find_clear_starts(t, nd, compact), (t, s, compact)
        finally:
            nd.close()


def scan_values(S, sel, padded: bytes, m):
    """{gate: LWE} of a scan schedule's extract-sums: window d's chunk of tests, term t =
    (selector t, position d m + t // 2, half t % 2), in the order of the level-1 jobs"""
    from selector_cases import balanced_chunks
    gates = [j.in_ref[0] for j in S.jobs[:S.level_off[1]]]
    sums = [[(t, d * m + t // 2, t % 2) for t in range(first, first + ln)]
            for d in range(len(padded) // m) for first, ln in balanced_chunks(2 * m)]
    assert len(sums) == len(gates) == len(set(gates))
    return {g: extract_sum(sel, padded, terms) for g, terms in zip(gates, sums)}


@pytest.mark.parametrize("pid", PIDS)
def test_scan_clear_words(request, key_blob, pid):
    """fr_scan_clear's output against Oracle.run_schedule on the scan's schedule, its
    extract-sums seeded from the numpy restatement over the padded compacted text: word for word"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    m = 3
    blob = ck.encrypt_needle("cab", seed=21)
    sel = c.expand_needle(blob)
    nd = sk.upload_needle(blob)
    try:
        cls, D, Dpad, win = F.window_classes(REP, m)
        padded = win + win[:m] * (Dpad - D)
        S = F.schedule_scan_clear(Dpad, m)
        O.run_schedule(S, None, values=scan_values(S, sel, padded, m))
        want = O._output(*S.parts[0])
        out, _ = c.scan_clear(REP, nd)
        got = c.download_radix(out)[0]
        c.release(out)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    finally:
        nd.close()


# ------------------------------------------------------------------ plan cache, ownership, lanes
def test_cache_is_keyed_by_m_and_padded_classes(key_blob):
    c, ck, sk, _, _ = pn.e2e(key_blob, "k1n2048")
    t1, t2 = REP, b"the cab is a cab, not a cat; a cab."  # another length, another D, the same padded D
    masks = F.needle_masks(b"cab")
    nd = sk.upload_needle(c.encrypt_needle(masks, seed=31))
    c.set_plan_cache(0), c.set_plan_cache(8)
    used, handles = in_use(c), c.handle_count()
    try:
        stats = c.plan_cache_stats()
        r1, st1 = c.scan_clear_starts(t1, nd, stats=True)
        d1 = c.scan_classes()
        r2, st2 = c.scan_clear_starts(t2, nd, stats=True)
        d2 = c.scan_classes()
        assert d1[0] != d2[0] and d1[1] == d2[1] == 64 and len(t1) != len(t2)
        assert (st1.plan_cached, st2.plan_cached) == (0, 1)
        after = c.plan_cache_stats()
        assert (after["misses"], after["hits"], after["entries"]) == (stats["misses"] + 1, stats["hits"] + 1, 1)
        for t, r in ((t1, r1), (t2, r2)):
            reply = struct.pack("<II", F.COMPACT_REPLY, 1) + r
            assert ck.decrypt_starts(reply) == plain_starts(t, masks) != []
        # the boolean is another plan (starts = false), and fr_find_clear's never the scan's
        out, st3 = c.scan_clear(t1, nd)
        out2, st4 = c.scan_clear(t2, nd)
        assert (st3.plan_cached, st4.plan_cached) == (0, 1) and ck.decrypt(out) == ck.decrypt(out2) == 1
        hs, st5 = c.find_clear_starts(bytes(64), nd, stats=True)  # n = 64 = padded D, m = 3: a miss
        ref, st6 = c.find_clear(t1, nd)  # and on the same text
        assert (st5.plan_cached, st6.plan_cached) == (0, 0) and ck.decrypt(ref) == 1
        for h in hs + [out, out2, ref]:
            c.release(h)
        # no handle and no slot beyond the cached plans'
        assert c.handle_count() == handles
        c.set_plan_cache(0)
        assert in_use(c) == used
    finally:
        c.set_plan_cache(8)
        nd.close()


def test_lanes(key_blob):
    """two asynchronous scans on two lanes: the serial replies byte for byte"""
    c, ck, sk, _, _ = pn.e2e(key_blob, "k1n2048")
    t1, t2 = REP, HIGH + REP[:20]
    nd = sk.upload_needle(ck.encrypt_needle("cab", seed=41))
    serial = [c.scan_clear_starts(t, nd) for t in (t1, t2)]
    c.set_lanes(2)
    c.set_async(True)
    try:
        for rep in range(2):  # (the first round compiles each lane's plan copy)
            assert [c.scan_clear_starts(t, nd) for t in (t1, t2)] == serial, rep
        outs = [c.scan_clear(t, nd)[0] for t in (t1, t2, t2, t1)]
        assert [ck.decrypt(h) for h in outs] == [1, 1, 1, 1]
        for h in outs:
            c.release(h)
    finally:
        c.set_lanes(1)
        nd.close()


# ------------------------------------------------------------------ noise
@pytest.mark.parametrize("pid", PIDS)
def test_error_of_starts_that_share_one_row(key_blob, pid):
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    n = 256
    nd = sk.upload_needle(ck.encrypt_needle("aa", seed=51))
    try:
        blob = c.scan_clear_starts(b"a" * n, nd)
        assert c.scan_classes() == (1, 64)
        words, got_n = c.expand_packed_compact(blob)
        assert got_n == n
        want = np.array([1] * (n - 1) + [0], dtype=np.int64) << DELTA_LOG  # the last start does not fit
        err = c.packed_phase(words).astype(np.int64)[:n] - want
        worst = int(np.abs(err).max())
        print(f"{pid}: 255 starts on one row, largest distance from the bit 2^{np.log2(max(worst, 1)):.2f}, "
              f"rms 2^{np.log2(np.sqrt(np.mean(err.astype(np.float64) ** 2))):.2f}")
        assert worst < 2 ** 55
    finally:
        nd.close()


# ------------------------------------------------------------------ refusals
def scan_rc(c, text, needle_h):
    """the codes of fr_scan_clear, of fr_scan_clear_starts' size query and of the call itself"""
    out = (C.c_uint32 * 1)()
    n = C.c_size_t()
    lib = F.lib()
    buf = C.create_string_buffer(1 << 16)
    return (lib.fr_scan_clear(c.h, text, len(text), needle_h, 0, len(text), out, None),
            lib.fr_scan_clear_starts(c.h, text, len(text), needle_h, 0, len(text), 1, None, 0, C.byref(n), None),
            lib.fr_scan_clear_starts(c.h, text, len(text), needle_h, 0, len(text), 1, buf, 1 << 16, C.byref(n), None))


def test_refusals(key_blob, monkeypatch):
    """an error code each, nothing planned or launched, timers and arena as they were"""
    c1, ck1, sk1, _, _ = pn.e2e(key_blob, "k1n2048")
    c2, ck2, sk2, _, _ = pn.e2e(key_blob, "k2n1024")
    n1 = sk1.upload_needle(ck1.encrypt_needle("abc", seed=71))
    n2 = sk2.upload_needle(ck2.encrypt_needle("abc", seed=72))
    state = lambda c: (c.plan_cache_stats(), c.arena_stats(), c.device_timers())  # noqa: E731
    INV = F.ERR_INVALID
    rns = tg.device_ctx(key_blob, monkeypatch, "rns", {})
    other = tg.device_ctx(key_blob, monkeypatch, "k1n2048", {})  # the same (k, N), another context, no packing key
    for c, needle, msg in ((rns, n1, "FFT ring only"), (c1, n2, "needle"), (c2, n1, "needle"), (other, n1, "needle")):
        c.set_profiling(1)
        try:
            before = state(c)
            assert scan_rc(c, b"xxabcxx", needle.h) == (INV, INV, INV)
            assert msg in F.lib().fr_last_error().decode()
            assert state(c) == before
        finally:
            c.set_profiling(0)
    own = other.upload_needle(ck1.encrypt_needle("abc", seed=73))  # no packing key: the boolean runs, the reply does not
    before = state(other)
    n = C.c_size_t()
    assert F.lib().fr_scan_clear_starts(other.h, b"xxabcxx", 7, own.h, 0, 7, 1, None, 0, C.byref(n), None) == INV
    assert "packing key" in F.lib().fr_last_error().decode() and state(other) == before
    own.close()
    # a short cap: the needed size comes back, nothing is launched
    c1.set_profiling(1)
    try:
        before = state(c1)
        need = 32 + 2 * (c1.params.k * c1.params.N + 7)
        buf = C.create_string_buffer(need)
        fn = F.lib().fr_scan_clear_starts
        assert fn(c1.h, b"xxabcxx", 7, n1.h, 0, 7, 1, None, 0, C.byref(n), None) == 0 and n.value == need
        n.value = 0
        assert fn(c1.h, b"xxabcxx", 7, n1.h, 0, 7, 1, buf, need - 1, C.byref(n), None) == INV and n.value == need
        out = (C.c_uint32 * 1)()
        assert F.lib().fr_scan_clear(c1.h, None, 4, n1.h, 0, 4, out, None) == INV
        assert F.lib().fr_scan_clear(c1.h, b"abcd", 4, n1.h, 3, 2, out, None) == INV
        assert fn(c1.h, b"abcd", 4, n1.h, 0, 2 ** 24 + 1, 1, None, 0, C.byref(n), None) == INV
        assert state(c1) == before
    finally:
        c1.set_profiling(0)
    n1.close(), n2.close()
