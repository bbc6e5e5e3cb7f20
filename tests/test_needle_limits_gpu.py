"""Private search at its needle-length limits on the device: fr_find*, fr_find_clear* and
fr_scan_clear* end to end at m = 8, 16, 17 and 64 (tests/needle_limits.py says what changes at
each), where the other device tests stop at 9.

Whole finds are compared word for word with Oracle.run_schedule, as tests/test_private_needle_gpu.py
and tests/test_find_clear_gpu.py do at m = 3 and 9: on encrypted content that pins the selector
index of every job up to 127 (a 4 MB table at k = 1) in every compiled selector shape, the chunked
AND above it and, at m = 64, a level 1 of exactly 256 rotations (the last latency launch) and of
384 (pair at k = 1, throughput at k = 2), read back from the device timers; on clear content the
chunks' sums (a full 16 terms at m = 8, 16 and 64) and the gates of offset -31 over them.  The scan
is held byte for byte to fr_find_clear_starts, and word for word to the oracle over 128 padded
windows of 64 bytes.  Two 64-character needles alive at once bind their tables per call.

Helpers, contexts and oracles are those of the modules named above and tests/test_gate_programs.py.
Oracle time per case is printed.  The largest cases are the find at m = 16 (17 starts: 1,193
rotations for both calls) and the scan over 128 windows (1,161): 1.3 s and 1.6 s on 16 threads, the
rest under a second; the whole file takes 26 s on one MI355X."""
import time

import numpy as np
import pytest

import fheregex as F
import needle_limits as nl
import selector_cases as sc
import test_find_clear_gpu as fc
import test_gate_programs as tg
import test_private_needle_gpu as pn
import test_scan_clear_gpu as scg

pytestmark = pytest.mark.gpu

U = np.uint64
PIDS = fc.PIDS
NEEDLE_SEED = 21
# (m, text): every length on its own slice of the text, and m = 64 also on 65 bytes
FIND_CASES = [(m, nl.DEVICE_TEXT[m]) for m in nl.LIMITS] + [(64, nl.TEXT_65)]
case_id = lambda c: "m%d-n%d" % (c[0], len(c[1]))  # noqa: E731
_MIXED, _FIND_WORDS = {}, {}


def needle_blob(c, m, text, name="plain"):
    masks = dict(nl.cases(m, text))[name]
    return masks, c.encrypt_needle(masks, seed=NEEDLE_SEED)


def mixed(c, sk, pid, text):
    """the text's handles with its first four characters trivial"""
    if (pid, text) not in _MIXED:
        _MIXED[pid, text] = [sk.create_trivial_radix(b) for b in text[:4]] + fc.encrypted(c, pid, text)[4:]
    return _MIXED[pid, text]


def timed(what, f):
    t = time.perf_counter()
    out = f()
    print("oracle %s: %.2f s" % (what, time.perf_counter() - t))
    return out


def find_words(request, c, pid, m, text, sel, content, kind):
    """oracle_find_words of the case, once per (point, case, kind of content), with the content
    LWEs and selectors they were computed from"""
    key = (pid, m, text, kind)
    if key not in _FIND_WORDS:
        lwes = np.stack([c.download_radix(h) for h in content])
        words = timed("%s find m = %d over %d %s characters" % (pid, m, len(text), kind),
                      lambda: pn.oracle_find_words(c, tg.oracle(request, pid), sel, m, content))
        _FIND_WORDS[key] = lwes, sel, words
    return _FIND_WORDS[key]


# ------------------------------------------------------------------ a. encrypted content
@pytest.mark.parametrize("kind", ["fresh", "partly-trivial"])
@pytest.mark.parametrize("case", FIND_CASES, ids=case_id)
@pytest.mark.parametrize("pid", PIDS)
def test_find_words_and_replies(request, key_blob, pid, case, kind):
    """every output of fr_find and fr_find_starts equals Oracle.run_schedule's word for word, on
    fresh content and with the first four characters trivial; the outputs decrypt to py_starts
    within check_outputs' noise bound, both reply forms decrypt to it, and the absent needle is
    found nowhere"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    m, text = case
    masks, blob = needle_blob(c, m, text)
    want = nl.starts_of(text, masks)
    assert len(text) - m in want
    bits = [int(p in want) for p in range(len(text))]
    sel = c.expand_needle(blob)
    assert sel.shape == (2 * m, c.params.k + 1, c.params.N)
    content = fc.encrypted(c, pid, text) if kind == "fresh" else mixed(c, sk, pid, text)
    nd = sk.upload_needle(blob)
    gone = sk.upload_needle(needle_blob(c, m, text, "absent")[1])
    try:
        _, _, words = find_words(request, c, pid, m, text, sel, content, kind)
        got = pn.device_find_words(c, nd, content)
        assert got.shape == words.shape == (1 + len(text), c.lwe_len)
        bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], words[i])]  # (-1: fr_find's)
        assert not bad, (pid, m, kind, bad)
        out, _ = c.find(content, nd)
        starts = c.find_starts(content, nd)
        fc.check_outputs(request, c, ck, pid, [out] + starts, [1] + bits)
        for h in [out] + starts:
            c.release(h)
        for compact in (False, True):
            assert ck.decrypt_starts(sk.find_starts(content, nd, compact=compact)) == want, (pid, m, kind, compact)
        out = sk.find(content, gone)
        assert ck.decrypt(out) == 0
        c.release(out)
        assert ck.decrypt_starts(sk.find_starts(content, gone, compact=True)) == []
    finally:
        nd.close(), gone.close()


@pytest.mark.parametrize("pid", PIDS)
def test_level_one_on_either_side_of_256_rotations(key_blob, pid):
    """m = 64 is 128 selector rotations a start: two starts are one launch of 256, the last of
    the latency shape; three are 384, the pair shape at k = 1 and the throughput shape at k = 2.
    The levels above (16 + 2 and 24 + 3 sign gates, the OR) are latency launches."""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    nd = sk.upload_needle(needle_blob(c, 64, nl.DEVICE_TEXT[64])[1])
    c.set_profiling(1)
    try:
        for text, fit in ((nl.TEXT_65, 2), (nl.DEVICE_TEXT[64], 3)):
            content = fc.encrypted(c, pid, text)
            for starts in (True, False):
                S = F.schedule_find(len(text), 64, starts=starts)
                sizes = nl.level_jobs(64, fit, starts, clear=False)
                assert sizes[:3] == [128 * fit, 8 * fit, fit] and len(sizes) == (3 if starts else 4)
                t0 = c.device_timers()
                outs, st = c.find_starts(content, nd, stats=True) if starts else c.find(content, nd)
                t1 = c.device_timers()  # (synchronises)
                for h in outs if starts else [outs]:
                    c.release(h)
                assert st.pbs == st.blind_rotations == len(S.jobs) == sum(sizes) and st.levels == len(sizes)
                big = sizes[0] > 256
                pair = sizes[0] if big and pid == "k1n2048" else 0
                d = {k: t1[k] - t0[k] for k in ("br_launches", "br_gates", "lat_gates", "pair_gates")}
                assert d == {"br_launches": len(sizes), "br_gates": sum(sizes), "pair_gates": pair,
                             "lat_gates": sum(sizes) - (sizes[0] if big else 0)}, (pid, fit, starts, d, sizes)
    finally:
        c.set_profiling(0)
        nd.close()


# ------------------------------------------------------------------ b. every compiled selector shape
@pytest.mark.parametrize("shape", list(pn.SHAPES))
def test_selector_indices_in_every_shape(request, key_blob, monkeypatch, shape):
    """the m = 64 find over 66 characters (selector indices 0..127 from a compiled plan) in each
    shape the selector kernels are compiled in, forced by the context's environment: the words of
    the default context's run, which are the oracle's"""
    pid, c = pn.ctx_of(key_blob, monkeypatch, shape)
    m, text = 64, nl.DEVICE_TEXT[64]
    e2e_c = pn.e2e(key_blob, pid)[0]
    masks, blob = needle_blob(c, m, text)
    sel = c.expand_needle(blob)
    lwes, sel0, words = find_words(request, e2e_c, pid, m, text, e2e_c.expand_needle(needle_blob(e2e_c, m, text)[1]),
                                   fc.encrypted(e2e_c, pid, text), "fresh")
    content = c.upload_radix(c.encrypt_blocks([(b >> (2 * i)) & 3 for b in text for i in range(4)], seed=12))
    nd = c.upload_needle(blob)
    try:
        # the same inputs on this context: the oracle's rows hold for it
        assert np.array_equal(sel, sel0) and np.array_equal(np.stack([c.download_radix(h) for h in content]), lwes)
        got = pn.device_find_words(c, nd, content)
        bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], words[i])]
        assert got.shape == words.shape and not bad, (shape, bad)
    finally:
        nd.close()
        for h in content:
            c.release(h)


# ------------------------------------------------------------------ c. clear content
@pytest.mark.parametrize("case", FIND_CASES, ids=case_id)
@pytest.mark.parametrize("pid", PIDS)
def test_find_clear_words_and_replies(request, key_blob, pid, case):
    """every output of fr_find_clear and fr_find_clear_starts against Oracle.run_schedule seeded
    from extract_sum; the stats are the schedule's; decryption, noise, and both reply forms equal
    to fr_find_starts' on an encryption of the same text"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    m, text = case
    masks, blob = needle_blob(c, m, text)
    want = nl.starts_of(text, masks)
    bits = [int(p in want) for p in range(len(text))]
    sel = c.expand_needle(blob)
    nd = sk.upload_needle(blob)
    try:
        words = timed("%s find_clear m = %d over %d bytes" % (pid, m, len(text)),
                      lambda: fc.oracle_find_clear_words(O, sel, m, text))
        got = fc.device_find_clear_words(c, nd, text)
        assert got.shape == words.shape == (1 + len(text), c.lwe_len)
        bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], words[i])]  # (-1: fr_find_clear's)
        assert not bad, (pid, m, bad)
        for starts in (True, False):
            S = F.schedule_find_clear(len(text), m, starts=starts)
            if starts:
                outs, st = c.find_clear_starts(text, nd, stats=True)
            else:
                out, st = c.find_clear(text, nd)
                outs = [out]
            assert st.pbs == st.blind_rotations == len(S.jobs) and st.levels == len(S.level_off) - 1
            fc.check_outputs(request, c, ck, pid, outs, bits if starts else [1])
            for h in outs:
                c.release(h)
        enc = fc.encrypted(c, pid, text)
        for compact in (False, True):
            clear = ck.decrypt_starts(sk.find_clear_starts(text, nd, compact=compact))
            assert clear == ck.decrypt_starts(sk.find_starts(enc, nd, compact=compact)) == want, (pid, m, compact)
    finally:
        nd.close()
    gone = sk.upload_needle(needle_blob(c, m, text, "absent")[1])
    try:
        out = sk.find_clear(text, gone)
        assert ck.decrypt(out) == 0
        c.release(out)
        assert ck.decrypt_starts(sk.find_clear_starts(text, gone, compact=True)) == []
    finally:
        gone.close()


# ------------------------------------------------------------------ d. the scan
@pytest.mark.parametrize("m", nl.LIMITS)
@pytest.mark.parametrize("pid", PIDS)
def test_scan_is_find_clear_byte_for_byte(key_blob, pid, m):
    """fr_scan_clear_starts' reply equals fr_find_clear_starts' in both forms, on a text whose
    windows of m bytes recur; the classes are fr_window_classes'"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    text = nl.SCAN_TEXT
    masks, blob = needle_blob(c, m, text)
    want = scg.plain_starts(text, masks)
    assert want == nl.starts_of(text, masks) and len(want) >= 3 and want[-1] == len(text) - m
    nd = sk.upload_needle(blob)
    handles = c.handle_count()
    try:
        for compact in (False, True):
            got, ref = sk.scan_clear_starts(text, nd, compact), sk.find_clear_starts(text, nd, compact)
            assert got == ref, (pid, m, compact, [i for i in range(min(len(got), len(ref))) if got[i] != ref[i]][:8])
            assert ck.decrypt_starts(got) == want
        cls, D, Dpad, _ = F.window_classes(text, m)
        assert c.scan_classes() == (D, Dpad) == F.window_classes(text, m)[1:3] and D < len(text) - m + 1
        out, st = c.scan_clear(text, nd)
        S = F.schedule_scan_clear(Dpad, m)
        assert st.pbs == st.blind_rotations == len(S.jobs) and st.levels == len(S.level_off) - 1
        assert ck.decrypt(out) == 1
        c.release(out)
        assert c.handle_count() == handles
    finally:
        nd.close()


@pytest.mark.parametrize("pid", PIDS)
def test_scan_past_64_windows_of_64_bytes(request, key_blob, pid):
    """130 seeded bytes at m = 64: 67 distinct windows, padded to 128, the plan's text 8,192 bytes.
    fr_scan_clear's output word for word against Oracle.run_schedule over scan_values (window d's
    terms at d 64 ..), and the reply equal to fr_find_clear_starts'.  The needle is the last
    window, class 66: the OR's answer comes from the far end of the compacted text."""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    text, m = nl.RANDOM_TEXT, 64
    masks = F.needle_masks(nl.needle(m, text))
    blob = c.encrypt_needle(masks, seed=NEEDLE_SEED)
    sel = c.expand_needle(blob)
    cls, D, Dpad, win = F.window_classes(text, m)
    assert (D, Dpad) == (67, 128) and scg.plain_starts(text, masks) == [66]
    padded = win + win[:m] * (Dpad - D)
    S = F.schedule_scan_clear(Dpad, m)
    assert len(padded) == 8192 and len(S.jobs) == 128 * 9 + 8 + 1

    def run():
        O.run_schedule(S, None, values=scg.scan_values(S, sel, padded, m))
        return O._output(*S.parts[0])
    want = timed("%s scan m = 64 over 128 windows" % pid, run)
    nd = sk.upload_needle(blob)
    try:
        out, st = c.scan_clear(text, nd)
        assert c.scan_classes() == (D, Dpad) and st.pbs == len(S.jobs) and st.levels == len(S.level_off) - 1
        got = c.download_radix(out)[0]
        assert ck.decrypt(out) == 1
        c.release(out)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        for compact in (False, True):
            got = sk.scan_clear_starts(text, nd, compact)
            assert got == sk.find_clear_starts(text, nd, compact), (pid, compact)
            assert ck.decrypt_starts(got) == [66]
    finally:
        nd.close()


# ------------------------------------------------------------------ e. two full-size tables
@pytest.mark.parametrize("pid", PIDS)
def test_two_needles_of_64_characters_bind_per_call(key_blob, pid):
    """two 64-character needles (128 selectors each) alive at once and used alternately in
    fr_find* and fr_find_clear*: each call reads its own needle's table, serially and on two
    asynchronous lanes word for word; closing both returns every slot and handle"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    text = nl.DEVICE_TEXT[64]
    content = fc.encrypted(c, pid, text)
    blobs = [needle_blob(c, 64, text)[1], c.encrypt_needle(F.needle_masks(text[:64]), seed=NEEDLE_SEED + 1)]
    answers = [[2], [0]]
    c.set_plan_cache(0), c.set_plan_cache(8)  # (the plans own slots: counted with the cache empty)
    arena, handles = c.arena_stats(), c.handle_count()
    needles = [sk.upload_needle(b) for b in blobs]
    try:
        alone = []
        for nd, want in zip(needles, answers):
            alone.append((pn.device_find_words(c, nd, content), fc.device_find_clear_words(c, nd, text)))
            assert ck.decrypt_starts(sk.find_starts(content, nd, compact=True)) == want
            assert ck.decrypt_starts(sk.find_clear_starts(text, nd, compact=True)) == want
        assert not np.array_equal(alone[0][0], alone[1][0]) and not np.array_equal(alone[0][1], alone[1][1])
        order = [0, 1, 1, 0, 1, 0]
        for lanes in (1, 2):
            c.set_lanes(lanes)
            c.set_async(True)
            for rep, i in enumerate(order):
                assert np.array_equal(pn.device_find_words(c, needles[i], content), alone[i][0]), (lanes, rep, i)
                assert np.array_equal(fc.device_find_clear_words(c, needles[i], text), alone[i][1]), (lanes, rep, i)
            # queued back to back, read afterwards: a later call's binding does not reach an earlier one
            outs = [(i, c.find(content, needles[i])[0], c.find_clear(text, needles[i])[0]) for i in order]
            for i, a, b in outs:
                assert np.array_equal(c.download_radix(a)[0], alone[i][0][0]), (lanes, i)
                assert np.array_equal(c.download_radix(b)[0], alone[i][1][0]), (lanes, i)
                c.release(a), c.release(b)
    finally:
        c.set_lanes(1)
        for nd in needles:
            nd.close()
    c.set_plan_cache(0)
    after = c.arena_stats()  # (synchronises every lane: deferred frees return)
    c.set_plan_cache(8)
    assert after["slots"] - after["free_slots"] == arena["slots"] - arena["free_slots"]
    assert c.handle_count() == handles
