"""Precomputed key products (k_key_products + k_blind_rotate_fft_kp, k = 1, N = 2048): the
smallest latency-shape launches form the MAC's key-only products K_own, K_oth of every step
before the rotation starts.  The products are the MAC's own operations in its own order, so
every output word must equal the latency shape's (FR_FFT_KPRE_BATCH=0) and the oracle's.

Contexts (one per limit, shared by the tests): ON covers every launch of these tests (64),
OFF never takes the path (0), EDGE switches between 3 and 4 bootstraps."""
import numpy as np
import pytest

import fheregex as F
import test_gate_programs as tg  # its programs, oracle rows and contexts, computed once for both

pytestmark = pytest.mark.gpu

SEED = 42
POINT = (1, 2048)
ON, OFF, EDGE = 64, 0, 3
_CTX = {}


def ctx_for(key_blob, monkeypatch, limit):
    if limit not in _CTX:
        monkeypatch.setenv("FR_FFT_KPRE_BATCH", str(limit))
        c = F.Context(device=0, params=F.default_params(k=POINT[0], N=POINT[1], ring=F.RING_FFT))
        monkeypatch.delenv("FR_FFT_KPRE_BATCH")
        c.load_client_key(key_blob)
        c.gen_server_key(SEED)
        _CTX[limit] = c
    return _CTX[limit]


@pytest.fixture(scope="module")
def inputs(oracle_k1):
    """8 keyswitched fresh encryptions, random 16-entry LUTs and the oracle's rows"""
    O = oracle_k1
    rng = np.random.default_rng(77)
    ks = O.keyswitch(O.encrypt_blocks(rng.integers(0, 16, 8), seed=78))
    luts = rng.integers(0, 16, (8, 16), dtype=np.uint8)
    want = np.stack([O.blind_rotate(ks[q], list(luts[q])) for q in range(8)])
    return ks, luts, want


def same(got, want):
    return [q for q in range(len(want)) if not (got[q] == want[q]).all()]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_batches_word_for_word(key_blob, monkeypatch, inputs, n):
    """batches of 1, 2 and 3: the new path, the latency shape and the oracle agree on every word"""
    ks, luts, want = inputs
    new = ctx_for(key_blob, monkeypatch, ON).dev_blind_rotate(ks[:n], luts[:n])
    old = ctx_for(key_blob, monkeypatch, OFF).dev_blind_rotate(ks[:n], luts[:n])
    assert not same(new, want[:n]) and not same(old, want[:n])


def test_dispatch_edge(key_blob, monkeypatch, inputs):
    """FR_FFT_KPRE_BATCH=3: a launch of 3 (key products) and one of 4 (the key itself)"""
    ks, luts, want = inputs
    c = ctx_for(key_blob, monkeypatch, EDGE)
    assert not same(c.dev_blind_rotate(ks[2:5], luts[2:5]), want[2:5])
    assert not same(c.dev_blind_rotate(ks[4:8], luts[4:8]), want[4:8])


def test_idle_steps(key_blob, monkeypatch, oracle_k1, inputs):
    """Zeroed mask pairs -- the first, the last, two adjacent ones, a run -- are skipped by the
    producer (nothing stored for them) and by the rotation's next-step table alike; in a
    batch of 2 one pair is idle for the first bootstrap only."""
    O = oracle_k1
    ks, luts, _ = inputs
    last = (O.n + 1) // 2 - 1
    a = ks[:3].copy()
    for t in (0, last, 100, 101, 200, 201, 202, 203, 368):
        a[0, 2 * t:2 * t + 2] = 0
    for t in (0, 1, last - 1, last):
        a[1, 2 * t:2 * t + 2] = 0
    a[2] = ks[2]
    a[1, 2 * 7:2 * 7 + 2] = 0  # idle for bootstrap 1 only in the launch (a[1], a[2])
    want = np.stack([O.blind_rotate(a[q], list(luts[q])) for q in range(3)])
    new, old = ctx_for(key_blob, monkeypatch, ON), ctx_for(key_blob, monkeypatch, OFF)
    for lo, hi in ((0, 1), (1, 3), (0, 3)):
        assert not same(new.dev_blind_rotate(a[lo:hi], luts[lo:hi]), want[lo:hi]), (lo, hi)
        assert not same(old.dev_blind_rotate(a[lo:hi], luts[lo:hi]), want[lo:hi]), (lo, hi)


def test_scratch_grows_and_is_reused(key_blob, monkeypatch, inputs):
    """one context: batch 1 (allocates), batch 3 (grows), batch 1 again (reuses)"""
    ks, luts, want = inputs
    monkeypatch.setenv("FR_FFT_KPRE_BATCH", str(ON))
    c = F.Context(device=0, params=F.default_params(k=POINT[0], N=POINT[1], ring=F.RING_FFT))
    monkeypatch.delenv("FR_FFT_KPRE_BATCH")
    c.load_client_key(key_blob)
    c.gen_server_key(SEED)
    for lo, hi in ((5, 6), (0, 3), (7, 8)):
        assert not same(c.dev_blind_rotate(ks[lo:hi], luts[lo:hi]), want[lo:hi]), (lo, hi)
    c.close()


def _match_words(c, lanes, count):
    s = "xxabcxxxxxxxxxab"
    hs = c.upload_radix(c.encrypt_str(s, seed=5))
    c.set_lanes(lanes)
    outs = [c.has_match(hs, "/abc/")[0] for _ in range(count)]
    words = [c.download_radix(o) for o in outs]
    c.set_lanes(1)
    for h in outs + hs:
        c.release(h)
    assert all(c.decrypt_radix(w) == 1 for w in words)
    return words


def test_regex_match_on_off_and_lanes(key_blob, monkeypatch):
    """/abc/ on 16 chars: the result words with the path on and off; then two lanes (consecutive
    matches take consecutive lanes, each with a scratch of its own) against the one-lane run"""
    on = _match_words(ctx_for(key_blob, monkeypatch, ON), 1, 1)
    off = _match_words(ctx_for(key_blob, monkeypatch, OFF), 1, 1)
    assert np.array_equal(on[0], off[0])
    for w in _match_words(ctx_for(key_blob, monkeypatch, ON), 2, 4):
        assert np.array_equal(w, on[0])


@pytest.mark.parametrize("lanes", [1, 2])
def test_small_gate_program(request, key_blob, monkeypatch, lanes):
    """The small program (levels of at most 64 jobs, the second a single one: multi-value,
    direct and sign jobs in one launch) with the limit covering every level, twice in a row:
    every gate's words equal the oracle's and the default dispatch's."""
    p = tg.program("small")
    rows, words = tg.expected(request, "k1n2048", "small")
    assert max(len(jl) for jl in p.jobs()) <= ON
    got = {}
    for name, c in (("on", ctx_for(key_blob, monkeypatch, ON)), ("default", tg.device_ctx(key_blob, monkeypatch, "k1n2048", {}))):
        c.set_lanes(lanes)
        for rep in range(2 if name == "on" else 1):
            hs = p.upload(c, rows)
            outs = c.run_gates(p.fr_gates(hs))
            got[name] = np.stack([c.download_radix(h)[0] for h in outs])
            for h in outs + hs:
                c.release(h)
            bad = [gi for gi in range(len(p.gates)) if not (got[name][gi] == words[gi]).all()]
            assert not bad, (name, rep, len(bad), bad[:12])
        c.set_lanes(1)
    assert np.array_equal(got["on"], got["default"])
