"""The step schedule's entry packing (step_sched.h), on the host through fr_debug_scalar: ops 5
and 6 are the put and get the blind rotation's prologue and step loop use."""
import itertools

import fheregex as F

FIELDS, BITS, MASK, END = 5, 12, 0xFFF, 0xFFF


def put(L, e, f, v):
    return L.fr_debug_scalar(5, e, (f << BITS) | v)


def test_fields_round_trip_at_their_edges():
    """t = 0 and 370, e = 0 and 4095 in every field, every combination: each field reads back
    its own value and leaves the others alone"""
    L = F.lib()
    for vals in itertools.product((0, 370), (0, 4095), (0, 4095), (0, 4095), (0, 4095)):
        e = 0
        for f, v in enumerate(vals):
            e = put(L, e, f, v)
        assert e == sum(v << (BITS * f) for f, v in enumerate(vals))
        assert e < 1 << (FIELDS * BITS)
        assert tuple(L.fr_debug_scalar(6, e, f) for f in range(FIELDS)) == vals


def test_single_field_patterns():
    """one field at a time over bit patterns that straddle the 32-bit halves of the entry"""
    L = F.lib()
    for f in range(FIELDS):
        for v in (1, 2, 0x7FF, 0x800, 0xAAA, 0x555, 370, 511, MASK):
            e = put(L, 0, f, v)
            assert e == v << (BITS * f)
            assert [L.fr_debug_scalar(6, e, g) for g in range(FIELDS)] == [v if g == f else 0 for g in range(FIELDS)]


def test_end_entry_is_no_step():
    """the end entry's step field is above every step of a rotation (n <= 1024: t < 512), and a
    live entry of the last step with all-ones pairs is not the end entry"""
    L = F.lib()
    assert L.fr_debug_scalar(6, END, 0) == END and END > 511
    e = put(L, 0, 0, 511)
    for f in range(1, FIELDS):
        e = put(L, e, f, MASK)
    assert L.fr_debug_scalar(6, e, 0) == 511 != END


def test_mod_switch_of_written_words():
    """v 2^(64 - log2 2N) mod-switches to v: the mask words tests/test_step_schedule_gpu.py writes"""
    L = F.lib()
    for v in (0, 1, 370, 4095):
        assert L.fr_debug_scalar(3, v << 52, 12) == v
    for v in (0, 1, 2047):
        assert L.fr_debug_scalar(3, v << 53, 11) == v
