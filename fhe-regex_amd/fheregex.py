"""Python mirror of the reference's regex API over the MI355X C-ABI (libfheregex.so).

Reference API (RKlompUU/fhe-regex) -> here:
  src/regex/ciphertext.rs:42-45  gen_keys()                    -> gen_keys(...)
  src/regex/ciphertext.rs:32-40  encrypt_str(ck, s)            -> ClientKey.encrypt_str(s)
  src/regex/ciphertext.rs:8-30   create_trivial_radix(sk, m)   -> ServerKey.create_trivial_radix(m)
  src/regex/engine.rs:8-42       has_match(sk, content, pat)   -> has_match(sk, content, pat)
  RadixClientKey::decrypt                                      -> ClientKey.decrypt(ct)
  src/regex/parser.rs:146-185    parse(pattern)                -> parse(pattern) (canonical AST string)

Errors mirror the reference: a pattern the reference rejects raises ``ParseError``
(reference: ``Err``), a pattern/content on which the reference panics raises
``ReferencePanic``, non-ASCII content raises ``ValueError`` (ciphertext.rs:33-35).

All homomorphic work runs in the HIP kernels behind the C-ABI; there is no CPU
fallback: a GPU op on a context without a device raises ``NoDevice``.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass
from typing import Tuple, List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FHEREGEX_LIB") or os.path.join(HERE, "libfheregex.so")
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "include", "fheregex.h")

FR_OK = 0
ERR_INVALID, ERR_PARSE, ERR_REF_PANIC, ERR_NO_DEVICE, ERR_HIP, ERR_NO_KEY, ERR_OOM, ERR_NON_ASCII = range(-1, -9, -1)
ERR_RNG = -9
LOWER_FAITHFUL, LOWER_THRESHOLD, LOWER_FAITHFUL_TREE = 0, 1, 2
ENGINE_AUTO, ENGINE_ENUMERATE, ENGINE_MERGED = 0, 1, 2
GRAMMAR_REFERENCE, GRAMMAR_EXT = 0, 1
KEYGEN_AUTO, KEYGEN_HOST, KEYGEN_DEVICE = 0, 1, 2
NULL_CT = 0xFFFFFFFF


class FheRegexError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class ParseError(FheRegexError):
    pass


class ReferencePanic(FheRegexError):
    pass


class NoDevice(FheRegexError):
    pass


class Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("ks_base_log", C.c_int32),
                ("ks_level", C.c_int32), ("pbs_base_log", C.c_int32), ("pbs_level", C.c_int32),
                ("ring", C.c_int32), ("lwe_sigma", C.c_double), ("glwe_sigma", C.c_double)]


class MatchStats(C.Structure):
    _fields_ = [("ct_ops", C.c_uint64), ("cache_hits", C.c_uint64), ("n_branches", C.c_uint64),
                ("pbs", C.c_uint64), ("blind_rotations", C.c_uint64), ("levels", C.c_uint64), ("max_level_width", C.c_uint64),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("br_kernel_ms", C.c_double),
                ("ks_kernel_ms", C.c_double), ("br_launches", C.c_uint64), ("br_gates", C.c_uint64),
                ("plan_cached", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PlainResult(C.Structure):
    _fields_ = [("ct_ops", C.c_uint64), ("cache_hits", C.c_uint64), ("n_branches", C.c_uint64),
                ("pbs", C.c_uint64), ("levels", C.c_uint64), ("max_level_width", C.c_uint64),
                ("result_recorded", C.c_int32), ("result_lowered", C.c_int32)]


GATE_LUT, GATE_SIGN = 0, 1


class Gate(C.Structure):
    """fr_gate: offset in units of Delta/2; kind GATE_LUT or GATE_SIGN."""
    _fields_ = [("n_in", C.c_int32), ("offset", C.c_int32), ("kind", C.c_int32), ("in_", C.c_uint32 * 16),
                ("in_block", C.c_int8 * 16), ("in_w", C.c_int8 * 16), ("lut", C.c_uint8 * 16),
                ("out", C.c_uint32)]


class FrJob(C.Structure):
    """fr_job: one rotation job of a match schedule (fr_schedule_match)."""
    _fields_ = [("n_in", C.c_int32), ("offset", C.c_int32), ("in_ref", C.c_int32 * 16), ("in_w", C.c_int32 * 16),
                ("n_out", C.c_int32), ("kind", C.c_int32), ("out_gate", C.c_int32 * 8), ("lut", (C.c_uint8 * 16) * 8)]


JOB_MULTI, JOB_DIRECT, JOB_SIGN, JOB_ACC = 0, 1, 2, 3
NEEDLE_HEADER = 64  # bytes before a needle blob's bodies

u64p = C.POINTER(C.c_uint64)
_lib = None

# every exported symbol of include/fheregex.h, with (restype, argtypes)
_SIGS = {
    "fr_ctx_create": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]),
    "fr_ctx_destroy": (C.c_int, [C.c_void_p]),
    "fr_last_error": (C.c_char_p, []),
    "fr_default_params": (C.c_int, [C.POINTER(Params)]),
    "fr_load_client_key": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "fr_gen_client_key": (C.c_int, [C.c_void_p, C.c_uint64]),
    # *_keyed: key = 32 bytes, or None (NULL) for the OS CSPRNG
    "fr_gen_client_key_keyed": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fr_gen_server_key_keyed": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fr_encrypt_str_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, u64p]),
    "fr_encrypt_blocks_keyed": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_char_p, C.c_uint64,
                                          u64p]),
    "fr_encrypt_upload_str_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                              C.POINTER(C.c_uint32)]),
    "fr_serialize_client_key": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_gen_server_key": (C.c_int, [C.c_void_p, C.c_uint64]),
    "fr_set_keygen": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_export_server_key": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t]),
    "fr_server_key_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fr_load_server_key": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t]),
    "fr_gen_server_key_compact": (C.c_int, [C.c_void_p, C.c_uint64]),
    "fr_gen_server_key_compact_keyed": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fr_server_key_compact_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "fr_export_server_key_compact": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_load_server_key_compact": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "fr_device_timers_key_load": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_gen_packing_key": (C.c_int, [C.c_void_p, C.c_uint64]),
    "fr_gen_packing_key_keyed": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fr_packing_key_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "fr_export_packing_key": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_load_packing_key": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fr_gen_packing_key_compact": (C.c_int, [C.c_void_p, C.c_uint64]),
    "fr_gen_packing_key_compact_keyed": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fr_packing_key_compact_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "fr_export_packing_key_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_load_packing_key_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fr_device_timers_packing_key_load": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_packed_result_size": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_pack_bools": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, u64p]),
    "fr_pack_bools_blob": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "fr_decrypt_packed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_size_t)]),
    "fr_packed_compact_size": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_pack_bools_compact": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "fr_compress_packed": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_expand_packed_compact": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, u64p, C.POINTER(C.c_size_t)]),
    "fr_decrypt_packed_compact": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8),
                                            C.POINTER(C.c_size_t)]),
    "fr_match_starts_packed": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t,
                                         C.c_size_t, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(MatchStats)]),
    "fr_dev_packing_limb_column": (C.c_int, [C.c_void_p, C.c_int32, u64p]),
    "fr_device_timers_pack": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_device_timers_pack_compact": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_gen_packing_rows_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, u64p]),
    "fr_gen_packing_rows_compact_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, u64p]),
    "fr_pack_lwes": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, u64p]),
    "fr_packed_phase": (C.c_int, [C.c_void_p, u64p, u64p]),
    "fr_compact_content_size": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_encrypt_str_compact_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_size_t,
                                               C.POINTER(C.c_size_t)]),
    "fr_encrypt_blocks_compact_keyed": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_char_p,
                                                  C.c_uint64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_expand_compact_content": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, u64p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "fr_upload_compact_str": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "fr_upload_compact_blocks": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "fr_device_timers_content": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_needle_size": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_encrypt_needle_keyed": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.c_size_t, C.c_char_p, C.c_char_p,
                                          C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_expand_needle": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_upload_needle": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "fr_needle_len": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "fr_needle_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fr_find": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                          C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_find_starts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                 C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_schedule_find": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32, C.POINTER(FrJob),
                                   C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_plain_find": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint16), C.c_size_t, C.c_size_t, C.c_size_t,
                                C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "fr_dev_blind_rotate_acc": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p]),
    "fr_find_clear": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_find_clear_starts": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                       C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_schedule_find_clear": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32, C.POINTER(FrJob),
                                         C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "fr_plain_find_clear": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint16), C.c_size_t, C.c_size_t,
                                      C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "fr_dev_select_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.c_size_t, u64p]),
    "fr_dev_select_sum_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fr_scan_clear": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_scan_clear_starts": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                       C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t),
                                       C.POINTER(MatchStats)]),
    "fr_scan_classes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fr_window_classes": (C.c_int, [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32),
                                    C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.c_char_p, C.c_size_t]),
    "fr_schedule_scan_clear": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int32, C.POINTER(FrJob), C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "fr_plain_scan_clear": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint16), C.c_size_t, C.c_size_t,
                                      C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "fr_needle_bytes_size": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_encrypt_needle_bytes_keyed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p,
                                                C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_expand_needle_bytes": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, u64p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "fr_needle_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "fr_schedule_find_clear_bytes": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32,
                                               C.POINTER(FrJob), C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_schedule_scan_clear_bytes": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int32, C.POINTER(FrJob), C.c_size_t,
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t,
                                               C.POINTER(C.c_size_t)]),
    "fr_plain_find_clear_bytes": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t,
                                            C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "fr_plain_scan_clear_bytes": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t,
                                            C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "fr_dev_pack_mapped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_int32), C.c_size_t,
                                     C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_pack_lwes_mapped": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t,
                                      C.POINTER(C.c_int32), C.c_size_t, u64p]),
    "fr_encrypt_str": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, u64p]),
    "fr_encrypt_blocks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_uint64, C.c_uint64, u64p]),
    "fr_decrypt_radix": (C.c_int, [C.c_void_p, u64p, u64p]),
    "fr_decode_block": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_uint32)]),
    "fr_upload_radix": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_upload_bool": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_encrypt_upload_str": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint32)]),
    "fr_radix_serialize": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_uint64, C.c_char_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "fr_radix_deserialize": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, u64p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "fr_download_radix": (C.c_int, [C.c_void_p, C.c_uint32, u64p]),
    "fr_release": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fr_trivial": (C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(C.c_uint32)]),
    "fr_eq_const": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint8, C.POINTER(C.c_uint32)]),
    "fr_gt_const": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint8, C.POINTER(C.c_uint32)]),
    "fr_le_const": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint8, C.POINTER(C.c_uint32)]),
    "fr_and": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fr_or": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fr_not": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fr_or_many": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_run_gates": (C.c_int, [C.c_void_p, C.POINTER(Gate), C.c_size_t]),
    "fr_has_match": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.POINTER(C.c_uint32),
                               C.POINTER(MatchStats)]),
    "fr_has_match_range": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t,
                                     C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_has_match_parts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t,
                                     C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t),
                                     C.POINTER(MatchStats)]),
    "fr_match_starts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t,
                                  C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_plain_match_starts": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32,
                                        C.c_int32, C.c_int32, C.POINTER(PlainResult), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fr_schedule_match_starts": (C.c_int, [C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.POINTER(FrJob), C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "fr_plain_match_parts": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_size_t, C.POINTER(PlainResult),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "fr_schedule_match_parts": (C.c_int, [C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_size_t, C.POINTER(FrJob), C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "fr_debug_enumeration_cost": (C.c_int, [C.c_char_p, C.c_int32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64,
                                            C.c_uint64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "fr_parse": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "fr_set_plan_cache": (C.c_int, [C.c_void_p, C.c_size_t]),
    "fr_set_plan_cache_slots": (C.c_int, [C.c_void_p, C.c_size_t]),
    "fr_set_async": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_set_lanes": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_plan_cache_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fr_has_match_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t, C.c_char_p,
                                     C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_set_engine": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_set_grammar": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_parse_ex": (C.c_int, [C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t]),
    "fr_plain_match_g": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                   C.c_int32, C.POINTER(PlainResult)]),
    "fr_plain_match_ex": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                    C.POINTER(PlainResult)]),
    "fr_plain_match": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32,
                                 C.POINTER(PlainResult)]),
    "fr_set_lowering": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_set_multi_value": (C.c_int, [C.c_void_p, C.c_int32]),
    "fr_dev_blind_rotate_multi": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, u64p]),
    "fr_dev_keyswitch": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p]),
    "fr_dev_blind_rotate": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_uint8), C.c_size_t, u64p]),
    "fr_dev_ring_mul": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p]),
    "fr_dev_bench_pbs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_int32,
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fr_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "fr_debug_scalar": (C.c_uint64, [C.c_int32, C.c_uint64, C.c_uint64]),
    "fr_debug_arena_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fr_debug_handle_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "fr_export_bool_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p]),
    "fr_export_bool_device_async": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p]),
    "fr_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fr_import_bool_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_device_timers": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]),
    "fr_device_timers_latency": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]),
    "fr_device_timers_pair": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    "fr_shard_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t,
                                C.POINTER(C.c_void_p), C.POINTER(MatchStats)]),
    "fr_shard_levels": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "fr_shard_jobs": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fr_shard_outputs": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fr_shard_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fr_shard_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "fr_shard_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "fr_shard_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(MatchStats)]),
    "fr_shard_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fr_schedule_match": (C.c_int, [C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.POINTER(FrJob), C.c_size_t, C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
}


def lib():
    """Load the in-tree libfheregex.so (fails loudly if it was not built).

    A process that also uses torch on the GPU imports torch first: the torch wheel
    bundles its own HIP runtime with the soname of /opt/rocm's, so loaded first it is the
    one runtime this library binds to; loaded second, torch finds no device."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C {HERE}` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc: int):
    if rc == FR_OK:
        return
    msg = lib().fr_last_error().decode(errors="replace")
    cls = {ERR_PARSE: ParseError, ERR_REF_PANIC: ReferencePanic, ERR_NO_DEVICE: NoDevice}.get(rc, FheRegexError)
    if rc == ERR_NON_ASCII:
        raise ValueError(msg)
    raise cls(rc, msg)


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u64p)


def seed_key(seed: int) -> bytes:
    """The 32-byte generator key that a 64-bit seed stands for (RngKey::from_seed):
    the seed, then six fixed words.  A keyed call with it draws a seeded call's words."""
    return (seed & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little") + b"".join(
        w.to_bytes(4, "little") for w in (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0))


def _rng_arg(seed):
    """The randomness argument of the key and encryption calls: (keyed, value).
    int: a 64-bit seed (reproducible: tests, benchmarks); 32 bytes: a 256-bit generator
    key; None: the OS CSPRNG (a NULL key)."""
    if seed is None:
        return True, None
    if isinstance(seed, (bytes, bytearray, memoryview)):
        key = bytes(seed)
        if len(key) != 32:
            raise ValueError(f"a generator key is 32 bytes, not {len(key)}")
        return True, key
    if isinstance(seed, (int, np.integer)):
        return False, int(seed) & 0xFFFFFFFFFFFFFFFF
    raise TypeError("seed: an int (seeded), 32 bytes (keyed) or None (OS randomness)")


RING_RNS, RING_FFT = 0, 1  # fheregex.h FR_RING_*


def default_params(k: Optional[int] = None, N: Optional[int] = None, ring: Optional[int] = None) -> Params:
    p = Params()
    _check(lib().fr_default_params(C.byref(p)))
    if k is not None:
        p.k = k
    if N is not None:
        p.N = N
    if ring is not None:
        p.ring = ring
    elif (p.k, p.N) not in ((1, 2048), (2, 1024)):
        p.ring = RING_RNS  # the FFT ring is built for k = 1, N = 2048 and k = 2, N = 1024
    return p


def parse(pattern: str, grammar: int = GRAMMAR_REFERENCE) -> str:
    """Canonical AST string (parser.rs:146-185; GRAMMAR_EXT: the opt-in class extension)."""
    size = 1 << 16
    while True:
        buf = C.create_string_buffer(size)
        rc = lib().fr_parse_ex(pattern.encode("latin-1"), grammar, buf, len(buf))
        if rc == ERR_INVALID and size < (1 << 28) and b"buffer too small" in lib().fr_last_error():
            size <<= 2
            continue
        _check(rc)
        return buf.value.decode()


def plain_match(content: bytes | str, pattern: str, lowering: int = LOWER_THRESHOLD,
                start_lo: int = 0, start_hi: Optional[int] = None, engine: int = ENGINE_ENUMERATE,
                grammar: int = GRAMMAR_REFERENCE) -> PlainResult:
    """Host-only symbolic run: reference counters + plaintext result of the
    recorded circuit and of the lowered PBS program."""
    if isinstance(content, str):
        content = content.encode("latin-1")
    hi = len(content) if start_hi is None else start_hi
    r = PlainResult()
    _check(lib().fr_plain_match_g(content, len(content), pattern.encode("latin-1"), start_lo, hi, lowering, engine,
                                  grammar, C.byref(r)))
    return r


COST_COUNTED, COST_PANIC, COST_MEMORY = 0, 1, 2


def enumeration_cost(pattern: str, n_chars: int, start_lo: int = 0, start_hi: Optional[int] = None,
                     cap: int = 1 << 22, enumerate: bool = False, grammar: int = GRAMMAR_REFERENCE,
                     mem_bytes: int = 0, with_outcome: bool = False):
    """(counted, enumerated): the reference enumeration's variant count from the AST
    (None without a count: where it would panic, or past the counter's memo bound
    mem_bytes, 0 = AUTO's) and, if asked, by enumerating; both saturate at cap + 1.
    with_outcome: (outcome, counted, enumerated), outcome one of COST_*."""
    hi = n_chars if start_hi is None else start_hi
    o, c, e = C.c_int32(), C.c_uint64(), C.c_uint64()
    _check(lib().fr_debug_enumeration_cost(pattern.encode("latin-1"), grammar, n_chars, start_lo, hi, cap, mem_bytes,
                                           int(enumerate), C.byref(o), C.byref(c), C.byref(e)))
    counted = c.value if o.value == COST_COUNTED else None
    enumerated = e.value if enumerate else None
    return (o.value, counted, enumerated) if with_outcome else (counted, enumerated)


def plain_match_parts(content: bytes | str, pattern: str, start_lo: int, start_hi: int, max_parts: int,
                      lowering: int = LOWER_THRESHOLD, engine: int = ENGINE_ENUMERATE,
                      grammar: int = GRAMMAR_REFERENCE):
    """Host-only run of fr_has_match_parts' program: (PlainResult with result_lowered =
    the OR of the parts, [plaintext value of each part])"""
    if isinstance(content, str):
        content = content.encode("latin-1")
    r = PlainResult()
    vals = (C.c_int32 * max_parts)()
    n = C.c_size_t()
    _check(lib().fr_plain_match_parts(content, len(content), pattern.encode("latin-1"), start_lo, start_hi, lowering,
                                      engine, grammar, max_parts, C.byref(r), vals, C.byref(n)))
    return r, list(vals)[:n.value]


def plain_match_starts(content: bytes | str, pattern: str, start_lo: int = 0, start_hi: Optional[int] = None,
                       lowering: int = LOWER_THRESHOLD, engine: int = ENGINE_ENUMERATE,
                       grammar: int = GRAMMAR_REFERENCE):
    """Host-only run of fr_match_starts' merged program: (PlainResult, [value per start of the
    lowered program], [value per start of the start's recorded circuit])"""
    if isinstance(content, str):
        content = content.encode("latin-1")
    hi = len(content) if start_hi is None else start_hi
    r = PlainResult()
    cap = max(hi - start_lo, 1)
    low, rec = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = C.c_size_t()
    _check(lib().fr_plain_match_starts(content, len(content), pattern.encode("latin-1"), start_lo, hi, lowering,
                                       engine, grammar, C.byref(r), low, rec, cap, C.byref(n)))
    return r, list(low)[:n.value], list(rec)[:n.value]


class Context:
    """One fr_ctx: params, keys, device arena.  device=-1: host-only."""

    def __init__(self, device: int = 0, params: Optional[Params] = None):
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        _check(lib().fr_ctx_create(C.byref(self.params), device, C.byref(h)))
        self.h = h
        self.device = device
        self.big = self.params.k * self.params.N
        self.lwe_len = self.big + 1

    def close(self):
        if getattr(self, "h", None):
            lib().fr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> str:
        buf = C.create_string_buffer(256)
        _check(lib().fr_device_info(self.h, buf, 256))
        return buf.value.decode()

    # keys
    def load_client_key(self, blob: bytes):
        _check(lib().fr_load_client_key(self.h, blob, len(blob)))

    def gen_client_key(self, seed=None):
        """gen_keys_radix(&PARAM_MESSAGE_2_CARRY_2, 4) (ciphertext.rs:44): a fresh
        uniform binary client key.  `seed`: None draws from the OS CSPRNG (as the
        reference does), 32 bytes are a 256-bit generator key, an int is a 64-bit seed
        (reproducible; tests and benchmarks)."""
        keyed, v = _rng_arg(seed)
        _check(lib().fr_gen_client_key_keyed(self.h, v) if keyed else lib().fr_gen_client_key(self.h, v))

    def serialize_client_key(self) -> bytes:
        """bincode RadixClientKey (engine.rs:238-246 generate_test_keys): the layout
        load_client_key reads; a loaded key comes back byte for byte."""
        n = C.c_size_t()
        _check(lib().fr_serialize_client_key(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_serialize_client_key(self.h, buf, n.value, C.byref(n)))
        return buf.raw

    def gen_server_key(self, seed=None, compact=False):
        """ServerKey::new (engine.rs:252): on the GPU for the FFT ring (KEYGEN_AUTO),
        else on the host; both give the same key bit for bit.  `seed` as in
        gen_client_key.  A server key from an int seed must not leave the client: whoever
        guesses the seed recomputes the key's noise and solves for the client key.
        compact=True (FFT ring): the compact form, whose masks are ChaCha20 words of a
        public mask key, so that export_server_key_compact ships the bodies only."""
        keyed, v = _rng_arg(seed)
        L = lib()
        if compact:
            f = L.fr_gen_server_key_compact_keyed if keyed else L.fr_gen_server_key_compact
        else:
            f = L.fr_gen_server_key_keyed if keyed else L.fr_gen_server_key
        _check(f(self.h, v))

    def set_keygen(self, where: int):
        """KEYGEN_AUTO (device when present, FFT ring), KEYGEN_HOST or KEYGEN_DEVICE."""
        _check(lib().fr_set_keygen(self.h, where))

    def export_server_key(self):
        a, b = C.c_size_t(), C.c_size_t()
        _check(lib().fr_server_key_sizes(self.h, C.byref(a), C.byref(b)))
        ksk = np.zeros(a.value, dtype=np.uint64)
        bsk = np.zeros(b.value, dtype=np.uint64)
        _check(lib().fr_export_server_key(self.h, _p(ksk), len(ksk), _p(bsk), len(bsk)))
        return ksk, bsk

    def load_server_key(self, ksk: np.ndarray, bsk: np.ndarray):
        """install an exported server key (export_server_key's arrays): a server context
        holding only sk, as has_match(sk, ...) takes it (engine.rs:8); no client key needed"""
        k = np.ascontiguousarray(ksk, dtype=np.uint64)
        b = np.ascontiguousarray(bsk, dtype=np.uint64)
        _check(lib().fr_load_server_key(self.h, _p(k), len(k), _p(b), len(b)))

    def server_key_compact_size(self) -> int:
        n = C.c_size_t()
        _check(lib().fr_server_key_compact_size(self.h, C.byref(n)))
        return n.value

    def export_server_key_compact(self) -> bytes:
        """the compact wire blob (fheregex.h: magic, parameters, mask key, bodies) of a key
        generated with compact=True or loaded from such a blob"""
        n = C.c_size_t()
        _check(lib().fr_export_server_key_compact(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_export_server_key_compact(self.h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def load_server_key_compact(self, blob: bytes):
        """install a compact server key: no client key needed; a device context uploads
        the bodies and expands the masks on the GPU"""
        blob = bytes(blob)
        _check(lib().fr_load_server_key_compact(self.h, blob, len(blob)))

    # packed results
    def gen_packing_key(self, seed=None, compact=False):
        """the optional packing key (fheregex.h "packed results"; 201 MB): on the GPU on a
        device context, word for word the host generator's rows.  `seed` as in gen_client_key.
        compact=True: the compact form, whose masks are ChaCha20 words of a public mask key
        and whose bodies are rounded to 40 bits, so that export_packing_key_compact ships
        63 MB; a compact key from an int seed must not leave the client."""
        keyed, v = _rng_arg(seed)
        L = lib()
        if compact:
            f = L.fr_gen_packing_key_compact_keyed if keyed else L.fr_gen_packing_key_compact
        else:
            f = L.fr_gen_packing_key_keyed if keyed else L.fr_gen_packing_key
        _check(f(self.h, v))

    def packing_key_size(self) -> int:
        n = C.c_size_t()
        _check(lib().fr_packing_key_size(self.h, C.byref(n)))
        return n.value

    def export_packing_key(self) -> np.ndarray:
        """the packing key's wire blob as a uint8 array (load_packing_key takes it back)"""
        n = C.c_size_t()
        _check(lib().fr_export_packing_key(self.h, None, 0, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        _check(lib().fr_export_packing_key(self.h, buf.ctypes.data, n.value, C.byref(n)))
        return buf

    def load_packing_key(self, blob):
        """install a packing key blob (bytes or a uint8 array): no client key needed"""
        b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob,
                                 dtype=np.uint8)
        _check(lib().fr_load_packing_key(self.h, b.ctypes.data, len(b)))

    def packing_key_compact_size(self) -> int:
        n = C.c_size_t()
        _check(lib().fr_packing_key_compact_size(self.h, C.byref(n)))
        return n.value

    def export_packing_key_compact(self) -> np.ndarray:
        """the compact wire blob (fheregex.h: header, mask key, two planes of 40-bit bodies)
        as a uint8 array, of a key generated with compact=True or loaded from such a blob"""
        n = C.c_size_t()
        _check(lib().fr_export_packing_key_compact(self.h, None, 0, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        _check(lib().fr_export_packing_key_compact(self.h, buf.ctypes.data, n.value, C.byref(n)))
        return buf

    def load_packing_key_compact(self, blob):
        """install a compact packing key blob (bytes or a uint8 array): no client key needed;
        a device context uploads the planes and rebuilds masks and bodies on the GPU"""
        b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob,
                                 dtype=np.uint8)
        _check(lib().fr_load_packing_key_compact(self.h, b.ctypes.data, len(b)))

    def gen_packing_rows(self, seed, row_lo: int, row_hi: int, compact=False) -> np.ndarray:
        """rows [row_lo, row_hi) of the packing key gen_packing_key(seed, compact) draws, on
        the host: (rows, (k+1) N) words"""
        keyed, v = _rng_arg(seed)
        key = v if keyed else seed_key(v)
        W = (self.params.k + 1) * self.params.N
        out = np.zeros((row_hi - row_lo, W), dtype=np.uint64)
        f = lib().fr_gen_packing_rows_compact_keyed if compact else lib().fr_gen_packing_rows_keyed
        _check(f(self.h, key, row_lo, row_hi, _p(out)))
        return out

    def packed_result_size(self, n: int) -> int:
        b = C.c_size_t()
        _check(lib().fr_packed_result_size(self.h, n, C.byref(b)))
        return b.value

    def pack_bools_words(self, handles: Sequence[int]) -> np.ndarray:
        """the (k+1) N words of the boolean handles' packed GLWE (fr_pack_bools)"""
        hs = (C.c_uint32 * len(handles))(*handles)
        out = np.zeros((self.params.k + 1) * self.params.N, dtype=np.uint64)
        _check(lib().fr_pack_bools(self.h, hs, len(handles), _p(out)))
        return out

    def pack_bools(self, handles: Sequence[int]) -> bytes:
        """up to N boolean handles as one packed result blob (32,792 bytes), which
        decrypt_packed opens on a context holding the client key"""
        hs = (C.c_uint32 * len(handles))(*handles)
        n = C.c_size_t()
        _check(lib().fr_pack_bools_blob(self.h, hs, len(handles), None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_pack_bools_blob(self.h, hs, len(handles), buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def decrypt_packed(self, blob: bytes) -> List[int]:
        """the bits of a packed result blob (client key needed)"""
        blob = bytes(blob)
        n = C.c_size_t()
        _check(lib().fr_decrypt_packed(self.h, blob, len(blob), None, C.byref(n)))
        bits = (C.c_uint8 * n.value)()
        _check(lib().fr_decrypt_packed(self.h, blob, len(blob), bits, C.byref(n)))
        return list(bits)

    # compact reply: every sent coefficient rounded to 16 bits, 32 + 2 (kN + n) bytes
    def packed_compact_size(self, n: int) -> int:
        b = C.c_size_t()
        _check(lib().fr_packed_compact_size(self.h, n, C.byref(b)))
        return b.value

    def pack_bools_compact(self, handles: Sequence[int]) -> bytes:
        """pack_bools in the compact form (fr_pack_bools_compact): the blob decrypt_packed_compact opens"""
        hs = (C.c_uint32 * len(handles))(*handles)
        n = C.c_size_t()
        _check(lib().fr_pack_bools_compact(self.h, hs, len(handles), None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_pack_bools_compact(self.h, hs, len(handles), buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def compress_packed(self, words: np.ndarray, n: int) -> bytes:
        """the compact blob of a packed GLWE's (k+1) N words carrying n booleans, on the host"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if len(words) != (self.params.k + 1) * self.params.N:
            raise ValueError("compress_packed: (k+1) N words")
        sz = C.c_size_t()
        _check(lib().fr_compress_packed(self.h, None, n, None, 0, C.byref(sz)))
        buf = C.create_string_buffer(sz.value)
        _check(lib().fr_compress_packed(self.h, _p(words), n, buf, sz.value, C.byref(sz)))
        return buf.raw[:sz.value]

    def expand_packed_compact(self, blob: bytes) -> Tuple[np.ndarray, int]:
        """(the (k+1) N words a compact blob installs, its n)"""
        blob = bytes(blob)
        n = C.c_size_t()
        out = np.zeros((self.params.k + 1) * self.params.N, dtype=np.uint64)
        _check(lib().fr_expand_packed_compact(self.h, blob, len(blob), _p(out), C.byref(n)))
        return out, n.value

    def decrypt_packed_compact(self, blob: bytes) -> List[int]:
        """the bits of a compact packed result blob (client key needed)"""
        blob = bytes(blob)
        n = C.c_size_t()
        _check(lib().fr_decrypt_packed_compact(self.h, blob, len(blob), None, C.byref(n)))
        bits = (C.c_uint8 * n.value)()
        _check(lib().fr_decrypt_packed_compact(self.h, blob, len(blob), bits, C.byref(n)))
        return list(bits)

    def pack_lwes(self, lwes: Optional[np.ndarray], w=None, off=None, n: Optional[int] = None) -> np.ndarray:
        """the packing keyswitch in plain host loops (fr_pack_lwes) of the booleans
        off[j] 2^58 + w[j] lwes[j]: the (k+1) N words the device must give"""
        if lwes is not None:
            lwes = np.ascontiguousarray(lwes, dtype=np.uint64).reshape(-1, self.lwe_len)
            n = len(lwes)
        wa = None if w is None else (C.c_int32 * n)(*[int(x) for x in w])
        oa = None if off is None else (C.c_int32 * n)(*[int(x) for x in off])
        out = np.zeros((self.params.k + 1) * self.params.N, dtype=np.uint64)
        _check(lib().fr_pack_lwes(self.h, None if lwes is None else _p(lwes), wa, oa, n, _p(out)))
        return out

    def packed_phase(self, words: np.ndarray) -> np.ndarray:
        """the N phase words of a packed GLWE under the client key"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        out = np.zeros(self.params.N, dtype=np.uint64)
        _check(lib().fr_packed_phase(self.h, _p(words), _p(out)))
        return out

    def dev_packing_limb_column(self, col: int) -> np.ndarray:
        """column `col` of the packing key's byte-limb operand, recombined: the 3 kN torus words"""
        out = np.zeros(3 * self.big, dtype=np.uint64)
        _check(lib().fr_dev_packing_limb_column(self.h, col, _p(out)))
        return out

    def pack_timers(self) -> List[float]:
        """ms of the last pack_bools' stages under set_profiling: digits, GEMM, rotate-sum"""
        ms = (C.c_double * 3)()
        _check(lib().fr_device_timers_pack(self.h, ms))
        return list(ms)

    def pack_timers_compact(self) -> List[float]:
        """pack_timers and, fourth, the compact form's rounding kernel, of the last pack of
        either form (match_starts_packed's included)"""
        ms = (C.c_double * 4)()
        _check(lib().fr_device_timers_pack_compact(self.h, ms))
        return list(ms)

    def key_load_timers(self) -> List[float]:
        """ms of the last load_server_key_compact's stages under set_profiling: H2D copy,
        KSK expansion, BSK expansion, KSK limbs, BSK Fourier transform"""
        ms = (C.c_double * 5)()
        _check(lib().fr_device_timers_key_load(self.h, ms))
        return list(ms)

    def packing_key_load_timers(self) -> List[float]:
        """ms of the last load_packing_key_compact's stages under set_profiling: H2D copy,
        expansion, byte limbs"""
        ms = (C.c_double * 3)()
        _check(lib().fr_device_timers_packing_key_load(self.h, ms))
        return list(ms)

    def set_lowering(self, mode: int):
        _check(lib().fr_set_lowering(self.h, mode))

    def set_engine(self, engine: int):
        """ENGINE_AUTO (default), ENGINE_ENUMERATE (the reference's variant
        enumeration) or ENGINE_MERGED (state merging; same decrypted result)."""
        _check(lib().fr_set_engine(self.h, engine))

    def set_grammar(self, grammar: int):
        """GRAMMAR_REFERENCE (default: parser.rs exactly) or GRAMMAR_EXT (also
        bare digits and mixed bracket classes such as [a-z0-9]; beyond the reference)."""
        _check(lib().fr_set_grammar(self.h, grammar))

    def set_multi_value(self, on: bool):
        _check(lib().fr_set_multi_value(self.h, int(on)))

    def set_plan_cache(self, capacity: int):
        """Plans kept for repeat has_match calls (0: off, frees the cached plans)."""
        _check(lib().fr_set_plan_cache(self.h, capacity))

    def set_async(self, on: bool):
        """has_match returns once its launches are enqueued (default) or blocks (False)."""
        _check(lib().fr_set_async(self.h, int(on)))

    def set_lanes(self, n: int):
        """fr_set_lanes: consecutive asynchronous matches round-robin over n streams of this
        context (one key, a plan copy per lane); every other call waits for them device-side."""
        _check(lib().fr_set_lanes(self.h, int(n)))

    def set_plan_cache_slots(self, max_slots: int):
        """Bound on the intermediate arena slots held by all cached plans."""
        _check(lib().fr_set_plan_cache_slots(self.h, max_slots))

    def plan_cache_stats(self):
        v = [C.c_uint64() for _ in range(4)]
        _check(lib().fr_plan_cache_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("entries", "slots", "hits", "misses"), (x.value for x in v)))

    def arena_stats(self):
        """fr_debug_arena_stats, after a synchronisation of every lane: `slots` ever handed
        out and `free_slots` on the free list (their difference is held by handles and plans)"""
        v = [C.c_uint64() for _ in range(2)]
        _check(lib().fr_debug_arena_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("slots", "free_slots"), (x.value for x in v)))

    def handle_count(self) -> int:
        """fr_debug_handle_count: the handles not yet released"""
        v = C.c_uint64()
        _check(lib().fr_debug_handle_count(self.h, C.byref(v)))
        return v.value

    def set_profiling(self, on):
        """0/False off, 1/True blind-rotation timers, 2 also keyswitch timers (fr_set_profiling)."""
        _check(lib().fr_set_profiling(self.h, int(on)))

    # client side
    # `seed` of the three encryption calls: None draws masks and noise from the OS CSPRNG
    # (as the reference does), 32 bytes are a 256-bit generator key, an int is a 64-bit
    # seed (tests and benchmarks: two calls with one seed share masks and noise)
    def encrypt_str(self, s: bytes | str, seed=None) -> np.ndarray:
        if isinstance(s, str):
            s = s.encode("latin-1")
        keyed, v = _rng_arg(seed)
        out = np.zeros((len(s), 4, self.lwe_len), dtype=np.uint64)
        f = lib().fr_encrypt_str_keyed if keyed else lib().fr_encrypt_str
        _check(f(self.h, s, len(s), v, _p(out)))
        return out

    def encrypt_blocks(self, msgs, seed=None, first_block: int = 0) -> np.ndarray:
        m = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint8))
        keyed, v = _rng_arg(seed)
        out = np.zeros((len(m), self.lwe_len), dtype=np.uint64)
        f = lib().fr_encrypt_blocks_keyed if keyed else lib().fr_encrypt_blocks
        _check(f(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)), len(m), v, first_block, _p(out)))
        return out

    def decrypt_radix(self, blocks: np.ndarray) -> int:
        b = np.ascontiguousarray(blocks, dtype=np.uint64)
        v = C.c_uint64()
        _check(lib().fr_decrypt_radix(self.h, _p(b), C.byref(v)))
        return v.value

    def decode_block(self, lwe: np.ndarray) -> int:
        b = np.ascontiguousarray(lwe, dtype=np.uint64)
        v = C.c_uint32()
        _check(lib().fr_decode_block(self.h, _p(b), C.byref(v)))
        return v.value

    # arena
    def upload_radix(self, blocks: np.ndarray) -> List[int]:
        b = np.ascontiguousarray(blocks.reshape(-1, 4, self.lwe_len), dtype=np.uint64)
        out = (C.c_uint32 * b.shape[0])()
        _check(lib().fr_upload_radix(self.h, _p(b), b.shape[0], out))
        return list(out)

    def encrypt_upload_str(self, s: bytes | str, seed=None) -> List[int]:
        """encrypt_str on the device into content handles (same words as encrypt_str)."""
        if isinstance(s, str):
            s = s.encode("latin-1")
        keyed, v = _rng_arg(seed)
        out = (C.c_uint32 * len(s))()
        f = lib().fr_encrypt_upload_str_keyed if keyed else lib().fr_encrypt_upload_str
        _check(f(self.h, s, len(s), v, out))
        return list(out)

    # compact (seeded) content (fheregex.h): the bodies and a public mask key travel, the
    # server rebuilds the masks.  The C-ABI is keyed only: an int seed stands for seed_key(seed).
    @staticmethod
    def _compact_key(seed):
        keyed, v = _rng_arg(seed)
        return v if keyed else seed_key(v)

    def compact_content_size(self, n_blocks: int) -> int:
        n = C.c_size_t()
        _check(lib().fr_compact_content_size(self.h, n_blocks, C.byref(n)))
        return n.value

    def encrypt_str_compact(self, s: bytes | str, seed=None) -> bytes:
        """encrypt_str as a compact blob of 64 + 32 len(s) bytes (4 blocks per char)"""
        if isinstance(s, str):
            s = s.encode("latin-1")
        key = self._compact_key(seed)
        n = C.c_size_t()
        _check(lib().fr_encrypt_str_compact_keyed(self.h, s, len(s), key, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_encrypt_str_compact_keyed(self.h, s, len(s), key, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def encrypt_blocks_compact(self, msgs, seed=None, first_block: int = 0) -> bytes:
        """encrypt_blocks as a compact blob of 64 + 8 len(msgs) bytes"""
        m = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint8))
        mp = m.ctypes.data_as(C.POINTER(C.c_uint8))
        key = self._compact_key(seed)
        n = C.c_size_t()
        _check(lib().fr_encrypt_blocks_compact_keyed(self.h, mp, len(m), key, first_block, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_encrypt_blocks_compact_keyed(self.h, mp, len(m), key, first_block, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def expand_compact_content(self, blob: bytes) -> np.ndarray:
        """the full LWE words [n_blocks, lwe_len] of a compact blob, on the host; no key needed"""
        blob = bytes(blob)
        n = C.c_size_t()
        _check(lib().fr_expand_compact_content(self.h, blob, len(blob), None, 0, C.byref(n)))
        out = np.zeros((n.value, self.lwe_len), dtype=np.uint64)
        _check(lib().fr_expand_compact_content(self.h, blob, len(blob), _p(out), out.size, C.byref(n)))
        return out

    def _upload_compact(self, fn, blob, per_handle) -> List[int]:
        blob = bytes(blob)
        cap = max(0, len(blob) - 64) // (8 * per_handle)
        out = (C.c_uint32 * max(cap, 1))()
        n = C.c_size_t()
        _check(fn(self.h, blob, len(blob), out, cap, C.byref(n)))
        return list(out)[:n.value]

    def upload_compact_str(self, blob: bytes) -> List[int]:
        """a compact string blob expanded on the device into radix handles (as upload_radix);
        no client key needed; returns once enqueued"""
        return self._upload_compact(lib().fr_upload_compact_str, blob, 4)

    def upload_compact_blocks(self, blob: bytes) -> List[int]:
        """a compact blob expanded on the device into boolean handles (as upload_bool)"""
        return self._upload_compact(lib().fr_upload_compact_blocks, blob, 1)

    # ---- private search (fr_find*): an encrypted needle on encrypted content
    def needle_size(self, m: int) -> int:
        n = C.c_size_t()
        _check(lib().fr_needle_size(self.h, m, C.byref(n)))
        return n.value

    def encrypt_needle(self, masks: Sequence[Tuple[int, int]], seed=None) -> bytes:
        """fr_encrypt_needle_keyed: the needle blob of (lo_mask, hi_mask) per character
        (needle_masks); seed None: the OS CSPRNG, else an int seed or a 32-byte key"""
        flat = [v for lo_hi in masks for v in lo_hi]
        arr = (C.c_uint16 * max(len(flat), 1))(*flat)
        n = C.c_size_t()
        key = self._compact_key(seed)
        _check(lib().fr_encrypt_needle_keyed(self.h, arr, len(masks), key, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_encrypt_needle_keyed(self.h, arr, len(masks), key, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def expand_needle(self, blob: bytes) -> np.ndarray:
        """fr_expand_needle: the selectors [2 m][k + 1][N] of a needle blob (no key needed)"""
        m = C.c_size_t()
        _check(lib().fr_expand_needle(self.h, blob, len(blob), None, 0, C.byref(m)))
        out = np.zeros((2 * m.value, self.params.k + 1, self.params.N), dtype=np.uint64)
        _check(lib().fr_expand_needle(self.h, blob, len(blob), _p(out), out.size, C.byref(m)))
        return out

    # ---- byte-table needles: one 256-entry table per character, clear content only
    def needle_bytes_size(self, m: int) -> int:
        n = C.c_size_t()
        _check(lib().fr_needle_bytes_size(self.h, m, C.byref(n)))
        return n.value

    def encrypt_needle_bytes(self, tables: Sequence[int], seed=None) -> bytes:
        """fr_encrypt_needle_bytes_keyed: the byte-table needle blob of one 256-bit set per
        character (needle_tables: bit b of the int accepts byte b); seed as in encrypt_needle"""
        flat = _tables_bytes(tables)
        n = C.c_size_t()
        key = self._compact_key(seed)
        _check(lib().fr_encrypt_needle_bytes_keyed(self.h, flat, len(tables), key, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_encrypt_needle_bytes_keyed(self.h, flat, len(tables), key, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def expand_needle_bytes(self, blob: bytes) -> np.ndarray:
        """fr_expand_needle_bytes: the selectors [ceil(256 m / N)][k + 1][N] of a byte-table needle
        blob (no key needed)"""
        m = C.c_size_t()
        _check(lib().fr_expand_needle_bytes(self.h, blob, len(blob), None, 0, C.byref(m)))
        tpg = self.params.N // 256
        out = np.zeros(((m.value + tpg - 1) // tpg, self.params.k + 1, self.params.N), dtype=np.uint64)
        _check(lib().fr_expand_needle_bytes(self.h, blob, len(blob), _p(out), out.size, C.byref(m)))
        return out

    def upload_needle(self, blob: bytes) -> "Needle":
        h = C.c_void_p()
        _check(lib().fr_upload_needle(self.h, blob, len(blob), C.byref(h)))
        return Needle(self, h)

    def _find(self, fn, content, needle, lo, hi, starts, clear=False):
        """one fr_find* / fr_find_clear* / fr_scan_clear call over the starts [lo, hi) (default: all
        of the content): ([handles], MatchStats).  clear: the content is a text, else handles"""
        if needle.h is None:
            raise ValueError("needle is closed")
        if clear:
            arr = content = _text_bytes(content)
        else:
            content = np.ascontiguousarray(content, dtype=np.uint32)
            arr = content.ctypes.data_as(C.POINTER(C.c_uint32))
        lo = 0 if lo is None else lo
        hi = len(content) if hi is None else hi
        n_out = max(hi - lo, 0) if starts else 1
        out = (C.c_uint32 * max(n_out, 1))()
        st = MatchStats()
        _check(fn(self.h, arr, len(content), needle.h, lo, hi, out, C.byref(st)))
        return list(out)[:n_out], st

    def find(self, content: Sequence[int], needle: "Needle", lo: Optional[int] = None, hi: Optional[int] = None):
        """fr_find: (boolean handle, MatchStats): the needle matches at some start of [lo, hi)"""
        out, st = self._find(lib().fr_find, content, needle, lo, hi, False)
        return out[0], st

    def find_starts(self, content: Sequence[int], needle: "Needle", lo: Optional[int] = None,
                    hi: Optional[int] = None, stats: bool = False):
        """fr_find_starts: one boolean handle per start offset of [lo, hi)"""
        hs, st = self._find(lib().fr_find_starts, content, needle, lo, hi, True)
        return (hs, st) if stats else hs

    def dev_blind_rotate_acc(self, ks: np.ndarray, accs: np.ndarray) -> np.ndarray:
        """fr_dev_blind_rotate_acc: one selector launch, rotation i from the GLWE accs[i]"""
        a = np.ascontiguousarray(ks.reshape(-1, self.params.n + 1), dtype=np.uint64)
        g = np.ascontiguousarray(accs, dtype=np.uint64).reshape(a.shape[0], (self.params.k + 1) * self.params.N)
        out = np.zeros((a.shape[0], self.lwe_len), dtype=np.uint64)
        _check(lib().fr_dev_blind_rotate_acc(self.h, _p(a), _p(g), a.shape[0], _p(out)))
        return out

    # ---- private search over clear content (fr_find_clear*): the server's own bytes
    def find_clear(self, text: bytes | str, needle: "Needle", lo: Optional[int] = None, hi: Optional[int] = None):
        """fr_find_clear: (boolean handle, MatchStats): the needle matches the clear text at some
        start of [lo, hi)"""
        out, st = self._find(lib().fr_find_clear, text, needle, lo, hi, False, clear=True)
        return out[0], st

    def find_clear_starts(self, text: bytes | str, needle: "Needle", lo: Optional[int] = None,
                          hi: Optional[int] = None, stats: bool = False):
        """fr_find_clear_starts: one boolean handle per start offset of [lo, hi)"""
        hs, st = self._find(lib().fr_find_clear_starts, text, needle, lo, hi, True, clear=True)
        return (hs, st) if stats else hs

    # ---- scan of a long clear text (fr_scan_clear*): one rotation per distinct window
    def scan_clear(self, text: bytes | str, needle: "Needle", lo: Optional[int] = None, hi: Optional[int] = None):
        """fr_scan_clear: find_clear's (boolean handle, MatchStats) at one rotation per distinct
        window of the text"""
        out, st = self._find(lib().fr_scan_clear, text, needle, lo, hi, False, clear=True)
        return out[0], st

    def scan_clear_starts(self, text: bytes | str, needle: "Needle", lo: Optional[int] = None,
                          hi: Optional[int] = None, compact: bool = True, stats: bool = False):
        """fr_scan_clear_starts: the blobs of the chunks of N starts of [lo, hi), back to back
        (compact: FRCPRES1, else FRPKRES1), with no handle in between; with stats=True also the
        MatchStats"""
        if needle.h is None:
            raise ValueError("needle is closed")
        b = _text_bytes(text)
        lo = 0 if lo is None else lo
        hi = len(b) if hi is None else hi
        n = C.c_size_t()
        st = MatchStats()
        args = (self.h, b, len(b), needle.h, lo, hi, int(compact))
        _check(lib().fr_scan_clear_starts(*args, None, 0, C.byref(n), None))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(lib().fr_scan_clear_starts(*args, buf, n.value, C.byref(n), C.byref(st)))
        return (buf.raw[:n.value], st) if stats else buf.raw[:n.value]

    def scan_classes(self) -> Tuple[int, int]:
        """fr_scan_classes: (D, padded D) of this context's last scan"""
        d, dp = C.c_uint64(), C.c_uint64()
        _check(lib().fr_scan_classes(self.h, C.byref(d), C.byref(dp)))
        return d.value, dp.value

    def dev_pack_mapped(self, handles: Sequence[int], map_: Sequence[int], compact: bool = False) -> bytes:
        """fr_dev_pack_mapped: the mapped pack alone; start j is the boolean handles[map_[j]]
        (map_[j] < 0: the constant 0) -> the blob of the len(map_) starts"""
        hs = (C.c_uint32 * max(len(handles), 1))(*handles)
        mp = (C.c_int32 * max(len(map_), 1))(*[int(v) for v in map_])
        n = C.c_size_t()
        args = (self.h, hs, len(handles), mp, len(map_), int(compact))
        _check(lib().fr_dev_pack_mapped(*args, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_dev_pack_mapped(*args, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def pack_lwes_mapped(self, lwes: Optional[np.ndarray], map_: Sequence[int], w=None, off=None,
                         n_rows: Optional[int] = None) -> np.ndarray:
        """fr_pack_lwes_mapped: pack_lwes where start j reads row map_[j] of the n_rows booleans
        off[r] 2^58 + w[r] lwes[r] (map_[j] < 0: the constant 0), in plain host loops"""
        if lwes is not None:
            lwes = np.ascontiguousarray(lwes, dtype=np.uint64).reshape(-1, self.lwe_len)
            n_rows = len(lwes)
        wa = None if w is None else (C.c_int32 * max(n_rows, 1))(*[int(x) for x in w])
        oa = None if off is None else (C.c_int32 * max(n_rows, 1))(*[int(x) for x in off])
        mp = (C.c_int32 * max(len(map_), 1))(*[int(v) for v in map_])
        out = np.zeros((self.params.k + 1) * self.params.N, dtype=np.uint64)
        _check(lib().fr_pack_lwes_mapped(self.h, None if lwes is None else _p(lwes), wa, oa, n_rows, mp, len(map_),
                                         _p(out)))
        return out

    def dev_select_sum(self, needle: "Needle", text: bytes | str, sums: Sequence[Sequence[Tuple[int, int, int]]]
                       ) -> np.ndarray:
        """fr_dev_select_sum: the extract-sum kernel alone; sums[i] is the list of sum i's terms
        (selector q, content position pos, half h) -> [len(sums)][k N + 1] u64"""
        if needle.h is None:
            raise ValueError("needle is closed")
        b = _text_bytes(text)
        flat = [int(v) for s in sums for t in s for v in t]
        terms = (C.c_int32 * max(len(flat), 1))(*flat)
        counts = (C.c_int32 * max(len(sums), 1))(*[len(s) for s in sums])
        out = np.zeros((len(sums), self.lwe_len), dtype=np.uint64)
        _check(lib().fr_dev_select_sum(self.h, needle.h, b, len(b), terms, counts, len(sums), _p(out)))
        return out

    def select_sum_timer(self) -> float:
        """ms of the last dev_select_sum's kernel under set_profiling"""
        ms = C.c_double()
        _check(lib().fr_dev_select_sum_ms(self.h, C.byref(ms)))
        return ms.value

    def content_expand_timer(self) -> float:
        """ms of the last upload_compact_*'s expansion kernel under set_profiling"""
        ms = C.c_double()
        _check(lib().fr_device_timers_content(self.h, C.byref(ms)))
        return ms.value

    def serialize_radix(self, blocks: np.ndarray, degree: int = 3) -> bytes:
        """bincode RadixCiphertext (tfhe-rs 0.2 layout, [ext] unverified) of one radix (4 blocks)."""
        b = np.ascontiguousarray(blocks.reshape(-1, self.lwe_len), dtype=np.uint64)
        n = C.c_size_t()
        _check(lib().fr_radix_serialize(self.h, _p(b), b.shape[0], degree, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_radix_serialize(self.h, _p(b), b.shape[0], degree, buf, n.value, C.byref(n)))
        return buf.raw

    def deserialize_radix(self, data: bytes) -> np.ndarray:
        n = C.c_size_t()
        _check(lib().fr_radix_deserialize(self.h, data, len(data), None, 0, C.byref(n)))
        out = np.zeros((n.value, self.lwe_len), dtype=np.uint64)
        _check(lib().fr_radix_deserialize(self.h, data, len(data), _p(out), n.value, C.byref(n)))
        return out

    def upload_bool(self, lwes: np.ndarray) -> List[int]:
        b = np.ascontiguousarray(lwes.reshape(-1, self.lwe_len), dtype=np.uint64)
        out = (C.c_uint32 * b.shape[0])()
        _check(lib().fr_upload_bool(self.h, _p(b), b.shape[0], out))
        return list(out)

    def download_radix(self, h: int) -> np.ndarray:
        out = np.zeros((4, self.lwe_len), dtype=np.uint64)
        _check(lib().fr_download_radix(self.h, h, _p(out)))
        return out

    def release(self, h: int):
        _check(lib().fr_release(self.h, h))

    def trivial(self, v: int) -> int:
        out = C.c_uint32()
        _check(lib().fr_trivial(self.h, v, C.byref(out)))
        return out.value

    # eager ops (the smart_* replacements)
    def _op1c(self, fn, a, c):
        out = C.c_uint32()
        _check(fn(self.h, a, c, C.byref(out)))
        return out.value

    def eq_const(self, a, c): return self._op1c(lib().fr_eq_const, a, c)
    def gt_const(self, a, c): return self._op1c(lib().fr_gt_const, a, c)
    def le_const(self, a, c): return self._op1c(lib().fr_le_const, a, c)
    def and_(self, a, b): return self._op1c(lib().fr_and, a, b)
    def or_(self, a, b): return self._op1c(lib().fr_or, a, b)

    def not_(self, a):
        out = C.c_uint32()
        _check(lib().fr_not(self.h, a, C.byref(out)))
        return out.value

    def or_many(self, hs: Sequence[int]) -> int:
        arr = (C.c_uint32 * len(hs))(*hs)
        out = C.c_uint32()
        _check(lib().fr_or_many(self.h, arr, len(hs), C.byref(out)))
        return out.value

    def or_each(self, groups: Sequence[Sequence[int]]) -> List[int]:
        """one OR per group of <= 16 booleans, all groups in one launch (fr_run_gates:
        independent sign gates, the threshold OR of fr_or_many): the final bitor of
        many start-sharded matches at once"""
        gates = []
        for grp in groups:
            if not 1 <= len(grp) <= 16:
                raise ValueError("or_each: 1..16 booleans per group")
            g = Gate()
            g.n_in, g.offset, g.kind = len(grp), -1, GATE_SIGN
            for q, h in enumerate(grp):
                g.in_[q], g.in_block[q], g.in_w[q] = h, 0, 1
            gates.append(g)
        return self.run_gates(gates) if gates else []

    def run_gates(self, gates: Sequence[Gate]) -> List[int]:
        arr = (Gate * len(gates))(*gates)
        _check(lib().fr_run_gates(self.h, arr, len(gates)))
        return [g.out for g in arr]

    def has_match(self, content: Sequence[int], pattern: str, start_lo: Optional[int] = None,
                  start_hi: Optional[int] = None):
        """engine.rs:8-42 over content handles (a sequence, or a uint32 numpy array: no copy)"""
        if isinstance(content, np.ndarray):
            content = np.ascontiguousarray(content, dtype=np.uint32)
            arr = content.ctypes.data_as(C.POINTER(C.c_uint32))
        else:
            arr = (C.c_uint32 * len(content))(*content)
        out = C.c_uint32()
        st = MatchStats()
        if start_lo is None and start_hi is None:
            _check(lib().fr_has_match(self.h, arr, len(content), pattern.encode("latin-1"), C.byref(out), C.byref(st)))
        else:
            lo = 0 if start_lo is None else start_lo
            hi = len(content) if start_hi is None else start_hi
            _check(lib().fr_has_match_range(self.h, arr, len(content), pattern.encode("latin-1"), lo, hi,
                                            C.byref(out), C.byref(st)))
        return out.value, st

    def has_match_parts(self, content: Sequence[int], pattern: str, start_lo: int, start_hi: int, max_parts: int):
        """fr_has_match_parts: ([<= max_parts boolean handles whose OR is the range's
        match], stats) -- a start shard's result for a caller-side OR over shards"""
        content = np.ascontiguousarray(content, dtype=np.uint32)
        arr = content.ctypes.data_as(C.POINTER(C.c_uint32))
        out = (C.c_uint32 * max_parts)()
        n = C.c_size_t()
        st = MatchStats()
        _check(lib().fr_has_match_parts(self.h, arr, len(content), pattern.encode("latin-1"), start_lo, start_hi,
                                        max_parts, out, C.byref(n), C.byref(st)))
        return list(out)[:n.value], st

    def match_starts(self, content: Sequence[int], pattern: str, lo: Optional[int] = None,
                     hi: Optional[int] = None, stats: bool = False):
        """fr_match_starts: one boolean handle per start offset of [lo, hi) (default: every
        offset of the content), the encrypted "the pattern matches starting here"; with
        stats=True also the MatchStats"""
        content = np.ascontiguousarray(content, dtype=np.uint32)
        arr = content.ctypes.data_as(C.POINTER(C.c_uint32))
        lo = 0 if lo is None else lo
        hi = len(content) if hi is None else hi
        out = (C.c_uint32 * max(hi - lo, 1))()
        st = MatchStats()
        _check(lib().fr_match_starts(self.h, arr, len(content), pattern.encode("latin-1"), lo, hi, out, C.byref(st)))
        hs = list(out)[:max(hi - lo, 0)]
        return (hs, st) if stats else hs

    def match_starts_packed(self, content: Sequence[int], pattern: str, lo: Optional[int] = None,
                            hi: Optional[int] = None, compact: bool = True, stats: bool = False):
        """fr_match_starts_packed: the booleans of match_starts over [lo, hi) (at most N starts)
        as one reply blob -- compact: the FRCPRES1 form decrypt_packed_compact opens, else the
        FRPKRES1 form of pack_bools -- with no handle in between; with stats=True also the
        MatchStats"""
        content = np.ascontiguousarray(content, dtype=np.uint32)
        arr = content.ctypes.data_as(C.POINTER(C.c_uint32))
        lo = 0 if lo is None else lo
        hi = len(content) if hi is None else hi
        pat = pattern.encode("latin-1")
        n = C.c_size_t()
        st = MatchStats()
        _check(lib().fr_match_starts_packed(self.h, arr, len(content), pat, lo, hi, int(compact), None, 0, C.byref(n),
                                            None))
        buf = C.create_string_buffer(n.value)
        _check(lib().fr_match_starts_packed(self.h, arr, len(content), pat, lo, hi, int(compact), buf, n.value,
                                            C.byref(n), C.byref(st)))
        blob = buf.raw[:n.value]
        return (blob, st) if stats else blob

    def has_match_batch(self, contents: Sequence[Sequence[int]], pattern: str):
        """M independent matches of one pattern over M equal-length contents in
        shared launches (fr_has_match_batch): ([out handle per match], stats)."""
        M = len(contents)
        n = len(contents[0]) if M else 0
        if any(len(c) != n for c in contents):
            raise ValueError("has_match_batch: contents must have one length")
        flat = [h for c in contents for h in c]
        arr = (C.c_uint32 * max(len(flat), 1))(*flat)
        out = (C.c_uint32 * max(M, 1))()
        st = MatchStats()
        _check(lib().fr_has_match_batch(self.h, arr, n, M, pattern.encode("latin-1"), out, C.byref(st)))
        return list(out)[:M], st

    def export_bool_device(self, hs: Sequence[int], dev_ptr: int):
        arr = (C.c_uint32 * len(hs))(*hs)
        _check(lib().fr_export_bool_device(self.h, arr, len(hs), C.c_void_p(dev_ptr)))

    def export_bool_device_async(self, hs: Sequence[int], dev_ptr: int):
        """stream-ordered export (no synchronisation): order other streams after it with
        an event on stream_ptr()"""
        arr = (C.c_uint32 * len(hs))(*hs)
        _check(lib().fr_export_bool_device_async(self.h, arr, len(hs), C.c_void_p(dev_ptr)))

    def stream_ptr(self) -> int:
        """the context's hipStream_t (for torch.cuda.ExternalStream)"""
        s = C.c_void_p()
        _check(lib().fr_stream(self.h, C.byref(s)))
        return s.value or 0

    def import_bool_device(self, dev_ptr: int, n: int) -> List[int]:
        out = (C.c_uint32 * n)()
        _check(lib().fr_import_bool_device(self.h, C.c_void_p(dev_ptr), n, out))
        return list(out)

    def device_timers(self):
        br, ks = C.c_double(), C.c_double()
        nl, ng = C.c_uint64(), C.c_uint64()
        _check(lib().fr_device_timers(self.h, C.byref(br), C.byref(ks), C.byref(nl), C.byref(ng)))
        lb, ll, lg = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(lib().fr_device_timers_latency(self.h, C.byref(lb), C.byref(ll), C.byref(lg)))
        pb, pl, pg = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(lib().fr_device_timers_pair(self.h, C.byref(pb), C.byref(pl), C.byref(pg)))
        return {"br_ms": br.value, "ks_ms": ks.value, "br_launches": nl.value, "br_gates": ng.value,
                "lat_br_ms": lb.value, "lat_launches": ll.value, "lat_gates": lg.value,
                "pair_br_ms": pb.value, "pair_launches": pl.value, "pair_gates": pg.value}

    # single-stage device entry points
    def dev_keyswitch(self, lwes: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(lwes.reshape(-1, self.lwe_len), dtype=np.uint64)
        out = np.zeros((a.shape[0], self.params.n + 1), dtype=np.uint64)
        _check(lib().fr_dev_keyswitch(self.h, _p(a), a.shape[0], _p(out)))
        return out

    def dev_blind_rotate(self, ks: np.ndarray, luts) -> np.ndarray:
        a = np.ascontiguousarray(ks.reshape(-1, self.params.n + 1), dtype=np.uint64)
        l = np.ascontiguousarray(np.asarray(luts, dtype=np.uint8).reshape(a.shape[0], 16))
        out = np.zeros((a.shape[0], self.lwe_len), dtype=np.uint64)
        _check(lib().fr_dev_blind_rotate(self.h, _p(a), l.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[0], _p(out)))
        return out

    def dev_blind_rotate_multi(self, ks: np.ndarray, luts, direct: bool = False) -> np.ndarray:
        a = np.ascontiguousarray(ks.reshape(self.params.n + 1), dtype=np.uint64)
        l = np.ascontiguousarray(np.asarray(luts, dtype=np.uint8).reshape(-1, 16))
        out = np.zeros((l.shape[0], self.lwe_len), dtype=np.uint64)
        _check(lib().fr_dev_blind_rotate_multi(self.h, _p(a), l.ctypes.data_as(C.POINTER(C.c_uint8)), l.shape[0],
                                               int(direct), _p(out)))
        return out

    def dev_ring_mul(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a.reshape(-1, self.params.N), dtype=np.uint64)
        b = np.ascontiguousarray(b.reshape(-1, self.params.N), dtype=np.uint64)
        out = np.zeros_like(a)
        _check(lib().fr_dev_ring_mul(self.h, _p(a), _p(b), a.shape[0], _p(out)))
        return out

    def dev_bench_pbs(self, handles: Sequence[int], iters: int):
        arr = (C.c_uint32 * len(handles))(*handles)
        br, tot = C.c_double(), C.c_double()
        _check(lib().fr_dev_bench_pbs(self.h, arr, len(handles), iters, C.byref(br), C.byref(tot)))
        return br.value, tot.value


class Needle:
    """An uploaded needle (fr_upload_needle): close() releases its device memory, after every
    lane's queued finds."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    def __len__(self) -> int:
        m = C.c_size_t()
        _check(lib().fr_needle_len(self.h, C.byref(m)))
        return m.value

    @property
    def form(self) -> int:
        """fr_needle_form: NEEDLE_NIBBLES or NEEDLE_BYTES"""
        f = C.c_int32()
        _check(lib().fr_needle_form(self.h, C.byref(f)))
        return f.value

    def close(self):
        if self.h is not None and self.ctx.h:
            _check(lib().fr_needle_free(self.ctx.h, self.h))
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def needle_masks(s: bytes | str, ignore_case: bool = False, any_char: Optional[str] = None) -> List[Tuple[int, int]]:
    """(lo_mask, hi_mask) per character of a needle: bit v of a mask accepts nibble value v.  A
    literal byte is one bit in each; ignore_case gives an ASCII letter both cases (high nibble 4
    or 6, 5 or 7); a character equal to any_char matches any byte."""
    b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    wild = None if any_char is None else (any_char.encode("latin-1") if isinstance(any_char, str) else bytes(any_char))
    if wild is not None and len(wild) != 1:
        raise ValueError("any_char is one character")
    out = []
    for c in b:
        if wild is not None and c == wild[0]:
            out.append((0xFFFF, 0xFFFF))
            continue
        lo, hi = 1 << (c & 15), 1 << (c >> 4)
        if ignore_case and (0x41 <= (c & ~0x20) <= 0x5A):
            hi = (1 << ((c >> 4) & ~2)) | (1 << ((c >> 4) | 2))
        out.append((lo, hi))
    return out


NEEDLE_NIBBLES, NEEDLE_BYTES = 0, 1  # Needle.form
NEEDLE_MAX_CHARS = 64
_ALL_BYTES = (1 << 256) - 1
_SHORTHAND = {
    "d": sum(1 << b for b in range(0x30, 0x3A)),
    "w": sum(1 << b for b in list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F]),
    "s": sum(1 << b for b in b" \t\n\r\f\v"),
}
_CONTROL = {"t": 9, "n": 10, "r": 13, "f": 12, "v": 11, "0": 0}


def _fold_case(t: int) -> int:
    """a byte set with the other case of every ASCII letter it holds"""
    for b in range(0x41, 0x5B):
        if (t >> b | t >> (b | 0x20)) & 1:
            t |= (1 << b) | (1 << (b | 0x20))
    return t


def needle_tables(pattern: bytes | str, ignore_case: bool = False) -> List[int]:
    """One 256-bit set per position of a fixed-length pattern (bit b accepts byte b), for a
    byte-table needle.  One character is consumed per item: a literal; `.`, any byte; `[...]` with
    ranges and a leading `^` (a `]` placed first and a `-` placed first or last are literals);
    \\d \\w \\s \\D \\W \\S (ASCII); \\xHH; \\t \\n \\r \\f \\v \\0; an escaped punctuation character.
    ignore_case gives every ASCII letter of a set both cases, before a class is negated.  Whatever
    makes the length variable or the form cannot hold raises ValueError naming the character:
    * + ? | ( ) { }, the anchors ^ and $, an empty or unterminated class, a character past 0xFF,
    and a pattern of 0 or more than 64 items."""
    if isinstance(pattern, str):
        for ch in pattern:
            if ord(ch) > 255:
                raise ValueError(f"needle pattern: character {ch!r} is not one byte")
        s = pattern
    else:
        s = bytes(pattern).decode("latin-1")
    fold = _fold_case if ignore_case else (lambda t: t)

    def escape(i: int, in_class: bool) -> Tuple[int, int, bool]:
        """the set of the escape whose backslash is at s[i]: (set, next index, is one literal byte)"""
        if i + 1 >= len(s):
            raise ValueError("needle pattern: '\\\\' at the end of the pattern")
        c = s[i + 1]
        if c.lower() in _SHORTHAND:
            t = fold(_SHORTHAND[c.lower()])
            return (t if c.islower() else _ALL_BYTES & ~t), i + 2, False
        if c == "x":
            hx = s[i + 2:i + 4]
            if len(hx) != 2 or any(h not in "0123456789abcdefABCDEF" for h in hx):
                raise ValueError(f"needle pattern: '\\\\x' at {i} is not followed by two hex digits")
            return 1 << int(hx, 16), i + 4, True
        if c in _CONTROL:
            return 1 << _CONTROL[c], i + 2, True
        if c.isalnum():
            raise ValueError(f"needle pattern: escape '\\\\{c}' is not supported")
        return 1 << ord(c), i + 2, True

    out: List[int] = []
    i = 0
    while i < len(s):
        c = s[i]
        if c in "*+?|(){}":
            raise ValueError(f"needle pattern: {c!r} at {i} would make the length variable; a needle is fixed-length")
        if c in "^$":
            raise ValueError(f"needle pattern: anchor {c!r} at {i}; a needle matches at every start")
        if c == ".":
            out.append(_ALL_BYTES)
            i += 1
        elif c == "\\":
            t, i, lit = escape(i, False)
            out.append(fold(t) if lit else t)
        elif c == "[":
            j = i + 1
            neg = j < len(s) and s[j] == "^"
            j += neg
            t, first = 0, True
            while True:
                if j >= len(s):
                    raise ValueError(f"needle pattern: class '[' at {i} is not closed")
                if s[j] == "]" and not first:
                    break
                first = False
                if s[j] == "\\":
                    lo_set, j, lit = escape(j, True)
                else:
                    lo_set, j, lit = 1 << ord(s[j]), j + 1, True
                # a range: a literal, '-', and a literal that is not the closing bracket
                if lit and j + 1 < len(s) and s[j] == "-" and s[j + 1] != "]":
                    if s[j + 1] == "\\":
                        hi_set, j2, hi_lit = escape(j + 1, True)
                    else:
                        hi_set, j2, hi_lit = 1 << ord(s[j + 1]), j + 2, True
                    if not hi_lit:
                        raise ValueError(f"needle pattern: range at {j} ends in a class escape")
                    lo, hi = lo_set.bit_length() - 1, hi_set.bit_length() - 1
                    if hi < lo:
                        raise ValueError(f"needle pattern: range {chr(lo)!r}-{chr(hi)!r} at {j} is reversed")
                    lo_set, j = sum(1 << b for b in range(lo, hi + 1)), j2
                t |= lo_set
            t = fold(t)
            t = _ALL_BYTES & ~t if neg else t
            if not t:
                raise ValueError(f"needle pattern: class '[' at {i} is empty")
            out.append(t)
            i = j + 1
        elif c == "]":
            raise ValueError(f"needle pattern: ']' at {i} closes no class")
        else:
            out.append(fold(1 << ord(c)))
            i += 1
        if len(out) > NEEDLE_MAX_CHARS:
            raise ValueError(f"needle pattern: more than {NEEDLE_MAX_CHARS} items at {c!r}")
    if not out:
        raise ValueError("needle pattern: no item at all")
    return out


def _tables_bytes(tables: Sequence[int]) -> bytes:
    """32 bytes per 256-bit set: bit b of table i at byte 32 i + b // 8, bit b % 8"""
    for t in tables:
        if not 0 <= int(t) <= _ALL_BYTES:
            raise ValueError("a byte table is a set of the 256 byte values")
    return b"".join(int(t).to_bytes(32, "little") for t in tables)


def _text_bytes(text: bytes | str) -> bytes:
    """clear content as bytes: a str is its latin-1 bytes (one byte per character)"""
    return text.encode("latin-1") if isinstance(text, str) else bytes(text)


def _plain_needle(fn, content, masks, start_lo, start_hi) -> Tuple[List[int], int]:
    """one of the three plaintext needle evaluators (fn) over the starts of [start_lo, start_hi)
    (default: to the content's end): (starts, any)"""
    b = _text_bytes(content)
    hi = len(b) if start_hi is None else start_hi
    flat = [v for lo_hi in masks for v in lo_hi]
    arr = (C.c_uint16 * max(len(flat), 1))(*flat)
    out = (C.c_uint8 * max(hi - start_lo, 1))()
    any_ = C.c_int32()
    _check(fn(b, len(b), arr, len(masks), start_lo, hi, out, C.byref(any_)))
    return list(out)[:max(hi - start_lo, 0)], any_.value


def plain_find_clear(content: bytes | str, masks: Sequence[Tuple[int, int]], start_lo: int = 0,
                     start_hi: Optional[int] = None) -> Tuple[List[int], int]:
    """fr_plain_find_clear: the lowered programs of find_clear_starts and find_clear in
    plaintext, extract-sums included: (starts, any)"""
    return _plain_needle(lib().fr_plain_find_clear, content, masks, start_lo, start_hi)


def plain_scan_clear(content: bytes | str, masks: Sequence[Tuple[int, int]], start_lo: int = 0,
                     start_hi: Optional[int] = None) -> Tuple[List[int], int]:
    """fr_plain_scan_clear: plain_find_clear by the scan's route (windows classed, the lowered
    programs over the compacted text, every start its class's output): (starts, any)"""
    return _plain_needle(lib().fr_plain_scan_clear, content, masks, start_lo, start_hi)


def _plain_needle_bytes(fn, content, tables, start_lo, start_hi) -> Tuple[List[int], int]:
    b = _text_bytes(content)
    hi = len(b) if start_hi is None else start_hi
    out = (C.c_uint8 * max(hi - start_lo, 1))()
    any_ = C.c_int32()
    _check(fn(b, len(b), _tables_bytes(tables), len(tables), start_lo, hi, out, C.byref(any_)))
    return list(out)[:max(hi - start_lo, 0)], any_.value


def plain_find_clear_bytes(content: bytes | str, tables: Sequence[int], start_lo: int = 0,
                           start_hi: Optional[int] = None) -> Tuple[List[int], int]:
    """fr_plain_find_clear_bytes: plain_find_clear for a byte-table needle (needle_tables)"""
    return _plain_needle_bytes(lib().fr_plain_find_clear_bytes, content, tables, start_lo, start_hi)


def plain_scan_clear_bytes(content: bytes | str, tables: Sequence[int], start_lo: int = 0,
                           start_hi: Optional[int] = None) -> Tuple[List[int], int]:
    """fr_plain_scan_clear_bytes: plain_scan_clear for a byte-table needle (needle_tables)"""
    return _plain_needle_bytes(lib().fr_plain_scan_clear_bytes, content, tables, start_lo, start_hi)


def window_classes(text: bytes | str, m: int, start_lo: int = 0, start_hi: Optional[int] = None
                   ) -> Tuple[List[int], int, int, bytes]:
    """fr_window_classes: (cls, D, padded D, the D distinct windows side by side) for the starts
    of [start_lo, min(start_hi, len(text))); cls[p - start_lo] = -1 where the window does not fit"""
    b = _text_bytes(text)
    hi = len(b) if start_hi is None else start_hi
    n_cls, d, dp = C.c_size_t(), C.c_uint64(), C.c_uint64()
    _check(lib().fr_window_classes(b, len(b), m, start_lo, hi, None, 0, C.byref(n_cls), C.byref(d), C.byref(dp),
                                   None, 0))
    cls = (C.c_int32 * max(n_cls.value, 1))()
    win = C.create_string_buffer(max(d.value * m, 1))
    _check(lib().fr_window_classes(b, len(b), m, start_lo, hi, cls, n_cls.value, C.byref(n_cls), C.byref(d),
                                   C.byref(dp), win, d.value * m))
    return list(cls)[:n_cls.value], d.value, dp.value, win.raw[:d.value * m]


def plain_find(content: bytes | str, masks: Sequence[Tuple[int, int]], start_lo: int = 0,
               start_hi: Optional[int] = None) -> Tuple[List[int], int]:
    """fr_plain_find: the lowered programs of find_starts and find in plaintext: (starts, any)"""
    return _plain_needle(lib().fr_plain_find, content, masks, start_lo, start_hi)


# ------------------------------------------------------------- reference API
# first word of a compact match_starts reply; never a chunk count of the full form's framing
COMPACT_REPLY = 0xFFFFFFFF


def _starts_reply(chunks: int, blobs: bytes, compact: bool) -> bytes:
    """the frame of a starts reply around its chunks' blobs, back to back: a u32 count of chunks
    (FRPKRES1 blobs), or u32 COMPACT_REPLY and the u32 count (FRCPRES1 blobs)"""
    head = struct.pack("<II", COMPACT_REPLY, chunks) if compact else struct.pack("<I", chunks)
    return head + blobs


@dataclass
class ClientKey:
    ctx: Context

    def encrypt_str(self, s: str, seed=None) -> List[int]:
        """encrypt_str (ciphertext.rs:32-40) + upload: one radix handle per char.  By
        default the masks and noise come from the OS CSPRNG, fresh per call, as in the
        reference; an int seed or a 32-byte key makes the call reproducible (tests)."""
        if any(ord(ch) > 127 for ch in s):
            raise ValueError("content contains non-ascii characters")
        return self.ctx.upload_radix(self.ctx.encrypt_str(s, seed))

    def encrypt_str_compact(self, s: str, seed=None) -> bytes:
        """encrypt_str as the compact wire blob (64 + 32 len(s) bytes) that
        ServerKey.upload_str expands on the server's GPU; `seed` as in encrypt_str"""
        if any(ord(ch) > 127 for ch in s):
            raise ValueError("content contains non-ascii characters")
        return self.ctx.encrypt_str_compact(s, seed)

    def encrypt_needle(self, s: str, ignore_case: bool = False, any_char: Optional[str] = None, seed=None) -> bytes:
        """the private-search query for s as a needle blob (64 + 16 len(s) N bytes) that
        ServerKey.upload_needle takes: the server learns len(s) and nothing else.  ignore_case
        and any_char as in needle_masks; `seed` as in encrypt_str"""
        return self.ctx.encrypt_needle(needle_masks(s, ignore_case, any_char), seed)

    def encrypt_needle_classes(self, pattern: bytes | str, ignore_case: bool = False, seed=None) -> bytes:
        """the private-search query for a fixed-length pattern of byte classes (needle_tables:
        literals, `.`, `[...]`, \\d \\w \\s, \\xHH) as a byte-table needle blob, for searches over the
        server's clear text (ServerKey.find_clear*, scan_clear*): the server learns the number of
        positions and nothing else.  `seed` as in encrypt_str"""
        return self.ctx.encrypt_needle_bytes(needle_tables(pattern, ignore_case), seed)

    def decrypt(self, ct: int) -> int:
        return self.ctx.decrypt_radix(self.ctx.download_radix(ct))

    def decrypt_packed(self, blob: bytes) -> List[int]:
        """the bits of a ServerKey.pack_bools reply"""
        return self.ctx.decrypt_packed(blob)

    def decrypt_starts(self, reply: bytes) -> List[int]:
        """the offsets at which the pattern matches, from a ServerKey.match_starts reply"""
        if len(reply) < 4:
            raise ValueError("not a match_starts reply")
        (chunks,) = struct.unpack_from("<I", reply, 0)
        if chunks == COMPACT_REPLY:
            return self._decrypt_starts_compact(reply)
        if chunks == 0 and len(reply) == 4:
            return []  # an empty content has no start
        size = (len(reply) - 4) // chunks if chunks else 0
        if chunks == 0 or 4 + chunks * size != len(reply):
            raise ValueError("not a match_starts reply")
        offs, base = [], 0
        for c in range(chunks):
            bits = self.ctx.decrypt_packed(reply[4 + c * size:4 + (c + 1) * size])
            offs += [base + j for j, b in enumerate(bits) if b]
            base += len(bits)
        return offs

    def _decrypt_starts_compact(self, reply: bytes) -> List[int]:
        """the compact reply: u32 0xFFFFFFFF, u32 chunks, then the chunks' FRCPRES1 blobs, each
        delimited by its own header (32 + 2 (kN + n) bytes, n at byte 16)"""
        if len(reply) < 8:
            raise ValueError("not a match_starts reply")
        (chunks,) = struct.unpack_from("<I", reply, 4)
        kN = self.ctx.params.k * self.ctx.params.N
        offs, base, at = [], 0, 8
        for _ in range(chunks):
            if at + 32 > len(reply):
                raise ValueError("not a match_starts reply: a chunk's header overruns the reply")
            (n,) = struct.unpack_from("<Q", reply, at + 16)
            size = 32 + 2 * (kN + n)
            if n > self.ctx.params.N or at + size > len(reply):
                raise ValueError("not a match_starts reply: a chunk overruns the reply")
            bits = self.ctx.decrypt_packed_compact(reply[at:at + size])
            offs += [base + j for j, b in enumerate(bits) if b]
            base += len(bits)
            at += size
        if at != len(reply):
            raise ValueError("not a match_starts reply: bytes after the last chunk")
        return offs

    def serialize(self) -> bytes:
        """bincode::serialize of the RadixClientKey (engine.rs:238-246)."""
        return self.ctx.serialize_client_key()


@dataclass
class ServerKey:
    ctx: Context

    def create_trivial_radix(self, msg: int) -> int:
        return self.ctx.trivial(msg)

    def upload_str(self, blob: bytes) -> List[int]:
        """content handles of a client's compact blob (ClientKey.encrypt_str_compact): the
        masks are rebuilt on the GPU, only the bodies cross the bus; no client key needed"""
        return self.ctx.upload_compact_str(blob)

    def pack_bools(self, handles: Sequence[int]) -> bytes:
        """up to N boolean handles as one 32 KB reply under the client's key (needs the
        packing key: gen_keys(packing=True) or load(..., packing_path))"""
        return self.ctx.pack_bools(handles)

    def match_starts(self, content: Sequence[int], pattern: str, compact: bool = False) -> bytes:
        """where the pattern matches in the content, as one reply for ClientKey.decrypt_starts:
        a u32 count of chunks, then one packed result blob per chunk of N start offsets (a
        content of up to N characters: one 32 KB blob).  The handles are released.
        compact=True: u32 0xFFFFFFFF (no chunk count of the form above), a u32 count of chunks,
        then one compact blob of 32 + 2 (kN + n) bytes per chunk of n <= N starts, each from one
        fr_match_starts_packed call: no handles, 4,640 bytes for 256 characters at (1, 2048)."""
        N = self.ctx.params.N
        if compact:
            blobs = [self.ctx.match_starts_packed(content, pattern, lo, min(lo + N, len(content)))
                     for lo in range(0, len(content), N)]
        else:
            blobs = self._packed_chunks(self.ctx.match_starts(content, pattern), False)
        return _starts_reply(len(blobs), b"".join(blobs), compact)

    def _packed_chunks(self, hs: Sequence[int], compact: bool) -> List[bytes]:
        """one blob per chunk of N of the boolean handles hs (compact: FRCPRES1, else FRPKRES1);
        the handles are released, whether the packs succeed or not"""
        N = self.ctx.params.N
        pack = self.ctx.pack_bools_compact if compact else self.ctx.pack_bools
        try:
            return [pack(hs[i:i + N]) for i in range(0, len(hs), N)]
        finally:
            for h in hs:
                self.ctx.release(h)

    def upload_needle(self, blob: bytes) -> Needle:
        """a client's needle blob (ClientKey.encrypt_needle) on the device; no client key needed"""
        return self.ctx.upload_needle(blob)

    def find(self, content: Sequence[int], needle: Needle) -> int:
        """boolean handle: the encrypted needle occurs in the encrypted content"""
        return self.ctx.find(content, needle)[0]

    def find_starts(self, content: Sequence[int], needle: Needle, compact: bool = False) -> bytes:
        """where the needle occurs, as match_starts' reply for ClientKey.decrypt_starts (both
        forms): fr_find_starts, then one pack per chunk of N starts.  The handles are released."""
        blobs = self._packed_chunks(self.ctx.find_starts(content, needle), compact)
        return _starts_reply(len(blobs), b"".join(blobs), compact)

    def find_clear(self, text: bytes | str, needle: Needle) -> int:
        """boolean handle: the encrypted needle occurs in the server's own clear text"""
        return self.ctx.find_clear(text, needle)[0]

    def find_clear_starts(self, text: bytes | str, needle: Needle, compact: bool = False) -> bytes:
        """where the needle occurs in the clear text, as find_starts' reply for
        ClientKey.decrypt_starts (both forms): fr_find_clear_starts, then one pack per chunk of N
        starts.  The handles are released."""
        blobs = self._packed_chunks(self.ctx.find_clear_starts(text, needle), compact)
        return _starts_reply(len(blobs), b"".join(blobs), compact)

    def scan_clear(self, text: bytes | str, needle: Needle) -> int:
        """find_clear for a long text: one rotation per distinct window of len(needle) bytes
        instead of one per start (fr_scan_clear)"""
        return self.ctx.scan_clear(text, needle)[0]

    def scan_clear_starts(self, text: bytes | str, needle: Needle, compact: bool = False) -> bytes:
        """find_clear_starts' reply, byte for byte, from one fr_scan_clear_starts call: no handle
        per start, one rotation per distinct window, one mapped pack per chunk of N starts"""
        N = self.ctx.params.N
        chunks = (len(_text_bytes(text)) + N - 1) // N
        return _starts_reply(chunks, self.ctx.scan_clear_starts(text, needle, compact=compact), compact)

    def save(self, path: str, packing_path: Optional[str] = None):
        """the server key as an .npz of its (ksk, bsk) arrays (fr_export_server_key's layout);
        packing_path: the packing key's raw blob as a second file"""
        ksk, bsk = self.ctx.export_server_key()
        np.savez(path, ksk=ksk, bsk=bsk)
        if packing_path is not None:
            self.ctx.export_packing_key().tofile(packing_path)

    @staticmethod
    def load(path: str, device: int = 0, params: Optional[Params] = None,
             packing_path: Optional[str] = None) -> "ServerKey":
        """a server context holding only this server key (fr_load_server_key; no client key),
        and the packing key of packing_path if given"""
        ctx = Context(device, params)
        with np.load(path, allow_pickle=False) as z:
            ctx.load_server_key(z["ksk"], z["bsk"])
        if packing_path is not None:
            ctx.load_packing_key(np.fromfile(packing_path, dtype=np.uint8))
        return ServerKey(ctx)

    def save_compact(self, path: str, packing_path: Optional[str] = None):
        """the raw compact blob (fr_export_server_key_compact) of a compact-form key;
        packing_path: the compact blob of a compact-form packing key as a second file"""
        with open(path, "wb") as f:
            f.write(self.ctx.export_server_key_compact())
        if packing_path is not None:
            self.ctx.export_packing_key_compact().tofile(packing_path)

    @staticmethod
    def load_compact(path: str, device: int = 0, params: Optional[Params] = None,
                     packing_path: Optional[str] = None) -> "ServerKey":
        """a server context holding only the server key of a compact blob, and the packing
        key of the compact blob at packing_path if given"""
        ctx = Context(device, params)
        with open(path, "rb") as f:
            ctx.load_server_key_compact(f.read())
        if packing_path is not None:
            ctx.load_packing_key_compact(np.fromfile(packing_path, dtype=np.uint8))
        return ServerKey(ctx)


COMPACT_MAGIC = b"FRCSKEY1"
COMPACT_CONTENT_MAGIC = b"FRCCTXT1"
COMPACT_PACKING_MAGIC = b"FRCPKEY1"
# magic -> (the blob's name, the mask key's offset, the header's size) (include/fheregex.h)
_MASK_KEY_AT = {COMPACT_MAGIC: ("server key", 40, 72), COMPACT_CONTENT_MAGIC: ("content", 32, 64),
                COMPACT_PACKING_MAGIC: ("packing key", 56, 96)}


def _mask_key(blob, magic: bytes) -> bytes:
    what, at, header = _MASK_KEY_AT[magic]
    if len(blob) < header or bytes(blob[:8]) != magic:
        raise ValueError(f"not a compact {what} blob")
    return bytes(blob[at:at + 32])


def compact_mask_key(blob: bytes) -> bytes:
    """the public 32-byte mask key of a compact server-key blob (bytes 40..71)"""
    return _mask_key(blob, COMPACT_MAGIC)


def compact_content_mask_key(blob: bytes) -> bytes:
    """the public 32-byte mask key of a compact content blob (bytes 32..63)"""
    return _mask_key(blob, COMPACT_CONTENT_MAGIC)


def compact_packing_mask_key(blob) -> bytes:
    """the public 32-byte mask key of a compact packing-key blob (bytes 56..87)"""
    return _mask_key(blob, COMPACT_PACKING_MAGIC)


def gen_keys(client_key_blob: Optional[bytes] = None, seed=None, device: int = 0,
             params: Optional[Params] = None, client_seed=None, compact: bool = False, packing: bool = False,
             packing_seed=None, packing_compact: bool = False):
    """gen_keys (ciphertext.rs:42-45): (client key, server key).

    Without a blob the client key is fresh (gen_keys_radix(&PARAM_MESSAGE_2_CARRY_2, 4),
    ciphertext.rs:44), drawn under `client_seed`; with a blob it is that bincode key
    (read_test_keys, engine.rs:248-254).  The server key's masks and noise
    (ServerKey::new, engine.rs:252) are drawn under `seed`.  Both default to None: 256
    bits of the OS CSPRNG each, as the reference draws.  32 bytes are a generator key, an
    int a 64-bit seed; a server key from an int seed is reproducible (tests, benchmarks,
    multi-rank keygen) and must not leave the client.  compact=True: the server key in
    compact form (ServerKey.save_compact ships it).  packing=True: also the packing key
    (ServerKey.pack_bools), drawn under `packing_seed`; packing_compact=True: that key in
    its compact form (ServerKey.save_compact(path, packing_path) ships it)."""
    ctx = Context(device, params)
    if client_key_blob is None:
        ctx.gen_client_key(client_seed)
    else:
        ctx.load_client_key(client_key_blob)
    ctx.gen_server_key(seed, compact=compact)
    if packing:
        ctx.gen_packing_key(packing_seed, compact=packing_compact)
    return ClientKey(ctx), ServerKey(ctx)


def has_match(sk: ServerKey, content: Sequence[int], pattern: str) -> int:
    """engine.rs:8-42: returns the encrypted 0/1 result handle."""
    out, _ = sk.ctx.has_match(content, pattern)
    return out


def shard_starts(L: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous range [lo, hi) of start offsets owned by `rank`.

    The reference's driver ORs one branch set per start offset
    (engine.rs:22-35); offsets are independent, so ranks split them into
    contiguous ranges, evaluate their OR tree locally (fr_has_match_range) and
    a final OR over the gathered per-rank booleans gives the full result."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    base, extra = divmod(L, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


# ------------------------------------------------------- one match across ranks
def job_slice(J: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous slice [a, b) of a level's J rotation jobs owned by `rank`
    (ceil(r J / world) boundaries: balanced, and rank 0 owns a lone job)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    return -(-rank * J // world), -(-(rank + 1) * J // world)


def run_sharded(ex, world: int, rank: int, all_gather, times=None):
    """Level-sharded evaluation of one match plan (fheregex.h fr_shard_*):
    every level but the last is split into contiguous job slices, each rank runs
    its slice, and the slices' output LWEs are all-gathered so that every rank
    holds the level; rank 0 runs the last level.  `ex` is an executor (ShardPlan
    on the GPU, or a CPU evaluator in tests) with levels / jobs(l) /
    outputs(l, a, b) / run(l, a, b) / export(l, a, b, cap) -> buffer /
    import_(l, a, b, buffer); all_gather(buffer) returns every rank's buffer in
    rank order.  `times` (a dict) accumulates wall milliseconds per phase: slices
    (runs + exports, which wait for the device), gather, import, top.  Returns the
    number of gathered LWEs."""
    import time
    clock = time.perf_counter

    def tick(phase, t0):
        if times is not None:
            times[phase] = times.get(phase, 0.0) + (clock() - t0) * 1e3
        return clock()

    gathered = 0
    nl = ex.levels
    t = clock()
    for l in range(nl - 1):
        parts = [job_slice(ex.jobs(l), world, r) for r in range(world)]
        counts = [ex.outputs(l, a, b) for a, b in parts]
        a, b = parts[rank]
        if b > a:
            ex.run(l, a, b)
        send = ex.export(l, a, b, max(counts))
        t = tick("slices_ms", t)
        bufs = all_gather(send)
        t = tick("gather_ms", t)
        for r, (ar, br) in enumerate(parts):
            if r != rank and counts[r]:
                ex.import_(l, ar, br, bufs[r])
        t = tick("import_ms", t)
        gathered += sum(counts)
    if rank == 0 and nl:
        ex.run(nl - 1, 0, ex.jobs(nl - 1))
    tick("top_ms", t)
    return gathered


def _runs(idx) -> List[Tuple[int, int]]:
    """maximal contiguous [a, b) runs of a sorted index list"""
    out = []
    for i in idx:
        if out and out[-1][1] == i:
            out[-1] = (out[-1][0], i + 1)
        else:
            out.append((i, i + 1))
    return out


def closure_parts(S: "Schedule", world: int):
    """Dependency-closure sharding of one match schedule (fr_schedule_match).

    The top of the circuit (the last level, widened downwards while it is fed by
    too few jobs to split evenly over `world` ranks) runs on rank 0; the jobs that feed it (the frontier)
    are cut into `world` contiguous parts, and rank r runs the transitive closure
    of its part (every job its part depends on, level by level; a job two parts
    need runs on both ranks).  Only the frontier outputs travel, once, to rank 0.
    The regex circuit is local in the content (a start's branch reads the
    characters after it, engine.rs:45-214), so a contiguous part's closure is a
    contiguous window of each level and the duplicated work is the few jobs at
    the window edges.

    Returns (runs, frontier, top): runs[r][l] = [(a, b), ...] job runs of level l
    that rank r executes before the gather; frontier[r] = [(l, a, b), ...] the
    runs of rank r's frontier part, in gather order; top[l] = the runs rank 0
    executes after the gather."""
    nl = len(S.level_off) - 1
    level = []
    for l in range(nl):
        level += [l] * (S.level_off[l + 1] - S.level_off[l])
    prod = {}
    for gi, j in enumerate(S.jobs):
        for f in range(j.n_out):
            prod[j.out_gate[f]] = gi

    def producers(js):
        return {prod[S.jobs[gi].in_ref[q]] for gi in js for q in range(S.jobs[gi].n_in) if S.jobs[gi].in_ref[q] >= 0}

    def by_level(js):
        per = [[] for _ in range(nl)]
        for gi in sorted(js):
            per[level[gi]].append(gi - S.level_off[level[gi]])
        return per

    top = set(range(S.level_off[nl - 1], S.level_off[nl])) if nl else set()
    front = producers(top) - top
    # widen while some rank would get no part, or the parts are uneven and few
    while 0 < len(front) and (len(front) < world or (len(front) % world and len(front) < 4 * world)):
        wider = producers(top | front) - top - front
        if len(wider) <= len(front):
            break
        top |= front
        front = wider
    front = sorted(front)
    runs, frontier = [], []
    for r in range(world):
        a, b = job_slice(len(front), world, r)
        part = front[a:b]
        need, stack = set(), list(part)
        while stack:
            gi = stack.pop()
            if gi in need:
                continue
            need.add(gi)
            stack += list(producers([gi]))
        runs.append([_runs(x) for x in by_level(need)])
        frontier.append([(l, x, y) for l, xs in enumerate(by_level(part)) for x, y in _runs(xs)])
    return runs, frontier, [_runs(x) for x in by_level(top)]


def run_closure_sharded(ex, S: "Schedule", world: int, rank: int, all_gather, parts=None, times=None):
    """One match over `world` ranks by dependency-closure sharding (closure_parts):
    no exchange until the top of the circuit, then one all_gather of the frontier
    LWEs (device to device with torch_all_gather) and rank 0 runs the top.  `ex`
    is a run_sharded executor whose schedule is S; `parts` = closure_parts(S,
    world), computed once by a caller that repeats the match (it costs
    milliseconds of host time).  `times` (a dict) accumulates this rank's wall
    milliseconds per phase: closure (its jobs and the export of its frontier, which
    waits for the device), gather, top (imports and the top's launches; the top's
    device time lands in the caller's finish).  Returns the number of gathered LWEs."""
    import time

    import torch

    clock = time.perf_counter

    def tick(phase, t0):
        if times is not None:
            times[phase] = times.get(phase, 0.0) + (clock() - t0) * 1e3
        return clock()

    t = clock()
    nl = ex.levels
    if nl != len(S.level_off) - 1 or any(ex.jobs(l) != S.level_off[l + 1] - S.level_off[l] for l in range(nl)):
        raise ValueError("executor and schedule disagree")
    runs, frontier, top = parts if parts is not None else closure_parts(S, world)
    for l in range(nl):
        for a, b in runs[rank][l]:
            ex.run(l, a, b)
    sizes = [sum(ex.outputs(l, a, b) for l, a, b in frontier[r]) for r in range(world)]
    if max(sizes, default=0):
        parts = [ex.export(l, a, b, ex.outputs(l, a, b)).reshape(-1)[:ex.outputs(l, a, b) * ex.lwe_len]
                 for l, a, b in frontier[rank]]
        cap = max(sizes) * ex.lwe_len
        have = sum(p.numel() for p in parts)
        if have < cap:
            parts.append(torch.zeros(cap - have, dtype=torch.int64,
                                     device=parts[0].device if parts else ex.buffer_device()))
        send = torch.cat(parts).contiguous()
        t = tick("closure_ms", t)
        bufs = all_gather(send)
        t = tick("gather_ms", t)
        if rank == 0:
            for r in range(1, world):
                off = 0
                for l, a, b in frontier[r]:
                    n = ex.outputs(l, a, b) * ex.lwe_len
                    ex.import_(l, a, b, bufs[r][off:off + n])
                    off += n
    else:
        t = tick("closure_ms", t)
    if rank == 0:
        for l in range(nl):
            for a, b in top[l]:
                ex.run(l, a, b)
    tick("top_ms", t)
    return sum(sizes)


class ShardPlan:
    """fr_shard_* executor for run_sharded: a compiled, device-resident plan of one
    match; buffers are torch CUDA tensors (export / import go device to device)."""

    def __init__(self, ctx: Context, content: Sequence[int], pattern: str, start_lo: int = 0,
                 start_hi: Optional[int] = None):
        self.ctx = ctx
        arr = (C.c_uint32 * len(content))(*content)
        hi = len(content) if start_hi is None else start_hi
        h = C.c_void_p()
        self.stats = MatchStats()
        _check(lib().fr_shard_plan(ctx.h, arr, len(content), pattern.encode("latin-1"), start_lo, hi, C.byref(h),
                                   C.byref(self.stats)))
        self.h = h
        self.lwe_len = ctx.lwe_len
        n = C.c_uint32()
        _check(lib().fr_shard_levels(h, C.byref(n)))
        self.levels = n.value
        self._jobs = []
        for l in range(self.levels):
            _check(lib().fr_shard_jobs(h, l, C.byref(n)))
            self._jobs.append(n.value)

    def jobs(self, level: int) -> int:
        return self._jobs[level]

    def buffer_device(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def outputs(self, level: int, a: int, b: int) -> int:
        n = C.c_uint32()
        _check(lib().fr_shard_outputs(self.h, level, a, b, C.byref(n)))
        return n.value

    def run(self, level: int, a: int, b: int):
        _check(lib().fr_shard_run(self.ctx.h, self.h, level, a, b))

    def export(self, level: int, a: int, b: int, cap: int):
        import torch
        buf = torch.empty(max(cap, 1) * self.ctx.lwe_len, dtype=torch.int64, device=f"cuda:{self.ctx.device}")
        _check(lib().fr_shard_export(self.ctx.h, self.h, level, a, b, C.c_void_p(buf.data_ptr())))
        return buf

    def import_(self, level: int, a: int, b: int, buf):
        _check(lib().fr_shard_import(self.ctx.h, self.h, level, a, b, C.c_void_p(buf.data_ptr())))

    def finish(self) -> Tuple[int, MatchStats]:
        out = C.c_uint32()
        st = MatchStats()
        _check(lib().fr_shard_finish(self.ctx.h, self.h, C.byref(out), C.byref(st)))
        return out.value, st

    def free(self):
        if getattr(self, "h", None):
            _check(lib().fr_shard_free(self.ctx.h, self.h))
            self.h = None


def torch_all_gather(group=None):
    """all_gather for run_sharded over torch.distributed (RCCL on GPU tensors):
    the returned views of one gathered tensor are valid once this returns."""
    import torch
    import torch.distributed as dist

    staged = dist.get_backend(group) == "gloo"  # gloo rehearsal: device buffers go through the host

    def gather(buf):
        world = dist.get_world_size(group)
        src = buf.cpu() if staged and buf.is_cuda else buf
        out = torch.empty(world * src.numel(), dtype=src.dtype, device=src.device)
        dist.all_gather_into_tensor(out, src, group=group)
        if staged and buf.is_cuda:
            out = out.to(buf.device)
        if out.is_cuda:
            torch.cuda.synchronize(out.device)  # the library reads it on its own stream
        return list(out.view(world, -1))
    return gather


@dataclass
class Schedule:
    """fr_schedule_match: rotation jobs by level, without a device."""
    jobs: list
    level_off: List[int]
    out_gate: int
    out_w: int
    out_const: int
    n_gates: int
    parts: List[Tuple[int, int, int]] = None  # (out_gate, out_w, out_const) of each part


def schedule_match(n_chars: int, pattern: str, start_lo: int = 0, start_hi: Optional[int] = None,
                   lowering: int = LOWER_THRESHOLD, engine: int = ENGINE_AUTO, grammar: int = GRAMMAR_REFERENCE,
                   multi_value: bool = True, max_parts: int = 1) -> Schedule:
    """max_parts > 1: fr_has_match_parts' schedule (Schedule.parts; out_* = part 0)"""
    hi = n_chars if start_hi is None else start_hi
    nj, nl, npart = C.c_size_t(), C.c_size_t(), C.c_size_t()
    outs3 = (C.c_int32 * (3 * max_parts))()
    pat = pattern.encode("latin-1")
    args = (n_chars, pat, start_lo, hi, lowering, engine, grammar, int(multi_value), max_parts)
    _check(lib().fr_schedule_match_parts(*args, None, 0, C.byref(nj), None, 0, C.byref(nl), outs3, C.byref(npart)))
    jobs = (FrJob * max(nj.value, 1))()
    off = (C.c_uint32 * (nl.value + 1))()
    _check(lib().fr_schedule_match_parts(*args, jobs, len(jobs), C.byref(nj), off, len(off), C.byref(nl), outs3,
                                         C.byref(npart)))
    n_gates = 1 + max([max(j.out_gate[f] for f in range(j.n_out)) for j in jobs[:nj.value]] or [-1])
    parts = [(outs3[3 * j], outs3[3 * j + 1], outs3[3 * j + 2]) for j in range(npart.value)]
    return Schedule(list(jobs[:nj.value]), list(off), parts[0][0], parts[0][1], parts[0][2], n_gates, parts)


def schedule_match_starts(n_chars: int, pattern: str, start_lo: int = 0, start_hi: Optional[int] = None,
                          lowering: int = LOWER_THRESHOLD, engine: int = ENGINE_AUTO,
                          grammar: int = GRAMMAR_REFERENCE, multi_value: bool = True) -> Schedule:
    """fr_match_starts' schedule: Schedule.parts holds (out_gate, out_w, out_const) per start"""
    hi = n_chars if start_hi is None else start_hi
    nj, nl, ns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    cap = max(hi - start_lo, 1)
    outs3 = (C.c_int32 * (3 * cap))()
    args = (n_chars, pattern.encode("latin-1"), start_lo, hi, lowering, engine, grammar, int(multi_value))
    _check(lib().fr_schedule_match_starts(*args, None, 0, C.byref(nj), None, 0, C.byref(nl), outs3, cap, C.byref(ns)))
    jobs = (FrJob * max(nj.value, 1))()
    off = (C.c_uint32 * (nl.value + 1))()
    _check(lib().fr_schedule_match_starts(*args, jobs, len(jobs), C.byref(nj), off, len(off), C.byref(nl), outs3, cap,
                                          C.byref(ns)))
    n_gates = 1 + max([max(j.out_gate[f] for f in range(j.n_out)) for j in jobs[:nj.value]] or [-1])
    parts = [(outs3[3 * j], outs3[3 * j + 1], outs3[3 * j + 2]) for j in range(ns.value)]
    first = parts[0] if parts else (-1, 0, 0)
    return Schedule(list(jobs[:nj.value]), list(off), first[0], first[1], first[2], n_gates, parts)


def schedule_find_clear(n_chars: int, m: int, start_lo: int = 0, start_hi: Optional[int] = None,
                        starts: bool = False) -> Schedule:
    """fr_schedule_find_clear: schedule_find for find_clear / find_clear_starts (no selector job;
    the extract-sums are level 0 and are no jobs)"""
    return schedule_find(n_chars, m, start_lo, start_hi, starts, _fn="fr_schedule_find_clear")


def schedule_find_clear_bytes(n_chars: int, m: int, start_lo: int = 0, start_hi: Optional[int] = None,
                              starts: bool = False) -> Schedule:
    """fr_schedule_find_clear_bytes: schedule_find_clear for a byte-table needle (m terms a start)"""
    return schedule_find(n_chars, m, start_lo, start_hi, starts, _fn="fr_schedule_find_clear_bytes")


def schedule_scan_clear_bytes(n_windows: int, m: int, starts: bool = False) -> Schedule:
    """fr_schedule_scan_clear_bytes: schedule_scan_clear for a byte-table needle"""
    return schedule_scan_clear(n_windows, m, starts, _fn="fr_schedule_scan_clear_bytes")


def schedule_scan_clear(n_windows: int, m: int, starts: bool = False, _fn: str = "fr_schedule_scan_clear"
                        ) -> Schedule:
    """fr_schedule_scan_clear: the schedule of scan_clear (one output) or of scan_clear_starts'
    plan (Schedule.parts: one output per window) over n_windows windows of m bytes"""
    nj, nl, ns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    cap = max(n_windows, 1)
    outs3 = (C.c_int32 * (3 * cap))()
    args = (n_windows, m, int(starts))
    fn = getattr(lib(), _fn)
    _check(fn(*args, None, 0, C.byref(nj), None, 0, C.byref(nl), outs3, cap, C.byref(ns)))
    jobs = (FrJob * max(nj.value, 1))()
    off = (C.c_uint32 * (nl.value + 1))()
    _check(fn(*args, jobs, len(jobs), C.byref(nj), off, len(off), C.byref(nl), outs3, cap, C.byref(ns)))
    n_gates = 1 + max([max(j.out_gate[f] for f in range(j.n_out)) for j in jobs[:nj.value]] or [-1])
    parts = [(outs3[3 * j], outs3[3 * j + 1], outs3[3 * j + 2]) for j in range(ns.value)]
    first = parts[0] if parts else (-1, 0, 0)
    return Schedule(list(jobs[:nj.value]), list(off), first[0], first[1], first[2], n_gates, parts)


def schedule_find(n_chars: int, m: int, start_lo: int = 0, start_hi: Optional[int] = None,
                  starts: bool = False, _fn: str = "fr_schedule_find") -> Schedule:
    """fr_schedule_find: the schedule of find (one output) or find_starts (Schedule.parts: one
    (out_gate, out_w, out_const) per start) for a needle of m characters"""
    hi = n_chars if start_hi is None else start_hi
    nj, nl, ns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    cap = max(hi - start_lo, 1)
    outs3 = (C.c_int32 * (3 * cap))()
    args = (n_chars, m, start_lo, hi, int(starts))
    fn = getattr(lib(), _fn)
    _check(fn(*args, None, 0, C.byref(nj), None, 0, C.byref(nl), outs3, cap, C.byref(ns)))
    jobs = (FrJob * max(nj.value, 1))()
    off = (C.c_uint32 * (nl.value + 1))()
    _check(fn(*args, jobs, len(jobs), C.byref(nj), off, len(off), C.byref(nl), outs3, cap, C.byref(ns)))
    n_gates = 1 + max([max(j.out_gate[f] for f in range(j.n_out)) for j in jobs[:nj.value]] or [-1])
    parts = [(outs3[3 * j], outs3[3 * j + 1], outs3[3 * j + 2]) for j in range(ns.value)]
    first = parts[0] if parts else (-1, 0, 0)
    return Schedule(list(jobs[:nj.value]), list(off), first[0], first[1], first[2], n_gates, parts)


def content_window(n_chars: int, pattern: str, start_lo: int, start_hi: int, lowering: int = LOWER_THRESHOLD,
                   engine: int = ENGINE_AUTO, grammar: int = GRAMMAR_REFERENCE) -> Tuple[int, int]:
    """[wlo, whi): the content positions the circuit of starts [start_lo, start_hi)
    reads, from its lowered schedule (a start's branch reads the characters after
    it, engine.rs:45-214): a start-offset shard needs only this window of the
    content.  (lo, lo) when the circuit reads no content."""
    S = schedule_match(n_chars, pattern, start_lo, start_hi, lowering=lowering, engine=engine, grammar=grammar)
    pos = [(-1 - j.in_ref[q]) // 4 for j in S.jobs for q in range(j.n_in) if j.in_ref[q] < 0]
    return (min(pos), max(pos) + 1) if pos else (start_lo, start_lo)


def header_symbols() -> List[str]:
    import re
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(fr_[a-z_]+)\s*\(", txt)) - {"fr_ctx", "FR_GATE_REF"})
