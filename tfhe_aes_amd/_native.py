"""ctypes binding of the C ABI in include/fheaes.h (libfheaes.so).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, creating an
``Engine`` raises.  ``load_library()`` alone (symbol checks) works without a GPU.
"""
from __future__ import annotations

import ctypes
import os
import re
from pathlib import Path

import numpy as np

from . import _build
from .params import CParams, WopbsParameters

HOST, DEVICE = 0, 1
MAC_NONE = 0xFFFFFFFF           # FHEAES_MAC_NONE: "no block" in a src_block table of mac_link
KW_MIN_SEMIBLOCKS, KW_MAX_SEMIBLOCKS, KW_MAX_KEYS = 2, 8, 4096      # FHEAES_KW_*: a wrapped key's payload in 8-byte semiblocks, keys per unwrap call
AES_WINDOW_OFF = 0xFFFFFFFF     # FHEAES_AES_WINDOW_OFF: fheaes_aes_set_window's "one launch per round"
GATE_LWE, GATE_GLWE = 0, 1       # FHEAES_GATE_*: the input form of fheaes_gate_ggsw
K2_PARK_SLOTS = 1024            # FHEAES_K2_PARK_SLOTS: owner words of the paired kernel's shared parking slots, 128 per XCC
AUDIT_MAX_ROWS, AUDIT_RECORDS = 256, 16      # FHEAES_AUDIT_*: sampled rows per audited launch, records of wrong rows kept
WS_BUFFERS = 17                 # FHEAES_WS_BUFFERS: the scratch buffers fheaes_workspace_info lists
WS_CLASSES = ("f64", "words", "tables")                  # FHEAES_WS_F64 / _WORDS / _TABLES
WS_POISON_FILL, WS_POISON_RELEASE = 0, 1                 # FHEAES_WS_POISON_*: the modes of fheaes_workspace_poison
STAGES = ("keyswitch", "blind_rotate", "pfpks", "ggsw_fft", "vertical_packing", "linear")
AUDIT_STAGES = ("keyswitch", "blind_rotate", "pfpks")    # the stages that have an audit (fheaes_audit_stage_set), in the order they run

_u64p = ctypes.POINTER(ctypes.c_uint64)
_dp = ctypes.POINTER(ctypes.c_double)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_ctx = ctypes.c_void_p
_c = ctypes

# name -> (restype, argtypes); every function declared in include/fheaes.h
SIGNATURES = {
    "fheaes_create": (_c.c_int, [_c.POINTER(CParams), _c.c_int, _c.POINTER(_ctx)]),
    "fheaes_destroy": (None, [_ctx]),
    "fheaes_last_error": (_c.c_char_p, [_ctx]),
    "fheaes_key_words": (_c.c_size_t, [_ctx, _c.c_int]),
    "fheaes_upload_keys": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_key_body_words": (_c.c_size_t, [_ctx, _c.c_int]),
    "fheaes_upload_keys_seeded": (_c.c_int, [_ctx, _c.POINTER(_c.c_uint32), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_clone_keys": (_c.c_int, [_ctx, _ctx]),
    "fheaes_clone_info": (_c.c_int, [_ctx, _c.POINTER(_c.c_int), _u64p, _dp]),
    "fheaes_noise_level_seen": (_c.c_int, [_ctx, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32)]),
    "fheaes_set_stream": (_c.c_int, [_ctx, _c.c_void_p]),
    "fheaes_synchronize": (_c.c_int, [_ctx]),
    "fheaes_reserve": (_c.c_int, [_ctx, _c.c_uint64]),
    "fheaes_keyswitch_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_cbs_pbs_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_pfpks_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_forward_fourier_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_vertical_packing_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                                 _c.c_int, _c.c_void_p, _c.c_int]),
    "fheaes_inv_mix_columns_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_wopbs_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_int,
                                      _c.c_void_p, _c.c_int]),
    "fheaes_gen_lut": (_c.c_int, [_c.c_uint32, _u64p, _u64p]),
    "fheaes_sbox": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_int]),
    "fheaes_many_sbox": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_int]),
    "fheaes_aes_key_expansion": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_aes_encrypt": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decryption_round_keys": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decrypt_equivalent": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_key_expansion_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_aes_encrypt_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decryption_round_keys_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decrypt_equivalent_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_add_scalar": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _u64p, _c.c_int]),
    "fheaes_aes_encrypt_public_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_ctr_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _u64p, _c.c_uint64, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_public_plan": (_c.c_int, [_u64p, _c.c_uint64, _c.c_uint32, _u64p]),
    "fheaes_aes_ctr32_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _u64p, _c.c_uint64, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decrypt_public_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _u64p, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_cbc_decrypt_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _u64p, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_xts_decrypt_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint32, _u64p, _c.c_uint64, _c.c_uint64, _c.c_uint64, _u64p, _c.c_uint64,
                                               _c.c_void_p, _c.c_int]),
    "fheaes_aes_xts_decrypt_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint32, _u64p, _c.c_uint64, _c.c_uint64, _c.c_uint64, _u64p, _c.c_uint64,
                                                 _c.c_void_p, _c.c_int]),
    "fheaes_xts_tweaks": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_xts_tweak_row": (_c.c_int, [_c.c_uint32, _c.c_uint32, _u32p, _u32p]),
    "fheaes_aes_xts_plan": (_c.c_int, [_c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint32, _u64p, _u64p, _u64p, _u32p]),
    "fheaes_aes_key_expansion_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decryption_round_keys_batch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_encrypt_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt_equivalent_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_public_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _u64p, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_public_plan_keyed": (_c.c_int, [_u64p, _u32p, _c.c_uint64, _c.c_uint64, _c.c_uint32, _u64p]),
    "fheaes_aes_decrypt_public_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _u64p, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decrypt_public_plan_keyed": (_c.c_int, [_u64p, _u32p, _c.c_uint64, _c.c_uint64, _c.c_uint32, _u64p]),
    "fheaes_packed_words": (_c.c_size_t, [_ctx, _c.c_uint64]),
    "fheaes_pack_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_unpack_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_expand_lwe_seeded": (_c.c_int, [_ctx, _u32p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_packed_words_mod": (_c.c_size_t, [_ctx, _c.c_uint64, _c.c_uint32]),
    "fheaes_packed_mod_switch": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_pack_bits_mod": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_unpack_bits_mod": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_int]),
    "fheaes_round_keys_packed_glwes": (_c.c_uint32, [_c.c_uint32]),
    "fheaes_pack_round_keys": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_unpack_round_keys": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_encrypt_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_decrypt_equivalent_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_public_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _u64p, _u64p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_decrypt_public_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _u32p, _u64p, _u64p, _c.c_uint64, _c.c_void_p,
                                                          _c.c_int]),
    "fheaes_aes_cbc_mac_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _u32p, _u8p, _c.c_void_p, _u8p, _c.c_void_p,
                                            _c.c_void_p, _c.c_int]),
    "fheaes_aes_cbc_mac_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _u32p, _u8p, _c.c_void_p, _u8p,
                                                   _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_aes_ccm_open_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _u32p, _u64p, _u64p, _u64p, _u8p, _u8p, _u32p,
                                             _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_aes_ccm_open_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _u32p, _u64p, _u64p, _u64p, _u8p, _u8p,
                                                    _u32p, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_mac_link": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_uint64, _u32p, _u8p, _u8p, _c.c_int]),
    "fheaes_xts_whiten": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _u32p, _u8p, _c.c_uint64, _c.c_int]),
    "fheaes_aes_mac_plan": (_c.c_int, [_u32p, _u32p, _c.c_uint64, _u64p, _u64p, _c.c_uint64, _u64p, _u64p]),
    "fheaes_cmac_subkey_row": (_c.c_int, [_c.c_uint32, _c.c_uint32, _u32p, _u32p]),
    "fheaes_cmac_double": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_cmac_subkeys_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_cmac_subkeys_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_aes_cmac_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_uint64, _u32p, _u64p, _u8p, _u8p, _u32p, _c.c_void_p,
                                         _c.c_void_p, _c.c_int]),
    "fheaes_aes_cmac_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_uint64, _u32p, _u64p, _u8p, _u8p, _u32p,
                                                _c.c_void_p, _c.c_void_p, _c.c_int]),
    "fheaes_aes_cmac_plan": (_c.c_int, [_u64p, _c.c_uint64, _u64p, _u64p, _u64p]),
    "fheaes_aes_kw_unwrap_keyed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _c.c_uint32, _u8p, _c.c_void_p, _c.c_void_p,
                                              _c.c_int]),
    "fheaes_aes_kw_unwrap_keyed_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _u32p, _c.c_uint32, _u8p, _c.c_void_p,
                                                     _c.c_void_p, _c.c_int]),
    "fheaes_kw_link": (_c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_uint32, _u8p, _c.c_int]),
    "fheaes_aes_kw_plan": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint64, _u64p, _u64p, _u64p]),
    "fheaes_gate_ggsw": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _u64p, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_int]),
    "fheaes_gate_bits": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _u64p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_gate_packed": (_c.c_int, [_ctx, _c.c_void_p, _c.c_uint64, _u64p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "fheaes_gate_plan": (_c.c_int, [_u64p, _c.c_uint64, _c.c_uint32, _u64p, _u32p]),
    "fheaes_profile_enable": (_c.c_int, [_ctx, _c.c_int]),
    "fheaes_profile_reset": (_c.c_int, [_ctx]),
    "fheaes_profile_read": (_c.c_int, [_ctx, _c.c_int, _dp, _u64p, _u64p]),
    "fheaes_get_twiddles": (_c.c_int, [_dp]),
    "fheaes_read_bsk_fourier": (_c.c_int, [_ctx, _c.c_uint32, _dp]),
    "fheaes_k2_launch_plan": (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.POINTER(_c.c_int), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32),
                                       _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32)]),
    "fheaes_k2_launch_plan_forms": (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_uint64),
                                             _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32)]),
    "fheaes_k2_context_plan": (_c.c_int, [_ctx, _c.c_uint64, _c.POINTER(_c.c_int), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32),
                                        _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32), _c.c_char_p, _c.c_size_t]),
    "fheaes_k2_set_parking": (_c.c_int, [_ctx, _c.c_int]),
    "fheaes_k2_set_forms": (_c.c_int, [_ctx, _c.c_int, _c.c_int]),
    "fheaes_aes_window_plan": (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_uint32, _u64p, _u64p, _u64p, _u64p]),
    "fheaes_aes_context_window": (_c.c_int, [_ctx, _c.c_uint64, _c.c_uint32, _u64p]),
    "fheaes_aes_set_window": (_c.c_int, [_ctx, _c.c_uint32]),
    "fheaes_k2_park_debug": (_c.c_int, [_ctx, _c.POINTER(_c.c_uint32), _c.c_int]),
    "fheaes_k2_park_read": (_c.c_int, [_ctx, _u64p, _u64p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32), _c.c_uint64, _u64p]),
    "fheaes_audit_set": (_c.c_int, [_ctx, _c.c_uint32, _c.c_uint64, _c.c_uint64]),
    "fheaes_audit_rows": (_c.c_int, [_c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint32, _u64p]),
    "fheaes_audit_read": (_c.c_int, [_ctx, _u64p, _u64p, _u64p, _u64p, _c.c_uint64, _u64p]),
    "fheaes_audit_debug": (_c.c_int, [_ctx, _c.c_uint64, _c.c_uint32, _c.c_uint64]),
    "fheaes_audit_stage_set": (_c.c_int, [_ctx, _c.c_int, _c.c_uint32, _c.c_uint64, _c.c_uint64]),
    "fheaes_audit_stage_read": (_c.c_int, [_ctx, _c.c_int, _u64p, _u64p, _u64p, _u64p, _c.c_uint64, _u64p]),
    "fheaes_audit_stage_debug": (_c.c_int, [_ctx, _c.c_int, _c.c_uint64, _c.c_uint32, _c.c_uint64]),
    "fheaes_audit_plain_batch": (_c.c_int, [_ctx, _c.c_int, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p]),
    "fheaes_workspace_info": (_c.c_int, [_ctx, _c.c_uint32, _c.c_char_p, _c.c_size_t, _u64p, _c.POINTER(_c.c_int), _u64p, _u64p]),
    "fheaes_workspace_poison": (_c.c_int, [_ctx, _c.c_int, _u64p]),
    "fheaes_alloc_debug": (_c.c_int, [_ctx, _c.c_uint64, _u64p]),
    "fheaes_version": (_c.c_char_p, []),
}

_libs = {}          # resolved path of a library -> its bound CDLL


def header_symbols() -> list[str]:
    """every function name declared in include/fheaes.h"""
    text = (_build.ROOT / "include" / "fheaes.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fheaes_[a-z0-9_]+)\s*\(", text)))


def load_library(build: bool = True, path=None, partial: bool = False):
    """dlopen a library and bind the declared symbols, once per resolved path.  path None: the product's libfheaes.so, built in-tree
    first if needed; a given path is loaded as it is, never built.  partial: bind the symbols the library has and skip the rest (an
    older build in an A/B run); without it a missing symbol is an AttributeError naming it."""
    if path is None:
        path = _build.build_engine() if build else _build.ENGINE_SO
    path = Path(path).resolve()
    if path in _libs:
        return _libs[path]
    try:
        # PyTorch-ROCm ships its own libamdhip64; two HIP runtimes in one process cannot both own the
        # GPU ("No HIP GPUs are available" in whichever comes second).  Loading torch first makes
        # libfheaes.so resolve its libamdhip64.so.7 dependency to the runtime torch already mapped.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not path.exists():
        raise RuntimeError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % path.name)
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        if partial and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)      # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    _libs[path] = lib
    return lib


class FheAesError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("fheaes error %d: %s" % (code, message))
        self.code = code


def _ptr(x):
    """numpy array (host), torch tensor (host or cuda) or int -> (void pointer value, memspace or None)"""
    if x is None:
        return None, None
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"], "array must be C-contiguous"
        return x.ctypes.data, HOST
    if hasattr(x, "data_ptr"):  # torch tensor
        assert x.is_contiguous()
        return x.data_ptr(), (DEVICE if x.is_cuda else HOST)
    raise TypeError("expected numpy array or torch tensor, got %r" % type(x))


class Engine:
    """Owns one ``fheaes_ctx``.  Thin: argument marshalling and error translation only."""

    def __init__(self, params: WopbsParameters, device: int = 0, allow_dev_build: bool = False, library=None):
        """library: the path of another build of libfheaes.so to run this context on (an A/B run); None: the product's"""
        self.params = params
        self._lib = load_library() if library is None else load_library(path=library, partial=True)
        self._h = _ctx()
        # a library built with developer knobs (csrc/knobs.h: possibly a wrong-result ablation) says so in its version string
        version = (self._lib.fheaes_version() or b"").decode()
        if version.endswith(" dev") and not (allow_dev_build or os.environ.get("FHEAES_ALLOW_DEV_BUILD") == "1"):
            raise RuntimeError("libfheaes.so is a developer build (%r): rebuild it with tfhe_aes_amd._build.build_engine(force=True), or pass "
                               "allow_dev_build=True / FHEAES_ALLOW_DEV_BUILD=1 if that is what you mean to run" % version)
        cp = params.c_struct()
        rc = self._lib.fheaes_create(ctypes.byref(cp), device, ctypes.byref(self._h))
        if rc != 0:
            raise FheAesError(rc, (self._lib.fheaes_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fheaes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise FheAesError(rc, (self._lib.fheaes_last_error(self._h) or b"").decode())

    def _space(self, *arrays):
        spaces = {s for _, s in map(_ptr, arrays) if s is not None}
        if len(spaces) != 1:
            raise ValueError("all arrays of one call must live in the same memory space")
        return spaces.pop()

    # -- keys / control ---------------------------------------------------------
    def key_words(self, which: int) -> int:
        return self._lib.fheaes_key_words(self._h, which)

    def upload_keys(self, ksk, bsk, pfpksk):
        sp = self._space(ksk, bsk, pfpksk)
        for which, a in enumerate((ksk, bsk, pfpksk)):
            n = a.size if isinstance(a, np.ndarray) else a.numel()
            if n != self.key_words(which):
                raise ValueError("key %d has %d words, expected %d" % (which, n, self.key_words(which)))
        self._check(self._lib.fheaes_upload_keys(self._h, _ptr(ksk)[0], _ptr(bsk)[0], _ptr(pfpksk)[0], sp))

    def upload_keys_seeded(self, mask_key, ksk_body, bsk_body, pfpksk_body):
        """keys as (public 256-bit mask key = 8 uint32, bodies): masks are regenerated on the GPU (include/fheaes.h)"""
        mk = np.ascontiguousarray(np.asarray(mask_key, dtype=np.uint32).reshape(8))
        sp = self._space(ksk_body, bsk_body, pfpksk_body)
        for which, a in enumerate((ksk_body, bsk_body, pfpksk_body)):
            n = a.size if isinstance(a, np.ndarray) else a.numel()
            if n != self._lib.fheaes_key_body_words(self._h, which):
                raise ValueError("key body %d has %d words, expected %d" % (which, n, self._lib.fheaes_key_body_words(self._h, which)))
        self._check(self._lib.fheaes_upload_keys_seeded(self._h, mk.ctypes.data_as(_c.POINTER(_c.c_uint32)), _ptr(ksk_body)[0], _ptr(bsk_body)[0],
                                                        _ptr(pfpksk_body)[0], sp))

    def clone_keys_from(self, other: "Engine"):
        """device-to-device copy of `other`'s converted key images into this context (fheaes_clone_keys): one PCIe upload serves
        several contexts -- on other GPUs (over xGMI) or on the same one (independent streams and workspaces)"""
        self._check(self._lib.fheaes_clone_keys(self._h, other._h))

    def clone_info(self) -> dict:
        """how the last clone_keys_from() into this context moved the keys: {"path": "none" | "same_device" | "peer" | "staged", "bytes", "seconds"}"""
        path, nbytes, secs = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_double()
        self._check(self._lib.fheaes_clone_info(self._h, ctypes.byref(path), ctypes.byref(nbytes), ctypes.byref(secs)))
        return {"path": ("none", "same_device", "peer", "staged")[path.value], "bytes": nbytes.value, "seconds": secs.value}

    def noise_level_seen(self) -> tuple[int, int]:
        """(highest number of nominal-noise ciphertexts any linear layer of this context has summed, the parameter set's limit)"""
        seen, limit = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.fheaes_noise_level_seen(self._h, ctypes.byref(seen), ctypes.byref(limit)))
        return seen.value, limit.value

    def set_stream(self, stream_handle: int | None):
        self._check(self._lib.fheaes_set_stream(self._h, stream_handle))

    def synchronize(self):
        self._check(self._lib.fheaes_synchronize(self._h))

    def reserve(self, max_bits: int):
        self._check(self._lib.fheaes_reserve(self._h, max_bits))

    # -- stages -----------------------------------------------------------------
    def keyswitch_batch(self, lwe_in, lwe_out, m: int):
        self._check(self._lib.fheaes_keyswitch_batch(self._h, _ptr(lwe_in)[0], m, _ptr(lwe_out)[0], self._space(lwe_in, lwe_out)))

    def cbs_pbs_batch(self, lwe_small, lwe_out, m: int, level: int = 1):
        self._check(self._lib.fheaes_cbs_pbs_batch(self._h, _ptr(lwe_small)[0], m, level, _ptr(lwe_out)[0], self._space(lwe_small, lwe_out)))

    def pfpks_batch(self, lwe_in, ggsw_out, m: int):
        self._check(self._lib.fheaes_pfpks_batch(self._h, _ptr(lwe_in)[0], m, _ptr(ggsw_out)[0], self._space(lwe_in, ggsw_out)))

    def forward_fourier_batch(self, polys_in, fourier_out, polys: int):
        self._check(self._lib.fheaes_forward_fourier_batch(self._h, _ptr(polys_in)[0], polys, _ptr(fourier_out)[0], self._space(polys_in, fourier_out)))

    def vertical_packing_batch(self, ggsw_fourier, n_inputs, bits, luts, n_luts, lut_per_input, lwe_out):
        self._check(self._lib.fheaes_vertical_packing_batch(self._h, _ptr(ggsw_fourier)[0], n_inputs, bits, _ptr(luts)[0], n_luts,
                                                            int(bool(lut_per_input)), _ptr(lwe_out)[0], self._space(ggsw_fourier, luts, lwe_out)))

    def inv_mix_columns_batch(self, multiples, n_blocks: int, state_out):
        """K6 alone: InvMixColumns over many_sbox(.., inv=True) of a state's bytes, [n_blocks][16][4][8][kN+1] -> [n_blocks][16][8][kN+1]"""
        self._check(self._lib.fheaes_inv_mix_columns_batch(self._h, _ptr(multiples)[0], n_blocks, _ptr(state_out)[0], self._space(multiples, state_out)))

    def wopbs_batch(self, lwe_in, n_inputs, bits, luts, n_luts, lut_per_input, lwe_out):
        self._check(self._lib.fheaes_wopbs_batch(self._h, _ptr(lwe_in)[0], n_inputs, bits, _ptr(luts)[0], n_luts, int(bool(lut_per_input)),
                                                 _ptr(lwe_out)[0], self._space(lwe_in, luts, lwe_out)))

    def sbox(self, bytes_ct, n_bytes: int, inv: bool):
        self._check(self._lib.fheaes_sbox(self._h, _ptr(bytes_ct)[0], n_bytes, int(inv), self._space(bytes_ct)))

    def many_sbox(self, bytes_ct, n_bytes: int, inv: bool, out):
        self._check(self._lib.fheaes_many_sbox(self._h, _ptr(bytes_ct)[0], n_bytes, int(inv), _ptr(out)[0], self._space(bytes_ct, out)))

    # -- Server API -------------------------------------------------------------
    def aes_key_expansion(self, key, round_keys):
        self._check(self._lib.fheaes_aes_key_expansion(self._h, _ptr(key)[0], _ptr(round_keys)[0], self._space(key, round_keys)))

    def aes_encrypt(self, round_keys, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_encrypt(self._h, _ptr(round_keys)[0], _ptr(state)[0], n_blocks, self._space(round_keys, state)))

    def aes_decrypt(self, round_keys, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_decrypt(self._h, _ptr(round_keys)[0], _ptr(state)[0], n_blocks, self._space(round_keys, state)))

    def aes_decryption_round_keys(self, round_keys, dec_round_keys):
        """the equivalent inverse cipher's round keys (FIPS-197 section 5.3.5): dw[r] = InvMixColumns(w[r]) for r = 1..9, refreshed"""
        self._check(self._lib.fheaes_aes_decryption_round_keys(self._h, _ptr(round_keys)[0], _ptr(dec_round_keys)[0],
                                                               self._space(round_keys, dec_round_keys)))

    def aes_decrypt_equivalent(self, dec_round_keys, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_decrypt_equivalent(self._h, _ptr(dec_round_keys)[0], _ptr(state)[0], n_blocks,
                                                            self._space(dec_round_keys, state)))

    # AES-192 / AES-256 (and AES-128 again): the same five with the key size as an argument, key_bits in {128, 192, 256};
    # key [key_bits/8][8][kN+1], round keys [Nr+1][16][8][kN+1] with Nr = 10 / 12 / 14
    def aes_key_expansion_bits(self, key, key_bits: int, round_keys):
        self._check(self._lib.fheaes_aes_key_expansion_bits(self._h, _ptr(key)[0], key_bits, _ptr(round_keys)[0], self._space(key, round_keys)))

    def aes_encrypt_bits(self, round_keys, key_bits: int, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_encrypt_bits(self._h, _ptr(round_keys)[0], key_bits, _ptr(state)[0], n_blocks,
                                                      self._space(round_keys, state)))

    def aes_decrypt_bits(self, round_keys, key_bits: int, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_decrypt_bits(self._h, _ptr(round_keys)[0], key_bits, _ptr(state)[0], n_blocks,
                                                      self._space(round_keys, state)))

    def aes_decryption_round_keys_bits(self, round_keys, key_bits: int, dec_round_keys):
        self._check(self._lib.fheaes_aes_decryption_round_keys_bits(self._h, _ptr(round_keys)[0], key_bits, _ptr(dec_round_keys)[0],
                                                                    self._space(round_keys, dec_round_keys)))

    def aes_decrypt_equivalent_bits(self, dec_round_keys, key_bits: int, state, n_blocks: int):
        self._check(self._lib.fheaes_aes_decrypt_equivalent_bits(self._h, _ptr(dec_round_keys)[0], key_bits, _ptr(state)[0], n_blocks,
                                                                 self._space(dec_round_keys, state)))

    def add_scalar(self, state, n_blocks: int, counters):
        cnt = np.zeros((n_blocks, 2), dtype=np.uint64)
        for i, v in enumerate(counters):
            cnt[i, 0] = (int(v) >> 64) & (2 ** 64 - 1)
            cnt[i, 1] = int(v) & (2 ** 64 - 1)
        self._check(self._lib.fheaes_add_scalar(self._h, _ptr(state)[0], n_blocks, cnt.ctypes.data_as(_u64p), self._space(state)))

    # public blocks / CTR with a public nonce: clear 128-bit values travel as host (hi, lo) pairs, as add_scalar's counters
    def _public(self, symbol: str, round_keys, key_bits: int, mid, n_blocks: int, state_out, data=None, data_per: str = "block", keys=None):
        """The one marshaller of the public-block calls: fn(ctx, round_keys, key_bits, [n_keys, key_of_block,] *mid, n_blocks, state_out,
        memspace).  `mid`: what the C signature has between the keys and n_blocks, in its order -- a list of 128-bit values goes as (hi, lo)
        pairs, an int as it is, and DATA stands for the optional `data` (None: NULL, else one block per block of the call).  `keys`:
        (n_keys, key_of_block) of a keyed call."""
        args = [] if keys is None else [keys[0], key_indices(keys[1], n_blocks)]
        for m in mid:
            if m is DATA:
                m = None if data is None else u128_pairs(data)
                if m is not None and len(m) != n_blocks:
                    raise ValueError("one data block per %s expected" % data_per)
            elif not isinstance(m, int):
                m = u128_pairs(m)
            args.append(m)
        ptrs = [m.ctypes.data_as(_u32p if m.dtype == np.uint32 else _u64p) if isinstance(m, np.ndarray) else m for m in args]
        self._check(getattr(self._lib, symbol)(self._h, _ptr(round_keys)[0], key_bits, *ptrs, n_blocks, _ptr(state_out)[0], self._space(round_keys, state_out)))

    def aes_encrypt_public_bits(self, round_keys, key_bits: int, blocks, state_out):
        self._public("fheaes_aes_encrypt_public_bits", round_keys, key_bits, [blocks], len(blocks), state_out)

    def aes_ctr_bits(self, round_keys, key_bits: int, iv: int, first_block: int, data, n_blocks: int, state_out, counter_bits: int = 128):
        """counter_bits 128: SP 800-38A CTR (fheaes_aes_ctr_bits); 32: the counter field of GCM, `iv` being the initial counter block
        (fheaes_aes_ctr32_bits)"""
        if counter_bits not in (32, 128):
            raise ValueError("counter_bits must be 32 or 128, got %r" % (counter_bits,))
        self._public("fheaes_aes_ctr32_bits" if counter_bits == 32 else "fheaes_aes_ctr_bits", round_keys, key_bits, [[iv], first_block, DATA], n_blocks, state_out,
                     data=data, data_per="counter block")

    # public blocks through the equivalent inverse cipher (dec_round_keys: aes_decryption_round_keys*), CBC decryption
    def aes_decrypt_public_bits(self, dec_round_keys, key_bits: int, blocks, data, state_out):
        self._public("fheaes_aes_decrypt_public_bits", dec_round_keys, key_bits, [blocks, DATA], len(blocks), state_out, data=data)

    def aes_cbc_decrypt_bits(self, dec_round_keys, key_bits: int, iv, ciphertext, state_out):
        self._public("fheaes_aes_cbc_decrypt_bits", dec_round_keys, key_bits, [[iv], ciphertext], len(ciphertext), state_out)

    # XTS-AES decryption: dec_round_keys1 (key 1, decryption round keys) and round_keys2 (key 2, plain expansion), or two one-key packed
    # stores; `tweaks`: the 16-byte tweak block of units 0 .. as u128 (byte 0 = MSB), `ciphertext`: the blocks of the call
    def aes_xts_decrypt_bits(self, dec_round_keys1, round_keys2, key_bits: int, tweaks, blocks_per_unit: int, first_block: int, ciphertext, state_out,
                             packed: bool = False):
        twk, cnt = u128_pairs(tweaks), u128_pairs(ciphertext)
        fn = self._lib.fheaes_aes_xts_decrypt_packed if packed else self._lib.fheaes_aes_xts_decrypt_bits
        self._check(fn(self._h, _ptr(dec_round_keys1)[0], _ptr(round_keys2)[0], key_bits, twk.ctypes.data_as(_u64p), len(twk), blocks_per_unit, first_block,
                       cnt.ctypes.data_as(_u64p), len(cnt), _ptr(state_out)[0], self._space(dec_round_keys1, round_keys2, state_out)))

    def xts_tweaks(self, anchor, n_units: int, first_offset: int, n_offsets: int, out):
        """out[u][t] = anchor[u] * alpha^(first_offset + t), the raw gather (fheaes_xts_tweaks): anchor [n_units][128][kN+1], out
        [n_units][n_offsets][128][kN+1]; needs no keys"""
        self._check(self._lib.fheaes_xts_tweaks(self._h, _ptr(anchor)[0], n_units, first_offset, n_offsets, _ptr(out)[0], self._space(anchor, out)))

    # many AES keys: round keys [n_keys][Nr+1][16][8][kN+1]; key_of_block (one key index per block) travels as a host uint32 array
    def aes_key_expansion_batch(self, keys, key_bits: int, n_keys: int, round_keys):
        self._check(self._lib.fheaes_aes_key_expansion_batch(self._h, _ptr(keys)[0], key_bits, n_keys, _ptr(round_keys)[0], self._space(keys, round_keys)))

    def aes_decryption_round_keys_batch(self, round_keys, key_bits: int, n_keys: int, dec_round_keys):
        self._check(self._lib.fheaes_aes_decryption_round_keys_batch(self._h, _ptr(round_keys)[0], key_bits, n_keys, _ptr(dec_round_keys)[0],
                                                                     self._space(round_keys, dec_round_keys)))

    def _keyed(self, fn, round_keys, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        kob = key_indices(key_of_block, n_blocks)
        self._check(fn(self._h, _ptr(round_keys)[0], key_bits, n_keys, kob.ctypes.data_as(_u32p), _ptr(state)[0], n_blocks, self._space(round_keys, state)))

    def aes_encrypt_keyed(self, round_keys, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_encrypt_keyed, round_keys, key_bits, n_keys, key_of_block, state, n_blocks)

    def aes_decrypt_keyed(self, round_keys, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_decrypt_keyed, round_keys, key_bits, n_keys, key_of_block, state, n_blocks)

    def aes_decrypt_equivalent_keyed(self, dec_round_keys, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_decrypt_equivalent_keyed, dec_round_keys, key_bits, n_keys, key_of_block, state, n_blocks)

    def aes_public_keyed(self, round_keys, key_bits: int, n_keys: int, key_of_block, blocks, data, state_out, packed: bool = False,
                         inverse: bool = False):
        """`packed`: round_keys is a packed store [n_keys][G][(k+1)N] (fheaes_aes_public_keyed_packed); `inverse`: the decryption
        direction, round_keys being decryption round keys (fheaes_aes_decrypt_public_keyed / _packed)"""
        symbol = ("fheaes_aes_decrypt_public_keyed" if inverse else "fheaes_aes_public_keyed") + ("_packed" if packed else "")
        self._public(symbol, round_keys, key_bits, [blocks, DATA], len(blocks), state_out, data=data, keys=(n_keys, key_of_block))

    # CBC-MAC chains and CCM (include/fheaes.h): the per-stream tables are host arrays, the ciphertext arrays live in one memory space
    def aes_cbc_mac_keyed(self, round_keys, key_bits: int, n_keys: int, key_of_stream, stream_blocks, clear, enc, enc_bytes, init, mac_out,
                          packed: bool = False):
        """stream s chains stream_blocks[s] blocks: `clear` [blocks][16] bytes, optionally plus the first enc_bytes[b] bytes of enc[b];
        init [n_streams][16][8][kN+1] or None; mac_out [n_streams][16][8][kN+1]"""
        sb = np.ascontiguousarray(np.asarray(stream_blocks, dtype=np.uint32).reshape(-1))
        kos = key_indices(key_of_stream, len(sb))
        clr = np.ascontiguousarray(np.asarray(clear, dtype=np.uint8).reshape(-1, 16))
        if len(clr) != int(sb.sum()):
            raise ValueError("%d clear blocks for streams of %d blocks in all" % (len(clr), int(sb.sum())))
        eb = None
        if enc is not None:
            eb = np.ascontiguousarray(np.asarray(enc_bytes, dtype=np.uint8).reshape(-1))
            if len(eb) != len(clr):
                raise ValueError("one enc_bytes entry per block expected")
        fn = self._lib.fheaes_aes_cbc_mac_keyed_packed if packed else self._lib.fheaes_aes_cbc_mac_keyed
        self._check(fn(self._h, _ptr(round_keys)[0], key_bits, n_keys, len(sb), kos.ctypes.data_as(_u32p), sb.ctypes.data_as(_u32p), clr.ctypes.data_as(_u8p),
                       _ptr(enc)[0], eb.ctypes.data_as(_u8p) if eb is not None else None, _ptr(init)[0], _ptr(mac_out)[0],
                       self._space(round_keys, enc, init, mac_out)))

    def aes_ccm_open_keyed(self, round_keys, key_bits: int, n_keys: int, key_of_stream, head_blocks, head, ctr0, payload_bytes, ciphertext, tags, tag_bytes,
                           plaintext_out, valid_out, packed: bool = False):
        """fheaes_aes_ccm_open_keyed / _packed: head_blocks[s] u128 blocks of `head` (B0, then the AAD blocks) per stream, ctr0 one u128 per
        stream, payload_bytes[s] bytes of `ciphertext` per stream, tags [n][16] bytes with tag_bytes[s] real ones"""
        hb = np.ascontiguousarray(np.asarray(head_blocks, dtype=np.uint32).reshape(-1))
        kos = key_indices(key_of_stream, len(hb))
        hd, c0 = u128_pairs(head), u128_pairs(ctr0)
        pb = np.ascontiguousarray(np.asarray(payload_bytes, dtype=np.uint64).reshape(-1))
        ct = np.frombuffer(bytes(ciphertext) + b"\x00", dtype=np.uint8)            # never an empty buffer
        tg = np.ascontiguousarray(np.asarray(tags, dtype=np.uint8).reshape(-1, 16))
        tb = np.ascontiguousarray(np.asarray(tag_bytes, dtype=np.uint32).reshape(-1))
        if not (len(c0) == len(pb) == len(tg) == len(tb) == len(hb)) or len(hd) != int(hb.sum()) or len(ct) - 1 != int(pb.sum()):
            raise ValueError("the per-stream arrays of a CCM call do not agree")
        fn = self._lib.fheaes_aes_ccm_open_keyed_packed if packed else self._lib.fheaes_aes_ccm_open_keyed
        self._check(fn(self._h, _ptr(round_keys)[0], key_bits, n_keys, len(hb), kos.ctypes.data_as(_u32p), hb.ctypes.data_as(_u32p), hd.ctypes.data_as(_u64p),
                       c0.ctypes.data_as(_u64p), pb.ctypes.data_as(_u64p), ct.ctypes.data_as(_u8p), tg.ctypes.data_as(_u8p), tb.ctypes.data_as(_u32p),
                       _ptr(plaintext_out)[0], _ptr(valid_out)[0], self._space(round_keys, plaintext_out, valid_out)))

    def mac_link(self, state, first: bool, init, enc, src_block, enc_bytes, clear):
        """K6 alone (fheaes_mac_link): state[s] = (first ? init[s] or 0 : state[s]) + the first enc_bytes[s] bytes of enc[src_block[s]]
        (MAC_NONE: none) + trivial(clear[s]); state, init [n][16][8][kN+1], enc [n_enc][16][8][kN+1]; needs no keys"""
        n = int(state.shape[0])
        clr = np.ascontiguousarray(np.asarray(clear, dtype=np.uint8).reshape(n, 16))
        src = eb = None
        if enc is not None:
            src = np.ascontiguousarray(np.asarray(src_block, dtype=np.uint32).reshape(n))
            eb = np.ascontiguousarray(np.asarray(enc_bytes, dtype=np.uint8).reshape(n))
        self._check(self._lib.fheaes_mac_link(self._h, _ptr(state)[0], n, int(bool(first)), _ptr(init)[0], _ptr(enc)[0], int(enc.shape[0]) if enc is not None else 0,
                                              src.ctypes.data_as(_u32p) if src is not None else None, eb.ctypes.data_as(_u8p) if eb is not None else None,
                                              clr.ctypes.data_as(_u8p), self._space(state, init, enc)))

    # CMAC (include/fheaes.h): the subkeys [n_keys][2][16][8][kN+1], the messages as host bytes
    def cmac_double(self, l, n_keys: int, out):
        """K6 alone (fheaes_cmac_double): out[key][which] = l[key] * x^(which + 1) in CMAC's byte order, the raw gather: l
        [n_keys][128][kN+1], out [n_keys][2][128][kN+1]; needs no keys"""
        self._check(self._lib.fheaes_cmac_double(self._h, _ptr(l)[0], n_keys, _ptr(out)[0], self._space(l, out)))

    def aes_cmac_subkeys_keyed(self, round_keys, key_bits: int, n_keys: int, subkeys_out, packed: bool = False):
        fn = self._lib.fheaes_aes_cmac_subkeys_keyed_packed if packed else self._lib.fheaes_aes_cmac_subkeys_keyed
        self._check(fn(self._h, _ptr(round_keys)[0], key_bits, n_keys, _ptr(subkeys_out)[0], self._space(round_keys, subkeys_out)))

    def aes_cmac_keyed(self, round_keys, key_bits: int, n_keys: int, subkeys, key_of_stream, message_bytes, data, tags, tag_bytes, mac_out, valid_out,
                       packed: bool = False):
        """fheaes_aes_cmac_keyed / _packed: message_bytes[s] bytes of `data` per stream; tags [n][16] bytes with tag_bytes[s] real ones, or
        both None; subkeys [n_keys][2][16][8][kN+1] or None (derived in the call)"""
        mb = np.ascontiguousarray(np.asarray(message_bytes, dtype=np.uint64).reshape(-1))
        kos = key_indices(key_of_stream, len(mb))
        dt = np.frombuffer(bytes(data) + b"\x00", dtype=np.uint8)                  # never an empty buffer
        if len(dt) - 1 != int(mb.sum()) or (tags is None) != (tag_bytes is None):
            raise ValueError("the per-stream arrays of a CMAC call do not agree")
        tg = tb = None
        if tags is not None:
            tg = np.ascontiguousarray(np.asarray(tags, dtype=np.uint8).reshape(-1, 16))
            tb = np.ascontiguousarray(np.asarray(tag_bytes, dtype=np.uint32).reshape(-1))
            if not len(tg) == len(tb) == len(mb):
                raise ValueError("the per-stream arrays of a CMAC call do not agree")
        fn = self._lib.fheaes_aes_cmac_keyed_packed if packed else self._lib.fheaes_aes_cmac_keyed
        self._check(fn(self._h, _ptr(round_keys)[0], key_bits, n_keys, _ptr(subkeys)[0], len(mb), kos.ctypes.data_as(_u32p), mb.ctypes.data_as(_u64p),
                       dt.ctypes.data_as(_u8p), tg.ctypes.data_as(_u8p) if tg is not None else None, tb.ctypes.data_as(_u32p) if tb is not None else None,
                       _ptr(mac_out)[0], _ptr(valid_out)[0], self._space(round_keys, subkeys, mac_out, valid_out)))

    # AES key unwrap (include/fheaes.h): the wrapped keys as host bytes [n_keys][8 (n + 1)], the KEKs' decryption round keys
    def kw_link(self, state, regs, semiblocks: int, step: int, wrapped=None):
        """K6 alone (fheaes_kw_link): link `step` = 0 .. 6n of the unwrap on state [n_keys][16][8][kN+1] and regs [n_keys][8 n][8][kN+1], in
        place; wrapped [n_keys][8 (n + 1)] bytes, read by step 0 alone; needs no keys"""
        n_keys = int(state.shape[0])
        wr = None
        if wrapped is not None:
            wr = wrapped_bytes(wrapped, semiblocks)
            if len(wr) != n_keys:
                raise ValueError("one wrapped key per state expected: %d for %d" % (len(wr), n_keys))
        self._check(self._lib.fheaes_kw_link(self._h, _ptr(state)[0], _ptr(regs)[0], n_keys, semiblocks, step, wr.ctypes.data_as(_u8p) if wr is not None else None,
                                             self._space(state, regs)))

    def aes_kw_unwrap_keyed(self, dec_round_keys, key_bits: int, n_keks: int, kek_of_key, semiblocks: int, wrapped, keys_out, valid_out,
                            packed: bool = False):
        """fheaes_aes_kw_unwrap_keyed / _packed: wrapped [n_keys][8 (semiblocks + 1)] bytes, kek_of_key one KEK index per key or None (one
        KEK); keys_out [n_keys][8 semiblocks][8][kN+1], valid_out [n_keys][kN+1]"""
        wr = wrapped_bytes(wrapped, semiblocks)
        n_keys = len(wr)
        kok = key_indices(kek_of_key, n_keys) if kek_of_key is not None else None
        if n_keys == 0:
            wr = np.zeros((1, 8 * (semiblocks + 1)), dtype=np.uint8)              # never an empty buffer
        fn = self._lib.fheaes_aes_kw_unwrap_keyed_packed if packed else self._lib.fheaes_aes_kw_unwrap_keyed
        self._check(fn(self._h, _ptr(dec_round_keys)[0], key_bits, n_keks, n_keys, kok.ctypes.data_as(_u32p) if kok is not None else None, semiblocks,
                       wr.ctypes.data_as(_u8p), _ptr(keys_out)[0], _ptr(valid_out)[0], self._space(dec_round_keys, keys_out, valid_out)))

    def xts_whiten(self, dst, src, tweaks, tweak_of_block, clear):
        """K6 alone (fheaes_xts_whiten): dst[b] = (src[b] or 0) + tweaks[tweak_of_block[b]] + trivial(clear[b]); src may be dst or None,
        clear [n][16] bytes or None; needs no keys"""
        n = int(dst.shape[0])
        tab = key_indices(tweak_of_block, n)
        clr = None if clear is None else np.ascontiguousarray(np.asarray(clear, dtype=np.uint8).reshape(n, 16))
        self._check(self._lib.fheaes_xts_whiten(self._h, _ptr(dst)[0], _ptr(src)[0], _ptr(tweaks)[0], int(tweaks.shape[0]), tab.ctypes.data_as(_u32p),
                                                clr.ctypes.data_as(_u8p) if clr is not None else None, n, self._space(dst, src, tweaks)))

    # packed round keys: a store [n_keys][G][(k+1)N], G = round_keys_packed_glwes(key_bits); the keyed calls read their key words from it
    def pack_round_keys(self, round_keys, key_bits: int, n_keys: int, packed_out):
        self._check(self._lib.fheaes_pack_round_keys(self._h, _ptr(round_keys)[0], key_bits, n_keys, _ptr(packed_out)[0], self._space(round_keys, packed_out)))

    def unpack_round_keys(self, packed, key_bits: int, first_key: int, n_keys: int, round_keys_out):
        self._check(self._lib.fheaes_unpack_round_keys(self._h, _ptr(packed)[0], key_bits, first_key, n_keys, _ptr(round_keys_out)[0],
                                                       self._space(packed, round_keys_out)))

    def aes_encrypt_keyed_packed(self, packed, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_encrypt_keyed_packed, packed, key_bits, n_keys, key_of_block, state, n_blocks)

    def aes_decrypt_keyed_packed(self, packed, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_decrypt_keyed_packed, packed, key_bits, n_keys, key_of_block, state, n_blocks)

    def aes_decrypt_equivalent_keyed_packed(self, packed, key_bits: int, n_keys: int, key_of_block, state, n_blocks: int):
        self._keyed(self._lib.fheaes_aes_decrypt_equivalent_keyed_packed, packed, key_bits, n_keys, key_of_block, state, n_blocks)

    # -- packed ciphertexts: N bits per GLWE (include/fheaes.h) -------------------
    def packed_words(self, m: int) -> int:
        return self._lib.fheaes_packed_words(self._h, m)

    def pack_bits(self, lwe_in, m: int, glwe_out):
        self._check(self._lib.fheaes_pack_bits(self._h, _ptr(lwe_in)[0], m, _ptr(glwe_out)[0], self._space(lwe_in, glwe_out)))

    def unpack_bits(self, glwe_in, m: int, lwe_out):
        self._check(self._lib.fheaes_unpack_bits(self._h, _ptr(glwe_in)[0], m, _ptr(lwe_out)[0], self._space(glwe_in, lwe_out)))

    # -- the gate: ciphertexts times an encrypted bit (include/fheaes.h) --
    @staticmethod
    def _runs(runs):
        r = np.ascontiguousarray(np.asarray(runs, dtype=np.uint64).reshape(-1))
        return r, r.ctypes.data_as(_u64p)

    def gate_ggsw(self, ggsw_fourier, runs, ct_in, m: int, form: int, ct_out):
        """the kernel alone on caller-made Fourier GGSWs [n_gates][1][k+1][k+1][256][2]; form GATE_LWE / GATE_GLWE; ct_out may be ct_in"""
        r, rp = self._runs(runs)
        self._check(self._lib.fheaes_gate_ggsw(self._h, _ptr(ggsw_fourier)[0], r.size, rp, _ptr(ct_in)[0], m, form, _ptr(ct_out)[0],
                                               self._space(ggsw_fourier, ct_in, ct_out)))

    def gate_bits(self, gates_lwe, runs, lwe_in, m: int, lwe_out):
        r, rp = self._runs(runs)
        self._check(self._lib.fheaes_gate_bits(self._h, _ptr(gates_lwe)[0], r.size, rp, _ptr(lwe_in)[0], m, _ptr(lwe_out)[0],
                                               self._space(gates_lwe, lwe_in, lwe_out)))

    def gate_packed(self, gates_lwe, runs, glwe_in, n_glwe: int, glwe_out):
        r, rp = self._runs(runs)
        self._check(self._lib.fheaes_gate_packed(self._h, _ptr(gates_lwe)[0], r.size, rp, _ptr(glwe_in)[0], n_glwe, _ptr(glwe_out)[0],
                                                 self._space(gates_lwe, glwe_in, glwe_out)))

    # -- wire formats: seeded input ciphertexts, modulus-switched packed outputs (include/fheaes.h) --
    def expand_lwe_seeded(self, mask_key, first_index: int, bodies, m: int, lwe_out):
        """lwe_out[t] = [mask words of ciphertext first_index + t | bodies[t]]; mask_key: the public 256-bit key, 8 uint32 on the host"""
        mk = np.ascontiguousarray(np.asarray(mask_key, dtype=np.uint32).reshape(8))
        self._check(self._lib.fheaes_expand_lwe_seeded(self._h, mk.ctypes.data_as(_u32p), int(first_index), _ptr(bodies)[0], m, _ptr(lwe_out)[0],
                                                       self._space(bodies, lwe_out)))

    def packed_words_mod(self, m: int, width: int) -> int:
        return self._lib.fheaes_packed_words_mod(self._h, m, width)

    def packed_mod_switch(self, glwe_in, n_glwe: int, width: int, out):
        self._check(self._lib.fheaes_packed_mod_switch(self._h, _ptr(glwe_in)[0], n_glwe, width, _ptr(out)[0], self._space(glwe_in, out)))

    def pack_bits_mod(self, lwe_in, m: int, width: int, out):
        self._check(self._lib.fheaes_pack_bits_mod(self._h, _ptr(lwe_in)[0], m, width, _ptr(out)[0], self._space(lwe_in, out)))

    def unpack_bits_mod(self, packed_in, m: int, width: int, lwe_out):
        self._check(self._lib.fheaes_unpack_bits_mod(self._h, _ptr(packed_in)[0], m, width, _ptr(lwe_out)[0], self._space(packed_in, lwe_out)))

    # -- measurement ------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        self._check(self._lib.fheaes_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._lib.fheaes_profile_reset(self._h))

    def profile_read(self) -> dict:
        out = {}
        for i, name in enumerate(STAGES):
            ms, launches, units = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
            self._check(self._lib.fheaes_profile_read(self._h, i, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(units)))
            out[name] = {"ms": ms.value, "launches": launches.value, "units": units.value}
        return out

    def k2_plan(self, bits: int) -> dict:
        """the blind-rotation kernel this context really launches for a batch of `bits` (after the occupancy fallbacks) and its cut"""
        form, um, rm, ut, rt = _c.c_int(), _c.c_uint64(), _c.c_uint32(), _c.c_uint64(), _c.c_uint32()
        name = _c.create_string_buffer(96)
        self._check(self._lib.fheaes_k2_context_plan(self._h, bits, _c.byref(form), _c.byref(um), _c.byref(rm), _c.byref(ut), _c.byref(rt), name, len(name)))
        return {"form": form.value, "kernel": name.value.decode(), "units_main": um.value, "r_main": rm.value,
                "units_tail": ut.value, "r_tail": rt.value}

    def k2_set_parking(self, claimed: bool):
        """paired blind-rotation kernel: parking slots claimed from a shared pool (default) or one private slot per workgroup"""
        self._check(self._lib.fheaes_k2_set_parking(self._h, 1 if claimed else 0))

    def k2_set_forms(self, allow_pair: bool = True, allow_home: bool = True):
        """test hook (fheaes_k2_set_forms): take the paired kernel and / or the 16-form's LDS-home variant away from this context, as a
        refused occupancy query does; True restores "whatever the query allows", never more.  k2_plan reports what launches"""
        self._check(self._lib.fheaes_k2_set_forms(self._h, 1 if allow_pair else 0, 1 if allow_home else 0))

    def aes_window(self, n_blocks: int, steps: int) -> int:
        """the window, in blocks, this context cuts `steps` WoPBS over n_blocks blocks into (fheaes_aes_context_window); 0: round by round"""
        w = _c.c_uint64()
        self._check(self._lib.fheaes_aes_context_window(self._h, n_blocks, steps, _c.byref(w)))
        return w.value

    def aes_set_window(self, window_blocks: int = 0):
        """fheaes_aes_set_window: 0 = automatic (default), AES_WINDOW_OFF = one launch per round, else that window forced (test hook)"""
        self._check(self._lib.fheaes_aes_set_window(self._h, int(window_blocks)))

    def k2_park_debug(self, initial=None, record: bool = False):
        """test hook (fheaes_k2_park_debug): claimed-mode paired launches start from the owner words `initial` (K2_PARK_SLOTS words;
        nonzero = taken for the whole launch) instead of zeros, None restores the default; `record`: each such launch records
        {slot, XCC} per workgroup (k2_park_read)"""
        ptr = None
        if initial is not None:
            pat = np.ascontiguousarray(np.asarray(initial, dtype=np.uint32))
            if pat.shape != (K2_PARK_SLOTS,):
                raise ValueError("initial owner words: expected %d, got shape %s" % (K2_PARK_SLOTS, pat.shape))
            ptr = pat.ctypes.data_as(_c.POINTER(_c.c_uint32))
        self._check(self._lib.fheaes_k2_park_debug(self._h, ptr, 1 if record else 0))

    def k2_park_read(self) -> dict:
        """{"fallbacks", "violations": the context's cumulative counters, "owner": uint32[K2_PARK_SLOTS] as the last claimed launch left
        them, "record": uint32[grid][2] = (slot, XCC) per workgroup of the last recorded launch (empty: none)}"""
        fb, vi, n = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
        u32p = _c.POINTER(_c.c_uint32)
        self._check(self._lib.fheaes_k2_park_read(self._h, None, None, None, None, 0, _c.byref(n)))
        owner = np.zeros(K2_PARK_SLOTS, dtype=np.uint32)
        rec = np.zeros((n.value, 2), dtype=np.uint32)
        self._check(self._lib.fheaes_k2_park_read(self._h, _c.byref(fb), _c.byref(vi), owner.ctypes.data_as(u32p), rec.ctypes.data_as(u32p),
                                                  n.value, _c.byref(n)))
        return {"fallbacks": fb.value, "violations": vi.value, "owner": owner, "record": rec[:n.value]}

    def audit_set(self, rows: int, min_bits: int = 0, seed: int = 0):
        """fheaes_audit_set: rows 0 = off; else every blind-rotation launch of this context of at least min_bits bits is re-run on
        min(rows, m) sampled rows through the latency form and compared on the device; zeroes the counters and the launch number"""
        self._check(self._lib.fheaes_audit_set(self._h, int(rows), int(min_bits), int(seed) & (2 ** 64 - 1)))

    @staticmethod
    def audit_rows(seed: int, launch: int, m: int, rows: int) -> list[int]:
        """the rows that audited launch number `launch` of m bits checks under `seed` (fheaes_audit_rows: host only, no GPU)"""
        return audit_rows(seed, launch, m, rows)

    def _audit_read(self, read, *stage) -> dict:
        """the counters and records of one audit through its C entry point, fheaes_audit_read or fheaes_audit_stage_read with its stage"""
        la, ch, wr, n = _c.c_uint64(), _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
        rec = np.zeros((AUDIT_RECORDS, 5), dtype=np.uint64)
        self._check(read(self._h, *stage, _c.byref(la), _c.byref(ch), _c.byref(wr), rec.ctypes.data_as(_u64p), AUDIT_RECORDS, _c.byref(n)))
        return {"launches": la.value, "rows_checked": ch.value, "rows_wrong": wr.value, "records": rec[:n.value]}

    def audit_read(self) -> dict:
        """{"launches", "rows_checked", "rows_wrong": the counters since audit_set, "records": uint64[n][5] = (launch, row, first differing
        word, word of the product launch, word of the audit) of the first AUDIT_RECORDS wrong rows}; synchronises the stream"""
        return self._audit_read(self._lib.fheaes_audit_read)

    def audit_debug(self, row: int, word: int, xor_mask: int):
        """test hook (fheaes_audit_debug), one shot: the next audited launch XORs xor_mask into word `word` of row `row` of its output"""
        self._check(self._lib.fheaes_audit_debug(self._h, int(row), int(word), int(xor_mask)))

    @staticmethod
    def _audit_stage(stage) -> int:
        """a name of AUDIT_STAGES (or a stage number of STAGES) -> FHEAES_STAGE_*"""
        return STAGES.index(stage) if isinstance(stage, str) else int(stage)

    def audit_stage_set(self, stage, rows: int, min_rows: int = 0, seed: int = 0):
        """fheaes_audit_stage_set: the audit of one stage of AUDIT_STAGES ("blind_rotate": audit_set); for a key switch every launch of at
        least min_rows rows is computed again on min(rows, m) sampled rows by the plain form; zeroes that stage's counters and launch number"""
        self._check(self._lib.fheaes_audit_stage_set(self._h, self._audit_stage(stage), int(rows), int(min_rows), int(seed) & (2 ** 64 - 1)))

    def audit_stage_read(self, stage) -> dict:
        """audit_read for one stage of AUDIT_STAGES; a record's word is the offset among the words the launch wrote for the row"""
        return self._audit_read(self._lib.fheaes_audit_stage_read, self._audit_stage(stage))

    def audit_stage_debug(self, stage, row: int, word: int, xor_mask: int):
        """test hook (fheaes_audit_stage_debug), one shot: that stage's next audited launch XORs xor_mask into word `word` of row `row`"""
        self._check(self._lib.fheaes_audit_stage_debug(self._h, self._audit_stage(stage), int(row), int(word), int(xor_mask)))

    def audit_plain_batch(self, stage, lwe_in, out, m: int, block: int = -1):
        """test and tool hook (fheaes_audit_plain_batch): the plain form of a key switch alone over m rows; "keyswitch": out [m][n+1];
        "pfpks": out [m][k+1][(k+1)N], or [m][(k+1)N] for one key block 0..k.  Device tensors only: the hook stages nothing"""
        if self._space(lwe_in, out) != DEVICE:
            raise ValueError("audit_plain_batch takes device tensors only")
        self._check(self._lib.fheaes_audit_plain_batch(self._h, self._audit_stage(stage), _ptr(lwe_in)[0], int(m), int(block), _ptr(out)[0]))

    def workspace_info(self) -> list[dict]:
        """test hook (fheaes_workspace_info): the context's scratch buffers, each {"name", "bytes", "class": one of WS_CLASSES, "first",
        "last": its first and last 8-byte words}; synchronises the stream"""
        out = []
        for i in range(WS_BUFFERS):
            name, nbytes, cls, first, last = _c.create_string_buffer(32), _c.c_uint64(), _c.c_int(), _c.c_uint64(), _c.c_uint64()
            self._check(self._lib.fheaes_workspace_info(self._h, i, name, len(name), _c.byref(nbytes), _c.byref(cls), _c.byref(first), _c.byref(last)))
            out.append({"name": name.value.decode(), "bytes": nbytes.value, "class": WS_CLASSES[cls.value], "first": first.value, "last": last.value})
        return out

    def workspace_poison(self, mode: int = WS_POISON_FILL) -> int:
        """test hook (fheaes_workspace_poison): WS_POISON_FILL overwrites every scratch buffer with the pattern of its class,
        WS_POISON_RELEASE frees them all (the next call grows everything from nothing); returns the bytes filled or freed"""
        n = _c.c_uint64()
        self._check(self._lib.fheaes_workspace_poison(self._h, int(mode), _c.byref(n)))
        return n.value

    def alloc_debug(self, fail_nth: int = 0) -> int:
        """test hook (fheaes_alloc_debug), one shot: the fail_nth-th device allocation this context makes from now on is refused by the
        runtime (FheAesError.code -4); 0 disarms.  Returns the allocations made since the hook was last set, and counts from 0 again"""
        n = _c.c_uint64()
        self._check(self._lib.fheaes_alloc_debug(self._h, int(fail_nth), _c.byref(n)))
        return n.value

    def read_bsk_fourier(self, i: int) -> np.ndarray:
        p = self.params
        out = np.empty((p.pbs_level, p.k + 1, p.k + 1, 256, 2), dtype=np.float64)
        self._check(self._lib.fheaes_read_bsk_fourier(self._h, i, out.ctypes.data_as(_dp)))
        return out


DATA = object()          # Engine._public: the place of the optional clear data blocks in a call's arguments


def u128_pairs(values) -> np.ndarray:
    """128-bit values (ints, or 16 `bytes` each with byte 0 the most significant) -> the (hi, lo) uint64 pairs of the C ABI, [n][2]"""
    out = np.zeros((len(values), 2), dtype=np.uint64)
    for i, v in enumerate(values):
        if isinstance(v, (bytes, bytearray)):
            if len(v) != 16:
                raise ValueError("an AES block has 16 bytes, got %d" % len(v))
            v = int.from_bytes(v, "big")
        v = int(v)
        if not 0 <= v < 1 << 128:
            raise ValueError("a block is a 128-bit value")
        out[i, 0], out[i, 1] = v >> 64, v & (2 ** 64 - 1)
    return out


def key_indices(key_of_block, n_blocks: int) -> np.ndarray:
    """one AES key index per block -> the host uint32 array of the C ABI (at least one word, so that its pointer is never NULL)"""
    idx = [int(k) for k in key_of_block]
    if len(idx) != n_blocks:
        raise ValueError("one key index per block expected: %d for %d blocks" % (len(idx), n_blocks))
    if any(not 0 <= k < 1 << 32 for k in idx):
        raise ValueError("a key index is a uint32")
    out = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    out[:n_blocks] = idx
    return out


def wrapped_bytes(wrapped, semiblocks: int) -> np.ndarray:
    """wrapped keys -- byte strings of 8 (semiblocks + 1) bytes each, or a uint8 array of them -- as the host array [n_keys][8 (semiblocks + 1)]
    of the C ABI"""
    size = 8 * (semiblocks + 1)
    if not isinstance(wrapped, np.ndarray):
        wrapped = [bytes(w) for w in wrapped]
        if any(len(w) != size for w in wrapped):
            raise ValueError("a wrapped key of %d semiblocks has %d bytes" % (semiblocks, size))
        wrapped = np.frombuffer(b"".join(wrapped), dtype=np.uint8)
    return np.ascontiguousarray(np.asarray(wrapped, dtype=np.uint8).reshape(-1, size))


def aes_public_plan_keyed(blocks, key_of_block, n_keys: int, key_bits: int = 128) -> list[int]:
    """aes_public_plan for aes_encrypt_public_keyed / aes_ctr_streams: the id of a round-1 input is (key, position, byte), so equal blocks
    under different keys share nothing (fheaes_aes_public_plan_keyed: host only, no GPU)"""
    cnt = u128_pairs(blocks)
    kob = key_indices(key_of_block, len(cnt))
    out = np.zeros(14, dtype=np.uint64)
    rc = load_library().fheaes_aes_public_plan_keyed(cnt.ctypes.data_as(_u64p), kob.ctypes.data_as(_u32p), len(cnt), n_keys, key_bits, out.ctypes.data_as(_u64p))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_public_plan_keyed: key_bits must be 128, 192 or 256, n_keys in 1..65536 and every key index below n_keys")
    return [int(x) for x in out[:{128: 10, 192: 12, 256: 14}[key_bits]]]


def aes_decrypt_public_plan_keyed(blocks, key_of_block, n_keys: int, key_bits: int = 128) -> list[int]:
    """byte-WoPBS per round (rounds 1..Nr) of aes_decrypt_public_keyed / aes_cbc_streams for these blocks; key_of_block None: one key
    (fheaes_aes_decrypt_public_plan_keyed: host only, no GPU)"""
    cnt = u128_pairs(blocks)
    kob = key_indices(key_of_block, len(cnt)) if key_of_block is not None else None
    out = np.zeros(14, dtype=np.uint64)
    rc = load_library().fheaes_aes_decrypt_public_plan_keyed(cnt.ctypes.data_as(_u64p), kob.ctypes.data_as(_u32p) if kob is not None else None, len(cnt),
                                                             n_keys, key_bits, out.ctypes.data_as(_u64p))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_decrypt_public_plan_keyed: key_bits must be 128, 192 or 256, n_keys in 1..65536 and every key index below n_keys")
    return [int(x) for x in out[:{128: 10, 192: 12, 256: 14}[key_bits]]]


def aes_decrypt_public_plan(blocks, key_bits: int = 128) -> list[int]:
    """byte-WoPBS per round (rounds 1..Nr) that aes_decrypt_public / aes_cbc_decrypt run for these blocks (host only, no GPU)"""
    return aes_decrypt_public_plan_keyed(blocks, None, 1, key_bits)


def xts_tweak_row(offset: int, bit: int) -> list[int]:
    """the source bits whose sum is output bit `bit` of the multiplication by alpha^offset in GF(2^128), offset <= 121 (fheaes_xts_tweak_row:
    host only, no GPU)"""
    src, n = (_c.c_uint32 * 4)(), _c.c_uint32()
    rc = load_library().fheaes_xts_tweak_row(offset, bit, src, _c.byref(n))
    if rc != 0:
        raise FheAesError(rc, "fheaes_xts_tweak_row: offset must be at most 121 and bit below 128")
    return [int(x) for x in src[:n.value]]


def aes_xts_plan(n_units: int, blocks_per_unit: int, first_block: int, n_blocks: int, key_bits: int = 128) -> dict:
    """fheaes_aes_xts_plan (host only, no GPU): {"segments", "tweak_refresh_bytes", "cipher_bytes", "max_terms"} of an aes_xts_decrypt call"""
    seg, ref, cip, terms = _c.c_uint64(), _c.c_uint64(), _c.c_uint64(), _c.c_uint32()
    rc = load_library().fheaes_aes_xts_plan(n_units, blocks_per_unit, first_block, n_blocks, key_bits, _c.byref(seg), _c.byref(ref), _c.byref(cip), _c.byref(terms))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_xts_plan: key_bits must be 128 or 256, blocks_per_unit in 1..2^20, and n_units cover the blocks")
    return {"segments": seg.value, "tweak_refresh_bytes": ref.value, "cipher_bytes": cip.value, "max_terms": terms.value}


def aes_mac_plan(stream_blocks, payload_blocks=None) -> dict:
    """fheaes_aes_mac_plan (host only, no GPU): what a CBC-MAC chain over streams of these lengths runs -- {"steps", "n_active" (live streams
    per cipher pass), "chained_blocks" (their sum), "public_blocks" (2 n + the payload blocks of a CCM call; 0 without payload_blocks)}"""
    sb = np.ascontiguousarray(np.asarray(stream_blocks, dtype=np.uint32).reshape(-1))
    pb = None if payload_blocks is None else np.ascontiguousarray(np.asarray(payload_blocks, dtype=np.uint32).reshape(-1))
    if pb is not None and len(pb) != len(sb):
        raise ValueError("one payload block count per stream expected")
    cap = int(sb.max()) if len(sb) else 0
    act = np.zeros(max(cap, 1), dtype=np.uint64)
    steps, pub, chained = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
    rc = load_library().fheaes_aes_mac_plan(sb.ctypes.data_as(_u32p), pb.ctypes.data_as(_u32p) if pb is not None else None, len(sb), _c.byref(steps),
                                            act.ctypes.data_as(_u64p), len(act), _c.byref(pub), _c.byref(chained))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_mac_plan: at most 2^20 streams of at most 2^16 blocks, payload blocks within them")
    return {"steps": steps.value, "n_active": [int(x) for x in act[:steps.value]], "chained_blocks": chained.value, "public_blocks": pub.value}


def cmac_subkey_row(which: int, bit: int) -> list[int]:
    """the source bits whose sum is output bit `bit` of L * x^(which + 1) in CMAC's big-endian byte order, which 0 (K1) or 1 (K2)
    (fheaes_cmac_subkey_row: host only, no GPU)"""
    src, n = (_c.c_uint32 * 3)(), _c.c_uint32()
    rc = load_library().fheaes_cmac_subkey_row(which, bit, src, _c.byref(n))
    if rc != 0:
        raise FheAesError(rc, "fheaes_cmac_subkey_row: which must be 0 or 1 and bit below 128")
    return [int(x) for x in src[:n.value]]


def aes_cmac_plan(message_bytes) -> dict:
    """fheaes_aes_cmac_plan (host only, no GPU): what a CMAC call over messages of these lengths runs -- {"steps" (cipher passes),
    "chained_blocks" (cipher blocks in all), "padded_streams" (streams whose last block takes K2)}"""
    mb = np.ascontiguousarray(np.asarray(message_bytes, dtype=np.uint64).reshape(-1))
    steps, chained, padded = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
    rc = load_library().fheaes_aes_cmac_plan(mb.ctypes.data_as(_u64p), len(mb), _c.byref(steps), _c.byref(chained), _c.byref(padded))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_cmac_plan: at most 2^20 streams of at most 16 * 2^16 bytes")
    return {"steps": steps.value, "chained_blocks": chained.value, "padded_streams": padded.value}


def aes_kw_plan(key_bits: int, semiblocks: int, n_keys: int) -> dict:
    """fheaes_aes_kw_plan (host only, no GPU): what unwrapping n_keys keys of `semiblocks` semiblocks under AES-key_bits KEKs runs --
    {"steps" (cipher passes, 6 n), "cipher_blocks" (6 n n_keys), "byte_wopbs" (the cipher's, the payload's refresh, the tag check's first)}"""
    steps, blocks, wopbs = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
    rc = load_library().fheaes_aes_kw_plan(key_bits, semiblocks, n_keys, _c.byref(steps), _c.byref(blocks), _c.byref(wopbs))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_kw_plan: key_bits 128 / 192 / 256, %d..%d semiblocks, at most %d keys" % (KW_MIN_SEMIBLOCKS, KW_MAX_SEMIBLOCKS, KW_MAX_KEYS))
    return {"steps": steps.value, "cipher_blocks": blocks.value, "byte_wopbs": wopbs.value}


def gate_plan(runs, k: int) -> dict:
    """fheaes_gate_plan (host only, no GPU): the grid a gate call over these runs launches at GLWE dimension k --
    {"workgroups", "instances_per_workgroup"}"""
    r = np.ascontiguousarray(np.asarray(runs, dtype=np.uint64).reshape(-1))
    wgs, per = _c.c_uint64(), _c.c_uint32()
    rc = load_library().fheaes_gate_plan(r.ctypes.data_as(_u64p), r.size, k, _c.byref(wgs), _c.byref(per))
    if rc != 0:
        raise FheAesError(rc, "fheaes_gate_plan: k must be 4 or 1")
    return {"workgroups": wgs.value, "instances_per_workgroup": per.value}


def audit_rows(seed: int, launch: int, m: int, rows: int) -> list[int]:
    """fheaes_audit_rows (host only, no GPU): the min(rows, m) rows, ascending, that audited launch number `launch` of m bits checks"""
    out = np.zeros(max(min(int(rows), int(m)), 1), dtype=np.uint64)
    rc = load_library().fheaes_audit_rows(int(seed) & (2 ** 64 - 1), int(launch), int(m), int(rows), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise FheAesError(rc, "fheaes_audit_rows: m at least 1 and rows in 1..%d" % AUDIT_MAX_ROWS)
    return [int(x) for x in out]


def round_keys_packed_glwes(key_bits: int) -> int:
    """GLWEs that hold one key's packed round keys: 3 / 4 / 4 for AES-128 / 192 / 256, 0 for anything else (host only, no GPU)"""
    return int(load_library().fheaes_round_keys_packed_glwes(int(key_bits)))


def aes_public_plan(blocks, key_bits: int = 128) -> list[int]:
    """byte-WoPBS per round (rounds 1..Nr) that aes_encrypt_public / aes_ctr run for these blocks (fheaes_aes_public_plan: host only, no GPU)"""
    cnt = u128_pairs(blocks)
    out = np.zeros(14, dtype=np.uint64)
    rc = load_library().fheaes_aes_public_plan(cnt.ctypes.data_as(_u64p), len(cnt), key_bits, out.ctypes.data_as(_u64p))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_public_plan: key_bits must be 128, 192 or 256")
    return [int(x) for x in out[:{128: 10, 192: 12, 256: 14}[key_bits]]]


def aes_window_plan(n_blocks: int, steps: int, cu_count: int = 256, k: int = 4) -> dict:
    """fheaes_aes_window_plan (host only, no GPU): {"window", "launches", "generations", "generations_by_round"}; window 0 = not rolled"""
    w, la, g, gr = _c.c_uint64(), _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
    rc = load_library().fheaes_aes_window_plan(n_blocks, steps, cu_count, k, _c.byref(w), _c.byref(la), _c.byref(g), _c.byref(gr))
    if rc != 0:
        raise FheAesError(rc, "fheaes_aes_window_plan: n_blocks, steps and cu_count must be at least 1")
    return {"window": w.value, "launches": la.value, "generations": g.value, "generations_by_round": gr.value}


def get_twiddles() -> np.ndarray:
    out = np.empty((512, 2), dtype=np.float64)
    rc = load_library().fheaes_get_twiddles(out.ctypes.data_as(_dp))
    if rc != 0:
        raise FheAesError(rc, "fheaes_get_twiddles")
    return out


def gen_lut(nb_block: int, f_table) -> np.ndarray:
    f = np.ascontiguousarray(f_table, dtype=np.uint64)
    if f.size != 1 << nb_block:
        raise ValueError("f_table must have 2^nb_block entries")
    out = np.empty((nb_block, max(512, 1 << nb_block)), dtype=np.uint64)
    rc = load_library().fheaes_gen_lut(nb_block, f.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise FheAesError(rc, "fheaes_gen_lut")
    return out
