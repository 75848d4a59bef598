"""What test_gpu_alloc_failures.py needs beside the case table of workspace_state.py: the expected refusal code of every entry point that
allocates, the number of device allocations each case of workspace_state.CASES makes from a released workspace (the `A` of the sweep;
counted with fheaes_alloc_debug armed far ahead, fixed by the schedule of the call at PARAM_TOY and not by the device), the positions at
which a failed call is repeated without a release, which inputs a call writes, and the probe.  A helper module like workspace_state.py:
no test, no fixture.  test_alloc_failures_cpu.py pins it without a GPU.

The contract under test is written at FHEAES_ERR_NOMEM in include/fheaes.h."""
import re

import numpy as np

import workspace_state as ws

OK, INVALID, NOKEYS, DEVICE, NOMEM = 0, -1, -2, -3, -4
FAR = 1 << 62                     # fheaes_alloc_debug armed this far ahead never fires: it only counts

# what a refused allocation makes of the call, per entry point: every case's entry points and the five calls outside the table
REFUSAL = {e: NOMEM for c in ws.CASES for e in c.entry}
REFUSAL.update({"fheaes_reserve": NOMEM, "fheaes_upload_keys": NOMEM, "fheaes_upload_keys_seeded": NOMEM, "fheaes_clone_keys": NOMEM, "fheaes_audit_set": NOMEM,
                "fheaes_k2_park_debug": NOMEM})

# A per case: ctx_malloc calls of the case's run on resident inputs after fheaes_workspace_poison(RELEASE).  At least one per buffer
# the run leaves non-empty; more where the schedule grows a buffer twice (K1's digit planes, then K3's larger ones, in every WoPBS).
ALLOCATIONS = {
    "k1_keyswitch": 1, "k2_cbs_pbs": 0, "k3_pfpks": 1, "k4_forward_fourier": 0, "k5_vertical_packing": 0, "wopbs_8_bits_shared_luts": 6,
    "wopbs_9_bits_per_input_luts": 6, "wopbs_11_bits_tree": 7, "sbox": 7, "sbox_inv": 7, "many_sbox": 6, "many_sbox_inv": 6,
    "aes_key_expansion_128": 8, "aes_key_expansion_256": 8, "aes_key_expansion_batch": 9, "aes_decryption_round_keys": 9,
    "aes_decryption_round_keys_batch": 10, "aes_encrypt": 7, "aes_decrypt": 7, "aes_decrypt_equivalent": 7, "aes_encrypt_keyed": 9,
    "aes_decrypt_keyed": 9, "aes_decrypt_equivalent_keyed": 9, "aes_encrypt_keyed_packed": 8, "aes_decrypt_keyed_packed": 8,
    "aes_decrypt_equivalent_keyed_packed": 8, "pack_unpack_round_keys": 2, "add_scalar": 14, "aes_encrypt_public": 21, "aes_ctr": 21, "aes_ctr32": 22,
    "aes_decrypt_public": 9, "aes_cbc_decrypt": 9, "aes_cfb_decrypt": 9, "aes_public_keyed": 21, "aes_decrypt_public_keyed": 21,
    "aes_xts_decrypt": 29, "aes_cbc_mac_streams": 9, "aes_ccm_decrypt": 28, "aes_ccm_decrypt_gate": 28, "aes_cmac_subkeys": 18, "aes_cmac_verify": 20,
    "aes_key_unwrap": 11, "aes_key_unwrap_packed": 13, "gate": 7, "gate_packed": 6, "gate_ggsw": 3, "pack_unpack_513": 2,
    "pack_unpack_513_width16": 3, "expand_seeded": 0,
}

# cases that take longer than the slowest PARAM_TOY test of the suite with every position refused: step 3 at every second position (the
# retry positions always among them)
THINNED = frozenset()

# the device allocations of an upload on a context without key images: the three images, the staging array of the full keys (host
# memspace, or seeded: the masks are expanded into it), the staging array of the bodies (seeded from host memory)
UPLOAD_ALLOCATIONS = {("plain", "host"): 4, ("plain", "device"): 3, ("seeded", "host"): 5, ("seeded", "device"): 4}
IMAGES = 3


def retry_positions(a):
    """the refusals after which the call is repeated without a release: the first, the middle and the last allocation"""
    return sorted({1, (a + 1) // 2, a}) if a > 0 else []


def fail_positions(a, thinned=False):
    """the allocations that are refused, one run each: all of them; thinned: every second one and the retry positions"""
    return sorted(set(range(1, a + 1, 2 if thinned else 1)) | set(retry_positions(a)))


def written(case):
    """the resident inputs the case's call writes (in-place calls); every other input is only read"""
    return {"state"} | ({"x"} if case.name in ("sbox", "sbox_inv") else set())


def refused_bytes(message):
    """the byte count a refusal's message names, or None"""
    m = re.search(r"hipMalloc\((\d+) bytes\)", message)
    return int(m.group(1)) if m else None


def probe_inputs(env):
    """one fixed ciphertext and the oracle's key switch of it.  fheaes_keyswitch_batch ends in HIP_TRY(hipGetLastError()): an error state
    that a refused allocation left on the thread would make this call, whose kernels ran, come back FHEAES_ERR_DEVICE"""
    x = env.client.encrypt_bits(np.array([1], dtype=np.uint8)).reshape(1, env.p.big1)
    return {"x": x, "want": env.oracle.keyswitch(x)}
