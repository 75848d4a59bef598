"""The case table of workspace_state.py, pinned without a GPU: every case's inputs build in both variants and differ between them, the
clear model's answer is the published vector wherever one fits the shape (FIPS-197, SP 800-38A / B / C, IEEE 1619, RFC 3394), the
names are unique, the pairing of step c is fixed and never a case with itself, and the C entry points the cases reach are all the
entry points that take a context and a memspace, minus the explicit leftovers of workspace_state.LEFTOVERS -- so an entry point added
later fails this test until it gets a case or a reason."""
import re

import numpy as np
import pytest

import workspace_state as ws
from tfhe_aes_amd import _build, _native


@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


def memspace_entry_points():
    """the functions of include/fheaes.h whose parameters hold a context and `int memspace`"""
    text = re.sub(r"/\*.*?\*/", "", (_build.ROOT / "include" / "fheaes.h").read_text(), flags=re.S)
    found = re.findall(r"\b(fheaes_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)
    return {name for name, args in found if "fheaes_ctx" in args and re.search(r"\bint\s+memspace\b", args)}


def test_names_are_unique_and_the_pairing_is_fixed():
    names = [c.name for c in ws.CASES]
    assert len(names) == len(set(names)) == len(ws.BY_NAME) == 50
    for c in ws.CASES:
        assert c.pair in ws.GROWERS, c.name
        assert not set(ws.GROWERS[c.pair].entry) & set(c.entry), "%s is paired with its own entry point" % c.name
        assert set(ws.GROWN) <= set(ws.GROWERS[c.pair].uses)
    assert set(ws.GROWERS) == {"public_keyed_24", "decrypt_public_keyed_24"}


def test_buffer_names_are_the_header_s_count():
    used = {b for c in ws.CASES for b in c.uses}
    listed = {"ws_small", "ws_pbs", "ws_ggsw", "ws_ggswf", "ws_vp", "ws_tmp_a", "ws_tmp_b", "ws_tmp_c", "ws_luts", "ws_misc", "ws_digits", "ws_park", "ws_tree",
              "stage[0]", "stage[1]", "stage[2]", "stage[3]"}
    assert len(listed) == _native.WS_BUFFERS
    # every workspace a PARAM_TOY call can grow with resident arguments is poisoned non-empty by some case: the staging buffers belong to
    # host-memspace calls, and the toy set's blind rotation parks nothing below 257 bits
    assert used == listed - {"ws_park", "stage[0]", "stage[1]", "stage[2]", "stage[3]"}


def test_the_cases_reach_every_entry_point_with_a_context_and_a_memspace():
    declared = memspace_entry_points()
    assert declared <= set(_native.SIGNATURES) and len(declared) > 60
    reached = {e for c in ws.CASES for e in c.entry}
    assert reached <= declared, sorted(reached - declared)
    assert not reached & set(ws.LEFTOVERS), sorted(reached & set(ws.LEFTOVERS))
    assert reached | set(ws.LEFTOVERS) == declared, "no case and no reason: %s; unknown: %s" % (
        sorted(declared - reached - set(ws.LEFTOVERS)), sorted((reached | set(ws.LEFTOVERS)) - declared))
    assert all(isinstance(reason, str) and reason for reason in ws.LEFTOVERS.values())


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("case", ws.CASES + list(ws.GROWERS.values()), ids=lambda c: c.name)
def test_inputs_build_and_the_clear_model_gives_the_vectors(case, env):
    h = [case.build(env, v) for v in (0, 1)]
    for inputs in h:
        assert inputs["dev"] and all(isinstance(inputs[name], np.ndarray) and inputs[name].dtype in (np.uint64, np.float64) for name in inputs["dev"])
        assert any(k in inputs for k in ("expect", "want", "valid", "clear")), "no reference value in %s" % case.name
    assert [inputs[name].shape for name in h[0]["dev"]] == [inputs[name].shape for name in h[1]["dev"]]        # one shape, ...
    if case.pair is not None:
        assert any(not _same(h[0][name], h[1][name]) for name in h[0] if name != "dev"), "the two variants of %s are the same call" % case.name
    if "vector" in h[0]:
        model, published = h[0]["vector"]
        assert model == published, case.name
    assert "vector" not in h[1]


def test_which_cases_carry_a_published_vector(env):
    with_vector = {c.name for c in ws.CASES if "vector" in c.build(env, 0)}
    assert with_vector == {"aes_key_expansion_128", "aes_key_expansion_256", "aes_key_expansion_batch", "aes_encrypt", "aes_decrypt", "aes_decrypt_equivalent",
                           "aes_encrypt_public", "aes_ctr", "aes_decrypt_public", "aes_cbc_decrypt", "aes_cfb_decrypt", "aes_xts_decrypt", "aes_ccm_decrypt",
                           "aes_ccm_decrypt_gate", "aes_cmac_subkeys", "aes_cmac_verify", "aes_key_unwrap", "aes_key_unwrap_packed"}


def test_patterns_restate_the_header():
    assert ws.pattern_bytes("f64", 16) == bytes.fromhex("f87ff87ff87ff87f") * 2
    assert np.isnan(np.frombuffer(ws.pattern_bytes("f64", 8), dtype=np.float64)[0])
    assert ws.pattern_bytes("words", 5) == b"\xa5" * 5
    assert ws.pattern_bytes("tables", 12) == b"\x01\x00\x00\x00" * 3 and ws.pattern_bytes("tables", 7) == b"\x01\x00\x00\x00\xa5\xa5\xa5"
    assert ws.pattern_words("tables", 12) == (0x0000000100000001, 0x0000000100000001)      # the last WHOLE word: bytes 0..7 of 12
    assert ws.pattern_words("tables", 6) == (0xA5A500000001, 0xA5A500000001) and ws.pattern_words("words", 0) == (0, 0)
