"""Packed round keys without a GPU: the host-only entry point and the binding, the numpy model of "key word from the packed form"
(packed_key_model.py) against the reference of the packing (aes_model.ref_pack / ref_unpack), the PackedRoundKeys value and its file form."""
import numpy as np
import pytest

from aes_model import ref_pack, ref_unpack
from aes_vectors import A2_KEY, NR, key_words, own_client
from packed_key_model import key_bit, key_glwes, key_lwe, key_word
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native, aes_clear
from tfhe_aes_amd.client import PackedRoundKeys, load_ciphertexts, packed_key_glwes, save_ciphertexts

NEW_SYMBOLS = ("fheaes_round_keys_packed_glwes", "fheaes_pack_round_keys", "fheaes_unpack_round_keys", "fheaes_aes_encrypt_keyed_packed",
               "fheaes_aes_decrypt_keyed_packed", "fheaes_aes_decrypt_equivalent_keyed_packed", "fheaes_aes_public_keyed_packed")


def test_glwes_per_key_and_the_new_symbols():
    lib = _native.load_library()
    assert [lib.fheaes_round_keys_packed_glwes(b) for b in (128, 192, 256)] == [3, 4, 4]
    assert [lib.fheaes_round_keys_packed_glwes(b) for b in (0, 64, 129, 512)] == [0, 0, 0, 0]
    assert [_native.round_keys_packed_glwes(b) for b in (128, 192, 256, 100)] == [3, 4, 4, 0]
    for bits in (128, 192, 256):
        assert packed_key_glwes(PARAM_OPT, bits) == key_glwes(PARAM_OPT, bits) == lib.fheaes_round_keys_packed_glwes(bits)
    for name in NEW_SYMBOLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES and hasattr(lib, name)
    # the sizes the header quotes, at PARAM_OPT
    lwe = {b: (NR[b] + 1) * 128 * PARAM_OPT.big1 * 8 for b in NR}
    packed = {b: key_glwes(PARAM_OPT, b) * (PARAM_OPT.k + 1) * PARAM_OPT.N * 8 for b in NR}
    assert lwe == {128: 23079936, 192: 27276288, 256: 31472640} and packed == {128: 61440, 192: 81920, 256: 81920}
    assert 65536 * packed[128] == 4026531840 and round(lwe[128] / packed[128], 1) == 375.6


@pytest.fixture(scope="module")
def toy_store(toy):
    """the round keys of an AES-192 key (13 x 128 = 1,664 bits: GLWE 3 a quarter filled) as fresh encryptions, their reference packing, its
    reference extraction, and a two-key store whose second key is the first with every word complemented"""
    c = own_client(toy)
    rk = c.encrypt_bytes(key_words(aes_clear.expand_key(A2_KEY)).reshape(-1)).reshape(13, 16, 8, toy.params.big1)
    packed = ref_pack(toy, rk)
    assert packed.shape == (4, (toy.params.k + 1) * toy.params.N)
    store = np.stack([packed, ~packed])
    return rk, packed, ref_unpack(packed, 1664, toy.params), store


@pytest.mark.parametrize("t", [0, 511, 512, 1663], ids=["first bit", "last coefficient", "second GLWE", "last bit of AES-192"])
def test_key_word_model_is_the_extraction_of_the_reference_packing(toy, toy_store, t):
    p = toy.params
    _, packed, lwe, store = toy_store
    got = key_lwe(store, 192, 0, t, p)
    assert np.array_equal(got, lwe[t])
    assert [key_word(store, 192, 0, t, w, p) for w in (0, 1, t % p.N, (t % p.N + 1) % p.N, p.N - 1, p.big)] == \
        [int(lwe[t][w]) for w in (0, 1, t % p.N, (t % p.N + 1) % p.N, p.N - 1, p.big)]
    glwe = packed[t // p.N].reshape(p.k + 1, p.N)
    i = t % p.N
    neg = np.uint64(0) - glwe[0]
    assert got[p.big] == glwe[p.k, i]
    assert np.array_equal(got[:i + 1], glwe[0, i::-1])                               # c <= i: A[i - c], as it is
    assert np.array_equal(got[i + 1:p.N], neg[:i:-1])                                # c > i: -A[i - c + N]
    if t == 0:
        assert got[0] == glwe[0, 0] and np.array_equal(got[1:p.N], neg[:0:-1])       # every mask word but c = 0 negated
    if t == 511:
        assert np.array_equal(got[:p.N], glwe[0, ::-1])                              # none negated
    # the second key of the store: found by its offset, G GLWEs on
    second = ref_unpack(store[1], 1664, p)
    assert np.array_equal(key_lwe(store, 192, 1, t, p), second[t])
    assert key_word(store, 192, 1, t, 3, p) == int(second[t][3]) and key_word(store, 192, 1, t, p.big, p) == int(second[t][p.big])


def test_bit_positions_of_the_definition(toy, toy_store):
    """bit t = round * 128 + byte * 8 + bit: the model reads round keys [Nr+1][16][8] in their own order, and the packed bits decrypt to them"""
    p = toy.params
    rk, packed, lwe, store = toy_store
    assert key_bit(0, 0, 0) == 0 and key_bit(3, 15, 7) == 511 and key_bit(4, 0, 0) == 512 and key_bit(12, 15, 7) == 1663
    c = own_client(toy)
    want = c.decrypt_bits(rk.reshape(-1, p.big1))
    assert np.array_equal(c.decrypt_packed(packed, 1664), want)
    for rnd, byte, bit in ((0, 0, 0), (3, 15, 7), (4, 0, 0), (7, 9, 2), (12, 15, 7)):
        t = key_bit(rnd, byte, bit)
        assert c.decrypt_bits(key_lwe(store, 192, 0, t, p)[None])[0] == want[t]


# ---- the PackedRoundKeys value -------------------------------------------------------------------------------------------------------------
def _store(p, bits, n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 63, (n, key_glwes(p, bits), (p.k + 1) * p.N), dtype=np.uint64)


def test_packed_round_keys_shapes_slices_and_concat():
    p = PARAM_TOY
    a = PackedRoundKeys(p, 128, _store(p, 128, 3))
    assert (a.n_keys, len(a), a.key_bits, a.nbytes) == (3, 3, 128, 3 * 3 * 1024 * 8) and a.params is p
    assert PackedRoundKeys(PARAM_OPT, 128, _store(PARAM_OPT, 128, 1)).nbytes == 61440
    assert PackedRoundKeys(PARAM_OPT, 256, _store(PARAM_OPT, 256, 2)).nbytes == 2 * 81920
    one = a[1]
    assert isinstance(one, PackedRoundKeys) and one.n_keys == 1 and one.key_bits == 128 and np.array_equal(one.data[0], a.data[1])
    assert np.array_equal(a[-1].data[0], a.data[2])
    assert np.shares_memory(one.data, a.data)                                        # a slice is a view: a key is a store on its own
    part = a[1:]
    assert part.n_keys == 2 and np.array_equal(part.data, a.data[1:])
    b = PackedRoundKeys(p, 128, _store(p, 128, 2, seed=2))
    joined = PackedRoundKeys.concat([a[2], b, a[:1]])
    assert joined.n_keys == 4 and np.array_equal(joined.data, np.concatenate([a.data[2:3], b.data, a.data[:1]]))
    for bad in (lambda: PackedRoundKeys(p, 128, _store(p, 192, 2)),                  # 4 GLWEs a key are not AES-128
                lambda: PackedRoundKeys(p, 192, _store(p, 128, 2)),
                lambda: PackedRoundKeys(p, 100, _store(p, 128, 2)),
                lambda: PackedRoundKeys(p, 128, _store(p, 128, 2)[0]),               # one key is [1][G][..]
                lambda: PackedRoundKeys(p, 128, _store(p, 128, 2)[:, :, :-1]),
                lambda: PackedRoundKeys(PARAM_OPT, 128, _store(p, 128, 2)),
                lambda: a[1:1], lambda: a[::2],
                lambda: PackedRoundKeys.concat([]),
                lambda: PackedRoundKeys.concat([a, PackedRoundKeys(p, 192, _store(p, 192, 1))])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(IndexError):
        a[3]


def test_packed_round_keys_file_round_trip(tmp_path):
    p = PARAM_TOY
    prk = PackedRoundKeys(p, 192, _store(p, 192, 2, seed=3))
    path = tmp_path / "keys.npz"
    save_ciphertexts(path, p, "packed_round_keys", prk)
    for back in (load_ciphertexts(path, p, "packed_round_keys"), load_ciphertexts(path, p, "packed_round_keys", key_bits=192)):
        assert isinstance(back, PackedRoundKeys) and (back.key_bits, back.n_keys) == (192, 2) and back.params == p
        assert back.data.dtype == np.uint64 and np.array_equal(back.data, prk.data)
    for bad in (lambda: load_ciphertexts(path, p, "packed_round_keys", key_bits=256),    # 4 GLWEs a key as well, but the file says 192
                lambda: load_ciphertexts(path, p, "packed_round_keys", key_bits=128),
                lambda: load_ciphertexts(path, p, "packed"),
                lambda: load_ciphertexts(path, p, "round_keys"),
                lambda: load_ciphertexts(path, PARAM_OPT, "packed_round_keys"),
                lambda: load_ciphertexts(path, p, "packed_round_keys", width=16),
                lambda: save_ciphertexts(path, p, "packed_round_keys", prk.data),        # the bare words do not say their key size
                lambda: save_ciphertexts(path, PARAM_OPT, "packed_round_keys", prk),
                lambda: save_ciphertexts(path, p, "packed", prk)):
        with pytest.raises((ValueError, TypeError)):
            bad()
    other = tmp_path / "packed.npz"
    save_ciphertexts(other, p, "packed", prk.data.reshape(-1, 1024))
    with pytest.raises(ValueError):
        load_ciphertexts(other, p, "packed_round_keys")
    with pytest.raises(ValueError):
        load_ciphertexts(other, p, "packed", key_bits=192)
