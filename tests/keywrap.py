"""What the key-unwrap tests share: the six vectors of RFC 3394 section 4 as data, the link of the unwrap (kw_link_kernel) restated in
numpy as moves plus 1 << 63 on body words, the composition of older entry points that fheaes_aes_kw_unwrap_keyed must equal word for
word, and the clear key wrap of many keys at once in numpy (wrap_many), for the tests that need hundreds of blobs.  A plain module like
cmac.py: imported by name, not collected."""
import numpy as np

import ccm

h = bytes.fromhex

KEK = bytes(range(32))                                  # 000102..: its first 16 / 24 / 32 bytes are the KEKs of the vectors
PAYLOAD = h("00112233445566778899AABBCCDDEEFF" "000102030405060708090A0B0C0D0E0F")
ICV = 0xA6A6A6A6A6A6A6A6

# RFC 3394 section -> (KEK bits, payload bytes, wrapped)
VECTORS = {
    "4.1": (128, 16, h("1FA68B0A8112B447" "AEF34BD8FB5A7B82" "9D3E862371D2CFE5")),
    "4.2": (192, 16, h("96778B25AE6CA435" "F92B5B97C050AED2" "468AB8A17AD84E5D")),
    "4.3": (256, 16, h("64E8C3F9CE0F5BA2" "63E9777905818A2A" "93C8191E7D6E8AE7")),
    "4.4": (192, 24, h("031D33264E15D332" "68F24EC260743EDC" "E1C6C7DDEE725A93" "6BA814915C6762D2")),
    "4.5": (256, 24, h("A8F9BC1612C68B3F" "F6E6F4FBE30E71E4" "769C8B80A32CB895" "8CD5D17D6B254DA1")),
    "4.6": (256, 32, h("28C9F404C4B810F4" "CBCCB35CFB87F826" "3F5786E2D80ED326" "CBC7F0E71A99F43B" "FB988B9B7A02DD21")),
}


def vector(name):
    """(kek, payload, wrapped) of a VECTORS entry"""
    bits, size, wrapped = VECTORS[name]
    return KEK[:bits // 8], PAYLOAD[:size], wrapped


def register(n, s):
    """i_s: the register step s works on, 1 .. n"""
    return n - s % n


def counter(n, s):
    """t_s: the counter of step s, 6n .. 1"""
    return 6 * n - s


def rfc_steps(n):
    """(t, i) in the order of RFC 3394 2.2.2: for j = 5 .. 0, for i = n .. 1, t = n j + i"""
    return [(n * j + i, i) for j in range(5, -1, -1) for i in range(n, 0, -1)]


def add_trivial(rows, data):
    """rows [8 len(data)][kN+1] += the trivial ciphertexts of the bytes `data`: bit b of byte p is 1 << 63 on the body word of row 8p + b"""
    bits = np.array([v >> b & 1 for v in bytes(data) for b in range(8)], dtype=np.uint64)
    rows[:len(bits), -1] += bits << np.uint64(63)                    # an array add: it wraps


def np_link(state, regs, n, s, wrapped):
    """kw_link_kernel in numpy, link s = 0 .. 6n: state [n_keys][16][8][kN+1], regs [n_keys][8 n][8][kN+1], wrapped a list of n_keys byte
    strings of 8 (n + 1) bytes (read by the load alone) -> the linked (state, regs), new arrays"""
    lw = state.shape[-1]
    state, regs = state.copy(), regs.copy()
    for key in range(len(state)):
        st, rg = state[key].reshape(128, lw), regs[key].reshape(n, 64, lw)
        if s == 0:
            c = bytes(wrapped[key])
            st[:] = 0
            rg[:] = 0
            add_trivial(st[:64], (int.from_bytes(c[:8], "big") ^ counter(n, 0)).to_bytes(8, "big"))
            add_trivial(st[64:], c[8 * n:])
            add_trivial(rg.reshape(64 * n, lw), c[8:])
        elif s < 6 * n:
            back = st[64:].copy()
            st[64:] = rg[register(n, s) - 1]
            rg[register(n, s - 1) - 1] = back
            add_trivial(st[:64], counter(n, s).to_bytes(8, "big"))
        else:
            rg[0] = st[64:]
            st[64:] = 0
            add_trivial(st[:64], ICV.to_bytes(8, "big"))
    return state, regs


def _xtime(v):
    return ((v << 1) ^ np.where(v & 0x80, 0x1B, 0)) & 0xFF


def np_encrypt_blocks(round_keys, blocks):
    """AES encryption (FIPS-197 Fig. 5) of many blocks at once in numpy: round_keys [n][Nr+1][16] and blocks [n][16], bytes as integers ->
    [n][16].  What a test uses where hundreds of aes_clear.aes_encrypt_block calls would be its cost; held to aes_clear by
    test_chunk_seams_calls_cpu.py"""
    from tfhe_aes_amd import aes_clear

    sbox = np.array(aes_clear.SBOX, dtype=np.int64)
    shift = np.array([(i + 4 * (i % 4)) % 16 for i in range(16)])          # ShiftRows on the column-major state
    rk = np.asarray(round_keys, dtype=np.int64)
    s = np.asarray(blocks, dtype=np.int64) ^ rk[:, 0]
    nr = rk.shape[1] - 1
    for rnd in range(1, nr + 1):
        s = sbox[s][:, shift]
        if rnd < nr:
            c = s.reshape(-1, 4, 4)
            every = c[:, :, 0:1] ^ c[:, :, 1:2] ^ c[:, :, 2:3] ^ c[:, :, 3:4]
            s = (c ^ every ^ _xtime(c ^ np.roll(c, -1, axis=2))).reshape(-1, 16)
        s = s ^ rk[:, rnd]
    return s


def wrap_many(keks, kek_of_key, payloads):
    """aes_clear.key_wrap of payloads[j] under keks[kek_of_key[j]] for all j at once (payloads of one length): a list of byte strings"""
    from tfhe_aes_amd import aes_clear

    expanded = np.array([aes_clear.expand_key(k) for k in keks], dtype=np.int64)
    rk = expanded[np.asarray(kek_of_key)]
    r = np.array([list(d) for d in payloads], dtype=np.int64).reshape(len(payloads), -1, 8)
    n = r.shape[1]
    a = np.tile(np.array(list(ICV.to_bytes(8, "big")), dtype=np.int64), (len(payloads), 1))
    for j in range(6):
        for i in range(n):
            b = np_encrypt_blocks(rk, np.concatenate([a, r[:, i]], axis=1))
            a, r[:, i] = b[:, :8] ^ np.array(list((n * j + i + 1).to_bytes(8, "big")), dtype=np.int64), b[:, 8:]
    return [bytes(x.tolist()) + bytes(y.reshape(-1).tolist()) for x, y in zip(a, r)]


def compose_unwrap(server, tc, dec_rk, kek_of_key, wrapped):
    """fheaes_aes_kw_unwrap_keyed out of np_link and older calls, on host arrays: per step the link and aes_decrypt_equivalent_keyed on all
    states, the last link, the identity WoPBS XTS and CMAC use on the registers, and the two WoPBS of ccm.tag_luts on the state (the
    composition cmac.compose_verify ends with).  dec_rk [n_keks][Nr+1][16][8][kN+1]; returns (keys [n_keys][8 n][8][kN+1], valid
    [n_keys][kN+1])"""
    from oracle import oracle as orc
    from xts import LUTSET_IDENTITY

    lw = tc.params.big1
    n_keys, n = len(wrapped), len(wrapped[0]) // 8 - 1
    kek_of_key = [0] * n_keys if kek_of_key is None else list(kek_of_key)
    state = np.zeros((n_keys, 16, 8, lw), dtype=np.uint64)
    regs = np.zeros((n_keys, 8 * n, 8, lw), dtype=np.uint64)
    for s in range(6 * n):
        state, regs = np_link(state, regs, n, s, wrapped)
        server.aes_decrypt_equivalent_keyed(dec_rk, kek_of_key, state)
    state, regs = np_link(state, regs, n, 6 * n, wrapped)
    ident = list(orc.build_lutset(LUTSET_IDENTITY))
    keys = np.ascontiguousarray(server.many_wopbs_without_padding(regs.reshape(-1, 8, lw), ident)[:, 0]).reshape(regs.shape)
    ne0, eq0 = ccm.tag_luts()
    w1 = server.many_wopbs_without_padding(state.reshape(16 * n_keys, 8, lw), [ne0])
    w2 = server.many_wopbs_without_padding(np.ascontiguousarray(w1[:, 0, 0, :]).reshape(n_keys, 16, lw), [eq0])
    return keys, np.ascontiguousarray(w2[:, 0, 0, :])
