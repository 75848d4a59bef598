// aes_schedule.h -- the AES schedules of the reference's Server (src/server/server.rs:39-178) on device buffers: encryption, both
// decryptions, the decryption round keys, the key expansion, add_scalar, public blocks / CTR with a public nonce, and XTS decryption.
#pragma once

static int many_sbox_dev(fheaes_ctx *c, const uint64_t *bytes, uint64_t n_bytes, int set, uint64_t *out)
{
    return wopbs_dev(c, bytes, n_bytes, 8, c->lutset_d[set], (uint32_t)c->lutset_n[set], 0, out);
}

// ---- Server API -------------------------------------------------------------------------------
// FIPS-197 Fig. 4: Nr = 10 / 12 / 14 rounds for Nk = 4 / 6 / 8 key words; 0: not an AES key size.  The reference is AES-128 only
// (server.rs:107, main.rs); every schedule below is its schedule with Nr in place of 10.
static int aes_rounds(uint32_t key_bits) { return key_bits == 128 ? 10 : key_bits == 192 ? 12 : key_bits == 256 ? 14 : 0; }

static int check_key_bits(fheaes_ctx *c, uint32_t key_bits)
{
    if (!aes_rounds(key_bits)) return c->fail(FHEAES_ERR_INVALID, "key_bits must be 128, 192 or 256, got %u", key_bits);
    return FHEAES_OK;
}

// A block cipher is an initial AddRoundKey and a list of steps.  A step: a WoPBS with LUT set `set` on every state byte, then the linear
// layer `table` over its n_luts outputs per byte plus round key `key_round` of the call's keys (< 0: none), written over the state.
struct AesStep { int set; uint32_t n_luts; GatherTable table; int key_round; };
struct AesSchedule {
    int first_key_round = 0;
    uint32_t max_luts = 0;
    std::vector<AesStep> steps;
    void add(int set, uint32_t n_luts, const GatherTable &t, int key_round) { steps.push_back({set, n_luts, t, key_round}); max_luts = std::max(max_luts, n_luts); }
};

static AesSchedule aes_encrypt_schedule(int nr)
{
    AesSchedule s;
    s.first_key_round = 0;                                                               // server.rs:42
    for (int round = 1; round < nr; ++round) s.add(LUTSET_ENC_ROUND, 3, table_enc_round(), round);          // server.rs:44-57
    s.add(LUTSET_SBOX, 1, table_shift_rows(false), nr);                                  // server.rs:59-63
    return s;
}

// the reference's own schedule (server.rs:67-105): 2 Nr - 1 WoPBS per block
static AesSchedule aes_decrypt_schedule(int nr)
{
    AesSchedule s;
    s.first_key_round = nr;                                                              // server.rs:70
    for (int round = nr; round >= 2; --round) {                                          // server.rs:72-96
        // inv_shift_rows commutes with the bytewise S-Box: INV_SBOX first, then the permutation + round key
        s.add(LUTSET_INV_SBOX, 1, table_shift_rows(true), round - 1);
        s.add(LUTSET_DEC_MUL, 4, table_dec_mix(), -1);
    }
    s.add(LUTSET_INV_SBOX, 1, table_shift_rows(true), 0);                                // server.rs:98-104
    return s;
}

// The equivalent inverse cipher (FIPS-197 section 5.3.5, Fig. 15): InvMixColumns is linear, so IMC(InvS(x)) + IMC(w[r]) is one WoPBS
// per byte with the composed tables {9, 11, 13, 14} * InvS[x] (LUTSET_DEC_EQ_ROUND), summed through the InvShiftRows-folded gather with
// dw[r] = IMC(w[r]) as the round key: Nr WoPBS per block like encryption, against the 2 Nr - 1 of aes_decrypt_schedule (the reference's own
// schedule, server.rs:67-105, which says at :86-89 that it almost doubles the time of encryption).  dw: fheaes_aes_decryption_round_keys.
static AesSchedule aes_decrypt_eq_schedule(int nr)
{
    AesSchedule s;
    s.first_key_round = nr;
    for (int round = nr - 1; round >= 1; --round) s.add(LUTSET_DEC_EQ_ROUND, 4, table_dec_eq_round(), round);   // 4 WoPBS outputs + dw[round] = 5
    s.add(LUTSET_INV_SBOX, 1, table_shift_rows(true), 0);
    return s;
}

// Runs a schedule over n blocks.  Window 0 (aes_context_window): step by step, one WoPBS over all blocks each.  Window w: the steps x n
// block-rounds, in (step, block) order, are cut into launches of w; launch j covers stream indices [j w, j w + w), at most two segments:
// blocks [b0, n) of step s and blocks [0, b1) of step s + 1, b1 <= b0.  K1 reads each segment from its place in the state into consecutive
// rows of ws_small; K2, K3 and K4 run once over the window; K5 once, or per segment where the two steps' LUT sets differ (the second
// segment's outputs lie behind the first's in ws_vp); the linear layer per segment, over the state in place.  Segments are whole blocks of
// 128 ciphertexts, K1's tile.  No block is twice in a window (w <= n), so a launch reads only what the launches before it wrote.
static int aes_run_dev(fheaes_ctx *c, const KeySets &rk, uint64_t *state, uint64_t n_blocks, const AesSchedule &sch)
{
    const uint64_t bw = 8ull * c->big1, sw = 16 * bw, steps = sch.steps.size();
    auto key_of = [&](const AesStep &st, uint64_t first_block) {
        if (st.key_round < 0) return KeySets{nullptr, nullptr, 0};
        return rk.round((uint64_t)st.key_round, sw, first_block);
    };
    const uint64_t w = aes_context_window(c, n_blocks, steps);
    TRY(ensure(c, c->ws_vp, (w ? w : n_blocks) * 16 * sch.max_luts * bw * 8));
    uint64_t *vp = (uint64_t *)c->ws_vp.p;
    TRY(launch_add_bcast(c, state, rk.round((uint64_t)sch.first_key_round, sw), sw, n_blocks));
    if (w == 0) {
        for (const AesStep &st : sch.steps) {
            TRY(many_sbox_dev(c, state, 16 * n_blocks, st.set, vp));
            TRY(launch_gather(c, vp, st.n_luts, key_of(st, 0), state, n_blocks, st.table));
        }
        return FHEAES_OK;
    }
    const uint64_t ggsw_words = (uint64_t)c->k1 * c->k1 * FHE_N, total = steps * n_blocks;     // cbs_level == 1
    TRY(ensure_wopbs_ws(c, w * AES_BLOCK_BITS));
    uint64_t *small = (uint64_t *)c->ws_small.p;
    const double2 *ggswf = (const double2 *)c->ws_ggswf.p;
    struct Segment { const AesStep *st; uint64_t first, blocks, row; uint64_t *vp; };            // row: its first block's place in the window
    for (uint64_t i0 = 0; i0 < total; i0 += w) {
        const uint64_t len = std::min<uint64_t>(w, total - i0), s = i0 / n_blocks, b0 = i0 % n_blocks, m = len * AES_BLOCK_BITS;
        Segment seg[2] = {{&sch.steps[s], b0, std::min<uint64_t>(len, n_blocks - b0), 0, vp}, {}};
        int n_seg = 1;
        if (seg[0].blocks < len) {
            seg[1] = {&sch.steps[s + 1], 0, len - seg[0].blocks, seg[0].blocks, vp + seg[0].blocks * 16 * seg[0].st->n_luts * bw};
            n_seg = 2;
        }
        for (int g = 0; g < n_seg; ++g)
            TRY(launch_keyswitch(c, state + seg[g].first * sw, seg[g].blocks * AES_BLOCK_BITS, small + seg[g].row * AES_BLOCK_BITS * (c->n + 1)));
        TRY(cbs_from_small(c, m));
        if (n_seg == 1 || seg[0].st->set == seg[1].st->set) {
            const int set = seg[0].st->set;
            TRY(launch_vertical_packing(c, ggswf, 16 * len, 8, c->lutset_d[set], (uint32_t)c->lutset_n[set], 0, vp));
        } else {
            for (int g = 0; g < n_seg; ++g) {
                const int set = seg[g].st->set;
                TRY(launch_vertical_packing(c, ggswf + seg[g].row * AES_BLOCK_BITS * (ggsw_words / 2), 16 * seg[g].blocks, 8, c->lutset_d[set],
                                            (uint32_t)c->lutset_n[set], 0, seg[g].vp));
            }
        }
        for (int g = 0; g < n_seg; ++g)
            TRY(launch_gather(c, seg[g].vp, seg[g].st->n_luts, key_of(*seg[g].st, seg[g].first), state + seg[g].first * sw, seg[g].blocks, seg[g].st->table));
    }
    return FHEAES_OK;
}

static int aes_encrypt_dev(fheaes_ctx *c, const KeySets &rk, uint64_t *state, uint64_t n_blocks, int nr) { return aes_run_dev(c, rk, state, n_blocks, aes_encrypt_schedule(nr)); }
static int aes_decrypt_dev(fheaes_ctx *c, const KeySets &rk, uint64_t *state, uint64_t n_blocks, int nr) { return aes_run_dev(c, rk, state, n_blocks, aes_decrypt_schedule(nr)); }
static int aes_decrypt_eq_dev(fheaes_ctx *c, const KeySets &dw, uint64_t *state, uint64_t n_blocks, int nr) { return aes_run_dev(c, dw, state, n_blocks, aes_decrypt_eq_schedule(nr)); }

typedef int (*AesDevFn)(fheaes_ctx *, const KeySets &, uint64_t *, uint64_t, int);

// dw[0] = w[0], dw[Nr] = w[Nr], dw[r] = InvMixColumns(w[r]) for r = 1..Nr-1, for n_keys sets of round keys [n_keys][Nr+1][16]: the
// 16 (Nr - 1) n_keys middle bytes in one batch -- the 4-LUT {9x, 11x, 13x, 14x} WoPBS, the InvMixColumns gather (4 terms, no key) and an
// identity WoPBS that brings every byte back to nominal noise, as the key expansion's refresh does (server.rs:150): a round of the
// equivalent inverse cipher then sums 4 WoPBS outputs + 1 key.  A WoPBS reads and writes contiguous bytes: with several keys the middle
// bytes are gathered from their stride first and the refreshed ones placed back; one key's already are where they belong.
static int dec_round_keys_dev(fheaes_ctx *c, const uint64_t *w, uint64_t *dw, int nr, uint64_t n_keys)
{
    const uint64_t bw = 8ull * c->big1, sw = 16 * bw, ks = (uint64_t)(nr + 1) * sw, mid = (uint64_t)(nr - 1) * 16, nbytes = mid * n_keys;
    const bool strided = n_keys > 1;
    TRY(ensure(c, c->ws_vp, nbytes * 4 * bw * 8));
    TRY(ensure(c, c->ws_tmp_a, nbytes * bw * 8));
    if (strided) TRY(ensure(c, c->ws_tmp_b, nbytes * bw * 8));
    uint64_t *vp = (uint64_t *)c->ws_vp.p, *mix = (uint64_t *)c->ws_tmp_a.p, *flat = (uint64_t *)c->ws_tmp_b.p;
    TRY(launch_key_rows(c, dw, ks, w, ks, 0, nullptr, 0, 0, 16, n_keys, 1));
    TRY(launch_key_rows(c, dw + (uint64_t)nr * sw, ks, w + (uint64_t)nr * sw, ks, 0, nullptr, 0, 0, 16, n_keys, 1));
    if (strided) TRY(launch_key_rows(c, flat, mid * bw, w + sw, ks, 0, nullptr, 0, 0, (uint32_t)mid, n_keys, 1));
    TRY(many_sbox_dev(c, strided ? flat : w + sw, nbytes, LUTSET_DEC_MUL, vp));
    TRY(launch_gather(c, vp, 4, KeySets{nullptr, nullptr, 0}, mix, nbytes / 16, table_dec_mix()));
    TRY(many_sbox_dev(c, mix, nbytes, LUTSET_IDENTITY, strided ? flat : dw + sw));
    if (strided) TRY(launch_key_rows(c, dw + sw, ks, flat, mid * bw, 0, nullptr, 0, 0, (uint32_t)mid, n_keys, 1));
    return FHEAES_OK;
}

// FIPS-197 section 5.2 for Nk = 4 / 6 / 8 key words under the reference's rule (server.rs:107-155 is the Nk = 4 case): every new word is
// refreshed by an identity WoPBS; RotWord + SubWord + Rcon when i % Nk == 0, SubWord alone when Nk > 6 and i % Nk == 4; 4 (Nr + 1) words.
// n_keys keys at once, key [n_keys][4 Nk][8][kN+1] -> w [n_keys][Nr+1][16][8][kN+1]: word i of key j lives at j * (Nr+1) * 16 bytes, and every
// step works on word i of ALL keys -- one launch per word operation and one WoPBS over 4 n_keys bytes, whatever n_keys is.  The WoPBS
// work on contiguous words [n_keys][4]: ta (sums, RotWord), tb (SubWord results), tc (refreshed words, placed at their stride after;
// one key's word is written where it belongs).
static int key_expansion_dev(fheaes_ctx *c, const uint64_t *key, uint64_t *w, int nr, uint64_t n_keys)
{
    static const uint8_t RCON[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
    const uint64_t bw = 8ull * c->big1, ww = 4 * bw, ks = (uint64_t)(nr + 1) * 16 * bw;
    const int nk = nr - 6;                                                                          // FIPS-197 Fig. 4: Nr = Nk + 6
    const bool strided = n_keys > 1;
    TRY(ensure(c, c->ws_tmp_a, n_keys * ww * 8));
    TRY(ensure(c, c->ws_tmp_b, n_keys * ww * 8));
    if (strided) TRY(ensure(c, c->ws_tmp_c, n_keys * ww * 8));
    uint64_t *ta = (uint64_t *)c->ws_tmp_a.p, *tb = (uint64_t *)c->ws_tmp_b.p, *tc = (uint64_t *)c->ws_tmp_c.p;
    TRY(launch_key_rows(c, w, ks, key, (uint64_t)nk * ww, 0, nullptr, 0, 0, 4u * nk, n_keys, 1));      // server.rs:122-128
    for (int i = nk; i < 4 * (nr + 1); ++i) {                                                       // server.rs:131-155
        const uint64_t *prev = w + (uint64_t)(i - 1) * ww, *back = w + (uint64_t)(i - nk) * ww;
        if (i % nk == 0) {
            TRY(launch_key_rows(c, ta, ww, prev, ks, 1, nullptr, 0, 0, 4, n_keys, 1));              // fhe_rot_word
            TRY(many_sbox_dev(c, ta, 4 * n_keys, LUTSET_SBOX, tb));                                 // fhe_sub_word
            TRY(launch_key_rows(c, ta, ww, tb, ww, 0, back, ks, RCON[i / nk - 1], 4, n_keys, 2));   // + Rcon (trivial) + w[i - Nk]
        } else if (nk > 6 && i % nk == 4) {                                                         // FIPS-197 5.2: SubWord alone (Nk = 8)
            if (strided) TRY(launch_key_rows(c, ta, ww, prev, ks, 0, nullptr, 0, 0, 4, n_keys, 1));
            TRY(many_sbox_dev(c, strided ? ta : prev, 4 * n_keys, LUTSET_SBOX, tb));
            TRY(launch_key_rows(c, ta, ww, tb, ww, 0, back, ks, 0, 4, n_keys, 2));
        } else {
            TRY(launch_key_rows(c, ta, ww, prev, ks, 0, back, ks, 0, 4, n_keys, 2));
        }
        uint64_t *fresh = w + (uint64_t)i * ww;
        TRY(many_sbox_dev(c, ta, 4 * n_keys, LUTSET_IDENTITY, strided ? tc : fresh));               // refresh, server.rs:150
        if (strided) TRY(launch_key_rows(c, fresh, ks, tc, ww, 0, nullptr, 0, 0, 4, n_keys, 1));
    }
    return FHEAES_OK;
}

// Host bytes that a device call needs go through the context's pinned buffer, so that the call only ENQUEUES (fheaes.h: FHEAES_DEVICE
// calls are not synchronised): `fill` writes `bytes` bytes into it and they are copied to the front of ws_misc (grown to ws_bytes).
// The only wait is for the copy out of that buffer that an earlier call enqueued (pin_ev).
template <class Fill> static int upload_pinned(fheaes_ctx *c, size_t bytes, size_t ws_bytes, Fill fill)
{
    if (c->pin_ev) HIP_TRY(c, hipEventSynchronize(c->pin_ev));
    else HIP_TRY(c, hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming));
    if (c->pin_bytes < bytes) {
        if (c->pin) { HIP_TRY(c, hipHostFree(c->pin)); c->pin = nullptr; c->pin_bytes = 0; }
        HIP_TRY(c, hipHostMalloc((void **)&c->pin, bytes, hipHostMallocDefault));
        c->pin_bytes = bytes;
    }
    fill(c->pin);
    TRY(ensure(c, c->ws_misc, ws_bytes));
    HIP_TRY(c, hipMemcpyAsync(c->ws_misc.p, c->pin, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->pin_ev, c->stream));
    return FHEAES_OK;
}

static int add_scalar_dev(fheaes_ctx *c, uint64_t *state, uint64_t n_blocks, const uint64_t *counters)
{
    const uint32_t lw = c->big1;
    // counter bytes, MSB first (server.rs:174-178): addend[byte][blk], in front of the carries in ws_misc
    TRY(upload_pinned(c, 16 * n_blocks, 16 * n_blocks + n_blocks * lw * 8 + 64, [&](uint8_t *add) {
        for (uint64_t b = 0; b < n_blocks; ++b) {
            uint64_t hi = counters[2 * b], lo = counters[2 * b + 1];
            for (int j = 0; j < 8; ++j) { add[(15 - j) * n_blocks + b] = (uint8_t)(lo >> (8 * j)); add[(7 - j) * n_blocks + b] = (uint8_t)(hi >> (8 * j)); }
        }
    }));
    uint8_t *add_d = (uint8_t *)c->ws_misc.p;
    uint64_t *carry = (uint64_t *)((uint8_t *)c->ws_misc.p + ((16 * n_blocks + 63) / 64) * 64);
    TRY(ensure(c, c->ws_tmp_a, n_blocks * 9ull * lw * 8));
    TRY(ensure(c, c->ws_tmp_b, n_blocks * 2ull * 9 * lw * 8));
    TRY(ensure(c, c->ws_luts, n_blocks * 2ull * 9 * FHE_N * 8));
    uint64_t *in9 = (uint64_t *)c->ws_tmp_a.p, *res = (uint64_t *)c->ws_tmp_b.p, *luts = (uint64_t *)c->ws_luts.p;
    for (int byte = 15; byte >= 0; --byte) {
        const uint32_t bits = byte == 15 ? 8 : 9;
        dim3 g1((bits * lw + 255) / 256, (unsigned)n_blocks);
        hipLaunchKernelGGL(pack9_kernel, g1, dim3(256), 0, c->stream, (const uint64_t *)state, (const uint64_t *)carry, in9, (uint32_t)byte, lw, n_blocks, bits);
        hipLaunchKernelGGL(counter_lut_kernel, dim3((2 * bits * FHE_N + 255) / 256, (unsigned)n_blocks), dim3(256), 0, c->stream, luts,
                           (const uint8_t *)(add_d + (size_t)byte * n_blocks), bits, n_blocks);
        HIP_TRY(c, hipGetLastError());
        TRY(wopbs_dev(c, in9, n_blocks, bits, luts, 2, 1, res));
        hipLaunchKernelGGL(unpack_sum_carry_kernel, dim3((9 * lw + 255) / 256, (unsigned)n_blocks), dim3(256), 0, c->stream, (const uint64_t *)res, bits, state, carry,
                           (uint32_t)byte, lw, n_blocks);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// ---- public blocks and CTR with a public nonce ------------------------------------------------
// aes_encrypt -- or the equivalent inverse cipher, PublicDirection below; the rule is written out for encryption -- on PUBLIC blocks
// (trivial ciphertexts) with every distinct S-Box input of the batch evaluated once.  A WoPBS is a deterministic function of its input words, so two state bytes with word-equal inputs need one evaluation.  The rule that finds them
// is exact and runs on the host before anything is enqueued: every S-Box input gets an id, round by round,
//   round 1:   id(b, p) = (key of b, p, byte p of block b)            -- the input is rk[key][0][p] + trivial(byte)
//   round r+1: id(b, p) = (p, id_r(b, s_0), .., id_r(b, s_3))         -- s_j: the four sources of table_enc_round() for position p
// and equal tuples are one id: sums of word-equal ciphertexts plus the same round-key byte are word-equal (the sources of an id all belong
// to one block, so an id has one AES key: equal blocks under different keys are never shared).  The ids of a round are its
// POOL; round r runs one WoPBS over pool r and an indexed gather (kern_linear.h) into pool r+1, the last gather writes [block][16].
struct PublicPlan {
    struct Layer { size_t head, term; uint32_t n, terms; };     // offsets into `words`; n outputs of `terms` terms each
    std::vector<Layer> layers;      // [0]: pool of round 1 (no terms), [r]: pool of round r+1 (4 terms), [Nr]: the state, 16 n_blocks bytes (1 term)
    std::vector<uint32_t> words;    // every layer's PUBLIC_HEAD words, then its PUBLIC_TERM words: one upload per call
    uint64_t max_vp_bytes_per_bw = 0;                            // max over the rounds of pool size x LUTs of that round's set
};

static inline uint32_t u128_byte(const uint64_t *hi_lo, int p) { return (uint32_t)((p < 8 ? hi_lo[0] >> (8 * (7 - p)) : hi_lo[1] >> (8 * (15 - p))) & 0xFF); }

struct PublicKey5 {
    uint32_t v[5];
    bool operator==(const PublicKey5 &o) const { return !memcmp(v, o.v, sizeof v); }
};
struct PublicKey5Hash {
    size_t operator()(const PublicKey5 &k) const
    {
        uint64_t h = 0xCBF29CE484222325ull;
        for (uint32_t x : k.v) { h ^= x; h *= 0x100000001B3ull; }
        return (size_t)(h ^ (h >> 29));
    }
};

// Which cipher the public blocks go through: the round gather and the last layer's, the LUT set and LUT count of the rounds and of the
// last round, and which round key layer r = 0..Nr adds.  The rule above holds for either direction, with the direction's sources in
// place of table_enc_round()'s and its first round key in place of rk[key][0].
struct PublicDirection {
    GatherTable round, last;
    int round_set, last_set;
    uint32_t round_luts, last_luts;
    bool keys_descend;                                          // layer r adds round key Nr - r, not r
    uint64_t key_round(int layer, int nr) const { return (uint64_t)(keys_descend ? nr - layer : layer); }
};

// aes_encrypt_schedule on pools
static PublicDirection public_forward() { return {table_enc_round(), table_shift_rows(false), LUTSET_ENC_ROUND, LUTSET_SBOX, 3, 1, false}; }
// aes_decrypt_eq_schedule on pools: rk is a set of decryption round keys dw, the pool of round 1 is dw[Nr][key][p] + trivial(byte), pool
// r + 1 sums the four {9, 11, 13, 14} InvS outputs of table_dec_eq_round() plus dw[Nr - r] (5 terms for the noise guard, as
// aes_decrypt_equivalent), the last layer is InvS through InvShiftRows plus dw[0] (plus CBC's clear chaining block)
static PublicDirection public_inverse() { return {table_dec_eq_round(), table_shift_rows(true), LUTSET_DEC_EQ_ROUND, LUTSET_INV_SBOX, 4, 1, true}; }

// blocks / data: n_blocks (hi, lo) pairs, data may be null; key_of_block: n_blocks key indices below PUBLIC_MAX_KEYS, or null (all 0)
static void public_plan(const PublicDirection &dir, const uint64_t *blocks, const uint64_t *data, const uint32_t *key_of_block, uint64_t n_blocks, int nr,
                        PublicPlan &pl)
{
    auto key_of = [&](uint64_t b) { return key_of_block ? key_of_block[b] : 0u; };
    const GatherTable &t_round = dir.round, &t_shift = dir.last;
    const uint64_t nbytes = 16 * n_blocks;
    std::vector<uint32_t> id(nbytes), next(nbytes);
    pl.layers.clear(); pl.words.clear();
    pl.layers.reserve((size_t)nr + 1);
    {   // round 1
        std::unordered_map<uint32_t, uint32_t> seen;              // the head word IS (key, p, byte)
        std::vector<uint32_t> head;
        for (uint64_t b = 0; b < n_blocks; ++b) for (int p = 0; p < 16; ++p) {
            const uint32_t h = PUBLIC_HEAD(p, u128_byte(blocks + 2 * b, p), key_of(b));
            auto ins = seen.emplace(h, (uint32_t)head.size());
            if (ins.second) head.push_back(h);
            id[16 * b + p] = ins.first->second;
        }
        pl.layers.push_back({0, head.size(), (uint32_t)head.size(), 0});
        pl.words = std::move(head);
    }
    for (int r = 1; r < nr; ++r) {   // pool of round r + 1 from the ids of round r
        std::unordered_map<PublicKey5, uint32_t, PublicKey5Hash> seen;
        seen.reserve(nbytes);
        std::vector<uint32_t> head, term;
        for (uint64_t b = 0; b < n_blocks; ++b) for (int p = 0; p < 16; ++p) {
            PublicKey5 k{{(uint32_t)p, 0, 0, 0, 0}};
            for (int j = 0; j < 4; ++j) k.v[1 + j] = id[16 * b + t_round.src[p][j]];
            auto ins = seen.emplace(k, (uint32_t)head.size());
            if (ins.second) {
                head.push_back(PUBLIC_HEAD(p, 0, key_of(b)));
                for (int j = 0; j < 4; ++j) term.push_back(PUBLIC_TERM(k.v[1 + j], t_round.lut[p][j]));
            }
            next[16 * b + p] = ins.first->second;
        }
        id.swap(next);
        const size_t h0 = pl.words.size();
        pl.layers.push_back({h0, h0 + head.size(), (uint32_t)head.size(), 4});
        pl.words.insert(pl.words.end(), head.begin(), head.end());
        pl.words.insert(pl.words.end(), term.begin(), term.end());
    }
    {   // ShiftRows + the last round key (+ CTR's clear data) into [block][16]
        const size_t h0 = pl.words.size();
        pl.layers.push_back({h0, h0 + nbytes, (uint32_t)nbytes, 1});
        pl.words.resize(h0 + 2 * nbytes);
        for (uint64_t b = 0; b < n_blocks; ++b) for (int p = 0; p < 16; ++p) {
            pl.words[h0 + 16 * b + p] = PUBLIC_HEAD(p, data ? u128_byte(data + 2 * b, p) : 0, key_of(b));
            pl.words[h0 + nbytes + 16 * b + p] = PUBLIC_TERM(id[16 * b + t_shift.src[p][0]], 0);
        }
    }
    pl.max_vp_bytes_per_bw = 0;
    for (int r = 1; r <= nr; ++r) pl.max_vp_bytes_per_bw = std::max<uint64_t>(pl.max_vp_bytes_per_bw, (uint64_t)pl.layers[r - 1].n * (r < nr ? dir.round_luts : dir.last_luts));
}

static_assert(FHEAES_MAX_KEYS == PUBLIC_MAX_KEYS, "fheaes.h's bound on n_keys is the key field of PUBLIC_HEAD");
#define PUBLIC_MAX_BLOCKS (1ull << 26)      /* 16 n pool entries x 4 must fit a PUBLIC_TERM word */

// terms == 0 (the pool of round 1): pool and term are not read, and the layer declares level 1 -- a trivial ciphertext carries no noise
static int launch_gather_indexed(fheaes_ctx *c, const uint64_t *pool, uint32_t n_luts, const uint32_t *head, const uint32_t *term, uint32_t terms,
                                 const KeySets &rk, uint64_t *out, uint64_t n_out)
{
    TRY(noise_guard(c, terms + 1u, terms ? "the indexed linear layer (MixColumns / ShiftRows + AddRoundKey over a pool)" : "the initial AddRoundKey on public bytes"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, (n_out + 15) / 16);
    dim3 grid((8 * c->big1 + 1023) / 1024, (unsigned)std::min<uint64_t>(n_out, 65535));
    with_keys(c, rk, [&](auto keys) {
        hipLaunchKernelGGL(gather_add_indexed_kernel<decltype(keys)>, grid, dim3(256), 0, c->stream, pool, n_luts, head, term, terms, keys, out, n_out, c->big1);
    });
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// `out` [n_blocks][16][8][kN+1] doubles as the pool buffer: no pool has more than 16 n_blocks entries.  rk: the call's sets of round keys
// ([n_keys][Nr+1][16][8][kN+1] or a packed store); the key of every pool entry is in its head word, so rk.of_block is not read
static int aes_public_dev(fheaes_ctx *c, const PublicDirection &dir, const KeySets &rk, const PublicPlan &pl, int nr, uint64_t *out)
{
    const uint64_t bw = 8ull * c->big1, sw = 16 * bw;
    // the index tables go through the context's pinned buffer (as add_scalar's counter bytes): the call only enqueues
    const size_t tab_bytes = pl.words.size() * sizeof(uint32_t);
    TRY(upload_pinned(c, tab_bytes, tab_bytes, [&](uint8_t *pin) { memcpy(pin, pl.words.data(), tab_bytes); }));
    const uint32_t *tab = (const uint32_t *)c->ws_misc.p;
    TRY(ensure(c, c->ws_vp, pl.max_vp_bytes_per_bw * bw * 8));               // the largest pool, not 16 n
    uint64_t *vp = (uint64_t *)c->ws_vp.p;
    for (int round = 0; round <= nr; ++round) {                              // layer 0 is the pool of round 1: nothing to evaluate before it
        const PublicPlan::Layer &to = pl.layers[round];
        if (round > 0) TRY(many_sbox_dev(c, out, pl.layers[round - 1].n, round < nr ? dir.round_set : dir.last_set, vp));
        TRY(launch_gather_indexed(c, vp, round < nr ? dir.round_luts : dir.last_luts, tab + to.head, tab + to.term, to.terms, rk.round(dir.key_round(round, nr), sw), out, to.n));
    }
    return FHEAES_OK;
}

// ---- XTS-AES decryption (IEEE 1619, SP 800-38E) -------------------------------------------------
// P_j = D_K1(C_j ^ T_j) ^ T_j, T_j = E_K2(tweak) * alpha^j: the first mode here whose per-block mask is ENCRYPTED, so the public path does
// not apply to the blocks -- only to the tweak blocks.  Levels against the guard's 5: E_K2(tweak) leaves the public call at 2 (S-Box output +
// round key) and an identity WoPBS makes it 1: the ANCHOR of a data unit.  One gather (bit_rows_kernel<XtsRows>) gives T_j at up to 4 terms; used
// raw on both sides of the cipher it would pass going in (4 + dw[Nr] = 5) but not coming out (InvS + dw[0] + 4 = 6), so every T_j is
// refreshed by an identity WoPBS: 2 going in, 3 coming out.  A gather reaches offset 121, so a unit is cut into segments of XTS_SEGMENT
// blocks: segment s gathers offsets 0 .. 120 from anchor s, and the refreshed offset 120 -- block 120 (s + 1)'s place, computed for this
// alone -- is anchor s + 1.  Block j of a unit takes offset j % 120 of segment j / 120.
#define XTS_SEGMENT 120u
#define XTS_MAX_BLOCKS_PER_UNIT (1u << 20)      /* IEEE 1619 5.1: a data unit has at most 2^20 blocks */

// The units a call touches fall into at most three classes of consecutive units with the same blocks [a, e): the first, the whole ones
// between, the last.  Per segment every class is one gather, the classes' outputs lie one behind the other, and one WoPBS refreshes them.
struct XtsGather { uint64_t unit0, units; uint32_t off0, n_off; uint64_t row0; int64_t anchor_row; uint64_t anchor_stride_rows; };   // rows: tweak blocks
struct XtsPlan {
    uint64_t unit0 = 0, units = 0;                      // the units the call touches: unit0 .. unit0 + units - 1
    std::vector<std::vector<XtsGather>> segments;       // anchor_row < 0: the anchor is row `unit0` of the anchors of segment 0
    std::vector<uint64_t> seg_row0, seg_rows;           // each segment's rows in the buffer of refreshed tweaks
    uint64_t rows = 0;
    std::vector<uint32_t> tweak_of_block;               // the row of every block of the call (want_table)
};

static bool xts_plan(uint64_t n_units, uint64_t bpu, uint64_t first_block, uint64_t n_blocks, bool want_table, XtsPlan &pl)
{
    if (bpu == 0 || bpu > XTS_MAX_BLOCKS_PER_UNIT || first_block + n_blocks < first_block) return false;
    if (n_blocks == 0) return true;
    const uint64_t last = first_block + n_blocks - 1, u0 = first_block / bpu, u1 = last / bpu;
    if (u1 >= n_units) return false;
    pl.unit0 = u0; pl.units = u1 - u0 + 1;
    struct Class { uint64_t unit0, units, a, e; };      // unit0 counted from the first touched unit
    std::vector<Class> cls;
    auto add = [&](uint64_t unit0, uint64_t units, uint64_t a, uint64_t e) {
        if (units == 0) return;
        if (!cls.empty() && cls.back().a == a && cls.back().e == e) cls.back().units += units;      // a whole first or last unit joins the ones between
        else cls.push_back({unit0, units, a, e});
    };
    add(0, 1, first_block % bpu, u1 == u0 ? last % bpu + 1 : bpu);
    if (u1 > u0) { add(1, u1 - u0 - 1, 0, bpu); add(u1 - u0, 1, 0, last % bpu + 1); }
    std::vector<uint64_t> prev_row0(cls.size(), 0);
    std::vector<uint32_t> prev_lo(cls.size(), 0), prev_n(cls.size(), 0);
    struct Place { uint64_t row0; uint32_t lo, n; };      // [class][segment]: where the class's tweaks of that segment start, and which offsets they are
    std::vector<std::vector<Place>> place(cls.size());
    for (uint64_t s = 0;; ++s) {
        std::vector<XtsGather> gs;
        const uint64_t seg0 = pl.rows;
        for (size_t k = 0; k < cls.size(); ++k) {
            const Class &q = cls[k];
            const uint64_t segs = (q.e - 1) / XTS_SEGMENT + 1, sa = q.a / XTS_SEGMENT;
            if (s >= segs) continue;
            const uint32_t lo = s < sa ? XTS_SEGMENT : s == sa ? (uint32_t)(q.a % XTS_SEGMENT) : 0;
            const uint32_t hi = s + 1 < segs ? XTS_SEGMENT : (uint32_t)((q.e - 1) % XTS_SEGMENT);
            XtsGather g{q.unit0, q.units, lo, hi - lo + 1, pl.rows, -1, 1};
            if (s > 0) { g.anchor_row = (int64_t)(prev_row0[k] + (XTS_SEGMENT - prev_lo[k])); g.anchor_stride_rows = prev_n[k]; }
            prev_row0[k] = g.row0; prev_lo[k] = lo; prev_n[k] = g.n_off;
            place[k].push_back({g.row0, lo, g.n_off});
            pl.rows += g.units * g.n_off;
            gs.push_back(g);
        }
        if (gs.empty()) break;
        pl.seg_row0.push_back(seg0); pl.seg_rows.push_back(pl.rows - seg0);
        pl.segments.push_back(std::move(gs));
    }
    if (pl.rows > 0xFFFFFFFFull) return false;
    if (want_table) {
        pl.tweak_of_block.resize(n_blocks);
        for (uint64_t b = 0; b < n_blocks; ++b) {
            const uint64_t g = first_block + b, u = g / bpu - u0, j = g % bpu;
            size_t k = 0;
            while (u >= cls[k].unit0 + cls[k].units) ++k;
            const Place &at = place[k][j / XTS_SEGMENT];
            pl.tweak_of_block[b] = (uint32_t)(at.row0 + (u - cls[k].unit0) * at.n + (j % XTS_SEGMENT - at.lo));
        }
    }
    return true;
}

// rk2: the expanded key 2 (the tweak key, forward cipher on the public tweak blocks); dw1: the decryption round keys of key 1.
// tweaks: the (hi, lo) pairs of units 0 .. ; ct: the n_blocks ciphertext blocks; out [n_blocks][16][8][kN+1].  Workspace: ws_tmp_a the
// raw tweaks of one segment (and E_K2(tweak) first), ws_tmp_b the refreshed tweaks of the call, ws_tmp_c the anchors of segment 0.
static int aes_xts_decrypt_dev(fheaes_ctx *c, const KeySets &dw1, const KeySets &rk2, int nr, const uint64_t *tweaks, const XtsPlan &pl, const uint64_t *ct,
                               uint64_t n_blocks, uint64_t *out)
{
    const uint64_t tw = AES_BLOCK_BITS * c->big1;                           // words of one tweak block == of one state
    uint64_t raw_rows = pl.units;
    for (uint64_t r : pl.seg_rows) raw_rows = std::max(raw_rows, r);
    TRY(ensure(c, c->ws_tmp_a, raw_rows * tw * 8));
    TRY(ensure(c, c->ws_tmp_b, pl.rows * tw * 8));
    TRY(ensure(c, c->ws_tmp_c, pl.units * tw * 8));
    uint64_t *raw = (uint64_t *)c->ws_tmp_a.p, *fresh = (uint64_t *)c->ws_tmp_b.p, *anchor0 = (uint64_t *)c->ws_tmp_c.p;
    {   // E_K2(tweak) of the touched units, equal tweaks shared by the public rule; refreshed: the anchors of segment 0
        PublicPlan pp;
        public_plan(public_forward(), tweaks + 2 * pl.unit0, nullptr, nullptr, pl.units, nr, pp);
        TRY(aes_public_dev(c, public_forward(), rk2, pp, nr, raw));
        TRY(many_sbox_dev(c, raw, 16 * pl.units, LUTSET_IDENTITY, anchor0));
    }
    for (size_t s = 0; s < pl.segments.size(); ++s) {
        for (const XtsGather &g : pl.segments[s]) {
            const uint64_t *anchor = g.anchor_row < 0 ? anchor0 + g.unit0 * tw : fresh + (uint64_t)g.anchor_row * tw;
            TRY(launch_xts_tweaks(c, anchor, g.anchor_stride_rows * tw, g.units, g.off0, g.n_off, raw + (g.row0 - pl.seg_row0[s]) * tw));
        }
        TRY(many_sbox_dev(c, raw, 16 * pl.seg_rows[s], LUTSET_IDENTITY, fresh + pl.seg_row0[s] * tw));
    }
    // the table of tweak rows and the clear ciphertext bytes, through the pinned buffer (after the public call's tables: same stream)
    const size_t tab_bytes = n_blocks * sizeof(uint32_t), all_bytes = tab_bytes + 16 * n_blocks;
    TRY(upload_pinned(c, all_bytes, all_bytes, [&](uint8_t *pin) {
        memcpy(pin, pl.tweak_of_block.data(), tab_bytes);
        for (uint64_t b = 0; b < n_blocks; ++b) for (int p = 0; p < 16; ++p) pin[tab_bytes + 16 * b + p] = (uint8_t)u128_byte(ct + 2 * b, p);
    }));
    const uint32_t *tab = (const uint32_t *)c->ws_misc.p;
    const uint8_t *clear = (const uint8_t *)c->ws_misc.p + tab_bytes;
    TRY(launch_xts_whiten(c, out, nullptr, fresh, tab, clear, n_blocks, 1));                // trivial(C) + T: one nominal term; + dw[Nr] = 2 in the cipher
    TRY(aes_run_dev(c, dw1, out, n_blocks, aes_decrypt_eq_schedule(nr)));
    TRY(launch_xts_whiten(c, out, out, fresh, tab, nullptr, n_blocks, 3));                  // InvS output + dw[0] + T
    return FHEAES_OK;
}

// ---- CBC-MAC chains over many streams, and CCM decryption with its tag check (SP 800-38C, RFC 3610) ----------------------------------
// X_{i+1} = E_K(X_i ^ B_i) is serial inside a stream and parallel across streams, and every block has its own key (KeySets.of_block), so
// step i of ALL live streams is one ordinary windowed cipher pass.  The host sorts the streams by chain length, descending and stable: the
// live set of step i is the prefix [0, n_active(i)) of one state array [n_streams][128][kN+1] and nothing is compacted.  Between two
// passes one mac_link_kernel launch adds the step's blocks -- clear bytes as trivial ciphertexts, and encrypted addends byte-exact (a partial
// last block adds its real bytes only).  Levels against the guard's 5: a cipher or public-call output is 2; a link of public blocks goes
// into AddRoundKey at 2 + 1 = 3, a link of encrypted addends at X (2) + P (2) + round key = 5, the figure aes_decrypt_eq_schedule runs at;
// a caller's addend or init counts as 2.
#define MAC_MAX_STREAMS FHEAES_MAC_MAX_STREAMS
#define MAC_MAX_STREAM_BLOCKS FHEAES_MAC_MAX_STREAM_BLOCKS
static_assert(MAC_NONE == FHEAES_MAC_NONE && sizeof(MacSlot) == 32, "fheaes.h's 'none' is the kernel's, and a link record is 32 bytes");

struct MacPlan {
    std::vector<uint32_t> order, slot_of;       // sorted slot -> stream of the call, and back
    std::vector<uint64_t> n_active;             // per chain step: the streams still running (a prefix of the slots)
    uint64_t chained = 0;                       // cipher blocks of the whole chain: the sum of n_active
};

static void mac_plan(const uint32_t *len, uint64_t n, MacPlan &pl)
{
    pl.order.resize(n); pl.slot_of.resize(n);
    for (uint64_t s = 0; s < n; ++s) pl.order[s] = (uint32_t)s;
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](uint32_t x, uint32_t y) { return len[x] > len[y]; });
    for (uint64_t j = 0; j < n; ++j) pl.slot_of[pl.order[j]] = (uint32_t)j;
    const uint32_t steps = n ? len[pl.order[0]] : 0;
    pl.n_active.assign(steps, 0);
    pl.chained = 0;
    uint64_t live = n;
    for (uint32_t i = 0; i < steps; ++i) {
        while (live && len[pl.order[live - 1]] <= i) --live;
        pl.n_active[i] = live;
        pl.chained += live;
    }
}

// What a chain uploads and runs: the key of every sorted slot, the link records of every step one behind the other (and behind them
// whatever records the caller runs after the chain), and per step where its records start, how many slots it links and encrypts, and
// the level it declares.  Step 0 links ALL slots from where the chain starts (a stream of length 0 keeps its start: it is copied, not
// skipped); the later steps link their live prefix in place.
struct MacChain {
    std::vector<uint32_t> key_of_slot;
    std::vector<MacSlot> slots;
    struct Step { size_t first; uint64_t n_link, n_active; uint32_t level; };
    std::vector<Step> steps;
};

static MacSlot mac_slot(uint32_t a, uint32_t b, uint32_t b_bytes, uint32_t out_bytes, const uint8_t *clear, uint32_t clear_bytes = 16)
{
    MacSlot r{a, b_bytes ? b : MAC_NONE, b_bytes, out_bytes, {}};
    if (clear) memcpy(r.clear, clear, clear_bytes);
    return r;
}

// stream s chains len[s] blocks: block i adds `clear` (16 bytes) and, where `enc` is given, the first enc_bytes bytes of block enc of the
// addend buffer; block(s, i, clear16, &enc, &enc_bytes) says which.  start(s): the block of the start buffer stream s begins from, or
// MAC_NONE (a zero state).
template <class Block, class Start>
static void mac_chain(const MacPlan &pl, const uint32_t *len, const uint32_t *key_of_stream, uint64_t n, Block block, Start start, MacChain &ch)
{
    ch.key_of_slot.resize(n);
    for (uint64_t j = 0; j < n; ++j) ch.key_of_slot[j] = key_of_stream[pl.order[j]];
    const size_t steps = std::max<size_t>(pl.n_active.size(), n ? 1 : 0);
    for (size_t i = 0; i < steps; ++i) {
        const uint64_t n_active = i < pl.n_active.size() ? pl.n_active[i] : 0, n_link = i == 0 ? n : n_active;
        bool any_a = i > 0, any_b = false;
        const size_t first = ch.slots.size();
        for (uint64_t j = 0; j < n_link; ++j) {
            const uint32_t s = pl.order[j], a = i == 0 ? start(s) : (uint32_t)j;
            uint8_t clear[16] = {};
            uint32_t enc = MAC_NONE, enc_bytes = 0;
            if (len[s] > i) block(s, (uint32_t)i, clear, &enc, &enc_bytes);
            if (enc == MAC_NONE) enc_bytes = 0;
            any_a = any_a || a != MAC_NONE;
            any_b = any_b || enc_bytes;
            ch.slots.push_back(mac_slot(a, enc, enc_bytes, 16, clear));
        }
        ch.steps.push_back({first, n_link, n_active, (any_a ? 2u : 0u) + (any_b ? 2u : 0u) + 1u});
    }
}

// Runs the chain over `state` [n_streams][128][kN+1] (sorted slots): start / enc are the buffers the records' a (step 0) and b index.
// One upload for the whole call through the pinned buffer (FHEAES_DEVICE calls only enqueue); *recs: the records on the device.
static int cbc_mac_dev(fheaes_ctx *c, const KeySets &rk, int nr, uint64_t n_keys, const MacChain &ch, const uint64_t *start, const uint64_t *enc, uint64_t *state,
                       const MacSlot **recs)
{
    const size_t key_bytes = (ch.key_of_slot.size() * sizeof(uint32_t) + 31) / 32 * 32, rec_bytes = ch.slots.size() * sizeof(MacSlot);
    TRY(upload_pinned(c, key_bytes + rec_bytes, key_bytes + rec_bytes, [&](uint8_t *pin) {
        memcpy(pin, ch.key_of_slot.data(), ch.key_of_slot.size() * sizeof(uint32_t));
        memcpy(pin + key_bytes, ch.slots.data(), rec_bytes);
    }));
    *recs = (const MacSlot *)((const uint8_t *)c->ws_misc.p + key_bytes);
    KeySets keys = rk;
    keys.of_block = n_keys > 1 ? (const uint32_t *)c->ws_misc.p : nullptr;
    const AesSchedule sch = aes_encrypt_schedule(nr);
    for (size_t i = 0; i < ch.steps.size(); ++i) {
        const MacChain::Step &st = ch.steps[i];
        TRY(launch_mac_link(c, state, i == 0 ? start : state, enc, *recs + st.first, st.n_link, st.level, "a CBC-MAC link (chaining value + block + the round key that follows)"));
        if (st.n_active) TRY(aes_run_dev(c, keys, state, st.n_active, sch));
    }
    return FHEAES_OK;
}

// A CCM call on the host: the public batch is [the payload counters Ctr_1.. of every stream, stream after stream | B0 of every stream |
// Ctr_0 of every stream] with data [C_1.. | none | none], so its outputs are the plaintext blocks P, then X_1, then S0.  The chain of
// stream s runs from X_1 over its `aad` public blocks and then its payload blocks, whose addend is the encrypted P (the last one with its
// real bytes).  Behind the chain's records: n_streams tag records (the caller's order) and the payload records that bring P to the output.
struct CcmCall {
    uint64_t n = 0, payload_blocks = 0;
    std::vector<uint64_t> pub_blocks, pub_data;         // (hi, lo) pairs
    std::vector<uint32_t> pub_key, len;
    MacPlan plan;
    MacChain chain;
    size_t tag0 = 0, pt0 = 0;                           // where the tag and the payload records start
};

// The tag check of CCM and CMAC.  diff [n][128][kN+1] is zero on its first 8t rows iff the tag is right, and zero words from row 8t on;
// WoPBS 1 (8 bits, every byte of the 16) gives byte != 0, WoPBS 2 takes those 16 bits as one input and gives 1 on input 0.  valid_out
// [n][kN+1]: row 0 of the second WoPBS.  diff is overwritten (the bits of the second WoPBS); ws_vp (n states, the caller's) holds both outputs.
static int tag_check_dev(fheaes_ctx *c, uint64_t *diff, uint64_t n, uint64_t *valid_out)
{
    const uint64_t row = (uint64_t)c->big1 * 8;
    uint64_t *vp = (uint64_t *)c->ws_vp.p;
    TRY(wopbs_dev(c, diff, 16 * n, 8, c->lut_tag_d[0], 1, 0, vp));
    HIP_TRY(c, hipMemcpy2DAsync(diff, row, vp, 8 * row, row, 16 * n, hipMemcpyDeviceToDevice, c->stream));
    TRY(wopbs_dev(c, diff, n, 16, c->lut_tag_d[1], 1, 0, vp));
    HIP_TRY(c, hipMemcpy2DAsync(valid_out, row, vp, 16 * row, row, n, hipMemcpyDeviceToDevice, c->stream));
    return FHEAES_OK;
}

// ws_tmp_a: the public call's outputs; ws_tmp_b: the chain's state; ws_tmp_c: the tag difference, then the bits of the second WoPBS.
// diff = X_final + S0 + trivial(tag) on its first 8t rows (level 4), then tag_check_dev.
static int ccm_open_dev(fheaes_ctx *c, const KeySets &rk, int nr, uint64_t n_keys, const CcmCall &cc, const PublicPlan &pp, uint64_t *plaintext_out,
                        uint64_t *valid_out)
{
    const uint64_t sw = AES_BLOCK_BITS * c->big1, n = cc.n;
    TRY(ensure(c, c->ws_tmp_a, (cc.payload_blocks + 2 * n) * sw * 8));
    TRY(ensure(c, c->ws_tmp_b, n * sw * 8));
    TRY(ensure(c, c->ws_tmp_c, n * sw * 8));
    TRY(ensure(c, c->ws_vp, n * sw * 8));
    uint64_t *pub = (uint64_t *)c->ws_tmp_a.p, *state = (uint64_t *)c->ws_tmp_b.p, *diff = (uint64_t *)c->ws_tmp_c.p;
    TRY(aes_public_dev(c, public_forward(), rk, pp, nr, pub));
    const MacSlot *recs = nullptr;
    TRY(cbc_mac_dev(c, rk, nr, n_keys, cc.chain, pub, pub, state, &recs));
    TRY(launch_mac_link(c, diff, state, pub, recs + cc.tag0, n, 4, "the CCM tag difference (X + S0 + tag)"));
    TRY(launch_mac_link(c, plaintext_out, nullptr, pub, recs + cc.pt0, cc.payload_blocks, 2, "the CCM plaintext"));
    return tag_check_dev(c, diff, n, valid_out);
}

// ---- CMAC over many streams (SP 800-38B, RFC 4493) -----------------------------------------------------------------------------------------
// T = the CBC-MAC of the message whose last block also gets a subkey added: K1 = L x under a whole last block, K2 = L x^2 under a padded
// one, L = E_K(0^128).  Every block is public, so the chain above runs as it is with the subkey as the last block's encrypted addend: the
// records' b is 2 * key + which into the subkey array.  Levels against the guard's 5: L leaves the public call at 2, an identity WoPBS
// makes it 1; the gather (bit_rows_kernel<CmacRows>) gives K1 at 2 and K2 at 3; a second identity WoPBS makes both 1, counted -- as every
// addend of a chain -- as 2: the last link is X (2) + subkey (2) + round key = 5.  Without the second refresh it would be 2 + 3 + 1 = 6,
// and without the first K2 alone would be 2 * 3.  48 byte-WoPBS per key, against 16 Nr per chained block.

// The subkeys of keys key_of[0 .. m) of rk, out [m][2][16][8][kN+1].  Workspace: ws_tmp_a E_K(0) of the m keys,
// ws_tmp_c L, ws_tmp_b the raw subkeys -- ensured by the caller for m, m and 2m states; out may be ws_tmp_a.
static int cmac_subkeys_dev(fheaes_ctx *c, const KeySets &rk, int nr, const uint32_t *key_of, uint64_t m, uint64_t *out)
{
    uint64_t *enc0 = (uint64_t *)c->ws_tmp_a.p, *l = (uint64_t *)c->ws_tmp_c.p, *raw = (uint64_t *)c->ws_tmp_b.p;
    const std::vector<uint64_t> zero(2 * m, 0);
    PublicPlan pp;
    public_plan(public_forward(), zero.data(), nullptr, key_of, m, nr, pp);
    TRY(aes_public_dev(c, public_forward(), rk, pp, nr, enc0));
    TRY(many_sbox_dev(c, enc0, 16 * m, LUTSET_IDENTITY, l));
    TRY(launch_cmac_double(c, l, m, raw));
    TRY(many_sbox_dev(c, raw, 32 * m, LUTSET_IDENTITY, out));
    return FHEAES_OK;
}

// A CMAC call on the host: len[s] chain blocks per stream, the chain's records and, behind them, n records that bring the MACs to the
// caller's order (mac0; only where the call returns them) and n tag-difference records (tag0; only with tags).  used: the keys some
// stream names, ascending -- the subkeys a call without the caller's own derives, in this order.
struct CmacCall {
    uint64_t n = 0;
    std::vector<uint32_t> len, used;
    MacPlan plan;
    MacChain chain;
    size_t mac0 = 0, tag0 = 0;
};

// the chain blocks of a message of `bytes` bytes (SP 800-38B 6.2: the empty message is one padded block)
static uint64_t cmac_blocks(uint64_t bytes) { return bytes ? (bytes + 15) / 16 : 1; }

// subkeys: the caller's [n_keys][2][16][8][kN+1], or null: derived for cc.used into ws_tmp_a.  ws_tmp_b: the chain's state; ws_tmp_c: the
// tag difference.  diff = X + trivial(tag) on its first 8t rows (level 2), then tag_check_dev.  mac_out, valid_out: either may be null.
static int cmac_dev(fheaes_ctx *c, const KeySets &rk, int nr, uint64_t n_keys, const CmacCall &cc, const uint64_t *subkeys, uint64_t *mac_out, uint64_t *valid_out)
{
    const uint64_t sw = AES_BLOCK_BITS * c->big1, n = cc.n, m = subkeys ? 0 : cc.used.size();
    TRY(ensure(c, c->ws_tmp_a, 2 * m * sw * 8));
    TRY(ensure(c, c->ws_tmp_b, std::max(2 * m, n) * sw * 8));
    TRY(ensure(c, c->ws_tmp_c, std::max(m, n) * sw * 8));
    if (valid_out) TRY(ensure(c, c->ws_vp, n * sw * 8));
    if (!subkeys) {
        TRY(cmac_subkeys_dev(c, rk, nr, cc.used.data(), m, (uint64_t *)c->ws_tmp_a.p));
        subkeys = (const uint64_t *)c->ws_tmp_a.p;
    }
    uint64_t *state = (uint64_t *)c->ws_tmp_b.p, *diff = (uint64_t *)c->ws_tmp_c.p;
    const MacSlot *recs = nullptr;
    TRY(cbc_mac_dev(c, rk, nr, n_keys, cc.chain, nullptr, subkeys, state, &recs));
    if (mac_out) TRY(launch_mac_link(c, mac_out, state, nullptr, recs + cc.mac0, n, 2, "the CMACs in the caller's order"));
    if (!valid_out) return FHEAES_OK;
    TRY(launch_mac_link(c, diff, state, nullptr, recs + cc.tag0, n, 2, "the CMAC tag difference (T + tag)"));
    return tag_check_dev(c, diff, n, valid_out);
}

// ---- AES key unwrap over many keys (RFC 3394, SP 800-38F) ----------------------------------------------------------------------------------
// Wrapped keys are public data; the key-encryption keys (KEKs) are encrypted.  6n block decryptions per key, serial inside a key and
// parallel across keys -- the shape of the chains above, with every chain of the same length, so nothing is sorted or compacted: step s of
// ALL keys is one kw_link_kernel launch and one windowed pass of the equivalent inverse cipher, key j under KEK kek_of[j]
// (KeySets.of_block).  Levels against the guard's 5: a cipher output is 2, a step's input goes into AddRoundKey at 2 + 1 = 3; the raw key
// out of the last step is 2, and an identity WoPBS (the one XTS and CMAC use) makes it fresh, a valid argument of the key expansion, where
// the raw key words become round key 0 and count as 1; the tag difference goes into the first tag WoPBS at 2.

// wrapped: the device table [n_keys][8 (n + 1)]; dw: the KEKs' decryption round keys, of_block set where there is more than one.
// ws_tmp_a: the register file, ws_tmp_b: the state, ws_vp: the cipher's and the tag check's outputs -- all had before the first launch.
// keys_out [n_keys][8 n][8][kN+1], NOT gated on valid_out [n_keys][kN+1].
static int kw_unwrap_dev(fheaes_ctx *c, const KeySets &dw, int nr, const uint8_t *wrapped, uint32_t n, uint64_t n_keys, uint64_t *keys_out, uint64_t *valid_out)
{
    const uint64_t bw = 8ull * c->big1, sw = 16 * bw;
    const AesSchedule sch = aes_decrypt_eq_schedule(nr);
    const uint64_t w = aes_context_window(c, n_keys, sch.steps.size());
    TRY(ensure(c, c->ws_tmp_a, n_keys * 8 * n * bw * 8));
    TRY(ensure(c, c->ws_tmp_b, n_keys * sw * 8));
    TRY(ensure(c, c->ws_vp, std::max<uint64_t>((w ? w : n_keys) * 16 * sch.max_luts * bw * 8, n_keys * sw * 8)));
    uint64_t *regs = (uint64_t *)c->ws_tmp_a.p, *state = (uint64_t *)c->ws_tmp_b.p;
    for (uint32_t s = 0; s < 6 * n; ++s) {
        TRY(launch_kw_link(c, state, regs, wrapped, n_keys, n, s));
        TRY(aes_run_dev(c, dw, state, n_keys, sch));
    }
    TRY(launch_kw_link(c, state, regs, wrapped, n_keys, n, 6 * n));
    TRY(many_sbox_dev(c, regs, 8ull * n * n_keys, LUTSET_IDENTITY, keys_out));
    return tag_check_dev(c, state, n_keys, valid_out);
}
