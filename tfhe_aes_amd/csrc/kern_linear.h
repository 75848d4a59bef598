// kern_linear.h -- K6: the linear AES layers on LWE vectors (XOR == uint64 wrapping add of the
// 1-bit-at-the-MSB encodings) and the small data-movement kernels of the schedule.
//   mix_columns (+ShiftRows)  src/server/encrypt/mix_columns.rs:4-78
//   shift_rows                src/server/encrypt/shift_rows.rs:5-21
//   inv_mix_columns           src/server/decrypt/inv_mix_columns.rs:4-58
//   inv_shift_rows            src/server/decrypt/inv_shift_rows.rs:5-21
//   add_round_key             src/server/server.rs:278-282
//   (no counterpart)          the XTS tweak layer: multiplication by alpha^j in GF(2^128), bit_rows_kernel over XtsRows below
//   (no counterpart)          the CMAC subkeys: multiplication by x and x^2 in the big-endian byte order, bit_rows_kernel over CmacRows below
//   (no counterpart)          the key-unwrap link (RFC 3394): half blocks moved between a state and a register file, kw_link_kernel below
// All of them but the last are one "gather-add": out[blk][byte] = sum_t src[blk][tab.src[byte][t]][tab.lut[byte][t]] (+ rk[byte]).
// The round key comes from a source type (LweKeys, PackedKeys below): every layer that adds one is ONE kernel template over that type,
// so round keys in LWE form and in a packed store go through the same body.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct GatherTable {
    int32_t terms;          // 1..4
    int8_t src[16][4];      // source byte index inside the block
    int8_t lut[16][4];      // which LUT output of that byte
};

#define PACK_N 512           /* the polynomial size N the packing kernels and the packed key stores are written for */

// ---- sample extraction: the one rule ---------------------------------------------------------------------------------------------------
// The LWE of coefficient i of a GLWE (A_0 .. A_{k-1}, B): the blind rotation's extraction of coefficient 0, for any coefficient.
//   mask word jN + c = A_j[i - c] (c <= i), -A_j[i - c + N] (c > i); body = B[i]
// A GLWE is read through one of two readers: g[e] is its word e < (k+1) N.

// 64-bit words
struct GlweWords {
    const uint64_t *p;
    __device__ __forceinline__ GlweWords glwe(uint64_t g, uint32_t k) const { return {p + g * (k + 1) * PACK_N}; }
    __device__ __forceinline__ uint64_t operator[](uint32_t e) const { return p[e]; }
};

// field e of a switched GLWE (mod_switch_pack_kernel), read back: x' = v << (64 - w), from one or two words
__device__ __forceinline__ uint64_t mod_field(const uint64_t *glwe, uint32_t e, uint32_t w)
{
    const uint32_t bit = e * w, word = bit >> 6, off = bit & 63;
    uint64_t v = glwe[word] >> off;
    if (off + w > 64) v |= glwe[word + 1] << (64 - off);               // the field straddles two words (off > 0 here)
    return v << (64 - w);
}

// width-bit fields: a GLWE is (k+1) 8 width words
struct GlweFields {
    const uint64_t *p;
    uint32_t width;
    __device__ __forceinline__ GlweFields glwe(uint64_t g, uint32_t k) const { return {p + g * (k + 1) * 8 * width, width}; }
    __device__ __forceinline__ uint64_t operator[](uint32_t e) const { return mod_field(p, e, width); }
};

// word w (<= kN) of the LWE of coefficient i (< N) of `glwe`
template <class Glwe>
__device__ __forceinline__ uint64_t sample_extract_word(const Glwe &glwe, uint32_t i, uint32_t w, uint32_t k)
{
    const uint32_t big = k * PACK_N;
    if (w == big) return glwe[big + i];
    const uint32_t c = w & (PACK_N - 1);
    const uint64_t v = glwe[(w - c) + ((i - c) & (PACK_N - 1))];
    return c <= i ? v : (uint64_t)0 - v;
}

// ---- where a linear layer reads its round key ---------------------------------------------------------------------------------------------
// Two by-value sources with the same two members: key(j), the source at key j of a block or pool entry, and word(p, w, lwe_words), word w
// of state byte p of that key's round key ([16][8][lwe_words]; word(0, i, ..) for i < 128 lwe_words is word i of the whole round key).
// The kernels below are templates over the source.  All offsets in 64 bits: key 65,535 of a packed AES-128 store at k = 4 starts at
// byte 4,026,470,400 (past 2^31; AES-192 / 256 stores pass 2^32), and sets in LWE form are 2.9 MB apart and more.

// LWE form: `base` is the round in question of key 0, [16][8][lwe_words]; key j's `stride` words further.  base null: no round key
struct LweKeys {
    const uint64_t *base;
    uint64_t stride;
    __device__ __forceinline__ bool none() const { return base == nullptr; }
    __device__ __forceinline__ LweKeys key(uint64_t j) const { return {base + j * stride, stride}; }
    __device__ __forceinline__ uint64_t word(uint32_t p, uint32_t w, uint32_t lwe_words) const { return base[(uint64_t)p * 8 * lwe_words + w]; }
};

// A packed store (fheaes_pack_round_keys) holds key j as G = ceil((Nr+1) 128 / N) GLWEs at j * key_words words, key_words = G (k+1) N:
// fheaes_pack_bits of the key's round keys flattened, so bit t = round * 128 + byte * 8 + bit sits in GLWE t / N, coefficient t % N, and
// bit0 = round * 128.  Word w of the LWE of bit t is sample_extract_kernel's word, taken at the moment AddRoundKey needs it.  Consecutive
// lanes take consecutive w, so the state and WoPBS-output streams stay forward; the key read alone runs backwards through one polynomial
// (a wave reads one contiguous run, two where it wraps).
struct PackedKeys {
    const uint64_t *store;
    uint64_t key_words;
    uint32_t bit0, k;
    __device__ __forceinline__ bool none() const { return false; }
    __device__ __forceinline__ PackedKeys key(uint64_t j) const { return {store + j * key_words, key_words, bit0, k}; }
    __device__ __forceinline__ uint64_t word(uint32_t p, uint32_t w, uint32_t lwe_words) const
    {
        const uint32_t bit = w / lwe_words, t = bit0 + p * 8 + bit;
        return sample_extract_word(GlweWords{store}.glwe(t / PACK_N, k), t & (PACK_N - 1), w - bit * lwe_words, k);
    }
};

// src: [n_blocks][16][n_luts][byte_words], byte_words = 8 lwe_words; keys: the round key to add, or none; key_of_block: [n_blocks] or null
// (every block under the first key); out: [n_blocks][16][byte_words]
template <class Keys>
__global__ __launch_bounds__(256) void gather_add_kernel(const uint64_t *src, uint32_t n_luts, const Keys keys, const uint32_t *key_of_block, uint64_t *out,
                                                         uint64_t n_blocks, uint32_t lwe_words, const GatherTable tab)
{
    const uint64_t blk = blockIdx.z;
    const uint32_t byte = blockIdx.y, byte_words = 8 * lwe_words;
    const uint64_t *sb = src + blk * 16 * (uint64_t)n_luts * byte_words;
    const bool keyed = !keys.none();
    const Keys key = keys.key(keyed && key_of_block ? key_of_block[blk] : 0);
    uint64_t *ob = out + (blk * 16 + byte) * (uint64_t)byte_words;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < byte_words; w += gridDim.x * blockDim.x) {
        uint64_t v = keyed ? key.word(byte, w, lwe_words) : 0;
        for (int t = 0; t < tab.terms; ++t)
            v += sb[((uint64_t)tab.src[byte][t] * n_luts + tab.lut[byte][t]) * byte_words + w];
        ob[w] = v;
    }
}

// dst[blk][i] += word i of the round key of key_of_block[blk]  (add_round_key; key_of_block null: one key for all blocks).
// dst: [n_blocks][words_per_block], words_per_block = 128 lwe_words
template <class Keys>
__global__ __launch_bounds__(256) void add_bcast_kernel(uint64_t *dst, const Keys keys, const uint32_t *key_of_block, uint64_t words_per_block,
                                                        uint64_t n_blocks, uint32_t lwe_words)
{
    for (uint64_t blk = blockIdx.y; blk < n_blocks; blk += gridDim.y) {
        const Keys key = keys.key(key_of_block ? key_of_block[blk] : 0);
        uint64_t *db = dst + blk * words_per_block;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words_per_block; i += (uint64_t)gridDim.x * blockDim.x)
            db[i] += key.word(0, (uint32_t)i, lwe_words);
    }
}

// v + trivial(clear) at word w of a byte's [8][lwe_words] words: bit w / lwe_words of `clear`, << 63, on the body word of that bit
__device__ __forceinline__ uint64_t add_trivial_bit(uint64_t v, uint32_t clear, uint32_t w, uint32_t lwe_words)
{
    const uint32_t bit = w / lwe_words;
    return w - bit * lwe_words == lwe_words - 1 ? v + ((uint64_t)((clear >> bit) & 1u) << 63) : v;
}

// ---- XTS (IEEE 1619): the tweak layer ---------------------------------------------------------------------------------------------------
// T_j = T * alpha^j in GF(2^128) mod x^128 + x^7 + x^2 + x + 1.  Bit b (LSB first) of block byte p is degree 8p + b, the flattened
// [16][8] index of a state, and the product is linear over GF(2): output bit i is the sum (XOR == wrapping add of the MSB encodings) of
//   bit i - j                                     if i >= j
//   bit 128 - j + m, m in {i, i-1, i-2, i-7}      if 0 <= m < j     (the j bits shifted out, reduced ONCE by x^128 = x^7 + x^2 + x + 1)
// which holds while no shifted-out bit lands at degree 128 or above again: m + 7 <= 127 for every m < j, that is j <= 121.  The sources
// of a row are distinct and at most 4 (i >= j leaves m < j <= i, so m = i is out).  Returns their count; sources[] are bit indices < 128.
#define XTS_MAX_OFFSET 121u
__host__ __device__ __forceinline__ uint32_t xts_tweak_row(uint32_t j, uint32_t i, uint32_t (&sources)[4])
{
    const uint32_t back[4] = {0, 1, 2, 7};
    uint32_t n = 0;
    if (i >= j) sources[n++] = i - j;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
        if (i >= back[t] && i - back[t] < j && n < 4) sources[n++] = 128 - j + (i - back[t]);
    return n;
}

// ---- bit-row gathers: out row r = the sum of at most 4 source rows of ONE block of 128 rows ------------------------------------------------------
// The XTS tweaks and the CMAC subkeys.  Which block and which rows comes from a by-value rule type with one member,
//   n = rows.row(r, block, sources):  block = the source block's [128][lwe_words], sources[0..n-1] = its rows to sum, n <= Rows::MAX_SOURCES
// out: [n_rows][lwe_words].  Each output bit is gathered from its block in ONE sum (doubling step by step would add a ciphertext to itself:
// the message cancels, the noise does not).  One workgroup per output bit, lanes on consecutive w (rows of kN + 1 words are 8-byte aligned
// and no more: 8-byte accesses); rows are taken in order, so the workgroups that read one block are adjacent in the grid and re-read it
// (2 MB at PARAM_OPT) from L2: HBM sees the 16,392 B per output bit that are written.  All offsets in 64 bits.
template <class Rows>
__global__ __launch_bounds__(256) void bit_rows_kernel(const Rows rows, uint64_t *out, uint64_t n_rows, uint32_t lwe_words)
{
    for (uint64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const uint64_t *block;
        uint32_t s[Rows::MAX_SOURCES];
        const uint32_t n = rows.row(r, block, s);
        const uint64_t *p[Rows::MAX_SOURCES];                    // fully unrolled so that the pointers stay in registers
#pragma unroll
        for (uint32_t t = 0; t < Rows::MAX_SOURCES; ++t) p[t] = block + (uint64_t)(t < n ? s[t] : 0u) * lwe_words;
        uint64_t *o = out + r * lwe_words;
        for (uint32_t w = threadIdx.x; w < lwe_words; w += blockDim.x) {
            uint64_t v = 0;
#pragma unroll
            for (uint32_t t = 0; t < Rows::MAX_SOURCES; ++t)
                if (t < n) v += p[t][w];
            o[w] = v;
        }
    }
}

// out[u][t][i] = the row (off0 + t, i) of xts_tweak_row over anchor[u]: the tweaks off0 .. off0 + n_off - 1 (all <= XTS_MAX_OFFSET) of every
// unit from its anchor, unit u's [128][lwe_words] at u * anchor_stride words.  The up to 121 offsets of a unit re-read its anchor.
struct XtsRows {
    static constexpr uint32_t MAX_SOURCES = 4;
    const uint64_t *anchor;
    uint64_t anchor_stride;
    uint32_t n_off, off0;
    __device__ __forceinline__ uint32_t row(uint64_t r, const uint64_t *&block, uint32_t (&sources)[4]) const
    {
        const uint64_t ut = r >> 7, u = ut / n_off;
        block = anchor + u * anchor_stride;
        return xts_tweak_row(off0 + (uint32_t)(ut - u * n_off), (uint32_t)(r & 127), sources);
    }
};

// XTS whitening, before and after the cipher: dst[b] = (src ? src[b] : 0) + tweaks[tweak_of_block[b]] + trivial(clear block b).
// dst, src: [n_blocks][16][8][lwe_words] (src == dst: in place); tweaks: rows of 128 lwe_words words; clear: [n_blocks][16] bytes, or null
__global__ __launch_bounds__(256) void xts_whiten_kernel(uint64_t *dst, const uint64_t *src, const uint64_t *tweaks, const uint32_t *tweak_of_block,
                                                         const uint8_t *clear, uint64_t n_blocks, uint32_t lwe_words)
{
    const uint32_t byte_words = 8 * lwe_words;
    const uint64_t words_per_block = 16ull * byte_words;
    for (uint64_t blk = blockIdx.y; blk < n_blocks; blk += gridDim.y) {
        const uint64_t *tb = tweaks + (uint64_t)tweak_of_block[blk] * words_per_block;
        const uint64_t *sb = src ? src + blk * words_per_block : nullptr;
        uint64_t *db = dst + blk * words_per_block;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words_per_block; i += gridDim.x * blockDim.x) {
            uint64_t v = tb[i];
            if (sb) v += sb[i];
            if (clear) {
                const uint32_t p = i / byte_words;
                v = add_trivial_bit(v, clear[blk * 16 + p], i - p * byte_words, lwe_words);
            }
            db[i] = v;
        }
    }
}

// ---- CBC-MAC (SP 800-38C CCM): the link between two chain steps -------------------------------------------------------------------------
// One record per slot (a stream of the chain, or an output block): which block of `a` and of `b` it sums (MAC_NONE: none), how many
// leading bytes of the `b` block are real (0..16: a partial last payload block contributes its real bytes, the zero padding nothing),
// how many leading bytes of the output are written as sums (the rest are zero words: a truncated tag), and 16 clear bytes.
#define MAC_NONE 0xFFFFFFFFu
struct MacSlot {
    uint32_t a, b;
    uint32_t b_bytes, out_bytes;
    uint8_t clear[16];
};

// dst[s][row] = row < 8 out_bytes[s] ? a[a_s][row] + (row < 8 b_bytes[s] ? b[b_s][row] : 0) + trivial(bit `row` of clear[s]) : 0 for every
// slot s < n_slots; rows are [16][8], bit LSB first inside a byte, the trivial term is bit << 63 on the body word.  dst, a, b: blocks of
// 128 lwe_words words; a null or a_s == MAC_NONE: no term (the first step of a chain without an init), and the same for b.  In place
// (a == dst) where every a_s == s: a lane reads the word it writes.  With the records' indices this one body is the chain link (dst = a =
// the state, b = the encrypted addends), the first link (a = where the chain starts), the tag difference (dst in the caller's order, a =
// the state by sorted slot, b = S0, clear = the received tag, out_bytes = t) and the copies that put results in the caller's order.
// Lanes on consecutive words, 8-byte accesses (rows of kN + 1 words are 8-byte aligned and no more); one launch whatever n_slots is.
__global__ __launch_bounds__(256) void mac_link_kernel(uint64_t *dst, const uint64_t *a, const uint64_t *b, const MacSlot *slots, uint64_t n_slots,
                                                       uint32_t lwe_words)
{
    const uint32_t byte_words = 8 * lwe_words;
    const uint64_t words_per_block = 16ull * byte_words;
    for (uint64_t s = blockIdx.y; s < n_slots; s += gridDim.y) {
        const MacSlot *sl = slots + s;
        const uint32_t ia = sl->a, ib = sl->b;
        const uint64_t *ab = a && ia != MAC_NONE ? a + (uint64_t)ia * words_per_block : nullptr;
        const uint64_t *bb = b && ib != MAC_NONE ? b + (uint64_t)ib * words_per_block : nullptr;
        const uint32_t b_words = sl->b_bytes * byte_words, out_words = sl->out_bytes * byte_words;
        uint64_t *db = dst + s * words_per_block;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words_per_block; i += gridDim.x * blockDim.x) {
            uint64_t v = 0;
            if (i < out_words) {
                if (ab) v = ab[i];
                if (bb && i < b_words) v += bb[i];
                const uint32_t p = i / byte_words;
                v = add_trivial_bit(v, sl->clear[p], i - p * byte_words, lwe_words);
            }
            db[i] = v;
        }
    }
}

// ---- AES key unwrap (RFC 3394, SP 800-38F): the link between two steps ------------------------------------------------------------------
// Unwrapping C[0..n] (n + 1 semiblocks of 8 bytes, 2 <= n <= 8) is 6n block decryptions chained through 64-bit halves.  Step
// s = 0 .. 6n - 1 works on register i_s = n - s % n under the counter t_s = 6n - s (the RFC's t = n j + i, j = 5 .. 0, i = n .. 1):
//   B = D_KEK((A ^ t_s) | R[i_s]);  A = MSB64(B);  R[i_s] = LSB64(B)
// from A = C[0], R[i] = C[i]; the key is R[1..n], valid iff A == A6A6A6A6A6A6A6A6.  t_s is a big-endian 64-bit integer, so it lands in
// block byte 7 (6n <= 48).
#define KW_MIN_SEMIBLOCKS 2u
#define KW_MAX_SEMIBLOCKS 8u
__host__ __device__ __forceinline__ uint32_t kw_register(uint32_t n, uint32_t s) { return n - s % n; }      // i_s, 1 .. n
__host__ __device__ __forceinline__ uint32_t kw_counter(uint32_t n, uint32_t s) { return 6 * n - s; }       // t_s, 6n .. 1

// Link s = 0 .. 6n of every key.  state: [n_keys][16][8][lwe_words], A on rows 0..63 and the register at work on rows 64..127; regs:
// [n_keys][8 n][8][lwe_words], register i on bytes 8 (i-1) .. 8 i - 1, so that after the last link regs IS the unwrapped key in the layout
// of the key expansion.  wrapped: [n_keys][8 (n + 1)] bytes, read by the load alone.  With half = 64 lwe_words words:
//   s = 0, load:        regs = trivial(C[1..n]); state rows 0..63 = trivial(C[0] ^ t_0), rows 64..127 = trivial(C[n])
//   0 < s < 6n, shuffle: regs[i_{s-1}] <- state rows 64..127 <- regs[i_s]; state rows 0..63 += trivial(t_s)
//   s = 6n, unload:     regs[1] <- state rows 64..127 <- zero words; state rows 0..63 += trivial(A6 x 8): the state is then the `diff` of
//                       the tag check, zero on its first 64 rows iff the key is valid and zero words beyond
// i_{s-1} != i_s since n >= 2, and every lane reads the words it overwrites before it writes them: the link runs in place.  The trivial
// terms are bit << 63 on body words (add_trivial_bit).  Lanes on consecutive words, 8-byte accesses (rows of kN + 1 words are 8-byte aligned
// and no more); one launch whatever n_keys is, the keys beyond the grid's y taken by the loop.  All offsets in 64 bits.
__global__ __launch_bounds__(256) void kw_link_kernel(uint64_t *state, uint64_t *regs, const uint8_t *wrapped, uint64_t n_keys, uint32_t n, uint32_t s,
                                                      uint32_t lwe_words)
{
    const uint32_t byte_words = 8 * lwe_words, half = 8 * byte_words, steps = 6 * n;
    const bool load = s == 0, unload = s == steps;
    const uint32_t t = unload ? 0u : kw_counter(n, s);
    const uint32_t r_in = unload ? 0u : kw_register(n, s) - 1, r_out = load ? 0u : kw_register(n, s - 1) - 1;   // registers from 0
    for (uint64_t key = blockIdx.y; key < n_keys; key += gridDim.y) {
        uint64_t *sb = state + key * 2 * half, *rb = regs + key * (uint64_t)n * half;
        const uint8_t *c = load ? wrapped + key * 8 * (n + 1) : nullptr;
        const uint32_t words = load ? (n + 2) * half : 2 * half;                // the load also fills every register
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) {
            const uint32_t p = i / byte_words, w = i - p * byte_words;          // byte p of [A | the register at work | regs]
            if (i < half) {
                const uint32_t clear = (unload ? 0xA6u : p == 7 ? t : 0u) ^ (load ? c[p] : 0u);
                sb[i] = add_trivial_bit(load ? 0 : sb[i], clear, w, lwe_words);
            } else if (load) {
                if (i < 2 * half) sb[i] = add_trivial_bit(0, c[8 * n + (p - 8)], w, lwe_words);
                else rb[i - 2 * half] = add_trivial_bit(0, c[8 + (p - 16)], w, lwe_words);
            } else {
                const uint32_t j = i - half;
                const uint64_t back = sb[i], next = unload ? 0 : rb[(uint64_t)r_in * half + j];
                rb[(uint64_t)r_out * half + j] = back;
                sb[i] = next;
            }
        }
    }
}

// ---- CMAC (SP 800-38B, RFC 4493): the subkeys --------------------------------------------------------------------------------------------
// K1 = L * x and K2 = L * x^2 in GF(2^128) mod x^128 + x^7 + x^2 + x + 1, L = E_K(0^128): the XTS arithmetic in the other byte order.  A
// CMAC block is a big-endian integer, so bit b (LSB first) of block byte p -- flattened [16][8] index i = 8p + b -- is degree
// 8 (15 - p) + b where XTS has 8p + b.  The map between index and degree is its own inverse.
__host__ __device__ __forceinline__ uint32_t cmac_bit_degree(uint32_t i) { return (120u - (i & ~7u)) | (i & 7u); }

// The sources of output bit i of L * x^(which + 1), which in {0: K1, 1: K2}: xts_tweak_row's rule for j = which + 1 on degrees, mapped back
// to indices.  With j <= 2 only the degrees 0, 1, 2, 3, 7 and 8 receive reduction terms, one or two each: the sources are distinct, at
// most 2 for K1 and 3 for K2 (131 and 134 ones in the two 128 x 128 matrices).  Returns their count; sources[] are indices < 128.
__host__ __device__ __forceinline__ uint32_t cmac_subkey_row(uint32_t which, uint32_t i, uint32_t (&sources)[3])
{
    const uint32_t back[4] = {0, 1, 2, 7};
    const uint32_t j = which + 1, d = cmac_bit_degree(i);
    uint32_t n = 0;
    if (d >= j) sources[n++] = cmac_bit_degree(d - j);
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
        if (d >= back[t] && d - back[t] < j && n < 3) sources[n++] = cmac_bit_degree(128 - j + (d - back[t]));
    return n;
}

// out[key][which][i] = the row (which, i) of cmac_subkey_row over l[key]: both subkeys of every key in ONE launch of bit_rows_kernel (K2 is
// not a doubling of the computed K1, for the reason given there).  l: [n_keys][128][lwe_words]; out: [n_keys][2][128][lwe_words], 256 rows
// per key.
struct CmacRows {
    static constexpr uint32_t MAX_SOURCES = 3;
    const uint64_t *l;
    uint32_t lwe_words;
    __device__ __forceinline__ uint32_t row(uint64_t r, const uint64_t *&block, uint32_t (&sources)[3]) const
    {
        block = l + (r >> 8) * 128 * lwe_words;
        return cmac_subkey_row((uint32_t)(r >> 7) & 1u, (uint32_t)(r & 127), sources);
    }
};

// Rows of bytes moved between strided sets, one set per AES key: the word operations of the key expansion over all keys at once (RotWord,
// w[i-1] or the SubWord result + w[i-Nk] + Rcon, placing refreshed words at their stride) and the strided copies of the round-key
// conversion.  For key j and byte q < n_bytes:
//   dst[j][q] = a[j][(q & ~3) | ((q + rot) & 3)] + (b ? b[j][q] : 0) + (q == 0 ? trivial(rcon) : 0)
// a, b, dst: rows of byte_words = 8 * lwe_words words, key j's at j * {a,b,dst}_stride words.  trivial(v): bit j of v << 63 on body j.
__global__ __launch_bounds__(256) void key_rows_kernel(uint64_t *dst, uint64_t dst_stride, const uint64_t *a, uint64_t a_stride, uint32_t rot,
                                                       const uint64_t *b, uint64_t b_stride, uint32_t rcon, uint32_t lwe_words, uint64_t n_keys)
{
    const uint32_t byte_words = 8 * lwe_words, q = blockIdx.y;
    const uint32_t clear = q == 0 ? rcon : 0u;
    for (uint64_t j = blockIdx.z; j < n_keys; j += gridDim.z) {
        const uint64_t *ab = a + j * a_stride + (uint64_t)((q & ~3u) | ((q + rot) & 3u)) * byte_words;
        const uint64_t *bb = b ? b + j * b_stride + (uint64_t)q * byte_words : nullptr;
        uint64_t *ob = dst + j * dst_stride + (uint64_t)q * byte_words;
        for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < byte_words; w += gridDim.x * blockDim.x) {
            uint64_t v = ab[w];
            if (bb) v += bb[w];
            if (clear) v = add_trivial_bit(v, clear, w, lwe_words);
            ob[w] = v;
        }
    }
}

// ---- public blocks / CTR with a public nonce (fheaes_aes_encrypt_public_bits, fheaes_aes_ctr_bits) ------------------------------
// Every distinct S-Box input of a batch of PUBLIC blocks is evaluated once: a round works on a POOL of distinct bytes instead of
// [n_blocks][16].  One uint32 head word per pool entry says where it sits in the state and which clear byte goes with it:
#define PUBLIC_HEAD(pos, clear, key) ((uint32_t)(pos) | ((uint32_t)(clear) << 8) | ((uint32_t)(key) << 16))     // bits 0..3: state position p, 8..15: clear byte, 16..31: AES key
#define PUBLIC_MAX_KEYS 65536u      /* the key index of a pool entry has 16 bits */
// and one uint32 per term says what to sum: WoPBS output `lut` of pool entry `src` of the round before
#define PUBLIC_TERM(src, lut) (((uint32_t)(src) << 2) | (uint32_t)(lut))

// The linear layer into a pool, and from the last pool into the state: gather_add_kernel with the sources of every output byte read
// from a table in device memory instead of being the same for every block.
//   out[u] = sum_{j < terms} pool[src_uj][lut_uj] + rk[key_u][p_u] + trivial(clear_u)
// pool: [n_src][n_luts][byte_words] (WoPBS outputs of the round before); head: [n_out] PUBLIC_HEAD; term: [n_out][terms] PUBLIC_TERM;
// keys: the round key of this layer; out: [n_out][byte_words], byte_words = 8 lwe_words.  Wrapping uint64 sums: any order of the terms
// gives gather_add_kernel's words.  clear_u is 0 except in two layers.  The pool of round 1 has terms == 0 (pool and term are not read)
// and clear_u = the public byte: out[u] = rk0[key_u][p_u] + trivial(v_u), word for word the initial AddRoundKey on a trivial ciphertext
// (mask 0, body = bit << 63) of v_u.  CTR's last layer adds the data byte.
template <class Keys>
__global__ __launch_bounds__(256) void gather_add_indexed_kernel(const uint64_t *pool, uint32_t n_luts, const uint32_t *head, const uint32_t *term,
                                                                 uint32_t terms, const Keys keys, uint64_t *out, uint64_t n_out, uint32_t lwe_words)
{
    const uint32_t byte_words = 8 * lwe_words;
    for (uint64_t u = blockIdx.y; u < n_out; u += gridDim.y) {
        const uint32_t h = head[u], pos = h & 15u, clear = (h >> 8) & 0xFFu;
        const Keys key = keys.key(h >> 16);
        const uint64_t *s[4];                                    // terms <= 4; fully unrolled so that the pointers stay in registers
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t e = t < terms ? term[u * terms + t] : 0u;
            s[t] = pool + ((uint64_t)(e >> 2) * n_luts + (e & 3u)) * byte_words;
        }
        uint64_t *ob = out + u * byte_words;
        for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < byte_words; w += gridDim.x * blockDim.x) {
            uint64_t v = key.word(pos, w, lwe_words);
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t)
                if (t < terms) v += s[t][w];
            if (clear) v = add_trivial_bit(v, clear, w, lwe_words);
            ob[w] = v;
        }
    }
}

// Builds the radix inputs of add_scalar (server.rs:216-222): in[blk][0..8) = state[blk][byte] and, for
// bits == 9, in[blk][8] = carry[blk]
__global__ __launch_bounds__(256) void pack9_kernel(const uint64_t *state, const uint64_t *carry, uint64_t *in9,
                                                    uint32_t byte, uint32_t lwe_words, uint64_t n_blocks, uint32_t bits)
{
    const uint64_t blk = blockIdx.y;
    const uint64_t *sb = state + (blk * 16 + byte) * 8ull * lwe_words;
    const uint64_t *cb = carry + blk * lwe_words;
    uint64_t *o = in9 + blk * (uint64_t)bits * lwe_words;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < bits * lwe_words; w += gridDim.x * blockDim.x)
        o[w] = (w < 8 * lwe_words) ? sb[w] : cb[w - 8 * lwe_words];
}

// Scatter the results of one add_scalar step: res [n_blocks][2][bits][lwe]: LUT 0 blocks 0..7 -> state byte,
// LUT 1 block 0 -> carry
__global__ __launch_bounds__(256) void unpack_sum_carry_kernel(const uint64_t *res, uint32_t bits, uint64_t *state, uint64_t *carry,
                                                               uint32_t byte, uint32_t lwe_words, uint64_t n_blocks)
{
    const uint64_t blk = blockIdx.y;
    const uint64_t *rb = res + blk * 2ull * bits * lwe_words;
    uint64_t *sb = state + (blk * 16 + byte) * 8ull * lwe_words;
    uint64_t *cb = carry + blk * lwe_words;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < 9 * lwe_words; w += gridDim.x * blockDim.x) {
        if (w < 8 * lwe_words) sb[w] = rb[w];
        else cb[w - 8 * lwe_words] = rb[(uint64_t)bits * lwe_words + (w - 8 * lwe_words)];
    }
}

// LUTs of add_scalar (server.rs:181-197, :225-248) for every block: luts[blk][2][bits][512];
// addend[blk] = the counter byte added at this position.  bits = 8: f=(x+c)%256, g = x+c>255;
// bits = 9: x = byte | carry<<8.
__global__ __launch_bounds__(256) void counter_lut_kernel(uint64_t *luts, const uint8_t *addend, uint32_t bits, uint64_t n_blocks)
{
    const uint64_t blk = blockIdx.y;
    const uint32_t c = addend[blk];
    uint64_t *L = luts + blk * 2ull * bits * 512;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < 2 * bits * 512; e += gridDim.x * blockDim.x) {
        uint32_t which = e / (bits * 512), rem = e % (bits * 512);
        uint32_t bit = rem / 512, idx = rem % 512;
        uint32_t x = idx & ((1u << bits) - 1);
        uint32_t s = (x & 0xFF) + ((bits == 9) ? ((x >> 8) & 1) : 0) + c;
        uint32_t val = which == 0 ? (s & 0xFF) : (s > 255 ? 1u : 0u);
        L[e] = (uint64_t)((val >> bit) & 1u) << 63;
    }
}

// ---- seeded evaluation keys (fheaes_upload_keys_seeded) -------------------------------------------------------------
// Mask word j of key ciphertext q of key `tag` = 64-bit word j % 8 of ChaCha20 block j / 8 under (public mask key,
// nonce = (tag, q)): the counter-based stream of csrc/client.c (RFC 8439 block function; kept identical here).
struct MaskKey {
    uint32_t k[8];
};

#define FHEAES_QR(a, b, c, d)                                                   \
    a += b; d ^= a; d = (d << 16) | (d >> 16); c += d; b ^= c; b = (b << 12) | (b >> 20); \
    a += b; d ^= a; d = (d << 8) | (d >> 24);  c += d; b ^= c; b = (b << 7) | (b >> 25)

__device__ __forceinline__ void fheaes_chacha20_block(const MaskKey &key, uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t (&out)[16])
{
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                            key.k[4], key.k[5], key.k[6], key.k[7], counter, n0, n1, n2};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll 1
    for (int r = 0; r < 10; ++r) {
        FHEAES_QR(x[0], x[4], x[8], x[12]); FHEAES_QR(x[1], x[5], x[9], x[13]);
        FHEAES_QR(x[2], x[6], x[10], x[14]); FHEAES_QR(x[3], x[7], x[11], x[15]);
        FHEAES_QR(x[0], x[5], x[10], x[15]); FHEAES_QR(x[1], x[6], x[11], x[12]);
        FHEAES_QR(x[2], x[7], x[8], x[13]); FHEAES_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

// out [n_cts][mask_words + body_words] <- regenerated masks | bodies [n_cts][body_words].  One thread per (ciphertext,
// 8-word block of its mask); the bodies are copied by the threads of the last block(s).
__global__ __launch_bounds__(256) void expand_masks_kernel(uint64_t *out, const uint64_t *bodies, uint64_t n_cts, uint32_t mask_words,
                                                           uint32_t body_words, MaskKey key, uint32_t tag)
{
    const uint32_t ct_words = mask_words + body_words;
    const uint32_t mask_blocks = (mask_words + 7) / 8, body_blocks = (body_words + 7) / 8;
    const uint32_t blocks = mask_blocks + body_blocks;
    const uint64_t total = n_cts * blocks;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = i / blocks;
        const uint32_t bi = (uint32_t)(i - q * blocks);
        uint64_t *o = out + q * ct_words;
        if (bi < mask_blocks) {
            uint32_t w[16];
            fheaes_chacha20_block(key, bi, tag, (uint32_t)q, (uint32_t)(q >> 32), w);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t j = bi * 8 + e;
                if (j < mask_words) o[j] = (uint64_t)w[2 * e] | ((uint64_t)w[2 * e + 1] << 32);
            }
        } else {
            const uint32_t b0 = (bi - mask_blocks) * 8;
            for (uint32_t e = 0; e < 8 && b0 + e < body_words; ++e) o[mask_words + b0 + e] = bodies[q * body_words + b0 + e];
        }
    }
}

// ---- packing: N bits in the N coefficients of one GLWE (fheaes_pack_bits, fheaes_unpack_bits) -----------------------------------
// ks[t] = [(k+1)][N]: LWE t through key block r = k of the PFPKSK (f(x) = x: the message sits in the constant coefficient).
//   packed[g] = sum_{i < cnt_g} X^i * ks[gN + i]   negacyclic in each polynomial: coefficient c takes +P[c - i] (c >= i), -P[c - i + N] (c < i)
// Every input word is read once and nothing is reused: the kernel is a stream over ks.  One workgroup takes PACK_FOLD_ROWS values of i
// for one (GLWE, polynomial): for fixed i the 512 rotated reads of a row are two contiguous runs, each thread keeps coefficients c and
// c + 256, and the partial sums of the N / PACK_FOLD_ROWS workgroups of a polynomial meet in `packed` (zeroed by the launcher) with one
// 64-bit atomic add per coefficient.  Wrapping integer sums: any order gives the same words.
#define PACK_FOLD_ROWS 32
#define PACK_FOLD_UNROLL 8

// ks: [m][k1][N] (bits of this launch, the first one at coefficient 0 of packed[0]); packed: [ceil(m / N)][k1][N], zero on entry
__global__ __launch_bounds__(256) void pack_fold_kernel(const uint64_t *ks, uint64_t m, uint32_t k1, uint64_t *packed)
{
    const uint32_t split = blockIdx.x, j = blockIdx.y;
    const uint64_t g = blockIdx.z;
    const uint64_t left = m - g * PACK_N;                               // bits of this GLWE onward: the grid has no GLWE beyond m
    const uint32_t cnt = left < PACK_N ? (uint32_t)left : PACK_N;
    const uint32_t i0 = split * PACK_FOLD_ROWS;
    if (i0 >= cnt) return;                                              // a partly filled last GLWE: nothing to add from here on
    const uint32_t i1 = i0 + PACK_FOLD_ROWS < cnt ? i0 + PACK_FOLD_ROWS : cnt;
    const uint32_t c = threadIdx.x;                                     // coefficients c and c + 256
    const uint64_t row_words = (uint64_t)k1 * PACK_N;
    const uint64_t *src = ks + (g * PACK_N) * row_words + (uint64_t)j * PACK_N;
    uint64_t lo = 0, hi = 0;
    uint32_t i = i0;
    for (; i + PACK_FOLD_UNROLL <= i1; i += PACK_FOLD_UNROLL) {
        uint64_t a[PACK_FOLD_UNROLL], b[PACK_FOLD_UNROLL];
#pragma unroll
        for (int u = 0; u < PACK_FOLD_UNROLL; ++u) {
            const uint64_t *row = src + (uint64_t)(i + u) * row_words;
            a[u] = row[(c - (i + u)) & (PACK_N - 1)];
            b[u] = row[(c + 256 - (i + u)) & (PACK_N - 1)];
        }
#pragma unroll
        for (int u = 0; u < PACK_FOLD_UNROLL; ++u) {
            lo += c >= i + u ? a[u] : (uint64_t)0 - a[u];
            hi += c + 256 >= i + u ? b[u] : (uint64_t)0 - b[u];
        }
    }
    for (; i < i1; ++i) {
        const uint64_t *row = src + (uint64_t)i * row_words;
        const uint64_t a = row[(c - i) & (PACK_N - 1)], b = row[(c + 256 - i) & (PACK_N - 1)];
        lo += c >= i ? a : (uint64_t)0 - a;
        hi += c + 256 >= i ? b : (uint64_t)0 - b;
    }
    unsigned long long *dst = (unsigned long long *)(packed + g * row_words + (uint64_t)j * PACK_N);
    atomicAdd(dst + c, (unsigned long long)lo);
    atomicAdd(dst + c + 256, (unsigned long long)hi);
}

// Sample extraction of coefficient i = t % N of GLWE t / N (sample_extract_word).  One workgroup per bit writes the kN + 1 words of its
// LWE in order; the reads run backwards through a polynomial that the N bits of a GLWE share (20 KB, cache resident), so HBM sees the
// writes: 16,392 B per bit.
// packed: the first of ceil(m / N) GLWEs, through either reader; lwe: [m][kN + 1]
#define UNPACK_BITS_PER_WG 4
template <class Glwe>
__device__ __forceinline__ void sample_extract_bits(const Glwe packed, uint64_t m, uint32_t k, uint64_t *lwe)
{
    const uint32_t big = k * PACK_N;
    for (uint32_t u = 0; u < UNPACK_BITS_PER_WG; ++u) {
        const uint64_t t = (uint64_t)blockIdx.x * UNPACK_BITS_PER_WG + u;
        if (t >= m) return;
        const uint32_t i = (uint32_t)(t & (PACK_N - 1));
        const Glwe glwe = packed.glwe(t / PACK_N, k);
        uint64_t *o = lwe + t * (uint64_t)(big + 1);
        for (uint32_t w = threadIdx.x; w < big; w += blockDim.x) o[w] = sample_extract_word(glwe, i, w, k);
        if (threadIdx.x == 0) o[big] = sample_extract_word(glwe, i, big, k);
    }
}

// packed: [ceil(m / N)][k + 1][N]
__global__ __launch_bounds__(256) void sample_extract_kernel(const uint64_t *packed, uint64_t m, uint32_t k, uint64_t *lwe)
{
    sample_extract_bits(GlweWords{packed}, m, k, lwe);
}

// ---- wire formats (include/fheaes.h): seeded input ciphertexts, modulus-switched packed outputs --------------------------------------
// fheaes_expand_lwe_seeded: lwe[t] = [ mask words of ciphertext first + t | bodies[t] ], mask word j = 64-bit word j % 8 of ChaCha20
// block j / 8 under (key, nonce = (EXPAND_LWE_TAG, q low 32, q high 32)), q = first + t: expand_masks_kernel's stream for the shape
// mask_words = kN = 512 k, one body word.  A lane computes one block (8 words); the 64 blocks of a wave are one contiguous run of 512
// words of ONE ciphertext (kN / 8 = 64 k blocks).  Stored lane by lane, every store instruction would touch 64 separate 64-byte runs;
// the wave's blocks go through LDS instead and come back word e * 64 + lane, so that each of the 8 store instructions of a wave covers
// one run of 512 bytes.  LDS rows have 9 words: the b64 writes of a half wave (word 9 lane + e) fall on 32 different bank pairs.  The
// padding serves the writes only: a half wave reads words j + (j >> 3) of 32 consecutive j, that is 0..7, 9..16, 18..25, 27..34 past its
// first, and 32..34 share bank pairs with 0..2 -- three 2-way conflicts in each of the 8 b64 reads, a few cycles next to the ~1,000
// instructions of the block function, so no swizzle is spent on them.  A row of the output has kN + 1 words, so rows are 8-byte aligned
// and no more: 8-byte stores.  One workgroup = 4 waves = 4 runs; nothing is read but the bodies.
// A wave touches tile[wave] alone, so a wave-level wait for its LDS writes would do; the workgroup barrier is kept because it is the
// plain form, and every wave must reach it: a wave past the last run (`live` false, the last workgroup of a launch) skips the block
// function and the stores but returns only AFTER the barrier.
#define EXPAND_LWE_TAG 6u            /* MASK_TAG_LWE of csrc/client.c */
#define EXPAND_LWE_ROW 9             /* LDS words per block: 8 + 1 of padding */
// bodies: [m]; lwe: [m][64 k * 8 + 1]; runs = m * k waves of work
__global__ __launch_bounds__(256) void expand_lwe_kernel(uint64_t *lwe, const uint64_t *bodies, uint64_t m, uint32_t k, uint64_t first, MaskKey key)
{
    __shared__ uint64_t tile[4][64 * EXPAND_LWE_ROW];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t run = (uint64_t)blockIdx.x * 4 + wave;              // run r: blocks 64 (r % k) .. of ciphertext r / k
    const bool live = run < m * k;
    const uint64_t t = run / k;
    const uint32_t part = (uint32_t)(run - t * k);
    uint64_t *row = tile[wave];
    if (live) {
        const uint64_t q = first + t;
        uint32_t w[16];
        fheaes_chacha20_block(key, part * 64 + lane, EXPAND_LWE_TAG, (uint32_t)q, (uint32_t)(q >> 32), w);
#pragma unroll
        for (int e = 0; e < 8; ++e) row[lane * EXPAND_LWE_ROW + e] = (uint64_t)w[2 * e] | ((uint64_t)w[2 * e + 1] << 32);
    }
    __syncthreads();
    if (!live) return;
    const uint32_t big = k * PACK_N;
    uint64_t *o = lwe + t * (uint64_t)(big + 1) + (uint64_t)part * PACK_N;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t j = e * 64 + lane;                              // word j of the run: block j / 8, word j % 8
        o[j] = row[(j >> 3) * EXPAND_LWE_ROW + (j & 7)];
    }
    if (part == k - 1 && lane == 0) lwe[t * (uint64_t)(big + 1) + big] = bodies[t];
}

// fheaes_packed_mod_switch: word x of a packed GLWE -> the w-bit value v = ((x + 2^(63-w)) >> (64-w)) mod 2^w (the sum wraps in
// uint64: words within 2^(63-w) of 2^64 round to 0), field e = jN + c at bits [e w, (e+1) w) of the GLWE's little-endian bit string.
// One thread per OUTPUT word: it gathers the at most ceil(64 / w) + 1 fields that touch its 64 bits, so no two threads write one
// word.  A GLWE is (k+1) N w / 64 = (k+1) 8 w whole words.  8 <= w <= 32.
// glwe: [n_glwe][glwe_words]; out: [n_glwe][glwe_words * w / 64]
__global__ __launch_bounds__(256) void mod_switch_pack_kernel(const uint64_t *glwe, uint64_t n_glwe, uint32_t glwe_words, uint32_t w, uint64_t *out)
{
    const uint32_t out_words = glwe_words / 64 * w;
    const uint64_t total = n_glwe * out_words;
    const uint64_t half = 1ull << (63 - w);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = i / out_words;
        const uint32_t o = (uint32_t)(i - g * out_words);
        const uint64_t *src = glwe + g * glwe_words;
        const uint32_t bit0 = o * 64;                                  // < 2560 * 32: fits
        const uint32_t e0 = bit0 / w, e1 = (bit0 + 63) / w;            // e1 <= glwe_words - 1: the bit string ends with the last field
        uint64_t acc = 0;
        for (uint32_t e = e0; e <= e1; ++e) {
            const uint64_t v = (src[e] + half) >> (64 - w);
            const uint32_t at = e * w;
            acc |= at >= bit0 ? v << (at - bit0) : v >> (bit0 - at);
        }
        out[i] = acc;
    }
}

// sample_extract_kernel reading the w-bit fields: word for word the extraction of the read-back GLWEs
// in: [ceil(m / N)][(k + 1) 8 w]
__global__ __launch_bounds__(256) void sample_extract_mod_kernel(const uint64_t *in, uint64_t m, uint32_t k, uint32_t w, uint64_t *lwe)
{
    sample_extract_bits(GlweFields{in, w}, m, k, lwe);
}
