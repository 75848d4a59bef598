// host_tables.h -- tables that the host builds once: the transform's twiddles, the AES tables from the field definition,
// the LUT sets of the S-Box front end and the gather tables of the linear layers.
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// host tables
// ---------------------------------------------------------------------------------------------
struct HostTwiddles {
    double psi_re[FHE_N], psi_im[FHE_N];
    HostTwiddles()
    {
        // psi^j = exp(i pi j/512): half-angle recurrences in long double, products of the
        // binary powers, octant symmetry (same specification as oracle/fheaes_oracle.c).
        long double bc[8], bs[8];
        bc[7] = sqrtl(0.5L); bs[7] = bc[7];
        for (int m = 6; m >= 0; --m) {
            long double c = sqrtl((1.0L + bc[m + 1]) / 2.0L);
            long double s = bs[m + 1] / (2.0L * c);
            bc[m] = c; bs[m] = s;
        }
        for (int j = 0; j <= 128; ++j) {
            long double pr = 1.0L, pi = 0.0L;
            for (int m = 0; m < 8; ++m) if ((j >> m) & 1) {
                long double nr = pr * bc[m] - pi * bs[m];
                long double ni = pr * bs[m] + pi * bc[m];
                pr = nr; pi = ni;
            }
            psi_re[j] = (double)pr; psi_im[j] = (double)pi;
        }
        psi_re[0] = 1.0; psi_im[0] = 0.0;
        psi_im[128] = psi_re[128];
        for (int j = 129; j <= 256; ++j) { psi_re[j] = psi_im[256 - j]; psi_im[j] = psi_re[256 - j]; }
        for (int j = 257; j < 512; ++j) { psi_re[j] = -psi_re[512 - j]; psi_im[j] = psi_im[512 - j]; }
    }
    // psi^e, e mod 1024
    void pow(int e, double &re, double &im) const
    {
        e &= 1023;
        if (e < 512) { re = psi_re[e]; im = psi_im[e]; }
        else { re = -psi_re[e - 512]; im = -psi_im[e - 512]; }
    }
};

const HostTwiddles &twiddles()
{
    static HostTwiddles t;
    return t;
}

// AES tables from the field definition (tables/table.rs, sbox.rs:20-42)
struct AesTables {
    uint8_t sbox[256], inv[256];
    static uint8_t mul(uint8_t a, uint8_t b)
    {
        uint8_t r = 0;
        for (int i = 0; i < 8; ++i) { if (b & 1) r ^= a; uint8_t hi = a & 0x80; a = (uint8_t)(a << 1); if (hi) a ^= 0x1B; b >>= 1; }
        return r;
    }
    AesTables()
    {
        for (int x = 0; x < 256; ++x) {
            uint8_t y = 0;
            if (x) for (int c = 1; c < 256; ++c) if (mul((uint8_t)x, (uint8_t)c) == 1) { y = (uint8_t)c; break; }
            uint8_t s = y, v = y;
            for (int i = 0; i < 4; ++i) { v = (uint8_t)((v << 1) | (v >> 7)); s ^= v; }
            s ^= 0x63;
            sbox[x] = s; inv[s] = (uint8_t)x;
        }
    }
};

const AesTables &aes_tables()
{
    static AesTables t;
    return t;
}

// 0..4 mirror oracle.LUTSET_*; LUTSET_DEC_EQ_ROUND (the equivalent inverse cipher's round, FIPS-197 section 5.3.5) is appended after them
enum { LUTSET_ENC_ROUND = 0, LUTSET_SBOX, LUTSET_INV_SBOX, LUTSET_DEC_MUL, LUTSET_IDENTITY, LUTSET_DEC_EQ_ROUND, LUTSET_COUNT };

// words of one (LUT, output bit) row: gen_lut.rs:19-23, lut_size = max(2^nb_block, polynomial_size)
inline uint64_t lut_row_words(uint32_t nb) { return nb > 9 ? (1ull << nb) : (uint64_t)FHE_N; }

void gen_lut_host(uint32_t nb, const uint64_t *f, uint64_t *out)
{
    const uint64_t W = lut_row_words(nb);
    for (uint64_t idx = 0; idx < W; ++idx) {
        uint64_t v = f[idx & ((1ull << nb) - 1)];
        for (uint32_t b = 0; b < nb; ++b) out[(size_t)b * W + idx] = ((v >> b) & 1ull) << 63;
    }
}

int build_lutset_host(int which, std::vector<uint64_t> &out)
{
    const AesTables &T = aes_tables();
    uint64_t f[4][256];
    int n = 1;
    for (int x = 0; x < 256; ++x) {
        uint8_t s = T.sbox[x];
        switch (which) {
        case LUTSET_ENC_ROUND: f[0][x] = s; f[1][x] = AesTables::mul(s, 2); f[2][x] = AesTables::mul(s, 3); n = 3; break;
        case LUTSET_SBOX: f[0][x] = s; break;
        case LUTSET_INV_SBOX: f[0][x] = T.inv[x]; break;
        case LUTSET_DEC_MUL:
            f[0][x] = AesTables::mul((uint8_t)x, 9); f[1][x] = AesTables::mul((uint8_t)x, 11);
            f[2][x] = AesTables::mul((uint8_t)x, 13); f[3][x] = AesTables::mul((uint8_t)x, 14); n = 4; break;
        case LUTSET_DEC_EQ_ROUND:                                   // {9, 11, 13, 14} * InvS[x]: same order as LUTSET_DEC_MUL, so MC_DEC indexes it
            f[0][x] = AesTables::mul(T.inv[x], 9); f[1][x] = AesTables::mul(T.inv[x], 11);
            f[2][x] = AesTables::mul(T.inv[x], 13); f[3][x] = AesTables::mul(T.inv[x], 14); n = 4; break;
        default: f[0][x] = (uint64_t)x; break;
        }
    }
    out.assign((size_t)n * 8 * FHE_N, 0);
    for (int i = 0; i < n; ++i) gen_lut_host(8, f[i], out.data() + (size_t)i * 8 * FHE_N);
    return n;
}

// The two LUTs of the CCM tag check, one LUT each.  which = 0: 8 bits in, output bit 0 = (byte != 0); which = 1: 16 bits in (one per tag
// byte), output bit 0 = (input == 0), the validity bit.  The other output bits are 0.  Returns the input width.
uint32_t build_tag_lut_host(int which, std::vector<uint64_t> &out)
{
    const uint32_t nb = which ? 16 : 8;
    std::vector<uint64_t> f((size_t)1 << nb);
    for (size_t x = 0; x < f.size(); ++x) f[x] = which ? (x == 0) : (x != 0);
    out.assign((size_t)nb * lut_row_words(nb), 0);
    gen_lut_host(nb, f.data(), out.data());
    return nb;
}

const int MC_ENC[4][4] = {{1, 2, 0, 0}, {0, 1, 2, 0}, {0, 0, 1, 2}, {2, 0, 0, 1}};
const int MC_DEC[4][4] = {{3, 1, 2, 0}, {0, 3, 1, 2}, {2, 0, 3, 1}, {1, 2, 0, 3}};

// the four-term gather tables: out[col][row] = sum_j mc[row][j] * in[(col + shift * j) & 3][j], term j reads LUT mc[row][j] of the set
GatherTable table_mix(const int (&mc)[4][4], int shift)
{
    GatherTable t{}; t.terms = 4;
    for (int col = 0; col < 4; ++col) for (int row = 0; row < 4; ++row) for (int r2 = 0; r2 < 4; ++r2) {
        t.src[4 * col + row][r2] = (int8_t)(4 * ((col + shift * r2) & 3) + r2);
        t.lut[4 * col + row][r2] = (int8_t)mc[row][r2];
    }
    return t;
}
GatherTable table_enc_round() { return table_mix(MC_ENC, 1); }             // ShiftRows folded into MixColumns
GatherTable table_dec_mix() { return table_mix(MC_DEC, 0); }               // InvMixColumns alone
// InvShiftRows folded into InvMixColumns (the equivalent inverse cipher's round): out[c][r] = sum_j MC_DEC[r][j] * in[(c - j) & 3][j]
GatherTable table_dec_eq_round() { return table_mix(MC_DEC, -1); }
GatherTable table_shift_rows(bool inverse)
{
    GatherTable t{}; t.terms = 1;
    for (int col = 0; col < 4; ++col) for (int row = 0; row < 4; ++row) {
        t.src[4 * col + row][0] = (int8_t)(4 * ((inverse ? col - row : col + row) & 3) + row);
        t.lut[4 * col + row][0] = 0;
    }
    return t;
}

}  // namespace
