// kern_audit.h -- the audit (fheaes_audit_set, fheaes_audit_stage_set): S sampled rows of a launch are computed again by a second form of the
// stage and the two results are compared on the device, bit for bit.  The engine is deterministic and every form of a stage writes the same
// words, so a difference is a defect of the engine or of the machine and never noise.
//
// What every stage's audit runs (audit_begin, audit_compare in engine_launch.h), around the stage's own second form:
//   audit_tamper_kernel    the test hook (fheaes_audit_stage_debug): one thread XORs a mask into one word of the product launch's output;
//   (the second form)      the S sampled rows -> audit_out;
//   audit_compare_kernel   workgroup s compares audit_out[s] with row audit_row(s) of the product launch's output, row_words words at
//                          out + row out_stride, counts a wrong row and keeps a record of the first AUDIT_RECORDS of them.
//
// The blind rotation (K2): the sampled rows go through the latency form (kern_blindrot_latency.h: no parking, no slot pool, no owner words,
// no generation plan; tests/test_gpu_k2_shapes.py), which takes its inputs as one array:
//   audit_gather_kernel    workgroup s copies the small LWE of its sampled row (n + 1 words) into audit_in[s];
//   (the latency form)     audit_in -> audit_out, count = S.
// A row is the kN + 1 words of a ciphertext, out_stride = row_words; 2 x 16 KB per row: nothing here is near any roof.
//
// The key switches (K1, K3): both are an exact integer matrix product mod 2^64, so any order of evaluation gives the same words.  The
// product kernels (kern_keyswitch.h) slice it onto the int8 matrix cores: digit planes in A-fragment order, 15 byte products recombined with
// shifts, LDS-DMA double buffering.  The plain form below shares none of that:
//   keyswitch_plain_kernel  out[s][z][o] = body - sum_{i,l} digit_l(in[row(s)][i]) KEY[z][i levels + l][o] in wrapping uint64 arithmetic: the
//                           digits recomputed from the input words (decompose_all), the key words recombined from the only copy on the
//                           device, the balanced byte planes in B-fragment order (KEY = sum_j kb_j 2^(8j)), one 64-bit multiply-add per
//                           term.  No matrix cores, no digit planes, no LDS-DMA.  row(s) = audit_row(s) behind a launch, s itself under
//                           fheaes_audit_plain_batch.
// A row is n + 1 words for K1 and the (k+1)N words of each key block of the launch for K3.  What both forms share, and the audit therefore cannot see: the resident key bytes, decompose_all, keybytes_kernel (the oracle tests cover
// the last two).
#pragma once
#include <stdint.h>
#include "fft_dev.h"

#define AUDIT_MAX_ROWS 256       /* FHEAES_AUDIT_MAX_ROWS: one latency-form workgroup per sampled row, at most one per CU */
#define AUDIT_RECORDS 16         /* FHEAES_AUDIT_RECORDS */
#define AUDIT_RECORD_WORDS 5     /* {launch, row, first differing word, word of the product launch, word of the audit} */
#define AUDIT_THREADS 256
// the audit's state on the device, uint64 words: three counters, then the records
#define AUDIT_ST_LAUNCHES 0
#define AUDIT_ST_CHECKED 1
#define AUDIT_ST_WRONG 2
#define AUDIT_ST_RECORDS 3
#define AUDIT_STATE_WORDS (AUDIT_ST_RECORDS + AUDIT_RECORDS * AUDIT_RECORD_WORDS)

__host__ __device__ inline uint64_t audit_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// floor(s m / S) for s <= S <= AUDIT_MAX_ROWS without a product that could leave 64 bits: m = q S + r gives s q + floor(s r / S)
__host__ __device__ inline uint64_t audit_stratum_start(uint64_t m, uint32_t S, uint32_t s) { return s * (m / S) + s * (m % S) / S; }

// The row that sample s of audited launch `launch` checks in a batch of m rows, S = min(rows, m) samples: stratified, sample s lies in
// [floor(s m / S), floor((s + 1) m / S)) at offset mix(seed, launch, s) mod the stratum's length (include/fheaes.h, fheaes_audit_rows)
__host__ __device__ inline uint64_t audit_row(uint64_t seed, uint64_t launch, uint64_t m, uint32_t S, uint32_t s)
{
    const uint64_t lo = audit_stratum_start(m, S, s), hi = audit_stratum_start(m, S, s + 1);
    return lo + audit_splitmix64(audit_splitmix64(seed + launch) + s) % (hi - lo);
}

// grid S, AUDIT_THREADS threads: audit_in[s] = lwe_small[row(s)], n1 = n + 1 words
__global__ __launch_bounds__(AUDIT_THREADS) void audit_gather_kernel(const uint64_t *lwe_small, uint32_t n1, uint64_t seed, uint64_t launch, uint64_t m, uint32_t S,
                                                                     uint64_t *audit_in)
{
    const uint32_t s = blockIdx.x;
    const uint64_t *src = lwe_small + audit_row(seed, launch, m, S, s) * n1;
    uint64_t *dst = audit_in + (uint64_t)s * n1;
    for (uint32_t j = threadIdx.x; j < n1; j += AUDIT_THREADS) dst[j] = src[j];
}

// grid S, AUDIT_THREADS threads: the row_words words at out + row(s) out_stride against those at audit_out + s row_words (K2: the kN + 1 words
// of a ciphertext, out_stride = row_words; K1: n + 1 words; K3: the k + 1 key blocks, or the one of a single-block launch).  Rows are
// 8-byte aligned only (kN + 1 is odd): 8-byte loads, consecutive lanes on consecutive words.  The first differing word is a minimum in
// LDS; a wrong row takes a ticket from the wrong-row counter and, while the ticket is below AUDIT_RECORDS, writes its record.
__global__ __launch_bounds__(AUDIT_THREADS) void audit_compare_kernel(const uint64_t *out, uint64_t out_stride, const uint64_t *audit_out, uint32_t row_words,
                                                                      uint64_t seed, uint64_t launch, uint64_t m, uint32_t S, uint64_t *state)
{
    __shared__ unsigned first;
    const uint32_t s = blockIdx.x;
    const uint64_t row = audit_row(seed, launch, m, S, s);
    const uint64_t *got = out + row * out_stride, *want = audit_out + (uint64_t)s * row_words;
    if (threadIdx.x == 0) first = 0xFFFFFFFFu;
    __syncthreads();
    unsigned mine = 0xFFFFFFFFu;
    for (uint32_t j = threadIdx.x; j < row_words; j += AUDIT_THREADS)
        if (got[j] != want[j] && j < mine) mine = j;
    if (mine != 0xFFFFFFFFu) atomicMin(&first, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (s == 0) {
        atomicAdd((unsigned long long *)&state[AUDIT_ST_LAUNCHES], 1ull);
        atomicAdd((unsigned long long *)&state[AUDIT_ST_CHECKED], (unsigned long long)S);
    }
    const unsigned w = first;
    if (w == 0xFFFFFFFFu) return;
    const unsigned long long ticket = atomicAdd((unsigned long long *)&state[AUDIT_ST_WRONG], 1ull);
    if (ticket >= AUDIT_RECORDS) return;
    uint64_t *rec = state + AUDIT_ST_RECORDS + ticket * AUDIT_RECORD_WORDS;
    rec[0] = launch; rec[1] = row; rec[2] = w; rec[3] = got[w]; rec[4] = want[w];
}

// one thread: out[row][word] ^= mask (fheaes_audit_debug); the host has checked row < m and word < big1
__global__ void audit_tamper_kernel(uint64_t *out, uint32_t big1, uint64_t row, uint32_t word, uint64_t mask)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) out[row * big1 + word] ^= mask;
}

// ---- the plain form of the key switches (K1, K3) -----------------------------------------------------------------------------------
// The B fragments (kern_keyswitch.h): [z][kstep][column tile of 16][byte plane j][lane 64][16 B], lane l holding byte j of the key words of
// column 16 C + l % 16 in rows 64 kstep + 16 (l / 16) + e, e < 16.  A wave owns one column tile: per K step a lane takes the eight 16 B loads
// of its column and row quarter, recombines 16 key words and multiply-adds them into the accumulators of the workgroup's R rows; the four
// row quarters of a column meet in two lane exchanges at the end.  The four waves of a workgroup own four neighbouring column tiles and
// share the digits: 64 rows of the product x R ciphertexts per K step, recomputed from the input words into LDS (two tiles, so one barrier
// per K step).  Grid: x over the groups of R rows, y over the groups of four column tiles, z over the key blocks; the row groups are the
// fastest index, so the workgroups in flight read the same key bytes.  The fragments are padded with zero bytes; nothing here relies on
// it: digits are taken for rows < Q = n_in LEVELS only, input words read below n_in, columns stored below ncols, rows below S.
#define KSP_THREADS 256
#define KSP_COL_TILES (KSP_THREADS / 64)
#define KSP_KSTEP 64            /* KS_KSTEP */
#define KSP_NO_ROW (~0ull)

typedef int ksp_int4 __attribute__((ext_vector_type(4)));

struct KeyswitchPlainArgs {
    const uint64_t *in;        // row r: in + r in_stride, words 0 .. n_in - 1 decomposed
    uint64_t in_stride;
    uint32_t n_in;
    const int8_t *bfrag;       // [z][ksteps][coltiles][8][64][16]
    uint32_t ksteps, coltiles, ncols;
    int32_t body_index;        // >= 0: in[r][body_index] is added to column body_col; < 0: none
    uint32_t body_col;
    uint64_t *out;             // sample s, key block z, column o at out[s out_stride + z out_z_stride + o]
    uint64_t out_stride, out_z_stride;
    uint64_t seed, launch, m;  // sampled: sample s is row audit_row(seed, launch, m, S, s) of `in`; else row s
    uint32_t S;
    int sampled;
};

template <int BASE_LOG, int LEVELS, int R>
__global__ __launch_bounds__(KSP_THREADS) void keyswitch_plain_kernel(const KeyswitchPlainArgs A)
{
    __shared__ __attribute__((aligned(16))) int dig[2][R][KSP_KSTEP];
    __shared__ uint64_t row_of[R];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t z = blockIdx.z;
    const uint64_t s0 = (uint64_t)blockIdx.x * R;
    const uint32_t C = blockIdx.y * KSP_COL_TILES + wave;
    const bool live = C < A.coltiles;                        // wave-uniform; a wave without a column tile still builds digits and meets the barriers
    const uint64_t Q = (uint64_t)A.n_in * LEVELS;
    if (threadIdx.x < R) {
        const uint64_t s = s0 + threadIdx.x;
        row_of[threadIdx.x] = s >= A.S ? KSP_NO_ROW : A.sampled ? audit_row(A.seed, A.launch, A.m, A.S, (uint32_t)s) : s;
    }
    __syncthreads();

    uint64_t acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0;

    for (uint32_t ks = 0; ks < A.ksteps; ++ks) {
        int (*tile)[KSP_KSTEP] = dig[ks & 1];
        const uint64_t q = (uint64_t)ks * KSP_KSTEP + lane;
        for (int r = (int)wave; r < R; r += KSP_COL_TILES) {
            const uint64_t row = row_of[r];
            int v = 0;
            if (row != KSP_NO_ROW && q < Q) {
                int d[LEVELS];
                decompose_all<BASE_LOG, LEVELS>(A.in[row * A.in_stride + q / LEVELS], d);
                const uint32_t l = (uint32_t)(q % LEVELS);
#pragma unroll
                for (int ll = 0; ll < LEVELS; ++ll) if ((uint32_t)ll == l) v = d[ll];
            }
            tile[r][lane] = v;
        }
        __syncthreads();                                      // the tile of step ks is whole; the tile of step ks - 1 is read no more after the next one
        if (!live) continue;
        const int8_t *b = A.bfrag + ((((uint64_t)z * A.ksteps + ks) * A.coltiles + C) * 8) * 1024 + (uint64_t)lane * 16;
        ksp_int4 w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const ksp_int4 *>(b + (uint64_t)j * 1024);
        uint64_t key[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            uint64_t x = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) x += (uint64_t)(int64_t)(int8_t)((uint32_t)w[j][e >> 2] >> (8 * (e & 3))) << (8 * j);
            key[e] = x;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const ksp_int4 *t = reinterpret_cast<const ksp_int4 *>(&tile[r][16 * (lane >> 4)]);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const ksp_int4 d = t[g];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r] += (uint64_t)(int64_t)d[e] * key[4 * g + e];
            }
        }
    }
    if (!live) return;
    const uint32_t col = C * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        unsigned long long v = acc[r];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        const uint64_t row = row_of[r];
        if (lane >= 16 || col >= A.ncols || row == KSP_NO_ROW) continue;
        uint64_t o = (uint64_t)0 - v;
        if (A.body_index >= 0 && col == A.body_col) o += A.in[row * A.in_stride + (uint32_t)A.body_index];
        A.out[(s0 + r) * A.out_stride + (uint64_t)z * A.out_z_stride + col] = o;
    }
}
