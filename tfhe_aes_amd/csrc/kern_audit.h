// kern_audit.h -- the audit of the blind rotation (fheaes_audit_set): S sampled rows of a K2 launch are run again through the latency form
// (kern_blindrot_latency.h: no parking, no slot pool, no owner words, no generation plan) and the two results are compared on the device,
// bit for bit.  The engine is deterministic and every form writes the same words (tests/test_gpu_k2_shapes.py), so a difference is a defect
// of the engine or of the machine and never noise.  Three small kernels around the context's own latency-form launch:
//   audit_gather_kernel    workgroup s copies the small LWE of its sampled row (n + 1 words) into audit_in[s];
//   (the latency form)     audit_in -> audit_out, count = S;
//   audit_compare_kernel   workgroup s compares audit_out[s] with row audit_row(s) of the product launch's output (kN + 1 words), counts a
//                          wrong row and keeps a record of the first AUDIT_RECORDS of them;
//   audit_tamper_kernel    the test hook (fheaes_audit_debug): one thread XORs a mask into one word of the product launch's output.
// 2 x 16 KB per row: nothing here is near any roof.
#pragma once
#include <stdint.h>

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

// grid S, AUDIT_THREADS threads: out[row(s)] against audit_out[s] over big1 = kN + 1 words.  Rows are 8-byte aligned only (big1 is odd):
// 8-byte loads, consecutive lanes on consecutive words.  The first differing word is a minimum in LDS; a wrong row takes a ticket from
// the wrong-row counter and, while the ticket is below AUDIT_RECORDS, writes its record.
__global__ __launch_bounds__(AUDIT_THREADS) void audit_compare_kernel(const uint64_t *out, const uint64_t *audit_out, uint32_t big1, uint64_t seed, uint64_t launch,
                                                                      uint64_t m, uint32_t S, uint64_t *state)
{
    __shared__ unsigned first;
    const uint32_t s = blockIdx.x;
    const uint64_t row = audit_row(seed, launch, m, S, s);
    const uint64_t *got = out + row * big1, *want = audit_out + (uint64_t)s * big1;
    if (threadIdx.x == 0) first = 0xFFFFFFFFu;
    __syncthreads();
    unsigned mine = 0xFFFFFFFFu;
    for (uint32_t j = threadIdx.x; j < big1; j += AUDIT_THREADS)
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
