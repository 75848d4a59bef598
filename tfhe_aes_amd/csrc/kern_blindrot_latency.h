// kern_blindrot_latency.h -- K2 for SMALL batches (one AES block, key expansion, the counter-add chain).
//
// The throughput kernel (kern_blindrot16.h) walks the L decomposition levels one after the other so that three
// ciphertexts fit a workgroup; with at most a few hundred bits in flight the GPU is mostly empty and what counts
// is the length of the dependent chain of one iteration.  Here ONE ciphertext owns a 512-thread workgroup and all
// L x K1 digit polynomials of an iteration are transformed at once:
//   LDS                     the accumulator (K1 x 512 torus words) LIVES here, updated in place by the owner groups at the
//                           end of the iteration;
//   all 512 threads         thread j rebuilds coefficient j of d_p = acc_p * X^t - acc_p for every p, decomposes it once and
//                           writes the L digits into the tiles of the L x K1 digit polynomials;
//   groups 0..L*K1-1        group (l, p) transforms its digit polynomial in tile (l, p);
//   all 512 threads         multiply-accumulate: thread = (Fourier point, share of the K1 output columns); the whole
//                           L*K1-row chain (same order as everywhere: least significant level first, rows ascending);
//   groups 0..K1-1          inverse transform of output polynomial c, accumulate into LDS.
// Round 2: the chain of an iteration was dominated by exposed round trips, not by arithmetic -- 25 dependent GGSW
// row fetches with two rows in flight (~600 cycles each), and one LDS table read in flight per twiddle multiply.  Now
//   * nothing is held across the transform, three levels of rows are requested at once behind it (BL_ROWS_AHEAD, below) -- one
//     exposed L2 round trip per iteration instead of one per level;
//   * the multiply-accumulate is split by output column over all 512 threads (3 + 2 columns), halving its length and
//     the registers a row occupies; key rows come through raw buffer loads with scalar row offsets;
//   * the transform's table entries are read as one batch, a whole pass ahead of their use (fft_dev.h);
//   * the accumulator no longer has a register copy (64 VGPRs, and the publish step with its barrier, are gone).
// 4 workgroup barriers and 2 transform passes per iteration (11 and 6 in the throughput kernel).  Same arithmetic as
// the throughput kernel: results are bit-identical (tests/test_gpu_stages.py::test_k2_blind_rotation covers both).
#pragma once
#include <type_traits>
#include "fft_dev.h"
#include "kern_extprod.h"

#define BL_THREADS 512
#define BL_ROWS_AHEAD 3      /* levels of GGSW rows in flight during the multiply-accumulate: nothing is held across the transform; when its registers
                                are free the rows of levels 0, 1 and 2 are requested at once (three register sets), level k+3 refills the set level k
                                has just left, row by row: one exposed L2 round trip per iteration.  With one level in flight (rounds 2-5) the stamps
                                of round 6 (profiles/r06_latency_stamps_before.txt) show the phase waiting a whole (hot-spotted: every workgroup walks
                                the same rows at the same time) round trip per level: 9.7 k of an iteration's 25.6 k cycles for 300 fused
                                multiply-adds per thread */

template <int K1, int LEVELS, int BASE_LOG>
__global__ __launch_bounds__(BL_THREADS, 2) void blind_rotate_latency_kernel(const ExtProdArgs A)
{
    constexpr int ROWS = LEVELS * K1;
    constexpr int CA = (K1 + 1) / 2, CB = K1 - CA;        // output columns of threads 0..255 / 256..511
    static_assert(ROWS <= BL_THREADS / 16, "one lane group per digit polynomial");
    constexpr int LDS_DOUBLES = 2 * FHE_TW_ENTRIES + ROWS * GROUP_TILE_DOUBLES + K1 * FHE_N;
    __shared__ __attribute__((aligned(16))) double lds_all[LDS_DOUBLES];
    double2 *tw = reinterpret_cast<double2 *>(lds_all);                                        // table first: 16-bit offsets reach it
    double *lds = lds_all + 2 * FHE_TW_ENTRIES;                                                 // ROWS tiles
    uint64_t *accs = reinterpret_cast<uint64_t *>(lds + ROWS * GROUP_TILE_DOUBLES);            // [K1][512]

    const int tid = threadIdx.x;
    const int g = tid >> 4;
    const bool transform = g < ROWS;                  // group (l_idx, p): row index g = k*K1 + p, k = 0 is the least significant level
    const bool owner = g < K1;                        // output polynomial g is inverse-transformed by this group
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: what depends on it stays in SGPRs / scalar branches
    const bool half_b = wave_id >= 4;                 // multiply-accumulate role: columns CA..K1-1 (wave-uniform)

    ep_load_table(tw, A.tw);

    const uint64_t inst = blockIdx.x;                 // one ciphertext per workgroup, grid = count
    const uint64_t *lwe = A.lwe_in + inst * (uint64_t)(A.iters + 1);

    // accumulator init, straight into LDS
    {
        const int bt = mod_switch_1024(lwe[A.iters] + A.body_shift);
        const int t = (1024 - bt) & 1023;
        for (int j = tid; j < K1 * FHE_N; j += BL_THREADS) {
            const int p = j >> 9, c = j & 511;
            const int e = ((c - t) & 511) + t;
            const uint64_t v = ((e >> 9) & 1) ? (uint64_t)0 - A.tv_const : A.tv_const;
            accs[j] = (p == K1 - 1) ? v : 0;
        }
    }
    __syncthreads();

    constexpr unsigned GGSW_BYTES = LEVELS * K1 * K1 * FHE_H * 16;
    const __amdgpu_buffer_rsrc_t bsk_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double2 *>(A.ggsw), 0, (int)(A.iters * GGSW_BYTES), 0x00020000);
    // chain level k (0 = least significant) is GGSW storage level LEVELS-1-k; byte offset of its row p, column 0
    auto row_bytes = [&](int k, int p) -> unsigned { return (unsigned)(((LEVELS - 1 - k) * K1 + p) * K1) * (FHE_H * 16); };
    uint64_t a_next = lwe[0];
#ifdef EP_STAMPS
    unsigned long long ph_cyc[EP_NPH];
    for (int i = 0; i < EP_NPH; ++i) ph_cyc[i] = 0;
    unsigned long long t_last = __builtin_readcyclecounter();
#endif

    unsigned pf_sink = 0;
    // GGSW rows per thread: (Fourier point tid mod 256) x (this half's share of the columns)
    const unsigned col_bytes = half_b ? (unsigned)CA * (FHE_H * 16) : 0u;      // wave-uniform
    for (uint32_t it = 0; it < A.iters; ++it) {
        const int t = mod_switch_1024(a_next);
        a_next = lwe[it + 1];                          // one iteration ahead (the last one reads the body: unused)
        const unsigned g_bytes = it * GGSW_BYTES, g_next = g_bytes + GGSW_BYTES;
        int tq = tid;
        asm volatile("" : "+v"(tq));                   // addresses below are recomputed from this, not kept across iterations
        const int bq_ = tq & 15, mp = tq & 255;
        double *tile = lds + (transform ? (tq >> 4) : 0) * GROUP_TILE_DOUBLES;

        // ---- 1a. d = acc * X^t - acc and its gadget decomposition, ONCE per coefficient: thread j owns coefficient j of every
        //      polynomial and writes the L digits (as doubles) into the tiles of the (level, polynomial) groups that transform
        //      them.  (Round-2 first form: each of the L groups of a polynomial rebuilt d and peeled down to its own level -- five
        //      times the integer work, and the deepest groups set the length of the iteration.)
        {
            const int s0 = (tq - t) & 511;
            const bool neg = ((s0 + t) >> 9) & 1;
            uint64_t rv[K1], ra[K1];
#pragma unroll
            for (int p = 0; p < K1; ++p) { rv[p] = accs[p * FHE_N + s0]; ra[p] = accs[p * FHE_N + tq]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < K1; ++p) {
                uint64_t v = rv[p];
                if (neg) v = (uint64_t)0 - v;
                v -= ra[p];
                uint32_t st;
                int d = decompose_first<BASE_LOG, LEVELS>(v, st);
#pragma unroll
                for (int k = 0; k < LEVELS; ++k) {
                    if (k) d = decompose_next<BASE_LOG>(st);
                    lds[(k * K1 + p) * GROUP_TILE_DOUBLES + tq] = (double)d;
                }
            }
        }
        EP_STAMP(1);
        wg_barrier_lds_only();                         // digits of every level in place
        EP_STAMP(11);
        // ---- 1c. in a small batch every workgroup is at the same iteration, so the first touch of a GGSW would be a DRAM round trip
        //      on the multiply-accumulate's critical path.  The workgroups that share an XCD (dealt to the 8 XCDs round-robin) walk
        //      the NEXT iteration's GGSW between them, one dword per 128-byte line, an iteration ahead of its use.  Nobody waits
        //      for these loads: their values are folded into a dead sink after the multiply-accumulate, by when they have landed.
        unsigned pf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) pf[i] = 0;
        if (it + 1 < A.iters) {
            const unsigned nshare = gridDim.x >= 64 ? 8u : gridDim.x >= 32 ? 4u : gridDim.x >= 16 ? 2u : 1u;   // scalar
            const unsigned mine = (blockIdx.x >> 3) % nshare;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((unsigned)i * nshare < 8u)
                    pf[i] = __builtin_amdgcn_raw_buffer_load_b32(bsk_rsrc, (mine + nshare * ((unsigned)tq + 512u * i)) * 128u, g_next, 0);
        }
        // ---- 1b. every (level, polynomial) group transforms its digit polynomial ------------------------------------------
        if (transform) {
            double xr[16], xi[16];
            double2 w0[8], w1[8];
            fft_fwd_table(w0, w1, tw, bq_);            // lands during the coefficient reads and the first pass
#pragma unroll
            for (int a = 0; a < 16; ++a) { xr[a] = tile[16 * a + bq_]; xi[a] = tile[256 + 16 * a + bq_]; }
            wave_lds_sync();                           // the group's lanes have their coefficients before the transform reuses the tile
            nega_fwd_head(xr, xi, w0, w1);
            nega_fwd_tail(xr, xi, tile, bq_);
            EP_STAMP(2);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                double2 v; v.x = xr[k2]; v.y = xi[k2];
                *reinterpret_cast<double2 *>(tile + 2 * (bq_ + 16 * k2)) = v;
            }
        }
        // ---- 2. multiply-accumulate: all 512 threads, one Fourier point and a share of the columns each.  The two halves of the
        //      workgroup own 3 and 2 columns (k + 1 = 5): each half runs its OWN copy of the phase with the column count a compile-time
        //      constant and its own row registers (with one shared copy and a per-column `if (half_b)` the compiler sinks the conditional
        //      column's products of all 25 rows of the unrolled chain into one block and keeps every row alive until then: 179 spills) ----
        double fr[CA], fi[CA];
#pragma unroll
        for (int c = 0; c < CA; ++c) { fr[c] = 0.0; fi[c] = 0.0; }
        auto mac_phase = [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            auto load_row_n = [&](unsigned gb, int k, int p, double2 (&dst)[NC]) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    dst[c] = ep_key_load(bsk_rsrc, (unsigned)mp * 16u, gb + row_bytes(k, p) + col_bytes + (unsigned)c * (FHE_H * 16));
            };
            // one chain level: rows p = 0..K1-1 out of `cur`; after row p is consumed its registers take row p of level k + BL_ROWS_AHEAD
            auto mac_level = [&](const int k, double2 (&cur)[K1][NC]) {
                const double *dl = lds + (size_t)k * K1 * GROUP_TILE_DOUBLES + 2 * mp;      // digits of chain level k
                double2 dn = *reinterpret_cast<const double2 *>(dl);
#pragma unroll
                for (int p = 0; p < K1; ++p) {
                    double2 bv[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) bv[c] = cur[p][c];
                    if (k + BL_ROWS_AHEAD < LEVELS) load_row_n(g_bytes, k + BL_ROWS_AHEAD, p, cur[p]);      // the same row, BL_ROWS_AHEAD levels on
                    const double2 d = dn;
                    if (p + 1 < K1) dn = *reinterpret_cast<const double2 *>(dl + (p + 1) * GROUP_TILE_DOUBLES);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        fr[c] = __builtin_fma(d.x, bv[c].x, fr[c]);
                        fr[c] = __builtin_fma(-d.y, bv[c].y, fr[c]);
                        fi[c] = __builtin_fma(d.x, bv[c].y, fi[c]);
                        fi[c] = __builtin_fma(d.y, bv[c].x, fi[c]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            // the transform's registers are free: the rows of the first three levels are requested at once (they land behind the barrier)
            double2 rows[3][K1][NC];
            __builtin_amdgcn_sched_barrier(0);         // not earlier: during the transform there is no register to spare
#pragma unroll
            for (int k = 0; k < 3 && k < LEVELS; ++k)
#pragma unroll
                for (int p = 0; p < K1; ++p) load_row_n(g_bytes, k, p, rows[k][p]);
            __builtin_amdgcn_sched_barrier(0);
            EP_STAMP(3);
            wg_barrier_lds_only();                     // digits visible; the key loads stay in flight
            EP_STAMP(4);
#pragma unroll
            for (int k = 0; k < LEVELS; ++k) mac_level(k, rows[k % 3]);
        };
        if (half_b) mac_phase(std::integral_constant<int, CB>{}); else mac_phase(std::integral_constant<int, CA>{});
#pragma unroll
        for (int i = 0; i < 8; ++i) pf_sink ^= pf[i];
        EP_STAMP(5);
        wg_barrier_lds_only();                         // all digits consumed: tiles 0..K1-1 may take the products
        EP_STAMP(6);
#pragma unroll
        for (int c = 0; c < CA; ++c) {
            if (c < CB || !half_b) {
                double2 v; v.x = fr[c]; v.y = fi[c];
                *reinterpret_cast<double2 *>(lds + ((half_b ? CA : 0) + c) * GROUP_TILE_DOUBLES + 2 * mp) = v;
            }
        }
        EP_STAMP(7);
        wg_barrier_lds_only();
        EP_STAMP(8);
        // ---- 3. owner groups: inverse transform of output polynomial g; the result (still doubles) goes back to the tile in
        //      coefficient order.  Conversion to the torus and the accumulate are spread over all 512 threads below (on the five
        //      owner groups alone they were a third of this phase, with everyone else waiting).
        if (owner) {
            double xr[16], xi[16];
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                double2 v = *reinterpret_cast<const double2 *>(tile + 2 * (bq_ + 16 * k2));
                xr[k2] = v.x; xi[k2] = v.y;
            }
            wave_lds_sync();
            nega_inv(xr, xi, tw, tile, bq_);
            wave_lds_sync();                           // the transform's last reads of the tile are done in every lane of the group
#pragma unroll
            for (int a = 0; a < 16; ++a) { tile[16 * a + bq_] = xr[a]; tile[256 + 16 * a + bq_] = xi[a]; }
        }
        EP_STAMP(9);
        wg_barrier_lds_only();                         // results of all K1 polynomials in place
        // ---- 4. all threads: thread j converts and accumulates coefficient j of every polynomial ------------------------
#pragma unroll
        for (int p = 0; p < K1; ++p) accs[p * FHE_N + tq] += torus_from_double(lds[p * GROUP_TILE_DOUBLES + tq]);
        EP_STAMP(0);
        wg_barrier_lds_only();                         // accumulator complete before the next iteration's rotation reads it
        EP_STAMP(10);
    }
#ifdef EP_STAMPS
    if (A.stamps && (tid & 63) == 0)
        for (int i = 0; i < EP_NPH; ++i) A.stamps[((size_t)blockIdx.x * 8 + (tid >> 6)) * EP_NPH + i] = ph_cyc[i];
#endif

    // ---- sample extract coefficient 0, from the LDS accumulator -------------------------------------
    {
        const uint64_t big = (uint64_t)(K1 - 1) * FHE_N;
        uint64_t *o = A.out + inst * (big + 1);
        for (int j = tid; j < (K1 - 1) * FHE_N; j += BL_THREADS) {
            const int p = j >> 9, c = j & 511;
            const uint64_t v = accs[j];
            if (c == 0) o[(uint64_t)p * FHE_N] = v; else o[(uint64_t)p * FHE_N + FHE_N - c] = (uint64_t)0 - v;
        }
        if (tid == 0) o[big] = accs[(K1 - 1) * FHE_N] + A.post_add;
        if (pf_sink == 0x9e3779b9u && A.count == 0) o[0] = pf_sink;      // keeps the prefetch loads alive; never true
    }
}
