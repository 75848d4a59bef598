// kern_gate.h -- the gate: out = GGSW_g (x) in, one single-level external product with a zero "else" branch.  A ciphertext times the
// encrypted bit g that a circuit bootstrap turned into a Fourier GGSW: what multiplies a plaintext, a key or a whole packed GLWE by the
// `valid` bit of a tag check (fheaes_gate_ggsw, fheaes_gate_bits, fheaes_gate_packed).
//
// The product itself is ep_product_once (kern_extprod.h), the one cmux_level_kernel calls, here with ct0 = 0: 16 lane-groups of 16, group
// g < R*K1 owns polynomial g % K1 of instance g / K1.  All R instances of a workgroup share ONE gate, so each GGSW element fetched serves
// R instances; which gate, which instances and how many (<= R) come from a table the host builds from the caller's runs (GateWg).
//
// Two input forms:
//   GATE_LWE   in / out [m][kN+1].  The LWE ciphertext (a, b) is embedded on load into the GLWE whose coefficient 0 is that ciphertext,
//              the inverse of sample_extract_kernel at index 0: mask polynomial p has a[pN] at coefficient 0 and -a[pN + N - j] at
//              j = 1..N-1, the body polynomial is b at coefficient 0 and zero elsewhere.  The negation comes BEFORE the decomposition
//              (a tie word and its negative round differently).  On store coefficient 0 is extracted again: kN+1 words per instance,
//              never a GLWE in memory.
//   GATE_GLWE  in / out [G][(k+1)N] packed GLWEs (fheaes_pack_bits), one instance per GLWE, all N coefficients stored.
// In place (out == in) is safe: every row is read before the workgroup's first barrier and written after its last by the one
// workgroup that owns it.  A ragged last workgroup of a gate clamps its loads to the gate's last instance and masks its stores.
#pragma once
#include "kern_extprod.h"

#define GATE_LWE 0
#define GATE_GLWE 1

// one workgroup's share of a gate's run: instances first .. first + count - 1 (1 <= count <= R) under GGSW `gate`
struct GateWg {
    uint64_t first;
    uint32_t gate, count;
};

struct GateArgs {
    const double2 *ggsw;        // Fourier GGSWs [n_gates][K1][K1][256] (one decomposition level)
    const double2 *tw;          // [FHE_TW_ENTRIES] the transform's one table (fft_dev.h)
    const GateWg *wgs;          // [grid] (already offset to this launch's first workgroup)
    const uint64_t *in;         // GATE_LWE [m][kN+1], GATE_GLWE [G][K1][512]
    uint64_t *out;              // same shape; may be `in`
};

template <int K1, int BASE_LOG, int R, int FORM>
__global__ __launch_bounds__(EP_THREADS, 2) void gate_kernel(const GateArgs A)
{
    static_assert(R * K1 <= EP_GROUPS, "too many polynomials for 16 lane groups");
    static_assert(FORM == GATE_LWE || FORM == GATE_GLWE, "input form");
    __shared__ __attribute__((aligned(16))) double lds[EP_LDS_DOUBLES];
    double2 *tw = reinterpret_cast<double2 *>(lds + EP_GROUPS * GROUP_TILE_DOUBLES);
    const int tid = threadIdx.x;
    const int g = tid >> 4, b = tid & 15;
    const bool owner = g < R * K1;
    const int r_own = owner ? g / K1 : R - 1;
    const int p_own = owner ? g % K1 : K1 - 1;
    double *tile = lds + g * GROUP_TILE_DOUBLES;
    ep_load_table(tw, A.tw);

    const GateWg W = A.wgs[blockIdx.x];
    const bool valid = owner && (uint32_t)r_own < W.count;
    const uint64_t inst = W.first + ((uint32_t)r_own < W.count ? (uint32_t)r_own : W.count - 1);     // idle slots repeat the last instance
    constexpr uint64_t BIG = (uint64_t)(K1 - 1) * FHE_N;

    double xr[16], xi[16];
    if (FORM == GATE_LWE) {
        const uint64_t *ct = A.in + inst * (BIG + 1);
        if (p_own < K1 - 1) {
            const uint64_t *am = ct + (uint64_t)p_own * FHE_N;
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                const int j0 = 16 * a + b, j1 = j0 + 256;
                const uint64_t v0 = j0 == 0 ? am[0] : (uint64_t)0 - am[FHE_N - j0];
                const uint64_t v1 = (uint64_t)0 - am[FHE_N - j1];
                uint32_t st;
                xr[a] = (double)decompose_first<BASE_LOG, 1>(v0, st);
                xi[a] = (double)decompose_first<BASE_LOG, 1>(v1, st);
            }
        } else {
            const uint64_t body = ct[BIG];
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                uint32_t st;
                xr[a] = (double)decompose_first<BASE_LOG, 1>((a == 0 && b == 0) ? body : (uint64_t)0, st);
                xi[a] = (double)decompose_first<BASE_LOG, 1>((uint64_t)0, st);
            }
        }
    } else {
        const uint64_t *src = A.in + (inst * K1 + p_own) * FHE_N;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            uint32_t st;
            xr[a] = (double)decompose_first<BASE_LOG, 1>(src[16 * a + b], st);
            xi[a] = (double)decompose_first<BASE_LOG, 1>(src[256 + 16 * a + b], st);
        }
    }
    __syncthreads();   // tables visible; every row of the workgroup has been read (in place)
    ep_product_once<K1, R>(xr, xi, A.ggsw, W.gate, lds, tw, tile, tid, b);
    if (!valid) return;
    if (FORM == GATE_LWE) {
        // sample extract coefficient 0 (sample_extract_kernel's rule at i = 0)
        uint64_t *o = A.out + inst * (BIG + 1);
        if (p_own < K1 - 1) {
            uint64_t *om = o + (uint64_t)p_own * FHE_N;
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                const int j0 = 16 * a + b, j1 = j0 + 256;
                if (j0 == 0) om[0] = torus_from_double(xr[a]); else om[FHE_N - j0] = (uint64_t)0 - torus_from_double(xr[a]);
                om[FHE_N - j1] = (uint64_t)0 - torus_from_double(xi[a]);
            }
        } else if (b == 0) {
            o[BIG] = torus_from_double(xr[0]);
        }
    } else {
        uint64_t *o = A.out + (inst * K1 + p_own) * FHE_N;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            o[16 * a + b] = torus_from_double(xr[a]);
            o[256 + 16 * a + b] = torus_from_double(xi[a]);
        }
    }
}
