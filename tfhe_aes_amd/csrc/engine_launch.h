// engine_launch.h -- how a batch becomes kernel launches: the blind rotation's launch plan, one launcher per kernel of kern_*.h,
// the noise guard of the linear layers, and many_wopbs_without_padding on device buffers (many_wopbs.rs:31-116).
#pragma once

#define MAX_CHUNK_BITS 32768ull
#define K2_CALL_MAX_BITS 65536ull      /* bits per blind-rotation launch of fheaes_cbs_pbs_batch: at most 32,768 workgroups' parking, 64 KB each */
#define MAX_WOPBS_BITS 16u            /* widest radix input of many_wopbs_without_padding (LUT of 2^16 entries per output bit) */

namespace {

// ---- how a blind-rotation batch is cut into workgroups (fheaes_k2_launch_plan) -------------------------------------------------
#define LATENCY_BATCH_BITS 256ull      /* at most one 512-thread workgroup per CU */
#define K2_PAIR_MIN_BITS 768ull        /* batches above this take the paired form (kern_blindrot_pair.h): one 512-thread workgroup per CU */
struct K2Plan { int form; uint64_t units_main; uint32_t r_main; uint64_t units_tail; uint32_t r_tail; };
K2Plan k2_plan(uint64_t m, uint32_t cu_count, uint32_t k1, bool allow_pair = true)
{
    K2Plan pl{};
    if (m <= LATENCY_BATCH_BITS) { pl.form = 0; pl.units_main = m; pl.r_main = 1; return pl; }
    if (allow_pair && k1 == 5 && m > K2_PAIR_MIN_BITS) {
        // paired form: units of 6 and of 4 ciphertexts, one workgroup per CU, a whole number of generations that covers the batch
        // (16,384 bits = 2,560 x 6 + 256 x 4 = 11 generations; 4,096 = 512 x 6 + 256 x 4 = 3; 1,152 = 64 x 6 + 192 x 4 = 1); the
        // smaller units last: the last generation is filled with four-ciphertext units on every CU instead of covering fewer CUs
        // with six-ciphertext ones (measured at 4,096 bits)
        pl.form = 2; pl.r_main = 6; pl.r_tail = 4;
        const uint64_t gens = (m + 6ull * cu_count - 1) / (6ull * cu_count);
        uint64_t nu = gens * cu_count;
        uint64_t four = 6 * nu >= m ? (6 * nu - m) / 2 : 0;      // units that can give up two of their six slots
        if (four > nu) four = nu;
        if (four == nu && 4 * nu > m) { nu = (m + 3) / 4; four = nu; }          // less than one generation of 4-ciphertext units
        pl.units_tail = four; pl.units_main = nu - four;
        return pl;
    }
    pl.form = 1;
    pl.r_main = k1 == 5 ? 3 : 8;
    pl.units_main = (m + pl.r_main - 1) / pl.r_main;
    if (k1 == 5) {
        const uint64_t slots = 2ull * cu_count;
        pl.r_tail = 2;
        if ((m + 1) / 2 <= cu_count) {
            // at most one two-ciphertext unit per CU: shorter units than three-ciphertext ones, still one per CU
            pl.units_main = 0;
            pl.units_tail = (m + 1) / 2;
        } else if (pl.units_main > slots) {
            // more units than slots (two workgroups per CU): a whole number of generations of 3- and 2-ciphertext units that
            // cover the batch exactly, the 2-ciphertext ones last (see blind_rotate16_kernel)
            const uint64_t nu = slots * ((m + 3 * slots - 1) / (3 * slots));
            if (2 * nu <= m) {
                pl.units_tail = 3 * nu - m;
                pl.units_main = nu - pl.units_tail;
            }
        }
    }
    return pl;
}

// ---- how the block-rounds of an AES call are cut into blind-rotation launches (fheaes_aes_window_plan) ----------------------------
// A block cipher call is `steps` WoPBS over each of n blocks of 128 bits, and a step of block b needs only the step before it of the same
// block: the steps x n block-rounds are one stream in (step, block) order that may be cut anywhere.  Round by round, every step pays the
// launch's last, partly filled generation; cut into windows that are a whole number of six-ciphertext generations, only the call's last
// launch does.
#define AES_BLOCK_BITS 128ull
#define AES_WINDOW_MAX_BLOCKS (MAX_CHUNK_BITS / AES_BLOCK_BITS)
struct AesWindowPlan { uint64_t window, launches, generations, generations_by_round; };      // window 0: not rolled, one WoPBS per step

// generations of one workgroup per CU that a paired launch of m bits runs; a launch at or below the paired threshold counts as one
uint64_t k2_generations(uint64_t m, uint32_t cu_count, uint32_t k1)
{
    if (m == 0) return 0;
    if (m <= K2_PAIR_MIN_BITS) return 1;
    const K2Plan pl = k2_plan(m, cu_count, k1);
    return (pl.units_main + pl.units_tail + cu_count - 1) / cu_count;
}

// launches and generations of the stream cut into windows of w blocks (w <= n, w <= AES_WINDOW_MAX_BLOCKS)
void aes_window_count(uint64_t n, uint64_t steps, uint64_t w, uint32_t cu_count, uint32_t k1, uint64_t *launches, uint64_t *generations)
{
    const uint64_t total = steps * n, full = total / w, rest = total % w;
    *launches = full + (rest ? 1 : 0);
    *generations = full * k2_generations(w * AES_BLOCK_BITS, cu_count, k1) + k2_generations(rest * AES_BLOCK_BITS, cu_count, k1);
}

// pair: the full batch's launch takes the paired form on the device in question (k2_launch: after the occupancy fallbacks and the hook)
AesWindowPlan aes_window_plan(uint64_t n, uint64_t steps, uint32_t cu_count, uint32_t k1, bool allow_pair = true)
{
    AesWindowPlan pl{};
    // round by round: every step is cut into chunks of MAX_CHUNK_BITS (wopbs_dev)
    const uint64_t chunks = n / AES_WINDOW_MAX_BLOCKS, last = n % AES_WINDOW_MAX_BLOCKS;
    pl.launches = steps * (chunks + (last ? 1 : 0));
    pl.generations_by_round = steps * (chunks * k2_generations(MAX_CHUNK_BITS, cu_count, k1) + k2_generations(last * AES_BLOCK_BITS, cu_count, k1));
    pl.generations = pl.generations_by_round;
    if (n == 0 || steps == 0) return pl;
    const uint64_t gen_bits = 6ull * cu_count;
    if (k2_plan(std::min<uint64_t>(n * AES_BLOCK_BITS, MAX_CHUNK_BITS), cu_count, k1, allow_pair).form != 2) return pl;
    if (n * AES_BLOCK_BITS % gen_bits == 0) return pl;
    // the smallest block count whose bits are whole generations: lcm(128, 6 CUs) / 128 = 6 CUs / gcd(128, 6 CUs)
    uint64_t g = AES_BLOCK_BITS, r = gen_bits;
    while (r) { const uint64_t t = g % r; g = r; r = t; }
    const uint64_t base = gen_bits / g;
    const uint64_t w = std::min<uint64_t>(n, AES_WINDOW_MAX_BLOCKS) / base * base;
    if (w == 0) return pl;
    uint64_t launches, generations;
    aes_window_count(n, steps, w, cu_count, k1, &launches, &generations);
    if (generations >= pl.generations_by_round) return pl;
    pl.window = w; pl.launches = launches; pl.generations = generations;
    return pl;
}

// ---- the audit behind a product launch (kern_audit.h, StageAudit) and the plain form of the key switches ---------------------------
static_assert(FHEAES_AUDIT_MAX_ROWS == AUDIT_MAX_ROWS && FHEAES_AUDIT_RECORDS == AUDIT_RECORDS, "include/fheaes.h and kern_audit.h disagree");
static_assert(KSP_KSTEP == KS_KSTEP, "kern_audit.h reads the B fragments of kern_keyswitch.h");
#define KSP_ROWS_K1 4          /* rows per workgroup: K1 has few column tiles (42 at PARAM_OPT), so more row groups */
#define KSP_ROWS_K3 8

// The audit of one product launch runs behind it on the same stream and inside its StageScope: the time counts into the stage, `launches`
// and `units` count the product launch alone.  Nothing is allocated (the set call did) and the host waits for nothing: a mismatch is learnt
// from the read call.  A launcher that finds StageAudit::wants(m) calls audit_begin, runs the stage's second form on the S sampled rows
// into au.out (row s of it: row_words words), and calls audit_compare.
struct AuditLaunch {
    StageAudit &au;
    uint64_t m, launch;          // rows of the product launch; its number among the stage's audited launches
    uint32_t S;                  // sampled rows: row audit_row(au.seed, launch, m, S, s) for s < S
    uint64_t *out;               // the product launch's output: row r is the row_words words at out + r out_stride
    uint64_t out_stride;
    uint32_t row_words;
};

// takes the launch number and fires the one-shot hook on the product launch's output
AuditLaunch audit_begin(fheaes_ctx *c, StageAudit &au, uint64_t m, uint64_t *out, uint64_t out_stride, uint32_t row_words)
{
    const AuditLaunch L{au, m, au.launch++, (uint32_t)std::min<uint64_t>(au.rows, m), out, out_stride, row_words};
    if (au.hook) {
        au.hook = false;                             // one shot; a row or a word beyond this launch's is dropped without a write
        if (au.hook_row < m && au.hook_word < row_words)
            hipLaunchKernelGGL(audit_tamper_kernel, dim3(1), dim3(1), 0, c->stream, out, (uint32_t)out_stride, au.hook_row, au.hook_word, au.hook_mask);
    }
    return L;
}

// the sampled rows of the product launch against au.out, counted and recorded in au.state
int audit_compare(fheaes_ctx *c, const AuditLaunch &L)
{
    hipLaunchKernelGGL(audit_compare_kernel, dim3(L.S), dim3(AUDIT_THREADS), 0, c->stream, L.out, L.out_stride, (const uint64_t *)L.au.out.p, L.row_words, L.au.seed,
                       L.launch, L.m, L.S, (uint64_t *)L.au.state.p);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// rows 0 .. a.S - 1 (or the a.S sampled rows) of key switch `stage` through the plain form, nz key blocks
void launch_keyswitch_plain(fheaes_ctx *c, int stage, const KeyswitchPlainArgs &a, unsigned nz)
{
    const unsigned gy = (a.coltiles + KSP_COL_TILES - 1) / KSP_COL_TILES;
    if (stage == FHEAES_STAGE_KEYSWITCH)
        hipLaunchKernelGGL((keyswitch_plain_kernel<2, 6, KSP_ROWS_K1>), dim3((a.S + KSP_ROWS_K1 - 1) / KSP_ROWS_K1, gy, nz), dim3(KSP_THREADS), 0, c->stream, a);
    else
        hipLaunchKernelGGL((keyswitch_plain_kernel<12, 3, KSP_ROWS_K3>), dim3((a.S + KSP_ROWS_K3 - 1) / KSP_ROWS_K3, gy, nz), dim3(KSP_THREADS), 0, c->stream, a);
}

// K1's key, dimensions and body term, and K3's key, dimensions and -- `block` >= 0: key block r = `block` alone -- the offset and z-stride
// of a single block, as the product kernels and the plain form take them; the caller adds afrag, in, out, out_stride (K3) and m
KeyswitchArgs keyswitch_k1_args(const fheaes_ctx *c)
{
    KeyswitchArgs a{};
    a.bfrag = c->ksk_frag; a.ksteps = c->ks_ksteps; a.coltiles = c->ks_coltiles;
    a.in_stride = c->big1; a.body_index = (int32_t)c->big; a.body_col = c->n; a.ncols = c->n + 1;
    a.out_stride = c->n + 1; a.out_z_stride = 0;
    return a;
}
KeyswitchArgs keyswitch_k3_args(const fheaes_ctx *c, int block)
{
    KeyswitchArgs a{};
    a.bfrag = c->pfpksk_frag; a.ksteps = c->pf_ksteps; a.coltiles = c->pf_coltiles;
    if (block >= 0) a.bfrag += (size_t)block * c->pf_ksteps * c->pf_coltiles * 8 * 1024;
    a.in_stride = c->big1; a.body_index = -1; a.body_col = 0; a.ncols = c->k1 * FHE_N;
    a.out_z_stride = block >= 0 ? 0 : a.ncols;
    return a;
}
unsigned keyswitch_k3_blocks(const fheaes_ctx *c, int block) { return block >= 0 ? 1 : c->k1; }

// what the plain form takes over from a product launch: its input, its key bytes, its real dimensions; n_in: the words of a row it
// decomposes; nz: the key blocks, whose nz ncols words make up a row of the plain form's output (K3 over all blocks: out_z_stride = ncols)
KeyswitchPlainArgs keyswitch_plain_args(const KeyswitchArgs &prod, uint32_t n_in, unsigned nz)
{
    KeyswitchPlainArgs a{};
    a.in = prod.in; a.in_stride = prod.in_stride; a.n_in = n_in;
    a.bfrag = prod.bfrag; a.ksteps = prod.ksteps; a.coltiles = prod.coltiles; a.ncols = prod.ncols;
    a.body_index = prod.body_index; a.body_col = prod.body_col;
    a.out_stride = (uint64_t)nz * prod.ncols; a.out_z_stride = nz > 1 ? prod.ncols : 0;
    return a;
}

// The audit of one key-switch launch.  `prod`: the product launch's arguments, nz its key blocks: a row's written words are the nz ncols
// words at out + row out_stride, and a record's `word` is the offset among them.
int launch_keyswitch_audit(fheaes_ctx *c, int stage, const KeyswitchArgs &prod, uint32_t n_in, unsigned nz)
{
    const AuditLaunch L = audit_begin(c, c->audit[stage], prod.m, prod.out, prod.out_stride, nz * prod.ncols);
    KeyswitchPlainArgs a = keyswitch_plain_args(prod, n_in, nz);
    a.out = (uint64_t *)L.au.out.p;
    a.seed = L.au.seed; a.launch = L.launch; a.m = L.m; a.S = L.S; a.sampled = 1;
    launch_keyswitch_plain(c, stage, a, nz);
    return audit_compare(c, L);
}

// ---- kernel launchers ------------------------------------------------------------------------
int launch_keyswitch(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t *out)
{
    if (m == 0) return FHEAES_OK;
    StageScope sc(c, FHEAES_STAGE_KEYSWITCH, m);
    const uint64_t ct_tiles16 = ((m + KS_CT_TILE - 1) / KS_CT_TILE) * (KS_CT_TILE / 16);
    TRY(ensure(c, c->ws_digits, ct_tiles16 * c->ks_ksteps * 1024));
    int8_t *af = (int8_t *)c->ws_digits.p;
    const uint64_t threads = ct_tiles16 * c->ks_ksteps * 64;
    ks_launch_digits_k1(dim3((unsigned)((threads + 255) / 256)), c->stream, in, (uint64_t)c->big1, c->big, m, c->ks_ksteps, af);
    KeyswitchArgs a = keyswitch_k1_args(c);
    a.afrag = af; a.in = in; a.out = out; a.m = m;
    // K1 through the LDS-tiled kernel too (round 6: 1.87 -> 1.48 ms per 16,384-bit launch, same words)
    dim3 grid((c->ks_coltiles + KSL_COL_TILES - 1) / KSL_COL_TILES, (unsigned)((m + 16 * KSL_CT_TILES - 1) / (16 * KSL_CT_TILES)), 1);
    ks_launch_mfma_lds(1, grid, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (c->audit[FHEAES_STAGE_KEYSWITCH].wants(m)) TRY(launch_keyswitch_audit(c, FHEAES_STAGE_KEYSWITCH, a, c->big, 1));
    return FHEAES_OK;
}

// out: rows of one GGSW level: [m][out_stride] with key r at offset r*(k+1)N.  `block` >= 0: key block r = `block` alone, its
// (k+1)N words at offset 0 of every row (block k is the LWE -> GLWE key of fheaes_pack_bits): a fifth of the matrix product
int launch_pfpks(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t *out, uint64_t out_stride, int block = -1)
{
    if (m == 0) return FHEAES_OK;
    StageScope sc(c, FHEAES_STAGE_PFPKS, m);
    const uint64_t ct_tiles16 = ((m + KS_CT_TILE - 1) / KS_CT_TILE) * (KS_CT_TILE / 16);
    TRY(ensure(c, c->ws_digits, ct_tiles16 * c->pf_ksteps * 2 * 1024));
    int8_t *af = (int8_t *)c->ws_digits.p;
    const uint64_t threads = ct_tiles16 * c->pf_ksteps * 64;
    ks_launch_digits_k3(dim3((unsigned)((threads + 255) / 256)), c->stream, in, (uint64_t)c->big1, c->big1, m, c->pf_ksteps, af);
    KeyswitchArgs a = keyswitch_k3_args(c, block);
    a.afrag = af; a.in = in; a.out = out; a.out_stride = out_stride; a.m = m;
    dim3 grid((c->pf_coltiles + KSL_COL_TILES - 1) / KSL_COL_TILES, (unsigned)((m + 16 * KSL_CT_TILES - 1) / (16 * KSL_CT_TILES)), keyswitch_k3_blocks(c, block));
    ks_launch_mfma_lds(2, grid, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (c->audit[FHEAES_STAGE_PFPKS].wants(m)) TRY(launch_keyswitch_audit(c, FHEAES_STAGE_PFPKS, a, c->big1, grid.z));
    return FHEAES_OK;
}

int launch_forward_fourier(fheaes_ctx *c, const uint64_t *in, uint64_t polys, double2 *out, int stage)
{
    if (polys == 0) return FHEAES_OK;
    StageScope sc(c, stage, polys);
    uint64_t wgs = (polys + EP_GROUPS - 1) / EP_GROUPS;
    if (wgs > 8192) wgs = 8192;
    hipLaunchKernelGGL(forward_fourier_kernel, dim3((unsigned)wgs), dim3(EP_THREADS), 0, c->stream, in, out, polys, c->tw_d);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// the paired kernel takes nearly all of a CU's LDS: where the runtime cannot place even one such workgroup (a driver that reserves LDS)
// every batch falls back to the 16-form instead of failing the launch.  fheaes_k2_set_forms can only take the form away: "queried and allowed"
bool k2_pair_allowed(fheaes_ctx *c)
{
    if (c->k2_deny_pair) return false;
    if (c->k2_pair_ok < 0) {
        int per_cu = 0;
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, blind_rotate_pair_kernel<5, 5, 8, 3, 2>, BRP_THREADS, 0);
        c->k2_pair_ok = (oe == hipSuccess && per_cu >= 1) ? 1 : 0;
        (void)hipGetLastError();
    }
    return c->k2_pair_ok == 1;
}

// the 16-form's LDS-home variant takes exactly half of a CU's 160 KB per workgroup: use it only where the runtime really places two
bool k2_home_allowed(fheaes_ctx *c)
{
    if (c->k1 != 5 || c->k2_deny_home) return false;
    if (c->k2_home < 0) {
        int per_cu = 0;
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, blind_rotate16_kernel<5, 5, 8, 3, 2, true>, EP_THREADS, 0);
        c->k2_home = (oe == hipSuccess && per_cu >= 2) ? 1 : 0;
        (void)hipGetLastError();         // a failed query means "fall back", not a failed launch
    }
    return c->k2_home == 1;
}

// the paired kernel's owner words (BRP_PARK_SLOTS x uint32) and the BRP_PARK_TAIL_WORDS uint64 behind them (fallbacks, ownership
// violations, record pointer).  Zeroed once, when allocated: the reset before every launch touches only the owner words, so the counters
// accumulate for the life of the context (fheaes_k2_park_read); the record pointer is set by the launches under the test hook and
// cleared by fheaes_k2_park_debug
static_assert(FHEAES_K2_PARK_SLOTS == BRP_PARK_SLOTS, "include/fheaes.h and kern_blindrot_pair.h disagree on the number of parking slots");
constexpr size_t PARK_OWNER_BYTES = BRP_PARK_SLOTS * sizeof(uint32_t) + BRP_PARK_TAIL_WORDS * sizeof(uint64_t);
constexpr size_t PARK_RECORD_PTR_OFFSET = BRP_PARK_SLOTS * sizeof(uint32_t) + 2 * sizeof(uint64_t);

int ensure_park_owner(fheaes_ctx *c)
{
    if (c->ws_park_owner.p) return FHEAES_OK;
    TRY(ensure(c, c->ws_park_owner, PARK_OWNER_BYTES));
    HIP_TRY(c, hipMemsetAsync(c->ws_park_owner.p, 0, PARK_OWNER_BYTES, c->stream));
    return FHEAES_OK;
}

// bytes of the paired kernel's parking slab for a launch of `grid` workgroups: claimed slots = the shared pool + one private overflow slot
// per workgroup behind it (never touched unless a pool is exhausted), private slots = one per workgroup
size_t k2_pair_park_bytes(const fheaes_ctx *c, uint64_t grid)
{
    return (size_t)((c->k2_park_claim ? BRP_PARK_SLOTS : 0) + grid) * 2 * BRP_PARK_WORDS_PER_HALF * 8;
}

// Everything a blind-rotation launch of m bits on this context comes to: the plan after the occupancy fallbacks, the kernel and its name,
// the grid, the parking slab.  launch_cbs_pbs launches from it, fheaes_reserve sizes from it, fheaes_k2_context_plan reports it.
struct K2Launch {
    K2Plan pl;
    void (*kernel)(ExtProdArgs);
    const char *name;
    unsigned grid, threads;
    size_t park_bytes;          // 0: the form parks nothing
    bool park_owner;            // the launch claims its parking slots through the owner words (ensure_park_owner)
};
K2Launch k2_launch(fheaes_ctx *c, uint64_t m)
{
    K2Launch L{};
    L.pl = k2_plan(m, c->cu_count, c->k1, k2_pair_allowed(c));
    L.grid = (unsigned)(L.pl.units_main + L.pl.units_tail);
    if (L.pl.form == 0) {
        // latency regime: one ciphertext per 512-thread workgroup, all levels transformed at once (kern_blindrot_latency.h)
        L.threads = BL_THREADS;
        if (c->k1 == 5) { L.kernel = blind_rotate_latency_kernel<5, 5, 8>; L.name = "blind_rotate_latency_kernel<5,5,8>"; }
        else { L.kernel = blind_rotate_latency_kernel<2, 5, 8>; L.name = "blind_rotate_latency_kernel<2,5,8>"; }
        // (257..768 bits: the throughput form below with at most one workgroup per CU, 14.6 ms per launch; the latency form in
        //  two waves took 16-18 ms there)
    } else if (L.pl.form == 2) {
        // paired throughput form (kern_blindrot_pair.h): one 512-thread workgroup per CU, 6 (or 4) ciphertexts share every key fetch
        L.threads = BRP_THREADS;
        L.kernel = blind_rotate_pair_kernel<5, 5, 8, 3, 2>;
        L.name = c->k2_park_claim ? "blind_rotate_pair_kernel<5,5,8,3,2> parking=claimed" : "blind_rotate_pair_kernel<5,5,8,3,2> parking=private";
        L.park_bytes = k2_pair_park_bytes(c, L.grid);
        L.park_owner = c->k2_park_claim != 0;
    } else {
        // throughput form (kern_blindrot16.h): accumulator parked in HBM between uses, key rows prefetched across the transform
        L.threads = EP_THREADS;
        if (c->k1 == 5 && k2_home_allowed(c)) { L.kernel = blind_rotate16_kernel<5, 5, 8, 3, 2, true>; L.name = "blind_rotate16_kernel<5,5,8,3,2,true>"; }
        else if (c->k1 == 5) { L.kernel = blind_rotate16_kernel<5, 5, 8, 3, 2, false>; L.name = "blind_rotate16_kernel<5,5,8,3,2,false>"; }
        else { L.kernel = blind_rotate16_kernel<2, 5, 8, 8>; L.name = "blind_rotate16_kernel<2,5,8,8,0,false>"; }
        L.park_bytes = (size_t)L.grid * BR16_PARK_WORDS_PER_WG * 8;
    }
    return L;
}

// The window of this context for `steps` WoPBS over n blocks (fheaes_aes_context_window): what fheaes_aes_set_window forced, else
// aes_window_plan for the form the full batch's launch really takes here.  0: one WoPBS per step.
uint64_t aes_context_window(fheaes_ctx *c, uint64_t n, uint64_t steps)
{
    if (n == 0 || steps == 0 || c->aes_window == FHEAES_AES_WINDOW_OFF) return 0;
    if (c->aes_window) return std::min<uint64_t>(c->aes_window, std::min<uint64_t>(n, AES_WINDOW_MAX_BLOCKS));
    const bool pair = k2_launch(c, std::min<uint64_t>(n * AES_BLOCK_BITS, MAX_CHUNK_BITS)).pl.form == 2;
    return aes_window_plan(n, steps, c->cu_count, c->k1, pair).window;
}

// The audit of one blind-rotation launch.  `prod`: the product launch's arguments -- its input, output, row count and the three constants
// are the audit's; whatever form it took, the sampled rows are gathered and go through the latency form, which parks nothing.
static_assert(AUDIT_MAX_ROWS <= LATENCY_BATCH_BITS, "the audit's rows are one latency-form launch");
int launch_blind_rotate_audit(fheaes_ctx *c, const ExtProdArgs &prod)
{
    const AuditLaunch L = audit_begin(c, c->audit[FHEAES_STAGE_BLIND_ROTATE], prod.count, prod.out, c->big1, c->big1);
    uint64_t *const in = (uint64_t *)L.au.in.p;
    hipLaunchKernelGGL(audit_gather_kernel, dim3(L.S), dim3(AUDIT_THREADS), 0, c->stream, prod.lwe_in, c->n + 1, L.au.seed, L.launch, L.m, L.S, in);
    ExtProdArgs a{};
    a.ggsw = prod.ggsw; a.tw = prod.tw; a.iters = prod.iters;
    a.tv_const = prod.tv_const; a.body_shift = prod.body_shift; a.post_add = prod.post_add;
    a.lwe_in = in; a.out = (uint64_t *)L.au.out.p; a.count = L.S;
    void (*const latency)(ExtProdArgs) = c->k1 == 5 ? blind_rotate_latency_kernel<5, 5, 8> : blind_rotate_latency_kernel<2, 5, 8>;
    hipLaunchKernelGGL(latency, dim3(L.S), dim3(BL_THREADS), 0, c->stream, a);
    return audit_compare(c, L);
}

int launch_cbs_pbs(fheaes_ctx *c, const uint64_t *lwe_small, uint64_t m, uint32_t level, uint64_t *out)
{
    if (m == 0) return FHEAES_OK;
    // the blind-rotation kernels address the Fourier BSK as ONE raw buffer with 32-bit byte offsets
    if ((uint64_t)c->n * c->p.pbs_level * c->k1 * c->k1 * FHE_H * 16 > 0x7FFFFFFFull)
        return c->fail(FHEAES_ERR_INVALID, "bootstrapping key larger than 2 GiB is not supported by the blind-rotation kernels");
    StageScope sc(c, FHEAES_STAGE_BLIND_ROTATE, m);
    ExtProdArgs a{};
    a.ggsw = c->bskf; a.tw = c->tw_d;
    a.out = out; a.count = m; a.iters = c->n; a.lwe_in = lwe_small;
    const uint64_t half_delta = 1ull << (64 - c->p.cbs_base_log * level - 1);
    a.tv_const = (uint64_t)0 - half_delta; a.body_shift = 1ull << 62; a.post_add = half_delta;
    const K2Launch L = k2_launch(c, m);
    if (L.pl.form != 0) a.units_main = (uint32_t)L.pl.units_main;
    if (L.park_bytes) {
        if (L.park_bytes > 0x7FFFFFFFull) return c->fail(FHEAES_ERR_INVALID, "internal: parking slab of %zu bytes exceeds one raw buffer", L.park_bytes);
        TRY(ensure(c, c->ws_park, L.park_bytes));
        a.park = (uint64_t *)c->ws_park.p; a.park_bytes = L.park_bytes;
    }
    if (L.park_owner) {
        // owner words of the shared slots: all free when a launch starts (every workgroup gives its slot back before it ends; the
        // memset makes that hold even after a launch that was aborted) -- or, under the test hook, the pattern it set
        TRY(ensure_park_owner(c));
        if (c->k2_park_pattern)
            HIP_TRY(c, hipMemcpyAsync(c->ws_park_owner.p, c->ws_park_pattern.p, BRP_PARK_SLOTS * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        else
            HIP_TRY(c, hipMemsetAsync(c->ws_park_owner.p, 0, BRP_PARK_SLOTS * sizeof(uint32_t), c->stream));
        a.park_owner = (uint32_t *)c->ws_park_owner.p;
        if (c->k2_park_record) {
            TRY(ensure(c, c->ws_park_record, (size_t)L.grid * 2 * sizeof(uint32_t)));
            HIP_TRY(c, hipMemsetAsync(c->ws_park_record.p, 0xFF, (size_t)L.grid * 2 * sizeof(uint32_t), c->stream));   // unwritten = ~0
            const uint64_t rp = (uint64_t)(uintptr_t)c->ws_park_record.p;
            uint32_t *const rp_word = (uint32_t *)((char *)c->ws_park_owner.p + PARK_RECORD_PTR_OFFSET);
            HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)rp_word, (int)(uint32_t)rp, 1, c->stream));
            HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)(rp_word + 1), (int)(uint32_t)(rp >> 32), 1, c->stream));
            c->k2_park_record_n = L.grid;
        }
    }
#ifdef EP_STAMPS
    static const char *namesL[EP_NPH] = {"barrier (result) + accumulate", "rotate+decompose (1 coeff x K1)", "read digits + forward fft", "digit stores", "barrier (digits)", "MAC", "barrier (MAC done)",
                                         "products store + next rows", "barrier (products)", "inverse fft -> doubles", "barrier (acc)", "barrier (decomposition)"};
    static const char *namesT[EP_NPH] = {"stage+rotate+decomp_first", "decomp_next", "fwd head", "pre-level barrier", "fwd tail (transpose+dft16)",       // both throughput forms
                                         "digit stores+late loads", "exchange barrier", "MAC", "products exchange", "inverse fft", "convert+add", "loop head"};
    StampReport rep(c, (size_t)L.grid * (L.threads / 64), L.pl.form == 0 ? namesL : namesT, L.pl.form == 0 ? 8 : 0);
    a.stamps = rep.d;
#endif
    hipLaunchKernelGGL(L.kernel, dim3(L.grid), dim3(L.threads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (c->audit[FHEAES_STAGE_BLIND_ROTATE].wants(m)) TRY(launch_blind_rotate_audit(c, a));
    return FHEAES_OK;
}

int launch_vertical_packing(fheaes_ctx *c, const double2 *ggswf, uint64_t n_inputs, uint32_t bits, const uint64_t *luts,
                            uint32_t n_luts, int per_input, uint64_t *out)
{
    if (n_inputs == 0) return FHEAES_OK;
    StageScope sc(c, FHEAES_STAGE_VERTICAL_PACKING, n_inputs * n_luts * bits);
    // the kernel pair of this parameter set and R, its instances (or CMUX jobs) per workgroup
    const bool k4 = c->k1 == 5;
    const uint32_t R = k4 ? 3 : 8;
    void (*const cmux_kernel)(CmuxArgs) = k4 ? cmux_level_kernel<5, 15, 3> : cmux_level_kernel<2, 15, 8>;
    void (*const vp_kernel)(VpArgs) = k4 ? vertical_packing_kernel<5, 15, 3> : vertical_packing_kernel<2, 15, 8>;
    const uint32_t inst_per_input = n_luts * bits;
    const uint64_t W = lut_row_words(bits);
    // ---- inputs wider than 9 bits: CMUX tree over bits 9..bits-1 (kern_extprod.h, cmux_level_kernel), root -> ws_tree ----
    const uint64_t *glwe_root = nullptr;
    if (bits > 9) {
        const uint32_t tree_bits = bits - 9;
        const uint64_t instances = n_inputs * inst_per_input, gsz = (uint64_t)c->k1 * FHE_N;
        // level t writes (2^(tree_bits-1-t)) nodes per instance; ping-pong between the two halves of ws_tree
        const uint64_t half_words = instances * (1ull << (tree_bits - 1)) * gsz;
        TRY(ensure(c, c->ws_tree, 2 * half_words * 8));
        uint64_t *buf[2] = {(uint64_t *)c->ws_tree.p, (uint64_t *)c->ws_tree.p + half_words};
        for (uint32_t t = 0; t < tree_bits; ++t) {
            CmuxArgs a{};
            a.ggsw = ggswf; a.tw = c->tw_d;
            a.luts = t == 0 ? luts : nullptr; a.in = t == 0 ? nullptr : buf[(t - 1) & 1]; a.out = buf[t & 1];
            a.bits = bits; a.bit = 9 + t; a.nodes_out = 1u << (tree_bits - 1 - t);
            a.inst_per_input = inst_per_input; a.lut_per_input = per_input ? 1 : 0; a.lut_words = W;
            const uint64_t jobs = (uint64_t)inst_per_input * a.nodes_out;
            a.wg_per_input = (uint32_t)((jobs + R - 1) / R);
            hipLaunchKernelGGL(cmux_kernel, dim3((unsigned)(n_inputs * a.wg_per_input)), dim3(EP_THREADS), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
        }
        glwe_root = buf[(tree_bits - 1) & 1];
    }
    VpArgs a{};
    a.ggsw = ggswf; a.tw = c->tw_d;
    a.out = out; a.iters = bits < 9 ? bits : 9; a.ggsw_per_input = bits;
    a.luts = luts; a.lut_words = W; a.glwe_in = glwe_root;
    a.lut_per_input = per_input ? 1 : 0; a.inst_per_input = inst_per_input;
    a.wg_per_input = (inst_per_input + R - 1) / R;
    hipLaunchKernelGGL(vp_kernel, dim3((unsigned)(n_inputs * a.wg_per_input)), dim3(EP_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// ---- the gate (kern_gate.h): out = GGSW_g (x) in ---------------------------------------------------------------------------------
#define GATE_MAX_GRID 65536ull         /* workgroups per launch of gate_kernel; a larger table is cut into several launches */
// instances per workgroup: R K1 <= 16 lane groups
uint32_t gate_r(uint32_t k1) { return k1 == 5 ? 3 : 8; }

// The caller's runs (bits_of_gate[g] consecutive instances under gate g) as the kernel's workgroup table: every gate's run cut into
// workgroups of up to R instances, a gate of 0 instances none.  `chunk` > 0: the gates are bootstrapped `chunk` at a time into one
// workspace, so an entry names its gate inside its chunk, and chunk_end[c] is the number of workgroups of chunks 0..c.
// Returns the sum of the runs.
uint64_t gate_table(const uint64_t *bits_of_gate, uint64_t n_gates, uint32_t R, uint64_t chunk, std::vector<GateWg> *wgs, std::vector<uint64_t> *chunk_end,
                    uint64_t *n_wgs)
{
    uint64_t first = 0, count = 0;
    for (uint64_t g = 0; g < n_gates; ++g) {
        const uint64_t run = bits_of_gate[g];
        if (wgs)
            for (uint64_t i = 0; i < run; i += R)
                wgs->push_back({first + i, (uint32_t)(chunk ? g % chunk : g), (uint32_t)std::min<uint64_t>(R, run - i)});
        count += (run + R - 1) / R;
        first += run;
        if (chunk_end && chunk && ((g + 1) % chunk == 0 || g + 1 == n_gates)) chunk_end->push_back(count);
    }
    *n_wgs = count;
    return first;
}

// workgroups wg0 .. wg0 + n_wgs - 1 of the device table `wgs` over the Fourier GGSWs `ggswf` (the gates the table's entries index);
// form GATE_LWE / GATE_GLWE.  Accounted under vertical packing; units: bits, or GLWEs x N.
int launch_gate(fheaes_ctx *c, const double2 *ggswf, const GateWg *wgs, uint64_t n_wgs, uint64_t units, int form, const uint64_t *in, uint64_t *out)
{
    if (n_wgs == 0) return FHEAES_OK;
    StageScope sc(c, FHEAES_STAGE_VERTICAL_PACKING, form == GATE_GLWE ? units * FHE_N : units);
    const bool k4 = c->k1 == 5;
    void (*const kernel)(GateArgs) = form == GATE_GLWE ? (k4 ? gate_kernel<5, 15, 3, GATE_GLWE> : gate_kernel<2, 15, 8, GATE_GLWE>)
                                                       : (k4 ? gate_kernel<5, 15, 3, GATE_LWE> : gate_kernel<2, 15, 8, GATE_LWE>);
    for (uint64_t w0 = 0; w0 < n_wgs; w0 += GATE_MAX_GRID) {
        GateArgs a{};
        a.ggsw = ggswf; a.tw = c->tw_d; a.wgs = wgs + w0; a.in = in; a.out = out;
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<uint64_t>(GATE_MAX_GRID, n_wgs - w0)), dim3(EP_THREADS), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// static schedule assertion (NOT runtime noise tracking: words carry no metadata): every linear layer of the engine's own AES schedule
// declares here how many WoPBS outputs it sums per word; a table that would sum more than tfhe-rs' noise-asserts allow is refused
int noise_guard(fheaes_ctx *c, uint32_t level, const char *what)
{
    if (level > c->noise_level_seen) c->noise_level_seen = level;
    if (level > FHEAES_MAX_NOISE_LEVEL)
        return c->fail(FHEAES_ERR_INVALID, "%s would sum %u nominal-noise ciphertexts; the parameter set allows %u (MaxNoiseLevel, client.rs:92)", what, level,
                       (unsigned)FHEAES_MAX_NOISE_LEVEL);
    return FHEAES_OK;
}

// The AES keys of a call: `rk` holds n sets of round keys `stride` words apart (slice i of [n_keys][Nr+1][16][8][kN+1]) and block b works
// under set of_block[b] (a device table).  of_block null: one set for every block -- the single-key entry points, which upload no table.
// packed_glwes = G > 0: `rk` is a packed store instead (fheaes_pack_round_keys: key i = G GLWEs at i * stride words, stride = G (k+1) N) and
// `bit0` the first bit of the round in question.  with_keys() is the one place that turns either form into the source type of the K6
// kernels (kern_linear.h: LweKeys, PackedKeys), which read the same words from there; rk null (no round key) is an LweKeys without a base.
struct KeySets {
    const uint64_t *rk;
    const uint32_t *of_block;
    uint64_t stride;
    uint32_t packed_glwes = 0, bit0 = 0;
    // round r of every set; blocks from `first_block` on
    KeySets round(uint64_t r, uint64_t sw, uint64_t first_block = 0) const
    {
        const uint32_t *of = of_block ? of_block + first_block : nullptr;
        if (packed_glwes) return {rk, of, stride, packed_glwes, bit0 + (uint32_t)(r * AES_BLOCK_BITS)};
        return {rk + r * sw, of, stride};
    }
};

// f(source): the round-key source of `k` for a K6 kernel template
template <class F>
static void with_keys(const fheaes_ctx *c, const KeySets &k, F &&f)
{
    if (k.packed_glwes) f(PackedKeys{k.rk, k.stride, k.bit0, c->k});
    else f(LweKeys{k.rk, k.stride});
}

int launch_gather(fheaes_ctx *c, const uint64_t *src, uint32_t n_luts, const KeySets &k, uint64_t *out, uint64_t n_blocks, const GatherTable &t)
{
    if (n_blocks == 0) return FHEAES_OK;
    TRY(noise_guard(c, (uint32_t)t.terms + (k.rk ? 1u : 0u), "the linear layer (MixColumns / ShiftRows + AddRoundKey)"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_blocks);
    dim3 grid((8 * c->big1 + 1023) / 1024, 16, (unsigned)n_blocks);
    with_keys(c, k, [&](auto keys) {
        hipLaunchKernelGGL(gather_add_kernel<decltype(keys)>, grid, dim3(256), 0, c->stream, src, n_luts, keys, k.of_block, out, n_blocks, c->big1, t);
    });
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// The grid of the block-row kernels (add_bcast_kernel, xts_whiten_kernel, mac_link_kernel, kw_link_kernel): x over the words of an item, at
// most 64 workgroups; y over the n items, at most 16384 / x of them per pass -- 256 at both parameter sets, the SLOTS_PER_PASS of
// tests/chunk_seams.py; the kernels' loops take the items beyond.
dim3 block_rows_grid(uint64_t words_per_item, uint64_t n)
{
    const unsigned gx = (unsigned)std::min<uint64_t>((words_per_item + 255) / 256, 64);
    return dim3(gx, (unsigned)std::min<uint64_t>(n, std::max<uint64_t>(1, 16384 / gx)));
}

int launch_add_bcast(fheaes_ctx *c, uint64_t *dst, const KeySets &k, uint64_t words_per_block, uint64_t n_blocks)
{
    if (n_blocks == 0) return FHEAES_OK;
    TRY(noise_guard(c, 2, "the initial AddRoundKey"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_blocks);
    const dim3 grid = block_rows_grid(words_per_block, n_blocks);
    with_keys(c, k, [&](auto keys) {
        hipLaunchKernelGGL(add_bcast_kernel<decltype(keys)>, grid, dim3(256), 0, c->stream, dst, keys, k.of_block, words_per_block, n_blocks, c->big1);
    });
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// key_rows_kernel over n_bytes bytes of each of n_keys keys; `level`: the nominal-noise ciphertexts one output word sums (1: a copy)
int launch_key_rows(fheaes_ctx *c, uint64_t *dst, uint64_t dst_stride, const uint64_t *a, uint64_t a_stride, uint32_t rot, const uint64_t *b,
                    uint64_t b_stride, uint32_t rcon, uint32_t n_bytes, uint64_t n_keys, uint32_t level)
{
    if (level > 1) TRY(noise_guard(c, level, "a key-expansion word sum"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_keys);
    dim3 grid((8 * c->big1 + 1023) / 1024, n_bytes, (unsigned)std::min<uint64_t>(n_keys, 65535));
    hipLaunchKernelGGL(key_rows_kernel, grid, dim3(256), 0, c->stream, dst, dst_stride, a, a_stride, rot, b, b_stride, rcon, c->big1, n_keys);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// bit_rows_kernel over XtsRows: offsets off0 .. off0 + n_off - 1 of n_units units.  The layer's largest row weight is what it declares to the noise
// guard (at most 4: kern_linear.h); an offset beyond XTS_MAX_OFFSET would need a second reduction and is refused.  Units: tweak blocks.
int launch_xts_tweaks(fheaes_ctx *c, const uint64_t *anchor, uint64_t anchor_stride, uint64_t n_units, uint32_t off0, uint32_t n_off, uint64_t *out)
{
    if (n_off == 0 || off0 > XTS_MAX_OFFSET || n_off > XTS_MAX_OFFSET + 1 - off0)
        return c->fail(FHEAES_ERR_INVALID, "XTS tweak offsets %u .. %u: one gather reaches offset %u at most", off0, off0 + n_off - 1, XTS_MAX_OFFSET);
    if (n_units == 0) return FHEAES_OK;
    uint32_t weight = 0, s[4];
    for (uint32_t j = off0; j < off0 + n_off; ++j)
        for (uint32_t i = 0; i < 128; ++i) weight = std::max(weight, xts_tweak_row(j, i, s));
    TRY(noise_guard(c, weight, "the XTS tweak layer (multiplication by alpha^j)"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_units * n_off);
    const uint64_t rows = n_units * n_off * 128;
    hipLaunchKernelGGL(bit_rows_kernel<XtsRows>, dim3((unsigned)std::min<uint64_t>(rows, 1u << 20)), dim3(256), 0, c->stream,
                       XtsRows{anchor, anchor_stride, n_off, off0}, out, rows, c->big1);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// xts_whiten_kernel over n_blocks blocks; `level`: the nominal-noise ciphertexts one output word sums
int launch_xts_whiten(fheaes_ctx *c, uint64_t *dst, const uint64_t *src, const uint64_t *tweaks, const uint32_t *tweak_of_block, const uint8_t *clear,
                      uint64_t n_blocks, uint32_t level)
{
    if (n_blocks == 0) return FHEAES_OK;
    TRY(noise_guard(c, level, "the XTS whitening (tweak + block)"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_blocks);
    const dim3 grid = block_rows_grid(128ull * c->big1, n_blocks);
    hipLaunchKernelGGL(xts_whiten_kernel, grid, dim3(256), 0, c->stream, dst, src, tweaks, tweak_of_block, clear, n_blocks, c->big1);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// mac_link_kernel over n_slots records (a device table); `level`: the nominal-noise ciphertexts one word sums where it is used next -- a
// link that goes into the cipher counts the round key that aes_run_dev adds first.  In place (a == dst) only with records whose a is
// their own slot: the callers build them so.  Units: blocks.
int launch_mac_link(fheaes_ctx *c, uint64_t *dst, const uint64_t *a, const uint64_t *b, const MacSlot *slots, uint64_t n_slots, uint32_t level, const char *what)
{
    if (n_slots == 0) return FHEAES_OK;
    TRY(noise_guard(c, level, what));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_slots);
    const dim3 grid = block_rows_grid(128ull * c->big1, n_slots);
    hipLaunchKernelGGL(mac_link_kernel, grid, dim3(256), 0, c->stream, dst, a, b, slots, n_slots, c->big1);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// kw_link_kernel: link `step` = 0 .. 6n of n_keys keys of n semiblocks; `wrapped` (a device table) is read by the load alone.  What it
// declares is the level of the sum plus the round key that aes_run_dev adds next: the load leaves trivial ciphertexts (0 + 1), a shuffle
// a cipher output (2 + 1), the unload the tag difference and the raw key, cipher outputs both (2).  Units: keys.
int launch_kw_link(fheaes_ctx *c, uint64_t *state, uint64_t *regs, const uint8_t *wrapped, uint64_t n_keys, uint32_t n, uint32_t step)
{
    if (n_keys == 0) return FHEAES_OK;
    const bool load = step == 0, unload = step == 6 * n;
    TRY(noise_guard(c, load ? 1 : unload ? 2 : 3, load ? "the key-unwrap load (public semiblocks + the round key that follows)"
                                                  : unload ? "the key-unwrap unload (A + the integrity constant, the raw key)"
                                                           : "a key-unwrap link (cipher output + counter + the round key that follows)"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_keys);
    const dim3 grid = block_rows_grid(128ull * c->big1, n_keys);
    hipLaunchKernelGGL(kw_link_kernel, grid, dim3(256), 0, c->stream, state, regs, wrapped, n_keys, n, step, c->big1);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// bit_rows_kernel over CmacRows: K1 and K2 of n_keys keys from their L.  It declares the largest row weight, 3 (K2's: kern_linear.h).  The
// grid IS the rows -- 256 n_keys, 2^24 at FHEAES_MAX_KEYS keys, inside one grid dimension: the kernel's loop runs once.  Units: keys.
int launch_cmac_double(fheaes_ctx *c, const uint64_t *l, uint64_t n_keys, uint64_t *out)
{
    if (n_keys == 0) return FHEAES_OK;
    static_assert(256ull * FHEAES_MAX_KEYS <= 0x7FFFFFFFull, "the rows of FHEAES_MAX_KEYS keys are one grid dimension");
    TRY(noise_guard(c, 3, "the CMAC subkey layer (multiplication by x and x^2)"));
    StageScope sc(c, FHEAES_STAGE_LINEAR, n_keys);
    hipLaunchKernelGGL(bit_rows_kernel<CmacRows>, dim3((unsigned)(n_keys * 256)), dim3(256), 0, c->stream, CmacRows{l, c->big1}, out, n_keys * 256, c->big1);
    HIP_TRY(c, hipGetLastError());
    return FHEAES_OK;
}

// ---- packing (fheaes_pack_bits, fheaes_unpack_bits) ---------------------------------------------------------------------------
static_assert(PACK_N == FHE_N && PACK_N % PACK_FOLD_ROWS == 0, "kern_linear.h's packing kernels are written for N = 512");

// 64-bit GLWEs [n_glwe][(k+1)N] -> [n_glwe][(k+1) 8 width], device pointers, 8 <= width <= 32; the caller holds the StageScope
static void launch_mod_switch(fheaes_ctx *c, const uint64_t *glwe, uint64_t n_glwe, uint32_t width, uint64_t *out)
{
    const uint32_t gsz = c->k1 * FHE_N;
    const uint64_t total = n_glwe * (gsz / 64 * width);
    hipLaunchKernelGGL(mod_switch_pack_kernel, dim3((unsigned)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, c->stream, glwe, n_glwe, gsz,
                       width, out);
}

// in [m][kN+1] -> out [ceil(m/N)][(k+1)N], device pointers.  Chunks start on multiples of N bits, so a GLWE belongs to one chunk.
// Key block k's switch of a chunk goes into ws_ggsw, the workspace K3 owns: (k+1)N words per bit where a GGSW level takes (k+1)^2 N,
// so a workspace that fheaes_reserve (or an earlier WoPBS) has sized for b bits holds a chunk of up to 5b here and is not grown;
// only a context that has less than one GLWE's worth of it allocates (for this call's bits, at most MAX_CHUNK_BITS).
// width 8..32 (fheaes_pack_bits_mod): every chunk's GLWEs are folded into ws_tmp_a (at most MAX_CHUNK_BITS / N GLWEs; grown, as
// ws_ggsw is, only by a call that needs more of it than any before: ensure() then synchronises the stream) and
// switched from there into `out` [ceil(m/N)][(k+1) 8 width]; width 64: straight into `out`.
int pack_dev(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t *out, uint32_t width = 64)
{
    if (m == 0) return FHEAES_OK;
    const uint64_t gsz = (uint64_t)c->k1 * FHE_N;
    uint64_t chunk = c->ws_ggsw.bytes / (gsz * 8) / FHE_N * FHE_N;
    if (chunk == 0) {
        chunk = std::min<uint64_t>((m + FHE_N - 1) / FHE_N * FHE_N, MAX_CHUNK_BITS);
        TRY(ensure(c, c->ws_ggsw, chunk * gsz * 8));
    }
    chunk = std::min<uint64_t>(chunk, MAX_CHUNK_BITS);
    if (width != 64) TRY(ensure(c, c->ws_tmp_a, (std::min<uint64_t>(chunk, m) + FHE_N - 1) / FHE_N * gsz * 8));
    uint64_t *ks = (uint64_t *)c->ws_ggsw.p;
    for (uint64_t t0 = 0; t0 < m; t0 += chunk) {
        const uint64_t mc = std::min<uint64_t>(chunk, m - t0), glwes = (mc + FHE_N - 1) / FHE_N;
        TRY(launch_pfpks(c, in + t0 * c->big1, mc, ks, gsz, (int)c->k));
        uint64_t *o = width == 64 ? out + t0 / FHE_N * gsz : (uint64_t *)c->ws_tmp_a.p;
        StageScope sc(c, FHEAES_STAGE_LINEAR, mc);
        HIP_TRY(c, hipMemsetAsync(o, 0, glwes * gsz * 8, c->stream));
        hipLaunchKernelGGL(pack_fold_kernel, dim3(FHE_N / PACK_FOLD_ROWS, c->k1, (unsigned)glwes), dim3(256), 0, c->stream, ks, mc, c->k1, o);
        HIP_TRY(c, hipGetLastError());
        if (width != 64) {
            launch_mod_switch(c, o, glwes, width, out + t0 / FHE_N * (gsz / 64 * width));
            HIP_TRY(c, hipGetLastError());
        }
    }
    return FHEAES_OK;
}

// in [ceil(m/N)][(k+1)N] -> out [m][kN+1], device pointers: a permutation with signs, no workspace, no keys
int unpack_dev(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t *out)
{
    for (uint64_t t0 = 0; t0 < m; t0 += MAX_CHUNK_BITS) {
        const uint64_t mc = std::min<uint64_t>(MAX_CHUNK_BITS, m - t0);
        StageScope sc(c, FHEAES_STAGE_LINEAR, mc);
        hipLaunchKernelGGL(sample_extract_kernel, dim3((unsigned)((mc + UNPACK_BITS_PER_WG - 1) / UNPACK_BITS_PER_WG)), dim3(256), 0, c->stream,
                           in + t0 / FHE_N * (uint64_t)c->k1 * FHE_N, mc, c->k, out + t0 * c->big1);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// fheaes_pack_round_keys on device pointers: in [n_keys][m][kN+1] -> out [n_keys][ceil(m/N)][(k+1)N], slice i word for word pack_dev of slice
// i.  The keys' LWEs are contiguous, so key block k's switch runs over chunks of whole keys inside ws_ggsw under pack_dev's rule (grown only
// by a context that holds less than one key's worth of it); pack_fold_kernel then folds each key of the chunk from its own GLWE boundary.
int pack_keys_dev(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t n_keys, uint64_t *out)
{
    const uint64_t gsz = (uint64_t)c->k1 * FHE_N, glwes = (m + FHE_N - 1) / FHE_N, max_keys = MAX_CHUNK_BITS / m;
    uint64_t chunk = c->ws_ggsw.bytes / (gsz * 8) / m;
    if (chunk == 0) {
        chunk = std::min<uint64_t>(n_keys, max_keys);
        TRY(ensure(c, c->ws_ggsw, chunk * m * gsz * 8));
    }
    chunk = std::min<uint64_t>(chunk, max_keys);
    uint64_t *ks = (uint64_t *)c->ws_ggsw.p;
    for (uint64_t j0 = 0; j0 < n_keys; j0 += chunk) {
        const uint64_t kc = std::min<uint64_t>(chunk, n_keys - j0);
        TRY(launch_pfpks(c, in + j0 * m * c->big1, kc * m, ks, gsz, (int)c->k));
        uint64_t *o = out + j0 * glwes * gsz;
        StageScope sc(c, FHEAES_STAGE_LINEAR, kc * m);
        HIP_TRY(c, hipMemsetAsync(o, 0, kc * glwes * gsz * 8, c->stream));
        for (uint64_t j = 0; j < kc; ++j)
            hipLaunchKernelGGL(pack_fold_kernel, dim3(FHE_N / PACK_FOLD_ROWS, c->k1, (unsigned)glwes), dim3(256), 0, c->stream, ks + j * m * gsz, m, c->k1,
                               o + j * glwes * gsz);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// fheaes_unpack_round_keys on device pointers: in [n_keys][ceil(m/N)][(k+1)N] -> out [n_keys][m][kN+1], unpack_dev key by key (m <= MAX_CHUNK_BITS)
int unpack_keys_dev(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint64_t n_keys, uint64_t *out)
{
    const uint64_t key_words = (m + FHE_N - 1) / FHE_N * c->k1 * FHE_N;
    for (uint64_t j = 0; j < n_keys; ++j) TRY(unpack_dev(c, in + j * key_words, m, out + j * m * c->big1));
    return FHEAES_OK;
}

// fheaes_packed_mod_switch on device pointers, in chunks of MAX_CHUNK_BITS / N GLWEs
int mod_switch_dev(fheaes_ctx *c, const uint64_t *in, uint64_t n_glwe, uint32_t width, uint64_t *out)
{
    const uint64_t gsz = (uint64_t)c->k1 * FHE_N, step = MAX_CHUNK_BITS / FHE_N;
    for (uint64_t g0 = 0; g0 < n_glwe; g0 += step) {
        const uint64_t gc = std::min<uint64_t>(step, n_glwe - g0);
        StageScope sc(c, FHEAES_STAGE_LINEAR, gc * FHE_N);
        launch_mod_switch(c, in + g0 * gsz, gc, width, out + g0 * (gsz / 64 * width));
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// in [ceil(m/N)][(k+1) 8 width] -> out [m][kN+1], device pointers: unpack_dev reading width-bit fields
int unpack_mod_dev(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint32_t width, uint64_t *out)
{
    for (uint64_t t0 = 0; t0 < m; t0 += MAX_CHUNK_BITS) {
        const uint64_t mc = std::min<uint64_t>(MAX_CHUNK_BITS, m - t0);
        StageScope sc(c, FHEAES_STAGE_LINEAR, mc);
        hipLaunchKernelGGL(sample_extract_mod_kernel, dim3((unsigned)((mc + UNPACK_BITS_PER_WG - 1) / UNPACK_BITS_PER_WG)), dim3(256), 0, c->stream,
                           in + t0 / FHE_N * (uint64_t)c->k1 * 8 * width, mc, c->k, width, out + t0 * c->big1);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

// bodies [m] -> out [m][kN+1], device pointers: ciphertext t carries the masks of index first_index + t (mod 2^64)
int expand_lwe_dev(fheaes_ctx *c, const MaskKey &key, uint64_t first_index, const uint64_t *bodies, uint64_t m, uint64_t *out)
{
    for (uint64_t t0 = 0; t0 < m; t0 += MAX_CHUNK_BITS) {
        const uint64_t mc = std::min<uint64_t>(MAX_CHUNK_BITS, m - t0);
        StageScope sc(c, FHEAES_STAGE_LINEAR, mc);
        hipLaunchKernelGGL(expand_lwe_kernel, dim3((unsigned)((mc * c->k + 3) / 4)), dim3(256), 0, c->stream, out + t0 * c->big1, bodies + t0, mc, c->k,
                           first_index + t0, key);
        HIP_TRY(c, hipGetLastError());
    }
    return FHEAES_OK;
}

int check_keys(fheaes_ctx *c)
{
    if (!c) return FHEAES_ERR_INVALID;
    if (!c->have_keys) return c->fail(FHEAES_ERR_NOKEYS, "evaluation keys have not been uploaded");
    return FHEAES_OK;
}

// ---- many_wopbs_without_padding on device buffers ----------------------------------------------
// the workspace of one chunk of `bits` input bits: K1's output, K2's output, the GGSWs in both domains (cbs_level == 1)
int ensure_wopbs_ws(fheaes_ctx *c, uint64_t bits)
{
    const uint64_t ggsw_words = (uint64_t)c->k1 * c->k1 * FHE_N;
    TRY(ensure(c, c->ws_small, bits * (c->n + 1) * 8));
    TRY(ensure(c, c->ws_pbs, bits * c->big1 * 8));
    TRY(ensure(c, c->ws_ggsw, bits * ggsw_words * 8));
    TRY(ensure(c, c->ws_ggswf, bits * ggsw_words * 8));
    return FHEAES_OK;
}

// The circuit bootstrap's front half behind K1: the m small LWEs of ws_small -> m Fourier GGSWs in ws_ggswf (K2 at level 1, K3, K4, through
// ws_pbs and ws_ggsw; ensure_wopbs_ws has sized all four for m bits)
int cbs_from_small(fheaes_ctx *c, uint64_t m)
{
    const uint64_t ggsw_words = (uint64_t)c->k1 * c->k1 * FHE_N;    // cbs_level == 1
    TRY(launch_cbs_pbs(c, (const uint64_t *)c->ws_small.p, m, 1, (uint64_t *)c->ws_pbs.p));
    TRY(launch_pfpks(c, (const uint64_t *)c->ws_pbs.p, m, (uint64_t *)c->ws_ggsw.p, ggsw_words));
    TRY(launch_forward_fourier(c, (const uint64_t *)c->ws_ggsw.p, m * c->k1 * c->k1, (double2 *)c->ws_ggswf.p, FHEAES_STAGE_GGSW_FFT));
    return FHEAES_OK;
}

// the whole front half of m contiguous bits: in [m][kN+1] -> K1 -> cbs_from_small
int cbs_bits(fheaes_ctx *c, const uint64_t *in, uint64_t m)
{
    TRY(launch_keyswitch(c, in, m, (uint64_t *)c->ws_small.p));
    return cbs_from_small(c, m);
}

int wopbs_dev(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t n_inputs, uint32_t bits, const uint64_t *luts, uint32_t n_luts,
              int per_input, uint64_t *lwe_out)
{
    if (bits < 1 || bits > MAX_WOPBS_BITS) return c->fail(FHEAES_ERR_INVALID, "bits_per_input must be in 1..%u (got %u)", MAX_WOPBS_BITS, bits);
    if (n_luts < 1) return c->fail(FHEAES_ERR_INVALID, "n_luts must be >= 1");
    if (n_inputs == 0) return FHEAES_OK;
    uint64_t chunk_inputs = std::max<uint64_t>(1, MAX_CHUNK_BITS / bits);
    if (bits > 9) {
        // the CMUX tree keeps 2^(bits-9) GLWEs per (input, LUT, output bit) in flight: bound that workspace to ~2 GiB per chunk
        const uint64_t per_input = (uint64_t)n_luts * bits * (1ull << (bits - 9)) * c->k1 * FHE_N * 8;
        chunk_inputs = std::max<uint64_t>(1, std::min<uint64_t>(chunk_inputs, (2ull << 30) / per_input));
    }
    const uint64_t W = lut_row_words(bits);
    TRY(ensure_wopbs_ws(c, std::min<uint64_t>(n_inputs, chunk_inputs) * bits));
    for (uint64_t i0 = 0; i0 < n_inputs; i0 += chunk_inputs) {
        const uint64_t ni = std::min<uint64_t>(chunk_inputs, n_inputs - i0);
        TRY(cbs_bits(c, lwe_in + i0 * bits * c->big1, ni * bits));
        const uint64_t *l = per_input ? luts + i0 * n_luts * bits * W : luts;
        TRY(launch_vertical_packing(c, (const double2 *)c->ws_ggswf.p, ni, bits, l, n_luts, per_input, lwe_out + i0 * n_luts * bits * c->big1));
    }
    return FHEAES_OK;
}

}  // namespace
