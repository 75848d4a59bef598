// engine.hip -- C ABI (include/fheaes.h) and host-side schedule of the MI355X FHE-AES engine.
//
// The host code here is the native counterpart of the reference's Server
// (src/server/server.rs:24-282) and S-Box front end (src/server/sbox/sbox.rs:46-97,
// src/server/sbox/many_wopbs.rs:31-116): it owns the device copies of the keys, the workspace,
// the precomputed AES LUT sets, and enqueues the kernels of kern_*.h on one HIP stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "knobs.h"
#include "fheaes.h"
#include "fft_dev.h"
#include "kern_extprod.h"
#include "kern_gate.h"
#include "kern_blindrot_latency.h"
#include "kern_blindrot16.h"
#include "kern_blindrot_pair.h"
#include "kern_audit.h"
#include "ks_launch.h"                 // kern_keyswitch.h: the kernels themselves, or (two-unit product build) their argument block + launch functions
#include "kern_linear.h"

#define FHEAES_VERSION_STR "fheaes-mi355x 0.4 (gfx950)" FHEAES_BUILD_KIND      /* " dev" when built with developer knobs (knobs.h) */

// the host code of this translation unit, each header building on the ones before it (and on the kernels' headers above)
#include "host_tables.h"
#include "engine_ctx.h"
#include "engine_launch.h"
#include "aes_schedule.h"

namespace {

int supported(const fheaes_params *p, std::string &why)
{
    char buf[256];
    if (p->polynomial_size != FHE_N) { why = "polynomial_size must be 512"; return 0; }
    if (p->glwe_dimension != 4 && p->glwe_dimension != 1) { why = "glwe_dimension must be 4 (PARAM_OPT) or 1 (toy)"; return 0; }
    if (p->pbs_base_log != 8 || p->pbs_level != 5 || p->ks_base_log != 2 || p->ks_level != 6 || p->pfks_base_log != 12 ||
        p->pfks_level != 3 || p->cbs_base_log != 15 || p->cbs_level != 1) {
        snprintf(buf, sizeof buf, "unsupported gadget: kernels are instantiated for pbs(8,5) ks(2,6) pfks(12,3) cbs(15,1)");
        why = buf;
        return 0;
    }
    if (p->lwe_dimension < 1 || p->lwe_dimension > 4096) { why = "lwe_dimension out of range"; return 0; }
    return 1;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int fheaes_k2_launch_plan(uint64_t m, uint32_t cu_count, uint32_t k, int *form, uint64_t *units_main, uint32_t *r_main,
                          uint64_t *units_tail, uint32_t *r_tail)
{
    if (!form || !units_main || !r_main || !units_tail || !r_tail || cu_count == 0 || m == 0) return FHEAES_ERR_INVALID;
    const K2Plan pl = k2_plan(m, cu_count, k + 1);
    *form = pl.form; *units_main = pl.units_main; *r_main = pl.r_main; *units_tail = pl.units_tail; *r_tail = pl.r_tail;
    return FHEAES_OK;
}
int fheaes_k2_launch_plan_forms(uint64_t m, uint32_t cu_count, uint32_t k, int allow_pair, int *form, uint64_t *units_main, uint32_t *r_main,
                                uint64_t *units_tail, uint32_t *r_tail)
{
    if (!form || !units_main || !r_main || !units_tail || !r_tail || cu_count == 0 || m == 0 || (allow_pair != 0 && allow_pair != 1)) return FHEAES_ERR_INVALID;
    const K2Plan pl = k2_plan(m, cu_count, k + 1, allow_pair == 1);
    *form = pl.form; *units_main = pl.units_main; *r_main = pl.r_main; *units_tail = pl.units_tail; *r_tail = pl.r_tail;
    return FHEAES_OK;
}
int fheaes_k2_context_plan(fheaes_ctx *ctx, uint64_t m, int *form, uint64_t *units_main, uint32_t *r_main, uint64_t *units_tail,
                           uint32_t *r_tail, char *kernel, size_t kernel_cap)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if (!form || !units_main || !r_main || !units_tail || !r_tail || m == 0) return ctx->fail(FHEAES_ERR_INVALID, "k2_context_plan: null output or empty batch");
    const K2Launch L = k2_launch(ctx, m);
    const K2Plan &pl = L.pl;
    *form = pl.form; *units_main = pl.units_main; *r_main = pl.r_main; *units_tail = pl.units_tail; *r_tail = pl.r_tail;
    if (kernel && kernel_cap) { std::strncpy(kernel, L.name, kernel_cap - 1); kernel[kernel_cap - 1] = 0; }
    return FHEAES_OK;
}
int fheaes_k2_set_parking(fheaes_ctx *ctx, int claimed)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if (claimed != 0 && claimed != 1) return ctx->fail(FHEAES_ERR_INVALID, "k2_set_parking: 1 = claimed slots, 0 = one private slot per workgroup (got %d)", claimed);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->k2_park_claim = claimed;
    return FHEAES_OK;
}
int fheaes_k2_set_forms(fheaes_ctx *ctx, int allow_pair, int allow_home)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if ((allow_pair != 0 && allow_pair != 1) || (allow_home != 0 && allow_home != 1))
        return ctx->fail(FHEAES_ERR_INVALID, "k2_set_forms: each of allow_pair, allow_home is 0 or 1 (got %d, %d)", allow_pair, allow_home);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->k2_deny_pair = allow_pair == 0;
    ctx->k2_deny_home = allow_home == 0;
    return FHEAES_OK;
}
int fheaes_aes_window_plan(uint64_t n_blocks, uint32_t steps, uint32_t cu_count, uint32_t k, uint64_t *window_blocks, uint64_t *launches,
                           uint64_t *generations, uint64_t *generations_by_round)
{
    if (!window_blocks || !launches || !generations || !generations_by_round || n_blocks == 0 || steps == 0 || cu_count == 0) return FHEAES_ERR_INVALID;
    const AesWindowPlan pl = aes_window_plan(n_blocks, steps, cu_count, k + 1);
    *window_blocks = pl.window; *launches = pl.launches; *generations = pl.generations; *generations_by_round = pl.generations_by_round;
    return FHEAES_OK;
}
int fheaes_aes_context_window(fheaes_ctx *ctx, uint64_t n_blocks, uint32_t steps, uint64_t *window_blocks)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if (!window_blocks) return ctx->fail(FHEAES_ERR_INVALID, "aes_context_window: null output");
    *window_blocks = aes_context_window(ctx, n_blocks, steps);
    return FHEAES_OK;
}
int fheaes_aes_set_window(fheaes_ctx *ctx, uint32_t window_blocks)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->aes_window = window_blocks;
    return FHEAES_OK;
}
int fheaes_k2_park_debug(fheaes_ctx *ctx, const uint32_t *initial_owner, int record)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if (record != 0 && record != 1) return ctx->fail(FHEAES_ERR_INVALID, "k2_park_debug: record must be 0 or 1 (got %d)", record);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (initial_owner) {
        TRY(ensure(ctx, ctx->ws_park_pattern, BRP_PARK_SLOTS * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpy(ctx->ws_park_pattern.p, initial_owner, BRP_PARK_SLOTS * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (ctx->ws_park_owner.p)        // no record pointer until a recorded launch sets one
        HIP_TRY(ctx, hipMemset((char *)ctx->ws_park_owner.p + PARK_RECORD_PTR_OFFSET, 0, sizeof(uint64_t)));
    ctx->k2_park_pattern = initial_owner != nullptr;
    ctx->k2_park_record = record == 1;
    ctx->k2_park_record_n = 0;
    return FHEAES_OK;
}
int fheaes_k2_park_read(fheaes_ctx *ctx, uint64_t *fallbacks, uint64_t *violations, uint32_t *owner_out, uint32_t *record_out,
                        uint64_t record_cap, uint64_t *record_n)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    if (record_out && record_cap < ctx->k2_park_record_n)
        return ctx->fail(FHEAES_ERR_INVALID, "k2_park_read: %llu records do not fit record_cap = %llu", (unsigned long long)ctx->k2_park_record_n,
                         (unsigned long long)record_cap);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t words[PARK_OWNER_BYTES / sizeof(uint32_t)] = {};       // never allocated (no claimed paired launch yet): all zero
    if (ctx->ws_park_owner.p) HIP_TRY(ctx, hipMemcpy(words, ctx->ws_park_owner.p, PARK_OWNER_BYTES, hipMemcpyDeviceToHost));
    uint64_t counters[2];
    std::memcpy(counters, words + BRP_PARK_SLOTS, sizeof counters);
    if (fallbacks) *fallbacks = counters[0];
    if (violations) *violations = counters[1];
    if (owner_out) std::memcpy(owner_out, words, BRP_PARK_SLOTS * sizeof(uint32_t));
    if (record_out && ctx->k2_park_record_n)
        HIP_TRY(ctx, hipMemcpy(record_out, ctx->ws_park_record.p, ctx->k2_park_record_n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (record_n) *record_n = ctx->k2_park_record_n;
    return FHEAES_OK;
}
// ---- the audit (StageAudit in engine_ctx.h; kern_audit.h; audit_begin, audit_compare and the launchers in engine_launch.h) ---------------
namespace {
// au: the stage's audit, null for a stage that has none.  in_words: the words of a gathered input row, 0 for a second form that reads the
// sampled rows where they lie (no buffer).  out_words: the written words of one row of the stage's widest launch.
struct AuditShape { StageAudit *au; uint32_t in_words, out_words; };
AuditShape audit_shape(fheaes_ctx *c, int stage)
{
    switch (stage) {
    case FHEAES_STAGE_KEYSWITCH: return {&c->audit[stage], 0, c->n + 1};
    case FHEAES_STAGE_BLIND_ROTATE: return {&c->audit[stage], c->n + 1, c->big1};
    case FHEAES_STAGE_PFPKS: return {&c->audit[stage], 0, c->k1 * c->k1 * FHE_N};       // the k + 1 key blocks
    }
    return {nullptr, 0, 0};
}
}  // namespace
int fheaes_audit_stage_set(fheaes_ctx *ctx, int stage, uint32_t rows, uint64_t min_rows, uint64_t seed)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    const AuditShape sh = audit_shape(ctx, stage);
    StageAudit *const au = sh.au;
    if (!au) return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_set: stage %d has no audit (the key switch, the blind rotation, the packing key switch)", stage);
    if (rows > AUDIT_MAX_ROWS) return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_set: at most %d rows per launch (got %u)", AUDIT_MAX_ROWS, rows);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    au->rows = 0;                        // off until everything below has succeeded
    au->hook = false;
    au->launch = 0;
    if (rows == 0) {
        for (DevBuf *b : {&au->in, &au->out, &au->state})
            if (b->p) { HIP_TRY(ctx, hipFree(b->p)); b->p = nullptr; b->bytes = 0; }
        return FHEAES_OK;
    }
    // for FHEAES_AUDIT_MAX_ROWS rows whatever `rows` is: a later set with more rows moves nothing
    if (sh.in_words) TRY(ensure(ctx, au->in, (size_t)AUDIT_MAX_ROWS * sh.in_words * 8));
    TRY(ensure(ctx, au->out, (size_t)AUDIT_MAX_ROWS * sh.out_words * 8));
    TRY(ensure(ctx, au->state, AUDIT_STATE_WORDS * 8));
    HIP_TRY(ctx, hipMemset(au->state.p, 0, AUDIT_STATE_WORDS * 8));
    au->min_rows = min_rows;
    au->seed = seed;
    au->rows = rows;
    return FHEAES_OK;
}
int fheaes_audit_stage_read(fheaes_ctx *ctx, int stage, uint64_t *launches, uint64_t *rows_checked, uint64_t *rows_wrong, uint64_t *records_out,
                            uint64_t record_cap, uint64_t *record_n)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    const StageAudit *const au = audit_shape(ctx, stage).au;
    if (!au) return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_read: stage %d has no audit", stage);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t st[AUDIT_STATE_WORDS] = {};            // audit off: all zero
    if (au->state.p) HIP_TRY(ctx, hipMemcpy(st, au->state.p, sizeof st, hipMemcpyDeviceToHost));
    const uint64_t n = std::min<uint64_t>(st[AUDIT_ST_WRONG], AUDIT_RECORDS);
    if (records_out && record_cap < n)
        return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_read: %llu records do not fit record_cap = %llu", (unsigned long long)n, (unsigned long long)record_cap);
    if (launches) *launches = st[AUDIT_ST_LAUNCHES];
    if (rows_checked) *rows_checked = st[AUDIT_ST_CHECKED];
    if (rows_wrong) *rows_wrong = st[AUDIT_ST_WRONG];
    if (records_out && n) std::memcpy(records_out, st + AUDIT_ST_RECORDS, n * AUDIT_RECORD_WORDS * 8);
    if (record_n) *record_n = n;
    return FHEAES_OK;
}
int fheaes_audit_stage_debug(fheaes_ctx *ctx, int stage, uint64_t row, uint32_t word, uint64_t xor_mask)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    const AuditShape sh = audit_shape(ctx, stage);
    StageAudit *const au = sh.au;
    if (!au) return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_debug: stage %d has no audit", stage);
    if (xor_mask == 0 || word >= sh.out_words)
        return ctx->fail(FHEAES_ERR_INVALID, "audit_stage_debug: a non-zero mask and a word below %u (got mask %#llx, word %u)", sh.out_words,
                         (unsigned long long)xor_mask, word);
    au->hook = true;
    au->hook_row = row; au->hook_word = word; au->hook_mask = xor_mask;
    return FHEAES_OK;
}
// the blind rotation's audit under its first names
int fheaes_audit_set(fheaes_ctx *ctx, uint32_t rows, uint64_t min_bits, uint64_t seed)
{
    return fheaes_audit_stage_set(ctx, FHEAES_STAGE_BLIND_ROTATE, rows, min_bits, seed);
}
int fheaes_audit_read(fheaes_ctx *ctx, uint64_t *launches, uint64_t *rows_checked, uint64_t *rows_wrong, uint64_t *records_out, uint64_t record_cap,
                      uint64_t *record_n)
{
    return fheaes_audit_stage_read(ctx, FHEAES_STAGE_BLIND_ROTATE, launches, rows_checked, rows_wrong, records_out, record_cap, record_n);
}
int fheaes_audit_debug(fheaes_ctx *ctx, uint64_t row, uint32_t word, uint64_t xor_mask)
{
    return fheaes_audit_stage_debug(ctx, FHEAES_STAGE_BLIND_ROTATE, row, word, xor_mask);
}
int fheaes_audit_rows(uint64_t seed, uint64_t launch, uint64_t m, uint32_t rows, uint64_t *rows_out)
{
    if (!rows_out || m == 0 || rows == 0 || rows > AUDIT_MAX_ROWS) return FHEAES_ERR_INVALID;
    const uint32_t S = (uint32_t)std::min<uint64_t>(rows, m);
    for (uint32_t s = 0; s < S; ++s) rows_out[s] = audit_row(seed, launch, m, S, s);
    return FHEAES_OK;
}
int fheaes_audit_plain_batch(fheaes_ctx *ctx, int stage, const uint64_t *lwe_in, uint64_t m, int block, uint64_t *out)
{
    if (!ctx) return FHEAES_ERR_INVALID;
    CtxLock lock__(ctx);
    const bool k1 = stage == FHEAES_STAGE_KEYSWITCH;
    if (!k1 && stage != FHEAES_STAGE_PFPKS) return ctx->fail(FHEAES_ERR_INVALID, "audit_plain_batch: stage %d has no plain form (the two key switches have)", stage);
    if (block < -1 || block > (k1 ? -1 : (int)ctx->k))
        return ctx->fail(FHEAES_ERR_INVALID, "audit_plain_batch: block %d (the key switch takes -1, the packing key switch -1 .. %u)", block, ctx->k);
    TRY(check_keys(ctx));
    if (!lwe_in || !out) return ctx->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // device pointers only: a hook of tests and tools, which hold their arrays on the device; it stages nothing and only enqueues
    const unsigned nz = k1 ? 1 : keyswitch_k3_blocks(ctx, block);
    KeyswitchPlainArgs a = k1 ? keyswitch_plain_args(keyswitch_k1_args(ctx), ctx->big, nz) : keyswitch_plain_args(keyswitch_k3_args(ctx, block), ctx->big1, nz);
    // in groups of FHEAES_AUDIT_MAX_ROWS rows: the launches the audit makes
    for (uint64_t r0 = 0; r0 < m; r0 += AUDIT_MAX_ROWS) {
        a.in = lwe_in + r0 * a.in_stride; a.out = out + r0 * a.out_stride;
        a.S = (uint32_t)std::min<uint64_t>(AUDIT_MAX_ROWS, m - r0); a.m = a.S;
        launch_keyswitch_plain(ctx, stage, a, nz);
        HIP_TRY(ctx, hipGetLastError());
    }
    return FHEAES_OK;
}
const char *fheaes_version(void) { return FHEAES_VERSION_STR; }

const char *fheaes_last_error(const fheaes_ctx *ctx)
{
    if (!ctx) return g_create_error.c_str();
    if (tl_error_ctx_id != ctx->id) {            // this thread has not failed on ctx: hand out a private copy of the context's last message
        CtxLock lock__(ctx);
        tl_error = ctx->err;
        tl_error_ctx_id = ctx->id;
    }
    return tl_error.c_str();
}

int fheaes_get_twiddles(double *psi_out)
{
    if (!psi_out) return FHEAES_ERR_INVALID;
    const HostTwiddles &t = twiddles();
    for (int j = 0; j < FHE_N; ++j) { psi_out[2 * j] = t.psi_re[j]; psi_out[2 * j + 1] = t.psi_im[j]; }
    return FHEAES_OK;
}

int fheaes_gen_lut(uint32_t nb_block, const uint64_t *f_table, uint64_t *lut_out)
{
    if (nb_block < 1 || nb_block > MAX_WOPBS_BITS || !f_table || !lut_out) return FHEAES_ERR_INVALID;
    gen_lut_host(nb_block, f_table, lut_out);
    return FHEAES_OK;
}

int fheaes_create(const fheaes_params *params, int device, fheaes_ctx **out)
{
    if (!params || !out) { g_create_error = "null argument"; return FHEAES_ERR_INVALID; }
    std::string why;
    if (!supported(params, why)) { g_create_error = why; return FHEAES_ERR_INVALID; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_create_error = std::string("no HIP device: ") + hipGetErrorString(e); return FHEAES_ERR_DEVICE; }
    if (device < 0 || device >= ndev) { g_create_error = "device ordinal out of range"; return FHEAES_ERR_INVALID; }
    fheaes_ctx *c = new fheaes_ctx();
    c->p = *params; c->device = device;
    c->n = params->lwe_dimension; c->k = params->glwe_dimension; c->k1 = c->k + 1; c->big = c->k * FHE_N; c->big1 = c->big + 1;
    auto bail = [&](const char *what, hipError_t err) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        fheaes_destroy(c);
        return FHEAES_ERR_DEVICE;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cu_count = (uint32_t)cus;
    }
    c->stream = c->own_stream;
    // twiddle tables
    const HostTwiddles &t = twiddles();
    std::vector<double2> tw(FHE_TW_ENTRIES);
    for (auto &w : tw) { w.x = 0.0; w.y = 0.0; }
    for (int k1 = 0; k1 < 16; ++k1) for (int b = 0; b < 16; ++b) { double re, im; t.pow(b * (4 * k1 + 1), re, im); tw[FHE_TW_STRIDE * k1 + b].x = re; tw[FHE_TW_STRIDE * k1 + b].y = im; }
    // the kernels' compile-time constants (fft_consts.h, generated from this table) must BE this table
    for (int m = 0; m < 32; ++m)
        if (FHE_PSI16_RE[m] != t.psi_re[16 * m] || FHE_PSI16_IM[m] != t.psi_im[16 * m]) {
            g_create_error = "fft_consts.h does not match the twiddle table (regenerate it: tools/gen_fft_consts.py)";
            fheaes_destroy(c);
            return FHEAES_ERR_INVALID;
        }
    if ((e = hipMalloc((void **)&c->tw_d, FHE_TW_ENTRIES * sizeof(double2))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMemcpy(c->tw_d, tw.data(), FHE_TW_ENTRIES * sizeof(double2), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy", e);
    // AES LUT sets, built once (the reference rebuilds them on every call: sbox.rs:54-60, :85-94)
    for (int s = 0; s < LUTSET_COUNT; ++s) {
        std::vector<uint64_t> h;
        c->lutset_n[s] = build_lutset_host(s, h);
        if ((e = hipMalloc((void **)&c->lutset_d[s], h.size() * 8)) != hipSuccess) return bail("hipMalloc", e);
        if ((e = hipMemcpy(c->lutset_d[s], h.data(), h.size() * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy", e);
    }
    for (int w = 0; w < 2; ++w) {        // the CCM tag check's two LUTs
        std::vector<uint64_t> h;
        build_tag_lut_host(w, h);
        if ((e = hipMalloc((void **)&c->lut_tag_d[w], h.size() * 8)) != hipSuccess) return bail("hipMalloc", e);
        if ((e = hipMemcpy(c->lut_tag_d[w], h.data(), h.size() * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy", e);
    }
    *out = c;
    return FHEAES_OK;
}

void fheaes_destroy(fheaes_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto &pe : c->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto ev : c->free_events) (void)hipEventDestroy(ev);
    void *ptrs[] = {c->ksk_frag, c->pfpksk_frag, c->bskf, c->tw_d};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->pin_ev) (void)hipEventDestroy(c->pin_ev);
    for (int s = 0; s < LUTSET_COUNT; ++s) if (c->lutset_d[s]) (void)hipFree(c->lutset_d[s]);
    for (uint64_t *p : c->lut_tag_d) if (p) (void)hipFree(p);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                            // every DevBuf of the context (workspace, staging) frees itself here
}

size_t fheaes_key_words(const fheaes_ctx *c, int which)
{
    if (!c) return 0;
    switch (which) {
    case FHEAES_KEY_KSK: return (size_t)c->big * c->p.ks_level * (c->n + 1);
    case FHEAES_KEY_BSK: return (size_t)c->n * c->p.pbs_level * c->k1 * c->k1 * FHE_N;
    case FHEAES_KEY_PFPKSK: return (size_t)c->k1 * c->big1 * c->p.pfks_level * c->k1 * FHE_N;
    default: return 0;
    }
}

int fheaes_set_stream(fheaes_ctx *c, void *hip_stream)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return FHEAES_OK;
}

int fheaes_synchronize(fheaes_ctx *c)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FHEAES_OK;
}

int fheaes_reserve(fheaes_ctx *c, uint64_t max_bits)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t bits = std::min<uint64_t>(max_bits, MAX_CHUNK_BITS);
    TRY(ensure_wopbs_ws(c, bits));
    // the blind rotation's parking slab for the largest launch this reservation covers (64 KB per workgroup)
    const K2Launch L = k2_launch(c, bits);
    if (L.park_bytes) TRY(ensure(c, c->ws_park, L.park_bytes));
    if (L.park_owner) TRY(ensure_park_owner(c));
    return FHEAES_OK;
}

// ---- test hook of the allocations (tests/test_gpu_alloc_failures.py): ctx_malloc, engine_ctx.h ------------------------------------
int fheaes_alloc_debug(fheaes_ctx *c, uint64_t fail_nth, uint64_t *seen_out)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (seen_out) *seen_out = c->alloc_seen;
    c->alloc_seen = 0;
    c->alloc_fail_nth = fail_nth;
    return FHEAES_OK;
}

// ---- test hooks of the workspace state (tests/test_gpu_workspace_state.py) ----------------------------------------------------
// The scratch a call may grow, overwrite or free between two other calls: every ws_* buffer but the parking owner words, pattern and
// record (state: counters and hooks that persist across launches by design), and the four staging buffers.  Keys, twiddles, LUT
// sets and the pinned buffer are not scratch and are not listed.  The class says what a stale read of the poisoned buffer gives:
// a NaN (buffers that only ever hold doubles), a wrong word (torus words, digits, accumulators), or -- index tables and staged
// arguments -- entry 1 of whatever the index selects, which is in range wherever there are two of a thing.
namespace {

struct WsEntry { const char *name; DevBuf fheaes_ctx::*buf; int stage; int cls; };
const WsEntry WS_TABLE[FHEAES_WS_BUFFERS] = {
    {"ws_small", &fheaes_ctx::ws_small, -1, FHEAES_WS_WORDS},   {"ws_pbs", &fheaes_ctx::ws_pbs, -1, FHEAES_WS_WORDS},
    {"ws_ggsw", &fheaes_ctx::ws_ggsw, -1, FHEAES_WS_WORDS},     {"ws_ggswf", &fheaes_ctx::ws_ggswf, -1, FHEAES_WS_F64},
    {"ws_vp", &fheaes_ctx::ws_vp, -1, FHEAES_WS_WORDS},         {"ws_tmp_a", &fheaes_ctx::ws_tmp_a, -1, FHEAES_WS_WORDS},
    {"ws_tmp_b", &fheaes_ctx::ws_tmp_b, -1, FHEAES_WS_WORDS},   {"ws_tmp_c", &fheaes_ctx::ws_tmp_c, -1, FHEAES_WS_WORDS},
    {"ws_luts", &fheaes_ctx::ws_luts, -1, FHEAES_WS_WORDS},     {"ws_misc", &fheaes_ctx::ws_misc, -1, FHEAES_WS_TABLES},
    {"ws_digits", &fheaes_ctx::ws_digits, -1, FHEAES_WS_WORDS}, {"ws_park", &fheaes_ctx::ws_park, -1, FHEAES_WS_WORDS},
    {"ws_tree", &fheaes_ctx::ws_tree, -1, FHEAES_WS_WORDS},
    {"stage[0]", nullptr, 0, FHEAES_WS_TABLES}, {"stage[1]", nullptr, 1, FHEAES_WS_TABLES},
    {"stage[2]", nullptr, 2, FHEAES_WS_TABLES}, {"stage[3]", nullptr, 3, FHEAES_WS_TABLES},
};
DevBuf *ws_buf(fheaes_ctx *c, const WsEntry &e) { return e.stage >= 0 ? &c->stage[e.stage] : &(c->*(e.buf)); }

}  // namespace

int fheaes_workspace_info(fheaes_ctx *c, uint32_t index, char *name_out, size_t name_cap, uint64_t *bytes_out, int *class_out,
                          uint64_t *first_word_out, uint64_t *last_word_out)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (index >= FHEAES_WS_BUFFERS) return c->fail(FHEAES_ERR_INVALID, "workspace_info: index %u, the context has %d scratch buffers", index, FHEAES_WS_BUFFERS);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const WsEntry &e = WS_TABLE[index];
    const DevBuf &b = *ws_buf(c, e);
    if (name_out && name_cap) { std::strncpy(name_out, e.name, name_cap - 1); name_out[name_cap - 1] = 0; }
    if (bytes_out) *bytes_out = b.bytes;
    if (class_out) *class_out = e.cls;
    // the 8 bytes at offset 0 and the last whole 8-byte word at an aligned offset; a buffer of fewer than 8 bytes: its bytes, zero-extended
    uint64_t first = 0, last = 0;
    if (b.p && b.bytes) {
        const size_t take = std::min<size_t>(8, b.bytes), last_off = b.bytes >= 8 ? (b.bytes / 8 - 1) * 8 : 0;
        if (first_word_out) HIP_TRY(c, hipMemcpy(&first, b.p, take, hipMemcpyDeviceToHost));
        if (last_word_out) HIP_TRY(c, hipMemcpy(&last, (const char *)b.p + last_off, take, hipMemcpyDeviceToHost));
    }
    if (first_word_out) *first_word_out = first;
    if (last_word_out) *last_word_out = last;
    return FHEAES_OK;
}

int fheaes_workspace_poison(fheaes_ctx *c, int mode, uint64_t *bytes_out)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (mode != FHEAES_WS_POISON_FILL && mode != FHEAES_WS_POISON_RELEASE)
        return c->fail(FHEAES_ERR_INVALID, "workspace_poison: mode must be FHEAES_WS_POISON_FILL (0) or FHEAES_WS_POISON_RELEASE (1), got %d", mode);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t total = 0;
    for (const WsEntry &e : WS_TABLE) {
        DevBuf &b = *ws_buf(c, e);
        if (!b.p || !b.bytes) continue;
        total += b.bytes;
        if (mode == FHEAES_WS_POISON_RELEASE) {
            HIP_TRY(c, hipFree(b.p));
            b.p = nullptr; b.bytes = 0;
            continue;
        }
        const size_t words = b.bytes / 4, tail = b.bytes % 4;
        if (e.cls == FHEAES_WS_WORDS) {
            HIP_TRY(c, hipMemsetAsync(b.p, FHEAES_WS_PATTERN_WORDS, b.bytes, c->stream));
            continue;
        }
        // 32-bit fills: a quiet NaN whose two halves are equal, or the index 1; what is left of a size that is no multiple of 4 gets
        // the words' byte (a double buffer has none; a table's last bytes are read as bytes only, and must not be zero)
        const uint32_t v = e.cls == FHEAES_WS_F64 ? FHEAES_WS_PATTERN_F64_HALF : FHEAES_WS_PATTERN_TABLES;
        if (words) HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)b.p, (int)v, words, c->stream));
        if (tail) HIP_TRY(c, hipMemsetAsync((char *)b.p + words * 4, FHEAES_WS_PATTERN_WORDS, tail, c->stream));
    }
    if (mode == FHEAES_WS_POISON_FILL) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bytes_out) *bytes_out = total;
    return FHEAES_OK;
}

// Both uploads end in the same three conversions of the standard-domain words staged in HBM: KSK / PFPKSK -> balanced int8
// byte planes in MFMA fragment order, BSK -> Fourier.  `seeded`: the caller passed bodies only and the masks are
// regenerated on the GPU from the public 256-bit mask key (ChaCha20 stream of csrc/client.c) -- 0.19 GB over PCIe / xGMI
// instead of 1.04 GB.
static int upload_keys_impl(fheaes_ctx *c, const uint64_t *ksk, const uint64_t *bsk, const uint64_t *pfpksk, int memspace, bool seeded, const MaskKey &mask_key)
{
    if (!c || !ksk || !bsk || !pfpksk) return c ? c->fail(FHEAES_ERR_INVALID, "null key pointer") : FHEAES_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t kw = fheaes_key_words(c, FHEAES_KEY_KSK), bw = fheaes_key_words(c, FHEAES_KEY_BSK), pw = fheaes_key_words(c, FHEAES_KEY_PFPKSK);
    c->have_keys = false;
    // K1 / K3 keys: balanced int8 byte planes in MFMA fragment order (same byte count as the uint64 keys)
    const uint32_t rows1 = c->big * c->p.ks_level, ncol1 = c->n + 1;
    const uint32_t rows3 = c->big1 * c->p.pfks_level, ncol3 = c->k1 * FHE_N;
    c->ks_ksteps = (rows1 + KS_KSTEP - 1) / KS_KSTEP; c->ks_coltiles = (ncol1 + 15) / 16;
    c->pf_ksteps = (rows3 + KS_KSTEP - 1) / KS_KSTEP; c->pf_coltiles = (ncol3 + 15) / 16;
    const size_t frag1 = (size_t)c->ks_ksteps * c->ks_coltiles * 8 * 1024;
    const size_t frag3 = (size_t)c->k1 * c->pf_ksteps * c->pf_coltiles * 8 * 1024;
    if (!c->ksk_frag) TRY(ctx_malloc(c, (void **)&c->ksk_frag, frag1));
    if (!c->pfpksk_frag) TRY(ctx_malloc(c, (void **)&c->pfpksk_frag, frag3));
    if (!c->bskf) TRY(ctx_malloc(c, (void **)&c->bskf, bw * 8));
    c->ksk_frag_bytes = frag1; c->pfpksk_frag_bytes = frag3; c->bskf_bytes = bw * 8;
    // stage the standard-domain words in HBM (largest key first), transform, free
    void *tmp = nullptr, *tmp_body = nullptr;
    const size_t tmp_words = std::max(std::max(kw, bw), pw);
    // seeded: key ciphertext counts and body sizes
    const uint64_t cts[3] = {(uint64_t)rows1, (uint64_t)c->n * c->p.pbs_level * c->k1, (uint64_t)c->k1 * rows3};
    const uint32_t mask_w[3] = {c->n, c->big, c->big}, body_w[3] = {1, FHE_N, FHE_N};
    const uint64_t tags[3] = {3, 4, 5};                                  // MASK_TAG_* of csrc/client.c
    size_t body_max = 0;
    for (int i = 0; i < 3; ++i) body_max = std::max(body_max, (size_t)cts[i] * body_w[i]);
    if (memspace != FHEAES_DEVICE || seeded) TRY(ctx_malloc(c, &tmp, tmp_words * 8));
    if (seeded && memspace != FHEAES_DEVICE) {
        const int me = ctx_malloc(c, &tmp_body, body_max * 8);
        if (me != FHEAES_OK) { (void)hipFree(tmp); return me; }
    }
    hipError_t copy_err = hipSuccess;
    // which: 0 KSK, 1 BSK, 2 PFPKSK; returns the device pointer of the full standard-domain key
    auto staged = [&](int which, const uint64_t *src, size_t words) -> const uint64_t * {
        if (!seeded) {
            if (memspace == FHEAES_DEVICE) return src;
            hipError_t ce = hipMemcpyAsync(tmp, src, words * 8, hipMemcpyHostToDevice, c->stream);
            if (ce != hipSuccess && copy_err == hipSuccess) copy_err = ce;
            return (const uint64_t *)tmp;
        }
        const uint64_t *bodies = src;
        if (memspace != FHEAES_DEVICE) {
            hipError_t ce = hipMemcpyAsync(tmp_body, src, (size_t)cts[which] * body_w[which] * 8, hipMemcpyHostToDevice, c->stream);
            if (ce != hipSuccess && copy_err == hipSuccess) copy_err = ce;
            bodies = (const uint64_t *)tmp_body;
        }
        hipLaunchKernelGGL(expand_masks_kernel, dim3(8192), dim3(256), 0, c->stream, (uint64_t *)tmp, bodies, cts[which], mask_w[which], body_w[which],
                           mask_key, (uint32_t)tags[which]);
        return (const uint64_t *)tmp;
    };
    int rc = FHEAES_OK;
    {
        const uint64_t *d = staged(0, ksk, kw);
        const uint64_t threads = (uint64_t)c->ks_ksteps * c->ks_coltiles * 64;
        ks_launch_keybytes(dim3((unsigned)((threads + 255) / 256), 1), c->stream, d, (uint64_t)0, rows1, ncol1, c->ks_ksteps, c->ks_coltiles, c->ksk_frag);
        if (tmp) (void)hipStreamSynchronize(c->stream);
    }
    {
        const uint64_t *d = staged(2, pfpksk, pw);
        const uint64_t threads = (uint64_t)c->pf_ksteps * c->pf_coltiles * 64;
        ks_launch_keybytes(dim3((unsigned)((threads + 255) / 256), c->k1), c->stream, d, (uint64_t)rows3 * ncol3, rows3, ncol3, c->pf_ksteps, c->pf_coltiles,
                           c->pfpksk_frag);
        if (tmp) (void)hipStreamSynchronize(c->stream);
    }
    {
        // BSK: standard domain -> Fourier (the reference holds it in Fourier form already, many_wopbs.rs:34-35)
        const uint64_t *d = staged(1, bsk, bw);
        rc = launch_forward_fourier(c, d, bw / FHE_N, c->bskf, FHEAES_STAGE_GGSW_FFT);
        c->stage_launches[FHEAES_STAGE_GGSW_FFT] = 0; c->stage_units[FHEAES_STAGE_GGSW_FFT] = 0;
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (tmp) (void)hipFree(tmp);
    if (tmp_body) (void)hipFree(tmp_body);
    if (rc != FHEAES_OK) return rc;
    if (copy_err != hipSuccess) return c->fail(FHEAES_ERR_DEVICE, "key upload (host -> device copy): %s", hipGetErrorString(copy_err));
    if (e != hipSuccess) return c->fail(FHEAES_ERR_DEVICE, "key upload: %s", hipGetErrorString(e));
    HIP_TRY(c, hipGetLastError());
    if (c->prof) prof_flush(c);
    c->stage_ms[FHEAES_STAGE_GGSW_FFT] = 0;
    c->have_keys = true;
    return FHEAES_OK;
}

int fheaes_upload_keys(fheaes_ctx *c, const uint64_t *ksk, const uint64_t *bsk, const uint64_t *pfpksk, int memspace)
{
    CtxLock lock__(c);
    return upload_keys_impl(c, ksk, bsk, pfpksk, memspace, false, MaskKey{});
}

int fheaes_upload_keys_seeded(fheaes_ctx *c, const uint32_t *mask_key, const uint64_t *ksk_body, const uint64_t *bsk_body, const uint64_t *pfpksk_body,
                              int memspace)
{
    CtxLock lock__(c);
    if (!c || !mask_key) return c ? c->fail(FHEAES_ERR_INVALID, "null mask key") : FHEAES_ERR_INVALID;
    MaskKey k;
    memcpy(k.k, mask_key, sizeof k.k);                       // the 32-byte key itself is always a HOST array
    return upload_keys_impl(c, ksk_body, bsk_body, pfpksk_body, memspace, true, k);
}

// One upload over PCIe, then device-to-device copies of the CONVERTED key images (int8 fragment planes of KSK / PFPKSK, Fourier
// BSK: 1.04 GB) -- over xGMI when the contexts sit on different GPUs (hipMemcpyPeerAsync), inside HBM when they share one.
int fheaes_clone_keys(fheaes_ctx *dst, fheaes_ctx *src)
{
    if (!dst || !src) return FHEAES_ERR_INVALID;
    if (dst == src) return dst->fail(FHEAES_ERR_INVALID, "fheaes_clone_keys: source and destination are the same context");
    // both locks, in address order (two threads cloning in opposite directions must not deadlock)
    CtxLock l1(dst < src ? dst : src), l2(dst < src ? src : dst);
    if (!src->have_keys) return dst->fail(FHEAES_ERR_NOKEYS, "fheaes_clone_keys: the source context has no keys");
    if (memcmp(&dst->p, &src->p, sizeof(fheaes_params)) != 0) return dst->fail(FHEAES_ERR_INVALID, "fheaes_clone_keys: parameter sets differ");
    HIP_TRY(dst, hipSetDevice(src->device));
    HIP_TRY(dst, hipStreamSynchronize(src->stream));            // the source's conversions are complete
    HIP_TRY(dst, hipSetDevice(dst->device));
    dst->have_keys = false;
    dst->clone_path = FHEAES_CLONE_NONE; dst->clone_bytes = 0; dst->clone_seconds = 0.0;
    // Between two GPUs the copy is a direct xGMI transfer only if peer access is possible AND enabled; otherwise the runtime stages
    // it through host memory.  Ask, enable once per device pair ("already enabled" is fine), and remember which of the two it was.
    int path = FHEAES_CLONE_SAME_DEVICE;
    if (dst->device != src->device) {
        path = FHEAES_CLONE_STAGED;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dst->device, src->device) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(src->device, 0);           // the current device is dst's
            if (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) path = FHEAES_CLONE_PEER;
        }
        (void)hipGetLastError();                                                       // "already enabled" must not poison later HIP_TRY(hipGetLastError())
    }
    const auto t_clone = std::chrono::steady_clock::now();
    uint64_t moved = 0;
    struct { void **d; const void *s; size_t bytes; size_t *have; } img[3] = {
        {(void **)&dst->ksk_frag, src->ksk_frag, src->ksk_frag_bytes, &dst->ksk_frag_bytes},
        {(void **)&dst->pfpksk_frag, src->pfpksk_frag, src->pfpksk_frag_bytes, &dst->pfpksk_frag_bytes},
        {(void **)&dst->bskf, src->bskf, src->bskf_bytes, &dst->bskf_bytes}};
    for (auto &g : img) {
        if (*g.d && *g.have != g.bytes) { HIP_TRY(dst, hipStreamSynchronize(dst->stream)); HIP_TRY(dst, hipFree(*g.d)); *g.d = nullptr; }
        if (!*g.d) TRY(ctx_malloc(dst, g.d, g.bytes));
        *g.have = g.bytes;
        if (dst->device == src->device) HIP_TRY(dst, hipMemcpyAsync(*g.d, g.s, g.bytes, hipMemcpyDeviceToDevice, dst->stream));
        else HIP_TRY(dst, hipMemcpyPeerAsync(*g.d, dst->device, g.s, src->device, g.bytes, dst->stream));
        moved += g.bytes;
    }
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    dst->clone_path = path; dst->clone_bytes = moved;
    dst->clone_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_clone).count();
    dst->ks_ksteps = src->ks_ksteps; dst->ks_coltiles = src->ks_coltiles; dst->pf_ksteps = src->pf_ksteps; dst->pf_coltiles = src->pf_coltiles;
    dst->have_keys = true;
    return FHEAES_OK;
}

int fheaes_noise_level_seen(fheaes_ctx *c, uint32_t *max_seen, uint32_t *limit)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    if (max_seen) *max_seen = c->noise_level_seen;
    if (limit) *limit = FHEAES_MAX_NOISE_LEVEL;
    return FHEAES_OK;
}

int fheaes_clone_info(fheaes_ctx *c, int *path, uint64_t *bytes, double *seconds)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    if (path) *path = c->clone_path;
    if (bytes) *bytes = c->clone_bytes;
    if (seconds) *seconds = c->clone_seconds;
    return FHEAES_OK;
}

size_t fheaes_key_body_words(const fheaes_ctx *c, int which)
{
    if (!c) return 0;
    switch (which) {
    case FHEAES_KEY_KSK: return (size_t)c->big * c->p.ks_level;
    case FHEAES_KEY_BSK: return (size_t)c->n * c->p.pbs_level * c->k1 * FHE_N;
    case FHEAES_KEY_PFPKSK: return (size_t)c->k1 * c->big1 * c->p.pfks_level * FHE_N;
    default: return 0;
    }
}

int fheaes_read_bsk_fourier(fheaes_ctx *c, uint32_t i, double *out)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (i >= c->n || !out) return c->fail(FHEAES_ERR_INVALID, "bad GGSW index");
    const size_t words = (size_t)c->p.pbs_level * c->k1 * c->k1 * FHE_N;
    HIP_TRY(c, hipMemcpyAsync(out, (const double *)c->bskf + (size_t)i * words, words * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FHEAES_OK;
}

// ---- stage-by-stage ---------------------------------------------------------------------------
int fheaes_keyswitch_batch(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t m, uint64_t *lwe_out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!lwe_in || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(lwe_in, m * c->big1 * 8, &lwe_in));
    TRY(s.out(lwe_out, m * (c->n + 1) * 8, &lwe_out));
    TRY(launch_keyswitch(c, lwe_in, m, lwe_out));
    return s.finish();
}

int fheaes_cbs_pbs_batch(fheaes_ctx *c, const uint64_t *lwe_small, uint64_t m, uint32_t level, uint64_t *lwe_out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!lwe_small || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (level < 1 || level > c->p.cbs_level) return c->fail(FHEAES_ERR_INVALID, "cbs level %u out of range", level);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(lwe_small, m * (c->n + 1) * 8, &lwe_small));
    TRY(s.out(lwe_out, m * c->big1 * 8, &lwe_out));
    // one launch parks 64 KB per workgroup in ONE raw buffer of less than 2^31 bytes (launch_cbs_pbs refuses more): a batch beyond
    // K2_CALL_MAX_BITS is cut into launches of that many bits, as the WoPBS cuts its own at MAX_CHUNK_BITS
    for (uint64_t t0 = 0; t0 < m; t0 += K2_CALL_MAX_BITS) {
        const uint64_t mc = std::min<uint64_t>(K2_CALL_MAX_BITS, m - t0);
        TRY(launch_cbs_pbs(c, lwe_small + t0 * (c->n + 1), mc, level, lwe_out + t0 * c->big1));
    }
    return s.finish();
}

int fheaes_pfpks_batch(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t m, uint64_t *ggsw_rows_out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!lwe_in || !ggsw_rows_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t words = (uint64_t)c->k1 * c->k1 * FHE_N;
    Staged s(c, memspace);
    TRY(s.in(lwe_in, m * c->big1 * 8, &lwe_in));
    TRY(s.out(ggsw_rows_out, m * words * 8, &ggsw_rows_out));
    TRY(launch_pfpks(c, lwe_in, m, ggsw_rows_out, words));
    return s.finish();
}

int fheaes_forward_fourier_batch(fheaes_ctx *c, const uint64_t *polys_in, uint64_t polys, double *fourier_out, int memspace)
{
    CtxLock lock__(c);
    if (!c || !polys_in || !fourier_out) return c ? c->fail(FHEAES_ERR_INVALID, "null pointer") : FHEAES_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(polys_in, polys * FHE_N * 8, &polys_in));
    TRY(s.out(fourier_out, polys * FHE_N * 8, &fourier_out));
    TRY(launch_forward_fourier(c, polys_in, polys, (double2 *)fourier_out, FHEAES_STAGE_GGSW_FFT));
    return s.finish();
}

int fheaes_vertical_packing_batch(fheaes_ctx *c, const double *ggsw_fourier, uint64_t n_inputs, uint32_t bits, const uint64_t *luts,
                                  uint32_t n_luts, int lut_per_input, uint64_t *lwe_out, int memspace)
{
    CtxLock lock__(c);
    if (!c || !ggsw_fourier || !luts || !lwe_out) return c ? c->fail(FHEAES_ERR_INVALID, "null pointer") : FHEAES_ERR_INVALID;
    if (bits < 1 || bits > MAX_WOPBS_BITS || n_luts < 1) return c->fail(FHEAES_ERR_INVALID, "bits must be 1..%u and n_luts >= 1", MAX_WOPBS_BITS);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    const uint64_t gw = (uint64_t)c->k1 * c->k1 * FHE_N;
    const uint64_t sets = lut_per_input ? n_inputs : 1;
    TRY(s.in(ggsw_fourier, n_inputs * bits * gw * 8, &ggsw_fourier));
    TRY(s.in(luts, sets * n_luts * bits * lut_row_words(bits) * 8, &luts));
    TRY(s.out(lwe_out, n_inputs * n_luts * bits * c->big1 * 8, &lwe_out));
    TRY(launch_vertical_packing(c, (const double2 *)ggsw_fourier, n_inputs, bits, luts, n_luts, lut_per_input, lwe_out));
    return s.finish();
}

// ---- plugin API -------------------------------------------------------------------------------
int fheaes_wopbs_batch(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t n_inputs, uint32_t bits, const uint64_t *luts, uint32_t n_luts,
                       int lut_per_input, uint64_t *lwe_out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!lwe_in || !luts || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    // host memory: the sizes below need a valid width, so it is refused here; device memory uses no size and leaves that to wopbs_dev (its own text)
    if (s.host && (bits < 1 || bits > MAX_WOPBS_BITS || n_luts < 1)) return c->fail(FHEAES_ERR_INVALID, "bits must be 1..%u and n_luts >= 1", MAX_WOPBS_BITS);
    const uint64_t sets = lut_per_input ? n_inputs : 1, W = s.host ? lut_row_words(bits) : 0;
    TRY(s.in(lwe_in, n_inputs * bits * c->big1 * 8, &lwe_in));
    TRY(s.in(luts, sets * n_luts * bits * W * 8, &luts));
    TRY(s.out(lwe_out, n_inputs * n_luts * bits * c->big1 * 8, &lwe_out));
    TRY(wopbs_dev(c, lwe_in, n_inputs, bits, luts, n_luts, lut_per_input, lwe_out));
    return s.finish();
}

int fheaes_many_sbox(fheaes_ctx *c, const uint64_t *bytes, uint64_t n_bytes, int inv, uint64_t *out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!bytes || !out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    const int set = inv ? LUTSET_DEC_MUL : LUTSET_ENC_ROUND;
    Staged s(c, memspace);
    const uint64_t bw = 8ull * c->big1;
    TRY(s.in(bytes, n_bytes * bw * 8, &bytes));
    TRY(s.out(out, n_bytes * c->lutset_n[set] * bw * 8, &out));
    TRY(many_sbox_dev(c, bytes, n_bytes, set, out));
    return s.finish();
}

int fheaes_sbox(fheaes_ctx *c, uint64_t *bytes, uint64_t n_bytes, int inv, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!bytes) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    const int set = inv ? LUTSET_INV_SBOX : LUTSET_SBOX;
    const uint64_t bw = 8ull * c->big1;
    // in place for the caller only: the S-Boxes are written to ws_vp and copied back over their inputs
    Staged s(c, memspace);
    TRY(s.inout(bytes, n_bytes * bw * 8, &bytes));
    TRY(ensure(c, c->ws_vp, n_bytes * bw * 8));
    TRY(many_sbox_dev(c, bytes, n_bytes, set, (uint64_t *)c->ws_vp.p));
    HIP_TRY(c, hipMemcpyAsync(bytes, c->ws_vp.p, n_bytes * bw * 8, hipMemcpyDeviceToDevice, c->stream));
    return s.finish();
}

static bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

static int check_n_keys(fheaes_ctx *c, uint64_t n_keys)
{
    if (n_keys == 0 || n_keys > FHEAES_MAX_KEYS) return c->fail(FHEAES_ERR_INVALID, "n_keys must be in 1..%u (got %llu)", (unsigned)FHEAES_MAX_KEYS, (unsigned long long)n_keys);
    return FHEAES_OK;
}

// key_of_block (HOST, n_blocks entries) names one of n_keys sets of round keys per block
static int check_key_of_block(fheaes_ctx *c, const uint32_t *key_of_block, uint64_t n_blocks, uint64_t n_keys)
{
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (key_of_block[b] >= n_keys)
            return c->fail(FHEAES_ERR_INVALID, "key_of_block[%llu] = %u, but there are %llu keys", (unsigned long long)b, key_of_block[b], (unsigned long long)n_keys);
    return FHEAES_OK;
}

// G GLWEs hold the (Nr+1) 128 bits of one key's round keys; 0: not an AES key size
static uint32_t packed_key_glwes(uint32_t key_bits)
{
    const int nr = aes_rounds(key_bits);
    return nr ? (uint32_t)(((uint64_t)(nr + 1) * AES_BLOCK_BITS + FHE_N - 1) / FHE_N) : 0;
}

// The round keys of a cipher call.  What the caller says: `words`, n_keys sets of them for AES-`key_bits`, in LWE form
// [n_keys][Nr+1][16][8][kN+1] or (`packed`) a store [n_keys][G][(k+1)N] of fheaes_pack_round_keys, and key_of[i] (HOST, n_of entries), the
// set block or stream i works under -- null: the one set of a single-key entry point.  resolve_keys() refuses what is wrong with that and
// fills in the rest: Nr, the words from one key to the next (KeySets' stride), G (0: LWE form) and the bytes the call reads.
struct RoundKeys {
    const uint64_t *words; uint32_t key_bits; uint64_t n_keys; const uint32_t *key_of; uint64_t n_of; bool packed;
    int nr = 0; uint32_t glwes = 0; uint64_t key_words = 0, keys_bytes = 0;
    bool overlaps(const void *p, uint64_t bytes) const { return overlap(words, keys_bytes, p, bytes); }
    int stage(Staged &s) { return s.in(words, keys_bytes, &words); }
    // of_block: the DEVICE copy of key_of (aes_crypt); null where the call's plan carries the key of every block
    KeySets sets(const uint32_t *of_block = nullptr) const { return {words, of_block, key_words, glwes}; }
};
// max_streams: the bound on n_of of the calls on streams (it sits where they have always refused it, in front of the table's entries)
static int resolve_keys(fheaes_ctx *c, RoundKeys &k, uint64_t max_streams = ~0ull)
{
    TRY(check_key_bits(c, k.key_bits));
    TRY(check_n_keys(c, k.n_keys));
    if (k.n_of > max_streams) return c->fail(FHEAES_ERR_INVALID, "n_streams must be at most %llu (got %llu)", (unsigned long long)max_streams, (unsigned long long)k.n_of);
    if (k.key_of) TRY(check_key_of_block(c, k.key_of, k.n_of, k.n_keys));
    k.nr = aes_rounds(k.key_bits);
    k.glwes = k.packed ? packed_key_glwes(k.key_bits) : 0;
    k.key_words = k.packed ? (uint64_t)k.glwes * c->k1 * FHE_N : (uint64_t)(k.nr + 1) * 16 * 8 * c->big1;
    k.keys_bytes = k.n_keys * k.key_words * 8;
    return FHEAES_OK;
}

static RoundKeys one_key(const uint64_t *words, uint32_t key_bits, bool packed = false) { return {words, key_bits, 1, nullptr, 0, packed}; }

// The three block ciphers, in place.  keyed: block b runs under set key_of[b], the table going to the device through the pinned buffer
// (one key: no table); else the single-key entry points, one set and no table.
static int aes_crypt(fheaes_ctx *c, RoundKeys k, bool keyed, uint64_t *state, uint64_t n_blocks, int memspace, AesDevFn dev)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!k.words || (keyed && !k.key_of) || !state) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(resolve_keys(c, k));
    if (keyed && n_blocks == 0) return FHEAES_OK;
    const uint64_t sw = 16ull * 8 * c->big1;
    if (k.packed && k.overlaps(state, n_blocks * sw * 8)) return c->fail(FHEAES_ERR_INVALID, "the packed round keys and the state overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(k.stage(s));
    TRY(s.inout(state, n_blocks * sw * 8, &state));
    const uint32_t *table = nullptr;
    if (keyed && k.n_keys > 1) {
        TRY(upload_pinned(c, n_blocks * sizeof(uint32_t), n_blocks * sizeof(uint32_t), [&](uint8_t *pin) { memcpy(pin, k.key_of, n_blocks * sizeof(uint32_t)); }));
        table = (const uint32_t *)c->ws_misc.p;
    }
    TRY(dev(c, k.sets(table), state, n_blocks, k.nr));
    return s.finish();
}

int fheaes_aes_encrypt_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, one_key(round_keys, key_bits), false, state, n_blocks, memspace, aes_encrypt_dev);
}

int fheaes_aes_encrypt(fheaes_ctx *c, const uint64_t *round_keys, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return fheaes_aes_encrypt_bits(c, round_keys, 128, state, n_blocks, memspace);
}

int fheaes_aes_decrypt_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, one_key(round_keys, key_bits), false, state, n_blocks, memspace, aes_decrypt_dev);
}

int fheaes_aes_decrypt(fheaes_ctx *c, const uint64_t *round_keys, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return fheaes_aes_decrypt_bits(c, round_keys, 128, state, n_blocks, memspace);
}

int fheaes_aes_decrypt_equivalent_bits(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks,
                                       int memspace)
{
    return aes_crypt(c, one_key(dec_round_keys, key_bits), false, state, n_blocks, memspace, aes_decrypt_eq_dev);
}

int fheaes_aes_decrypt_equivalent(fheaes_ctx *c, const uint64_t *dec_round_keys, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return fheaes_aes_decrypt_equivalent_bits(c, dec_round_keys, 128, state, n_blocks, memspace);
}

int fheaes_aes_encrypt_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block, uint64_t *state,
                             uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {round_keys, key_bits, n_keys, key_of_block, n_blocks, false}, true, state, n_blocks, memspace, aes_encrypt_dev);
}

int fheaes_aes_decrypt_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block, uint64_t *state,
                             uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {round_keys, key_bits, n_keys, key_of_block, n_blocks, false}, true, state, n_blocks, memspace, aes_decrypt_dev);
}

int fheaes_aes_decrypt_equivalent_keyed(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                        uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {dec_round_keys, key_bits, n_keys, key_of_block, n_blocks, false}, true, state, n_blocks, memspace, aes_decrypt_eq_dev);
}

int fheaes_aes_encrypt_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                    uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {packed_round_keys, key_bits, n_keys, key_of_block, n_blocks, true}, true, state, n_blocks, memspace, aes_encrypt_dev);
}

int fheaes_aes_decrypt_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                    uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {packed_round_keys, key_bits, n_keys, key_of_block, n_blocks, true}, true, state, n_blocks, memspace, aes_decrypt_dev);
}

int fheaes_aes_decrypt_equivalent_keyed_packed(fheaes_ctx *c, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keys,
                                               const uint32_t *key_of_block, uint64_t *state, uint64_t n_blocks, int memspace)
{
    return aes_crypt(c, {packed_dec_round_keys, key_bits, n_keys, key_of_block, n_blocks, true}, true, state, n_blocks, memspace, aes_decrypt_eq_dev);
}

// the two per-key calls: n_keys sets in, n_keys sets out
static int dec_round_keys(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *dec_round_keys, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!round_keys || !dec_round_keys) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(check_key_bits(c, key_bits));
    TRY(check_n_keys(c, n_keys));
    const int nr = aes_rounds(key_bits);
    const uint64_t sw = 16ull * 8 * c->big1, bytes = n_keys * (uint64_t)(nr + 1) * sw * 8;
    if (overlap(round_keys, bytes, dec_round_keys, bytes)) return c->fail(FHEAES_ERR_INVALID, "round_keys and dec_round_keys overlap (the conversion is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(round_keys, bytes, &round_keys));
    TRY(s.out(dec_round_keys, bytes, &dec_round_keys));
    TRY(dec_round_keys_dev(c, round_keys, dec_round_keys, nr, n_keys));
    return s.finish();
}

int fheaes_aes_decryption_round_keys_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t *dec_round_keys_out, int memspace)
{
    return dec_round_keys(c, round_keys, key_bits, 1, dec_round_keys_out, memspace);
}

int fheaes_aes_decryption_round_keys(fheaes_ctx *c, const uint64_t *round_keys, uint64_t *dec_round_keys_out, int memspace)
{
    return fheaes_aes_decryption_round_keys_bits(c, round_keys, 128, dec_round_keys_out, memspace);
}

int fheaes_aes_decryption_round_keys_batch(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *dec_round_keys_out,
                                           int memspace)
{
    return dec_round_keys(c, round_keys, key_bits, n_keys, dec_round_keys_out, memspace);
}

static int key_expansion(fheaes_ctx *c, const uint64_t *key, uint32_t key_bits, uint64_t n_keys, uint64_t *round_keys, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!key || !round_keys) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(check_key_bits(c, key_bits));
    TRY(check_n_keys(c, n_keys));
    const int nr = aes_rounds(key_bits);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    const uint64_t bw = 8ull * c->big1, sw = 16 * bw;
    TRY(s.in(key, n_keys * (key_bits / 8) * bw * 8, &key));
    TRY(s.out(round_keys, n_keys * (uint64_t)(nr + 1) * sw * 8, &round_keys));
    TRY(key_expansion_dev(c, key, round_keys, nr, n_keys));
    return s.finish();
}

int fheaes_aes_key_expansion_bits(fheaes_ctx *c, const uint64_t *key, uint32_t key_bits, uint64_t *round_keys, int memspace)
{
    return key_expansion(c, key, key_bits, 1, round_keys, memspace);
}

int fheaes_aes_key_expansion(fheaes_ctx *c, const uint64_t *key, uint64_t *round_keys, int memspace)
{
    return fheaes_aes_key_expansion_bits(c, key, 128, round_keys, memspace);
}

int fheaes_aes_key_expansion_batch(fheaes_ctx *c, const uint64_t *keys, uint32_t key_bits, uint64_t n_keys, uint64_t *round_keys, int memspace)
{
    return key_expansion(c, keys, key_bits, n_keys, round_keys, memspace);
}

int fheaes_add_scalar(fheaes_ctx *c, uint64_t *state, uint64_t n_blocks, const uint64_t *counters_hi_lo, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!state || !counters_hi_lo) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_blocks == 0) return FHEAES_OK;
    Staged s(c, memspace);
    const uint64_t sw = 16ull * 8 * c->big1;
    TRY(s.inout(state, n_blocks * sw * 8, &state));
    TRY(add_scalar_dev(c, state, n_blocks, counters_hi_lo));
    return s.finish();
}

// The public-block calls, all eight of them.  An entry point says which direction, whether every pointer it requires is there (have_args)
// and what the blocks are: blocks_of(scratch) returns {blocks, data} -- the caller's own lists, or ones it builds in `scratch` (CTR, CBC),
// which happens only once the call is known to run.  k.key_of null: every block under the one set (decryption round keys for public_inverse()).
struct PublicBlocks { const uint64_t *blocks, *data; };
using BlocksOf = std::function<PublicBlocks(std::vector<uint64_t> &)>;
static BlocksOf given(const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo)
{
    return [=](std::vector<uint64_t> &) { return PublicBlocks{blocks_hi_lo, data_hi_lo}; };
}

static int aes_public(fheaes_ctx *c, const PublicDirection &dir, RoundKeys k, bool have_args, const BlocksOf &blocks_of, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!have_args) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(resolve_keys(c, k));
    if (n_blocks == 0) return FHEAES_OK;
    const uint64_t sw = 16ull * 8 * c->big1;
    if (k.packed && k.overlaps(state_out, n_blocks * sw * 8)) return c->fail(FHEAES_ERR_INVALID, "the packed round keys and state_out overlap");
    if (n_blocks > PUBLIC_MAX_BLOCKS) return c->fail(FHEAES_ERR_INVALID, "n_blocks must be at most %llu", (unsigned long long)PUBLIC_MAX_BLOCKS);
    std::vector<uint64_t> scratch;
    const PublicBlocks pb = blocks_of(scratch);
    HIP_TRY(c, hipSetDevice(c->device));
    PublicPlan pl;
    public_plan(dir, pb.blocks, pb.data, k.key_of, n_blocks, k.nr, pl);
    Staged s(c, memspace);
    TRY(k.stage(s));
    TRY(s.out(state_out, n_blocks * sw * 8, &state_out));
    TRY(aes_public_dev(c, dir, k.sets(), pl, k.nr, state_out));
    return s.finish();
}

int fheaes_aes_encrypt_public_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *blocks_hi_lo, uint64_t n_blocks,
                                   uint64_t *state_out, int memspace)
{
    return aes_public(c, public_forward(), one_key(round_keys, key_bits), round_keys && blocks_hi_lo && state_out, given(blocks_hi_lo, nullptr), n_blocks, state_out, memspace);
}

// counter block i = iv with its low `width` bits replaced by (those bits + first_block + i) mod 2^width: SP 800-38A appendix B.1 with m = 128,
// and with m = 32 the inc32 of SP 800-38D (iv being the initial counter block)
static void ctr_blocks(const uint64_t *iv_hi_lo, uint64_t first_block, uint64_t n_blocks, uint32_t width, std::vector<uint64_t> &ctr)
{
    const uint64_t count_hi = width > 64 ? ~0ull >> (128 - width) : 0, count_lo = width >= 64 ? ~0ull : ~0ull >> (64 - width);
    const uint64_t lo0 = iv_hi_lo[1] + first_block, hi0 = iv_hi_lo[0] + (lo0 < first_block ? 1 : 0);
    ctr.resize(2 * n_blocks);
    for (uint64_t i = 0; i < n_blocks; ++i) {
        const uint64_t lo = lo0 + i, hi = hi0 + (lo < lo0 ? 1 : 0);
        ctr[2 * i] = (iv_hi_lo[0] & ~count_hi) | (hi & count_hi);
        ctr[2 * i + 1] = (iv_hi_lo[1] & ~count_lo) | (lo & count_lo);
    }
}

static int aes_ctr(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *iv_hi_lo, uint64_t first_block, uint32_t width,
                   const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public(c, public_forward(), one_key(round_keys, key_bits), round_keys && iv_hi_lo && state_out, [&](std::vector<uint64_t> &ctr) {
        ctr_blocks(iv_hi_lo, first_block, n_blocks, width, ctr);
        return PublicBlocks{ctr.data(), data_hi_lo};
    }, n_blocks, state_out, memspace);
}

int fheaes_aes_ctr_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *iv_hi_lo, uint64_t first_block,
                        const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_ctr(c, round_keys, key_bits, iv_hi_lo, first_block, 128, data_hi_lo, n_blocks, state_out, memspace);
}

int fheaes_aes_ctr32_bits(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *icb_hi_lo, uint64_t first_block,
                          const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_ctr(c, round_keys, key_bits, icb_hi_lo, first_block, 32, data_hi_lo, n_blocks, state_out, memspace);
}

// the four keyed calls: forward or through the equivalent inverse cipher (decryption round keys), LWE-form keys or a packed store
static int aes_public_keyed(fheaes_ctx *c, const PublicDirection &dir, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                            const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace, bool packed)
{
    return aes_public(c, dir, {round_keys, key_bits, n_keys, key_of_block, n_blocks, packed}, round_keys && key_of_block && blocks_hi_lo && state_out,
                      given(blocks_hi_lo, data_hi_lo), n_blocks, state_out, memspace);
}

int fheaes_aes_public_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                            const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public_keyed(c, public_forward(), round_keys, key_bits, n_keys, key_of_block, blocks_hi_lo, data_hi_lo, n_blocks, state_out, memspace, false);
}

int fheaes_aes_public_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                   const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public_keyed(c, public_forward(), packed_round_keys, key_bits, n_keys, key_of_block, blocks_hi_lo, data_hi_lo, n_blocks, state_out, memspace, true);
}

int fheaes_aes_decrypt_public_bits(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo,
                                   uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public(c, public_inverse(), one_key(dec_round_keys, key_bits), dec_round_keys && blocks_hi_lo && state_out, given(blocks_hi_lo, data_hi_lo), n_blocks,
                      state_out, memspace);
}

int fheaes_aes_decrypt_public_keyed(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                    const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public_keyed(c, public_inverse(), dec_round_keys, key_bits, n_keys, key_of_block, blocks_hi_lo, data_hi_lo, n_blocks, state_out, memspace, false);
}

int fheaes_aes_decrypt_public_keyed_packed(fheaes_ctx *c, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                                           const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_public_keyed(c, public_inverse(), packed_dec_round_keys, key_bits, n_keys, key_of_block, blocks_hi_lo, data_hi_lo, n_blocks, state_out, memspace, true);
}

int fheaes_aes_cbc_decrypt_bits(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, const uint64_t *iv_hi_lo, const uint64_t *ct_hi_lo,
                                uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    // P_i = D_K(C_i) ^ C_{i-1}, C_{-1} = iv (SP 800-38A 6.2): the chaining blocks are the ciphertext moved down by one block
    return aes_public(c, public_inverse(), one_key(dec_round_keys, key_bits), dec_round_keys && iv_hi_lo && ct_hi_lo && state_out, [&](std::vector<uint64_t> &chain) {
        chain.resize(2 * n_blocks);
        chain[0] = iv_hi_lo[0]; chain[1] = iv_hi_lo[1];
        memcpy(chain.data() + 2, ct_hi_lo, 2 * (n_blocks - 1) * sizeof(uint64_t));
        return PublicBlocks{ct_hi_lo, chain.data()};
    }, n_blocks, state_out, memspace);
}

static void plan_counts(const PublicPlan &pl, uint64_t n_blocks, int nr, uint64_t *unique_bytes_per_round)
{
    for (int r = 1; r <= nr; ++r) unique_bytes_per_round[r - 1] = n_blocks ? pl.layers[r - 1].n : 0;
}

int fheaes_aes_public_plan(const uint64_t *blocks_hi_lo, uint64_t n_blocks, uint32_t key_bits, uint64_t *unique_bytes_per_round)
{
    const int nr = aes_rounds(key_bits);
    if (!blocks_hi_lo || !unique_bytes_per_round || !nr || n_blocks > PUBLIC_MAX_BLOCKS) return FHEAES_ERR_INVALID;
    PublicPlan pl;
    if (n_blocks) public_plan(public_forward(), blocks_hi_lo, nullptr, nullptr, n_blocks, nr, pl);
    plan_counts(pl, n_blocks, nr, unique_bytes_per_round);
    return FHEAES_OK;
}

int fheaes_aes_public_plan_keyed(const uint64_t *blocks_hi_lo, const uint32_t *key_of_block, uint64_t n_blocks, uint64_t n_keys, uint32_t key_bits,
                                 uint64_t *unique_bytes_per_round)
{
    const int nr = aes_rounds(key_bits);
    if (!blocks_hi_lo || !key_of_block || !unique_bytes_per_round || !nr || n_blocks > PUBLIC_MAX_BLOCKS || n_keys == 0 || n_keys > FHEAES_MAX_KEYS)
        return FHEAES_ERR_INVALID;
    for (uint64_t b = 0; b < n_blocks; ++b) if (key_of_block[b] >= n_keys) return FHEAES_ERR_INVALID;
    PublicPlan pl;
    if (n_blocks) public_plan(public_forward(), blocks_hi_lo, nullptr, key_of_block, n_blocks, nr, pl);
    plan_counts(pl, n_blocks, nr, unique_bytes_per_round);
    return FHEAES_OK;
}

int fheaes_aes_decrypt_public_plan_keyed(const uint64_t *blocks_hi_lo, const uint32_t *key_of_block, uint64_t n_blocks, uint64_t n_keys, uint32_t key_bits,
                                         uint64_t *unique_bytes_per_round)
{
    const int nr = aes_rounds(key_bits);
    if (!blocks_hi_lo || !unique_bytes_per_round || !nr || n_blocks > PUBLIC_MAX_BLOCKS || n_keys == 0 || n_keys > FHEAES_MAX_KEYS) return FHEAES_ERR_INVALID;
    if (key_of_block) for (uint64_t b = 0; b < n_blocks; ++b) if (key_of_block[b] >= n_keys) return FHEAES_ERR_INVALID;
    PublicPlan pl;
    if (n_blocks) public_plan(public_inverse(), blocks_hi_lo, nullptr, key_of_block, n_blocks, nr, pl);
    plan_counts(pl, n_blocks, nr, unique_bytes_per_round);
    return FHEAES_OK;
}

// K6 alone: the four-term gather without a round key (table_dec_mix(): InvMixColumns over the {9, 11, 13, 14} multiples), as
// fheaes_aes_decrypt_bits and the round-key conversion launch it
int fheaes_inv_mix_columns_batch(fheaes_ctx *c, const uint64_t *multiples, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (n_blocks == 0) return FHEAES_OK;
    if (!multiples || !state_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_blocks > 65535) return c->fail(FHEAES_ERR_INVALID, "n_blocks must be at most 65,535 (one grid), got %llu", (unsigned long long)n_blocks);
    const uint64_t out_bytes = n_blocks * 16 * 8 * c->big1 * 8, in_bytes = 4 * out_bytes;
    if (overlap(multiples, in_bytes, state_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "multiples and state_out overlap (the gather is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(multiples, in_bytes, &multiples));
    TRY(s.out(state_out, out_bytes, &state_out));
    TRY(launch_gather(c, multiples, 4, KeySets{nullptr, nullptr, 0}, state_out, n_blocks, table_dec_mix()));
    return s.finish();
}

// ---- XTS-AES decryption -----------------------------------------------------------------------
// k1: the decryption round keys of key 1, k2: the round keys of key 2, both of one size and in one form
static int aes_xts_decrypt(fheaes_ctx *c, RoundKeys k1, RoundKeys k2, const uint64_t *tweaks_hi_lo, uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block,
                           const uint64_t *ct_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!k1.words || !k2.words || !tweaks_hi_lo || !ct_hi_lo || !state_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (k1.key_bits != 128 && k1.key_bits != 256) return c->fail(FHEAES_ERR_INVALID, "XTS-AES has two keys of 128 or 256 bits each (key_bits %u)", k1.key_bits);
    if (blocks_per_unit == 0 || blocks_per_unit > XTS_MAX_BLOCKS_PER_UNIT)
        return c->fail(FHEAES_ERR_INVALID, "blocks_per_unit must be in 1..%u (got %llu)", XTS_MAX_BLOCKS_PER_UNIT, (unsigned long long)blocks_per_unit);
    if (n_blocks == 0) return FHEAES_OK;
    XtsPlan pl;
    if (!xts_plan(n_units, blocks_per_unit, first_block, n_blocks, true, pl))
        return c->fail(FHEAES_ERR_INVALID, "blocks %llu .. of %llu units of %llu blocks: n_units must cover the blocks of the call (and their tweaks number below 2^32)",
                       (unsigned long long)first_block, (unsigned long long)n_units, (unsigned long long)blocks_per_unit);
    if (pl.units > PUBLIC_MAX_BLOCKS) return c->fail(FHEAES_ERR_INVALID, "a call touches at most %llu data units", (unsigned long long)PUBLIC_MAX_BLOCKS);
    TRY(resolve_keys(c, k1));
    TRY(resolve_keys(c, k2));
    const uint64_t sw = 16ull * 8 * c->big1, out_bytes = n_blocks * sw * 8;
    if (k1.overlaps(state_out, out_bytes) || k2.overlaps(state_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "the round keys and state_out overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(k1.stage(s));
    TRY(k2.stage(s));
    TRY(s.out(state_out, out_bytes, &state_out));
    TRY(aes_xts_decrypt_dev(c, k1.sets(), k2.sets(), k1.nr, tweaks_hi_lo, pl, ct_hi_lo, n_blocks, state_out));
    return s.finish();
}

int fheaes_aes_xts_decrypt_bits(fheaes_ctx *c, const uint64_t *dec_round_keys1, const uint64_t *round_keys2, uint32_t key_bits, const uint64_t *tweaks_hi_lo,
                                uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block, const uint64_t *ct_hi_lo, uint64_t n_blocks, uint64_t *state_out,
                                int memspace)
{
    return aes_xts_decrypt(c, one_key(dec_round_keys1, key_bits), one_key(round_keys2, key_bits), tweaks_hi_lo, n_units, blocks_per_unit, first_block, ct_hi_lo, n_blocks,
                           state_out, memspace);
}

int fheaes_aes_xts_decrypt_packed(fheaes_ctx *c, const uint64_t *packed_dec_round_keys1, const uint64_t *packed_round_keys2, uint32_t key_bits,
                                  const uint64_t *tweaks_hi_lo, uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block, const uint64_t *ct_hi_lo,
                                  uint64_t n_blocks, uint64_t *state_out, int memspace)
{
    return aes_xts_decrypt(c, one_key(packed_dec_round_keys1, key_bits, true), one_key(packed_round_keys2, key_bits, true), tweaks_hi_lo, n_units, blocks_per_unit,
                           first_block, ct_hi_lo, n_blocks, state_out, memspace);
}

int fheaes_xts_tweaks(fheaes_ctx *c, const uint64_t *anchor, uint64_t n_units, uint32_t first_offset, uint32_t n_offsets, uint64_t *out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (n_offsets == 0 || first_offset > XTS_MAX_OFFSET || n_offsets > XTS_MAX_OFFSET + 1 - first_offset)
        return c->fail(FHEAES_ERR_INVALID, "XTS tweak offsets %u .. : one gather reaches offset %u at most and takes at least one", first_offset, XTS_MAX_OFFSET);
    if (n_units == 0) return FHEAES_OK;
    if (!anchor || !out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t tw = AES_BLOCK_BITS * c->big1, in_bytes = n_units * tw * 8, out_bytes = in_bytes * n_offsets;
    if (overlap(anchor, in_bytes, out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "anchor and out overlap (the gather is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(anchor, in_bytes, &anchor));
    TRY(s.out(out, out_bytes, &out));
    TRY(launch_xts_tweaks(c, anchor, tw, n_units, first_offset, n_offsets, out));
    return s.finish();
}

int fheaes_xts_tweak_row(uint32_t offset, uint32_t bit, uint32_t *sources_out, uint32_t *n_sources)
{
    if (offset > XTS_MAX_OFFSET || bit > 127 || !sources_out || !n_sources) return FHEAES_ERR_INVALID;
    uint32_t s[4] = {0, 0, 0, 0};
    *n_sources = xts_tweak_row(offset, bit, s);
    memcpy(sources_out, s, sizeof s);
    return FHEAES_OK;
}

int fheaes_aes_xts_plan(uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block, uint64_t n_blocks, uint32_t key_bits, uint64_t *segments,
                        uint64_t *tweak_refresh_bytes, uint64_t *cipher_bytes, uint32_t *max_terms)
{
    if (!segments || !tweak_refresh_bytes || !cipher_bytes || !max_terms || (key_bits != 128 && key_bits != 256)) return FHEAES_ERR_INVALID;
    XtsPlan pl;
    if (!xts_plan(n_units, blocks_per_unit, first_block, n_blocks, false, pl)) return FHEAES_ERR_INVALID;
    *segments = pl.segments.size();
    *tweak_refresh_bytes = 16 * (pl.units + pl.rows);                   // the anchors of segment 0, then every gathered tweak
    *cipher_bytes = 16ull * aes_rounds(key_bits) * n_blocks;
    // what the call declares to the noise guard: the gather's largest row, 2 going into the cipher, 5 in its rounds, 3 coming out
    uint32_t terms = n_blocks ? 5 : 0, s[4];
    for (const auto &seg : pl.segments) for (const XtsGather &g : seg)
        for (uint32_t j = g.off0; j < g.off0 + g.n_off; ++j) for (uint32_t i = 0; i < 128; ++i) terms = std::max(terms, xts_tweak_row(j, i, s));
    *max_terms = terms;
    return FHEAES_OK;
}

// K6 alone: the XTS whitening on caller buffers (the yardstick of the CBC-MAC link, tools/ccm.py)
int fheaes_xts_whiten(fheaes_ctx *c, uint64_t *dst, const uint64_t *src, const uint64_t *tweaks, uint64_t n_tweaks, const uint32_t *tweak_of_block, const uint8_t *clear,
                      uint64_t n_blocks, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (n_blocks == 0) return FHEAES_OK;
    if (!dst || !tweaks || !tweak_of_block) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_blocks > MAC_MAX_STREAMS) return c->fail(FHEAES_ERR_INVALID, "n_blocks must be at most %u (got %llu)", MAC_MAX_STREAMS, (unsigned long long)n_blocks);
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (tweak_of_block[b] >= n_tweaks)
            return c->fail(FHEAES_ERR_INVALID, "tweak_of_block[%llu] = %u, but there are %llu tweaks", (unsigned long long)b, tweak_of_block[b], (unsigned long long)n_tweaks);
    const uint64_t sw = 16ull * 8 * c->big1, bytes = n_blocks * sw * 8;
    if (overlap(tweaks, n_tweaks * sw * 8, dst, bytes) || (src && src != dst && overlap(src, bytes, dst, bytes))) return c->fail(FHEAES_ERR_INVALID, "dst overlaps an input");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    const bool in_place = src == dst;
    if (in_place) TRY(st.inout(dst, bytes, &dst)); else TRY(st.out(dst, bytes, &dst));
    if (in_place) src = dst; else if (src) TRY(st.in(src, bytes, &src));
    TRY(st.in(tweaks, n_tweaks * sw * 8, &tweaks));
    const size_t tab_bytes = n_blocks * sizeof(uint32_t), all_bytes = tab_bytes + (clear ? 16 * n_blocks : 0);
    TRY(upload_pinned(c, all_bytes, all_bytes, [&](uint8_t *pin) {
        memcpy(pin, tweak_of_block, tab_bytes);
        if (clear) memcpy(pin + tab_bytes, clear, 16 * n_blocks);
    }));
    TRY(launch_xts_whiten(c, dst, src, tweaks, (const uint32_t *)c->ws_misc.p, clear ? (const uint8_t *)c->ws_misc.p + tab_bytes : nullptr, n_blocks, src ? 3 : 2));
    return st.finish();
}

// ---- CBC-MAC chains and CCM decryption --------------------------------------------------------
// what every call on streams checks first, resolve_keys(.., MAC_MAX_STREAMS): the keys and the table that names one per stream
// k.key_of: the key of every stream, k.n_of of them
static int aes_cbc_mac(fheaes_ctx *c, RoundKeys k, const uint32_t *stream_blocks, const uint8_t *clear, const uint64_t *enc, const uint8_t *enc_bytes, const uint64_t *init,
                       uint64_t *mac_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    const uint64_t n_streams = k.n_of;
    const uint32_t *key_of_stream = k.key_of;
    if (!k.words || !key_of_stream || !stream_blocks || !mac_out || (enc != nullptr) != (enc_bytes != nullptr)) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(resolve_keys(c, k, MAC_MAX_STREAMS));
    std::vector<uint64_t> off(n_streams + 1, 0);
    for (uint64_t s = 0; s < n_streams; ++s) {
        if (stream_blocks[s] > MAC_MAX_STREAM_BLOCKS)
            return c->fail(FHEAES_ERR_INVALID, "stream_blocks[%llu] = %u: a stream chains at most %u blocks", (unsigned long long)s, stream_blocks[s], MAC_MAX_STREAM_BLOCKS);
        off[s + 1] = off[s] + stream_blocks[s];
    }
    const uint64_t total = off[n_streams];
    if (total && !clear) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (total > 0xFFFFFFFEull) return c->fail(FHEAES_ERR_INVALID, "a call chains fewer than 2^32 - 1 blocks");
    if (enc_bytes) for (uint64_t b = 0; b < total; ++b)
        if (enc_bytes[b] > 16) return c->fail(FHEAES_ERR_INVALID, "enc_bytes[%llu] = %u: a block has 16 bytes", (unsigned long long)b, (unsigned)enc_bytes[b]);
    if (n_streams == 0) return FHEAES_OK;
    const uint64_t sw = 16ull * 8 * c->big1, out_bytes = n_streams * sw * 8;
    if (k.overlaps(mac_out, out_bytes) || (enc && overlap(enc, total * sw * 8, mac_out, out_bytes)) || (init && overlap(init, out_bytes, mac_out, out_bytes)))
        return c->fail(FHEAES_ERR_INVALID, "mac_out overlaps an input");
    MacPlan pl;
    mac_plan(stream_blocks, n_streams, pl);
    MacChain ch;
    mac_chain(pl, stream_blocks, key_of_stream, n_streams, [&](uint32_t s, uint32_t i, uint8_t *clr, uint32_t *e, uint32_t *eb) {
        const uint64_t b = off[s] + i;
        memcpy(clr, clear + 16 * b, 16);
        if (enc) { *e = (uint32_t)b; *eb = enc_bytes[b]; }
    }, [&](uint32_t s) { return init ? s : MAC_NONE; }, ch);
    const size_t out0 = ch.slots.size();                                   // behind the chain: the results in the caller's order
    for (uint64_t s = 0; s < n_streams; ++s) ch.slots.push_back(mac_slot(pl.slot_of[s], MAC_NONE, 0, 16, nullptr));
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(k.stage(st));
    if (enc) TRY(st.in(enc, total * sw * 8, &enc));
    if (init) TRY(st.in(init, out_bytes, &init));
    TRY(st.out(mac_out, out_bytes, &mac_out));
    TRY(ensure(c, c->ws_tmp_b, out_bytes));
    uint64_t *state = (uint64_t *)c->ws_tmp_b.p;
    const MacSlot *recs = nullptr;
    TRY(cbc_mac_dev(c, k.sets(), k.nr, k.n_keys, ch, init, enc, state, &recs));
    TRY(launch_mac_link(c, mac_out, state, nullptr, recs + out0, n_streams, 2, "the CBC-MAC results in the caller's order"));
    return st.finish();
}

int fheaes_aes_cbc_mac_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams, const uint32_t *key_of_stream,
                             const uint32_t *stream_blocks, const uint8_t *clear, const uint64_t *enc, const uint8_t *enc_bytes, const uint64_t *init,
                             uint64_t *mac_out, int memspace)
{
    return aes_cbc_mac(c, {round_keys, key_bits, n_keys, key_of_stream, n_streams, false}, stream_blocks, clear, enc, enc_bytes, init, mac_out, memspace);
}

int fheaes_aes_cbc_mac_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                                    const uint32_t *key_of_stream, const uint32_t *stream_blocks, const uint8_t *clear, const uint64_t *enc, const uint8_t *enc_bytes,
                                    const uint64_t *init, uint64_t *mac_out, int memspace)
{
    return aes_cbc_mac(c, {packed_round_keys, key_bits, n_keys, key_of_stream, n_streams, true}, stream_blocks, clear, enc, enc_bytes, init, mac_out, memspace);
}

// K6 alone: one link of a chain on caller buffers (the kernel's test and measurement entry)
int fheaes_mac_link(fheaes_ctx *c, uint64_t *state, uint64_t n_slots, int first, const uint64_t *init, const uint64_t *enc, uint64_t n_enc, const uint32_t *src_block,
                    const uint8_t *enc_bytes, const uint8_t *clear, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (n_slots == 0) return FHEAES_OK;
    if (!state || !clear || (enc && (!src_block || !enc_bytes))) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_slots > MAC_MAX_STREAMS) return c->fail(FHEAES_ERR_INVALID, "n_slots must be at most %u (got %llu)", MAC_MAX_STREAMS, (unsigned long long)n_slots);
    if (init && !first) return c->fail(FHEAES_ERR_INVALID, "init belongs to the first link of a chain");
    const uint64_t sw = 16ull * 8 * c->big1, bytes = n_slots * sw * 8;
    bool any_b = false;
    std::vector<MacSlot> recs(n_slots);
    for (uint64_t s = 0; s < n_slots; ++s) {
        uint32_t b = MAC_NONE, eb = 0;
        if (enc) {
            if (enc_bytes[s] > 16) return c->fail(FHEAES_ERR_INVALID, "enc_bytes[%llu] = %u: a block has 16 bytes", (unsigned long long)s, (unsigned)enc_bytes[s]);
            if (src_block[s] != MAC_NONE && src_block[s] >= n_enc)
                return c->fail(FHEAES_ERR_INVALID, "src_block[%llu] = %u, but enc has %llu blocks", (unsigned long long)s, src_block[s], (unsigned long long)n_enc);
            b = src_block[s]; eb = b == MAC_NONE ? 0 : enc_bytes[s];
        }
        any_b = any_b || eb;
        recs[s] = mac_slot(first ? (init ? (uint32_t)s : MAC_NONE) : (uint32_t)s, b, eb, 16, clear + 16 * s);
    }
    if ((init && overlap(init, bytes, state, bytes)) || (enc && overlap(enc, n_enc * sw * 8, state, bytes))) return c->fail(FHEAES_ERR_INVALID, "state overlaps an input");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(st.inout(state, bytes, &state));
    if (init) TRY(st.in(init, bytes, &init));
    if (enc) TRY(st.in(enc, n_enc * sw * 8, &enc));
    const size_t rec_bytes = recs.size() * sizeof(MacSlot);
    TRY(upload_pinned(c, rec_bytes, rec_bytes, [&](uint8_t *pin) { memcpy(pin, recs.data(), rec_bytes); }));
    const uint32_t level = (!first || init ? 2u : 0u) + (any_b ? 2u : 0u) + 1u;
    TRY(launch_mac_link(c, state, first ? init : state, enc, (const MacSlot *)c->ws_misc.p, n_slots, level, "a CBC-MAC link (chaining value + block + the round key that follows)"));
    return st.finish();
}

static int aes_ccm_open(fheaes_ctx *c, RoundKeys k, const uint32_t *head_blocks, const uint64_t *head_hi_lo, const uint64_t *ctr0_hi_lo, const uint64_t *payload_bytes,
                        const uint8_t *ciphertext, const uint8_t *tags, const uint32_t *tag_bytes, uint64_t *plaintext_out, uint64_t *valid_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    const uint64_t n = k.n_of;
    const uint32_t *key_of_stream = k.key_of;
    if (!k.words || !key_of_stream || !head_blocks || !head_hi_lo || !ctr0_hi_lo || !payload_bytes || !tags || !tag_bytes || !valid_out)
        return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(resolve_keys(c, k, MAC_MAX_STREAMS));
    CcmCall cc;
    cc.n = n;
    cc.len.resize(n);
    std::vector<uint64_t> poff(n + 1, 0), hoff(n + 1, 0), boff(n + 1, 0);      // payload blocks, head blocks, payload bytes before stream s
    for (uint64_t s = 0; s < n; ++s) {
        const uint32_t t = tag_bytes[s], c0 = u128_byte(ctr0_hi_lo + 2 * s, 0);
        if (t < 4 || t > 16 || (t & 1)) return c->fail(FHEAES_ERR_INVALID, "tag_bytes[%llu] = %u: a CCM tag has 4, 6, .., 16 bytes", (unsigned long long)s, t);
        if (head_blocks[s] < 1 || head_blocks[s] > MAC_MAX_STREAM_BLOCKS)
            return c->fail(FHEAES_ERR_INVALID, "head_blocks[%llu] = %u: B0 and at most %u AAD blocks", (unsigned long long)s, head_blocks[s], MAC_MAX_STREAM_BLOCKS - 1);
        const uint32_t f0 = u128_byte(head_hi_lo + 2 * hoff[s], 0);
        if (c0 < 1 || c0 > 7) return c->fail(FHEAES_ERR_INVALID, "stream %llu: the flags byte of Ctr_0 is q - 1 = %u; a nonce has 7..13 bytes (q = 2..8)", (unsigned long long)s, c0);
        const uint32_t q = c0 + 1;
        if ((f0 & 7) != c0 || ((f0 >> 3) & 7) != (t - 2) / 2 || f0 >= 128 || ((f0 >> 6) & 1) != (head_blocks[s] > 1 ? 1u : 0u))
            return c->fail(FHEAES_ERR_INVALID, "stream %llu: the flags byte %#x of B0 does not say q = %u, t = %u, %s AAD", (unsigned long long)s, f0, q, t, head_blocks[s] > 1 ? "some" : "no");
        if (q < 8 && ((ctr0_hi_lo[2 * s + 1] & ((1ull << (8 * q)) - 1)) != 0 || payload_bytes[s] >> (8 * q)))
            return c->fail(FHEAES_ERR_INVALID, "stream %llu: the counter field of Ctr_0 must be zero and the payload shorter than 2^%u bytes", (unsigned long long)s, 8 * q);
        if (q == 8 && ctr0_hi_lo[2 * s + 1] != 0) return c->fail(FHEAES_ERR_INVALID, "stream %llu: the counter field of Ctr_0 must be zero", (unsigned long long)s);
        const uint64_t m = payload_bytes[s] / 16 + (payload_bytes[s] % 16 ? 1 : 0);
        if (payload_bytes[s] > 16ull * MAC_MAX_STREAM_BLOCKS || head_blocks[s] - 1 + m > MAC_MAX_STREAM_BLOCKS)
            return c->fail(FHEAES_ERR_INVALID, "stream %llu chains %llu blocks; at most %u", (unsigned long long)s, (unsigned long long)(head_blocks[s] - 1 + m), MAC_MAX_STREAM_BLOCKS);
        cc.len[s] = (uint32_t)(head_blocks[s] - 1 + m);
        poff[s + 1] = poff[s] + m; hoff[s + 1] = hoff[s] + head_blocks[s]; boff[s + 1] = boff[s] + payload_bytes[s];
    }
    if (n == 0) return FHEAES_OK;
    const uint64_t M = poff[n], n_pub = M + 2 * n;
    cc.payload_blocks = M;
    if (M && (!ciphertext || !plaintext_out)) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_pub > PUBLIC_MAX_BLOCKS) return c->fail(FHEAES_ERR_INVALID, "a call has at most %llu public blocks", (unsigned long long)PUBLIC_MAX_BLOCKS);
    const uint64_t sw = 16ull * 8 * c->big1, pt_bytes = M * sw * 8, valid_bytes = n * c->big1 * 8ull;
    if (k.overlaps(valid_out, valid_bytes) || (M && (k.overlaps(plaintext_out, pt_bytes) || overlap(plaintext_out, pt_bytes, valid_out, valid_bytes))))
        return c->fail(FHEAES_ERR_INVALID, "plaintext_out, valid_out and the round keys overlap");
    // the public batch: [Ctr_1.. of every stream | B0 | Ctr_0], data [C_1.. | 0 | 0]
    cc.pub_blocks.assign(2 * n_pub, 0); cc.pub_data.assign(2 * n_pub, 0); cc.pub_key.resize(n_pub);
    for (uint64_t s = 0; s < n; ++s) {
        for (uint64_t i = 0; i < poff[s + 1] - poff[s]; ++i) {
            const uint64_t b = poff[s] + i, have = std::min<uint64_t>(16, payload_bytes[s] - 16 * i);
            cc.pub_blocks[2 * b] = ctr0_hi_lo[2 * s]; cc.pub_blocks[2 * b + 1] = ctr0_hi_lo[2 * s + 1] + i + 1;
            for (uint64_t p = 0; p < have; ++p) cc.pub_data[2 * b + (p >> 3)] |= (uint64_t)ciphertext[boff[s] + 16 * i + p] << (8 * (7 - (p & 7)));
            cc.pub_key[b] = key_of_stream[s];
        }
        memcpy(&cc.pub_blocks[2 * (M + s)], head_hi_lo + 2 * hoff[s], 16);
        memcpy(&cc.pub_blocks[2 * (M + n + s)], ctr0_hi_lo + 2 * s, 16);
        cc.pub_key[M + s] = cc.pub_key[M + n + s] = key_of_stream[s];
    }
    mac_plan(cc.len.data(), n, cc.plan);
    mac_chain(cc.plan, cc.len.data(), key_of_stream, n, [&](uint32_t s, uint32_t i, uint8_t *clr, uint32_t *e, uint32_t *eb) {
        const uint32_t aad = head_blocks[s] - 1;
        if (i < aad) { for (int p = 0; p < 16; ++p) clr[p] = (uint8_t)u128_byte(head_hi_lo + 2 * (hoff[s] + 1 + i), p); return; }
        const uint64_t j = i - aad;
        *e = (uint32_t)(poff[s] + j);
        *eb = (uint32_t)std::min<uint64_t>(16, payload_bytes[s] - 16 * j);
    }, [&](uint32_t s) { return (uint32_t)(M + s); }, cc.chain);
    cc.tag0 = cc.chain.slots.size();
    for (uint64_t s = 0; s < n; ++s) cc.chain.slots.push_back(mac_slot(cc.plan.slot_of[s], (uint32_t)(M + n + s), 16, tag_bytes[s], tags + 16 * s, tag_bytes[s]));
    cc.pt0 = cc.chain.slots.size();
    for (uint64_t s = 0; s < n; ++s)
        for (uint64_t i = 0; i < poff[s + 1] - poff[s]; ++i)
            cc.chain.slots.push_back(mac_slot(MAC_NONE, (uint32_t)(poff[s] + i), (uint32_t)std::min<uint64_t>(16, payload_bytes[s] - 16 * i), 16, nullptr));
    PublicPlan pp;
    public_plan(public_forward(), cc.pub_blocks.data(), cc.pub_data.data(), cc.pub_key.data(), n_pub, k.nr, pp);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(k.stage(st));
    if (M) TRY(st.out(plaintext_out, pt_bytes, &plaintext_out));
    TRY(st.out(valid_out, valid_bytes, &valid_out));
    TRY(ccm_open_dev(c, k.sets(), k.nr, k.n_keys, cc, pp, plaintext_out, valid_out));
    return st.finish();
}

int fheaes_aes_ccm_open_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams, const uint32_t *key_of_stream,
                              const uint32_t *head_blocks, const uint64_t *head_hi_lo, const uint64_t *ctr0_hi_lo, const uint64_t *payload_bytes, const uint8_t *ciphertext,
                              const uint8_t *tags, const uint32_t *tag_bytes, uint64_t *plaintext_out, uint64_t *valid_out, int memspace)
{
    return aes_ccm_open(c, {round_keys, key_bits, n_keys, key_of_stream, n_streams, false}, head_blocks, head_hi_lo, ctr0_hi_lo, payload_bytes, ciphertext, tags, tag_bytes,
                        plaintext_out, valid_out, memspace);
}

int fheaes_aes_ccm_open_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                                     const uint32_t *key_of_stream, const uint32_t *head_blocks, const uint64_t *head_hi_lo, const uint64_t *ctr0_hi_lo,
                                     const uint64_t *payload_bytes, const uint8_t *ciphertext, const uint8_t *tags, const uint32_t *tag_bytes, uint64_t *plaintext_out,
                                     uint64_t *valid_out, int memspace)
{
    return aes_ccm_open(c, {packed_round_keys, key_bits, n_keys, key_of_stream, n_streams, true}, head_blocks, head_hi_lo, ctr0_hi_lo, payload_bytes, ciphertext, tags,
                        tag_bytes, plaintext_out, valid_out, memspace);
}

int fheaes_aes_mac_plan(const uint32_t *stream_blocks, const uint32_t *payload_blocks, uint64_t n_streams, uint64_t *steps, uint64_t *n_active_out, uint64_t n_active_cap,
                        uint64_t *public_blocks, uint64_t *chained_blocks)
{
    if ((n_streams && !stream_blocks) || !steps || !public_blocks || !chained_blocks || n_streams > MAC_MAX_STREAMS) return FHEAES_ERR_INVALID;
    uint64_t pub = payload_blocks ? 2 * n_streams : 0;
    for (uint64_t s = 0; s < n_streams; ++s) {
        if (stream_blocks[s] > MAC_MAX_STREAM_BLOCKS || (payload_blocks && payload_blocks[s] > stream_blocks[s])) return FHEAES_ERR_INVALID;
        if (payload_blocks) pub += payload_blocks[s];
    }
    MacPlan pl;
    mac_plan(stream_blocks, n_streams, pl);
    if (n_active_out) {
        if (n_active_cap < pl.n_active.size()) return FHEAES_ERR_INVALID;
        for (size_t i = 0; i < pl.n_active.size(); ++i) n_active_out[i] = pl.n_active[i];
    }
    *steps = pl.n_active.size(); *public_blocks = pub; *chained_blocks = pl.chained;
    return FHEAES_OK;
}

// ---- CMAC -------------------------------------------------------------------------------------
int fheaes_cmac_subkey_row(uint32_t which, uint32_t bit, uint32_t *sources_out, uint32_t *n_sources)
{
    if (which > 1 || bit > 127 || !sources_out || !n_sources) return FHEAES_ERR_INVALID;
    uint32_t s[3] = {0, 0, 0};
    *n_sources = cmac_subkey_row(which, bit, s);
    memcpy(sources_out, s, sizeof s);
    return FHEAES_OK;
}

int fheaes_cmac_double(fheaes_ctx *c, const uint64_t *l, uint64_t n_keys, uint64_t *out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (n_keys == 0) return FHEAES_OK;
    TRY(check_n_keys(c, n_keys));
    if (!l || !out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = n_keys * AES_BLOCK_BITS * c->big1 * 8, out_bytes = 2 * in_bytes;
    if (overlap(l, in_bytes, out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "l and out overlap (the gather is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(l, in_bytes, &l));
    TRY(s.out(out, out_bytes, &out));
    TRY(launch_cmac_double(c, l, n_keys, out));
    return s.finish();
}

static int aes_cmac_subkeys(fheaes_ctx *c, RoundKeys k, uint64_t *subkeys_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!k.words || !subkeys_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(resolve_keys(c, k));
    const uint64_t sw = 16ull * 8 * c->big1, out_bytes = 2 * k.n_keys * sw * 8;
    if (k.overlaps(subkeys_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "the round keys and subkeys_out overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(k.stage(st));
    TRY(st.out(subkeys_out, out_bytes, &subkeys_out));
    TRY(ensure(c, c->ws_tmp_a, k.n_keys * sw * 8));
    TRY(ensure(c, c->ws_tmp_b, 2 * k.n_keys * sw * 8));
    TRY(ensure(c, c->ws_tmp_c, k.n_keys * sw * 8));
    std::vector<uint32_t> all(k.n_keys);
    for (uint64_t j = 0; j < k.n_keys; ++j) all[j] = (uint32_t)j;
    TRY(cmac_subkeys_dev(c, k.sets(), k.nr, all.data(), k.n_keys, subkeys_out));
    return st.finish();
}

int fheaes_aes_cmac_subkeys_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *subkeys_out, int memspace)
{
    return aes_cmac_subkeys(c, {round_keys, key_bits, n_keys, nullptr, 0, false}, subkeys_out, memspace);
}

int fheaes_aes_cmac_subkeys_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *subkeys_out, int memspace)
{
    return aes_cmac_subkeys(c, {packed_round_keys, key_bits, n_keys, nullptr, 0, true}, subkeys_out, memspace);
}

// k.key_of: the key of every stream, k.n_of of them
static int aes_cmac(fheaes_ctx *c, RoundKeys k, const uint64_t *subkeys, const uint64_t *message_bytes, const uint8_t *data, const uint8_t *tags, const uint32_t *tag_bytes,
                    uint64_t *mac_out, uint64_t *valid_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    const uint64_t n = k.n_of;
    const uint32_t *key_of_stream = k.key_of;
    if (!k.words || !key_of_stream || !message_bytes || (tags != nullptr) != (tag_bytes != nullptr) || (tags ? !valid_out : !mac_out))
        return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (!tags && valid_out) return c->fail(FHEAES_ERR_INVALID, "valid_out without tags: there is nothing to compare");
    TRY(resolve_keys(c, k, MAC_MAX_STREAMS));
    CmacCall cc;
    cc.n = n;
    cc.len.resize(n);
    std::vector<uint64_t> boff(n + 1, 0);                                   // message bytes before stream s
    uint64_t total = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (message_bytes[s] > 16ull * MAC_MAX_STREAM_BLOCKS)
            return c->fail(FHEAES_ERR_INVALID, "message_bytes[%llu] = %llu: a stream chains at most %u blocks", (unsigned long long)s, (unsigned long long)message_bytes[s],
                           MAC_MAX_STREAM_BLOCKS);
        if (tags && (tag_bytes[s] < 4 || tag_bytes[s] > 16))
            return c->fail(FHEAES_ERR_INVALID, "tag_bytes[%llu] = %u: a CMAC tag is compared on 4..16 bytes", (unsigned long long)s, tag_bytes[s]);
        cc.len[s] = (uint32_t)cmac_blocks(message_bytes[s]);
        boff[s + 1] = boff[s] + message_bytes[s];
        total += cc.len[s];
    }
    if (boff[n] && !data) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (total > 0xFFFFFFFEull) return c->fail(FHEAES_ERR_INVALID, "a call chains fewer than 2^32 - 1 blocks");
    if (n == 0) return FHEAES_OK;
    const uint64_t sw = 16ull * 8 * c->big1, mac_bytes = n * sw * 8, valid_bytes = n * c->big1 * 8ull, sub_bytes = 2 * k.n_keys * sw * 8;
    if ((mac_out && (k.overlaps(mac_out, mac_bytes) || (subkeys && overlap(subkeys, sub_bytes, mac_out, mac_bytes)))) ||
        (valid_out && (k.overlaps(valid_out, valid_bytes) || (subkeys && overlap(subkeys, sub_bytes, valid_out, valid_bytes)))) ||
        (mac_out && valid_out && overlap(mac_out, mac_bytes, valid_out, valid_bytes)))
        return c->fail(FHEAES_ERR_INVALID, "mac_out, valid_out, the subkeys and the round keys overlap");
    // where a stream's subkeys are: the caller's array has every key's, a derived one those of the keys in use
    std::vector<uint32_t> at(k.n_keys, MAC_NONE);
    for (uint64_t s = 0; s < n; ++s) at[key_of_stream[s]] = 0;
    for (uint64_t j = 0; j < k.n_keys; ++j)
        if (subkeys) at[j] = (uint32_t)j;
        else if (at[j] != MAC_NONE) { at[j] = (uint32_t)cc.used.size(); cc.used.push_back((uint32_t)j); }
    mac_plan(cc.len.data(), n, cc.plan);
    mac_chain(cc.plan, cc.len.data(), key_of_stream, n, [&](uint32_t s, uint32_t i, uint8_t *clr, uint32_t *e, uint32_t *eb) {
        const uint64_t have = std::min<uint64_t>(16, message_bytes[s] - std::min<uint64_t>(message_bytes[s], 16ull * i));
        if (have) memcpy(clr, data + boff[s] + 16ull * i, have);
        if (i + 1 < cc.len[s]) return;
        if (have < 16) clr[have] = 0x80;                                     // the padded last block takes K2, the whole one K1
        *e = 2 * at[key_of_stream[s]] + (have < 16 ? 1u : 0u);
        *eb = 16;
    }, [&](uint32_t) { return MAC_NONE; }, cc.chain);
    cc.mac0 = cc.chain.slots.size();
    if (mac_out) for (uint64_t s = 0; s < n; ++s) cc.chain.slots.push_back(mac_slot(cc.plan.slot_of[s], MAC_NONE, 0, 16, nullptr));
    cc.tag0 = cc.chain.slots.size();
    if (tags) for (uint64_t s = 0; s < n; ++s) cc.chain.slots.push_back(mac_slot(cc.plan.slot_of[s], MAC_NONE, 0, tag_bytes[s], tags + 16 * s, tag_bytes[s]));
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(k.stage(st));
    if (subkeys) TRY(st.in(subkeys, sub_bytes, &subkeys));
    if (mac_out) TRY(st.out(mac_out, mac_bytes, &mac_out));
    if (valid_out) TRY(st.out(valid_out, valid_bytes, &valid_out));
    TRY(cmac_dev(c, k.sets(), k.nr, k.n_keys, cc, subkeys, mac_out, valid_out));
    return st.finish();
}

int fheaes_aes_cmac_keyed(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint64_t *subkeys, uint64_t n_streams,
                          const uint32_t *key_of_stream, const uint64_t *message_bytes, const uint8_t *data, const uint8_t *tags, const uint32_t *tag_bytes,
                          uint64_t *mac_out, uint64_t *valid_out, int memspace)
{
    return aes_cmac(c, {round_keys, key_bits, n_keys, key_of_stream, n_streams, false}, subkeys, message_bytes, data, tags, tag_bytes, mac_out, valid_out, memspace);
}

int fheaes_aes_cmac_keyed_packed(fheaes_ctx *c, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, const uint64_t *subkeys, uint64_t n_streams,
                                 const uint32_t *key_of_stream, const uint64_t *message_bytes, const uint8_t *data, const uint8_t *tags, const uint32_t *tag_bytes,
                                 uint64_t *mac_out, uint64_t *valid_out, int memspace)
{
    return aes_cmac(c, {packed_round_keys, key_bits, n_keys, key_of_stream, n_streams, true}, subkeys, message_bytes, data, tags, tag_bytes, mac_out, valid_out, memspace);
}

int fheaes_aes_cmac_plan(const uint64_t *message_bytes, uint64_t n_streams, uint64_t *steps, uint64_t *chained_blocks, uint64_t *padded_streams)
{
    if ((n_streams && !message_bytes) || !steps || !chained_blocks || !padded_streams || n_streams > MAC_MAX_STREAMS) return FHEAES_ERR_INVALID;
    std::vector<uint32_t> len(n_streams);
    uint64_t padded = 0;
    for (uint64_t s = 0; s < n_streams; ++s) {
        if (message_bytes[s] > 16ull * MAC_MAX_STREAM_BLOCKS) return FHEAES_ERR_INVALID;
        len[s] = (uint32_t)cmac_blocks(message_bytes[s]);
        padded += message_bytes[s] == 0 || message_bytes[s] % 16 != 0;
    }
    MacPlan pl;
    mac_plan(len.data(), n_streams, pl);
    *steps = pl.n_active.size(); *chained_blocks = pl.chained; *padded_streams = padded;
    return FHEAES_OK;
}

// ---- AES key unwrap ---------------------------------------------------------------------------
static_assert(KW_MIN_SEMIBLOCKS == FHEAES_KW_MIN_SEMIBLOCKS && KW_MAX_SEMIBLOCKS == FHEAES_KW_MAX_SEMIBLOCKS, "fheaes.h's bounds on a wrapped key are the kernel's");

static int check_kw_shape(fheaes_ctx *c, uint32_t semiblocks, uint64_t n_keys)
{
    if (semiblocks < KW_MIN_SEMIBLOCKS || semiblocks > KW_MAX_SEMIBLOCKS)
        return c->fail(FHEAES_ERR_INVALID, "semiblocks must be in %u..%u (got %u)", KW_MIN_SEMIBLOCKS, KW_MAX_SEMIBLOCKS, semiblocks);
    if (n_keys > FHEAES_KW_MAX_KEYS) return c->fail(FHEAES_ERR_INVALID, "a call unwraps at most %u keys (got %llu)", (unsigned)FHEAES_KW_MAX_KEYS, (unsigned long long)n_keys);
    return FHEAES_OK;
}

// K6 alone: one link of the unwrap on caller buffers (the kernel's test and measurement entry)
int fheaes_kw_link(fheaes_ctx *c, uint64_t *state, uint64_t *regs, uint64_t n_keys, uint32_t semiblocks, uint32_t step, const uint8_t *wrapped, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_kw_shape(c, semiblocks, n_keys));
    if (step > 6 * semiblocks) return c->fail(FHEAES_ERR_INVALID, "step must be in 0..%u for %u semiblocks (got %u)", 6 * semiblocks, semiblocks, step);
    if (!state || !regs || (step == 0 && !wrapped)) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_keys == 0) return FHEAES_OK;
    const uint64_t bw = 8ull * c->big1, state_bytes = n_keys * 16 * bw * 8, regs_bytes = n_keys * 8 * semiblocks * bw * 8;
    if (overlap(state, state_bytes, regs, regs_bytes)) return c->fail(FHEAES_ERR_INVALID, "state and regs overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    if (step == 0) {                                                         // the load writes every word of both
        TRY(st.out(state, state_bytes, &state));
        TRY(st.out(regs, regs_bytes, &regs));
        const size_t bytes = n_keys * 8 * (semiblocks + 1);
        TRY(upload_pinned(c, bytes, bytes, [&](uint8_t *pin) { memcpy(pin, wrapped, bytes); }));
    } else {
        TRY(st.inout(state, state_bytes, &state));
        TRY(st.inout(regs, regs_bytes, &regs));
    }
    TRY(launch_kw_link(c, state, regs, step == 0 ? (const uint8_t *)c->ws_misc.p : nullptr, n_keys, semiblocks, step));
    return st.finish();
}

// k: the KEKs' decryption round keys; k.key_of: the KEK of every wrapped key (null: the one KEK), k.n_of of them
static int aes_kw_unwrap(fheaes_ctx *c, RoundKeys k, uint32_t semiblocks, const uint8_t *wrapped, uint64_t *keys_out, uint64_t *valid_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    const uint64_t n_keys = k.n_of;
    if (!k.words || !wrapped || !keys_out || !valid_out || (!k.key_of && k.n_keys != 1)) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(check_kw_shape(c, semiblocks, n_keys));
    TRY(resolve_keys(c, k));
    if (n_keys == 0) return FHEAES_OK;
    const uint64_t bw = 8ull * c->big1, out_bytes = n_keys * 8 * semiblocks * bw * 8, valid_bytes = n_keys * c->big1 * 8ull;
    if (k.overlaps(keys_out, out_bytes) || k.overlaps(valid_out, valid_bytes) || overlap(keys_out, out_bytes, valid_out, valid_bytes))
        return c->fail(FHEAES_ERR_INVALID, "keys_out, valid_out and the round keys overlap");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged st(c, memspace);
    TRY(k.stage(st));
    TRY(st.out(keys_out, out_bytes, &keys_out));
    TRY(st.out(valid_out, valid_bytes, &valid_out));
    // one upload: the KEK of every key (more than one KEK only), then the wrapped bytes
    const bool table = k.n_keys > 1;
    const size_t tab_bytes = table ? (n_keys * sizeof(uint32_t) + 31) / 32 * 32 : 0, data_bytes = n_keys * 8 * (semiblocks + 1);
    TRY(upload_pinned(c, tab_bytes + data_bytes, tab_bytes + data_bytes, [&](uint8_t *pin) {
        if (table) memcpy(pin, k.key_of, n_keys * sizeof(uint32_t));
        memcpy(pin + tab_bytes, wrapped, data_bytes);
    }));
    const uint8_t *misc = (const uint8_t *)c->ws_misc.p;
    TRY(kw_unwrap_dev(c, k.sets(table ? (const uint32_t *)misc : nullptr), k.nr, misc + tab_bytes, semiblocks, n_keys, keys_out, valid_out));
    return st.finish();
}

int fheaes_aes_kw_unwrap_keyed(fheaes_ctx *c, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keks, uint64_t n_keys, const uint32_t *kek_of_key,
                               uint32_t semiblocks, const uint8_t *wrapped, uint64_t *keys_out, uint64_t *valid_out, int memspace)
{
    return aes_kw_unwrap(c, {dec_round_keys, key_bits, n_keks, kek_of_key, n_keys, false}, semiblocks, wrapped, keys_out, valid_out, memspace);
}

int fheaes_aes_kw_unwrap_keyed_packed(fheaes_ctx *c, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keks, uint64_t n_keys,
                                      const uint32_t *kek_of_key, uint32_t semiblocks, const uint8_t *wrapped, uint64_t *keys_out, uint64_t *valid_out, int memspace)
{
    return aes_kw_unwrap(c, {packed_dec_round_keys, key_bits, n_keks, kek_of_key, n_keys, true}, semiblocks, wrapped, keys_out, valid_out, memspace);
}

int fheaes_aes_kw_plan(uint32_t key_bits, uint32_t semiblocks, uint64_t n_keys, uint64_t *steps, uint64_t *cipher_blocks, uint64_t *byte_wopbs)
{
    const uint64_t nr = (uint64_t)aes_rounds(key_bits), n = semiblocks;
    if (!nr || n < KW_MIN_SEMIBLOCKS || n > KW_MAX_SEMIBLOCKS || n_keys > FHEAES_KW_MAX_KEYS || !steps || !cipher_blocks || !byte_wopbs) return FHEAES_ERR_INVALID;
    *steps = 6 * n;
    *cipher_blocks = 6 * n * n_keys;
    *byte_wopbs = 16 * nr * 6 * n * n_keys + 8 * n * n_keys + 16 * n_keys;
    return FHEAES_OK;
}

// ---- the gate: ciphertexts times an encrypted bit ------------------------------------------------
static_assert(GATE_LWE == FHEAES_GATE_LWE && GATE_GLWE == FHEAES_GATE_GLWE, "fheaes.h's input forms are the kernel's");

// ggsw_fourier: caller-made GGSWs (fheaes_gate_ggsw), else gates_lwe: the bits, circuit-bootstrapped here in wopbs_dev's workspaces and by its
// chunk rule (cbs_bits: K1, K2 at level 1, K3, K4), each chunk's GGSWs gating that chunk's runs before the next overwrites them
static int gate_call(fheaes_ctx *c, bool boot, const double *ggsw_fourier, const uint64_t *gates_lwe, uint64_t n_gates, const uint64_t *bits_of_gate, const uint64_t *in,
                     uint64_t m, int form, uint64_t *out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (boot) TRY(check_keys(c));
    if (form != GATE_LWE && form != GATE_GLWE) return c->fail(FHEAES_ERR_INVALID, "form must be 0 (LWE) or 1 (GLWE), got %d", form);
    if (n_gates && !bits_of_gate) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    if (n_gates > 0xFFFFFFFFull) return c->fail(FHEAES_ERR_INVALID, "a call takes at most 2^32 - 1 gates (got %llu)", (unsigned long long)n_gates);
    const uint32_t R = gate_r(c->k1);
    const uint64_t chunk = boot ? MAX_CHUNK_BITS : 0;
    std::vector<GateWg> wgs;
    std::vector<uint64_t> chunk_end;
    uint64_t n_wgs = 0, total = 0;
    for (uint64_t g = 0; g < n_gates; ++g) {
        if (bits_of_gate[g] > m - total) { total = ~0ull; break; }
        total += bits_of_gate[g];
    }
    if (total != m) return c->fail(FHEAES_ERR_INVALID, "the runs of bits_of_gate do not add up to m = %llu", (unsigned long long)m);
    if (m == 0) return FHEAES_OK;
    if (!in || !out || (boot ? !gates_lwe : !ggsw_fourier)) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t ggsw_words = (uint64_t)c->k1 * c->k1 * FHE_N, inst_words = form == GATE_GLWE ? (uint64_t)c->k1 * FHE_N : c->big1;
    const uint64_t bytes = m * inst_words * 8, gate_bytes = n_gates * (boot ? c->big1 : ggsw_words) * 8;
    const void *gates = boot ? (const void *)gates_lwe : (const void *)ggsw_fourier;
    if (out != in && overlap(in, bytes, out, bytes)) return c->fail(FHEAES_ERR_INVALID, "in and out overlap without being the same buffer");
    if (overlap(gates, gate_bytes, out, bytes)) return c->fail(FHEAES_ERR_INVALID, "out overlaps the gates");
    gate_table(bits_of_gate, n_gates, R, chunk, &wgs, &chunk_end, &n_wgs);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    if (boot) TRY(s.in(gates_lwe, gate_bytes, &gates_lwe));
    else TRY(s.in(ggsw_fourier, gate_bytes, &ggsw_fourier));
    if (out == in) { TRY(s.inout(out, bytes, &out)); in = out; }
    else { TRY(s.in(in, bytes, &in)); TRY(s.out(out, bytes, &out)); }
    const size_t tab_bytes = wgs.size() * sizeof(GateWg);
    TRY(upload_pinned(c, tab_bytes, tab_bytes, [&](uint8_t *pin) { memcpy(pin, wgs.data(), tab_bytes); }));
    const GateWg *tab = (const GateWg *)c->ws_misc.p;
    if (!boot) {
        TRY(launch_gate(c, (const double2 *)ggsw_fourier, tab, n_wgs, m, form, in, out));
        return s.finish();
    }
    TRY(ensure_wopbs_ws(c, std::min<uint64_t>(n_gates, chunk)));
    uint64_t wg0 = 0;
    for (uint64_t g0 = 0, ci = 0; g0 < n_gates; g0 += chunk, ++ci) {
        const uint64_t gc = std::min<uint64_t>(chunk, n_gates - g0);
        TRY(cbs_bits(c, gates_lwe + g0 * c->big1, gc));
        uint64_t units = 0;
        for (uint64_t g = g0; g < g0 + gc; ++g) units += bits_of_gate[g];
        TRY(launch_gate(c, (const double2 *)c->ws_ggswf.p, tab + wg0, chunk_end[ci] - wg0, units, form, in, out));
        wg0 = chunk_end[ci];
    }
    return s.finish();
}

int fheaes_gate_ggsw(fheaes_ctx *c, const double *ggsw_fourier, uint64_t n_gates, const uint64_t *bits_of_gate, const uint64_t *in, uint64_t m, int form,
                     uint64_t *out, int memspace)
{
    return gate_call(c, false, ggsw_fourier, nullptr, n_gates, bits_of_gate, in, m, form, out, memspace);
}

int fheaes_gate_bits(fheaes_ctx *c, const uint64_t *gates_lwe, uint64_t n_gates, const uint64_t *bits_of_gate, const uint64_t *lwe_in, uint64_t m,
                     uint64_t *lwe_out, int memspace)
{
    return gate_call(c, true, nullptr, gates_lwe, n_gates, bits_of_gate, lwe_in, m, GATE_LWE, lwe_out, memspace);
}

int fheaes_gate_packed(fheaes_ctx *c, const uint64_t *gates_lwe, uint64_t n_gates, const uint64_t *glwes_of_gate, const uint64_t *glwe_in, uint64_t n_glwe,
                       uint64_t *glwe_out, int memspace)
{
    return gate_call(c, true, nullptr, gates_lwe, n_gates, glwes_of_gate, glwe_in, n_glwe, GATE_GLWE, glwe_out, memspace);
}

int fheaes_gate_plan(const uint64_t *bits_of_gate, uint64_t n_gates, uint32_t k, uint64_t *workgroups, uint32_t *instances_per_workgroup)
{
    if ((n_gates && !bits_of_gate) || (k != 4 && k != 1) || !workgroups || !instances_per_workgroup) return FHEAES_ERR_INVALID;
    *instances_per_workgroup = gate_r(k + 1);
    gate_table(bits_of_gate, n_gates, *instances_per_workgroup, 0, nullptr, nullptr, workgroups);
    return FHEAES_OK;
}

// ---- packing ----------------------------------------------------------------------------------
size_t fheaes_packed_words(const fheaes_ctx *c, uint64_t m)
{
    if (!c) return 0;
    return (size_t)((m + FHE_N - 1) / FHE_N) * c->k1 * FHE_N;
}

int fheaes_pack_bits(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t m, uint64_t *glwe_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (m == 0) return FHEAES_OK;
    if (!lwe_in || !glwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = m * c->big1 * 8, out_bytes = (uint64_t)fheaes_packed_words(c, m) * 8;
    if (overlap(lwe_in, in_bytes, glwe_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "lwe_in and glwe_out overlap (packing is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(lwe_in, in_bytes, &lwe_in));
    TRY(s.out(glwe_out, out_bytes, &glwe_out));
    TRY(pack_dev(c, lwe_in, m, glwe_out));
    return s.finish();
}

int fheaes_unpack_bits(fheaes_ctx *c, const uint64_t *glwe_in, uint64_t m, uint64_t *lwe_out, int memspace)
{
    if (!c) return FHEAES_ERR_INVALID;
    CtxLock lock__(c);
    if (m == 0) return FHEAES_OK;
    if (!glwe_in || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = (uint64_t)fheaes_packed_words(c, m) * 8, out_bytes = m * c->big1 * 8;
    if (overlap(glwe_in, in_bytes, lwe_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "glwe_in and lwe_out overlap (unpacking is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(glwe_in, in_bytes, &glwe_in));
    TRY(s.out(lwe_out, out_bytes, &lwe_out));
    TRY(unpack_dev(c, glwe_in, m, lwe_out));
    return s.finish();
}

// ---- packed round keys --------------------------------------------------------------------------
uint32_t fheaes_round_keys_packed_glwes(uint32_t key_bits) { return packed_key_glwes(key_bits); }

int fheaes_pack_round_keys(fheaes_ctx *c, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *packed_out, int memspace)
{
    CtxLock lock__(c);
    TRY(check_keys(c));
    if (!round_keys || !packed_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(check_key_bits(c, key_bits));
    TRY(check_n_keys(c, n_keys));
    const uint64_t m = (uint64_t)(aes_rounds(key_bits) + 1) * AES_BLOCK_BITS, glwes = packed_key_glwes(key_bits);
    const uint64_t in_bytes = n_keys * m * c->big1 * 8, out_bytes = n_keys * glwes * c->k1 * FHE_N * 8;
    if (overlap(round_keys, in_bytes, packed_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "round_keys and packed_out overlap (packing is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(round_keys, in_bytes, &round_keys));
    TRY(s.out(packed_out, out_bytes, &packed_out));
    TRY(pack_keys_dev(c, round_keys, m, n_keys, packed_out));
    return s.finish();
}

int fheaes_unpack_round_keys(fheaes_ctx *c, const uint64_t *packed, uint32_t key_bits, uint64_t first_key, uint64_t n_keys, uint64_t *round_keys_out,
                             int memspace)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    if (!packed || !round_keys_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    TRY(check_key_bits(c, key_bits));
    TRY(check_n_keys(c, n_keys));
    if (first_key > FHEAES_MAX_KEYS - n_keys)
        return c->fail(FHEAES_ERR_INVALID, "keys %llu .. %llu lie beyond the %u a store can hold", (unsigned long long)first_key,
                       (unsigned long long)(first_key + n_keys), (unsigned)FHEAES_MAX_KEYS);
    const uint64_t m = (uint64_t)(aes_rounds(key_bits) + 1) * AES_BLOCK_BITS, key_words = (uint64_t)packed_key_glwes(key_bits) * c->k1 * FHE_N;
    packed += first_key * key_words;                                                     // only the keys asked for are read (and staged)
    const uint64_t in_bytes = n_keys * key_words * 8, out_bytes = n_keys * m * c->big1 * 8;
    if (overlap(packed, in_bytes, round_keys_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "packed and round_keys_out overlap (unpacking is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(packed, in_bytes, &packed));
    TRY(s.out(round_keys_out, out_bytes, &round_keys_out));
    TRY(unpack_keys_dev(c, packed, m, n_keys, round_keys_out));
    return s.finish();
}

// ---- wire formats -----------------------------------------------------------------------------
static bool mod_width_ok(uint32_t width) { return (width >= 8 && width <= 32) || width == 64; }

static int check_mod_width(fheaes_ctx *c, uint32_t width)
{
    if (!mod_width_ok(width)) return c->fail(FHEAES_ERR_INVALID, "width must be in 8..32, or 64 for the words as they are (got %u)", width);
    return FHEAES_OK;
}

int fheaes_expand_lwe_seeded(fheaes_ctx *c, const uint32_t *mask_key, uint64_t first_index, const uint64_t *bodies, uint64_t m, uint64_t *lwe_out,
                             int memspace)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    if (m == 0) return FHEAES_OK;
    if (!mask_key || !bodies || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = m * 8, out_bytes = m * c->big1 * 8;
    if (overlap(bodies, in_bytes, lwe_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "bodies and lwe_out overlap (expansion is not in place)");
    MaskKey mk;
    memcpy(mk.k, mask_key, 32);
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(bodies, in_bytes, &bodies));
    TRY(s.out(lwe_out, out_bytes, &lwe_out));
    TRY(expand_lwe_dev(c, mk, first_index, bodies, m, lwe_out));
    return s.finish();
}

size_t fheaes_packed_words_mod(const fheaes_ctx *c, uint64_t m, uint32_t width)
{
    if (!c || !mod_width_ok(width)) return 0;
    return (size_t)((m + FHE_N - 1) / FHE_N) * c->k1 * (FHE_N / 64) * width;
}

int fheaes_packed_mod_switch(fheaes_ctx *c, const uint64_t *glwe_in, uint64_t n_glwe, uint32_t width, uint64_t *out, int memspace)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    TRY(check_mod_width(c, width));
    if (n_glwe == 0) return FHEAES_OK;
    if (!glwe_in || !out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = n_glwe * c->k1 * FHE_N * 8, out_bytes = in_bytes / 64 * width;
    if (overlap(glwe_in, in_bytes, out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "glwe_in and out overlap (the switch is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(glwe_in, in_bytes, &glwe_in));
    TRY(s.out(out, out_bytes, &out));
    if (width == 64) HIP_TRY(c, hipMemcpyAsync(out, glwe_in, in_bytes, hipMemcpyDeviceToDevice, c->stream));
    else TRY(mod_switch_dev(c, glwe_in, n_glwe, width, out));
    return s.finish();
}

int fheaes_pack_bits_mod(fheaes_ctx *c, const uint64_t *lwe_in, uint64_t m, uint32_t width, uint64_t *out, int memspace)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    TRY(check_mod_width(c, width));
    TRY(check_keys(c));
    if (m == 0) return FHEAES_OK;
    if (!lwe_in || !out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = m * c->big1 * 8, out_bytes = (uint64_t)fheaes_packed_words_mod(c, m, width) * 8;
    if (overlap(lwe_in, in_bytes, out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "lwe_in and out overlap (packing is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(lwe_in, in_bytes, &lwe_in));
    TRY(s.out(out, out_bytes, &out));
    TRY(pack_dev(c, lwe_in, m, out, width));
    return s.finish();
}

int fheaes_unpack_bits_mod(fheaes_ctx *c, const uint64_t *in, uint64_t m, uint32_t width, uint64_t *lwe_out, int memspace)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    TRY(check_mod_width(c, width));
    if (m == 0) return FHEAES_OK;
    if (!in || !lwe_out) return c->fail(FHEAES_ERR_INVALID, "null pointer");
    const uint64_t in_bytes = (uint64_t)fheaes_packed_words_mod(c, m, width) * 8, out_bytes = m * c->big1 * 8;
    if (overlap(in, in_bytes, lwe_out, out_bytes)) return c->fail(FHEAES_ERR_INVALID, "in and lwe_out overlap (unpacking is not in place)");
    HIP_TRY(c, hipSetDevice(c->device));
    Staged s(c, memspace);
    TRY(s.in(in, in_bytes, &in));
    TRY(s.out(lwe_out, out_bytes, &lwe_out));
    if (width == 64) TRY(unpack_dev(c, in, m, lwe_out));
    else TRY(unpack_mod_dev(c, in, m, width, lwe_out));
    return s.finish();
}

// ---- measurement ------------------------------------------------------------------------------
int fheaes_profile_enable(fheaes_ctx *c, int on)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    if (!on && c->prof) TRY(prof_flush(c));
    c->prof = on != 0;
    return FHEAES_OK;
}

int fheaes_profile_reset(fheaes_ctx *c)
{
    CtxLock lock__(c);
    if (!c) return FHEAES_ERR_INVALID;
    TRY(prof_flush(c));
    for (int s = 0; s < FHEAES_STAGE_COUNT; ++s) { c->stage_ms[s] = 0; c->stage_launches[s] = 0; c->stage_units[s] = 0; }
    return FHEAES_OK;
}

int fheaes_profile_read(fheaes_ctx *c, int stage, double *total_ms, uint64_t *launches, uint64_t *units)
{
    CtxLock lock__(c);
    if (!c || stage < 0 || stage >= FHEAES_STAGE_COUNT) return FHEAES_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(prof_flush(c));
    if (total_ms) *total_ms = c->stage_ms[stage];
    if (launches) *launches = c->stage_launches[stage];
    if (units) *units = c->stage_units[stage];
    return FHEAES_OK;
}

}  // extern "C"
