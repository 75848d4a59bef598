// engine_ctx.h -- the context (fheaes_ctx) and what every entry point does around its work: error texts, the lock, workspace
// buffers, per-stage profiling, staging of host-memory arguments.
#pragma once

namespace {

std::string g_create_error;
// fheaes_last_error(): a context may be shared between threads (every call takes its lock), so the message a caller reads must
// not be one that another thread is overwriting.  fail() keeps a per-thread copy; the pointer fheaes_last_error returns is valid
// until the same thread's next call into the library.
thread_local std::string tl_error;
thread_local uint64_t tl_error_ctx_id = 0;           // id of the context tl_error belongs to (ids are never reused: a new context at a
                                                     // destroyed one's address does not inherit its message)
std::atomic<uint64_t> g_next_ctx_id{1};

}  // namespace

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// a device buffer that a context owns: grown by ensure(), freed with the context (fheaes_destroy sets the device and drains the stream first)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// The audit of one stage (fheaes_audit_stage_set; fheaes_audit_set is the blind rotation's; kern_audit.h): rows > 0 = every launch of the
// stage of at least min_rows rows is computed again on min(rows, m) sampled rows by the stage's second form; launch = audited launches of
// THIS stage since its set (the rows one stage's audit samples do not depend on whether another stage is audited).  out: the second form's
// results, one row per sample; state: the counters and records (AUDIT_STATE_WORDS).  The buffers are allocated by the set call and never
// by a launch; like the parking owner words they are state, not scratch (not among FHEAES_WS_BUFFERS).  hook*: the test hook
// (fheaes_audit_stage_debug), one shot: the next audited launch XORs hook_mask into word hook_word of row hook_row of its output.
// What differs between the stages (audit_shape in engine.hip, the launchers in engine_launch.h):
//   K2 (blind rotation)      second form: the latency form on the sampled rows' small LWEs, gathered into `in` (n + 1 words a row);
//                            a row is the kN + 1 words of an output ciphertext
//   K1 (LWE key switch)      second form: the plain form (keyswitch_plain_kernel), which reads the sampled rows where they lie: no `in`;
//                            a row is n + 1 words
//   K3 (packing key switch)  the plain form, no `in`; a row is the (k+1)N words of each key block of the launch: (k+1)^2 N at the widest
struct StageAudit {
    uint32_t rows = 0;
    uint64_t min_rows = 0, seed = 0, launch = 0;
    DevBuf in, out, state;
    bool hook = false;
    uint64_t hook_row = 0, hook_mask = 0;
    uint32_t hook_word = 0;
    bool wants(uint64_t m) const { return rows && m >= min_rows; }      // a launch of m rows is audited
};
static_assert(FHEAES_STAGE_KEYSWITCH == 0 && FHEAES_STAGE_BLIND_ROTATE == 1 && FHEAES_STAGE_PFPKS == 2, "fheaes_ctx::audit is indexed by these three stages");

struct fheaes_ctx {
    fheaes_params p{};
    const uint64_t id = g_next_ctx_id.fetch_add(1);
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    // The reference shares one `&Server` between rayon worker threads (main.rs:55-61).  A context is one GPU stream and one
    // workspace, so concurrent calls are made SAFE by serialising them here (batched calls are the way to use the GPU; this
    // only guarantees that a drop-in that keeps the per-block thread pool does not corrupt the workspace).
    std::recursive_mutex mu;
    // shapes
    uint32_t n = 0, k = 0, k1 = 0, big = 0, big1 = 0;
    uint32_t cu_count = 256;             // compute units of the device (MI355X: 256)
    // how the last fheaes_clone_keys INTO this context moved the key images (fheaes_clone_info)
    int clone_path = FHEAES_CLONE_NONE;
    uint64_t clone_bytes = 0;
    double clone_seconds = 0.0;
    // noise guard (the reference runs tfhe-rs with `noise-asserts` and MaxNoiseLevel::new(5), Cargo.toml:7, client.rs:92): the linear
    // layers count how many nominal-noise ciphertexts (fresh WoPBS outputs, round keys, client encryptions) they sum into one
    uint32_t noise_level_seen = 0;
    int k2_home = -1;                    // blind rotation: 1 = the LDS-home form runs two workgroups per CU here (queried once), 0 = parked form
    int k2_pair_ok = -1;                 // 1 = the paired kernel (159,504 B of LDS per workgroup) can be resident on a CU here (queried once)
    bool k2_deny_pair = false, k2_deny_home = false;     // test hook (fheaes_k2_set_forms): a form the queries allow is not used; never grants one
    int k2_park_claim = 1;               // paired kernel's parking slots: 1 = claimed from a shared pool (kern_blindrot_pair.h), 0 = one private slot per workgroup
    // test hook (fheaes_k2_park_debug): claimed-mode paired launches start from the owner words in ws_park_pattern instead of zeros, and
    // record {slot, XCC} per workgroup into ws_park_record; k2_park_record_n = grid of the last recorded launch since the hook was set
    bool k2_park_pattern = false, k2_park_record = false;
    uint64_t k2_park_record_n = 0;
    uint32_t aes_window = 0;             // fheaes_aes_set_window: 0 = automatic (aes_window_plan), FHEAES_AES_WINDOW_OFF = one WoPBS per step, else forced
    StageAudit audit[3];                 // by FHEAES_STAGE_KEYSWITCH, _BLIND_ROTATE, _PFPKS (launch_keyswitch, launch_cbs_pbs, launch_pfpks)
    // test hook (fheaes_alloc_debug), one shot: alloc_seen counts the device allocations ctx_malloc has been asked for since the hook was
    // last set; the alloc_fail_nth-th of them (0: none) goes to the runtime with a size it must refuse
    uint64_t alloc_seen = 0, alloc_fail_nth = 0;
    // keys
    int8_t *ksk_frag = nullptr, *pfpksk_frag = nullptr;      // balanced key bytes in MFMA B-fragment order
    uint32_t ks_ksteps = 0, ks_coltiles = 0, pf_ksteps = 0, pf_coltiles = 0;
    size_t ksk_frag_bytes = 0, pfpksk_frag_bytes = 0, bskf_bytes = 0;
    double2 *bskf = nullptr;
    bool have_keys = false;
    // tables
    double2 *tw_d = nullptr;            // the transform's table T[17 k1 + b] = psi^(b (4 k1 + 1)) (fft_dev.h)
    uint64_t *lutset_d[LUTSET_COUNT] = {};
    int lutset_n[LUTSET_COUNT] = {};
    uint64_t *lut_tag_d[2] = {};        // the CCM tag check (build_tag_lut_host): [0] 8 bits -> byte != 0, [1] 16 bits -> input == 0
    // workspace
    DevBuf ws_small, ws_pbs, ws_ggsw, ws_ggswf, ws_vp, ws_tmp_a, ws_tmp_b, ws_tmp_c, ws_luts, ws_misc, ws_digits, ws_park, ws_park_owner, ws_tree;
    DevBuf ws_park_pattern, ws_park_record;
    DevBuf stage[4];                     // host-memspace calls stage their arguments here (grow-only, reused)
    // pinned host staging for the counter bytes of add_scalar; `pin_ev` marks the last copy out of it
    uint8_t *pin = nullptr;
    size_t pin_bytes = 0;
    hipEvent_t pin_ev = nullptr;
    // profiling
    bool prof = false;
    struct Pending { hipEvent_t a, b; int stage; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    double stage_ms[FHEAES_STAGE_COUNT] = {};
    uint64_t stage_launches[FHEAES_STAGE_COUNT] = {};
    uint64_t stage_units[FHEAES_STAGE_COUNT] = {};

    int fail(int code, const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        tl_error = buf;
        tl_error_ctx_id = id;
        return code;
    }
};

#define HIP_TRY(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) return (ctx)->fail(FHEAES_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

#define TRY(expr)                  \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != FHEAES_OK) return rc__; \
    } while (0)

struct CtxLock {
    std::unique_lock<std::recursive_mutex> lk;
    explicit CtxLock(const fheaes_ctx *c) { if (c) lk = std::unique_lock<std::recursive_mutex>(const_cast<fheaes_ctx *>(c)->mu); }
};

namespace {

// The one place where a live context allocates device memory, and where a refused allocation becomes FHEAES_ERR_NOMEM (the contract is
// at FHEAES_ERR_NOMEM in include/fheaes.h).  In: ensure() -- every workspace, staging, parking and audit buffer --, the key images and
// staging arrays of upload_keys_impl, the images of fheaes_clone_keys (counted on the destination).  Out: fheaes_create (there is no
// context yet: it fails as a whole, FHEAES_ERR_DEVICE), the pinned HOST buffer of upload_pinned, the developer build's StampReport.
// Refused: *p is null, the message names the bytes asked for, and the runtime's last error is read away -- it outlives the call that
// caused it, and the next launcher's HIP_TRY(hipGetLastError()) on this thread would report a launch that succeeded as failed.
// Under fheaes_alloc_debug the chosen allocation asks the runtime for twice the device's total memory instead: the refusal, and the
// error state it leaves behind, are the runtime's own.
int ctx_malloc(fheaes_ctx *c, void **p, size_t bytes)
{
    size_t ask = bytes;
    *p = nullptr;
    if (++c->alloc_seen == c->alloc_fail_nth) {
        c->alloc_fail_nth = 0;
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(c, hipMemGetInfo(&free_bytes, &total_bytes));
        ask = 2 * total_bytes;
    }
    const hipError_t e = hipMalloc(p, ask);
    if (e == hipSuccess) return FHEAES_OK;
    *p = nullptr;
    (void)hipGetLastError();
    if (ask != bytes) return c->fail(FHEAES_ERR_NOMEM, "hipMalloc(%zu bytes): %s (fheaes_alloc_debug: the runtime was asked for %zu)", bytes, hipGetErrorString(e), ask);
    return c->fail(FHEAES_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
}

int ensure(fheaes_ctx *c, DevBuf &b, size_t bytes)
{
    if (b.bytes >= bytes) return FHEAES_OK;
    if (b.p) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    TRY(ctx_malloc(c, &b.p, bytes));
    b.bytes = bytes;
    return FHEAES_OK;
}

// ---- profiling -------------------------------------------------------------------------------
int prof_flush(fheaes_ctx *c)
{
    for (auto &pe : c->pending) {
        HIP_TRY(c, hipEventSynchronize(pe.b));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, pe.a, pe.b));
        c->stage_ms[pe.stage] += ms;
        c->free_events.push_back(pe.a);
        c->free_events.push_back(pe.b);
    }
    c->pending.clear();
    return FHEAES_OK;
}

struct StageScope {
    fheaes_ctx *c;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    StageScope(fheaes_ctx *ctx, int st, uint64_t units) : c(ctx), stage(st), on(ctx->prof)
    {
        c->stage_launches[stage] += 1;
        c->stage_units[stage] += units;
        if (!on) return;
        if (c->pending.size() > 4096) prof_flush(c);
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!c->free_events.empty()) { e = c->free_events.back(); c->free_events.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
            return e;
        };
        a = get(); b = get();
        if (a) (void)hipEventRecord(a, c->stream);
    }
    ~StageScope()
    {
        if (!on || !a || !b) return;
        (void)hipEventRecord(b, c->stream);
        c->pending.push_back({a, b, stage});
    }
};

#ifdef EP_STAMPS
// developer build: per-phase cycle counts written by the blind-rotation kernels
struct StampReport {
    fheaes_ctx *c; unsigned long long *d = nullptr; size_t waves; const char *const *names; int per_wg;
    StampReport(fheaes_ctx *ctx, size_t waves_, const char *const *names_, int per_wg_ = 0) : c(ctx), waves(waves_), names(names_), per_wg(per_wg_)
    {
        (void)hipMalloc((void **)&d, waves * EP_NPH * 8);
        (void)hipMemsetAsync(d, 0, waves * EP_NPH * 8, c->stream);
    }
    ~StampReport()
    {
        std::vector<unsigned long long> h(waves * EP_NPH);
        (void)hipMemcpyAsync(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        double tot[EP_NPH] = {}, all = 0;
        for (size_t w = 0; w < waves; ++w) for (int i = 0; i < EP_NPH; ++i) tot[i] += (double)h[w * EP_NPH + i];
        for (int i = 0; i < EP_NPH; ++i) all += tot[i];
        fprintf(stderr, "K2 phase cycles per wave per iteration (s_memtime ticks, avg over %zu waves):\n", waves);
        for (int i = 0; i < EP_NPH; ++i) fprintf(stderr, "  %-32s %9.0f  %5.1f %%\n", names[i], tot[i] / ((double)waves * c->n), 100.0 * tot[i] / all);
        fprintf(stderr, "  %-32s %9.0f\n", "total", all / ((double)waves * c->n));
        if (per_wg) {                                   // the same per wave slot of a workgroup (who is the slowest at each barrier)
            fprintf(stderr, "  per wave of a workgroup:      ");
            for (int w = 0; w < per_wg; ++w) fprintf(stderr, " %7d", w);
            fprintf(stderr, "\n");
            for (int i = 0; i < EP_NPH; ++i) {
                fprintf(stderr, "  %-30s", names[i]);
                for (int w = 0; w < per_wg; ++w) {
                    double t = 0;
                    for (size_t g = w; g < waves; g += per_wg) t += (double)h[g * EP_NPH + i];
                    fprintf(stderr, " %7.0f", t / ((double)(waves / per_wg) * c->n));
                }
                fprintf(stderr, "\n");
            }
        }
    }
};
#endif

// The arguments of an entry point, in the memory space of the call.  FHEAES_DEVICE: every pointer is used as it is and nothing but the
// work itself is enqueued.  Host memory: arguments are staged through context-owned device buffers (grown on demand, reused by later
// calls -- the per-byte `sbox` call pattern of the reference's Rust side must not pay a hipMalloc/hipFree each time), and finish()
// returns with the output copied back and the stream drained.  An entry point states every argument and its size once, here.
struct Staged {
    fheaes_ctx *c;
    const bool host;
    int used = 0;
    struct Back { void *host, *dev; size_t bytes; } back[2] = {};      // the outputs to copy back (host memory only)
    int n_back = 0;
    Staged(fheaes_ctx *ctx, int memspace) : c(ctx), host(memspace != FHEAES_DEVICE) {}
    ~Staged() { if (host) (void)hipStreamSynchronize(c->stream); }      // host pointers are borrowed for the duration of the call only
    // *dev: where the kernels find argument p of `bytes` bytes
    template <class T> int arg(T *p, size_t bytes, T **dev, bool read, bool written)
    {
        *dev = p;
        if (!host) return FHEAES_OK;
        if (used >= 4) return c->fail(FHEAES_ERR_INVALID, "internal: too many staged arguments");
        TRY(ensure(c, c->stage[used], bytes ? bytes : 8));
        *dev = (T *)c->stage[used++].p;
        if (read) HIP_TRY(c, hipMemcpyAsync((void *)*dev, p, bytes, hipMemcpyHostToDevice, c->stream));
        if (written) {
            if (n_back >= 2) return c->fail(FHEAES_ERR_INVALID, "internal: too many staged outputs");
            back[n_back++] = {(void *)p, (void *)*dev, bytes};
        }
        return FHEAES_OK;
    }
    template <class T> int in(const T *p, size_t bytes, const T **dev) { return arg(p, bytes, dev, true, false); }
    template <class T> int out(T *p, size_t bytes, T **dev) { return arg(p, bytes, dev, false, true); }
    template <class T> int inout(T *p, size_t bytes, T **dev) { return arg(p, bytes, dev, true, true); }
    int finish()
    {
        if (!host) return FHEAES_OK;
        for (int i = 0; i < n_back; ++i) HIP_TRY(c, hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FHEAES_OK;
    }
};

}  // namespace
