/*
 * fheaes.h -- C ABI of the MI355X-native FHE-AES engine (libfheaes.so).
 *
 * Drop-in boundary for the WoPBS S-Box hot path of rostin79s/TFHE-AES.  Every entry
 * point names the reference interface it replaces (paths relative to the reference
 * repository).  The reference is a pure-Rust crate with no FFI of its own; these are
 * the symbols a Rust `extern "C"` shim would bind.
 *
 * Conventions
 *   - all ciphertext / key words are uint64_t (torus q = 2^64), little endian, contiguous;
 *   - LWE ciphertext  = [a_0 .. a_{d-1}, b]                      (d+1 words);
 *   - GLWE ciphertext = [A_0 | .. | A_{k-1} | B], each N words   ((k+1)N words);
 *   - an AES byte     = 8 LWE ciphertexts under the big key (d = kN), block j = bit j (LSB first),
 *                       message bit at the MSB (delta = 2^63, no padding)   (client.rs:123-138);
 *   - an AES state    = 16 bytes, index = 4*col + row, byte 0 = MSB of the u128;
 *   - every function returns FHEAES_OK (0) or a negative error code and never unwinds;
 *     fheaes_last_error() gives the message.  Shape / parameter mismatches are errors;
 *   - `memspace` says where the data pointers of that call live: FHEAES_HOST (the engine
 *     stages them through HBM) or FHEAES_DEVICE (HBM pointers, work is enqueued on the
 *     context's stream and NOT synchronised: call fheaes_synchronize()).
 *   - per-call pointers are borrowed for the duration of the call; keys are copied into
 *     HBM by fheaes_upload_keys() and owned by the context (server.rs:32-35 takes keys by value).
 *     The HOST side arrays of a FHEAES_DEVICE call (key indices, counters, clear blocks and bytes, runs, a mask key) are consumed
 *     before the call returns -- the tables among them copied into the context's one pinned buffer, from which the stream uploads
 *     them -- so the caller may change or free them at once; the resident arrays are read and written when the stream gets there.  That pinned buffer is shared by
 *     the calls of a context: a call that needs it waits (on the host) for the previous upload out of it, not for the kernels
 *     that read the table.  A call that uploads a second table (XTS, the MAC chains, CCM, CMAC, the key unwrap) therefore waits for
 *     its own first upload, and so for whatever the stream still has in front of it: it enqueues all its work, but returns only
 *     when the stream has reached it (tests/test_gpu_async_contract.py, tests/test_gpu_workspace_state.py).
 */
#ifndef FHEAES_H
#define FHEAES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHEAES_OK 0
#define FHEAES_ERR_INVALID -1  /* bad argument / shape / parameter set */
#define FHEAES_ERR_NOKEYS -2   /* evaluation before fheaes_upload_keys */
#define FHEAES_ERR_DEVICE -3   /* HIP runtime error (message in last_error) */
/* FHEAES_ERR_NOMEM: the device refused an allocation of the context, in the middle of a call -- the workspace grows at request time, and
 * on a device that the caller's own arrays fill, the engine's hipMalloc is the one that fails.  Every device allocation of a live
 * context goes through one function (ctx_malloc, csrc/engine_ctx.h): the workspaces, the staging buffers of host-memspace calls, the
 * parking slab and owner words, the audit's buffers, the key images and staging arrays of the uploads, the images of fheaes_clone_keys
 * (reported on the destination).  Out: fheaes_create, which fails as a whole with FHEAES_ERR_DEVICE before there is a context, and the
 * pinned HOST buffer of the table uploads.  What a caller may rely on after -4 (tests/test_gpu_alloc_failures.py):
 *   - the message names the bytes asked for ("hipMalloc(N bytes): ...");
 *   - the call has enqueued whatever preceded the failed allocation, and nothing after it: no kernel, copy or memset is ever issued on
 *     the buffer that was refused (its size reads 0);
 *   - arrays the call writes, in place or not, hold unspecified words (a host-memspace call copies nothing back: the caller's host
 *     output is untouched); arrays it only reads are untouched;
 *   - the context stays usable and keeps its keys: the same call after memory has been freed returns the words of a call that never
 *     failed, whatever the failed one left in the workspace, and the next call that succeeds is not reported as failed -- the runtime's
 *     error state is read away where the refusal is met;
 *   - a failed fheaes_upload_keys / _seeded / fheaes_clone_keys leaves the context WITHOUT keys, also where it had some: the next
 *     evaluation is FHEAES_ERR_NOKEYS until an upload or a clone succeeds; the source of a failed clone is unharmed;
 *   - a failed fheaes_audit_set leaves the audit off; a failed fheaes_reserve leaves what it had grown so far;
 *   - profile counters: a stage counts a launch when its launcher is entered, before the launcher's own allocation, so after a failed
 *     call `launches` and `units` may include one launch per stage that never happened.  They are defined again after
 *     fheaes_profile_reset. */
#define FHEAES_ERR_NOMEM -4

#define FHEAES_HOST 0
#define FHEAES_DEVICE 1

/* WopbsParameters of the reference (client.rs:31-57), minus the noise fields that only
 * key generation needs.  polynomial_size must be 512. */
typedef struct fheaes_params {
    uint32_t lwe_dimension;   /* n   = 669 */
    uint32_t glwe_dimension;  /* k   = 4   */
    uint32_t polynomial_size; /* N   = 512 */
    uint32_t pbs_base_log;    /* 8  */
    uint32_t pbs_level;       /* 5  */
    uint32_t ks_base_log;     /* 2  */
    uint32_t ks_level;        /* 6  */
    uint32_t pfks_base_log;   /* 12 */
    uint32_t pfks_level;      /* 3  */
    uint32_t cbs_base_log;    /* 15 */
    uint32_t cbs_level;       /* 1  */
} fheaes_params;

typedef struct fheaes_ctx fheaes_ctx;

/* ---- lifetime ------------------------------------------------------------------ */
/* Server::new (server.rs:32): create an engine on HIP device `device`. */
int fheaes_create(const fheaes_params *params, int device, fheaes_ctx **out);
void fheaes_destroy(fheaes_ctx *ctx);
/* message of the last failing call on this context (ctx == NULL: last fheaes_create failure).  The pointer is a per-thread copy,
 * valid until the same thread's next call into the library (a context may be shared between threads). */
const char *fheaes_last_error(const fheaes_ctx *ctx);

/* ---- keys ---------------------------------------------------------------------- */
/* word counts of the three evaluation keys for this parameter set */
#define FHEAES_KEY_KSK 0    /* [kN][ks_level][n+1]                 pbs_server_key.key_switching_key (many_wopbs.rs:168) */
#define FHEAES_KEY_BSK 1    /* [n][pbs_level][k+1][k+1][N]  STANDARD domain  wopbs_server_key.bootstrapping_key (many_wopbs.rs:34-35) */
#define FHEAES_KEY_PFPKSK 2 /* [k+1][kN+1][pfks_level][(k+1)N]     cbs_pfpksk (many_wopbs.rs:76) */
size_t fheaes_key_words(const fheaes_ctx *ctx, int which);

/* Copies the keys into HBM and converts the BSK to the engine's Fourier layout.
 * Level index 0 is the most significant level (weight 2^(64-base_log)). */
int fheaes_upload_keys(fheaes_ctx *ctx, const uint64_t *ksk, const uint64_t *bsk, const uint64_t *pfpksk, int memspace);

/* The same keys as (public mask key, bodies): every mask word of the three keys is the output of a public, counter-based
 * ChaCha20 stream -- mask word j of key ciphertext q of key t (t = 3 KSK, 4 BSK, 5 PFPKSK) is 64-bit word j % 8 of the
 * RFC 8439 block j / 8 under (mask_key, nonce = (t, q)) (csrc/client.c) -- so only the bodies travel: KSK [kN][ks_level]
 * words, BSK [n][pbs_level][k+1][N], PFPKSK [k+1][kN+1][pfks_level][N]: 0.19 GB instead of 1.04 GB at PARAM_OPT, and the masks
 * are regenerated on the GPU.  `mask_key` is a HOST array of 8 uint32 (256 bits) whatever `memspace` says about the bodies.
 * The counterpart in the reference's world are tfhe-rs' Seeded* key containers, which client.rs:106-107 does not use (it builds
 * full keys in memory and hands them over by value, server.rs:32); device keys are bit-identical to fheaes_upload_keys of the
 * expanded keys. */
size_t fheaes_key_body_words(const fheaes_ctx *ctx, int which);
int fheaes_upload_keys_seeded(fheaes_ctx *ctx, const uint32_t *mask_key, const uint64_t *ksk_body, const uint64_t *bsk_body,
                              const uint64_t *pfpksk_body, int memspace);

/* Several engines, one upload.  The reference is ONE process that fans the CTR blocks out over rayon worker threads which share
 * `&Server` (main.rs:55-64, server.rs:32-35): a drop-in that wants G GPUs (or several concurrent streams on one GPU) creates G
 * contexts, uploads the keys into the first and clones the CONVERTED key images (1.04 GB) into the others, device to device:
 * hipMemcpyPeerAsync over xGMI between GPUs, an HBM copy inside one.  Block i then goes to context i * G / n_blocks, one host
 * thread per context (contexts are independent: own stream, own workspace; calls on ONE context are serialised by its lock).
 * Both contexts must have been created with the same parameter set. */
int fheaes_clone_keys(fheaes_ctx *dst, fheaes_ctx *src);
/* How the last fheaes_clone_keys INTO `ctx` moved the key images: `path` = FHEAES_CLONE_NONE (no clone yet), _SAME_DEVICE (HBM copy),
 * _PEER (hipDeviceCanAccessPeer said yes and peer access is enabled: hipMemcpyPeerAsync is a direct xGMI transfer) or _STAGED (no
 * peer access between the two devices: the runtime stages the copy through host memory); `bytes` moved and wall `seconds` of the
 * copies.  Any of the three out-pointers may be NULL.  (The cross-device paths have not run on hardware yet: a builder's box has
 * one GPU.  The reference has no counterpart: its rayon workers share one `&Server` in host memory, main.rs:55-64.) */
#define FHEAES_CLONE_NONE 0
#define FHEAES_CLONE_SAME_DEVICE 1
#define FHEAES_CLONE_PEER 2
#define FHEAES_CLONE_STAGED 3
int fheaes_clone_info(fheaes_ctx *ctx, int *path, uint64_t *bytes, double *seconds);

/* ---- noise guard ---------------------------------------------------------------- */
/* The reference builds tfhe-rs with `noise-asserts` (Cargo.toml:7) under MaxNoiseLevel::new(5) (client.rs:92): a sum of more than
 * five nominal-noise ciphertexts between two bootstraps panics (many_wopbs.rs:101-108 resets every WoPBS output to NOMINAL).
 * What the engine has is a STATIC SCHEDULE ASSERTION, not runtime noise tracking: each linear layer of the engine's own AES schedule
 * declares how many WoPBS outputs it sums per output word (MixColumns + AddRoundKey = 4 + 1, the key-expansion sums = 2, the equivalent
 * inverse cipher's InvShiftRows + InvMixColumns + AddRoundKey = 4 + 1, its round-key conversion's InvMixColumns = 4, refreshed after); a layer
 * whose gather table would sum more than the limit is refused with FHEAES_ERR_INVALID, and the largest count any call on this context
 * has declared can be read back.  Ciphertext words carry no noise metadata: a state that a caller has already summed before passing
 * it in counts as nominal here.  Callers that add ciphertext words themselves (the stage-level entry points hand out raw uint64
 * words) keep their own count, as users of tfhe-rs' `unchecked_*` do. */
#define FHEAES_MAX_NOISE_LEVEL 5
int fheaes_noise_level_seen(fheaes_ctx *ctx, uint32_t *max_seen, uint32_t *limit);

/* ---- stream / sync / workspace ------------------------------------------------- */
int fheaes_set_stream(fheaes_ctx *ctx, void *hip_stream); /* NULL: the context's own stream */
int fheaes_synchronize(fheaes_ctx *ctx);
/* pre-size the device workspace for batches of up to `max_bits` one-bit inputs in flight */
int fheaes_reserve(fheaes_ctx *ctx, uint64_t max_bits);

/* ---- the hot path, stage by stage (what many_wopbs.rs calls into tfhe 0.11.2) --- */
/* K1  shortint::wopbs::WopbsKey::extract_bits_assign (many_wopbs.rs:194): one LWE keyswitch
 *     big -> small per bit.  in [m][kN+1] -> out [m][n+1]. */
int fheaes_keyswitch_batch(fheaes_ctx *ctx, const uint64_t *lwe_in, uint64_t m, uint64_t *lwe_out, int memspace);
/* K2  the PBS inside circuit_bootstrap_boolean (many_wopbs.rs:253), CBS level `level` (1-based):
 *     in [m][n+1] -> out [m][kN+1] = LWE of bit * 2^(64 - cbs_base_log*level).  A batch of more than 65,536 bits is cut into
 *     launches of that many (one launch's parking space is one buffer below 2 GiB); up to that size it is one launch, as before. */
int fheaes_cbs_pbs_batch(fheaes_ctx *ctx, const uint64_t *lwe_small, uint64_t m, uint32_t level, uint64_t *lwe_out, int memspace);
/* K3  the k+1 private functional packing keyswitches of circuit_bootstrap_boolean:
 *     in [m][kN+1] -> out [m][k+1][(k+1)N]  (one GGSW level, standard domain). */
int fheaes_pfpks_batch(fheaes_ctx *ctx, const uint64_t *lwe_in, uint64_t m, uint64_t *ggsw_rows_out, int memspace);
/* K4  ggsw.fill_with_forward_fourier (many_wopbs.rs:263): `polys` torus polynomials -> Fourier,
 *     out [polys][256][2] doubles (natural order, re/im interleaved). */
int fheaes_forward_fourier_batch(fheaes_ctx *ctx, const uint64_t *polys_in, uint64_t polys, double *fourier_out, int memspace);
/* K5  vertical_packing (many_wopbs.rs:277).  ggsw_fourier [n_inputs][bits][cbs_level][k+1][k+1][256][2];
 *     luts [n_sets][n_luts][bits][W] with n_sets = lut_per_input ? n_inputs : 1 and W = max(2^bits, N) words per
 *     (LUT, output bit) as gen_lut.rs:19-23 sizes them; out [n_inputs][n_luts][bits][kN+1].
 *     bits <= 9 (all the AES path uses): one LUT polynomial per output bit, blind rotation only.  9 < bits <= 16: the
 *     2^(bits-9) polynomials go through the CMUX tree over input bits 9..bits-1 first, then the rotation over bits 0..8
 *     ("parity unpinned" for bits > 9: the reference never calls many_wopbs_without_padding wider than 9 bits and holds no
 *     fixture for it; the split follows upstream vertical_packing and is checked against this repo's oracle only). */
int fheaes_vertical_packing_batch(fheaes_ctx *ctx, const double *ggsw_fourier, uint64_t n_inputs, uint32_t bits,
                                  const uint64_t *luts, uint32_t n_luts, int lut_per_input, uint64_t *lwe_out, int memspace);

/* K6  one linear layer alone: InvMixColumns as Server::aes_decrypt takes it (inv_mix_columns.rs:4-58), the four-term gather WITHOUT a
 *     round key.  multiples [n_blocks][16][4][8][kN+1] = fheaes_many_sbox(.., inv = 1) of the state's bytes ({9x, 11x, 13x, 14x});
 *     state_out [n_blocks][16][8][kN+1], byte 4 col + row = sum over j of (InvMixColumns[row][j] x) of byte 4 col + j, wrapping sums of
 *     four words (declared to the noise guard as 4).  n_blocks <= 65,535; needs no keys; overlapping buffers are FHEAES_ERR_INVALID.
 *     Accounted under FHEAES_STAGE_LINEAR (units: blocks).  The yardstick of the other K6 kernels (tools/xts.py). */
int fheaes_inv_mix_columns_batch(fheaes_ctx *ctx, const uint64_t *multiples, uint64_t n_blocks, uint64_t *state_out, int memspace);

/* ---- the plugin API of the path ------------------------------------------------ */
/* many_wopbs_without_padding (many_wopbs.rs:31), batched over radix inputs.
 *   lwe_in [n_inputs][bits][kN+1], bits in {1..16}; luts as above; out [n_inputs][n_luts][bits][kN+1]. */
int fheaes_wopbs_batch(fheaes_ctx *ctx, const uint64_t *lwe_in, uint64_t n_inputs, uint32_t bits,
                       const uint64_t *luts, uint32_t n_luts, int lut_per_input, uint64_t *lwe_out, int memspace);
/* gen_lut (gen_lut.rs:9) for message_modulus 2, carry_modulus 1: f_table[2^nb_block] -> out [nb_block][max(2^nb_block, N)]
 * (host only), nb_block in 1..16. */
int fheaes_gen_lut(uint32_t nb_block, const uint64_t *f_table, uint64_t *lut_out);
/* sbox (sbox.rs:46), in place over n_bytes bytes: bytes [n_bytes][8][kN+1]; inv = 0 SBOX, 1 INV_SBOX. */
int fheaes_sbox(fheaes_ctx *ctx, uint64_t *bytes, uint64_t n_bytes, int inv, int memspace);
/* many_sbox (sbox.rs:68): out [n_bytes][L][8][kN+1], L = 3 {S,2S,3S} (inv=0) or 4 {9x,11x,13x,14x} (inv=1). */
int fheaes_many_sbox(fheaes_ctx *ctx, const uint64_t *bytes, uint64_t n_bytes, int inv, uint64_t *out, int memspace);

/* ---- Server API (server.rs) ---------------------------------------------------- */
/* Server::aes_key_expansion (server.rs:107): key [16][8][kN+1] -> round_keys [11][16][8][kN+1]. */
int fheaes_aes_key_expansion(fheaes_ctx *ctx, const uint64_t *key, uint64_t *round_keys, int memspace);
/* Server::aes_encrypt (server.rs:39), batched: state [n_blocks][16][8][kN+1] in place, one set of round keys. */
int fheaes_aes_encrypt(fheaes_ctx *ctx, const uint64_t *round_keys, uint64_t *state, uint64_t n_blocks, int memspace);
/* Server::aes_decrypt (server.rs:67), batched. */
int fheaes_aes_decrypt(fheaes_ctx *ctx, const uint64_t *round_keys, uint64_t *state, uint64_t n_blocks, int memspace);
/* The equivalent inverse cipher (FIPS-197 section 5.3.5, Fig. 15), added in 0.4 as two entry points next to the reference's schedule
 * (fheaes_aes_decrypt stays word for word Server::aes_decrypt, server.rs:67-105).  That schedule runs two WoPBS per round -- INV_SBOX,
 * then the 4-LUT {9x, 11x, 13x, 14x} InvMixColumns -- which, as server.rs:86-89 says, almost doubles the time of encryption: 19 x 128
 * bit circuit bootstraps per block against 1,280.  InvMixColumns is linear, so IMC(InvS(x)) + IMC(k) needs ONE WoPBS per byte, with the
 * composed tables {9, 11, 13, 14} * InvS[x], once the round keys have gone through InvMixColumns: 10 WoPBS per block, as for encryption.
 * The words differ from fheaes_aes_decrypt's (another algorithm); the plaintext is the same.
 *
 * Decryption round keys from the expanded ones, once per AES key (2 x 1,152 bit circuit bootstraps):
 * dw[0] = w[0], dw[10] = w[10], dw[r] = InvMixColumns(w[r]) for r = 1..9, each byte refreshed to nominal noise by an identity WoPBS
 * (as the key expansion's refresh, server.rs:150; without it a round would sum 4 WoPBS outputs + a key of level 4 = 8 > 5).
 * round_keys, dec_round_keys: [11][16][8][kN+1].  Identical (or overlapping) buffers are FHEAES_ERR_INVALID. */
int fheaes_aes_decryption_round_keys(fheaes_ctx *ctx, const uint64_t *round_keys, uint64_t *dec_round_keys, int memspace);
/* The equivalent inverse cipher, batched, in place: state [n_blocks][16][8][kN+1], dec_round_keys from fheaes_aes_decryption_round_keys. */
int fheaes_aes_decrypt_equivalent(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint64_t *state, uint64_t n_blocks, int memspace);
/* AES-192 and AES-256 (FIPS-197 with Nk = 6 / 8 key words and Nr = 12 / 14 rounds): the five AES entry points above with the key size as
 * an argument.  The reference has no counterpart: it is AES-128 only (server.rs:107 expands 4 key words into 44, main.rs runs that one
 * cipher); K1-K5 are blind to the key size, so these are the same schedules with Nr in place of 10.  `key_bits` is 128, 192 or 256,
 * anything else is FHEAES_ERR_INVALID; with key_bits = 128 every function gives word for word what its counterpart above gives (one
 * implementation: the entry points above pass 128).  round_keys and dec_round_keys are [Nr+1][16][8][kN+1], Nr = 10 / 12 / 14: round
 * key r is words 4r..4r+3 of the expanded key.
 *
 * Key expansion (FIPS-197 section 5.2): key [key_bits/8][8][kN+1], bytes in FIPS-197 order (byte 0 first).  The reference's rule
 * (server.rs:107-155: every new word refreshed by an identity WoPBS) for general Nk: RotWord + SubWord + Rcon when i % Nk == 0, SubWord
 * alone when Nk > 6 and i % Nk == 4; 40 / 46 / 52 new words of which 10 / 8 / 13 pass through SubWord.  Every sum has two nominal terms. */
int fheaes_aes_key_expansion_bits(fheaes_ctx *ctx, const uint64_t *key, uint32_t key_bits, uint64_t *round_keys, int memspace);
/* The cipher of FIPS-197 Fig. 5 with Server::aes_encrypt's schedule (server.rs:39): Nr - 1 rounds of the 3-LUT {S, 2S, 3S} WoPBS and
 * the MixColumns gather, then the S-Box round: Nr x 128 = 1,280 / 1,536 / 1,792 bit circuit bootstraps per block. */
int fheaes_aes_encrypt_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks, int memspace);
/* The inverse cipher of FIPS-197 Fig. 12 with Server::aes_decrypt's schedule (server.rs:67): two WoPBS in each of Nr - 1 rounds and one
 * in the last, (2 Nr - 1) x 128 = 2,432 / 2,944 / 3,456 bit circuit bootstraps per block. */
int fheaes_aes_decrypt_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks, int memspace);
/* The equivalent inverse cipher of FIPS-197 Fig. 15: dw[0] = w[0], dw[Nr] = w[Nr], dw[r] = InvMixColumns(w[r]) for r = 1..Nr-1, the
 * 16 (Nr - 1) middle bytes refreshed in one batch; then Nr WoPBS per block, as for encryption.  Overlapping buffers are FHEAES_ERR_INVALID. */
int fheaes_aes_decryption_round_keys_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t *dec_round_keys, int memspace);
int fheaes_aes_decrypt_equivalent_bits(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t *state, uint64_t n_blocks,
                                       int memspace);
/* Server::add_scalar (server.rs:172), batched: state[b] += counters[b] (u128 as {hi, lo}, host array
 * of 2*n_blocks words regardless of memspace).  The first-byte carry uses counter & 0xFF (the
 * reference's server.rs:182 is wrong for counters >= 256). */
int fheaes_add_scalar(fheaes_ctx *ctx, uint64_t *state, uint64_t n_blocks, const uint64_t *counters_hi_lo, int memspace);
/* Public blocks and CTR with a PUBLIC nonce (transciphering: the client sends data under AES-CTR and the AES key under FHE).  The reference
 * has no counterpart: its CTR (main.rs:59-61) encrypts the IV and adds the block index homomorphically (add_scalar: a 16-step carry chain,
 * 143 bit circuit bootstraps per block) before aes_encrypt.  With a public counter the carry chain is clear arithmetic, and most of the
 * first two rounds is common to all blocks of a batch: a WoPBS is a deterministic function of its input words, so every DISTINCT S-Box
 * input of the batch is evaluated once (the rule is exact; 128 consecutive AES-128 counters: 17,051 byte-WoPBS
 * instead of 20,480).  Clear 128-bit values are HOST arrays of (hi, lo) pairs whatever `memspace` says, as fheaes_add_scalar's counters:
 * value = hi << 64 | lo, byte 0 of the AES block the most significant.  round_keys [Nr+1][16][8][kN+1] and state_out
 * [n_blocks][16][8][kN+1] live in `memspace`; key_bits as above; n_blocks = 0 is FHEAES_OK; FHEAES_DEVICE calls only enqueue.
 *
 * aes_encrypt of public blocks: word for word what fheaes_aes_encrypt_bits writes for a state of trivial ciphertexts of these blocks
 * (mask 0, body = bit << 63). */
int fheaes_aes_encrypt_public_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *blocks_hi_lo,
                                   uint64_t n_blocks, uint64_t *state_out, int memspace);
/* SP 800-38A CTR: block i = E_K((iv + first_block + i) mod 2^128) ^ data[i], the clear data folded into the last linear layer (its bits
 * added to the bodies); data_hi_lo == NULL: the keystream itself.  iv_hi_lo: one (hi, lo) pair; data_hi_lo: n_blocks pairs. */
int fheaes_aes_ctr_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *iv_hi_lo, uint64_t first_block,
                        const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* How many byte-WoPBS the two calls above run in each round for these blocks: unique_bytes_per_round[r - 1], r = 1..Nr (host logic only,
 * no context, no GPU; fheaes_aes_encrypt_bits runs 16 n_blocks in every round). */
int fheaes_aes_public_plan(const uint64_t *blocks_hi_lo, uint64_t n_blocks, uint32_t key_bits, uint64_t *unique_bytes_per_round);
/* The keystream of AES-GCM (SP 800-38D GCTR): fheaes_aes_ctr_bits with a 32-bit counter field.  Counter block i is icb with its low 32
 * bits replaced by (low32(icb) + first_block + i) mod 2^32 (inc32); the upper 96 bits never change, so a batch may wrap.  For a 96-bit
 * GCM IV the data blocks start at icb = IV || 00000002 (J0 = IV || 00000001 masks the tag).  GHASH and the tag are NOT computed: a
 * product of two encrypted field elements is far above the five-term noise budget. */
int fheaes_aes_ctr32_bits(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, const uint64_t *icb_hi_lo, uint64_t first_block,
                          const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* The DECRYPTION direction of the public calls (AES-CBC data at rest, or any mode that deciphers public blocks): the equivalent inverse
 * cipher (fheaes_aes_decrypt_equivalent_bits) on public blocks with the same sharing rule.  dec_round_keys [Nr+1][16][8][kN+1] are
 * fheaes_aes_decryption_round_keys_bits' output.  The id of a round-1 input is (key, position, byte) -- the input is dw[Nr][p] +
 * trivial(byte) -- and the id of a later one is (position, ids of its four sources (4 ((col - j) mod 4) + j, InvShiftRows folded in));
 * a round is the 4-LUT {9, 11, 13, 14} InvS WoPBS over its pool and sums 4 outputs + dw[Nr - r], 5 terms as
 * fheaes_aes_decrypt_equivalent_bits; the last layer is InvS through InvShiftRows + dw[0].  data_hi_lo (n_blocks pairs, may be NULL) is
 * folded into the last layer as fheaes_aes_ctr_bits' data.  The result is, word for word, what fheaes_aes_decrypt_equivalent_bits writes
 * for trivial ciphertexts of the blocks, with bit << 63 of the data added to the bodies.  Argument rules of fheaes_aes_encrypt_public_bits. */
int fheaes_aes_decrypt_public_bits(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, const uint64_t *blocks_hi_lo,
                                   const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* SP 800-38A CBC decryption: block i = D_K(ct[i]) ^ (i ? ct[i-1] : iv), which is fheaes_aes_decrypt_public_bits with the ciphertext moved
 * down by one block as its data.  iv_hi_lo: one (hi, lo) pair; ct_hi_lo: n_blocks pairs.  A caller continuing a stream passes the
 * previous ciphertext block as iv.  Equal ciphertext blocks share their S-Boxes; CBC ENCRYPTION is serial and is not offered. */
int fheaes_aes_cbc_decrypt_bits(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, const uint64_t *iv_hi_lo,
                                const uint64_t *ct_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* XTS-AES decryption (IEEE 1619, SP 800-38E: disk images, volume snapshots, encrypted block storage) of a PUBLIC ciphertext under two
 * encrypted keys: P_j = D_K1(C_j ^ T_j) ^ T_j with T_j = E_K2(tweak) * alpha^j in GF(2^128), j the block's index in its data unit.  As
 * parallel as CBC decryption, but the per-block mask T_j is ENCRYPTED, so C_j ^ T_j is not public and the public path serves the tweak
 * blocks only.
 *
 * The field: bit b (LSB first) of block byte p is degree 8p + b, which is the flattened [16][8] index of a state -- no permutation.
 * Multiplication by alpha^j is linear over GF(2) and XOR of MSB-encoded bits is the wrapping add, so T * alpha^j is ONE gather: for
 * 0 <= j <= 121 output bit i sums bit i - j (if i >= j) and bits 128 - j + m for m in {i, i-1, i-2, i-7} with 0 <= m < j (the bits
 * shifted out, reduced once by x^128 = x^7 + x^2 + x + 1): distinct sources, at most 4.  (Beyond 121 a shifted-out bit is reduced
 * twice: weight 5 at 122.)  The rows are applied to the base in one sum: doubling step by step adds a ciphertext to itself, which
 * cancels the message but not the noise.
 *
 * Levels against FHEAES_MAX_NOISE_LEVEL = 5: E_K2(tweak) leaves the public call at 2 and an identity WoPBS makes it 1 (the ANCHOR of
 * the unit); the gather gives T_j at up to 4.  Raw on both sides of the cipher that passes going in (4 + dw[Nr] = 5) and fails coming out
 * (InvS + dw[0] + 4 = 6), so every T_j is refreshed by an identity WoPBS, 16 byte-WoPBS per block: 2 going in, 3 coming out, and
 * 16 (Nr + 1) byte-WoPBS per block in all (176 for AES-128).  A unit longer than 120 blocks is cut into segments of 120: segment s
 * gathers offsets 0 .. 119 from anchor s, and offset 120 as well when the call reaches beyond the segment: refreshed, that is anchor
 * s + 1.  Block j takes offset j % 120 of segment j / 120; a unit costs ceil(blocks / 120) serial refreshes after its anchor's, and a
 * segment that lies wholly before the call's first block yields its anchor only.
 *
 * dec_round_keys1: fheaes_aes_decryption_round_keys_bits of key 1; round_keys2: the plain expansion of key 2; both [Nr+1][16][8][kN+1];
 * key_bits 128 or 256 (XTS-AES-128 / -256: two keys of that size; 192 is FHEAES_ERR_INVALID).  tweaks_hi_lo: n_units (hi, lo) pairs, the
 * 16-byte tweak BLOCK of every unit as every clear block here: byte 0 the most significant byte of the u128 -- which is the LEAST
 * significant byte of IEEE 1619's little-endian data-unit number.  ct_hi_lo: n_blocks pairs.  Block b of the call is block
 * (first_block + b) % blocks_per_unit of unit (first_block + b) / blocks_per_unit, so a shard or a continued stream starts anywhere;
 * n_units must cover the blocks named; blocks_per_unit is 1 .. 2^20 (the IEEE bound).  n_blocks = 0 is FHEAES_OK; null or overlapping
 * buffers are FHEAES_ERR_INVALID; FHEAES_DEVICE calls only enqueue.  Equal tweaks share their S-Boxes by the public rule.  The result is
 * word for word: fheaes_aes_encrypt_public_bits(round_keys2, tweaks), the identity WoPBS, the rows above as wrapping sums, the identity
 * WoPBS chained through the anchors, + trivial(C), fheaes_aes_decrypt_equivalent_bits(dec_round_keys1), + T.
 * Not offered: ciphertext stealing (whole blocks only), XTS encryption, a key per block or unit. */
int fheaes_aes_xts_decrypt_bits(fheaes_ctx *ctx, const uint64_t *dec_round_keys1, const uint64_t *round_keys2, uint32_t key_bits,
                                const uint64_t *tweaks_hi_lo, uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block,
                                const uint64_t *ct_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* The same with the two key sets as one-key packed stores (fheaes_pack_round_keys, below): word for word the call above on
 * fheaes_unpack_round_keys of the stores. */
int fheaes_aes_xts_decrypt_packed(fheaes_ctx *ctx, const uint64_t *packed_dec_round_keys1, const uint64_t *packed_round_keys2, uint32_t key_bits,
                                  const uint64_t *tweaks_hi_lo, uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block,
                                  const uint64_t *ct_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* The raw gather alone (no refresh, no keys needed): out[u][t] = anchor[u] * alpha^(first_offset + t), anchor [n_units][128][kN+1],
 * out [n_units][n_offsets][128][kN+1], first_offset + n_offsets - 1 <= 121 and n_offsets >= 1, else FHEAES_ERR_INVALID.  The largest row
 * weight of the offsets is declared to the noise guard.  Accounted under FHEAES_STAGE_LINEAR (units: tweak blocks). */
int fheaes_xts_tweaks(fheaes_ctx *ctx, const uint64_t *anchor, uint64_t n_units, uint32_t first_offset, uint32_t n_offsets, uint64_t *out,
                      int memspace);
/* The sources of output bit `bit` (< 128) of the multiplication by alpha^offset (offset <= 121): their count in *n_sources, their bit
 * indices in sources_out[0 .. count), an array of 4 (host logic only, no context, no GPU). */
int fheaes_xts_tweak_row(uint32_t offset, uint32_t bit, uint32_t *sources_out /* [4] */, uint32_t *n_sources);
/* What fheaes_aes_xts_decrypt_bits runs for a call of this shape (host logic only): `segments` serial tweak refreshes after the anchors',
 * tweak_refresh_bytes byte-WoPBS of identity refresh (16 per touched unit for its anchor, 16 per gathered tweak: one per block of the
 * call and one per chained anchor), cipher_bytes = 16 Nr n_blocks, and the largest count the call declares to the noise guard. */
int fheaes_aes_xts_plan(uint64_t n_units, uint64_t blocks_per_unit, uint64_t first_block, uint64_t n_blocks, uint32_t key_bits,
                        uint64_t *segments, uint64_t *tweak_refresh_bytes, uint64_t *cipher_bytes, uint32_t *max_terms);

/* ---- many AES keys ---------------------------------------------------------------- */
/* One FHE key pair, many AES keys (producers, sessions, rotated keys), each reaching the server encrypted under that FHE key: short
 * messages under many keys.  The reference has no counterpart (one key, main.rs).  K1-K5 know nothing about AES keys and a WoPBS is a
 * deterministic function of its input words, so the calls below are the schedules above with the keys as one more batch axis: every
 * one gives, WORD FOR WORD, what the single-key calls give key by key, in launches that are as full as the whole batch makes them (a
 * key expansion step is one 32 n_keys-bit WoPBS instead of n_keys of 32 bits, 6.4 ms each whatever they carry).
 *
 * `n_keys` sets of round keys are [n_keys][Nr+1][16][8][kN+1]: slice i is a valid argument of every single-key entry point.  One key
 * size per call.  n_keys = 0 or n_keys > FHEAES_MAX_KEYS is FHEAES_ERR_INVALID (the bound: a key index has 16 bits in the head word of a
 * pool entry of the public calls).  `key_of_block` is a HOST array of n_blocks uint32 whatever `memspace` says, as fheaes_add_scalar's
 * counters; an entry >= n_keys is FHEAES_ERR_INVALID; a key that no block names is legal.  n_blocks = 0 is FHEAES_OK; FHEAES_DEVICE calls
 * only enqueue; the noise guard sees the counts of the single-key schedules. */
#define FHEAES_MAX_KEYS 65536
/* keys [n_keys][key_bits/8][8][kN+1] -> round_keys [n_keys][Nr+1][16][8][kN+1]: the rule of fheaes_aes_key_expansion_bits with every step
 * ONE WoPBS over the 4 n_keys bytes of word i of all keys (40 / 46 / 52 identity refreshes, 10 / 8 / 13 SubWords); slice i is word for
 * word fheaes_aes_key_expansion_bits of key i. */
int fheaes_aes_key_expansion_batch(fheaes_ctx *ctx, const uint64_t *keys, uint32_t key_bits, uint64_t n_keys, uint64_t *round_keys, int memspace);
/* The 16 (Nr - 1) n_keys middle bytes of all keys through one {9x, 11x, 13x, 14x} WoPBS, one InvMixColumns gather and one identity WoPBS;
 * slice i is word for word fheaes_aes_decryption_round_keys_bits of slice i.  Overlapping buffers are FHEAES_ERR_INVALID. */
int fheaes_aes_decryption_round_keys_batch(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys,
                                           uint64_t *dec_round_keys, int memspace);
/* fheaes_aes_encrypt_bits / _decrypt_bits / _decrypt_equivalent_bits with a key per block: state block b is processed in place under
 * round_keys[key_of_block[b]] (dec_round_keys for the equivalent inverse cipher), word for word what the single-key call writes for that
 * block under that key; every round is one WoPBS over all 16 n_blocks bytes. */
int fheaes_aes_encrypt_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                             uint64_t *state, uint64_t n_blocks, int memspace);
int fheaes_aes_decrypt_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                             uint64_t *state, uint64_t n_blocks, int memspace);
int fheaes_aes_decrypt_equivalent_keyed(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keys,
                                        const uint32_t *key_of_block, uint64_t *state, uint64_t n_blocks, int memspace);
/* fheaes_aes_encrypt_public_bits with a key per block; data_hi_lo (n_blocks pairs, may be NULL) is folded into the last layer as in
 * fheaes_aes_ctr_bits, so several CTR streams under several keys are one call (the caller builds the counter blocks).  The sharing rule
 * gains the key: the id of a round-1 input is (key, position, byte), so equal blocks under different keys are different inputs and are
 * never shared, and equal inputs under the same key still are. */
int fheaes_aes_public_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint32_t *key_of_block,
                            const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks, uint64_t *state_out, int memspace);
/* fheaes_aes_public_plan for the call above (host logic only, no context, no GPU); with every key 0 it gives fheaes_aes_public_plan's counts. */
int fheaes_aes_public_plan_keyed(const uint64_t *blocks_hi_lo, const uint32_t *key_of_block, uint64_t n_blocks, uint64_t n_keys,
                                 uint32_t key_bits, uint64_t *unique_bytes_per_round);
/* fheaes_aes_decrypt_public_bits with a key per block (dec_round_keys [n_keys][Nr+1][16][8][kN+1]): word for word what
 * fheaes_aes_decrypt_equivalent_keyed writes for trivial ciphertexts of the blocks, plus the data; several CBC streams under several keys
 * are one call (the caller moves each stream's ciphertext down by one block for data_hi_lo). */
int fheaes_aes_decrypt_public_keyed(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keys,
                                    const uint32_t *key_of_block, const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks,
                                    uint64_t *state_out, int memspace);
/* How many byte-WoPBS the decryption-direction calls run in each round (host logic only, no context, no GPU).  key_of_block may be NULL:
 * every block under key 0, the plan of fheaes_aes_decrypt_public_bits and fheaes_aes_cbc_decrypt_bits. */
int fheaes_aes_decrypt_public_plan_keyed(const uint64_t *blocks_hi_lo, const uint32_t *key_of_block, uint64_t n_blocks, uint64_t n_keys,
                                         uint32_t key_bits, uint64_t *unique_bytes_per_round);

/* ---- packed ciphertexts --------------------------------------------------------- */
/* Every entry point above hands its result out one LWE ciphertext per bit: kN + 1 words (16,392 bytes at PARAM_OPT) for one bit.  A
 * packing key switch puts N = 512 bits into the N coefficients of ONE GLWE ciphertext, (k+1)N words (20,480 bytes) for 512 bits:
 * 409.8 times smaller, for storing or sending what the engine computed.  The reference has nothing here: it hands whole radix
 * ciphertexts across in memory (client.rs:147-175) and never packs or serialises them; in tfhe-rs the counterpart is the compressed
 * ciphertext list, which needs a packing key of its own.  This needs NO new key: block r = k of the PFPKSK every context holds is
 * GLWE_S(sigma_i * 2^(64 - b(l+1))) with f(x) = x, an LWE -> GLWE key-switching key that puts the message into the constant coefficient.
 *
 * With ks[t] = [(k+1)][N] the private functional packing key switch of LWE t under key block k (what fheaes_pfpks_batch writes at
 * out[t][k]; the body goes through the gadget like the mask), in wrapping uint64 arithmetic:
 *   packed[g] = sum over i < N with gN + i < m of X^i * ks[gN + i],
 * negacyclic in each of the k+1 polynomials (coefficient c of X^i * P is P[c - i] for c >= i and -P[c - i + N] for c < i).  Bit t of the
 * flattened input lives in GLWE t / N, coefficient t % N (four AES blocks fill one GLWE); the coefficients of a partly filled last GLWE
 * beyond m are encryptions of zero.  Unpacking is sample extraction of coefficient i = t % N -- for polynomial j < k mask word
 * jN + c = A_j[i - c] (c <= i) or -A_j[i - c + N] (c > i), body = B[i] -- an LWE ciphertext of bit t under the big key (the GLWE key
 * flattened), a valid input of every entry point.
 *
 * Noise: packing adds an error of variance
 *   sigma^2 = N (kN+1) L (B^2 / 12) sigma_pfks^2 + (kN/2 + 1) 2^(2R) / 12,   B = 2^pfks_base_log, L = pfks_level, R = 64 - L pfks_base_log,
 * sigma_pfks = pfks_noise_std * 2^64: std 2^33.5 at PARAM_OPT against a decoding margin of 2^62; unpacking adds none.  Words carry no
 * noise metadata: an unpacked word counts as NOMINAL for the noise guard above, like any state a caller passes in. */
/* words of the packed form of m bits: ceil(m / N) * (k+1) * N; 0 for a NULL context */
size_t fheaes_packed_words(const fheaes_ctx *ctx, uint64_t m);
/* lwe_in [m][kN+1] -> glwe_out [ceil(m/N)][(k+1)N].  Needs uploaded keys (FHEAES_ERR_NOKEYS); m = 0 is FHEAES_OK; overlapping buffers
 * are FHEAES_ERR_INVALID; FHEAES_DEVICE calls only enqueue.  Works in chunks inside the workspace K3 owns (fheaes_reserve bounds it). */
int fheaes_pack_bits(fheaes_ctx *ctx, const uint64_t *lwe_in, uint64_t m, uint64_t *glwe_out, int memspace);
/* glwe_in [ceil(m/N)][(k+1)N] -> lwe_out [m][kN+1]: a permutation with signs, no keys needed.  Same argument rules. */
int fheaes_unpack_bits(fheaes_ctx *ctx, const uint64_t *glwe_in, uint64_t m, uint64_t *lwe_out, int memspace);

/* ---- wire formats --------------------------------------------------------------- */
/* Everything above is sized for compute: a client sends kN + 1 words (16,392 bytes at PARAM_OPT) per bit, 2,098,176 bytes for one AES-128
 * key, and a packed result is 64-bit words.  Two compact forms for the wire, one per direction; nothing above changes.
 *
 * SEEDED LWE CIPHERTEXTS (client -> server).  kN of the kN + 1 words of a fresh LWE ciphertext are a uniformly random mask, public by
 * construction.  A list of m seeded ciphertexts is (mask_key: a PUBLIC 256-bit key, uint32[8]; first_index: uint64; bodies: uint64[m]).
 * Ciphertext t expands to [ mask(first_index + t) | bodies[t] ]: mask word j < kN of ciphertext q is 64-bit word j % 8 of the RFC 8439
 * block j / 8 under (mask_key, nonce = (6, q low 32, q high 32)) -- the stream of fheaes_upload_keys_seeded with the tag MASK_TAG_LWE = 6
 * (csrc/client.c).  8 bytes per bit instead of 16,392; one AES-128 key is 128 x 8 + 40 = 1,064 bytes instead of 2 MB; 65,536 AES keys
 * are 67.1 MB instead of 137.5 GB.  An expanded ciphertext is an ordinary LWE under the big key, a legal input of every entry point.
 *   THE RULE THE CLIENT KEEPS: a (mask_key, index) pair is used for ONE ciphertext only, under ONE secret key.  Two ciphertexts with the
 *   same mask differ by their messages and noises alone (b - b' = (m - m') 2^63 + e - e'), which gives the message difference away.  The
 *   Python Client draws a fresh mask_key for every seeded encryption call; first_index exists so that one list can be cut into shards
 *   (shard s passes first_index + its offset) and so that a sender may run several lists under one mask_key on disjoint index ranges.
 * The reference has no counterpart (client.rs:123-138 hands full ciphertexts across in memory); in tfhe-rs it is SeededLweCiphertextList.
 *
 * lwe_out[t] = [ mask words of ciphertext first_index + t | bodies[t] ],  t < m;  lwe_out [m][kN+1].
 * mask_key: HOST array of 8 uint32 whatever memspace says (as fheaes_upload_keys_seeded); bodies, lwe_out in memspace.  No keys needed: a
 * context at any parameter set.  m = 0 is FHEAES_OK; overlapping buffers FHEAES_ERR_INVALID; FHEAES_DEVICE calls only enqueue.
 * Accounted under FHEAES_STAGE_LINEAR (units: bits). */
int fheaes_expand_lwe_seeded(fheaes_ctx *ctx, const uint32_t *mask_key, uint64_t first_index, const uint64_t *bodies, uint64_t m,
                             uint64_t *lwe_out, int memspace);

/* MODULUS-SWITCHED PACKED CIPHERTEXTS (server -> client, or to storage).  Width w, 8 <= w <= 32.  A word x of a packed GLWE becomes the
 * w-bit value
 *   v = ((x + 2^(63-w)) >> (64-w)) mod 2^w          (the sum wraps in uint64: words within 2^(63-w) of 2^64 round to 0)
 * and is read back as x' = v << (64-w).  Within GLWE g the word of polynomial j, coefficient c is field e = jN + c, at bits
 * [e w, (e+1) w) of that GLWE's little-endian bit string (bit b of the string = bit b % 64 of word b / 64).  With N = 512 a polynomial is
 * exactly 8 w words; a GLWE is (k+1) 8 w words and starts on a word boundary; the container stays uint64_t.  w = 64 means "not switched":
 * the _mod entry points then give the words of the plain ones.  Any other width is FHEAES_ERR_INVALID.  128 AES blocks at w = 16:
 * 163,840 bytes instead of 655,360 packed (268.6 MB unpacked).
 *
 * Noise: each word moves by at most 2^(63-w), uniformly; the phase of a coefficient moves by a sum over the body and the h set key bits:
 *   variance (1 + h) 2^(2(64-w)) / 12,   hard bound (1 + h) 2^(63-w).
 * At PARAM_OPT (h about 1,024) and w = 16: std 2^51.2, bound 2^57.0 (below 2^58), against a WoPBS output noise of std 2^53.8 (2^54.3 for an AES
 * output word, a fresh output plus a round-key word; derived from the parameter set in tests/noise_model.py, which the tests hold the oracle
 * and the kernels to, eight sigma at most per word) and a decoding
 * margin of 2^62 -- w = 16 cannot flip a bit that was decodable with that room (the default of the Python layer).  Smaller widths are the
 * caller's arithmetic, as summed ciphertexts are for the noise guard; words carry no noise metadata.
 *
 * Argument rules of fheaes_pack_bits / fheaes_unpack_bits: m = 0 or n_glwe = 0 is FHEAES_OK, overlapping buffers FHEAES_ERR_INVALID,
 * FHEAES_ERR_NOKEYS only where packing needs keys, FHEAES_DEVICE calls only enqueue; all under FHEAES_STAGE_LINEAR. */
size_t fheaes_packed_words_mod(const fheaes_ctx *ctx, uint64_t m, uint32_t width);     /* ceil(m/N)(k+1)N width/64; 0 for NULL or a bad width */
/* 64-bit packed GLWEs [n_glwe][(k+1)N] -> [n_glwe][(k+1) 8 width]: no keys */
int fheaes_packed_mod_switch(fheaes_ctx *ctx, const uint64_t *glwe_in, uint64_t n_glwe, uint32_t width, uint64_t *out, int memspace);
/* fheaes_pack_bits followed by the switch: word for word fheaes_packed_mod_switch(fheaes_pack_bits(..)); each chunk's 64-bit GLWEs are
 * staged in workspace the context owns (at most 64 GLWEs).  Like fheaes_pack_bits' own workspace it is grown, with a stream
 * synchronisation, by the first call that needs more of it than any call before (a larger m, up to one chunk); from then on a
 * FHEAES_DEVICE call only enqueues. */
int fheaes_pack_bits_mod(fheaes_ctx *ctx, const uint64_t *lwe_in, uint64_t m, uint32_t width, uint64_t *out, int memspace);
/* sample extraction straight from the w-bit fields: word for word fheaes_unpack_bits of the read-back GLWEs (x' = v << (64-w)) */
int fheaes_unpack_bits_mod(fheaes_ctx *ctx, const uint64_t *in, uint64_t m, uint32_t width, uint64_t *lwe_out, int memspace);

/* ---- packed round keys --------------------------------------------------------- */
/* The round keys are what a server keeps between requests, and in LWE form they are the fat object: [Nr+1][16][8][kN+1] is 23,079,936 /
 * 27,276,288 / 31,472,640 bytes per AES-128 / 192 / 256 key at PARAM_OPT, 1.51 TB for FHEAES_MAX_KEYS AES-128 keys.  Packed, key i of a
 * store is packed[i] = [G][(k+1)N] words, G = ceil((Nr+1) 128 / N) = 3 / 4 / 4 GLWEs: 61,440 / 81,920 / 81,920 bytes (375.6 / 333.0 /
 * 384.2 times smaller), 4.03 GB for 65,536 AES-128 keys.  packed[i] is WORD FOR WORD what fheaes_pack_bits writes for slice i of the round
 * keys flattened, m = (Nr+1) 128 bits: bit t = round * 128 + byte * 8 + bit (LSB first) lives in GLWE t / N, coefficient t % N; every key
 * starts on a GLWE boundary, so a slice is a packed key set on its own (store, send, concatenate, shard it without its neighbours); the
 * unused coefficients of a key's last GLWE are what fheaes_pack_bits leaves there (sums of nothing).  Decryption round keys
 * (fheaes_aes_decryption_round_keys*) have the same shape and pack the same way; the caller knows which kind it holds, as with the LWE
 * form.  64-bit words only.
 *
 * The *_keyed_packed calls read every round-key word from the store at the moment AddRoundKey needs it -- sample extraction of
 * coefficient t % N (fheaes_unpack_bits' rule: a signed, reversed read of one polynomial per mask run) inside the linear layers -- so a
 * key never exists in LWE form again once it is packed.  No new arithmetic: the words they write are, word for word, what the _keyed call
 * writes when given fheaes_unpack_round_keys of the same store.
 *
 * Noise: a key word read from the packed form carries the key's noise plus the packing's (std 2^33.5 at PARAM_OPT against a nominal
 * 2^53.8, the WoPBS output noise of tests/noise_model.py); it counts as NOMINAL for the noise guard, exactly as fheaes_unpack_bits outputs do, and the guard sees the counts of the
 * unpacked schedules.  All of it is accounted under FHEAES_STAGE_LINEAR, the packing's matrix product under FHEAES_STAGE_PFPKS. */
/* G: 3 / 4 / 4 for key_bits 128 / 192 / 256, 0 for anything else (host logic only, no context, no GPU) */
uint32_t fheaes_round_keys_packed_glwes(uint32_t key_bits);
/* round_keys [n_keys][Nr+1][16][8][kN+1] -> packed_out [n_keys][G][(k+1)N].  The K3 product runs over chunks of whole keys inside the
 * workspace fheaes_pack_bits uses, the fold places each key's bits from its own GLWE boundary.  Needs uploaded keys (FHEAES_ERR_NOKEYS);
 * n_keys as for the keyed calls; overlapping buffers are FHEAES_ERR_INVALID; FHEAES_DEVICE calls only enqueue. */
int fheaes_pack_round_keys(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *packed_out, int memspace);
/* keys first_key .. first_key + n_keys of the store `packed` -> round_keys_out [n_keys][Nr+1][16][8][kN+1], slice j word for word
 * fheaes_unpack_bits of packed[first_key + j].  No keys needed.  For migration, and the reference of the tests.  Only those keys' words
 * are read.  Overlapping buffers are FHEAES_ERR_INVALID. */
int fheaes_unpack_round_keys(fheaes_ctx *ctx, const uint64_t *packed, uint32_t key_bits, uint64_t first_key, uint64_t n_keys,
                             uint64_t *round_keys_out, int memspace);
/* fheaes_aes_encrypt_keyed / _decrypt_keyed / _decrypt_equivalent_keyed / fheaes_aes_public_keyed / _decrypt_public_keyed with a packed store
 * [n_keys][G][(k+1)N] in place of round_keys.  The rules of their counterparts (key_of_block a HOST array, an entry >= n_keys
 * FHEAES_ERR_INVALID, n_blocks = 0 FHEAES_OK, FHEAES_DEVICE only enqueues, the same windows), and a store that overlaps the state is
 * FHEAES_ERR_INVALID.  One key (n_keys = 1, key_of_block all 0) serves where a single-key call would. */
int fheaes_aes_encrypt_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys,
                                    const uint32_t *key_of_block, uint64_t *state, uint64_t n_blocks, int memspace);
int fheaes_aes_decrypt_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys,
                                    const uint32_t *key_of_block, uint64_t *state, uint64_t n_blocks, int memspace);
int fheaes_aes_decrypt_equivalent_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keys,
                                               const uint32_t *key_of_block, uint64_t *state, uint64_t n_blocks, int memspace);
int fheaes_aes_public_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys,
                                   const uint32_t *key_of_block, const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo, uint64_t n_blocks,
                                   uint64_t *state_out, int memspace);
int fheaes_aes_decrypt_public_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keys,
                                           const uint32_t *key_of_block, const uint64_t *blocks_hi_lo, const uint64_t *data_hi_lo,
                                           uint64_t n_blocks, uint64_t *state_out, int memspace);

/* ---- CBC-MAC chains and CCM decryption with its tag check --------------------------- */
/* A CBC-MAC X_{i+1} = E_K(X_i ^ B_i) is block encryptions and XORs only, so -- unlike GHASH, a product of encrypted field elements -- it
 * stays inside the noise budget: the first integrity result of the engine.  It is serial inside a stream and parallel across streams:
 * the streams are sorted by chain length (descending, stable), step i of all live streams is ONE windowed cipher pass over a prefix of
 * one state array, and one K6 launch (mac_link_kernel) links two passes.  Levels against FHEAES_MAX_NOISE_LEVEL = 5: a cipher or
 * public-call output is 2; a link of public blocks enters AddRoundKey at 3; a link with an encrypted addend at X (2) + P (2) + round key
 * = 5; the tag difference is 4; a caller's `enc` or `init` is counted as 2.
 *
 * Bounds: n_keys <= FHEAES_MAX_KEYS, n_streams <= FHEAES_MAC_MAX_STREAMS, a stream chains at most FHEAES_MAC_MAX_STREAM_BLOCKS blocks.
 * Refused with FHEAES_ERR_INVALID before anything is launched: a NULL argument that is not optional, overlapping in and out buffers, a
 * count above its bound, a key index >= n_keys, enc_bytes > 16, and for CCM a tag length outside {4, 6, .., 16} or flags bytes that do
 * not describe a 7..13-byte nonce.  n_streams = 0 is FHEAES_OK and writes nothing; FHEAES_DEVICE calls only enqueue. */
#define FHEAES_MAC_MAX_STREAMS (1u << 20)
#define FHEAES_MAC_MAX_STREAM_BLOCKS (1u << 16)
#define FHEAES_MAC_NONE 0xFFFFFFFFu
/* mac_out[s] = X after stream s's stream_blocks[s] blocks, X_0 = init[s] (or zero), X_{i+1} = E_{K[key_of_stream[s]]}(X_i + block i), where
 * block i = trivial(clear[b]) + the first enc_bytes[b] bytes of enc[b], b the block's index in the call (stream after stream, the caller's
 * order).  round_keys [n_keys][Nr+1][16][8][kN+1]; key_of_stream, stream_blocks: HOST arrays of n_streams; clear: HOST bytes [blocks][16];
 * enc [blocks][16][8][kN+1] with enc_bytes (HOST, [blocks], 0..16), both or neither; init [n_streams][16][8][kN+1] or NULL;
 * mac_out [n_streams][16][8][kN+1].  A stream of 0 blocks yields its init (zero words without one).  Word for word: per step,
 * fheaes_aes_encrypt_keyed on the wrapping sums of the live streams in sorted order. */
int fheaes_aes_cbc_mac_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                             const uint32_t *key_of_stream, const uint32_t *stream_blocks, const uint8_t *clear, const uint64_t *enc,
                             const uint8_t *enc_bytes, const uint64_t *init, uint64_t *mac_out, int memspace);
/* The same with the keys in a packed store (fheaes_pack_round_keys). */
int fheaes_aes_cbc_mac_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                                    const uint32_t *key_of_stream, const uint32_t *stream_blocks, const uint8_t *clear, const uint64_t *enc,
                                    const uint8_t *enc_bytes, const uint64_t *init, uint64_t *mac_out, int memspace);
/* AES-CCM decryption (SP 800-38C, RFC 3610) of n_streams PUBLIC messages, each under the encrypted key key_of_stream[s], with the tag
 * compared under encryption.  The caller formats (SP 800-38C A.2, A.3); this call sees blocks, every clear block as (hi, lo) with byte 0
 * the most significant byte of hi.  Per stream: head_blocks[s] = 1 + a blocks in head_hi_lo (B0, then the encoded, zero-padded AAD
 * blocks), stream after stream; Ctr_0 in ctr0_hi_lo (its counter field zero: Ctr_i is Ctr_0 + i); payload_bytes[s] bytes of `ciphertext`
 * (stream after stream, no padding); the received tag in tags[s][16], its first tag_bytes[s] = t bytes.  All of these are HOST arrays.
 *   (a) one public call over [Ctr_1.. | B0 | Ctr_0] with data [C_1.. | 0 | 0] yields the plaintext blocks P, X_1 and S0;
 *   (b) the CBC-MAC runs from X_1 over the a AAD blocks, then over the payload blocks with the encrypted P as addend, the last one with
 *       its real bytes only; a stream with a = 0 and no payload has MAC X_1;
 *   (c) diff = X_final + S0 + trivial(tag) on its first 8t rows, zero words beyond;
 *   (d) one 8-bit WoPBS per byte of diff (LUT: byte != 0), then one 16-bit WoPBS per stream over those 16 bits (LUT: 1 on input 0).
 * plaintext_out [sum of ceil(payload_bytes / 16)][16][8][kN+1], stream after stream, rows beyond a payload's length zero words (may be
 * NULL when no stream has a payload); valid_out [n_streams][kN+1], row 0 of (d): an encryption of 1 iff the tag is right.  The plaintext is
 * NOT gated on valid_out: a caller that releases it does so after reading the bit, or gates it first (fheaes_gate_bits). */
int fheaes_aes_ccm_open_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                              const uint32_t *key_of_stream, const uint32_t *head_blocks, const uint64_t *head_hi_lo, const uint64_t *ctr0_hi_lo,
                              const uint64_t *payload_bytes, const uint8_t *ciphertext, const uint8_t *tags, const uint32_t *tag_bytes,
                              uint64_t *plaintext_out, uint64_t *valid_out, int memspace);
int fheaes_aes_ccm_open_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t n_streams,
                                     const uint32_t *key_of_stream, const uint32_t *head_blocks, const uint64_t *head_hi_lo,
                                     const uint64_t *ctr0_hi_lo, const uint64_t *payload_bytes, const uint8_t *ciphertext, const uint8_t *tags,
                                     const uint32_t *tag_bytes, uint64_t *plaintext_out, uint64_t *valid_out, int memspace);
/* K6 alone, one link of a chain (needs no keys): state[s] = (first ? (init ? init[s] : 0) : state[s]) + the first enc_bytes[s] bytes of
 * enc[src_block[s]] (src_block[s] == FHEAES_MAC_NONE, or enc NULL: none) + trivial(clear[s]), for s < n_slots.  state, init
 * [n_slots][16][8][kN+1]; enc [n_enc][16][8][kN+1]; src_block, enc_bytes, clear ([n_slots][16]): HOST arrays.  Declares to the noise guard
 * what the link declares inside a chain (the level of the sum plus the round key that follows). */
int fheaes_mac_link(fheaes_ctx *ctx, uint64_t *state, uint64_t n_slots, int first, const uint64_t *init, const uint64_t *enc, uint64_t n_enc,
                    const uint32_t *src_block, const uint8_t *enc_bytes, const uint8_t *clear, int memspace);
/* K6 alone, the XTS whitening (needs no keys): dst[b] = (src ? src[b] : 0) + tweaks[tweak_of_block[b]] + trivial(clear[b]), b < n_blocks;
 * dst, src [n_blocks][16][8][kN+1] (src == dst: in place; NULL: none), tweaks [n_tweaks][16][8][kN+1], tweak_of_block (HOST, entries below
 * n_tweaks), clear (HOST, [n_blocks][16], or NULL).  Declared to the noise guard as 3 with a src, 2 without.  The yardstick the link
 * kernel is timed against (tools/ccm.py): the same traffic per output word. */
int fheaes_xts_whiten(fheaes_ctx *ctx, uint64_t *dst, const uint64_t *src, const uint64_t *tweaks, uint64_t n_tweaks, const uint32_t *tweak_of_block,
                      const uint8_t *clear, uint64_t n_blocks, int memspace);
/* What a chain over streams of stream_blocks[s] blocks runs (host logic only): *steps cipher passes, n_active_out[i] live streams in pass i
 * (n_active_out may be NULL; else n_active_cap >= *steps), *chained_blocks = their sum.  payload_blocks (NULL for a plain CBC-MAC): of a
 * CCM stream's chain, how many blocks are payload; *public_blocks = 2 n_streams + their sum, the blocks of the CCM public call (0 for NULL). */
int fheaes_aes_mac_plan(const uint32_t *stream_blocks, const uint32_t *payload_blocks, uint64_t n_streams, uint64_t *steps, uint64_t *n_active_out,
                        uint64_t n_active_cap, uint64_t *public_blocks, uint64_t *chained_blocks);

/* ---- CMAC --------------------------------------------------------------------------------- */
/* AES-CMAC (SP 800-38B, RFC 4493) of PUBLIC messages under encrypted keys: the MIC of LoRaWAN, AUTOSAR SecOC, the OMAC of EAX, the S2V of
 * SIV, CTR + CMAC as encrypt-then-MAC.  A CMAC is the CBC-MAC above whose last block also gets a subkey added: K1 = L x under a whole
 * last block, K2 = L x^2 under one padded with 0x80 00.., in GF(2^128) mod x^128 + x^7 + x^2 + x + 1 with L = E_K(0^128).  All blocks
 * are public, so no decryption precedes the tag check.  Levels against FHEAES_MAX_NOISE_LEVEL = 5: L leaves the public call at 2 and an
 * identity WoPBS makes it 1; one gather gives K1 at 2 and K2 at 3; a second identity WoPBS makes both 1, counted as a chain counts every
 * encrypted addend, 2: the last link is X (2) + subkey (2) + round key = 5, the tag difference 2.  Both refreshes are needed: a raw K2
 * from a raw L would be 2 * 3, an unrefreshed K2 from a refreshed L 2 + 3 + 1 = 6.  48 byte-WoPBS per key, against 16 Nr per chained block.
 *
 * Bounds and refusals as in the section above: a NULL argument that is not optional, overlapping in and out buffers, a count above its
 * bound, a key index >= n_keys, a tag length outside 4..16, key_bits not 128 / 192 / 256 and a message of more than
 * 16 * FHEAES_MAC_MAX_STREAM_BLOCKS bytes are FHEAES_ERR_INVALID before anything is launched, and the outputs are untouched.
 * n_streams = 0 is FHEAES_OK and writes nothing; FHEAES_DEVICE calls only enqueue. */
/* The sources of output bit `bit` (flattened [16][8] index: byte p, bit b LSB first, is 8p + b -- degree 8 (15 - p) + b of the field
 * element, where XTS has 8p + b) of L x^(which + 1), which = 0: K1, 1: K2.  At most 2 and 3 distinct sources; sources_out has room for 3.
 * Host logic only.  which > 1 or bit > 127: FHEAES_ERR_INVALID. */
int fheaes_cmac_subkey_row(uint32_t which, uint32_t bit, uint32_t *sources_out, uint32_t *n_sources);
/* K6 alone, the raw gather (needs no keys): out[key][which][i] = the wrapping sum over fheaes_cmac_subkey_row(which, i) of l[key][source].
 * l [n_keys][128][kN+1], out [n_keys][2][128][kN+1], both subkeys of all keys from one launch.  Declares row weight 3 to the noise guard. */
int fheaes_cmac_double(fheaes_ctx *ctx, const uint64_t *l, uint64_t n_keys, uint64_t *out, int memspace);
/* subkeys_out [n_keys][2][16][8][kN+1]: K1 and K2 of every key.  Word for word: fheaes_aes_public_keyed on one zero block per key, the
 * identity WoPBS on its 16 n_keys bytes, fheaes_cmac_double, the identity WoPBS on its 32 n_keys bytes. */
int fheaes_aes_cmac_subkeys_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, uint64_t *subkeys_out,
                                  int memspace);
int fheaes_aes_cmac_subkeys_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys,
                                         uint64_t *subkeys_out, int memspace);
/* The CMAC of n_streams public messages, stream s under key key_of_stream[s], and -- with tags -- its comparison under encryption.
 * subkeys: what fheaes_aes_cmac_subkeys_keyed gave for these keys, or NULL: they are derived here, only for the keys some stream names,
 * and the words do not depend on which.  HOST arrays: key_of_stream, message_bytes, data (the messages' bytes, stream after stream, no
 * padding; may be NULL when every message is empty), tags [n_streams][16] with tag_bytes [n_streams] (the first t = 4..16 bytes of the
 * tag are compared), or both NULL.
 *   (a) the blocks: n = max(1, ceil(bytes / 16)); a last block that is whole takes K1, else it is padded with 0x80 00.. and takes K2
 *       (the empty message: one block 0x80 00.. with K2);
 *   (b) fheaes_aes_cbc_mac_keyed with those blocks as `clear`, each stream's last block carrying its subkey as `enc` with enc_bytes = 16
 *       (0 elsewhere), init NULL;
 *   (c) with tags, diff = X + trivial(tag) on its first 8t rows, zero words beyond;
 *   (d) the two comparison WoPBS of fheaes_aes_ccm_open_keyed's step (d) on diff.
 * mac_out [n_streams][16][8][kN+1]: the full T of every stream (truncation is the caller's); required without tags, may be NULL with them.
 * valid_out [n_streams][kN+1]: an encryption of 1 iff the tag is right; required with tags, must be NULL without them.  EAX's OMAC^t is
 * this CMAC over [t]_128 || M and needs nothing more. */
int fheaes_aes_cmac_keyed(fheaes_ctx *ctx, const uint64_t *round_keys, uint32_t key_bits, uint64_t n_keys, const uint64_t *subkeys,
                          uint64_t n_streams, const uint32_t *key_of_stream, const uint64_t *message_bytes, const uint8_t *data,
                          const uint8_t *tags, const uint32_t *tag_bytes, uint64_t *mac_out, uint64_t *valid_out, int memspace);
int fheaes_aes_cmac_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_round_keys, uint32_t key_bits, uint64_t n_keys, const uint64_t *subkeys,
                                 uint64_t n_streams, const uint32_t *key_of_stream, const uint64_t *message_bytes, const uint8_t *data,
                                 const uint8_t *tags, const uint32_t *tag_bytes, uint64_t *mac_out, uint64_t *valid_out, int memspace);
/* What a CMAC call over messages of these lengths runs (host logic only): *steps cipher passes, *chained_blocks cipher blocks in all,
 * *padded_streams streams whose last block takes K2. */
int fheaes_aes_cmac_plan(const uint64_t *message_bytes, uint64_t n_streams, uint64_t *steps, uint64_t *chained_blocks, uint64_t *padded_streams);

/* ---- AES key unwrap ----------------------------------------------------------------------- */
/* The AES Key Unwrap of RFC 3394 / SP 800-38F (JWE's A128KW / A256KW, CMS, PKCS#11 CKM_AES_KEY_WRAP, KMIP) under encrypted
 * key-encryption keys (KEKs): wrapped keys -- PUBLIC data, 8 (n + 1) bytes for a payload of n semiblocks of 8 bytes -- in, the encrypted
 * payloads and an encrypted `valid` bit per key out.  The owner sends each KEK under FHE once; after that session keys come straight
 * from the key store and go into fheaes_aes_key_expansion_batch.  With C[0..n] the wrapped semiblocks, step s = 0 .. 6n - 1 works on
 * register i_s = n - s % n under the counter t_s = 6n - s:  B = D_KEK((A ^ t_s) | R[i_s]), A = MSB64(B), R[i_s] = LSB64(B), from
 * A = C[0], R[i] = C[i]; the payload is R[1..n], valid iff A == A6A6A6A6A6A6A6A6.  Serial inside a key and parallel across keys: step s of
 * ALL keys is one K6 launch (kw_link_kernel) and one windowed pass of the equivalent inverse cipher.  Levels against
 * FHEAES_MAX_NOISE_LEVEL = 5: a cipher output is 2, a step's input enters AddRoundKey at 3, the raw payload is 2 and an identity WoPBS
 * makes it fresh; the difference A + A6.. enters the tag check at 2.
 *
 * Bounds: 2..8 semiblocks (payloads of 16..64 bytes: AES keys of all three sizes, XTS key pairs, HMAC keys), one value per call; at most
 * FHEAES_KW_MAX_KEYS keys per call (a key takes 2.1 MB of state at PARAM_OPT and 1.05 MB per semiblock twice over, registers and output:
 * 4,096 keys of 8 semiblocks are about 77 GB beside the evaluation keys).  Refused with FHEAES_ERR_INVALID before anything is launched,
 * the outputs untouched: a NULL argument that is not optional, semiblocks outside 2..8, n_keys > FHEAES_KW_MAX_KEYS, n_keks outside
 * 1..FHEAES_MAX_KEYS, a KEK index >= n_keks, key_bits not 128 / 192 / 256, step > 6 semiblocks, overlapping buffers.  n_keys = 0 is
 * FHEAES_OK and writes nothing; FHEAES_DEVICE calls only enqueue.  Out: RFC 5649 padding (KWP), wrapping, mixed payload lengths in one
 * call, payloads above 64 bytes.  Gating the payload on `valid`: fheaes_gate_bits below. */
#define FHEAES_KW_MIN_SEMIBLOCKS 2
#define FHEAES_KW_MAX_SEMIBLOCKS 8
#define FHEAES_KW_MAX_KEYS 4096
/* dec_round_keys: what fheaes_aes_decryption_round_keys_batch gave for the n_keks KEKs (AES-key_bits); kek_of_key: HOST [n_keys], the KEK of
 * every wrapped key, may be NULL when n_keks == 1; wrapped: HOST bytes [n_keys][8 (semiblocks + 1)].  keys_out [n_keys][8 semiblocks][8][kN+1]:
 * the payloads, fresh ciphertexts in the layout fheaes_aes_key_expansion_batch takes, NOT gated on valid_out; valid_out [n_keys][kN+1]: an
 * encryption of 1 iff the integrity constant is right.  Word for word: for s = 0 .. 6n - 1, fheaes_kw_link(s) and
 * fheaes_aes_decrypt_equivalent_keyed on the n_keys states under kek_of_key; fheaes_kw_link(6n); fheaes_wopbs_batch with the identity LUT
 * on the 8 n n_keys bytes of regs; step (d) of fheaes_aes_ccm_open_keyed on the state. */
int fheaes_aes_kw_unwrap_keyed(fheaes_ctx *ctx, const uint64_t *dec_round_keys, uint32_t key_bits, uint64_t n_keks, uint64_t n_keys,
                               const uint32_t *kek_of_key, uint32_t semiblocks, const uint8_t *wrapped, uint64_t *keys_out, uint64_t *valid_out,
                               int memspace);
int fheaes_aes_kw_unwrap_keyed_packed(fheaes_ctx *ctx, const uint64_t *packed_dec_round_keys, uint32_t key_bits, uint64_t n_keks, uint64_t n_keys,
                                      const uint32_t *kek_of_key, uint32_t semiblocks, const uint8_t *wrapped, uint64_t *keys_out,
                                      uint64_t *valid_out, int memspace);
/* K6 alone, one link of the unwrap (needs no keys), step = 0 .. 6 semiblocks.  state [n_keys][16][8][kN+1]: A on rows 0..63, the register
 * at work on rows 64..127; regs [n_keys][8 semiblocks][8][kN+1]: register i on bytes 8 (i-1) .. 8 i - 1.
 *   step 0 (load):      regs = trivial(C[1..n]), state = trivial(C[0] ^ t_0) | trivial(C[n]); `wrapped` (HOST) is read here alone and may be
 *                       NULL otherwise
 *   0 < step < 6n:      regs[i_{step-1}] <- state rows 64..127 <- regs[i_step]; state rows 0..63 += trivial(t_step)
 *   step 6n (unload):   regs[1] <- state rows 64..127 <- zero words; state rows 0..63 += trivial(A6 x 8)
 * In place.  Declares to the noise guard the level of the sum plus the round key that follows: 1, 3 and 2. */
int fheaes_kw_link(fheaes_ctx *ctx, uint64_t *state, uint64_t *regs, uint64_t n_keys, uint32_t semiblocks, uint32_t step, const uint8_t *wrapped,
                   int memspace);
/* What an unwrap call runs (host logic only): *steps = 6 n cipher passes, *cipher_blocks = 6 n n_keys, *byte_wopbs = 16 Nr 6 n n_keys (the
 * cipher) + 8 n n_keys (the refresh of the payload) + 16 n_keys (the first WoPBS of the tag check). */
int fheaes_aes_kw_plan(uint32_t key_bits, uint32_t semiblocks, uint64_t n_keys, uint64_t *steps, uint64_t *cipher_blocks, uint64_t *byte_wopbs);

/* ---- the gate: ciphertexts times an encrypted bit ----------------------------------------- */
/* SP 800-38C and RFC 3394 forbid releasing a plaintext or a key whose check failed, and a server under FHE cannot branch on `valid`: it
 * multiplies the result by `valid` under encryption.  The gate is one single-level external product with a zero "else" branch,
 * out = GGSW(g) (x) in, in the circuit bootstrap's gadget (base 2^15, one level): one circuit bootstrap (K1, K2, K3, K4) per GATE and one
 * external product per ciphertext (gate_kernel, kern_gate.h), where the composition of older calls -- a 9-bit WoPBS per byte with the bit
 * as ninth input -- costs nine circuit bootstraps per BYTE.  Two forms: LWE ciphertexts [m][kN+1], each embedded on load into the GLWE
 * whose coefficient 0 it is and extracted again on store, and packed GLWEs [G][(k+1)N] of fheaes_pack_bits, 512 bits per product.
 *
 * Runs: bits_of_gate (HOST, n_gates entries) says how many CONSECUTIVE ciphertexts (GLWE form: GLWEs) each gate multiplies; a gate of 0
 * is allowed; the runs must add up to m.  In place (out == in) is allowed: every ciphertext is read before it is written, by the one
 * workgroup that owns it.  Refused with FHEAES_ERR_INVALID before anything is launched, the outputs untouched: a NULL context or a NULL
 * argument of a call with m > 0, runs that do not add up to m, a form other than 0 / 1, n_gates >= 2^32, `out` overlapping `in` without
 * being `in`, `out` overlapping the gates or GGSWs.  m = 0 is FHEAES_OK and writes nothing; FHEAES_DEVICE calls only enqueue.
 * FHEAES_ERR_NOKEYS: the two calls that bootstrap, without evaluation keys.  Kernel time is accounted under
 * FHEAES_STAGE_VERTICAL_PACKING (units: bits, or GLWEs x N for the GLWE form).
 *
 * Noise: words carry no level between calls and the noise guard counts linear layers only, so fheaes_noise_level_seen is unaffected.
 * The rule for a caller's own count: a gated ciphertext KEEPS THE LEVEL OF ITS INPUT.  What a gate adds is derived in tests/gate_model.py
 * and measured in tests/test_gpu_gate.py: the rounding of the input to 15 bits (zero under a gate of 0) plus
 * (k+1) N digits times a GGSW row, no more than one of the eight or more CMUX iterations every WoPBS output already carries.
 * Out: a select between two arrays, gating on the negation of a bit, modulus-switched packed input (gate before
 * fheaes_packed_mod_switch), keeping a gate's GGSW from call to call. */
#define FHEAES_GATE_LWE 0
#define FHEAES_GATE_GLWE 1
/* The kernel alone, on caller-made Fourier GGSWs [n_gates][1][k+1][k+1][256][2] -- the layout fheaes_vertical_packing_batch takes, e.g.
 * the four stage calls on the bits.  Needs no keys.  form FHEAES_GATE_LWE: in / out [m][kN+1]; FHEAES_GATE_GLWE: [m][(k+1)N].  A caller
 * who gates several arrays on the same bits bootstraps them once and calls this for each. */
int fheaes_gate_ggsw(fheaes_ctx *ctx, const double *ggsw_fourier, uint64_t n_gates, const uint64_t *bits_of_gate, const uint64_t *in, uint64_t m,
                     int form, uint64_t *out, int memspace);
/* gates_lwe [n_gates][kN+1]: encryptions of 0 / 1 at the bit encoding (a `valid_out`).  Word for word: fheaes_keyswitch_batch,
 * fheaes_cbs_pbs_batch at level 1, fheaes_pfpks_batch and fheaes_forward_fourier_batch on the gates, then fheaes_gate_ggsw -- the front
 * half of a WoPBS, in its workspaces, the gates cut into chunks of 32,768 by its rule (a chunk's runs are gated before the next chunk's
 * GGSWs replace it). */
int fheaes_gate_bits(fheaes_ctx *ctx, const uint64_t *gates_lwe, uint64_t n_gates, const uint64_t *bits_of_gate, const uint64_t *lwe_in, uint64_t m,
                     uint64_t *lwe_out, int memspace);
/* The same on packed GLWEs: glwes_of_gate counts GLWEs, glwe_in / glwe_out [n_glwe][(k+1)N]. */
int fheaes_gate_packed(fheaes_ctx *ctx, const uint64_t *gates_lwe, uint64_t n_gates, const uint64_t *glwes_of_gate, const uint64_t *glwe_in,
                       uint64_t n_glwe, uint64_t *glwe_out, int memspace);
/* The grid a gate call launches (host logic only): *instances_per_workgroup = R, the largest R with R (k+1) <= 16 lane groups that the
 * kernels are built for (3 at k = 4, 8 at k = 1); *workgroups = the sum over the gates of ceil(run / R) -- workgroups never mix gates.
 * k other than 4 or 1, or a NULL argument: FHEAES_ERR_INVALID. */
int fheaes_gate_plan(const uint64_t *bits_of_gate, uint64_t n_gates, uint32_t k, uint64_t *workgroups, uint32_t *instances_per_workgroup);

/* ---- audit --------------------------------------------------------------------- */
/* A server holds no secret key and cannot decrypt what it computed: a wrong word leaves the engine as a well-formed ciphertext.  The audit
 * is the check it can run.  The engine is deterministic and every blind-rotation form writes the same words, so S sampled rows of a
 * blind-rotation launch are run again through the latency form (kern_blindrot_latency.h: it parks nothing and shares no slot pool, owner
 * words or generation plan with the throughput forms) and compared on the device, bit for bit.  A difference is a defect of the engine or
 * of the machine, never noise.  Off by default; these four calls cover the blind rotation, the
 * section after them the two key switches (DESIGN.md says what is caught and what is not).
 * None of these calls takes data arrays or a memspace.
 *
 * fheaes_audit_set: `rows` = 0 (default) turns the audit off and frees its buffers; `rows` in 1..FHEAES_AUDIT_MAX_ROWS (one latency-form
 * workgroup per row) turns it on: every blind-rotation launch of this context of m >= `min_bits` bits -- the WoPBS of every call, the
 * gate, fheaes_cbs_pbs_batch -- is then audited on S = min(rows, m) rows, behind the launch on the same stream; the host waits for nothing
 * and FHEAES_DEVICE calls still only enqueue.  Takes the context's lock, synchronises its stream, allocates the audit's buffers (an audited
 * call never allocates; they are state that persists by design, like the parking owner words, and not among the FHEAES_WS_BUFFERS), zeroes
 * the counters and the launch number, and drops a pending fheaes_audit_debug.  With profiling on the audit's time counts into
 * FHEAES_STAGE_BLIND_ROTATE's total_ms; `launches` and `units` count the product launch only.  Per context, like fheaes_k2_set_forms.
 * `rows` > FHEAES_AUDIT_MAX_ROWS or a NULL context: FHEAES_ERR_INVALID. */
#define FHEAES_AUDIT_MAX_ROWS 256
#define FHEAES_AUDIT_RECORDS 16
int fheaes_audit_set(fheaes_ctx *ctx, uint32_t rows, uint64_t min_bits, uint64_t seed);
/* Host logic only, no context, no GPU: the S = min(rows, m) rows, ascending, that audited launch number `launch` (0 for the first one after
 * fheaes_audit_set) of m bits checks under `seed`; the kernels compute the same.  Stratified: sample s lies in the stratum
 * [floor(s m / S), floor((s + 1) m / S)) at offset mix(seed, launch, s) mod (stratum length), with
 *   mix(seed, l, s) = sm(sm(seed + l) + s)     and sm = splitmix64, all arithmetic mod 2^64:
 *   sm(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  return x ^ x >> 31
 * So any run of 2 ceil(m / S) - 1 consecutive wrong rows holds a whole stratum and is always caught, and W scattered wrong rows are caught
 * with probability about 1 - (1 - S / m)^W.  m = 0, rows = 0, rows > FHEAES_AUDIT_MAX_ROWS or a NULL `rows_out`: FHEAES_ERR_INVALID. */
int fheaes_audit_rows(uint64_t seed, uint64_t launch, uint64_t m, uint32_t rows, uint64_t *rows_out);
/* Synchronises, then reads the counters since the last fheaes_audit_set: audited launches, rows compared, rows that differed (sticky until
 * the next fheaes_audit_set), and the records of the first FHEAES_AUDIT_RECORDS wrong rows -- `records_out`: [record_cap][5] words or NULL,
 * each {launch, row, first differing word, that word of the product launch, that word of the audit}; `record_n` receives their number.  Any
 * out-pointer may be NULL; a `record_cap` below the number of records is FHEAES_ERR_INVALID.  Audit off: all zero. */
int fheaes_audit_read(fheaes_ctx *ctx, uint64_t *launches, uint64_t *rows_checked, uint64_t *rows_wrong, uint64_t *records_out, uint64_t record_cap,
                      uint64_t *record_n);
/* Test hook, one shot (tests/test_gpu_audit.py): the next audited launch XORs `xor_mask` (non-zero) into word `word` (<= kN) of row `row` of
 * its output, after the product kernel and before the audit, in a one-thread kernel on the stream; a `row` beyond that launch's m drops
 * the hook without a write.  One wrong word in the caller's own result and nothing else.  A zero mask, a word beyond kN or a NULL context:
 * FHEAES_ERR_INVALID. */
int fheaes_audit_debug(fheaes_ctx *ctx, uint64_t row, uint32_t word, uint64_t xor_mask);

/* ---- audit of the key switches ----------------------------------------------------- */
/* The same check for the two integer stages, K1 (the LWE key switch, FHEAES_STAGE_KEYSWITCH) and K3 (the private functional packing key
 * switch, FHEAES_STAGE_PFPKS).  Both are an exact integer matrix product mod 2^64, so any order of evaluation gives the same words: S sampled
 * rows of every launch are computed again by a plain form (kern_audit.h: the digits recomputed from the input words, the key words
 * recombined from the resident byte planes, one 64-bit multiply-add per term -- no matrix cores, no digit planes, no LDS-DMA) and compared
 * on the device, bit for bit.  Each stage has its own rows, seed, counters, records, launch number and hook; the launch number counts that
 * stage's audited launches alone, so the rows the blind rotation's audit samples do not depend on whether the key switches are audited.
 * `stage` = FHEAES_STAGE_BLIND_ROTATE: the first three calls ARE fheaes_audit_set / _read / _debug -- one implementation, one state per
 * stage, and what is said of a call here holds under either name.  Any other stage, a NULL context or `rows` > FHEAES_AUDIT_MAX_ROWS:
 * FHEAES_ERR_INVALID.
 *
 * fheaes_audit_stage_set: as fheaes_audit_set -- `rows` = 0 turns the stage's audit off and frees its buffers (fheaes_destroy frees them
 * too); else every launch of the stage of m >= `min_rows` rows is audited on S = min(rows, m) rows, the rows fheaes_audit_rows(seed,
 * launch, m, rows) names: the WoPBS chunks and round windows of every call, the gate's bootstrap, fheaes_keyswitch_batch,
 * fheaes_pfpks_batch, and the single-block launches of fheaes_pack_bits, fheaes_pack_bits_mod and fheaes_pack_round_keys.  The only place
 * that allocates (the gathered rows of the plain form and the state: two allocations, and the gathered inputs before them for the blind
 * rotation: three; sized for FHEAES_AUDIT_MAX_ROWS whatever `rows` is; refused: FHEAES_ERR_NOMEM and the stage is off); an
 * audited call allocates nothing and the host waits for nothing.  Zeroes the stage's counters and launch number, drops its pending hook.
 * With profiling on the audit's time counts into the stage's total_ms; `launches` and `units` count the product launch only.
 * fheaes_audit_stage_read: as fheaes_audit_read.  A record is {launch, row, word, that word of the product launch, that word of the plain
 * form}; `word` is the offset among the words the launch wrote for the row: the column for K1, z (k+1) N + o for key block z of K3 (o
 * alone in a single-block launch).
 * fheaes_audit_stage_debug: test hook, one shot, as fheaes_audit_debug: the stage's next audited launch XORs `xor_mask` into word `word` of
 * row `row` of its output; a row or a word beyond that launch's drops the hook without a write.  A zero mask or a `word` beyond the
 * stage's widest row (n + 1 words for K1, (k+1)^2 N for K3): FHEAES_ERR_INVALID. */
int fheaes_audit_stage_set(fheaes_ctx *ctx, int stage, uint32_t rows, uint64_t min_rows, uint64_t seed);
int fheaes_audit_stage_read(fheaes_ctx *ctx, int stage, uint64_t *launches, uint64_t *rows_checked, uint64_t *rows_wrong, uint64_t *records_out,
                            uint64_t record_cap, uint64_t *record_n);
int fheaes_audit_stage_debug(fheaes_ctx *ctx, int stage, uint64_t row, uint32_t word, uint64_t xor_mask);
/* Test and tool hook: the plain form alone over all m rows of lwe_in [m][kN+1], in groups of FHEAES_AUDIT_MAX_ROWS rows, no product launch,
 * no workspace, nothing counted under any stage.  DEVICE pointers only (it takes no memspace and stages nothing): it only enqueues on the
 * context's stream, as a FHEAES_DEVICE call does.  `stage` = FHEAES_STAGE_KEYSWITCH: `block` = -1, out [m][n+1] as fheaes_keyswitch_batch
 * writes it.  FHEAES_STAGE_PFPKS: `block` = -1: out [m][k+1][(k+1)N] as fheaes_pfpks_batch writes it; `block` = 0..k: that key block alone,
 * out [m][(k+1)N], as the launch of fheaes_pack_bits (block k).  Another stage or block: FHEAES_ERR_INVALID. */
int fheaes_audit_plain_batch(fheaes_ctx *ctx, int stage, const uint64_t *lwe_in, uint64_t m, int block, uint64_t *out);

/* ---- measurement --------------------------------------------------------------- */
#define FHEAES_STAGE_KEYSWITCH 0
#define FHEAES_STAGE_BLIND_ROTATE 1
#define FHEAES_STAGE_PFPKS 2
#define FHEAES_STAGE_GGSW_FFT 3
#define FHEAES_STAGE_VERTICAL_PACKING 4
#define FHEAES_STAGE_LINEAR 5
#define FHEAES_STAGE_COUNT 6
/* When enabled every kernel launch is bracketed by HIP events on the launch stream.  fheaes_pack_bits accounts its matrix product under
 * FHEAES_STAGE_PFPKS and its fold under FHEAES_STAGE_LINEAR, fheaes_unpack_bits its extraction under FHEAES_STAGE_LINEAR (units: bits);
 * the gate calls account gate_kernel under FHEAES_STAGE_VERTICAL_PACKING. */
int fheaes_profile_enable(fheaes_ctx *ctx, int on);
int fheaes_profile_reset(fheaes_ctx *ctx);
/* synchronises, then returns accumulated kernel time, launches and units (bits or polys) of a stage */
int fheaes_profile_read(fheaes_ctx *ctx, int stage, double *total_ms, uint64_t *launches, uint64_t *units);

/* ---- introspection (parity tests) ---------------------------------------------- */
/* psi^j = exp(i*pi*j/512), j < 512, re/im interleaved: the twiddle table the kernels use */
int fheaes_get_twiddles(double *psi_out);
/* Fourier image of GGSW `i` of the uploaded BSK: out [pbs_level][k+1][k+1][256][2] */
int fheaes_read_bsk_fourier(fheaes_ctx *ctx, uint32_t i, double *out);
/* How a blind-rotation launch of `m` bits is cut into workgroups on a device with `cu_count` compute units at GLWE dimension k
 * (host logic only, no GPU needed, DEVICE-INDEPENDENT: the plan a device takes when every kernel form can be placed on it).
 * `form` 0 = latency form (kern_blindrot_latency.h: one ciphertext per 512-thread workgroup, m <= 256), 1 = 16-form
 * (kern_blindrot16.h: 256-thread workgroups of 3 / 2 ciphertexts, two per CU; 257..768 bits, and every batch at k = 1),
 * 2 = paired form (kern_blindrot_pair.h: ONE 512-thread workgroup per CU carrying 6 / 4 ciphertexts; k = 4, m > 768).
 * `units_main` workgroups of `r_main` ciphertexts are followed by `units_tail` of `r_tail`.  With more workgroups than the device has
 * slots (form 1: two per CU, form 2: one per CU) the counts make the launch a whole number of generations that covers the batch exactly. */
int fheaes_k2_launch_plan(uint64_t m, uint32_t cu_count, uint32_t k, int *form, uint64_t *units_main, uint32_t *r_main,
                          uint64_t *units_tail, uint32_t *r_tail);
/* fheaes_k2_launch_plan for a device whose runtime cannot place the paired kernel (`allow_pair` = 0: every batch above 256 bits takes
 * form 1; up to two workgroups per CU, and beyond 2 x cu_count units of three a whole number of generations of three- and
 * two-ciphertext units that covers the batch exactly, the two-ciphertext units last, once the batch holds two ciphertexts per unit;
 * k = 1 is the same either way).  `allow_pair` = 1 is fheaes_k2_launch_plan; any other value is FHEAES_ERR_INVALID.  Host logic only. */
int fheaes_k2_launch_plan_forms(uint64_t m, uint32_t cu_count, uint32_t k, int allow_pair, int *form, uint64_t *units_main, uint32_t *r_main,
                                uint64_t *units_tail, uint32_t *r_tail);
/* The same for a CONTEXT: the form and the kernel this context really launches for a batch of `m` bits on its device, after the
 * occupancy fallbacks (the paired kernel needs 159,504 B of LDS per workgroup: where the runtime cannot place one on a CU every batch
 * takes form 1; the 16-form's LDS-home variant needs two workgroups of 81,920 B per CU, else its parked variant runs).  `kernel`
 * (may be NULL) receives the kernel's name, e.g. "blind_rotate_pair_kernel<5,5,8,3,2>".  Measurements must be labelled from this call. */
int fheaes_k2_context_plan(fheaes_ctx *ctx, uint64_t m, int *form, uint64_t *units_main, uint32_t *r_main, uint64_t *units_tail,
                           uint32_t *r_tail, char *kernel, size_t kernel_cap);
/* Where the paired blind-rotation kernel parks the half of its accumulators that does not fit a CU's registers and LDS: `claimed` = 1
 * (default): 64 KB slots of a shared pool, 128 per XCC, claimed with one compare-and-swap when a workgroup starts and released when it
 * ends, so that the slots the resident workgroups use stay in the caches; 0: one private slot per workgroup of the launch (64 KB x
 * the grid).  Same words either way (tests/test_gpu_fullsize.py).  The name `fheaes_k2_context_plan` reports carries the setting
 * (" parking=claimed" / " parking=private").  Ownership of a slot is recorded in memory and never inferred from the compute unit a
 * workgroup runs on: a queue preempted mid-kernel resumes its workgroups on other compute units (round 5's defect). */
int fheaes_k2_set_parking(fheaes_ctx *ctx, int claimed);
/* Test hook of the occupancy fallbacks (tests/test_gpu_k2_shapes.py): `allow_pair` = 0 takes the paired kernel away from this context,
 * `allow_home` = 0 the 16-form's LDS-home variant, exactly as a refused occupancy query does; 1 means "whatever the query allows" -- the
 * effective setting is "queried AND allowed", so the hook can only take a form away and never grants one the device refused.  Default:
 * both 1.  Each argument is 0 or 1 (else FHEAES_ERR_INVALID).  fheaes_k2_context_plan, fheaes_reserve and every launch follow the
 * setting; with the pair denied the paired kernel's parking pool and owner words are not touched.  Per context: other contexts and
 * the plans of k = 1 (which has neither form) are unaffected.  Synchronises the context's stream. */
int fheaes_k2_set_forms(fheaes_ctx *ctx, int allow_pair, int allow_home);
/* How the block ciphers cut their work into blind-rotation launches.  fheaes_aes_encrypt, fheaes_aes_decrypt_equivalent (`steps` = Nr
 * WoPBS per block) and fheaes_aes_decrypt (`steps` = 2 Nr - 1) on `n_blocks` blocks are `steps` x `n_blocks` block-rounds of 128 bits, and
 * a round of block b needs only the round before it of the same block.  Round by round, every one of the `steps` launches ends in a partly
 * filled generation of one workgroup per compute unit, which costs nearly a full one (16,384 bits on 256 CUs: 11 generations for 10.67 of
 * work).  ROLLED, the block-rounds are taken as one stream in (step, block) order and cut into windows of `window_blocks` blocks whose bits
 * are a whole number of six-ciphertext generations: only the call's last launch has a partial generation.  A window covers the end of one
 * step and the start of the next; the words of every block are those of the round-by-round schedule.
 * This is the decision, host logic only and DEVICE-INDEPENDENT like fheaes_k2_launch_plan: roll when the launch of the full batch
 * (min(n_blocks x 128, 32,768) bits) takes the paired form, n_blocks x 128 bits are not whole generations of 6 x cu_count, and the rolled
 * schedule has strictly fewer generations than the round-by-round one, both counted with fheaes_k2_launch_plan (a launch of up to 768 bits
 * counts as one).  The window is the largest multiple of lcm(128, 6 cu_count) / 128 blocks (12 on 256 CUs, 57 on 304) that exceeds neither
 * n_blocks nor 256 blocks.  `window_blocks` = 0: not rolled; then `launches` and `generations` are the round-by-round schedule's.  Rolled,
 * `launches` = ceil(steps x n_blocks / window_blocks).  128 blocks, 10 steps, 256 CUs: window 120, 11 launches, 107 generations for 110.
 * FHEAES_ERR_INVALID: a null output, n_blocks, steps or cu_count of 0. */
int fheaes_aes_window_plan(uint64_t n_blocks, uint32_t steps, uint32_t cu_count, uint32_t k, uint64_t *window_blocks, uint64_t *launches,
                           uint64_t *generations, uint64_t *generations_by_round);
/* The window THIS context uses for `steps` WoPBS over `n_blocks` blocks: fheaes_aes_window_plan for its device's compute units and the form its
 * launches really take (after the occupancy fallbacks and fheaes_k2_set_forms: a context without the paired kernel never rolls), or what
 * fheaes_aes_set_window set.  0: round by round. */
int fheaes_aes_context_window(fheaes_ctx *ctx, uint64_t n_blocks, uint32_t steps, uint64_t *window_blocks);
/* `window_blocks` = 0 (default): automatic, as above.  FHEAES_AES_WINDOW_OFF: one launch per round, the schedule without windows, for
 * word-exact comparison and same-process timing.  Any other value forces that window, clamped to n_blocks and to 256 blocks, whatever
 * the form of the blind rotation: every window in 1..n_blocks is a correct schedule, so the small parameter set can exercise every
 * shape of segment (tests/test_gpu_aes_windows.py).  Per context, like fheaes_k2_set_forms.  Synchronises the context's stream.  The
 * public-block / CTR calls, the key expansion and fheaes_add_scalar are not windowed. */
#define FHEAES_AES_WINDOW_OFF 0xFFFFFFFFu
int fheaes_aes_set_window(fheaes_ctx *ctx, uint32_t window_blocks);
/* Test hook of the claimed parking slots (tests/test_gpu_park_slots.py).  The pool is FHEAES_K2_PARK_SLOTS owner words, 128 per XCC
 * (0 = free, else 1 + the index of the owning workgroup).  `initial_owner` (host, FHEAES_K2_PARK_SLOTS words) non-NULL: every
 * claimed-mode paired launch starts from a copy of these words instead of zeros -- a nonzero word is a slot someone else owns for the
 * whole launch; NULL restores the default.  `record` = 1: every such launch writes {slot used, XCC id when it released the slot} per workgroup (slot >=
 * FHEAES_K2_PARK_SLOTS: the workgroup's private fallback slot FHEAES_K2_PARK_SLOTS + its index).  No effect on the other kernel forms or
 * with private parking.  Synchronises the context's stream. */
#define FHEAES_K2_PARK_SLOTS 1024
int fheaes_k2_park_debug(fheaes_ctx *ctx, const uint32_t *initial_owner, int record);
/* Synchronises, then reads the two counters the paired kernel keeps for the life of the context (workgroups that fell back to a private
 * slot; releases that found an owner word other than their own), the owner words as the last claimed launch left them (`owner_out`:
 * FHEAES_K2_PARK_SLOTS words or NULL) and the records of the last launch recorded since fheaes_k2_park_debug (`record_out`: [record_cap][2]
 * words or NULL; `record_n` receives the number of records, that launch's grid, or 0).  A `record_cap` below it is FHEAES_ERR_INVALID. */
int fheaes_k2_park_read(fheaes_ctx *ctx, uint64_t *fallbacks, uint64_t *violations, uint32_t *owner_out, uint32_t *record_out,
                        uint64_t record_cap, uint64_t *record_n);
/* Test hooks of the workspace state (tests/test_gpu_workspace_state.py): no call may depend on what an earlier call left in the scratch
 * the calls of a context share, on where that scratch lay, or on how large it was.  The FHEAES_WS_BUFFERS scratch buffers are the
 * grow-only workspaces and the four staging buffers of host-memspace calls; the keys, the twiddles, the LUT sets, the pinned upload
 * buffer and the parking owner words, pattern and record of fheaes_k2_park_debug / _read (state that persists by design) are not among
 * them and are never touched.  Every buffer has a class, and a class a fill pattern under which a stale read yields wrong words and
 * never a wild address:
 *   FHEAES_WS_F64     only ever doubles                      every double the quiet NaN 0x7FF87FF87FF87FF8
 *   FHEAES_WS_WORDS   torus words, digits, accumulators      every byte 0xA5
 *   FHEAES_WS_TABLES  index tables and staged arguments      every 32-bit word 1: as an index entry 1, in range wherever there are two
 *                                                            of a thing; as a word or a byte non-zero (the last size % 4 bytes: 0xA5)
 * fheaes_workspace_info: buffer `index` (>= FHEAES_WS_BUFFERS: FHEAES_ERR_INVALID) -- its name, current size in bytes (0: never grown, or
 * released), class, the 8 bytes at offset 0 and its last whole 8-byte word (offset (bytes / 8 - 1) * 8); a buffer of fewer than 8 bytes
 * reports its bytes zero-extended in both, an empty one 0.  Any out-pointer may be NULL.  Synchronises the context's stream first.
 * fheaes_workspace_poison: takes the context's lock and synchronises its stream; FHEAES_WS_POISON_FILL overwrites every buffer over its
 * whole current size with the pattern of its class (hipMemset*Async on the context's stream, then synchronised: no kernel);
 * FHEAES_WS_POISON_RELEASE frees every buffer and sets its size to 0, so that the next call grows everything from nothing, as on a fresh
 * context but without a new key upload.  *bytes_out (may be NULL): the bytes filled or freed.  Any other mode is FHEAES_ERR_INVALID. */
#define FHEAES_WS_BUFFERS 17
#define FHEAES_WS_F64 0
#define FHEAES_WS_WORDS 1
#define FHEAES_WS_TABLES 2
#define FHEAES_WS_PATTERN_F64_HALF 0x7FF87FF8u
#define FHEAES_WS_PATTERN_WORDS 0xA5
#define FHEAES_WS_PATTERN_TABLES 1u
#define FHEAES_WS_POISON_FILL 0
#define FHEAES_WS_POISON_RELEASE 1
int fheaes_workspace_info(fheaes_ctx *ctx, uint32_t index, char *name_out, size_t name_cap, uint64_t *bytes_out, int *class_out,
                          uint64_t *first_word_out, uint64_t *last_word_out);
int fheaes_workspace_poison(fheaes_ctx *ctx, int mode, uint64_t *bytes_out);
/* Test hook of FHEAES_ERR_NOMEM (tests/test_gpu_alloc_failures.py), one shot.  `fail_nth` = n > 0: the n-th device allocation this
 * context makes from now on (see FHEAES_ERR_NOMEM for what counts) is put to the runtime with twice the device's total memory
 * (hipMemGetInfo) in place of its size: the refusal, and the error state it leaves, are the runtime's own, and nothing is reserved.
 * `fail_nth` = 0 disarms.  Either way *seen_out (may be NULL) receives the number of allocations the context has made since the hook
 * was last set, the refused one included -- arming far ahead counts a call's allocations -- and the count starts again from 0.  The
 * message of the refused call names the allocation's own size.  Takes the context's lock and synchronises its stream.  A NULL
 * context: FHEAES_ERR_INVALID. */
int fheaes_alloc_debug(fheaes_ctx *ctx, uint64_t fail_nth, uint64_t *seen_out);
const char *fheaes_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FHEAES_H */
