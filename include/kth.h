/*
 * kth.h -- C-ABI of the MI355X k-th element selection engine (libkth.so).
 *
 * Drop-in boundary for laertispappas/MPI-k-selection's selection path.  The
 * reference has no plugin/FFI layer; its boundary is the C-level contract
 * (IntVector data, n = data->size, k) -> int value used at
 *   kth-problem-seq.c:32-33        VecQuickSort(pVec); solution = VecGet(pVec, k-1);
 *   TODO-kth-problem-cgm.c:76-278  CGM rounds + final gather/sort/VecGet on rank 0
 * Every entry point below replaces one of those call sites (cited per function).
 *
 * Conventions (all functions):
 *   - k is 1-based, 1 <= k <= n (as in the reference's VecGet(k-1) call sites).
 *   - Order is signed int32 order (float32: IEEE total order, see "float32
 *     keys" below).
 *   - The input is NOT modified (the reference sorts in place; both of its
 *     drivers discard the data afterwards, kth-problem-seq.c:36,
 *     TODO-kth-problem-cgm.c:283-284, so not mutating is strictly compatible).
 *   - Return value is 0 (KTH_OK) or a negative KTH_E* code; the answer goes to
 *     *out, never in-band (the in-band VecGet sentinels live in vector.h's
 *     VecKthSelect only).
 *   - Streams are passed as `void *` holding a hipStream_t (NULL = HIP's null
 *     stream).  A new ctx owns a private non-blocking stream until
 *     kth_ctx_set_stream replaces it.  No C++ or framework types cross this
 *     boundary.
 *   - A kth_ctx is not thread-safe: one ctx per host thread or device.
 *   - The product path has no CPU fallback: without a usable GPU every compute
 *     entry point returns KTH_ENODEV.
 */
#ifndef KTH_H
#define KTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KTH_OK 0
#define KTH_EINVAL (-1)   /* bad n / k / pointer / shape                */
#define KTH_ENOMEM (-2)   /* device or pinned-host allocation failed    */
#define KTH_EHIP (-3)     /* HIP runtime or kernel launch error         */
#define KTH_ENODEV (-4)   /* no HIP device                              */
#define KTH_EINTERNAL (-5) /* device-side consistency check failed      */
#define KTH_ECOMM (-6)    /* RCCL missing or a collective failed        */

#define KTH_VERSION 1

/* Selection paths (kth_stats.path). */
#define KTH_PATH_LDS 1      /* n small: one workgroup, keys resident in LDS            */
#define KTH_PATH_RADIX 2    /* multi-pass radix select over the input                  */
#define KTH_PATH_WINDOW 3   /* sample window + one streaming pass + candidate radix    */
#define KTH_PATH_WINDOW_FALLBACK 4 /* window missed -> radix passes over the input     */
#define KTH_PATH_K16 5      /* 16-bit keys: settled by the first streaming pass        */
#define KTH_PATH_K16_FALLBACK 6 /* 16-bit keys: a second (or third) pass was taken     */

typedef struct kth_ctx kth_ctx;

typedef struct kth_stats {
    int32_t path;          /* KTH_PATH_*                                      */
    int32_t mode;          /* internal final mode (debug)                     */
    uint32_t lo_key, hi_key; /* sample window in order-preserving key space   */
    uint64_t n, k;
    uint64_t cnt_lt;       /* keys below the window                           */
    uint64_t cnt_eq_lo, cnt_eq_hi;
    uint64_t candidates;   /* keys strictly inside the window                 */
    uint64_t capacity;     /* candidate buffer capacity                       */
    int32_t answer;        /* after a float32 select: the answer's bit pattern
                            * (lo_key / hi_key stay in key space either way)  */
    int32_t error;         /* device-side error word (0 = none)               */
} kth_stats;

const char *kth_strerror(int code);
int kth_version(void);
/* Hash of the sources this libkth.so was built from (16 hex digits; "unknown"
 * outside the in-tree Makefile).  bench.py uses a PMC measurement only when it
 * was taken on the same build. */
const char *kth_build_id(void);
int kth_device_count(void);

/* --- one-shot entry point -------------------------------------------------
 * Replaces kth-problem-seq.c:32-33 and TODO-kth-problem-cgm.c:76-278.
 * keys may be host or device memory (detected with hipPointerGetAttributes).
 * Synchronous; uses a lazily created per-thread ctx on device 0. */
int kth_select_i32(const int32_t *keys, int64_t n, int64_t k, int32_t *out);

/* --- context API (scratch reuse, streams) ---------------------------------- */
int kth_ctx_create(int device, kth_ctx **ctx);
int kth_ctx_destroy(kth_ctx *ctx);
int kth_ctx_set_stream(kth_ctx *ctx, void *hip_stream);
int kth_ctx_sync(kth_ctx *ctx);
/* Pre-size scratch for inputs of up to n keys (optional; grows on demand). */
int kth_ctx_reserve(kth_ctx *ctx, int64_t n);

/* Synchronous select through a ctx; keys host or device.  Same contract as
 * kth_select_i32. */
int kth_select_i32_ctx(kth_ctx *ctx, const int32_t *keys, int64_t n, int64_t k, int32_t *out);

/* Asynchronous select: d_keys and d_out are device memory; the work is
 * enqueued on the ctx stream and *d_out is written on the device.  No host
 * synchronisation and no allocation once the ctx is reserved for n
 * (graph-capturable).
 *
 * Graph capture (this call, kth_select_f32_async, kth_select_multi_*_async and
 * kth_select_{,multi_}k16_async; tests/test_gpu_graph.py pins every line):
 *   - Capture on the stream the ctx is bound to, after the ctx has been
 *     reserved for that form and size (kth_ctx_reserve, kth_ctx_reserve_multi,
 *     kth_ctx_reserve_k16): the call then allocates and synchronises nothing.
 *   - While a graph that used the ctx is alive, make no call that grows one of
 *     the ctx's buffers (a larger n or m than reserved for, a first top-k):
 *     growing frees the old buffer, whose address the graph holds.  Destroy
 *     the graph before the ctx.
 *   - A graph holds the launches as they were enqueued: the ctx's cooperative
 *     or per-level mode, its test hooks and its timing switch (keep timing
 *     off while capturing) are frozen in it as they were at capture; changing
 *     them later changes no replay.
 *   - Any number of calls per graph, of any of these forms.  Every launch
 *     sequence leaves the ctx's scratch as it found it, so a replay may follow
 *     itself, another graph of the same ctx, or any eager call on the same ctx
 *     and stream (selects, multi and 16-bit calls, top-k, rows), in any order
 *     and number.  The same holds after a call whose error was only reported
 *     (the test hook KTH_HOOK_FAULT_BARRIER: its barriers complete).  A grid
 *     barrier that really timed out is excluded: workgroups may then still
 *     add into slots that others clear, so the scratch is not known clean
 *     and the asynchronous forms do not re-zero it: after a stats().error of
 *     64 from an asynchronous call, go on with a fresh ctx.
 *   - kth_ctx_last_stats reports the launches that ran last on the stream,
 *     replayed or eager (the device records it).  kth_ctx_multi_stats(ctx, i)
 *     maps i to a rank by the last multi or 16-bit call made -- or captured --
 *     through the API, and is KTH_EINVAL when what ran last is not a call of
 *     that form and key kind.
 * Top-k, the rows kernels and the sharded protocol are not claimed capturable. */
int kth_select_i32_async(kth_ctx *ctx, const int32_t *d_keys, int64_t n, int64_t k, int32_t *d_out);

/* --- float32 keys (one array) ------------------------------------------------
 * The _f32 twins of the three selects above: same error codes (KTH_EINVAL
 * before any device work, KTH_ENODEV without a GPU), same stream behaviour,
 * same cooperative back-off rule, the async form graph-capturable once the ctx
 * is reserved (under the conditions at kth_select_i32_async).  Order, the one
 * kth_select_rows_f32 uses: IEEE total order on the bit patterns, -0.0 <
 * +0.0, subnormals distinct, every NaN (either sign, any payload) above +inf
 * and equal to every other NaN.  The returned value has the bit pattern of an
 * input element, except that a NaN comes back as the canonical quiet NaN
 * 0x7FC00000.  The input is not modified.
 * The kernels are the int32 kernels instantiated for float32 words: a word
 * becomes an ordered int32 right after its load (integer operations only) and
 * a value turns back into a float only where it leaves the library. */
int kth_select_f32(const float *keys, int64_t n, int64_t k, float *out); /* host or device keys */
int kth_select_f32_ctx(kth_ctx *ctx, const float *keys, int64_t n, int64_t k, float *out);
int kth_select_f32_async(kth_ctx *ctx, const float *d_keys, int64_t n, int64_t k, float *d_out);
/* The order as numbers: kth_f32_order_key(x) is the uint32 whose unsigned
 * order is the key order (every NaN -> 0xFFFFFFFF); kth_f32_of_order_key is
 * its inverse (0xFFFFFFFF -> 0x7FC00000).  Host arithmetic only, no device
 * needed; the same definition the kernels compile (csrc/kth_device.hpp). */
uint32_t kth_f32_order_key(float x);
float kth_f32_of_order_key(uint32_t key);

/* --- several ranks of one array ----------------------------------------------
 * out[i] = the ks[i]-th smallest of keys[0..n), for m ranks at once: the
 * quantiles of one array (numpy.partition(a, [k1, k2, ...])[[k1, k2, ...]]).
 * ks is a host array of m 1-based ranks, read before the call returns; any
 * order, duplicates allowed (a duplicate is resolved once and copied).  Every
 * out[i] is bit-identical to what kth_select_i32 / kth_select_f32 returns for
 * that rank; float32 keys follow kth_select_f32's order, NaN rule and
 * canonical NaN.  The input is not modified.
 *   1 <= m <= KTH_MULTI_MAX_RANKS and 1 <= ks[i] <= n, else KTH_EINVAL before
 *   any device work with out untouched; KTH_ENODEV without a GPU.
 * The forms are those of the single select: the one-shot and _ctx forms take
 * host or device keys and are synchronous; the _async form takes device
 * memory only, enqueues on the ctx stream, makes no host synchronisation, and
 * no allocation once kth_ctx_reserve_multi(ctx, n, m) or an earlier call of
 * the same size has sized the scratch (graph-capturable, under the conditions
 * at kth_select_i32_async; any number of distinct ranks, and a duplicate's
 * copy is a node of the graph).
 * One pass: for n > 4 Mi keys on a ctx that runs the cooperative kernels, the
 * call reads the input from HBM ONCE: a sample phase per distinct rank, one
 * streaming launch that serves every rank's window from each loaded tile, a
 * finish phase per distinct rank over that rank's own counts and candidates
 * (with the single select's exact whole-input fallback for a rank whose
 * window missed or overflowed; the other ranks are not disturbed).
 * Not one pass, but exact: n <= 4 Mi keys (the LDS and radix paths), and a
 * ctx on the per-level path (KTH_COOP=0, or backing off after a grid-barrier
 * timeout); there the distinct ranks run one after the other through the
 * single select.  A call with one distinct rank is the single select too.
 * Scratch: beside the single select's, one candidate buffer per rank of
 * kth_dist_cand_capacity(n) keys (2^30 keys, 8 ranks: 8 x 128 MiB = 1 GiB),
 * and ~1.6 MB of slots.
 * Errors: a device-side error on rank i shows in kth_ctx_multi_stats(ctx, i)
 * .error; the synchronous forms then return KTH_EINTERNAL, and after a
 * reported grid-barrier timeout they redo the call on the per-level path, as
 * kth_select_i32_ctx does.  A multi call counts as one selection for the
 * cooperative back-off.  kth_ctx_last_stats after a multi call returns rank
 * m-1's stats.  Timing: on the one-pass path kth_ctx_take_timing counts a
 * multi call as one select whose main_ms covers the one streaming launch. */
#define KTH_MULTI_MAX_RANKS 8
int kth_select_multi_i32(const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out);
int kth_select_multi_i32_ctx(kth_ctx *ctx, const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out);
int kth_select_multi_i32_async(kth_ctx *ctx, const int32_t *d_keys, int64_t n, const int64_t *ks, int m,
                               int32_t *d_out);
int kth_select_multi_f32(const float *keys, int64_t n, const int64_t *ks, int m, float *out);
int kth_select_multi_f32_ctx(kth_ctx *ctx, const float *keys, int64_t n, const int64_t *ks, int m, float *out);
int kth_select_multi_f32_async(kth_ctx *ctx, const float *d_keys, int64_t n, const int64_t *ks, int m, float *d_out);
/* Pre-size the scratch of multi calls of up to m ranks over up to n keys. */
int kth_ctx_reserve_multi(kth_ctx *ctx, int64_t n, int m);
/* Stats of rank i (0 <= i < m) of the last multi call on this ctx
 * (synchronises the ctx stream). */
int kth_ctx_multi_stats(kth_ctx *ctx, int i, kth_stats *st);

/* --- 16-bit keys (one array) ---------------------------------------------------
 * The select and the multi-rank select for int16, uint16, float16 and bfloat16
 * keys, read as 2-byte words (a caller need not widen them to 32 bits).  kind
 * names the order: */
#define KTH_K16_I16  0   /* signed order                                   */
#define KTH_K16_U16  1   /* unsigned order                                 */
#define KTH_K16_F16  2   /* IEEE binary16, total order, NaN above +inf     */
#define KTH_K16_BF16 3   /* bfloat16, same rule                            */
/* kth_k16_order_key(bits, kind) is the uint16 whose unsigned order is the key
 * order: i16 bits ^ 0x8000, u16 bits; f16 / bf16 the float32 rule at 16 bits
 * (negative b -> ~b, any other b -> b | 0x8000, every NaN -> 0xFFFF; so -0.0 <
 * +0.0, subnormals distinct, every NaN equal to every other and above +inf,
 * whose keys are 0xFC00 / 0xFF80).  kth_k16_of_order_key is its inverse, 0xFFFF
 * -> the canonical quiet NaN 0x7E00 / 0x7FC0.  An unknown kind gives 0 from
 * both.  Host arithmetic, no device needed; the definitions the kernels
 * compile (csrc/kth_k16.hpp).
 * The selects follow kth_select_f32* and kth_select_multi_*: k and ks[i] are
 * 1-based, 1 <= m <= KTH_MULTI_MAX_RANKS, ranks in any order, a duplicate is
 * resolved once and copied; a bad n / k / m / kind / pointer is KTH_EINVAL
 * before any device work with out untouched, no GPU is KTH_ENODEV; the input
 * is not modified; the one-shot and _ctx forms take host or device keys and
 * are synchronous (they read the status once: a device-side error is
 * KTH_EINTERNAL); the _async forms take device memory only, enqueue on the ctx
 * stream, never synchronise, and allocate nothing once
 * kth_ctx_reserve_k16(ctx, n, m) or any earlier k16 call has run (the scratch,
 * ~1.3 MB, does not depend on n or m), so they are graph-capturable (under the
 * conditions at kth_select_i32_async; KTH_HOOK_K16_MISS is frozen too).  The
 * answer has the bit pattern of an input element, a NaN comes back canonical.
 * d_keys needs only 2-byte alignment.  Counts and ranks are 64-bit.
 * n <= 32768: the full 65536-bin histogram decides.  Above: a sample window
 * per distinct rank and ONE streaming launch for all ranks read the input once;
 * whether a second (and third) pass is needed is decided on the device, their
 * launches are always enqueued and return at once when every rank is settled.
 * Worst case: the input is read three times beside the sample.  The path has
 * no cooperative launch and no grid barrier: kth_ctx_coop's state is neither
 * used nor counted down.
 * Stats: kth_ctx_last_stats after a single k16 select and kth_ctx_multi_stats
 * (ctx, i) after a multi call give path KTH_PATH_K16 (one pass) or
 * KTH_PATH_K16_FALLBACK, lo_key / hi_key the last pass's window as 16-bit order
 * keys, cnt_lt the keys below it, candidates the keys inside, answer the
 * answer's bits, error the device-side error word.  kth_ctx_take_timing counts
 * a k16 call as one select whose main_ms is the first streaming launch (for
 * n <= 32768, where there is none, the histogram launch).  After a fallback
 * the window reported is the narrowed one of the last pass, not the sample's. */
uint16_t kth_k16_order_key(uint16_t bits, int kind);
uint16_t kth_k16_of_order_key(uint16_t key, int kind);
int kth_select_k16(const void *keys, int64_t n, int64_t k, int kind, uint16_t *out); /* host or device keys */
int kth_select_k16_ctx(kth_ctx *ctx, const void *keys, int64_t n, int64_t k, int kind, uint16_t *out);
int kth_select_k16_async(kth_ctx *ctx, const void *d_keys, int64_t n, int64_t k, int kind, uint16_t *d_out);
int kth_select_multi_k16(const void *keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *out);
int kth_select_multi_k16_ctx(kth_ctx *ctx, const void *keys, int64_t n, const int64_t *ks, int m, int kind,
                             uint16_t *out);
int kth_select_multi_k16_async(kth_ctx *ctx, const void *d_keys, int64_t n, const int64_t *ks, int m, int kind,
                               uint16_t *d_out);
int kth_ctx_reserve_k16(kth_ctx *ctx, int64_t n, int m);

/* Stats of the last select on this ctx (synchronises the ctx stream). */
int kth_ctx_last_stats(kth_ctx *ctx, kth_stats *st);

/* How the cooperative finish (k_finish) of the last select on this ctx ended,
 * read from the last-call word its final kernel leaves (synchronises the ctx
 * stream; follows a replayed graph like kth_ctx_last_stats):
 *   KTH_FINISH_NONE     the last selection ended in another kernel (LDS path,
 *                       per-level path, 16-bit keys)
 *   KTH_FINISH_COUNTS   decided from the streaming pass's counts, no level ran
 *   KTH_FINISH_SLICES   every workgroup scanned its slice of the domain and the
 *                       last to arrive resolved the picked bin (the slice tail)
 *   KTH_FINISH_GROUPED  one workgroup gathered the picked bin from the grouped
 *                       candidates by k_main<0>'s directory
 *   KTH_FINISH_LEVELS   grid-wide levels to the end, no tail (heavy ties, the
 *                       fallback over the input)
 * KTH_EINVAL before the first selection. */
#define KTH_FINISH_NONE 0
#define KTH_FINISH_COUNTS 1
#define KTH_FINISH_SLICES 2
#define KTH_FINISH_GROUPED 3
#define KTH_FINISH_LEVELS 4
int kth_ctx_last_finish_form(kth_ctx *ctx, int *form);

/* Diagnostics: 1 when the ctx runs the cooperative (grid-barrier) kernels,
 * 0 while it is on the per-level path -- for COOP_BACKOFF = 64 selections of
 * any entry point after a grid-barrier timeout (the synchronous entry points
 * redo the timed-out select; the asynchronous ones report it in the stats). */
int kth_ctx_coop(const kth_ctx *ctx);

/* --- test hooks (TEST ONLY: never set by the product path) ------------------
 * Fault injectors for the parity tests' error paths.  They are off in every
 * new ctx and are not read from the environment; only this call turns them on.
 *   KTH_HOOK_FAULT_TOPK_RANK  value != 0: kth_topk_i32, kth_topk_f32 and
 *                             kth_topk_k16 select a neighbouring rank, so
 *                             their count pass must report the bracket
 *                             failure (outputs unwritten, stats .error set)
 *   KTH_HOOK_FAULT_BARRIER    1: every grid barrier of the cooperative kernels
 *                             reports a timeout; 2: only the next cooperative
 *                             launch does; 0: off
 *   KTH_HOOK_TOPK_SEG_CAP     entries per staged top-k segment (0 = sized from n;
 *                             small values force the segment-overflow fallback)
 *   KTH_HOOK_K16_MISS         value != 0: the sample phase of the 16-bit select
 *                             publishes a window that holds no key, so the
 *                             later passes must produce every answer
 *   KTH_HOOK_FINISH_SLICES    value != 0: k_finish ignores the group directory
 *                             and takes the slice tail (the grouped form's
 *                             reference); frozen in a captured graph
 *   KTH_HOOK_K16_TOPK_NOSKIP  value != 0: kth_topk_k16's count pass ignores the
 *                             flags its streaming pass recorded and loads
 *                             every tile (the skipping path's reference)
 * Returns KTH_EINVAL for an unknown hook or a bad value. */
#define KTH_HOOK_FAULT_TOPK_RANK 1
#define KTH_HOOK_FAULT_BARRIER 2
#define KTH_HOOK_TOPK_SEG_CAP 3
#define KTH_HOOK_K16_MISS 4
#define KTH_HOOK_FINISH_SLICES 5
#define KTH_HOOK_K16_TOPK_NOSKIP 6 /* (kth_topk_k16) */
int kth_ctx_test_hook(kth_ctx *ctx, int hook, int64_t value);

/* --- timing (bench) ----------------------------------------------------------
 * When enabled, every select records HIP events on the ctx stream around the
 * streaming pass (the dominant kernel) and around the whole select. */
int kth_ctx_enable_timing(kth_ctx *ctx, int on);
/* Synchronises; returns sums over the selects since the last call and resets:
 * *n_selects, *main_ms (sum of dominant-kernel durations), *total_ms. */
int kth_ctx_take_timing(kth_ctx *ctx, int64_t *n_selects, double *main_ms, double *total_ms);

/* --- batched rows (BASELINE config 5; no reference counterpart) -------------
 * out[r] = k-th smallest of row r of a rows x cols row-major matrix.  cols <=
 * 4096: one wavefront per row, the row held in the wave's registers (64 keys a
 * lane at most); wider rows: one workgroup per row, the row resident in LDS.
 * 1 <= cols <= KTH_ROWS_MAX_COLS.
 * float32 order: IEEE total order with -0.0 < +0.0 and every NaN last
 * (a NaN answer is returned as the canonical quiet NaN 0x7FC00000). */
#define KTH_ROWS_MAX_COLS 16384
int kth_select_rows_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int32_t k,
                        int32_t *d_out);
int kth_select_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int32_t k,
                        float *d_out);

/* --- top-k per row (the MoE-routing shape) ---------------
 * The k smallest keys of each row (largest != 0: the k largest), with their
 * column indices, in column order; of the keys equal to the k-th, the first
 * ones by column.  d_vals: rows x k values, d_idx: rows x k int32 columns;
 * either may be NULL (not both).  1 <= k <= cols <= KTH_TOPK_MAX_COLS.  Same
 * orders as kth_select_rows_* (float: IEEE total order, NaN above +inf, so
 * NaNs come last for smallest and first for largest).  A value in d_vals has
 * the bit pattern of an input element; kth_topk_rows_f32 writes a NaN in
 * d_vals as the canonical quiet NaN 0x7FC00000. */
#define KTH_TOPK_MAX_COLS 4096
int kth_topk_rows_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int32_t k, int largest,
                      int32_t *d_vals, int32_t *d_idx);
int kth_topk_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int32_t k, int largest,
                      float *d_vals, int32_t *d_idx);

/* --- 16-bit rows: k-th and top-k per row of 2-byte keys ----------------------
 * kth_select_rows_* and kth_topk_rows_* for int16, uint16, float16 and
 * bfloat16 rows, read as they are (2 bytes a key; no widened copy).  d_keys is
 * a row-major rows x cols matrix of 2-byte words in device memory; kind is
 * KTH_K16_I16 / U16 / F16 / BF16 and the order is kth_k16_order_key's: -0.0 <
 * +0.0, subnormals distinct, every NaN (either sign, any payload) equal to
 * every other and above +inf.  1 <= k <= cols <= KTH_ROWS16_MAX_COLS for both.
 *   select: d_out[r] = the bits of the k-th smallest element of row r; a NaN
 *     comes back canonical (0x7E00 / 0x7FC0).
 *   top-k: the k smallest keys of each row (largest != 0: the k largest) with
 *     their columns, in column order; of the keys equal to the k-th, the first
 *     ones by column.  d_vals: rows x k 2-byte values (NaN canonical), d_idx:
 *     rows x k int32 columns; either may be NULL, not both.  NaNs come last
 *     for smallest and first for largest, as in kth_topk_rows_f32.
 * KTH_EINVAL before any device work: a NULL ctx or keys, no output pointer,
 * rows < 0, a bad cols, k or kind.  rows == 0 returns KTH_OK and launches
 * nothing.  Asynchronous on the ctx stream; no ctx scratch, no allocation and
 * no host synchronisation.  As the other rows calls, not claimed capturable.
 * d_keys, d_out and d_vals need only 2-byte alignment and any cols is exact;
 * the fast path is a 16-byte aligned d_keys with cols % 8 == 0 (every row
 * then starts on a 16-byte boundary and is read with 16-byte loads), anything
 * else is read with guarded 2-byte loads.
 * One wavefront per row, the row held in registers as packed pairs; an order
 * key of 16 bits is two 8-bit digits, so every row takes the same two
 * histogram passes whatever its values (csrc/kth_rows16.hpp). */
#define KTH_ROWS16_MAX_COLS 8192
int kth_select_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int32_t k,
                        int kind, uint16_t *d_out);
int kth_topk_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int32_t k, int largest,
                      int kind, uint16_t *d_vals, int32_t *d_idx);

/* --- top-k of one array ------------------------------------
 * The k smallest keys of d_keys[0..n) (largest != 0: the k largest) with their
 * int64 indices, in index order; of the keys equal to the k-th, the first ones
 * by index.  The reference implies this as sort(a)[0..k) after its select
 * block (kth-problem-seq.c:32-33, VecQuickSort then index); here it is the
 * select (kth_select_i32_async) plus a count pass, a chunk scan and an ordered
 * compaction that reads only the chunks holding output keys.  d_vals: k int32,
 * d_idx: k int64; either may be NULL (not both).  1 <= k <= n.  Asynchronous on
 * the ctx stream (device memory only); a device-side inconsistency leaves the
 * outputs unwritten and shows as kth_ctx_last_stats().error. */
int kth_topk_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t n, int64_t k, int largest, int32_t *d_vals,
                 int64_t *d_idx);
/* float32 keys, in the order of kth_select_f32 (NaNs last for smallest, first
 * for largest; a NaN value is written as 0x7FC00000); ties at the k-th key go
 * to the first ones by index, errors are reported as for kth_topk_i32.  Every
 * k is exact.  The staged variant of the int32 top-k (n / 65536 < k <= n / 16
 * on 16-byte aligned keys, which stages the kept keys during the streaming
 * pass) is int32 only: float32 keys take the row-word path for that k range. */
int kth_topk_f32(kth_ctx *ctx, const float *d_keys, int64_t n, int64_t k, int largest, float *d_vals,
                 int64_t *d_idx);

/* --- top-k of one array, 16-bit keys -------------------------------------------
 * kth_topk_f32's contract for int16, uint16, float16 and bfloat16 keys, read
 * as 2-byte words (no widened copy): the k smallest keys of d_keys[0..n), or
 * the k largest when largest != 0, with their int64 indices, in index order;
 * of the keys equal to the k-th, the first ones by index.  A 16-bit key has
 * 65536 values, so the k-th value nearly always has a large tie group: the
 * tie quota is the normal case here.  kind is KTH_K16_I16 / U16 / F16 / BF16
 * and the order is kth_k16_order_key's: -0.0 < +0.0, subnormals distinct,
 * every NaN equal to every other and above +inf, so NaNs come last for
 * smallest and first for largest.
 * d_vals: k 2-byte words, each the bit pattern of the input element except
 * that a NaN is written canonical (0x7E00 / 0x7FC0); d_idx: k int64; either
 * may be NULL, not both.  1 <= k <= n.  KTH_EINVAL before any device work,
 * outputs untouched: a NULL ctx or keys, no output pointer, a bad n, k or
 * kind; KTH_ENODEV without a GPU.
 * d_keys and d_vals need only 2-byte alignment and any n is exact; the fast
 * path is a 16-byte aligned d_keys, anything else reads the first and last
 * tile with guarded 2-byte loads (and the select its head and tail).
 * Asynchronous on the ctx stream, device memory only, no host
 * synchronisation, no allocation once a call of the same n has run; like the
 * other top-k calls not claimed graph-capturable.  The call leaves the ctx's
 * 16-bit scratch (sample histogram, bins, states) and the top-k arrival
 * counter as it found them, so any eager call or graph replay on the same
 * ctx may follow (the rule of the graph-capture section above).
 * It is the 16-bit select (kth_select_k16_async's launches, one rank) plus a
 * count pass, kth_topk_i32's tile scan and an ordered compaction that reads
 * only the tiles holding output.  For k <= n / 16384 the select's streaming
 * pass also records which of its 2048-key rows can hold output, and the
 * count pass loads only those (decided on the device; a window that missed on
 * the far side turns the skipping off for that call).
 * Errors: a device-side inconsistency (counts that do not bracket k: 32)
 * leaves the outputs unwritten and shows in kth_ctx_last_stats().error.
 * Stats: kth_ctx_last_stats reports the embedded select (path KTH_PATH_K16 /
 * KTH_PATH_K16_FALLBACK, answer = the k-th key's bits). */
int kth_topk_k16(kth_ctx *ctx, const void *d_keys, int64_t n, int64_t k, int largest, int kind,
                 uint16_t *d_vals, int64_t *d_idx);
/* Diagnostics of the last kth_topk_k16 on this ctx (synchronises the ctx
 * stream): *tiles = its count-pass tiles (2048 keys each), *tiles_read = how
 * many of them the count pass loaded from the input; the rest were proven
 * empty by the select's streaming pass.  KTH_EINVAL before the first such
 * call. */
int kth_ctx_last_topk_k16_tiles(kth_ctx *ctx, uint64_t *tiles, uint64_t *tiles_read);

/* --- wide rows: k-th and top-k per row of up to 2^24 columns -------------------
 * kth_select_rows_* and kth_topk_rows_* for the shape between them and the
 * one-array calls: a batch of 1 to a few thousand rows of 32 Ki to 1 Mi int32
 * or float32 keys (a logits matrix, a quantile per long channel).  Row r is
 * d_keys[r*ld .. r*ld + cols), ld >= cols in elements (a padded vocabulary, a
 * column view).  1 <= k <= cols <= KTH_WIDE_MAX_COLS; rows >= 0, rows == 0
 * returns KTH_OK and launches nothing.  Any cols, ld and base alignment is
 * exact; the fast case is a 16-byte aligned base with ld % 4 == 0 (16-byte
 * loads), anything else takes guarded 4-byte loads.
 * Order and results are exactly those of kth_select_rows_* / kth_topk_rows_*:
 * int32 in signed order, float32 in IEEE total order (-0.0 < +0.0, subnormals
 * distinct, every NaN equal to every other and above +inf); a value written
 * has the bit pattern of an input element, a NaN is written as 0x7FC00000.
 * Top-k: the k smallest keys (largest != 0: the k largest) with their int32
 * columns, in column order; of the keys equal to the k-th, the first ones by
 * column.  d_vals, d_idx: dense rows x k, either may be NULL, not both.  For
 * cols in the existing calls' ranges the outputs are bit-identical to theirs.
 * Asynchronous on the ctx stream, device memory only, no host synchronisation;
 * no allocation once kth_ctx_reserve_wide_rows(ctx, rows, cols) or an earlier
 * call of that shape has run; graph-capturable under the conditions written at
 * kth_select_i32_async (a forced plan is frozen at capture).  The calls use
 * scratch of their own in the ctx, which every launch sequence leaves as it
 * found it, and touch no other ctx buffer nor the last-call word: any eager
 * call or replay may precede or follow, and kth_ctx_last_stats is unaffected.
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx or keys, no
 * output pointer, rows < 0, a bad cols, ld or k.  KTH_ENODEV without a GPU.
 * Two forms, chosen by kth_wide_rows_plan from (rows, cols, num_cu)
 * (csrc/kth_rows_wide.hpp): `slices` workgroups share a row when the rows
 * alone do not fill the GPU (a radix select of at most three digits, the
 * row's histogram in scratch, every hand-off a kernel boundary); slices == 1
 * is one workgroup per row with every digit in one launch.  Rows are
 * processed in groups of group_rows, so the scratch (scratch_bytes of the
 * plan, 0 for slices == 1) stays at or below 32 MiB whatever rows is;
 * slice_keys (a multiple of 4) is the columns of a slice. */
#define KTH_WIDE_MAX_COLS   (1 << 24)
#define KTH_WIDE_MAX_SLICES 256
int kth_select_wide_rows_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                             int32_t *d_out);
int kth_select_wide_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                             float *d_out);
int kth_topk_wide_rows_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                           int largest, int32_t *d_vals, int32_t *d_idx);
int kth_topk_wide_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                           int largest, float *d_vals, int32_t *d_idx);
/* Pre-size the scratch for wide-rows calls of up to `rows` rows (whatever plan,
 * forced ones included, they take). */
int kth_ctx_reserve_wide_rows(kth_ctx *ctx, int64_t rows, int32_t cols);
/* The automatic plan.  Host arithmetic only, no device needed; any output
 * pointer may be NULL.  KTH_EINVAL: rows < 0, a bad cols, num_cu < 1. */
int kth_wide_rows_plan(int64_t rows, int32_t cols, int num_cu, int32_t *slices, int32_t *slice_keys,
                       int32_t *group_rows, int64_t *scratch_bytes);
/* Tests and tuning: force the plan of this ctx; 0 = automatic for that field
 * (slices == 1 forces the fused form; more slices than cols / 4 allows, or
 * more group_rows than the scratch bound, are cut down).  KTH_EINVAL: a NULL
 * ctx, a negative value, slices > KTH_WIDE_MAX_SLICES. */
int kth_ctx_wide_rows_force(kth_ctx *ctx, int32_t slices, int32_t group_rows);

/* --- wide rows, 16-bit keys ------------------------------------------------------
 * The wide-rows calls for int16, uint16, float16 and bfloat16 rows, read as
 * they are (2 bytes a key; no widened copy): a bfloat16 or float16 logits
 * matrix of batch x vocabulary.  Row r is the 2-byte words d_keys[r*ld .. r*ld
 * + cols), ld >= cols in elements.  1 <= k <= cols <= KTH_WIDE_MAX_COLS; rows
 * >= 0, rows == 0 returns KTH_OK and launches nothing.  kind is KTH_K16_I16 /
 * U16 / F16 / BF16 and the order is kth_k16_order_key's: -0.0 < +0.0,
 * subnormals distinct, every NaN equal to every other and above +inf.
 * Results are exactly those of kth_select_rows_k16 / kth_topk_rows_k16 (for
 * cols <= KTH_ROWS16_MAX_COLS bit-identical to theirs): a value written has
 * the bit pattern of an input element, a NaN is written canonical (0x7E00 /
 * 0x7FC0).  Top-k: the k smallest keys (largest != 0: the k largest) with
 * their int32 columns, in column order; of the keys equal to the k-th, the
 * first ones by column; NaNs come last for smallest and first for largest.
 * d_vals, d_idx: dense rows x k, either may be NULL, not both.  A 16-bit key
 * has 65536 values and a row can have millions of columns, so the k-th value
 * nearly always has a large tie group: the tie quota is the normal case here.
 * Any cols, any ld and any 2-byte aligned base are exact; the fast case is a
 * 16-byte aligned base with ld % 8 == 0 (16-byte loads of 8 keys, a row's last
 * partial vector by guarded 2-byte loads), anything else takes guarded 2-byte
 * loads throughout.  Nothing at or past cols of a row is ever loaded.
 * Launch behaviour is that of the 32-bit wide-rows calls: asynchronous on the
 * ctx stream, no host synchronisation, graph-capturable under the conditions
 * written at kth_select_i32_async.  They use the same ctx scratch (sizes and
 * the 32 MiB bound unchanged): kth_ctx_reserve_wide_rows(ctx, rows, cols) also
 * covers these calls and kth_ctx_wide_rows_force also forces their plan.
 * Every launch sequence leaves that scratch as it found it, so 32-bit and
 * 16-bit wide calls, and any other call, may alternate on one ctx; no other
 * ctx buffer nor the last-call word is touched (kth_ctx_last_stats is
 * unaffected).
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx or keys, no
 * output pointer, rows < 0, a bad cols, ld, k or kind.  KTH_ENODEV without a
 * GPU.
 * An order key of 16 bits is two radix digits (11 + 5 bits), not three: the
 * select reads a row twice, the top-k three times (csrc/kth_rows_wide16.hpp).
 * kth_wide_rows_plan_k16 is kth_wide_rows_plan for these calls: the same
 * rule in columns, but that a slice keeps 8192 columns (the same 16 KiB), with
 * slice_keys a multiple of 8 so that every slice of an aligned row starts on
 * a 16-byte boundary. */
int kth_select_wide_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                             int32_t k, int kind, uint16_t *d_out);
int kth_topk_wide_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                           int32_t k, int largest, int kind, uint16_t *d_vals, int32_t *d_idx);
int kth_wide_rows_plan_k16(int64_t rows, int32_t cols, int num_cu, int32_t *slices, int32_t *slice_keys,
                           int32_t *group_rows, int64_t *scratch_bytes);

/* --- wide rows, ragged: per-row length and per-row k from device memory -----------
 * The "var" twins of the six wide-rows calls: every row has its own length
 * and its own rank, read from device arrays when the launches run.  Per-request
 * top-k sampling (one k a request) and top-k over variable-length score rows
 * in one padded matrix, in one call, and under graph capture: a captured launch
 * freezes cols and k, but a replay sees what d_lens and d_ks hold at replay
 * time.
 * d_lens, d_ks: device arrays of `rows` int32, 4-byte aligned; either or both
 * may be NULL.  d_lens == NULL: every row has cols keys.  d_ks == NULL: every
 * row uses the host k.  They are never read on the host.
 * cols is the largest row length: the plan, the scratch and the host checks use
 * it.  Row r is d_keys[r*ld .. r*ld + len_r), len_r = clamp(d_lens[r], 0,
 * cols).  Nothing at or past len_r of a row is ever loaded.
 * Top-k: k is the output stride and the bound on every row's k, 1 <= k <=
 * cols.  k_r = min(clamp(d_ks[r], 0, k), len_r), or min(k, len_r) when d_ks is
 * NULL.  Entries [0, k_r) of row r's k output slots hold exactly what
 * kth_topk_wide_rows_* would write for a matrix holding that row's first len_r
 * columns and rank k_r (column order, ties to the first by column, a NaN
 * written canonical, `largest` as there).  Entries [k_r, k) are padding: d_idx
 * -1 and d_vals the zero word (0, +0.0, 0x0000).  Every one of the rows * k
 * slots of each non-NULL output is written by every call.  d_cnt[r] = k_r;
 * d_cnt (rows int32, 4-byte aligned) may be NULL.  d_vals and d_idx may each be
 * NULL, not both.
 * Select: k_r = clamp(d_ks[r], 1, len_r), or clamp(k, 1, len_r) when d_ks is
 * NULL: a rank below 1 is the row's minimum, a rank above len_r its maximum.
 * A row with len_r == 0 writes the zero word.  1 <= k <= cols is checked on
 * the host either way.
 * Both arrays NULL: the outputs are bit-identical to the existing call's, and
 * d_cnt[r] = k.
 * Everything else is the wide-rows contract: asynchronous on the ctx stream, no
 * host synchronisation, no allocation after kth_ctx_reserve_wide_rows,
 * graph-capturable under the conditions written at kth_select_i32_async.  The
 * same ctx scratch, left as found (row histogram zero, nmn / mx zero), so var
 * calls, the existing wide calls of either width and any other call may
 * alternate on one ctx; kth_ctx_last_stats is unaffected;
 * kth_ctx_wide_rows_force forces their plan too.
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx or keys, no
 * output pointer, rows < 0, a bad cols, ld, k or kind.  rows == 0 returns
 * KTH_OK and launches nothing.  KTH_ENODEV without a GPU.
 * (csrc/kth_rows_wide.hpp "Ragged rows": a slice past its row's end and a row
 * with nothing to select.) */
int kth_select_wide_rows_var_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, int32_t *d_out);
int kth_select_wide_rows_var_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, float *d_out);
int kth_select_wide_rows_var_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, int kind, uint16_t *d_out);
int kth_topk_wide_rows_var_i32(kth_ctx *ctx, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, int32_t *d_vals,
                               int32_t *d_idx, int32_t *d_cnt);
int kth_topk_wide_rows_var_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, float *d_vals,
                               int32_t *d_idx, int32_t *d_cnt);
int kth_topk_wide_rows_var_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, int kind,
                               uint16_t *d_vals, int32_t *d_idx, int32_t *d_cnt);

/* --- synthetic inputs (bench / tests) --------------------------------------
 * Fills d_out[0..n) with the keys of global indices offset..offset+n of an
 * n_total-key input of family `dist` (oracle/kth_oracle.h enum ko_dist;
 * bit-identical to the CPU generator). */
int kth_fill_synthetic(kth_ctx *ctx, int32_t *d_out, int64_t n, int64_t offset, int64_t n_total,
                       int dist, uint64_t seed, int32_t param);

/* --- wide rows, top-p: the nucleus of each row of float logits -----------------
 * The filter of an LLM sampler that the var top-k leaves open: keep the
 * smallest set of the largest logits of a row whose softmax mass reaches p.
 * A nucleus is a weighted select -- the value at which the probability mass of
 * the larger keys reaches p, where a select looks for the count reaching k --
 * and is found by the wide rows' radix passes with a mass per bin, not by
 * sorting the row.  float32 rows (_f32) and float16 / bfloat16 rows (_k16,
 * kind KTH_K16_F16 or KTH_K16_BF16; the integer kinds are KTH_EINVAL).
 *
 * Per-row arrays and scalars.  d_lens is what it is in the var calls: len_r =
 * clamp(d_lens[r], 0, cols), NULL: cols; nothing at or past len_r of a row is
 * ever loaded.  d_ps, d_temps: device arrays of `rows` float32, 4-byte
 * aligned, read only on the device when the launches run; either may be NULL,
 * then the host scalar p / temp holds for every row.  temp must be finite and
 * > 0 (checked on the host either way); a device temps[r] that is not finite
 * or is <= 0 counts as 1.0.
 *
 * The row.  Order the row's first len_r keys by the library's float order,
 * largest first, ties by column -- the order of the var top-k with largest =
 * 1, which puts NaN on top.  Let m be the first key.
 * Weights.  w_i = 1 for a key equal to m in that order; w_i = 0 if m is +inf
 * or NaN, or if x_i is -inf; otherwise w_i = exp((x_i - m) / T_r).  S(j) = the
 * weight of the first j keys, Z = S(len_r).
 * The nucleus size n_r.  For 0 <= p_r < 1 the contract value is the least n >=
 * 1 with S(n) >= p_r * Z.  p_r < 0 counts as 0 (greedy: n_r = 1).  p_r >= 1 or
 * NaN: n_r = len_r exactly, no filter.  len_r == 0: n_r = 0.
 *
 * Tolerance.  The device evaluates a weight in float32 and sums weights as
 * 64-bit fixed point, rint(w * 2^39).  A call may therefore return any n
 * inside a band around the contract value:
 *     S(n) >= p * Z * (1 - eps)  and  (S(n - 1) < p * Z * (1 + eps) or n == 1),
 *     eps = 2^-16 + cols * 2^-39.
 * The first term bounds the float32 error of a weight.  Its exponent (x_i - m)
 * * (1 / T) carries three roundings, at most |d| * 3 * 2^-24 for d = (x_i - m)
 * / T; only |d| <= 27 matters, since exp(-27) is below the fixed point's
 * quantum 2^-39, which makes about 5e-6; a few ulp of expf (2^-22 or so) come
 * on top, and 2^-16 = 1.5e-5 covers both.  The second term is the quantisation
 * of `cols` weights to 2^-39 (half a quantum each, against Z >= 1), on both
 * sides of the compare.
 *
 * Determinism is part of the contract: a row's n_r and threshold depend only
 * on its keys, its length, p and T -- not on the plan (fused, any number of
 * slices, any group size), the load path or the run.  Weights are only ever
 * added as integers, which commute; no float atomic is used.  With cols <=
 * 2^24 a sum stays below 2^63.
 *
 * kth_nucleus_wide_rows_*: d_n[r] = n_r; d_thr[r] = the n_r-th key of that
 * order, the smallest kept logit: the bit pattern of an input element, a NaN
 * written canonical, the zero word for an empty row.  Either may be NULL, not
 * both.
 * kth_topp_wide_rows_*: a top-k cap and the nucleus jointly, both on the
 * unrenormalised row.  The outputs are bit for bit what the var top-k writes
 * with largest = 1, the same k and d_lens, and d_ks[r] = min(n_r, cap_r):
 * values and columns in column order, the padding (index -1, the zero word)
 * and d_cnt.  cap_r = clamp(d_ks[r], 0, k), or k when d_ks is NULL; 1 <= k <=
 * cols.  d_vals and d_idx may each be NULL, not both; d_cnt may be NULL.
 * "Top-k first, then top-p on the renormalised rest" is a different filter and
 * is not offered.
 *
 * Everything else is the wide-rows contract: asynchronous on the ctx stream, no
 * host synchronisation, no allocation once kth_ctx_reserve_topp_rows (which
 * covers the var top-k's scratch too) or an earlier call of that shape has
 * run, graph-capturable under the conditions written at kth_select_i32_async
 * -- a replay sees what d_ps, d_temps, d_lens and d_ks hold at replay time.
 * Scratch of its own in the ctx, left as found, groups of rows keeping it at
 * or below 32 MiB, so these calls and every other call may alternate on one
 * ctx; kth_ctx_last_stats is unaffected; kth_ctx_wide_rows_force forces this
 * plan too.
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx or keys, no
 * output pointer, rows < 0, a bad cols, ld, k, temp or kind, a NaN host p when
 * d_ps is NULL.  rows == 0 returns KTH_OK and launches nothing.  KTH_ENODEV
 * without a GPU.  (csrc/kth_rows_topp.hpp.) */
int kth_nucleus_wide_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                              const int32_t *d_lens, const float *d_ps, float p, const float *d_temps, float temp,
                              int32_t *d_n, float *d_thr);
int kth_nucleus_wide_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                              const int32_t *d_lens, const float *d_ps, float p, const float *d_temps, float temp,
                              int kind, int32_t *d_n, uint16_t *d_thr);
int kth_topp_wide_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                           const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                           const float *d_temps, float temp, float *d_vals, int32_t *d_idx, int32_t *d_cnt);
int kth_topp_wide_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                           const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                           const float *d_temps, float temp, int kind, uint16_t *d_vals, int32_t *d_idx,
                           int32_t *d_cnt);
int kth_ctx_reserve_topp_rows(kth_ctx *ctx, int64_t rows, int32_t cols);

/* --- wide rows, sampling: one token per row from the filtered distribution ------
 * The sampler's last step: draw one column of each row from the softmax of its
 * logits restricted to the top-k / top-p kept set.  The library holds no
 * generator: the caller fills d_us with one uniform number a row (torch.rand,
 * say), so that a graph replay draws afresh and a fixed u reproduces a token.
 * Drawing is the weighted select the nucleus is, run against the running mass;
 * the result is one int32 a row -- no rows * k output, no sort, no float sum
 * whose order the hardware picks.  float32 rows (_f32) and float16 / bfloat16
 * rows (_k16, kind KTH_K16_F16 or KTH_K16_BF16; the integer kinds are
 * KTH_EINVAL).
 *
 * The row, its order (largest first, ties by column), the weights w_i, S(j), Z,
 * len_r, p_r and T_r are exactly those of the top-p section above, with its
 * clamps and its rows where m is +inf or NaN; d_lens, d_ps, d_temps as there.
 *
 * Cap.  c_r = d_ks[r], or the host k when d_ks is NULL (d_ks: `rows` int32 on
 * the device, read when the launches run).  c_r <= 0 means no cap, the sampler
 * convention for "top-k off" -- on purpose not that of kth_topp_*, where k is
 * an output stride.  No upper bound is checked; a cap at or above len_r does
 * not bind.
 * Kept keys.  n_r = min(N_r, c_r), or N_r without a cap, where N_r is the
 * nucleus size kth_nucleus_wide_rows_* returns for the same keys, length, p and
 * T, bit for bit: the same fixed-point arithmetic, hence the same band.
 * d_cnt[r] = n_r; d_cnt may be NULL.
 * The number.  d_us is required: `rows` float32 on the device, 4-byte aligned,
 * read only on the device when the launches run.  u_r = d_us[r]; NaN or a
 * negative value counts as 0; a value of 1 or more selects the last kept key of
 * non-zero weight (the clamp below).
 * The token.  j_r is the least j >= 1 with S(j) > u_r * S(n_r); on the device,
 * t = min(S_fix(n_r), floor(u_r * S_fix(n_r)) + 1), computed in double by one
 * thread a row, then the least j with S_fix(j) >= t (S_fix: the 2^39 fixed-point
 * sums of the top-p section).  t <= S_fix(n_r), so j_r <= n_r by integer
 * arithmetic.  d_tok[r] = the column of the j_r-th key of the order -- a single
 * column, since ties are ordered by column.  An empty row: d_tok[r] = -1 and
 * d_cnt[r] = 0.  For u uniform on [0, 1) a kept key i is drawn with probability
 * w_i / S(n_r); a key outside the kept set is never drawn, nor is a key of
 * weight 0.
 *
 * Tolerance.  For the n returned, a call may return any j with 1 <= j <= n,
 *     S(j) >= A (1 - e)  and  (j == 1 or S(j - 1) <= A (1 + e)),
 *     A = u S(n) in exact arithmetic,  e = 2 * eps,  eps = 2^-16 + cols * 2^-39
 * (the eps of the top-p section).  Derivation: the device compares S_fix(j)
 * with u * S_fix(n).  Both sums carry the nucleus's weight error -- every
 * float32 weight is within a factor (1 +- 2^-16) of its exact value -- and they
 * stand on the two sides of the compare, so the relative errors add: 2 * 2^-16.
 * The quantisation of a weight to 2^-39 is absolute, at most cols * 2^-40 a
 * sum.  Where A <= 1 the first key decides (S(1) = 1 exactly on both sides, so
 * j = 1 is returned and admitted); where A > 1 an absolute cols * 2^-40 on
 * each side is at most a relative cols * 2^-39 in all, and the floor and the +1
 * of t are two quanta more, far inside the same term.  Together e = 2 * 2^-16 +
 * 2 * cols * 2^-39.
 *
 * Determinism is part of the contract: d_tok and d_cnt depend on the row's
 * keys, length, p, T, cap and u only -- not on the plan (fused, any number of
 * slices, any group size), the load path or the run.  Weights are only ever
 * added as integers; no float atomic is used.
 *
 * Everything else is the wide-rows contract: asynchronous on the ctx stream, no
 * host read of any device array, no allocation once
 * kth_ctx_reserve_sample_rows or an earlier call of that shape has run,
 * graph-capturable under the conditions written at kth_select_i32_async -- a
 * replay sees what d_us, d_ps, d_temps, d_lens and d_ks hold at replay time.
 * kth_ctx_wide_rows_force forces this plan too.  Scratch in the ctx (the top-p
 * calls' bins and a state of its own), left as found, groups of rows keeping
 * it at or below 32 MiB, so these calls and every other call may alternate on
 * one ctx; kth_ctx_last_stats is unaffected.
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx, keys, d_us
 * or d_tok, rows < 0, a bad cols, ld, temp or kind, a NaN host p when d_ps is
 * NULL.  rows == 0 returns KTH_OK and launches nothing.  KTH_ENODEV without a
 * GPU.  (csrc/kth_rows_sample.hpp.) */
int kth_sample_wide_rows_f32(kth_ctx *ctx, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                             const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                             const float *d_temps, float temp, const float *d_us, int32_t *d_tok, int32_t *d_cnt);
int kth_sample_wide_rows_k16(kth_ctx *ctx, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                             const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                             const float *d_temps, float temp, const float *d_us, int kind, int32_t *d_tok,
                             int32_t *d_cnt);
int kth_ctx_reserve_sample_rows(kth_ctx *ctx, int64_t rows, int32_t cols);

/* --- rows, sorted top-k: each row of a rows x k top-k output, best first ---------
 * Every per-row top-k above (kth_topk_rows_*, kth_topk_rows_k16, the wide and
 * ragged wide calls, kth_topp_wide_rows_*) writes its k keys in column order.
 * These calls put such an output in the order torch.topk(sorted=True) gives: a
 * stable sort, in place, of each row's values with their indices.
 *
 * Row.  Row r is d_vals[r*k .. r*k + k) and, when d_idx is given, d_idx[r*k ..
 * r*k + k).  Only its first n_r entries take part: n_r = clamp(d_cnt[r], 0, k),
 * or k when d_cnt is NULL (d_cnt: `rows` int32 on the device, read when the
 * launch runs, so a graph replay sees its current contents -- the d_cnt the
 * ragged and top-p calls write).  Entries [n_r, k), the ragged calls' padding,
 * are neither read nor written.
 * Order.  After the call the n_r entries stand best first: ascending in the
 * order key when largest == 0, descending when largest != 0.  The order key is
 * the signed order for int32, kth_f32_order_key for float32 (-0.0 < +0.0,
 * subnormals distinct, every NaN equal to every other NaN and above +inf) and
 * kth_k16_order_key(bits, kind) for the 16-bit kinds.
 * Ties.  The sort is stable: entries of equal order key keep their input order,
 * in either direction.  The top-k calls write in column order, so on their
 * output ties stand by ascending column, the tie rule of the whole library; the
 * same definition holds for d_idx == NULL and for any other payload.
 * Moves.  Values and indices are moved bit for bit: a NaN keeps its payload, and
 * d_idx is an opaque int32 payload that is never interpreted.  A row with n_r
 * <= 1 is not stored to at all.
 *
 * 1 <= k <= KTH_SORT_MAX_K.  One launch: k <= 64 packs 64 / k' rows into a
 * wavefront (k' the power of two at or above k) and exchanges across lanes;
 * larger k sorts a row a workgroup in LDS.  Asynchronous on the ctx stream,
 * device memory only, no host synchronisation, no allocation, no scratch, no
 * atomics; graph-capturable under the conditions written at
 * kth_select_i32_async.  No ctx buffer and not the last-call word is touched:
 * kth_ctx_last_stats is unaffected, and these calls may alternate with every
 * other call on one ctx.
 * KTH_EINVAL before any device work, outputs untouched: a NULL ctx or d_vals,
 * rows < 0, k < 1, k > KTH_SORT_MAX_K, a bad kind.  d_idx and d_cnt may be
 * NULL.  rows == 0 returns KTH_OK and launches nothing.  KTH_ENODEV without a
 * GPU.  (csrc/kth_rows_sort.hpp.) */
#define KTH_SORT_MAX_K 4096
int kth_sort_topk_rows_i32(kth_ctx *ctx, int32_t *d_vals, int32_t *d_idx, int64_t rows, int32_t k,
                           const int32_t *d_cnt, int largest);
int kth_sort_topk_rows_f32(kth_ctx *ctx, float *d_vals, int32_t *d_idx, int64_t rows, int32_t k,
                           const int32_t *d_cnt, int largest);
int kth_sort_topk_rows_k16(kth_ctx *ctx, uint16_t *d_vals, int32_t *d_idx, int64_t rows, int32_t k,
                           const int32_t *d_cnt, int largest, int kind);

/* --- sharded selection, one process per GPU (TODO-kth-problem-cgm.c:76-278) --
 * The CGM rounds (local median :125-131, Gather :135-136, weighted median
 * :139-165, Bcast :168, 3-way count :171-185, Allreduce :190, discard
 * :194-225, final Gatherv + sort :242-278) become:
 *   every rank samples its shard -> the samples are all-gathered -> every rank
 *   derives the same window -> one streaming pass per shard (counts, local
 *   candidates and their first digit) -> per-rank histograms are all-reduced
 *   (uint64 SUM) after each step -> every rank picks the same digit from the
 *   same reduced histogram.
 * Collectives per selection: one all-gather and, when the window is at most
 * 2^24 key values wide (uniform 2^33 half-range keys: ~2^23.3), two
 * all-reduces; wider windows three; the exact fallback after a window miss or
 * a candidate overflow four; a selection decided by the window's counts alone
 * two (the second all-reduce carries an empty slot).
 * The host owns the collectives (RCCL through torch.distributed in
 * kselect/dist.py, or MPI/RCCL from C); these entry points only enqueue the
 * per-rank device work on the ctx stream.  The host waits once per selection:
 * kth_dist_level(1) waits for level 0's kernel (the device has the all-reduce
 * after it still queued) to learn how many levels follow.
 *
 * d_slots: caller-owned device memory of 3 * KTH_STATS_WORDS uint64 words,
 * bound by kth_dist_begin for one selection.  kth_dist_scan and
 * kth_dist_level return the index (0..2) of the slot the caller must
 * all-reduce (SUM) in place across ranks before the next call, or
 * KTH_DIST_DONE; every rank makes the same sequence of calls:
 *   kth_dist_begin   bind slots, set (n_total, k)
 *   kth_dist_sample  local sample of s_local keys of the shard -> d_sample
 *                    (order-preserving uint32 keys); caller all-gathers
 *   kth_dist_window  window from the gathered sample of s_total keys
 *   kth_dist_scan    streaming pass over the shard            -> slot
 *   kth_dist_level   level = 0, 1, 2, ... -> slot, until it returns
 *                    KTH_DIST_DONE (at most KTH_DIST_MAX_LEVELS slots)
 *   kth_dist_result  writes the k-th smallest of the union of all shards to
 *                    *d_out (device) */
#define KTH_STATS_WORDS (8 + 2 * 2048)
#define KTH_DIST_DONE 3
#define KTH_DIST_MAX_LEVELS 3
/* Deprecated (round-4 API): callers loop kth_dist_level until KTH_DIST_DONE;
 * kept so that code written against the old name still builds. */
#define KTH_DIST_LEVELS KTH_DIST_MAX_LEVELS
int kth_dist_begin(kth_ctx *ctx, uint64_t *d_slots, int64_t n_total, int64_t k);
int kth_dist_sample(kth_ctx *ctx, const int32_t *d_keys, int64_t n_local, uint32_t *d_sample,
                    int64_t s_local);
int kth_dist_window(kth_ctx *ctx, const uint32_t *d_sample, int64_t s_total);
int kth_dist_scan(kth_ctx *ctx, const int32_t *d_keys, int64_t n_local);
int kth_dist_level(kth_ctx *ctx, const int32_t *d_keys, int64_t n_local, int level);
int kth_dist_result(kth_ctx *ctx, int32_t *d_out);
/* Optional, right after level 0's slot is all-reduced and before
 * kth_dist_level(ctx, .., 1): enqueue the result as if level 0 were the last
 * (it is when the window is at most 2^24 values wide or decided by its counts),
 * so the device need not wait for the host's look at level 0's status.  If
 * more levels follow, it writes nothing and the protocol goes on; the closing
 * kth_dist_result with the same d_out is then the only launch that writes (and
 * costs nothing when the early one finished the select). */
int kth_dist_result_early(kth_ctx *ctx, int32_t *d_out);
/* The whole step sequence above in ONE call, for a caller that holds an RCCL
 * communicator (one process per GPU): kth_dist_begin .. kth_dist_result with
 * the all-gather of the samples and the slot all-reduces as ncclAllGather /
 * ncclAllReduce (uint64 SUM) on the ctx stream, the early result before
 * level 1 when `early` is nonzero.  nccl_all_reduce / nccl_all_gather are the
 * caller's ncclAllReduce / ncclAllGather entry points, so that the
 * communicator `nccl_comm` (an ncclComm_t of `world` ranks) and the calls come
 * from one RCCL copy.  d_sample: s_local uint32 words, d_gathered: world *
 * s_local; every rank passes the same (n_total, k, s_local).  The host waits
 * once, for level 0's status, as in the step sequence; the answer lands in
 * *d_out (device).  Replaces the per-step host round trips of a scripted
 * caller (kselect.dist uses it over RCCL). */
int kth_dist_select_rccl(kth_ctx *ctx, void *nccl_all_reduce, void *nccl_all_gather, void *nccl_comm, int world,
                         const int32_t *d_keys, int64_t n_local, int64_t n_total, int64_t k, uint64_t *d_slots,
                         uint32_t *d_sample, uint32_t *d_gathered, int64_t s_local, int32_t *d_out, int early);
/* Sample size for n keys (the single-GPU rule: min(2^20, n/64), a multiple
 * of 64).  Sharded callers take about kth_dist_sample_size(n_total) / P keys
 * per rank (a multiple of 64, at least 64), so that the all-gathered sample
 * has the single-GPU size. */
int64_t kth_dist_sample_size(int64_t n);
/* Sampler layout (diagnostics and tests): a sample of s keys from n is read as
 * ceil(s / C) chunks of C = kth_sample_chunk() consecutive keys, chunk c at
 * key c * (n / ceil(s / C)); the last chunk holds the remaining s mod C keys. */
int kth_sample_chunk(void);
/* Window half-width in sample standard deviations: the window ranks in a
 * sample of s keys for rank k of n are p*s -+ (z*sqrt(s*p*(1-p)) + 2), p = k/n
 * (KTH_WINDOW_Z overrides the built-in 5.0). */
double kth_window_z(void);
/* Candidate-buffer capacity (keys) of a streaming pass over n_local keys:
 * max(2^20, n_local / 32); more candidates than this on a rank set its
 * overflow count and the selection takes the exact fallback levels. */
int64_t kth_dist_cand_capacity(int64_t n_local);
/* Early-window slack of the sample phase, in 1/64ths: after each sample digit,
 * the window stops at the picked bins' edges when those hold at most
 * slack/64 times the sample keys the exact window would (96 = 1.5; the
 * KTH_HEAD_SLACK environment variable changes a new ctx's value, 0 = off). */
int kth_window_slack64(void);

/* --- sharded selection, one process driving several GPUs ---------------------
 * Replaces TODO-kth-problem-cgm.c:81-278 (block partition + Scatterv, the
 * weighted-median rounds, final Gatherv + rank-0 sort) for a caller holding one
 * shard per GPU in a single process: the kth_dist_* steps for every device,
 * with the collectives as grouped RCCL calls over communicators from
 * ncclCommInitAll (RCCL is dlopen'ed at first use: the librccl.so.1 already in
 * the process, else the system one; KTH_ECOMM if neither loads).
 * Local transport: ngpu > 1 copies of ONE device id (at most 64) put every
 * shard on that device with no RCCL: the same per-shard steps on one shared
 * stream, the samples gathered in place, each all-reduce a device-side sum of
 * the shards' slots (P shards of a 2^33-key input on one GPU).
 *   kth_sharded_create      devices[0..ngpu) distinct (RCCL), or all equal
 *                           (local); one ctx per shard, one stream and
 *                           communicator per device
 *   kth_sharded_select_i32  shard i = shards[i][0..shard_n[i]) in device
 *                           devices[i]'s memory; k-th smallest (1-based) of the
 *                           union -> *out (host).  Synchronous; the shards must
 *                           be complete when it is called (it does not order
 *                           against the caller's streams).  Shards of fewer
 *                           than 64 keys: the union is copied to device 0 and
 *                           selected there.  Any shard sizes are exact;
 *                           balanced shards (n/P + (i < n%P)) are the fast case.
 *   kth_select_i32_sharded  one-shot form; each shard's device is taken from
 *                           its pointer (device memory only), the handle is
 *                           cached per host thread for the same device list. */
typedef struct kth_sharded kth_sharded;
int kth_sharded_create(const int *devices, int ngpu, kth_sharded **out);
int kth_sharded_destroy(kth_sharded *h);
int kth_sharded_select_i32(kth_sharded *h, const int32_t *const *shards, const int64_t *shard_n, int64_t k,
                           int32_t *out);
int kth_select_i32_sharded(const int32_t *const *dev_shards, const int64_t *shard_n, int ngpu, int64_t k,
                           int32_t *out);
/* Per-shard sample sizes of kth_sharded_select_i32: about
 * kth_dist_sample_size(n_total) keys in all, split in proportion to the shard
 * sizes, each a multiple of 64, at least 64 and at most the shard rounded down
 * to 64.  Writes s_dev[0..P), returns their sum (KTH_EINVAL for bad input).
 * Host-only arithmetic (no device needed). */
int64_t kth_sharded_sample_split(const int64_t *shard_n, int P, int64_t *s_dev);
/* Diagnostics: host microseconds the last kth_sharded_select_i32 on h spent
 * enqueueing device work and collectives for every device (from its entry to
 * the last kth_dist_result enqueue; the wait for the answer excluded); -1 for
 * a NULL handle. */
double kth_sharded_enqueue_us(const kth_sharded *h);

#ifdef __cplusplus
}
#endif
#endif /* KTH_H */
