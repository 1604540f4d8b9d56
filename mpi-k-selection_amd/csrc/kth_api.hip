// kth_api.hip -- extern "C" boundary of libkth.so (include/kth.h).
//
// Host-side orchestration of the kernels in kth_kernels.hip: context and
// scratch management, path choice, the per-path launch sequences, timing
// events, and the per-rank steps of the sharded protocol.  No host
// synchronisation inside a select except in the synchronous wrappers, no
// allocation once a ctx is reserved, no CPU fallback: without a device every
// compute entry point returns KTH_ENODEV.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kth.h"
#include "kth_internal.h"
#include "kth_kernels.hip"
#include "kth_topk.hpp"
#include "kth_k16.hpp"
#include "kth_topk16.hpp"

using kth::SelState;
using kth::StepArgs;
using kth::u64;

namespace {

constexpr int64_t SMALL_N = 16384;           // LDS path
constexpr int64_t RADIX_MAX_N = 1ll << 22;   // radix path up to here, window path above
constexpr int64_t SAMPLE_MAX = 1ll << 20;    // sample keys (single GPU / total over ranks)
constexpr double WINDOW_Z = 5.0;             // window half-width in sample standard deviations (two-sided miss 5.7e-7)
// KTH_WINDOW_Z overrides it (design exploration); read once
double window_z() {
    static const double z = [] {
        const char *e = getenv("KTH_WINDOW_Z");
        const double v = e ? atof(e) : 0.0;
        return v > 0.0 ? v : WINDOW_Z;
    }();
    return z;
}
constexpr int LEVEL_GRID_MAX = 1024;
constexpr int POST_DENSE_GRID = 256;  // the candidates need ~100 dense WGs; the rare fallback streams the input with 256
constexpr int64_t HEAD_PER_WG = 16 * 1024;  // sample keys a k_head workgroup: 16 chunks of 1024
constexpr int HEAD_GRID_MAX = 64;  // k_head workgroups at most: 2^20 sample keys / (16 chunks of 1024 a workgroup)
static_assert(HEAD_GRID_MAX == SAMPLE_MAX / HEAD_PER_WG, "k_head's grid covers the largest sample");
int gather_grid(u64 nchunks) {
    const u64 per_wg = (u64)(kth::DENSE_BLK / kth::WAVE) * kth::GATHER_BATCH;  // chunks per workgroup round
    return (int)std::max<u64>(1, (nchunks + per_wg - 1) / per_wg);
}
constexpr size_t ISLOT_WORDS = 3 * (size_t)kth::STATS_WORDS + 2;  // 3 slots + cand_count + pad
// after the islots, in the same allocation: k_head's and k_finish's level
// slots and PreHist (zero between selects: k_finish leaves them so), then the
// grid-barrier words (never cleared by a select: the barrier resets itself)
constexpr size_t HSLOT_OFF = ISLOT_WORDS;
constexpr size_t HSLOT_WORDS = (size_t)kth::HEAD_LEVELS * kth::STATS_WORDS;
constexpr size_t FSLOT_OFF = HSLOT_OFF + HSLOT_WORDS;
constexpr size_t FSLOT_WORDS = (size_t)kth::FIN_LEVELS * kth::STATS_WORDS;
constexpr size_t PRE_OFF = FSLOT_OFF + FSLOT_WORDS;  // PreHist (u32 words)
static_assert(kth::PRE_WORDS % 4 == 0 && PRE_OFF % 2 == 0, "k_finish clears PreHist in 16-byte words");
constexpr size_t ZERO_WORDS = PRE_OFF + (size_t)kth::PRE_WORDS / 2;  // (in u64 words)
constexpr size_t BAR_OFF = ZERO_WORDS;
constexpr size_t TAIL_OFF = BAR_OFF + kth::BAR_WORDS / 2;  // k_finish's tail keys (FIN_LDS_KEYS u32)
constexpr size_t SLOT_ALLOC_WORDS = TAIL_OFF + kth::FIN_LDS_KEYS / 2;
static_assert(kth::BAR_TAIL % 2 == 0, "the tail word is a u64");
constexpr u64 FIN_SPARSE_PER_WG = (u64)kth::DENSE_BLK * kth::FIN_UNROLL * 4;  // one k_finish tile
constexpr double HEAD_SLACK = 1.5;  // k_head early window (EarlyWindow); KTH_HEAD_SLACK overrides, 0 = off
static_assert(KTH_STATS_WORDS == kth::STATS_WORDS, "include/kth.h slot size");
constexpr int MAX_EVENTS = 4 * 2048;
constexpr u64 TK_STAGE_MAX_FRAC = 16;  // staged top-k (k_main<5/6>) for k <= n / 16
constexpr int TK5_SPLIT = 4;            // workgroups per k_main workgroup in k_tk5_count / k_tk5_write (window-parallel)
constexpr int COOP_BACKOFF = 64;        // synchronous selects on the per-level path after a grid-barrier timeout
constexpr uint64_t DSCAN_PER_WG = 1ull << 16;  // candidates per workgroup of the sharded scan's first-digit histogram
// A rank's set of a multi-rank call (kth_select_multi_*), in one allocation:
// its three slots and candidate count, laid out as the ctx's islots, then its
// own sample-phase slots (its k_finish clears them, as the ctx's)
constexpr size_t MSET_HSLOT_OFF = ISLOT_WORDS;
constexpr size_t MSET_WORDS = MSET_HSLOT_OFF + HSLOT_WORDS;
static_assert(KTH_MULTI_MAX_RANKS == kth::MULTI_MAX, "include/kth.h rank limit");
constexpr int MULTI_VARIANTS = 3;  // k_main_multi<2 / 4 / 8>
// 16-bit keys (kth_k16.hpp): the sample histogram (u32 bins), then a set per rank
constexpr size_t K16_SHIST_WORDS = kth::K16_VALUES / 2;  // (in u64 words)
constexpr size_t K16_BUF_WORDS = K16_SHIST_WORDS + (size_t)KTH_MULTI_MAX_RANKS * kth::K16_RANK_WORDS;
constexpr size_t K16_HIST_LDS = (size_t)kth::K16_VALUES * 2;
static_assert(KTH_K16_I16 == 0 && KTH_K16_U16 == 1 && KTH_K16_F16 == 2 && KTH_K16_BF16 == 3, "kth_k16.hpp's key kinds");
static_assert(KTH_PATH_K16 == 5 && KTH_PATH_K16_FALLBACK == 6, "kth_k16.hpp's paths");

#define HIP_TRY(x)                                                                                    \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            if (getenv("KTH_DEBUG")) fprintf(stderr, "kth: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return KTH_EHIP;                                                                          \
        }                                                                                             \
    } while (0)

#define KTH_TRY(x)              \
    do {                        \
        int r_ = (x);           \
        if (r_ != KTH_OK) return r_; \
    } while (0)

// A device scratch buffer of a ctx: the pointer and its size in elements.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    u64 count = 0;

    // At least `want` elements.  Never shrinks; on failure the buffer is empty.
    int reserve(u64 want) {
        if (count >= want) return KTH_OK;
        (void)hipDeviceSynchronize();  // in-flight work may still use the old buffer
        release();
        if (hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return KTH_ENOMEM;
        }
        count = want;
        return KTH_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
};
template <typename... Bufs>
void release_all(Bufs &...bufs) {
    (bufs.release(), ...);
}

}  // namespace

struct kth_ctx {
    int device = 0;
    // streaming-pass workgroups per k_main<TF, F32> variant, [key kind][TF]
    // (float32 keys have no TF 5 / 6: those entries stay 0)
    int main_grid[2][7] = {};
    int multi_grid[2][MULTI_VARIANTS] = {};  // ... per k_main_multi<2 / 4 / 8, F32>, [key kind][variant]
    int main_wg_per_cu = 0;  // KTH_MAIN_WG_PER_CU: k_main workgroups a CU for every variant (0 = from its registers and LDS)
    bool fault_topk_rank = false;  // KTH_HOOK_FAULT_TOPK_RANK (tests): top-k selects a wrong rank on purpose
    bool fault_barrier = false;    // KTH_HOOK_FAULT_BARRIER (tests): the grid barriers report a timeout
    bool fault_once = false;       // (value 2) only the next cooperative launch does
    bool topk_stage = true;        // staged top-k (k_main<5/6>); KTH_TOPK_STAGE=0 turns it off
    u64 topk_seg_cap = 0;          // KTH_HOOK_TOPK_SEG_CAP (tests): entries per staging segment (0 = sized from n)
    u64 sparse_per_wg = 0;  // keys per workgroup of the sparse levels (KTH_SPARSE_PER_WG; 0 = default)
    int post_dense_grid = POST_DENSE_GRID;    // decide level after the pass (KTH_POST_DENSE_GRID)
    int post_sparse_grid = LEVEL_GRID_MAX;    // candidate levels (KTH_POST_SPARSE_GRID)
    bool coop = true;          // window / radix paths as k_head + k_main + k_finish (KTH_COOP=0: per-level launches)
    bool coop_wanted = true;   // coop as configured (env, LDS, residency); coop may be off for a while after a timeout
    int coop_backoff = 0;      // synchronous selects left on the per-level path after a grid-barrier timeout
    bool coop_resident = true; // the cooperative grids fit the device at once (occupancy check at ctx creation)
    int fin_grid = 256;        // k_finish workgroups (one per CU; KTH_FIN_GRID)
    uint32_t head_slack64 = (uint32_t)(HEAD_SLACK * 64);
    uint32_t head_abs_div = 1024;  // plain select: early-window floor s / head_abs_div sample keys (KTH_HEAD_ABS; 0 = off)
    bool pre_hist = true;      // k_main<0> histograms the candidates' first digit for k_finish (KTH_PRE_HIST=0: off)
    bool group = true;         // ... and writes them grouped by it, with a directory, for k_finish's gather (KTH_GROUP=0: off)
    bool finish_slices = false;  // KTH_HOOK_FINISH_SLICES (tests): k_finish ignores the directory and takes the slice tail
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    SelState *st = nullptr;   // 2 states (ping-pong)
    u64 *islots = nullptr;    // ISLOT_WORDS
    DevBuf<uint32_t> sample;
    DevBuf<uint32_t> cand;
    DevBuf<uint32_t> gdir;       // k_main<0>'s group directory: a row per workgroup (single-GPU window path)
    DevBuf<uint32_t> cand_rows;  // k_main<3/4>: each candidate's 1024-key row (top-k)
    // k_main<5/6> (top-k): per-wave segments of staged keys + positions, per wave-row counts
    DevBuf<int32_t> tk_segv;
    DevBuf<uint8_t> tk_segp;
    DevBuf<uint32_t> tk_wcnt;
    DevBuf<uint32_t> tk_wstart;  // staged top-k: entries before each window, per wave
    kth::TkSeg tk_seg{};  // the segments of the next launch_main<5/6>
    DevBuf<int32_t> staging;
    DevBuf<u64> topk;  // top-k chunk counts, bases, [need, error]
    int32_t *d_status = nullptr;  // [answer, error, the last-call word (LastCall), -]
    int32_t *h_status = nullptr;  // pinned
    SelState *h_state = nullptr;  // pinned
    int last_state = -1;          // the state the last single select enqueued here ends in (top-k reads it)
    uint32_t multi_tag = 0;       // while a multi call sends its ranks through the single select's launches: its LastCall word
    // multi-rank calls: a set per rank (states, slots, candidates), [answer, error] per rank
    DevBuf<SelState> mstate;  // 2 per rank
    DevBuf<u64> mslots;       // MSET_WORDS per rank, zero between calls
    DevBuf<uint32_t> mcand;   // per rank: the candidates, mcand_stride words apart
    int32_t *d_mstatus = nullptr, *h_mstatus = nullptr;  // 2 words per rank (device / pinned)
    int multi_m = 0;          // ranks of the last multi call (0: none yet)
    uint32_t multi_word = 0;  // ... and its LastCall word (form, key kind): the rank map below belongs to that call
    int multi_set[KTH_MULTI_MAX_RANKS] = {};  // ... and the set that resolved each (duplicates share one)
    u64 multi_cap = 0;        // ... and its per-rank candidate capacity
    bool multi_dirty = false; // a multi call was cut short or failed: re-zero mslots
    // 16-bit keys: the sample histogram and the ranks' sets, their states; the
    // call's rank -> set map and status words are the multi call's
    DevBuf<u64> k16;
    DevBuf<kth::K16State> k16st;
    int k16_grid[3] = {};     // k16_main<0 / 1 / 2>'s workgroups
    bool k16_ready = false;   // grids sized, k16_hist's LDS granted
    bool k16_dirty = false;   // a k16 call was cut short or failed: re-zero its scratch
    bool k16_miss = false;    // KTH_HOOK_K16_MISS (tests): the sample phase publishes an empty window
    // kth_topk_k16: k16_main_tf<0 / 1 / 2>'s workgroups; the last call's count-pass tiles (0: none yet)
    int k16_tf_grid[3] = {};
    u64 tk16_tiles = 0;
    DevBuf<u64> tk16_nread;        // ... and the tiles its count pass loaded from the input
    bool k16_topk_noskip = false;  // KTH_HOOK_K16_TOPK_NOSKIP (tests): the count pass ignores the streaming pass's flags
    // wide rows, split form: a histogram and a state per row of a group (zero between
    // calls but for the state's overwritten words), (better, equal) per slice
    DevBuf<uint32_t> wide_hist;
    DevBuf<kth::WideState> wide_state;
    DevBuf<uint32_t> wide_cnt;
    bool wide_dirty = false;   // a wide-rows sequence was cut short: re-zero its scratch
    int32_t wide_force_slices = 0, wide_force_group = 0;  // kth_ctx_wide_rows_force (0: automatic)
    // wide rows, top-p: a row's masses, counts and state (split form; zero between calls but
    // for the state's overwritten words), and the ranks kth_topp_* hands to the var top-k
    DevBuf<u64> tp_mass;
    DevBuf<uint32_t> tp_cnt;
    DevBuf<kth::TpState> tp_state;
    DevBuf<int32_t> tp_rank;
    bool tp_dirty = false;     // a top-p sequence was cut short: re-zero its scratch
    // wide rows, sampling (split form): a state per row of a group (its accumulating words zero
    // between calls) and the equal keys of every slice; the bins are the top-p calls'
    DevBuf<kth::SmState> sm_state;
    DevBuf<uint32_t> sm_loc;
    bool sm_dirty = false;     // a sample sequence was cut short: re-zero its state
    // timing: event pairs around the streaming pass and around whole selects
    bool timing = false;
    std::vector<hipEvent_t> ev_main, ev_total;
    int main_used = 0, total_used = 0;
    bool dirty = false;  // a launch sequence was cut short: re-zero the slots
    bool count_kept = false;  // a per-level top-k select left the candidate count: kth_topk_* clears it after k_topk_cands
    bool dist_zero = false;  // sharded: the bound slots still need clearing
    bool dist_open = false;  // sharded: begun, kth_dist_result not yet enqueued
    bool dist_coop_window = false;  // sharded: the window came from k_head (state carried, no pick left)
    bool counts_left = false;  // a cooperative window select left islot(1) / cand_count for the next k_head to clear
    // KTH_STAMPS=1 diagnostics: per-launch [WG][8] wall-clock stamps, dumped after each select
    u64 *stamps = nullptr;
    int stamp_next = 0;
    // sharded protocol
    u64 *uslots = nullptr;
    int64_t dist_n = 0, dist_k = 0, dist_cap = 0;
    int dist_level_next = 0;   // the next kth_dist_level call's level (-1: none expected)
    u64 dscan_per_wg = DSCAN_PER_WG;  // k_dscan_hist keys per workgroup (KTH_DSCAN_PER_WG)
    int dist_levels = -1;      // level calls that return a slot (from level 0's DistStatus; -1: unknown yet)
    int dist_result_slot = -1; // the slot the last level accumulated into (kth_dist_result reads it)
    int32_t *dist_early_out = nullptr;  // kth_dist_result_early's answer buffer this select (null: none)
    uint32_t *h_dist = nullptr;  // DistStatus, host-visible (pinned, mapped), written by level 0's k_dlevel
    uint32_t *d_dist = nullptr;  // ... its device address
    hipEvent_t ev_dist = nullptr;  // recorded after level 0
    uint32_t dist_tag = 0;     // level 0 calls so far (the DistStatus tag)
};

namespace {

// (islot(i) in the comments below: slot i of the three in c->islots)
u64 *cand_count(kth_ctx *c) { return c->islots + 3 * (size_t)kth::STATS_WORDS; }

// LastCall: which selection ran last on the ctx, for kth_ctx_last_stats and
// kth_ctx_multi_stats -- a word on the device, written by the last launch of
// every selection, because the host's own record only knows the calls it
// enqueued: a replayed graph runs a call again without the host.  The form, the
// key kind and where the final state lies: a single select's state (0 / 1), the
// set of a multi or 16-bit call's last rank.
enum : uint32_t { LAST_NONE = 0, LAST_SINGLE = 1, LAST_MULTI = 2, LAST_K16 = 3 };
struct LastCall {
    uint32_t form;
    bool f32;
    int index, k16_kind;
};
uint32_t last_word(uint32_t form, bool f32, int index, int k16_kind = 0) {
    return form | (f32 ? 4u : 0u) | (uint32_t)index << 4 | (uint32_t)k16_kind << 8;
}
LastCall last_of_word(uint32_t w) { return LastCall{w & 3u, (w & 4u) != 0, (int)(w >> 4 & 15u), (int)(w >> 8 & 3u)}; }
uint32_t *d_last(kth_ctx *c) { return reinterpret_cast<uint32_t *>(c->d_status + 2); }
// a single select that ends in state `state` (as a rank of a multi call: that call's word)
template <bool F32>
uint32_t single_word(const kth_ctx *c, int state) {
    return c->multi_tag ? c->multi_tag : last_word(LAST_SINGLE, F32, state);
}

int set_device(kth_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    return KTH_OK;
}

u64 cand_capacity(int64_t n) { return std::max<u64>(1ull << 20, (u64)n / 32); }

int64_t sample_size(int64_t n) {
    int64_t s = (n / 64) & ~int64_t(63);
    return std::min<int64_t>(SAMPLE_MAX, std::max<int64_t>(s, 64));
}

// rows: also a row per candidate (k_main<3/4>), as many as there are candidate
// slots (the kernels bound both by cand.count)
int reserve_cand(kth_ctx *c, int64_t n, bool rows = false) {
    KTH_TRY(c->cand.reserve(cand_capacity(n)));
    return rows ? c->cand_rows.reserve(c->cand.count) : KTH_OK;
}

// Is the plain pass's group directory in use, and its words (a row per
// workgroup of the larger of k_main<0>'s two grids)?
bool grouping(const kth_ctx *c) { return c->coop && c->pre_hist && c->group; }
u64 gdir_words(const kth_ctx *c) {
    return (u64)std::max(c->main_grid[0][0], c->main_grid[1][0]) * (kth::GDIR_ROW_BYTES / 4);
}

// The window path's scratch: the sample, the candidates and the group directory.
int reserve_window(kth_ctx *c, int64_t n) {
    KTH_TRY(c->sample.reserve((u64)sample_size(n)));
    if (grouping(c)) KTH_TRY(c->gdir.reserve(gdir_words(c)));
    return reserve_cand(c, n);
}

// Window ranks in a sample of s keys for rank k of n: +-Z sample sigmas.
void window_ranks(int64_t n, int64_t k, int64_t s, u64 *r_lo, u64 *r_hi) {
    const double p = (double)k / (double)n;
    const double r = p * (double)s;
    const double sig = std::sqrt(std::max(1.0, (double)s * p * (1.0 - p)));
    const double z = window_z();
    const double lo = std::floor(r - z * sig - 2.0), hi = std::ceil(r + z * sig + 2.0);
    *r_lo = lo < 1.0 ? 0 : (u64)lo;                       // 0 = no lower bound
    *r_hi = hi > (double)s ? (u64)s + 1 : (u64)std::max(1.0, hi);  // s+1 = no upper bound
}

constexpr int STAMP_LAUNCHES = 16, STAMP_WGS = 4096;
u64 *next_stamps(kth_ctx *c) {
    if (!c->stamps || c->stamp_next >= STAMP_LAUNCHES) return nullptr;
    return c->stamps + (size_t)(c->stamp_next++) * STAMP_WGS * 8;
}

// Per launch of the last select: WGs, and mean / max of each stamp relative to
// the launch's first entry, then the gap to the next launch (microseconds).
void dump_stamps(kth_ctx *c) {
    if (!c->stamps) return;
    std::vector<u64> h((size_t)STAMP_LAUNCHES * STAMP_WGS * 8);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h.data(), c->stamps, h.size() * 8, hipMemcpyDeviceToHost);
    u64 prev_end = 0;
    for (int l = 0; l < c->stamp_next; ++l) {
        const u64 *b = h.data() + (size_t)l * STAMP_WGS * 8;
        u64 t0 = ~0ull, tend = 0;
        int nwg = 0;
        for (int w = 0; w < STAMP_WGS; ++w)
            if (b[w * 8]) {
                nwg++;
                t0 = std::min(t0, b[w * 8]);
                for (int i = 0; i < 8; ++i) tend = std::max(tend, b[w * 8 + i]);
            }
        if (!nwg) continue;
        fprintf(stderr, "kth-stamps launch %d wgs %4d gap %7.2f |", l, nwg, prev_end ? (t0 - prev_end) / 100.0 : 0.0);
        for (int i = 0; i < 8; ++i) {
            double sum = 0, mx = 0;
            int cnt = 0;
            for (int w = 0; w < STAMP_WGS; ++w)
                if (b[w * 8] && b[w * 8 + i]) {
                    const double d = (b[w * 8 + i] - t0) / 100.0;
                    sum += d;
                    mx = std::max(mx, d);
                    cnt++;
                }
            if (cnt) fprintf(stderr, " p%d %6.2f/%6.2f", i, sum / cnt, mx);
        }
        fprintf(stderr, "\n");
        if (nwg >= 512) {  // end times (p5): percentiles over workgroups, and per blockIdx % 8
            std::vector<double> e;
            std::vector<double> ex[8];
            for (int w = 0; w < STAMP_WGS; ++w)
                if (b[w * 8] && b[w * 8 + 5]) {
                    const double d = (b[w * 8 + 5] - t0) / 100.0;
                    e.push_back(d);
                    ex[w % 8].push_back(d);
                }
            std::sort(e.begin(), e.end());
            if (!e.empty()) {
                auto pc = [&](double q) { return e[std::min(e.size() - 1, (size_t)(q * (double)e.size()))]; };
                fprintf(stderr, "kth-stamps   p5 pct: 1%% %.1f 10%% %.1f 25%% %.1f 50%% %.1f 75%% %.1f 90%% %.1f 99%% %.1f max %.1f\n",
                        pc(0.01), pc(0.10), pc(0.25), pc(0.50), pc(0.75), pc(0.90), pc(0.99), e.back());
                fprintf(stderr, "kth-stamps   p5 mean by wg%%8:");
                for (int x = 0; x < 8; ++x) {
                    double sm = 0;
                    for (double d : ex[x]) sm += d;
                    fprintf(stderr, " %.1f", ex[x].empty() ? 0.0 : sm / ex[x].size());
                }
                fprintf(stderr, "\n");
            }
        }
        if (nwg >= 512) {  // streaming pass: finish times (p3) by blockIdx % 8 (XCD under round-robin dispatch)
            for (int x = 0; x < 8; ++x) {
                double sum = 0, mn = 1e30, mx = 0;
                int cnt = 0;
                for (int w = x; w < STAMP_WGS; w += 8)
                    if (b[w * 8] && b[w * 8 + 3]) {
                        const double d = (b[w * 8 + 3] - t0) / 100.0;
                        sum += d;
                        mn = std::min(mn, d);
                        mx = std::max(mx, d);
                        cnt++;
                    }
                if (cnt) fprintf(stderr, "kth-stamps   wg%%8=%d p3 min %7.2f mean %7.2f max %7.2f\n", x, mn, sum / cnt, mx);
            }
        }
        prev_end = tend;
    }
    (void)hipMemsetAsync(c->stamps, 0, h.size() * 8, c->stream);
    c->stamp_next = 0;
}

// What one rank's selection owns beside its histogram slots: the two states
// and the candidates.  The ctx's own set serves every single select; a
// multi-rank call has one set per rank.
struct RankSet {
    SelState *st;     // 2 states (ping-pong)
    u64 *cand_count;
    uint32_t *cand;
    u64 cap;          // candidate buffer capacity (keys)
};
RankSet own_set(kth_ctx *c) { return RankSet{c->st, cand_count(c), c->cand.p, c->cand.count}; }

StepArgs step(kth_ctx *c, const RankSet &r, int adv, int st_in, int st_out, const u64 *in, u64 *acc, u64 *zero) {
    StepArgs a;
    memset(&a, 0, sizeof a);
    a.stamps = next_stamps(c);
    a.st_in = st_in >= 0 ? r.st + st_in : nullptr;
    a.st_out = r.st + st_out;
    a.stats_in = in;
    a.stats_acc = acc;
    a.stats_zero = zero;
    a.adv = adv;
    a.cand = r.cand;
    a.cand_count = r.cand_count;
    a.cap = r.cap;
    return a;
}
StepArgs step(kth_ctx *c, int adv, int st_in, int st_out, const u64 *in, u64 *acc, u64 *zero) {
    return step(c, own_set(c), adv, st_in, st_out, in, acc, zero);
}

// A chain of level steps over three rotating histogram slots and the two
// states.  Step l reads state (l + 1) % 2 and writes state l % 2; it reads slot
// l % 3, adds into slot (l + 1) % 3 and clears slot (l + 2) % 3 (so every slot
// is zero again before it is added into).  An ADV_INIT_* step starts a
// selection and reads no state.  `use` names the slots a step's kernel gets
// (the others are nullptr): the first step has no histogram to read, a result
// step adds and clears nothing, and a cooperative kernel that stands for
// several steps takes the position of its last one.
struct Chain {
    enum : unsigned { NONE = 0, IN = 1, ACC = 2, ZERO = 4, ALL = IN | ACC | ZERO };
    kth_ctx *c;
    u64 *slots;  // the three slots: c->islots, the sharded protocol's c->uslots, or a multi-rank set's
    int l = 0;   // the next step
    const RankSet *set = nullptr;  // the states and candidates (null: the ctx's own)

    u64 *slot(int i) const { return slots + (size_t)(i % 3) * kth::STATS_WORDS; }
    StepArgs next(int adv, unsigned use = ALL) {
        const bool init = adv == kth::ADV_INIT_SAMPLE || adv == kth::ADV_INIT_FULL;
        StepArgs a = step(c, set ? *set : own_set(c), adv, init ? -1 : (l + 1) % 2, l % 2, use & IN ? slot(l) : nullptr,
                          use & ACC ? slot(l + 1) : nullptr, use & ZERO ? slot(l + 2) : nullptr);
        ++l;
        return a;
    }
};

// StepArgs: the level runs over these input keys / over this sample (order keys)
void over_keys(StepArgs &a, const int32_t *keys, int64_t n) {
    a.keys = keys;
    a.n_local = (u64)n;
}
void over_sample(StepArgs &a, const uint32_t *sample, int64_t s) {
    a.sample = sample;
    a.sample_count = (u64)s;
}
// ... an ADV_INIT_* step's rank k of n and, for a window select, the window's
// ranks in the sample of s keys
void init_rank(StepArgs &a, int64_t n, int64_t k, int64_t s = 0, u64 r_lo = 0, u64 r_hi = 0) {
    a.init_n = (u64)n;
    a.init_k = (u64)k;
    a.init_s = (u64)s;
    a.r_lo = r_lo;
    a.r_hi = r_hi;
}

// Record one event of a (start, end) pair; pairs are never split because the
// pool sizes are even and start/end are always recorded together.
void ev_mark(kth_ctx *c, std::vector<hipEvent_t> &pool, int &used) {
    if (!c->timing || used >= (int)pool.size()) return;
    (void)hipEventRecord(pool[used++], c->stream);
}
void ev_main(kth_ctx *c) { ev_mark(c, c->ev_main, c->main_used); }

int launch_check() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (getenv("KTH_DEBUG")) fprintf(stderr, "kth: launch failed: %s\n", hipGetErrorString(e));
        return KTH_EHIP;
    }
    return KTH_OK;
}

// Histogram levels.  Dense levels (every key of the domain lands in the
// histogram: the first digit of a domain) run few 1024-thread workgroups of
// DENSE_PER_WG keys, so at most ~domain/DENSE_PER_WG workgroups add to each
// global bin; sparse levels (only keys matching the prefix) run many small ones.
constexpr u64 DENSE_PER_WG = 1ull << 16;
constexpr u64 SPARSE_PER_WG = (u64)kth::BLK * kth::LEVEL_UNROLL * 4;

int level_grid(u64 count, u64 per_wg) {
    u64 g = (count + per_wg - 1) / per_wg;
    return (int)std::max<u64>(1, std::min<u64>(LEVEL_GRID_MAX, g));
}

u64 sparse_wg(const kth_ctx *c) { return c->sparse_per_wg ? c->sparse_per_wg : SPARSE_PER_WG; }

// F32 (here and below): the key kind of a.keys, float32 or int32; the sample
// and the candidates are order keys either way.
template <bool F32 = false>
void launch_level(kth_ctx *c, StepArgs a, bool dense, int grid) {
    if (dense) {
        a.min_per_wg = DENSE_PER_WG;
        kth::k_level<kth::DENSE_BLK, F32><<<grid, kth::DENSE_BLK, 0, c->stream>>>(a);
    } else {
        a.min_per_wg = sparse_wg(c);
        kth::k_level<kth::BLK, F32><<<grid, kth::BLK, 0, c->stream>>>(a);
    }
}

// ---------------------------------------------------------------- paths
template <bool F32>
int run_small(kth_ctx *c, const int32_t *keys, int64_t n, int64_t k, int32_t *d_out, int32_t *d_status) {
    c->last_state = 1;
    ev_main(c);
    kth::k_small<F32><<<1, kth::SMALL_BLOCK, (size_t)n * 4, c->stream>>>(keys, (u64)n, (u64)k, d_out, d_status,
                                                                    c->st + 1, d_last(c), single_word<F32>(c, 1));
    ev_main(c);
    return launch_check();
}

kth::CoopArgs coop_args(kth_ctx *c, u64 slot_off, int32_t *d_out, int32_t *d_status) {
    kth::CoopArgs x;
    memset(&x, 0, sizeof x);
    x.slots = c->islots + slot_off;
    x.bar = reinterpret_cast<uint32_t *>(c->islots + BAR_OFF);
    x.tail = reinterpret_cast<uint32_t *>(c->islots + TAIL_OFF);
    x.d_out = d_out;
    x.d_status = d_status;
    x.dense_per_wg = DENSE_PER_WG;
    x.sparse_per_wg = FIN_SPARSE_PER_WG;
    x.slack64 = c->head_slack64;
    x.fault = c->fault_barrier ? 1u : 0u;
    if (c->fault_once) c->fault_barrier = false;
    return x;
}

// k_finish: the finish phase in one launch.  It leaves its slots, PreHist and
// the sample phase's slots zero, so nothing here depends on what ran before:
// the launch can run again as enqueued.
constexpr size_t FIN_DYN_LDS = (size_t)kth::FIN_LDS_KEYS * 4;
uint32_t *pre_words(kth_ctx *c) { return reinterpret_cast<uint32_t *>(c->islots + PRE_OFF); }

// last: the LastCall word the launch leaves
// with_pre: this select's k_main<0> histogrammed the candidates' first digit into PreHist
// head_slots: the sample phase's slots this launch clears (null: the ctx's own)
// group_rows: ... and wrote the candidates grouped, a directory row for each of this many workgroups (0: not)
template <bool F32>
void launch_finish(kth_ctx *c, const StepArgs &a, int32_t *d_out, int32_t *d_status, uint32_t last, bool with_pre = false,
                   u64 *head_slots = nullptr, int group_rows = 0) {
    kth::CoopArgs x = coop_args(c, FSLOT_OFF, d_out, d_status);
    x.zero2 = head_slots ? head_slots : c->islots + HSLOT_OFF;
    x.zero2_words = HSLOT_WORDS;
    x.pre = with_pre ? pre_words(c) : nullptr;
    x.last = d_last(c);
    kth::FinGroup fg{nullptr, 0u};
    if (with_pre && group_rows > 0 && !c->finish_slices)
        fg = kth::FinGroup{reinterpret_cast<const uint8_t *>(c->gdir.p), (uint32_t)group_rows};
    kth::k_finish<F32><<<c->fin_grid, kth::DENSE_BLK, FIN_DYN_LDS, c->stream>>>(a, x, last, fg);
}

template <bool F32>
int run_radix(kth_ctx *c, const int32_t *keys, int64_t n, int64_t k, int32_t *d_out, int32_t *d_status) {
    if (c->coop) {  // three radix levels over the input in one launch (steps 0 to 3: the state ends in st[1])
        StepArgs a = Chain{c, c->islots, 3}.next(kth::ADV_INIT_FULL, Chain::NONE);
        over_keys(a, keys, n);
        init_rank(a, n, k);
        ev_main(c);
        launch_finish<F32>(c, a, d_out, d_status, single_word<F32>(c, 1));
        ev_main(c);
        c->last_state = 1;
        return launch_check();
    }
    Chain ch{c, c->islots};
    StepArgs a = ch.next(kth::ADV_INIT_FULL, Chain::ACC | Chain::ZERO);
    over_keys(a, keys, n);
    init_rank(a, n, k);
    ev_main(c);  // the first radix pass is the dominant kernel here
    launch_level<F32>(c, a, true, level_grid((u64)n, DENSE_PER_WG));
    ev_main(c);
    for (int digit = 1; digit <= 2; ++digit) {
        a = ch.next(kth::ADV_PICK);
        over_keys(a, keys, n);
        launch_level<F32>(c, a, false, level_grid((u64)n, sparse_wg(c)));
    }
    a = ch.next(kth::ADV_PICK, Chain::IN);
    kth::k_result<F32><<<1, kth::BLK, 0, c->stream>>>(a, d_out, d_status, c->islots, ISLOT_WORDS, d_last(c),
                                                     single_word<F32>(c, 1));
    c->last_state = 1;
    return launch_check();
}

// k_head's step: the sample phase of a window select in one launch, so `ch`
// stands at step 2 (k_head is steps 0 to 2), the window state left in st[0].
// clear_counts: it also clears the streaming pass's count slot islot(1),
// islot(2) and the candidate count, which the cooperative single-GPU select
// leaves behind.
StepArgs head_step(Chain &ch, int64_t n, int64_t k, int64_t s, u64 r_lo, u64 r_hi, bool clear_counts) {
    StepArgs a = ch.next(kth::ADV_INIT_SAMPLE, clear_counts ? Chain::ZERO : Chain::NONE);
    if (clear_counts) a.zero_words = 2 * (u64)kth::STATS_WORDS + 1;
    init_rank(a, n, k, s, r_lo, r_hi);
    return a;
}

// The streaming pass, plain (tflag 0) or with the top-k records of k_main<tflag>.
// gdir: the plain pass (tflag 0) writes its candidates grouped and a row per workgroup here (null: not)
template <bool F32>
void launch_main(kth_ctx *c, const StepArgs &a, int tflag, uint32_t *tflags, uint32_t *gdir = nullptr) {
    const kth::TkSeg none{};
    // (the staged variants 5 / 6 exist for int32 keys only, and kth_topk_f32
    // never asks for them; a float32 pass that did would run plain)
    if (F32 && tflag >= 5) tflag = 0;
    const int g = c->main_grid[F32][tflag];
    uint32_t *cand = c->cand.p, *rows = c->cand_rows.p;
    switch (tflag) {
    case 1: kth::k_main<1, F32><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, nullptr, none); break;
    case 2: kth::k_main<2, F32><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, nullptr, none); break;
    case 3: kth::k_main<3, F32><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, rows, none); break;
    case 4: kth::k_main<4, F32><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, rows, none); break;
    case 5:
        if constexpr (!F32) kth::k_main<5><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, nullptr, c->tk_seg);
        break;
    case 6:
        if constexpr (!F32) kth::k_main<6><<<g, kth::BLK, 0, c->stream>>>(a, cand, tflags, nullptr, c->tk_seg);
        break;
    default: kth::k_main<0, F32><<<g, kth::BLK, 0, c->stream>>>(a, cand, gdir, nullptr, none); break;
    }
}

// The main pass + candidate levels + result, shared by the single-GPU window
// path.  Expects the window state in st[0] and the last sample digit's
// histogram in islot(0).
template <bool F32>
int run_window(kth_ctx *c, const int32_t *keys, int64_t n, int64_t k, int32_t *d_out, int32_t *d_status,
               int tflag = 0, uint32_t *tflags = nullptr) {
    const int64_t s = sample_size(n);
    const u64 nchunks = ((u64)s + kth::SAMPLE_CHUNK - 1) / kth::SAMPLE_CHUNK;
    const u64 stride = (u64)n / nchunks;
    u64 r_lo, r_hi;
    window_ranks(n, k, s, &r_lo, &r_hi);
    KTH_TRY(reserve_window(c, n));

    if (c->coop) {
        // sample phase in one launch -> window state in st[0]
        // (it also clears the streaming pass's count slot islot(1) and the candidate count)
        Chain ch{c, c->islots, 2};
        StepArgs a = head_step(ch, n, k, s, r_lo, r_hi, true);
        // the plain select takes a first-level window of up to s / head_abs_div
        // sample keys (~n / 1024 candidates) whatever the slack: at k near 1 or
        // n it spares the second sample level (the top-k variants keep the
        // narrow window: their count pass loads the rows below its far edge).
        // Sorted input at k = 1 / n: 0.672-0.675 -> 0.654-0.658 ms; uniform
        // keys unchanged (their edge bin holds ~1024 sample keys: s / 256 took
        // them, ~1 M candidates, and cost ~10 us more than the level saves)
        kth::CoopArgs hx = coop_args(c, HSLOT_OFF, nullptr, nullptr);
        if (tflag == 0 && c->head_abs_div) hx.abs_min = (u64)s / c->head_abs_div;
        kth::k_head<F32><<<gather_grid(nchunks), kth::DENSE_BLK, 0, c->stream>>>(a, hx, keys, (u64)n, stride,
                                                                               c->sample.p, (u64)s);
        // the streaming pass: counts into islot(1) (zero between selects);
        // the plain pass also histograms the candidates' first digit for k_finish
        a = ch.next(kth::ADV_CARRY, Chain::ACC);
        over_keys(a, keys, n);
        const bool pre = tflag == 0 && c->pre_hist;
        if (pre) a.pre_hist = pre_words(c);
        const bool grp = pre && grouping(c) && c->gdir.p != nullptr;
        ev_main(c);
        launch_main<F32>(c, a, tflag, tflags, grp ? c->gdir.p : nullptr);
        ev_main(c);
        // decide + candidate (or fallback) levels + answer in one launch
        a = ch.next(kth::ADV_DECIDE, Chain::IN);
        over_keys(a, keys, n);
        launch_finish<F32>(c, a, d_out, d_status, single_word<F32>(c, 0), pre, nullptr, grp ? c->main_grid[F32][0] : 0);
        c->last_state = 0;
        c->counts_left = true;  // (k_head clears them; a sharded select on this ctx must too)
        return launch_check();
    }
    // sample + first digit of the sample
    Chain ch{c, c->islots};
    StepArgs a = ch.next(kth::ADV_INIT_SAMPLE, Chain::ACC | Chain::ZERO);
    init_rank(a, n, k, s, r_lo, r_hi);
    kth::k_gather<true, F32><<<gather_grid(nchunks), kth::DENSE_BLK, 0, c->stream>>>(a, keys, (u64)n, stride,
                                                                                   c->sample.p, (u64)s);
    // digits 2, 3 of the sample ranks (sparse: only keys in the picked bins)
    const int gs = level_grid((u64)s, sparse_wg(c));
    for (int digit = 2; digit <= 3; ++digit) {
        a = ch.next(kth::ADV_PICK);
        over_sample(a, c->sample.p, s);
        launch_level(c, a, false, gs);
    }
    // the streaming pass
    a = ch.next(kth::ADV_PICK);
    over_keys(a, keys, n);
    ev_main(c);
    launch_main<F32>(c, a, tflag, tflags);
    ev_main(c);
    // decide + candidate (or fallback) levels.  The grids cover the fallback
    // (whole input); in the common case only the WGs the candidates need run.
    a = ch.next(kth::ADV_DECIDE);
    over_keys(a, keys, n);
    launch_level<F32>(c, a, true, c->post_dense_grid);
    for (int digit = 2; digit <= 3; ++digit) {
        a = ch.next(kth::ADV_PICK);
        over_keys(a, keys, n);
        launch_level<F32>(c, a, false, c->post_sparse_grid);
    }
    a = ch.next(kth::ADV_PICK, Chain::IN);
    // k_result clears the slots and the candidate count for the next select --
    // but a top-k with candidate rows (tflag 3 / 4) still reads the count in
    // k_topk_cands: there it clears the three slots only and the top-k clears
    // the count itself, on the stream right after that kernel (count_kept).
    // (It used to clear the count here too, and that top-k then missed the
    // candidates' share: a bracket failure, nothing written.  Then the NEXT
    // call cleared it, which a graph captured earlier does not do: its replay
    // appended its candidates after the top-k's.)
    const bool keep_count = tflag == 3 || tflag == 4;
    kth::k_result<F32><<<1, kth::BLK, 0, c->stream>>>(a, d_out, d_status, c->islots,
                                                     keep_count ? 3 * (u64)kth::STATS_WORDS : (u64)ISLOT_WORDS,
                                                     d_last(c), single_word<F32>(c, 1));
    if (keep_count) c->count_kept = true;
    c->last_state = 1;
    return launch_check();
}

// After a grid-barrier timeout the cooperative kernels stay off for
// COOP_BACKOFF selections of any entry point (synchronous, asynchronous,
// top-k, sharded); each one counts down here, then they are tried again.
void coop_tick(kth_ctx *c) {
    if (c->coop_backoff > 0 && --c->coop_backoff == 0) c->coop = c->coop_wanted;
}

// One select's launches; select_async below is the entry (it counts the
// selection for the cooperative back-off, a multi-rank call counts once).
template <bool F32 = false>
int select_enqueue(kth_ctx *c, const int32_t *d_keys, int64_t n, int64_t k, int32_t *d_out, int32_t *d_status,
                   int tflag = 0, uint32_t *tflags = nullptr) {
    if (c->dirty || c->count_kept) {  // (count_kept: that top-k failed before its clear)
        HIP_TRY(hipMemsetAsync(c->islots, 0, SLOT_ALLOC_WORDS * sizeof(u64), c->stream));
        c->dirty = c->count_kept = false;
    }
    int rc;
    ev_mark(c, c->ev_total, c->total_used);
    if (n <= SMALL_N)
        rc = run_small<F32>(c, d_keys, n, k, d_out, d_status);
    else if (n <= RADIX_MAX_N)
        rc = run_radix<F32>(c, d_keys, n, k, d_out, d_status);
    else
        rc = run_window<F32>(c, d_keys, n, k, d_out, d_status, tflag, tflags);
    ev_mark(c, c->ev_total, c->total_used);
    if (rc != KTH_OK) c->dirty = true;
    if (c->stamps) dump_stamps(c);
    return rc;
}

template <bool F32 = false>
int select_async(kth_ctx *c, const int32_t *d_keys, int64_t n, int64_t k, int32_t *d_out, int32_t *d_status,
                 int tflag = 0, uint32_t *tflags = nullptr) {
    if (!c || !d_keys || (!d_out && !d_status) || n < 1 || k < 1 || k > n) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    coop_tick(c);
    return select_enqueue<F32>(c, d_keys, n, k, d_out, d_status, tflag, tflags);
}

bool is_device_ptr(const void *p) {
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

thread_local kth_ctx *tl_ctx = nullptr;

// Rows: the wave-per-row register kernel (kth_rows.hpp) for cols <= 4096,
// KPL keys per lane; the LDS workgroup-per-row kernel above that.
#ifndef KTH_ROWS_R0
#define KTH_ROWS_R0 4  // first-pass histogram copies per wave in k_rows_reg
#endif
template <bool F32, int KPL, bool TOPK>
void launch_rows_reg(kth_ctx *c, bool vec, int g, const uint32_t *d_keys, u64 R, uint32_t C, uint32_t K,
                     uint32_t *d_out, uint32_t flip, uint32_t *vals, int32_t *idx) {
    if (vec && C == (uint32_t)(KPL * kth::WAVE))
        kth::k_rows_reg<F32, KPL, true, KTH_ROWS_R0, TOPK, true>
            <<<g, kth::RW_BLOCK, 0, c->stream>>>(d_keys, R, C, K, d_out, flip, vals, idx);
    else if (vec)
        kth::k_rows_reg<F32, KPL, true, KTH_ROWS_R0, TOPK, false>
            <<<g, kth::RW_BLOCK, 0, c->stream>>>(d_keys, R, C, K, d_out, flip, vals, idx);
    else
        kth::k_rows_reg<F32, KPL, false, KTH_ROWS_R0, TOPK, false>
            <<<g, kth::RW_BLOCK, 0, c->stream>>>(d_keys, R, C, K, d_out, flip, vals, idx);
}

// k-th per row (TOPK = false, into d_out) or top-k per row (into vals / idx;
// cols <= KTH_TOPK_MAX_COLS, checked by the caller).
template <bool F32, bool TOPK>
int launch_rows(kth_ctx *c, const uint32_t *d_keys, int64_t rows, int32_t cols, int32_t k, uint32_t *d_out,
                uint32_t flip = 0, uint32_t *vals = nullptr, int32_t *idx = nullptr) {
    const bool vec = (reinterpret_cast<uintptr_t>(d_keys) & 15u) == 0 && cols % 4 == 0;
    const int rows_per_wg = kth::RW_BLOCK / kth::WAVE;
    const int64_t g64 = (rows + rows_per_wg - 1) / rows_per_wg;  // one row per wave
    if (g64 > 0x7FFFFFFF) return KTH_EINVAL;
    const int g = (int)g64;
    const u64 R = (u64)rows;
    const uint32_t C = (uint32_t)cols, K = (uint32_t)k;
    if (cols <= 1024)
        launch_rows_reg<F32, 16, TOPK>(c, vec, g, d_keys, R, C, K, d_out, flip, vals, idx);
    else if (cols <= 2048)
        launch_rows_reg<F32, 32, TOPK>(c, vec, g, d_keys, R, C, K, d_out, flip, vals, idx);
    else if (cols <= 4096)
        launch_rows_reg<F32, 64, TOPK>(c, vec, g, d_keys, R, C, K, d_out, flip, vals, idx);
    else if (!TOPK)
        kth::k_rows<F32><<<(int)std::min<int64_t>(rows, 1 << 20), kth::ROWS_BLOCK, (size_t)cols * 4, c->stream>>>(
            d_keys, R, C, (u64)k, d_out);
    return launch_check();
}

// The four rows entry points: the argument check and the launch.  d_out is the
// k-th per row (TOPK = false); d_vals / d_idx, either may be null, the top-k.
template <bool F32, bool TOPK>
int rows_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int32_t k, void *d_out, int largest = 0,
               void *d_vals = nullptr, int32_t *d_idx = nullptr) {
    const bool has_out = TOPK ? d_vals || d_idx : d_out != nullptr;
    const int32_t max_cols = TOPK ? KTH_TOPK_MAX_COLS : KTH_ROWS_MAX_COLS;
    if (!c || !d_keys || !has_out || rows < 0 || cols < 1 || cols > max_cols || k < 1 || k > cols) return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    return launch_rows<F32, TOPK>(c, static_cast<const uint32_t *>(d_keys), rows, cols, k,
                                  static_cast<uint32_t *>(d_out), TOPK && largest ? 0xFFFFFFFFu : 0u,
                                  static_cast<uint32_t *>(d_vals), d_idx);
}

// 16-bit rows (kth_rows16.hpp): KW packed words per lane by cols, the 16-byte
// load path for an aligned base with cols % 8 == 0, else the guarded one.
static_assert(KTH_ROWS16_MAX_COLS == kth::R16_MAX_COLS, "include/kth.h 16-bit row limit");
template <bool FLT, int KW, bool TOPK>
void launch_rows16_kw(kth_ctx *c, bool vec, int g, const uint16_t *d_keys, u64 R, uint32_t C, uint32_t K, int kind,
                      uint32_t flip, uint16_t *d_out, uint16_t *vals, int32_t *idx) {
    if (vec)
        kth::k_rows16<FLT, KW, true, TOPK><<<g, kth::RW_BLOCK, 0, c->stream>>>(d_keys, R, C, K, kind, flip, d_out, vals, idx);
    else
        kth::k_rows16<FLT, KW, false, TOPK><<<g, kth::RW_BLOCK, 0, c->stream>>>(d_keys, R, C, K, kind, flip, d_out, vals, idx);
}

template <bool FLT, bool TOPK>
int launch_rows16(kth_ctx *c, const uint16_t *d_keys, int64_t rows, int32_t cols, int32_t k, int kind, uint32_t flip,
                  uint16_t *d_out, uint16_t *vals, int32_t *idx) {
    const bool vec = (reinterpret_cast<uintptr_t>(d_keys) & 15u) == 0 && cols % 8 == 0;
    const int rows_per_wg = kth::RW_BLOCK / kth::WAVE;
    const int64_t g64 = (rows + rows_per_wg - 1) / rows_per_wg;  // one row per wave
    if (g64 > 0x7FFFFFFF) return KTH_EINVAL;
    const int g = (int)g64;
    const u64 R = (u64)rows;
    const uint32_t C = (uint32_t)cols, K = (uint32_t)k;
    if (cols <= 512)
        launch_rows16_kw<FLT, 4, TOPK>(c, vec, g, d_keys, R, C, K, kind, flip, d_out, vals, idx);
    else if (cols <= 1024)
        launch_rows16_kw<FLT, 8, TOPK>(c, vec, g, d_keys, R, C, K, kind, flip, d_out, vals, idx);
    else if (cols <= 2048)
        launch_rows16_kw<FLT, 16, TOPK>(c, vec, g, d_keys, R, C, K, kind, flip, d_out, vals, idx);
    else if (cols <= 4096)
        launch_rows16_kw<FLT, 32, TOPK>(c, vec, g, d_keys, R, C, K, kind, flip, d_out, vals, idx);
    else
        launch_rows16_kw<FLT, 64, TOPK>(c, vec, g, d_keys, R, C, K, kind, flip, d_out, vals, idx);
    return launch_check();
}

// The two 16-bit rows entry points: the argument check and the launch.
template <bool TOPK>
int rows16_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int32_t k, int kind, uint16_t *d_out,
                 int largest = 0, uint16_t *d_vals = nullptr, int32_t *d_idx = nullptr) {
    const bool has_out = TOPK ? d_vals || d_idx : d_out != nullptr;
    if (!c || !d_keys || !has_out || rows < 0 || cols < 1 || cols > KTH_ROWS16_MAX_COLS || k < 1 || k > cols ||
        kind < KTH_K16_I16 || kind > KTH_K16_BF16)
        return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    const uint16_t *keys = static_cast<const uint16_t *>(d_keys);
    const uint32_t flip = TOPK && largest ? 0xFFFFFFFFu : 0u;
    return kth::k16_float(kind) ? launch_rows16<true, TOPK>(c, keys, rows, cols, k, kind, flip, d_out, d_vals, d_idx)
                                : launch_rows16<false, TOPK>(c, keys, rows, cols, k, kind, flip, d_out, d_vals, d_idx);
}

// Wide rows (kth_rows_wide.hpp).  The plan: how many workgroups share a row
// (slices; 1 = the fused one-workgroup-per-row kernel), the columns of a slice,
// and how many rows one launch sequence takes (group_rows, which bounds the
// scratch whatever `rows` is).
static_assert(KTH_WIDE_MAX_SLICES == kth::WD_MAX_SLICES, "include/kth.h wide-rows slice limit");
constexpr int64_t WIDE_SCRATCH_MAX = (int64_t)32 << 20;
// scratch bytes a row of a group: its histogram, its state, and (better, equal)
// for KTH_WIDE_MAX_SLICES slices, so that no forced plan needs more than a
// reserve of the same rows gave
constexpr int64_t WIDE_ROW_BYTES = 4 * ((int64_t)kth::NBINS + kth::WD_STATE_WORDS + 2 * kth::WD_MAX_SLICES);
constexpr int64_t WIDE_GROUP_MAX = WIDE_SCRATCH_MAX / WIDE_ROW_BYTES;  // 3266 rows: also below the grid's y limit
constexpr int64_t WIDE_FUSED_GROUP_MAX = 1 << 16;  // the fused form has no scratch: rows a launch
// Automatic plan (DESIGN.md "Wide rows", from profiles/rows_wide_plan_sweep.jsonl):
// the fused form when the rows alone fill the GPU (rows >= WIDE_FUSED_ROWS_PER_CU
// * num_cu) or a row is short enough for one workgroup to read it three times
// within the split sequence's launch-bound floor (cols <= WIDE_FUSED_COLS);
// else rows are split until the grid holds WIDE_WG_PER_CU workgroups a CU, a
// slice keeping at least WIDE_MIN_SLICE columns (a workgroup's fixed cost, its
// histogram cleared and 2048 bins flushed, is not worth fewer keys).
// Fewer than WIDE_MIN_SLICES slices never beat the fused form.
constexpr int WIDE_WG_PER_CU = 4;
constexpr int WIDE_FUSED_ROWS_PER_CU = 2;
constexpr int32_t WIDE_FUSED_COLS = 32768;
constexpr int32_t WIDE_MIN_SLICE = 4096;
constexpr int32_t WIDE_MIN_SLICES = 4;

struct WidePlan {
    int32_t slices, slice_keys, group_rows;
    int64_t scratch_bytes;
};

// The key width (4 or 2 bytes) sets both.  align: a slice's columns are a
// multiple of it, so that every slice of an aligned row starts on a 16-byte
// boundary (4 for 4-byte keys, 8 for 2-byte keys).  min_slice: the columns a
// slice keeps.  The 16-bit calls share every threshold, in columns, but this
// one: their sweep (profiles/rows_wide16_plan_sweep.jsonl) puts it at 8192
// columns, the same 16 KiB (DESIGN.md "16-bit wide rows").
constexpr int32_t WIDE16_MIN_SLICE = 8192;
constexpr int32_t wide_align(size_t key_bytes) { return (int32_t)(16 / key_bytes); }
WidePlan wide_plan(size_t key_bytes, int64_t rows, int32_t cols, int num_cu, int32_t force_slices, int32_t force_group) {
    const int32_t align = wide_align(key_bytes), min_slice = key_bytes == 2 ? WIDE16_MIN_SLICE : WIDE_MIN_SLICE;
    int64_t want = force_slices;
    if (want <= 0) {
        if (rows <= 0 || rows >= (int64_t)WIDE_FUSED_ROWS_PER_CU * num_cu || cols <= WIDE_FUSED_COLS) {
            want = 1;
        } else {
            want = std::min<int64_t>((int64_t)WIDE_WG_PER_CU * num_cu / rows, cols / min_slice);
            if (want < WIDE_MIN_SLICES) want = 1;
        }
    }
    want = std::max<int64_t>(1, std::min<int64_t>(want, KTH_WIDE_MAX_SLICES));
    WidePlan p;
    p.slice_keys = (int32_t)(((cols + want - 1) / want + align - 1) & ~(int64_t)(align - 1));
    p.slices = (cols + p.slice_keys - 1) / p.slice_keys;  // (the last slice is never empty)
    int64_t g = std::min(std::max<int64_t>(rows, 1), p.slices > 1 ? WIDE_GROUP_MAX : WIDE_FUSED_GROUP_MAX);
    if (force_group > 0) g = std::min<int64_t>(g, force_group);
    p.group_rows = (int32_t)g;
    p.scratch_bytes = p.slices > 1 ? g * WIDE_ROW_BYTES : 0;
    return p;
}

bool wide_dims_ok(int64_t rows, int32_t cols) { return rows >= 0 && cols >= 1 && cols <= KTH_WIDE_MAX_COLS; }

// The automatic plan of kth_wide_rows_plan and kth_wide_rows_plan_k16.
int wide_plan_out(size_t key_bytes, int64_t rows, int32_t cols, int num_cu, int32_t *slices, int32_t *slice_keys,
                  int32_t *group_rows, int64_t *scratch_bytes) {
    if (!wide_dims_ok(rows, cols) || num_cu < 1) return KTH_EINVAL;
    const WidePlan p = wide_plan(key_bytes, rows, cols, num_cu, 0, 0);
    if (slices) *slices = p.slices;
    if (slice_keys) *slice_keys = p.slice_keys;
    if (group_rows) *group_rows = p.group_rows;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return KTH_OK;
}

// The shape every wide-rows call checks (its outputs, k and kind are its own).
bool wide_shape_ok(const kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld) {
    return c && d_keys && wide_dims_ok(rows, cols) && ld >= cols;
}

// The reserve rule of the split forms' scratch.  One buffer of a family: the
// elements wanted, and whether its sequences need it zero when they start (a
// sequence that ends leaves it so).
template <class T>
struct Scratch {
    DevBuf<T> &buf;
    u64 want;
    bool zeroed;
    u64 had;
    Scratch(DevBuf<T> &b, u64 w, bool z) : buf(b), want(w), zeroed(z), had(b.count) {}
    int zero(kth_ctx *c, bool dirty) const {
        if (zeroed && (buf.count != had || dirty)) HIP_TRY(hipMemsetAsync(buf.p, 0, buf.count * sizeof(T), c->stream));
        return KTH_OK;
    }
};
// Every buffer or none; a zeroed one is cleared when it is new or when a
// sequence of the family was cut short (`dirty`).
template <class... T>
int reserve_scratch(kth_ctx *c, bool &dirty, const Scratch<T> &...s) {
    int rc = KTH_OK;
    if (!(((rc = s.buf.reserve(s.want)) == KTH_OK) && ...)) {
        release_all(s.buf...);
        return rc;
    }
    if (!(((rc = s.zero(c, dirty)) == KTH_OK) && ...)) return rc;
    dirty = false;
    return KTH_OK;
}

// The end of a split sequence: one that was cut short has left scratch that is
// not zero, which the families' next reserve clears.
template <class... B>
int sequence_check(B &...dirty) {
    const int rc = launch_check();
    if (rc != KTH_OK) ((dirty = true), ...);
    return rc;
}

// p + off of an output or a per-row array that may be absent.
template <class T>
T *ptr_at(T *p, u64 off) {
    return p ? p + off : nullptr;
}

// A wide-rows call once its arguments are checked: the plan for keys of
// sizeof(E) bytes with the ctx's forced values, the family's group cap and
// scratch (the split form's alone; the fused form's cap is wide_plan's), then
// launch(p, vec, the group's keys, r0, g) for each group of g rows from row r0.
// vec: every row starts on 16 bytes.
template <class E, class Launch>
int wide_rows_drive(kth_ctx *c, const E *keys, int64_t rows, int32_t cols, int64_t ld, int64_t group_max,
                    int (*reserve)(kth_ctx *, int64_t), Launch launch) {
    WidePlan p = wide_plan(sizeof(E), rows, cols, c->num_cu, c->wide_force_slices, c->wide_force_group);
    if (p.slices > 1) {
        p.group_rows = (int32_t)std::min<int64_t>(p.group_rows, group_max);
        KTH_TRY(reserve(c, p.group_rows));
    }
    const bool vec = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0 && ld % wide_align(sizeof(E)) == 0;
    for (int64_t r0 = 0; r0 < rows; r0 += p.group_rows)
        KTH_TRY(launch(p, vec, keys + (u64)r0 * (u64)ld, r0, std::min<int64_t>(p.group_rows, rows - r0)));
    return KTH_OK;
}

// The split form's scratch for groups of g rows; new buffers are zeroed.
int reserve_wide(kth_ctx *c, int64_t g) {
    return reserve_scratch(c, c->wide_dirty, Scratch(c->wide_hist, (u64)g * kth::NBINS, true),
                           Scratch(c->wide_state, (u64)g, true),
                           Scratch(c->wide_cnt, (u64)g * 2 * kth::WD_MAX_SLICES, false));
}

// A uniform kernel, or for the var calls (VAR) its _var twin, which takes the
// same arguments and then the group's WideVar.
template <bool VAR, class U, class V, class... A>
void launch_twin(U *uniform, V *var, dim3 grid, int block, kth_ctx *c, const kth::WideVar &v, A... args) {
    if constexpr (VAR)
        var<<<grid, block, 0, c->stream>>>(args..., v);
    else
        uniform<<<grid, block, 0, c->stream>>>(args...);
}

// One group of g rows: the fused launch, or the split form's sequence -- per
// digit a count and a pick, for the top-k a count per slice and the compaction.
// VAR: the var calls' kernels, which read row r's length and rank from `v`
// (the group's first row of d_lens / d_ks / d_cnt; `cols` and `k` stay the
// bounds, and the plan and the scratch are those of the uniform call).
template <bool F32, bool VEC, bool TOPK, bool VAR>
int launch_wide_group(kth_ctx *c, const WidePlan &p, const uint32_t *keys, int64_t g, uint32_t cols, u64 ld, uint32_t k,
                      uint32_t flip, uint32_t *out, uint32_t *vals, int32_t *idx, const kth::WideVar &v) {
    if (p.slices == 1) {
        launch_twin<VAR>(kth::k_wide_fused<F32, VEC, TOPK>, kth::k_wide_fused_var<F32, VEC, TOPK>, (int)g, kth::WD_FBLOCK, c,
                         v, keys, ld, cols, k, flip, out, vals, idx);
        return launch_check();
    }
    const dim3 grid((unsigned)p.slices, (unsigned)g);
    const uint32_t sk = (uint32_t)p.slice_keys;
    uint32_t *hist = c->wide_hist.p, *cnt = c->wide_cnt.p;
    kth::WideState *state = c->wide_state.p;
    for (int pass = 0; pass < 3; ++pass) {
        launch_twin<VAR>(kth::k_wide_count<F32, VEC>, kth::k_wide_count_var<F32, VEC>, grid, kth::WD_BLOCK, c, v, keys, ld,
                         cols, sk, flip, pass, hist, state);
        launch_twin<VAR>(kth::k_wide_pick<F32>, kth::k_wide_pick_var<F32>, (int)g, kth::WD_BLOCK, c, v, hist, state, pass,
                         cols, k, flip, TOPK ? nullptr : out);
    }
    if constexpr (TOPK) {
        launch_twin<VAR>(kth::k_wide_tk_count<F32, VEC>, kth::k_wide_tk_count_var<F32, VEC>, grid, kth::WD_BLOCK, c, v, keys,
                         ld, cols, sk, flip, state, cnt);
        launch_twin<VAR>(kth::k_wide_tk_write<F32, VEC>, kth::k_wide_tk_write_var<F32, VEC>, grid, kth::WD_BLOCK, c, v, keys,
                         ld, cols, sk, flip, k, state, cnt, vals, idx);
    }
    return sequence_check(c->wide_dirty);
}

// A var call's arrays at row r0 (the host loops advance them like the outputs).
kth::WideVar wide_var_at(const kth::WideVar &v, int64_t r0) {
    return kth::WideVar{ptr_at(v.lens, r0), ptr_at(v.ks, r0), ptr_at(v.cnt, r0)};
}

// The eight 32-bit wide-rows entry points: the argument check, then the rows.
template <bool F32, bool TOPK, bool VAR = false>
int wide_rows_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k, void *d_out,
                    int largest = 0, void *d_vals = nullptr, int32_t *d_idx = nullptr,
                    const kth::WideVar &var = kth::WideVar{}) {
    const bool has_out = TOPK ? d_vals || d_idx : d_out != nullptr;
    if (!wide_shape_ok(c, d_keys, rows, cols, ld) || !has_out || k < 1 || k > cols) return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    uint32_t *out = static_cast<uint32_t *>(d_out), *vals = static_cast<uint32_t *>(d_vals);
    const uint32_t flip = TOPK && largest ? 0xFFFFFFFFu : 0u;
    return wide_rows_drive(
        c, static_cast<const uint32_t *>(d_keys), rows, cols, ld, WIDE_GROUP_MAX, reserve_wide,
        [&](const WidePlan &p, bool vec, const uint32_t *gk, int64_t r0, int64_t g) {
            const auto launch = vec ? launch_wide_group<F32, true, TOPK, VAR> : launch_wide_group<F32, false, TOPK, VAR>;
            return launch(c, p, gk, g, (uint32_t)cols, (u64)ld, (uint32_t)k, flip, ptr_at(out, r0),
                          ptr_at(vals, (u64)r0 * (u64)k), ptr_at(d_idx, (u64)r0 * (u64)k), wide_var_at(var, r0));
        });
}

// 16-bit wide rows (kth_rows_wide16.hpp): the same plan with slices of a
// multiple of 8 columns, the same scratch, two digits instead of three.
// CV: k16_ord2's key class (0: uint16, 1: int16, 2: float16 / bfloat16).
template <int CV, bool VEC, bool TOPK, bool VAR>
int launch_wide16_group(kth_ctx *c, const WidePlan &p, const uint16_t *keys, int64_t g, uint32_t cols, u64 ld,
                        uint32_t k, uint32_t flip2, int kind, uint16_t *out, uint16_t *vals, int32_t *idx,
                        const kth::WideVar &v) {
    const uint32_t nl2 = kth::k16_nl(kind) * 0x10001u, top2 = kth::k16_top(kind) * 0x10001u;
    if (p.slices == 1) {
        launch_twin<VAR>(kth::k_wide16_fused<CV, VEC, TOPK>, kth::k_wide16_fused_var<CV, VEC, TOPK>, (int)g, kth::WD_FBLOCK,
                         c, v, keys, ld, cols, k, flip2, nl2, top2, kind, out, vals, idx);
        return launch_check();
    }
    const dim3 grid((unsigned)p.slices, (unsigned)g);
    const uint32_t sk = (uint32_t)p.slice_keys;
    uint32_t *hist = c->wide_hist.p, *cnt = c->wide_cnt.p;
    kth::WideState *state = c->wide_state.p;
    uint16_t *sel_out = TOPK ? nullptr : out;
    launch_twin<VAR>(kth::k_wide16_count<CV, VEC, 0>, kth::k_wide16_count_var<CV, VEC, 0>, grid, kth::WD_BLOCK, c, v, keys,
                     ld, cols, sk, flip2, nl2, top2, hist, state);
    launch_twin<VAR>(kth::k_wide16_pick, kth::k_wide16_pick_var, (int)g, kth::WD_BLOCK, c, v, hist, state, 0, cols, k, flip2,
                     kind, sel_out);
    launch_twin<VAR>(kth::k_wide16_count<CV, VEC, 1>, kth::k_wide16_count_var<CV, VEC, 1>, grid, kth::WD_BLOCK, c, v, keys,
                     ld, cols, sk, flip2, nl2, top2, hist, state);
    launch_twin<VAR>(kth::k_wide16_pick, kth::k_wide16_pick_var, (int)g, kth::WD_BLOCK, c, v, hist, state, 1, cols, k, flip2,
                     kind, sel_out);
    if constexpr (TOPK) {
        launch_twin<VAR>(kth::k_wide16_tk_count<CV, VEC>, kth::k_wide16_tk_count_var<CV, VEC>, grid, kth::WD_BLOCK, c, v,
                         keys, ld, cols, sk, flip2, nl2, top2, state, cnt);
        launch_twin<VAR>(kth::k_wide16_tk_write<CV, VEC>, kth::k_wide16_tk_write_var<CV, VEC>, grid, kth::WD_BLOCK, c, v,
                         keys, ld, cols, sk, flip2, nl2, top2, kind, k, state, cnt, vals, idx);
    }
    return sequence_check(c->wide_dirty);
}

// The four 16-bit wide-rows entry points: the argument check, then the rows,
// each group with the launch of the kind's key class and of the load.
template <bool TOPK, bool VAR = false>
int wide16_rows_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k, int kind,
                      uint16_t *d_out, int largest = 0, uint16_t *d_vals = nullptr, int32_t *d_idx = nullptr,
                      const kth::WideVar &var = kth::WideVar{}) {
    const bool has_out = TOPK ? d_vals || d_idx : d_out != nullptr;
    if (!wide_shape_ok(c, d_keys, rows, cols, ld) || !has_out || k < 1 || k > cols || kind < KTH_K16_I16 ||
        kind > KTH_K16_BF16)
        return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    const uint32_t flip2 = TOPK && largest ? 0xFFFFFFFFu : 0u;
    const int cv = kth::k16_float(kind) ? 2 : kind == KTH_K16_I16 ? 1 : 0;
    static constexpr decltype(&launch_wide16_group<0, false, TOPK, VAR>) launch[3][2] = {  // [CV][VEC]
        {launch_wide16_group<0, false, TOPK, VAR>, launch_wide16_group<0, true, TOPK, VAR>},
        {launch_wide16_group<1, false, TOPK, VAR>, launch_wide16_group<1, true, TOPK, VAR>},
        {launch_wide16_group<2, false, TOPK, VAR>, launch_wide16_group<2, true, TOPK, VAR>}};
    return wide_rows_drive(c, static_cast<const uint16_t *>(d_keys), rows, cols, ld, WIDE_GROUP_MAX, reserve_wide,
                           [&](const WidePlan &p, bool vec, const uint16_t *gk, int64_t r0, int64_t g) {
                               return launch[cv][vec](c, p, gk, g, (uint32_t)cols, (u64)ld, (uint32_t)k, flip2, kind,
                                                      ptr_at(d_out, r0), ptr_at(d_vals, (u64)r0 * (u64)k),
                                                      ptr_at(d_idx, (u64)r0 * (u64)k), wide_var_at(var, r0));
                           });
}

// Top-p rows (kth_rows_topp.hpp).  The wide-rows plan; the split form's scratch
// is the top-p calls' own, 24 KiB of bins and a state a row, so a group is
// smaller than the wide select's.
constexpr int64_t TP_ROW_BYTES = (int64_t)kth::NBINS * 12 + kth::TP_STATE_BYTES;
constexpr int64_t TP_GROUP_MAX = WIDE_SCRATCH_MAX / TP_ROW_BYTES;  // 1362 rows

// The split form's scratch for groups of g rows; new buffers are zeroed.
int reserve_topp(kth_ctx *c, int64_t g) {
    return reserve_scratch(c, c->tp_dirty, Scratch(c->tp_mass, (u64)g * kth::NBINS, true),
                           Scratch(c->tp_cnt, (u64)g * kth::NBINS, true), Scratch(c->tp_state, (u64)g, true));
}

// A top-p or sampling call's arrays at row r0 (wide_var_at's counterpart).
kth::TopP topp_at(const kth::TopP &v, int64_t r0) {
    return kth::TopP{ptr_at(v.lens, r0), ptr_at(v.ps, r0), ptr_at(v.temps, r0), ptr_at(v.ks, r0), v.p, v.temp, v.k};
}
// Those calls' check of kind (a KTH_K16_* float kind, or -1 for float32 keys),
// of temp and of the p that stands in for an absent d_ps.
bool topp_args_ok(int kind, const float *d_ps, float p, float temp) {
    return (kind == -1 || kind == KTH_K16_F16 || kind == KTH_K16_BF16) && temp > 0.0f && std::isfinite(temp) &&
           (d_ps || !std::isnan(p));
}
// f(K{}) for the key traits K of `kind`.
template <class F>
int topp_dispatch(int kind, F f) {
    if (kind == -1) return f(kth::TpF32{});
    return kind == KTH_K16_BF16 ? f(kth::TpK16<true>{}) : f(kth::TpK16<false>{});
}

// One group of g rows: the fused launch, or the split form's sequence -- pass M,
// then per digit a weighted count and a pick.  v, d_n, d_thr, rank: at the
// group's first row.
template <class K, bool VEC>
int launch_topp_group(kth_ctx *c, const WidePlan &p, const typename K::elem *keys, int64_t g, uint32_t cols, u64 ld,
                      const kth::TopP &v, int32_t *d_n, typename K::elem *d_thr, int32_t *rank) {
    if (p.slices == 1) {
        kth::k_tp_fused<K, VEC><<<(int)g, kth::WD_FBLOCK, 0, c->stream>>>(keys, ld, cols, v, d_n, d_thr, rank);
        return launch_check();
    }
    const dim3 grid((unsigned)p.slices, (unsigned)g);
    const uint32_t sk = (uint32_t)p.slice_keys;
    kth::k_tp_max<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, c->tp_state.p, v);
    for (int pass = 0; pass < K::PASSES; ++pass) {
        kth::k_tp_count<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, pass, c->tp_mass.p, c->tp_cnt.p,
                                                                    c->tp_state.p, v);
        kth::k_tp_pick<K><<<(int)g, kth::WD_BLOCK, 0, c->stream>>>(c->tp_mass.p, c->tp_cnt.p, c->tp_state.p, pass, cols, v,
                                                                 d_n, d_thr, rank);
    }
    return sequence_check(c->tp_dirty);
}

// The nucleus of every row.  The arguments have been checked.  rank
// (kth_topp_*): rows int32, min(n_r, cap_r).
template <class K>
int topp_rows(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, const kth::TopP &var, int32_t *d_n,
              void *d_thr, int32_t *rank) {
    using E = typename K::elem;
    static_assert(K::PER == wide_align(sizeof(E)), "a load of K::PER columns is the 16 bytes of the plan's alignment");
    E *thr = static_cast<E *>(d_thr);
    return wide_rows_drive(c, static_cast<const E *>(d_keys), rows, cols, ld, TP_GROUP_MAX, reserve_topp,
                           [&](const WidePlan &p, bool vec, const E *gk, int64_t r0, int64_t g) {
                               const auto launch = vec ? launch_topp_group<K, true> : launch_topp_group<K, false>;
                               return launch(c, p, gk, g, (uint32_t)cols, (u64)ld, topp_at(var, r0), ptr_at(d_n, r0),
                                             ptr_at(thr, r0), ptr_at(rank, r0));
                           });
}

// The four top-p entry points: the argument check, then the nucleus and, for
// kth_topp_* (TOPK), the var top-k sequence with the ranks the last pick wrote.
// kind: a KTH_K16_* float kind, or -1 for float32 keys.
template <bool TOPK>
int topp_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, const int32_t *d_lens,
               const int32_t *d_ks, int32_t k, const float *d_ps, float p, const float *d_temps, float temp, int kind,
               int32_t *d_n, void *d_thr, void *d_vals, int32_t *d_idx, int32_t *d_cnt) {
    const bool has_out = TOPK ? d_vals || d_idx : d_n || d_thr;
    if (!wide_shape_ok(c, d_keys, rows, cols, ld) || !has_out || !topp_args_ok(kind, d_ps, p, temp)) return KTH_EINVAL;
    if (TOPK && (k < 1 || k > cols)) return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    int32_t *rank = nullptr;
    if (TOPK) {
        KTH_TRY(c->tp_rank.reserve((u64)rows));
        rank = c->tp_rank.p;
    }
    const kth::TopP var{d_lens, d_ps, d_temps, TOPK ? d_ks : nullptr, p, temp, TOPK ? k : 0};
    KTH_TRY(topp_dispatch(
        kind, [&](auto K) { return topp_rows<decltype(K)>(c, d_keys, rows, cols, ld, var, d_n, d_thr, rank); }));
    if (!TOPK) return KTH_OK;
    const kth::WideVar ranks{d_lens, rank, d_cnt};
    if (kind == -1) return wide_rows_entry<true, true, true>(c, d_keys, rows, cols, ld, k, nullptr, 1, d_vals, d_idx, ranks);
    return wide16_rows_entry<true, true>(c, d_keys, rows, cols, ld, k, kind, nullptr, 1, static_cast<uint16_t *>(d_vals),
                                         d_idx, ranks);
}

// Sampling rows (kth_rows_sample.hpp).  The wide-rows plan; the split form adds a
// state and a count per slice a row to the top-p calls' bins, so a group is a
// little smaller than theirs.
constexpr int64_t SM_ROW_BYTES = TP_ROW_BYTES + kth::SM_STATE_BYTES + 4 * (int64_t)kth::WD_MAX_SLICES;
constexpr int64_t SM_GROUP_MAX = WIDE_SCRATCH_MAX / SM_ROW_BYTES;  // 1305 rows

// The split form's scratch for groups of g rows; a new state buffer is zeroed.
int reserve_sample(kth_ctx *c, int64_t g) {
    KTH_TRY(reserve_topp(c, g));
    return reserve_scratch(c, c->sm_dirty, Scratch(c->sm_state, (u64)g, true),
                           Scratch(c->sm_loc, (u64)g * kth::WD_MAX_SLICES, false));
}

// One group of g rows: the fused launch, or the split form's sequence -- pass M,
// per digit of descent A and of descent B a weighted count and a pick, then the
// locate's count and pick.  no_a: the host arguments alone say that no row
// needs descent A (no filter at all).  v, us, d_tok, d_cnt: at the group's first row.
template <class K, bool VEC>
int launch_sample_group(kth_ctx *c, const WidePlan &p, const typename K::elem *keys, int64_t g, uint32_t cols, u64 ld,
                        const kth::TopP &v, bool no_a, const float *us, int32_t *d_tok, int32_t *d_cnt) {
    if (p.slices == 1) {
        kth::k_sm_fused<K, VEC><<<(int)g, kth::WD_FBLOCK, 0, c->stream>>>(keys, ld, cols, v, us, d_tok, d_cnt);
        return launch_check();
    }
    const dim3 grid((unsigned)p.slices, (unsigned)g);
    const uint32_t sk = (uint32_t)p.slice_keys;
    kth::k_sm_max<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, c->sm_state.p, v);
    for (int phase = no_a ? 1 : 0; phase < 2; ++phase)
        for (int pass = 0; pass < K::PASSES; ++pass) {
            kth::k_sm_count<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, phase, pass, c->tp_mass.p,
                                                                        c->tp_cnt.p, c->sm_state.p, v);
            kth::k_sm_pick<K><<<(int)g, kth::WD_BLOCK, 0, c->stream>>>(c->tp_mass.p, c->tp_cnt.p, c->sm_state.p, phase, pass,
                                                                     cols, v, us);
        }
    kth::k_sm_loc_count<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, c->sm_state.p, c->sm_loc.p, v);
    kth::k_sm_loc_pick<K, VEC><<<grid, kth::WD_BLOCK, 0, c->stream>>>(keys, ld, cols, sk, c->sm_state.p, c->sm_loc.p, v,
                                                                   d_tok, d_cnt);
    return sequence_check(c->tp_dirty, c->sm_dirty);
}

// One token of every row.  The arguments have been checked.
template <class K>
int sample_rows(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, const kth::TopP &var, bool no_a,
                const float *d_us, int32_t *d_tok, int32_t *d_cnt) {
    using E = typename K::elem;
    return wide_rows_drive(c, static_cast<const E *>(d_keys), rows, cols, ld, SM_GROUP_MAX, reserve_sample,
                           [&](const WidePlan &p, bool vec, const E *gk, int64_t r0, int64_t g) {
                               const auto launch = vec ? launch_sample_group<K, true> : launch_sample_group<K, false>;
                               return launch(c, p, gk, g, (uint32_t)cols, (u64)ld, topp_at(var, r0), no_a, d_us + r0,
                                             d_tok + r0, ptr_at(d_cnt, r0));
                           });
}

// The two sample entry points: the argument check, then the rows.  kind: a
// KTH_K16_* float kind, or -1 for float32 keys.
int sample_entry(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, const int32_t *d_lens,
                 const int32_t *d_ks, int32_t k, const float *d_ps, float p, const float *d_temps, float temp,
                 const float *d_us, int kind, int32_t *d_tok, int32_t *d_cnt) {
    if (!wide_shape_ok(c, d_keys, rows, cols, ld) || !d_us || !d_tok || !topp_args_ok(kind, d_ps, p, temp))
        return KTH_EINVAL;
    if (rows == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    const kth::TopP var{d_lens, d_ps, d_temps, d_ks, p, temp, k};
    const bool no_a = !d_ps && p >= 1.0f && !d_ks && k <= 0;
    return topp_dispatch(
        kind, [&](auto K) { return sample_rows<decltype(K)>(c, d_keys, rows, cols, ld, var, no_a, d_us, d_tok, d_cnt); });
}

// Sorted top-k rows (kth_rows_sort.hpp): the form by k' = the power of two at
// or above k, the wave form's grid by its packing (64 / k' rows a wavefront,
// four wavefronts a workgroup), both bounded -- the kernels stride over rows.
static_assert(KTH_SORT_MAX_K == kth::SORT_MAX_K, "include/kth.h sorted top-k limit");
template <class T, int KP>
void launch_sort_wave(kth_ctx *c, typename T::elem *vals, int32_t *idx, int64_t rows, int32_t k, const int32_t *cnt,
                      uint32_t flip, int kind) {
    const int64_t rows_per_wg = (int64_t)(kth::WAVE / KP) * (kth::SORT_BLOCK / kth::WAVE);
    const int g = (int)std::min<int64_t>((rows + rows_per_wg - 1) / rows_per_wg, kth::SORT_GRID_MAX);
    kth::k_sort_wave<T, KP><<<g, kth::SORT_BLOCK, 0, c->stream>>>(vals, idx, (u64)rows, (uint32_t)k, cnt, flip, kind);
}

template <class T>
int launch_sort(kth_ctx *c, void *d_vals, int32_t *idx, int64_t rows, int32_t k, const int32_t *cnt, uint32_t flip,
                int kind) {
    typename T::elem *vals = static_cast<typename T::elem *>(d_vals);
    int kp = 2;
    while (kp < k) kp <<= 1;
    switch (kp) {
    case 2: launch_sort_wave<T, 2>(c, vals, idx, rows, k, cnt, flip, kind); break;
    case 4: launch_sort_wave<T, 4>(c, vals, idx, rows, k, cnt, flip, kind); break;
    case 8: launch_sort_wave<T, 8>(c, vals, idx, rows, k, cnt, flip, kind); break;
    case 16: launch_sort_wave<T, 16>(c, vals, idx, rows, k, cnt, flip, kind); break;
    case 32: launch_sort_wave<T, 32>(c, vals, idx, rows, k, cnt, flip, kind); break;
    case 64: launch_sort_wave<T, 64>(c, vals, idx, rows, k, cnt, flip, kind); break;
    default: {
        const int g = (int)std::min<int64_t>(rows, kth::SORT_GRID_MAX);
        kth::k_sort_wg<T><<<g, kth::SORT_BLOCK, (size_t)kp * sizeof(typename T::comp), c->stream>>>(
            vals, idx, (u64)rows, (uint32_t)k, cnt, flip, kind);
    }
    }
    return launch_check();
}

// The three sort entry points: the argument check, then the one launch.  kind:
// a KTH_K16_* value, -1 for float32 keys, -2 for int32 keys.  A row of one
// entry is sorted as it stands: k == 1 launches nothing.
int sort_entry(kth_ctx *c, void *d_vals, int32_t *d_idx, int64_t rows, int32_t k, const int32_t *d_cnt, int largest,
               int kind) {
    if (!c || !d_vals || rows < 0 || k < 1 || k > KTH_SORT_MAX_K || kind < -2 || kind > KTH_K16_BF16) return KTH_EINVAL;
    if (rows == 0 || k == 1) return KTH_OK;
    KTH_TRY(set_device(c));
    if (kind == -2) return launch_sort<kth::SortI32>(c, d_vals, d_idx, rows, k, d_cnt, largest ? 0xFFFFFFFFu : 0u, kind);
    if (kind == -1) return launch_sort<kth::SortF32>(c, d_vals, d_idx, rows, k, d_cnt, largest ? 0xFFFFFFFFu : 0u, kind);
    return launch_sort<kth::SortK16>(c, d_vals, d_idx, rows, k, d_cnt, largest ? 0xFFFFu : 0u, kind);
}

// ------------------------------------------------------- ctx creation, in parts
// Every tuning variable of a ctx (design exploration and A/B runs; unset: the
// defaults in kth_ctx).  Needs c->num_cu.  Read elsewhere: KTH_STAMPS (the
// stamps diagnostics, kth_ctx_create), KTH_WINDOW_Z (window_z, once a process)
// and KTH_DEBUG (error messages).
// (the fault injectors are not read from the environment: only
// kth_ctx_test_hook, which tests call explicitly, turns them on)
void read_tuning(kth_ctx *c) {
    if (const char *g = getenv("KTH_MAIN_WG_PER_CU")) c->main_wg_per_cu = std::max(0, atoi(g));
    if (const char *g = getenv("KTH_SPARSE_PER_WG")) c->sparse_per_wg = (u64)std::max(0, atoi(g));
    if (const char *g = getenv("KTH_DSCAN_PER_WG")) c->dscan_per_wg = (u64)std::max(1024, atoi(g));
    if (const char *g = getenv("KTH_POST_DENSE_GRID")) c->post_dense_grid = std::max(1, atoi(g));
    if (const char *g = getenv("KTH_POST_SPARSE_GRID")) c->post_sparse_grid = std::max(1, atoi(g));
    if (const char *g = getenv("KTH_COOP")) c->coop = atoi(g) != 0;
    if (const char *g = getenv("KTH_PRE_HIST")) c->pre_hist = atoi(g) != 0;
    if (const char *g = getenv("KTH_GROUP")) c->group = atoi(g) != 0;
    c->fin_grid = c->num_cu;
    if (const char *g = getenv("KTH_FIN_GRID")) c->fin_grid = std::max(1, std::min(atoi(g), c->num_cu));
    if (const char *g = getenv("KTH_HEAD_SLACK")) c->head_slack64 = (uint32_t)std::max(0.0, atof(g) * 64.0);
    if (const char *g = getenv("KTH_HEAD_ABS")) c->head_abs_div = (uint32_t)std::max(0, atoi(g));
    if (const char *g = getenv("KTH_TOPK_STAGE")) c->topk_stage = atoi(g) != 0;
}

// k_main<TF, F32>'s address; null for the float32 staged variants, which are not built
template <int TF, bool F32>
const void *main_fn() {
    if constexpr (F32 && TF >= 5)
        return nullptr;
    else
        return reinterpret_cast<const void *>(kth::k_main<TF, F32>);
}
template <bool F32>
std::array<const void *, 7> main_fns() {
    return {main_fn<0, F32>(), main_fn<1, F32>(), main_fn<2, F32>(), main_fn<3, F32>(),
            main_fn<4, F32>(), main_fn<5, F32>(), main_fn<6, F32>()};
}

// One resident wave of workgroups: every WG streams an equal share
// and no tail of late WGs.  Residency from each k_main variant's own
// VGPR and LDS use (4 waves per 256-thread WG = one per SIMD; a SIMD
// holds 512 / alloc(VGPR) waves, MI355X_MICROARCH.md register files);
// the top-k variants keep more keys live and may allocate more VGPRs.
// hipOccupancyMaxActiveBlocksPerMultiprocessor under-reports here.
template <bool F32>
std::array<const void *, 7 + MULTI_VARIANTS> pass_fns() {
    const std::array<const void *, 7> f = main_fns<F32>();
    return {f[0], f[1], f[2], f[3], f[4], f[5], f[6],
            reinterpret_cast<const void *>(kth::k_main_multi<2, F32>),
            reinterpret_cast<const void *>(kth::k_main_multi<4, F32>),
            reinterpret_cast<const void *>(kth::k_main_multi<8, F32>)};
}
int pass_grid(const kth_ctx *c, const void *fn) {
    int per = 4;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0) {
        const int alloc = (fa.numRegs + 7) / 8 * 8;
        const int by_vgpr = std::min(8, 512 / alloc);
        const int lds = (int)fa.sharedSizeBytes;
        const int by_lds = lds > 0 ? (160 * 1024) / lds : 8;
        per = std::max(1, std::min(by_vgpr, by_lds));
    }
    (void)hipGetLastError();
    if (c->main_wg_per_cu > 0) per = c->main_wg_per_cu;
    return c->num_cu * per;
}
void size_main_grids(kth_ctx *c) {
    // [key kind][TF] as c->main_grid, then the multi-rank variants as c->multi_grid
    const std::array<const void *, 7 + MULTI_VARIANTS> fns[2] = {pass_fns<false>(), pass_fns<true>()};
    for (int kind = 0; kind < 2; ++kind)
        for (int tf = 0; tf < 7 + MULTI_VARIANTS; ++tf) {
            if (!fns[kind][tf]) continue;
            (tf < 7 ? c->main_grid[kind][tf] : c->multi_grid[kind][tf - 7]) = pass_grid(c, fns[kind][tf]);
        }
}

// Workgroups a CU holds of k_finish<F32> and k_head<F32>; false when the
// occupancy query is unavailable.
template <bool F32>
bool coop_per_cu(int *fin, int *head) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(fin, reinterpret_cast<const void *>(kth::k_finish<F32>),
                                                        kth::DENSE_BLK, FIN_DYN_LDS) == hipSuccess &&
           hipOccupancyMaxActiveBlocksPerMultiprocessor(head, reinterpret_cast<const void *>(kth::k_head<F32>),
                                                        kth::DENSE_BLK, 0) == hipSuccess;
}

// Can the device hold k_finish's and k_head's grids at once?
// (both key kinds share the ctx's one coop switch: the smaller of
// the int32 and float32 instantiations' figures decides)
bool coop_grids_resident(const kth_ctx *c) {
    int fin[2] = {0, 0}, head[2] = {0, 0};
    const bool known = coop_per_cu<false>(&fin[0], &head[0]) && coop_per_cu<true>(&fin[1], &head[1]);
    (void)hipGetLastError();
    if (!known) return true;  // query unavailable: trust the static sizing
    return (int64_t)std::min(fin[0], fin[1]) * c->num_cu >= c->fin_grid &&
           (int64_t)std::min(head[0], head[1]) * c->num_cu >= HEAD_GRID_MAX;
}

}  // namespace

// ====================================================================== API
extern "C" {

const char *kth_strerror(int code) {
    switch (code) {
    case KTH_OK: return "ok";
    case KTH_EINVAL: return "invalid argument";
    case KTH_ENOMEM: return "out of memory";
    case KTH_EHIP: return "HIP runtime error";
    case KTH_ENODEV: return "no HIP device";
    case KTH_EINTERNAL: return "device-side consistency check failed";
    case KTH_ECOMM: return "RCCL unavailable or a collective failed";
    default: return "unknown error";
    }
}

int kth_version(void) { return KTH_VERSION; }

#ifndef KTH_BUILD_ID
#define KTH_BUILD_ID "unknown"
#endif
const char *kth_build_id(void) { return KTH_BUILD_ID; }

int kth_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int kth_ctx_create(int device, kth_ctx **out) {
    if (!out) return KTH_EINVAL;
    *out = nullptr;
    int ndev = kth_device_count();
    if (ndev <= 0) return KTH_ENODEV;
    if (device < 0 || device >= ndev) return KTH_EINVAL;
    kth_ctx *c = new kth_ctx();
    c->device = device;
    if (getenv("KTH_STAMPS")) {
        const size_t bytes = (size_t)STAMP_LAUNCHES * STAMP_WGS * 8 * 8;
        if (hipMalloc(reinterpret_cast<void **>(&c->stamps), bytes) != hipSuccess || hipMemset(c->stamps, 0, bytes) != hipSuccess) {
            (void)hipGetLastError();
            c->stamps = nullptr;
        }
    }
    int rc = KTH_OK;
    do {
        if (hipSetDevice(device) != hipSuccess) { rc = KTH_EHIP; break; }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            c->num_cu = prop.multiProcessorCount;
        read_tuning(c);
        size_main_grids(c);
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = KTH_EHIP; break; }
        c->own_stream = true;
        if (hipMalloc(reinterpret_cast<void **>(&c->st), 2 * sizeof(SelState)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&c->islots), SLOT_ALLOC_WORDS * sizeof(u64)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&c->d_status), 4 * sizeof(int32_t)) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void **>(&c->h_status), 4 * sizeof(int32_t), 0) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void **>(&c->h_state), sizeof(SelState), 0) != hipSuccess) {
            rc = KTH_ENOMEM;
            break;
        }
        if (hipMemset(c->st, 0, 2 * sizeof(SelState)) != hipSuccess ||
            hipMemset(c->d_status, 0, 4 * sizeof(int32_t)) != hipSuccess ||  // (LastCall: no selection yet)
            hipMemset(c->islots, 0, SLOT_ALLOC_WORDS * sizeof(u64)) != hipSuccess) {
            rc = KTH_EHIP;
            break;
        }
        // dynamic LDS beyond the 64 KiB default for the LDS / rows kernels
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_small<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, SMALL_N * 4);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_small<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, SMALL_N * 4);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_rows<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, KTH_ROWS_MAX_COLS * 4);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_rows<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, KTH_ROWS_MAX_COLS * 4);
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_finish<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIN_DYN_LDS) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(kth::k_finish<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIN_DYN_LDS) != hipSuccess)
            c->coop = false;  // no LDS-resident finish: per-level launches
        (void)hipGetLastError();
        // The grid barriers of k_head / k_finish need every workgroup resident
        // at once.  Their grids are sized for that (k_finish: one 1024-thread
        // workgroup per CU with ~145 KiB of LDS; k_head: at most 64
        // workgroups); check it against the occupancy query once, and refuse
        // the cooperative path when the device cannot hold the grid (a plain
        // launch checks nothing).  Residency can still be taken away at run
        // time by other streams or processes: the spins are bounded, a timeout
        // is reported (state error ERR_BARRIER, d_out untouched) and
        // kth_select_i32_ctx (hence kth_select_i32 and VecKthSelect) redoes the
        // select on the per-level path and stays on it for the next
        // COOP_BACKOFF synchronous selects.  The asynchronous entry points
        // (kth_select_i32_async, kth_topk_i32, kth_dist_*) report the error in
        // the state (kth_ctx_last_stats) and leave the retry to the caller.
        if (!coop_grids_resident(c)) {
            c->coop = false;
            c->coop_resident = false;
        }
    } while (0);
    c->coop_wanted = c->coop;
    if (rc != KTH_OK) {
        kth_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return KTH_OK;
}

int kth_ctx_test_hook(kth_ctx *c, int hook, int64_t value) {
    if (!c || value < 0) return KTH_EINVAL;
    switch (hook) {
    case KTH_HOOK_FAULT_TOPK_RANK: c->fault_topk_rank = value != 0; return KTH_OK;
    case KTH_HOOK_FAULT_BARRIER:
        if (value > 2) return KTH_EINVAL;
        c->fault_barrier = value != 0;
        c->fault_once = value == 2;
        return KTH_OK;
    case KTH_HOOK_TOPK_SEG_CAP:
        if (value > (int64_t)1 << 40) return KTH_EINVAL;
        c->topk_seg_cap = (u64)value;
        return KTH_OK;
    case KTH_HOOK_K16_MISS: c->k16_miss = value != 0; return KTH_OK;
    case KTH_HOOK_FINISH_SLICES: c->finish_slices = value != 0; return KTH_OK;
    case KTH_HOOK_K16_TOPK_NOSKIP: c->k16_topk_noskip = value != 0; return KTH_OK;
    default: return KTH_EINVAL;
    }
}

int kth_ctx_destroy(kth_ctx *c) {
    if (!c) return KTH_EINVAL;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev_main) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_total) (void)hipEventDestroy(e);
    if (c->st) (void)hipFree(c->st);
    if (c->islots) (void)hipFree(c->islots);
    release_all(c->sample, c->cand, c->gdir, c->cand_rows, c->tk_segv, c->tk_segp, c->tk_wcnt, c->tk_wstart, c->staging,
                c->topk, c->mstate, c->mslots, c->mcand, c->k16, c->k16st, c->tk16_nread, c->wide_hist, c->wide_state,
                c->wide_cnt, c->tp_mass, c->tp_cnt, c->tp_state, c->tp_rank, c->sm_state, c->sm_loc);
    if (c->d_mstatus) (void)hipFree(c->d_mstatus);
    if (c->h_mstatus) (void)hipHostFree(c->h_mstatus);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->stamps) (void)hipFree(c->stamps);
    if (c->h_status) (void)hipHostFree(c->h_status);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->h_dist) (void)hipHostFree(c->h_dist);
    if (c->ev_dist) (void)hipEventDestroy(c->ev_dist);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (tl_ctx == c) tl_ctx = nullptr;
    delete c;
    return KTH_OK;
}

int kth_ctx_set_stream(kth_ctx *c, void *s) {
    if (!c) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    if (c->own_stream && c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
        c->own_stream = false;
    }
    // NULL is HIP's null stream (what torch calls the default stream): it
    // orders against every blocking stream of the device, as a caller that
    // passes its "current stream" expects.
    c->stream = reinterpret_cast<hipStream_t>(s);
    return KTH_OK;
}

int kth_ctx_sync(kth_ctx *c) {
    if (!c) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KTH_OK;
}

int kth_ctx_reserve(kth_ctx *c, int64_t n) {
    if (!c || n < 0) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    return n > RADIX_MAX_N ? reserve_window(c, n) : KTH_OK;
}

int kth_select_i32_async(kth_ctx *c, const int32_t *d_keys, int64_t n, int64_t k, int32_t *d_out) {
    if (!d_out) return KTH_EINVAL;
    return select_async(c, d_keys, n, k, d_out, nullptr);
}

int kth_select_f32_async(kth_ctx *c, const float *d_keys, int64_t n, int64_t k, float *d_out) {
    if (!d_out) return KTH_EINVAL;
    return select_async<true>(c, reinterpret_cast<const int32_t *>(d_keys), n, k, reinterpret_cast<int32_t *>(d_out),
                              nullptr);
}

}  // extern "C"

namespace {

// One select into d_status, and [answer, error] fetched into h_status.
template <bool F32>
int select_fetch(kth_ctx *c, const int32_t *dk, int64_t n, int64_t k) {
    KTH_TRY(select_async<F32>(c, dk, n, k, nullptr, c->d_status));
    HIP_TRY(hipMemcpyAsync(c->h_status, c->d_status, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KTH_OK;
}

// The synchronous select through a ctx, either key kind (the words travel as
// int32; *out receives the caller's word: for float32 the answer's bits).
template <bool F32>
int select_ctx(kth_ctx *c, const int32_t *keys, int64_t n, int64_t k, int32_t *out) {
    if (!c || !keys || !out || n < 1 || k < 1 || k > n) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const int32_t *dk = keys;
    if (!is_device_ptr(keys)) {
        KTH_TRY(c->staging.reserve((u64)n));
        HIP_TRY(hipMemcpyAsync(c->staging.p, keys, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        dk = c->staging.p;
    }
    KTH_TRY(select_fetch<F32>(c, dk, n, k));
    if (c->h_status[1] == (int32_t)kth::ERR_BARRIER && c->coop) {
        // a cooperative grid was not co-resident (another stream or process
        // held CUs): redo the select on the per-level path, which needs no
        // residency; the slots are re-zeroed first (dirty)
        // (sticky for COOP_BACKOFF synchronous selects: while the CUs stay
        // contended, every cooperative launch would spin out its barriers)
        c->dirty = true;
        c->coop = false;
        c->coop_backoff = COOP_BACKOFF + 1;  // (the retry below counts one)
        KTH_TRY(select_fetch<F32>(c, dk, n, k));
    }
    if (c->h_status[1] != 0) {
        c->dirty = true;
        return KTH_EINTERNAL;
    }
    // d_status[0] is the ordered word (the top-k kernels compare against it);
    // a float32 answer is its order key turned back into bits
    *out = F32 ? (int32_t)kth::f32_of_key((uint32_t)c->h_status[0] ^ 0x80000000u) : c->h_status[0];
    return KTH_OK;
}

// The one-shot entry points' ctx: created on first use, one per host thread.
int thread_ctx() {
    if (tl_ctx) return KTH_OK;
    int dev = 0;
    if (kth_device_count() <= 0) return KTH_ENODEV;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    return kth_ctx_create(dev, &tl_ctx);
}

template <bool F32>
int select_oneshot(const int32_t *keys, int64_t n, int64_t k, int32_t *out) {
    if (!keys || !out || n < 1 || k < 1 || k > n) return KTH_EINVAL;
    KTH_TRY(thread_ctx());
    return select_ctx<F32>(tl_ctx, keys, n, k, out);
}

// ------------------------------------------------ several ranks of one array
// kth_select_multi_*: up to KTH_MULTI_MAX_RANKS ranks of the same keys.  On
// the window path with the cooperative kernels: k_head per distinct rank (each
// into its own set), ONE k_main_multi over the input, k_finish per distinct
// rank.  Otherwise (n <= RADIX_MAX_N, the per-level path, or one distinct
// rank) the distinct ranks go one after the other through the single select's
// launches, and each one's final state is copied into its set for
// kth_ctx_multi_stats.
bool multi_args_ok(const void *keys, int64_t n, const int64_t *ks, int m, const void *out) {
    if (!keys || !ks || !out || n < 1 || m < 1 || m > KTH_MULTI_MAX_RANKS) return false;
    for (int i = 0; i < m; ++i)
        if (ks[i] < 1 || ks[i] > n) return false;
    return true;
}

// candidate buffers of a multi call lie this many words apart (256-byte
// aligned, so that k_finish reads each with 16-byte loads)
u64 multi_stride(u64 cap) { return (cap + 63) & ~(u64)63; }

// Scratch of a multi call of m ranks over n keys: the sets (states, slots,
// status words: fixed size, made once) and, for the window path, m candidate
// buffers of the single select's capacity each (at 2^30 keys: 2^25 keys = 128
// MiB a rank, 1 GiB for eight) beside the single select's own scratch, which
// the per-level path uses.
// [answer, error] per rank of a multi call, on the device and pinned
int reserve_mstatus(kth_ctx *c) {
    if (!c->d_mstatus && hipMalloc(reinterpret_cast<void **>(&c->d_mstatus), 2 * KTH_MULTI_MAX_RANKS * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        c->d_mstatus = nullptr;
        return KTH_ENOMEM;
    }
    if (!c->h_mstatus && hipHostMalloc(reinterpret_cast<void **>(&c->h_mstatus), 2 * KTH_MULTI_MAX_RANKS * sizeof(int32_t), 0) != hipSuccess) {
        (void)hipGetLastError();
        c->h_mstatus = nullptr;
        return KTH_ENOMEM;
    }
    return KTH_OK;
}

int reserve_multi(kth_ctx *c, int64_t n, int m) {
    if (c->mslots.count == 0) {
        KTH_TRY(c->mstate.reserve(2 * (u64)KTH_MULTI_MAX_RANKS));
        KTH_TRY(c->mslots.reserve((u64)KTH_MULTI_MAX_RANKS * MSET_WORDS));
        HIP_TRY(hipMemsetAsync(c->mstate.p, 0, c->mstate.count * sizeof(SelState), c->stream));
        HIP_TRY(hipMemsetAsync(c->mslots.p, 0, c->mslots.count * sizeof(u64), c->stream));
    }
    KTH_TRY(reserve_mstatus(c));
    if (n <= RADIX_MAX_N) return KTH_OK;
    KTH_TRY(reserve_window(c, n));
    return c->mcand.reserve((u64)m * multi_stride(cand_capacity(n)));
}

// The distinct ranks of a multi call (a duplicate is resolved once): dk[j],
// first[j] = the first i with ks[i] == dk[j]; c->multi_set[i] = the j of ks[i].
int distinct_ranks(kth_ctx *c, const int64_t *ks, int m, int64_t *dk, int *first) {
    int D = 0;
    for (int i = 0; i < m; ++i) {
        int j = 0;
        while (j < D && dk[j] != ks[i]) ++j;
        if (j == D) {
            dk[D] = ks[i];
            first[D++] = i;
        }
        c->multi_set[i] = j;
    }
    c->multi_m = m;
    return D;
}

template <bool F32>
void launch_main_multi(kth_ctx *c, const kth::MultiArgs &ma) {
    const int v = ma.m <= 2 ? 0 : ma.m <= 4 ? 1 : 2;  // as c->multi_grid
    const int g = c->multi_grid[F32][v];
    switch (v) {
    case 0: kth::k_main_multi<2, F32><<<g, kth::BLK, 0, c->stream>>>(ma); break;
    case 1: kth::k_main_multi<4, F32><<<g, kth::BLK, 0, c->stream>>>(ma); break;
    default: kth::k_main_multi<8, F32><<<g, kth::BLK, 0, c->stream>>>(ma); break;
    }
}

// The one-pass path over D distinct ranks: rank j's answer to outs[j] (device,
// may be null) and its [answer, error] to d_status + 2 j (may be null).  Each
// rank's chain is run_window's cooperative one over its own set; the ctx's
// k_finish slot sets, barrier words and tail buffer serve the launches in
// turn (they are stream-ordered).
template <bool F32>
int run_multi_window(kth_ctx *c, const int32_t *keys, int64_t n, const int64_t *ks, int D, int32_t *const *outs,
                     int32_t *d_status) {
    const int64_t s = sample_size(n);
    const u64 nchunks = ((u64)s + kth::SAMPLE_CHUNK - 1) / kth::SAMPLE_CHUNK;
    const u64 stride = (u64)n / nchunks;
    const u64 cap = cand_capacity(n), cstride = multi_stride(cap);
    RankSet sets[KTH_MULTI_MAX_RANKS];
    Chain chains[KTH_MULTI_MAX_RANKS] = {};
    u64 *head_slots[KTH_MULTI_MAX_RANKS];
    kth::MultiArgs ma;
    memset(&ma, 0, sizeof ma);
    ma.keys = keys;
    ma.n = (u64)n;
    ma.m = D;
    for (int j = 0; j < D; ++j) {
        u64 *slots = c->mslots.p + (size_t)j * MSET_WORDS;
        head_slots[j] = slots + MSET_HSLOT_OFF;
        sets[j] = RankSet{c->mstate.p + 2 * (size_t)j, slots + 3 * (size_t)kth::STATS_WORDS,
                          c->mcand.p + (size_t)j * cstride, cap};
        // sample phase -> this rank's window in state 0 of its set (the
        // single select's window: the same early-window floor)
        Chain ch{c, slots, 2, &sets[j]};
        u64 r_lo, r_hi;
        window_ranks(n, ks[j], s, &r_lo, &r_hi);
        StepArgs a = head_step(ch, n, ks[j], s, r_lo, r_hi, true);
        kth::CoopArgs hx = coop_args(c, 0, nullptr, nullptr);
        hx.slots = head_slots[j];
        if (c->head_abs_div) hx.abs_min = (u64)s / c->head_abs_div;
        kth::k_head<F32><<<gather_grid(nchunks), kth::DENSE_BLK, 0, c->stream>>>(a, hx, keys, (u64)n, stride,
                                                                               c->sample.p, (u64)s);
        a = ch.next(kth::ADV_CARRY, Chain::ACC);
        ma.w[j] = kth::MultiWin{a.st_in, a.st_out, a.stats_acc, a.cand_count, sets[j].cand, a.cap};
        chains[j] = ch;
    }
    ev_main(c);
    launch_main_multi<F32>(c, ma);
    ev_main(c);
    for (int j = 0; j < D; ++j) {
        StepArgs a = chains[j].next(kth::ADV_DECIDE, Chain::IN);
        over_keys(a, keys, n);
        launch_finish<F32>(c, a, outs[j], d_status ? d_status + 2 * j : nullptr, c->multi_tag, false, head_slots[j]);
    }
    return launch_check();
}

// d_out: m answers on the device, or null; status: also [answer, error] per
// distinct rank into c->d_mstatus (set j = c->multi_set[i] resolved rank i).
template <bool F32>
int multi_async(kth_ctx *c, const int32_t *d_keys, int64_t n, const int64_t *ks, int m, int32_t *d_out, bool status) {
    KTH_TRY(set_device(c));
    coop_tick(c);  // one selection, however many ranks
    int64_t dk[KTH_MULTI_MAX_RANKS];
    int first[KTH_MULTI_MAX_RANKS];
    const int D = distinct_ranks(c, ks, m, dk, first);
    KTH_TRY(reserve_multi(c, n, D));
    int32_t *outs[KTH_MULTI_MAX_RANKS];
    for (int j = 0; j < D; ++j) outs[j] = d_out ? d_out + first[j] : nullptr;
    int32_t *d_status = status ? c->d_mstatus : nullptr;
    int rc = KTH_OK;
    // every final launch below leaves the call's LastCall word: the set of its last rank
    // (multi_tag is set for the launches of this call only, whichever way it returns)
    struct TagScope {
        kth_ctx *c;
        ~TagScope() { c->multi_tag = 0; }
    } tag_scope{c};
    c->multi_tag = c->multi_word = last_word(LAST_MULTI, F32, c->multi_set[m - 1]);
    // (one distinct rank is the single select: k_main<0> alone is HBM-bound,
    // 0.70 against 0.78 ms at 2^30 through k_main_multi)
    if (n > RADIX_MAX_N && c->coop && D > 1) {
        if (c->dirty || c->count_kept) {
            HIP_TRY(hipMemsetAsync(c->islots, 0, SLOT_ALLOC_WORDS * sizeof(u64), c->stream));
            c->dirty = c->count_kept = false;
        }
        if (c->multi_dirty) {
            HIP_TRY(hipMemsetAsync(c->mslots.p, 0, c->mslots.count * sizeof(u64), c->stream));
            c->multi_dirty = false;
        }
        c->multi_cap = cand_capacity(n);
        ev_mark(c, c->ev_total, c->total_used);
        rc = run_multi_window<F32>(c, d_keys, n, dk, D, outs, d_status);
        ev_mark(c, c->ev_total, c->total_used);
        if (c->stamps) dump_stamps(c);
    } else {
        for (int j = 0; j < D && rc == KTH_OK; ++j) {
            rc = select_enqueue<F32>(c, d_keys, n, dk[j], outs[j], d_status ? d_status + 2 * j : nullptr);
            if (rc == KTH_OK && hipMemcpyAsync(c->mstate.p + 2 * (size_t)j, c->st + c->last_state, sizeof(SelState),
                                               hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                rc = KTH_EHIP;
        }
        c->multi_cap = c->cand.count;
    }
    if (rc != KTH_OK) {
        c->dirty = c->multi_dirty = true;
        return rc;
    }
    if (d_out)
        for (int i = 0; i < m; ++i)
            if (first[c->multi_set[i]] != i)
                HIP_TRY(hipMemcpyAsync(d_out + i, d_out + first[c->multi_set[i]], sizeof(int32_t),
                                       hipMemcpyDeviceToDevice, c->stream));
    return KTH_OK;
}

// One multi call with its status words fetched into h_mstatus.
template <bool F32>
int multi_fetch(kth_ctx *c, const int32_t *dk, int64_t n, const int64_t *ks, int m) {
    KTH_TRY(multi_async<F32>(c, dk, n, ks, m, nullptr, true));
    HIP_TRY(hipMemcpyAsync(c->h_mstatus, c->d_mstatus, 2 * KTH_MULTI_MAX_RANKS * sizeof(int32_t), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KTH_OK;
}

// The synchronous multi call through a ctx, either key kind (as select_ctx).
template <bool F32>
int multi_ctx(kth_ctx *c, const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out) {
    if (!c || !multi_args_ok(keys, n, ks, m, out)) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const int32_t *dk = keys;
    if (!is_device_ptr(keys)) {
        KTH_TRY(c->staging.reserve((u64)n));
        HIP_TRY(hipMemcpyAsync(c->staging.p, keys, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        dk = c->staging.p;
    }
    KTH_TRY(multi_fetch<F32>(c, dk, n, ks, m));
    auto any_error = [&](bool barrier_only) {
        for (int i = 0; i < m; ++i) {
            const int32_t e = c->h_mstatus[2 * c->multi_set[i] + 1];
            if (barrier_only ? e == (int32_t)kth::ERR_BARRIER : e != 0) return true;
        }
        return false;
    };
    if (c->coop && any_error(true)) {
        // a cooperative grid was not co-resident: redo every rank on the
        // per-level path and stay on it, as select_ctx does
        c->dirty = c->multi_dirty = true;
        c->coop = false;
        c->coop_backoff = COOP_BACKOFF + 1;  // (the retry below counts one)
        KTH_TRY(multi_fetch<F32>(c, dk, n, ks, m));
    }
    if (any_error(false)) {
        c->dirty = c->multi_dirty = true;
        return KTH_EINTERNAL;
    }
    for (int i = 0; i < m; ++i) {
        const int32_t w = c->h_mstatus[2 * c->multi_set[i]];
        out[i] = F32 ? (int32_t)kth::f32_of_key((uint32_t)w ^ 0x80000000u) : w;
    }
    return KTH_OK;
}

template <bool F32>
int multi_oneshot(const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out) {
    if (!multi_args_ok(keys, n, ks, m, out)) return KTH_EINVAL;
    KTH_TRY(thread_ctx());
    return multi_ctx<F32>(tl_ctx, keys, n, ks, m, out);
}

template <bool F32>
int multi_entry_async(kth_ctx *c, const int32_t *d_keys, int64_t n, const int64_t *ks, int m, int32_t *d_out) {
    if (!c || !multi_args_ok(d_keys, n, ks, m, d_out)) return KTH_EINVAL;
    return multi_async<F32>(c, d_keys, n, ks, m, d_out, false);
}

// ---------------------------------------------------------- 16-bit keys
// kth_select_k16* / kth_select_multi_k16*: kth_k16.hpp's launches.  A single
// select is a call with one rank.  Kernel boundaries only: no cooperative
// launch, so the ctx's coop state is neither read nor counted down.
bool k16_args_ok(const void *keys, int64_t n, const int64_t *ks, int m, int kind, const void *out) {
    return kind >= KTH_K16_I16 && kind <= KTH_K16_BF16 && multi_args_ok(keys, n, ks, m, out);
}

template <int CV>
const void *k16_main_fn() {
    return reinterpret_cast<const void *>(kth::k16_main<CV>);
}
template <int CV>
const void *k16_main_tf_fn() {
    return reinterpret_cast<const void *>(kth::k16_main_tf<CV>);
}

// Scratch of every k16 call, whatever n and m: the sample histogram, a set of
// bins per rank and the states (~1.3 MB), the status words.
int reserve_k16(kth_ctx *c) {
    if (c->k16.count == 0) {
        KTH_TRY(c->k16.reserve(K16_BUF_WORDS));
        KTH_TRY(c->k16st.reserve(KTH_MULTI_MAX_RANKS));
        HIP_TRY(hipMemsetAsync(c->k16.p, 0, c->k16.count * sizeof(u64), c->stream));
        HIP_TRY(hipMemsetAsync(c->k16st.p, 0, c->k16st.count * sizeof(kth::K16State), c->stream));
    }
    KTH_TRY(reserve_mstatus(c));
    if (!c->k16_ready) {
        const void *hist[3] = {reinterpret_cast<const void *>(kth::k16_hist<0>), reinterpret_cast<const void *>(kth::k16_hist<1>),
                               reinterpret_cast<const void *>(kth::k16_hist<2>)};
        for (const void *f : hist) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K16_HIST_LDS));
        const void *mains[3] = {k16_main_fn<0>(), k16_main_fn<1>(), k16_main_fn<2>()};
        for (int v = 0; v < 3; ++v) c->k16_grid[v] = pass_grid(c, mains[v]);
        const void *flagged[3] = {k16_main_tf_fn<0>(), k16_main_tf_fn<1>(), k16_main_tf_fn<2>()};
        for (int v = 0; v < 3; ++v) c->k16_tf_grid[v] = pass_grid(c, flagged[v]);
        c->k16_ready = true;
    }
    return KTH_OK;
}

// tf (kth_topk_k16, D == 1): pass 0 is the flag-recording k16_main_tf; the
// later passes, which return at once unless the window missed, stay unflagged.
template <int CV>
int run_k16(kth_ctx *c, const uint16_t *keys, int64_t n, const int64_t *dk, int D, int kind, const kth::K16Out &out,
            const kth::K16Flags *tf = nullptr) {
    const bool small = n <= kth::K16_SMALL_N;
    const int64_t s = small ? n : sample_size(n);
    const u64 nchunks = ((u64)s + kth::K16_CHUNK - 1) / kth::K16_CHUNK;
    const u64 stride = small ? (u64)kth::K16_CHUNK : (u64)n / nchunks;
    const uint32_t nl = kth::k16_nl(kind), top = kth::k16_top(kind);
    const uint32_t nl2 = nl | nl << 16, top2 = top | top << 16;
    uint32_t *shist = reinterpret_cast<uint32_t *>(c->k16.p);
    u64 *bins = c->k16.p + K16_SHIST_WORDS;
    const int hist_grid = (int)(((u64)s + kth::K16_HIST_PER_WG - 1) / kth::K16_HIST_PER_WG);

    if (small) ev_main(c);
    kth::k16_hist<CV><<<hist_grid, kth::K16_HIST_BLK, K16_HIST_LDS, c->stream>>>(keys, (u64)n, (u64)s, stride, nl2, top2, shist);
    if (small) ev_main(c);
    kth::K16PickArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.shist = shist;
    pa.st = c->k16st.p;
    pa.D = D;
    pa.small = small;
    pa.miss = c->k16_miss;
    pa.n = (u64)n;
    pa.C = (uint32_t)(kth::K16_FIELDS / 2) / (D <= 1 ? 1u : D <= 2 ? 2u : D <= 4 ? 4u : 8u);
    pa.top = top;
    for (int j = 0; j < D; ++j) {
        pa.k[j] = (u64)dk[j];
        if (!small) window_ranks(n, dk[j], s, &pa.rlo[j], &pa.rhi[j]);
    }
    pa.out = out;
    pa.last = d_last(c);
    pa.last_word = c->multi_word = last_word(LAST_K16, false, c->multi_set[out.m - 1], kind);
    kth::k16_pick<<<1, kth::K16_HIST_BLK, 0, c->stream>>>(pa);
    if (!small) {
        const kth::K16Args ma{keys, (u64)n, D, nl2, top2, c->k16st.p, bins};
        const kth::K16FinArgs fa{c->k16st.p, bins, top, out};
        for (int pass = 0; pass < kth::K16_PASSES; ++pass) {  // (the later ones return at once when every rank is settled)
            if (pass == 0) ev_main(c);
            if (pass == 0 && tf)
                kth::k16_main_tf<CV><<<c->k16_tf_grid[CV], kth::BLK, 0, c->stream>>>(ma, *tf);
            else
                kth::k16_main<CV><<<c->k16_grid[CV], kth::BLK, 0, c->stream>>>(ma);
            if (pass == 0) ev_main(c);
            kth::k16_finish<<<D, kth::K16_HIST_BLK, 0, c->stream>>>(fa);
        }
    }
    return launch_check();
}

// d_out: m answers on the device, or null; status: also [bits, error] per
// distinct rank into c->d_mstatus.
int k16_async(kth_ctx *c, const uint16_t *d_keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *d_out,
              bool status) {
    KTH_TRY(set_device(c));
    int64_t dk[KTH_MULTI_MAX_RANKS];
    int first[KTH_MULTI_MAX_RANKS];
    const int D = distinct_ranks(c, ks, m, dk, first);
    KTH_TRY(reserve_k16(c));
    if (c->k16_dirty) {
        HIP_TRY(hipMemsetAsync(c->k16.p, 0, c->k16.count * sizeof(u64), c->stream));
        c->k16_dirty = false;
    }
    kth::K16Out out;
    memset(&out, 0, sizeof out);
    out.m = m;
    out.kind = kind;
    for (int i = 0; i < m; ++i) out.set[i] = c->multi_set[i];
    out.d_out = d_out;
    out.d_status = status ? c->d_mstatus : nullptr;
    ev_mark(c, c->ev_total, c->total_used);
    const int rc = kind == KTH_K16_U16   ? run_k16<0>(c, d_keys, n, dk, D, kind, out)
                   : kind == KTH_K16_I16 ? run_k16<1>(c, d_keys, n, dk, D, kind, out)
                                         : run_k16<2>(c, d_keys, n, dk, D, kind, out);
    ev_mark(c, c->ev_total, c->total_used);
    if (rc != KTH_OK) c->k16_dirty = true;
    return rc;
}

// The synchronous call through a ctx: host keys are staged, the status words
// are read once.
int k16_ctx(kth_ctx *c, const void *keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *out) {
    if (!c || !k16_args_ok(keys, n, ks, m, kind, out)) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const uint16_t *dk = static_cast<const uint16_t *>(keys);
    if (!is_device_ptr(keys)) {
        KTH_TRY(c->staging.reserve(((u64)n + 1) / 2));
        HIP_TRY(hipMemcpyAsync(c->staging.p, keys, (size_t)n * 2, hipMemcpyHostToDevice, c->stream));
        dk = reinterpret_cast<const uint16_t *>(c->staging.p);
    }
    KTH_TRY(k16_async(c, dk, n, ks, m, kind, nullptr, true));
    HIP_TRY(hipMemcpyAsync(c->h_mstatus, c->d_mstatus, 2 * KTH_MULTI_MAX_RANKS * sizeof(int32_t), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; ++i)
        if (c->h_mstatus[2 * c->multi_set[i] + 1] != 0) {
            c->k16_dirty = true;
            return KTH_EINTERNAL;
        }
    for (int i = 0; i < m; ++i) out[i] = (uint16_t)c->h_mstatus[2 * c->multi_set[i]];
    return KTH_OK;
}

int k16_oneshot(const void *keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *out) {
    if (!k16_args_ok(keys, n, ks, m, kind, out)) return KTH_EINVAL;
    KTH_TRY(thread_ctx());
    return k16_ctx(tl_ctx, keys, n, ks, m, kind, out);
}

int k16_entry_async(kth_ctx *c, const void *d_keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *d_out) {
    if (!c || !k16_args_ok(d_keys, n, ks, m, kind, d_out)) return KTH_EINVAL;
    return k16_async(c, static_cast<const uint16_t *>(d_keys), n, ks, m, kind, d_out, false);
}

}  // namespace

extern "C" {

int kth_select_i32_ctx(kth_ctx *c, const int32_t *keys, int64_t n, int64_t k, int32_t *out) {
    return select_ctx<false>(c, keys, n, k, out);
}

int kth_select_f32_ctx(kth_ctx *c, const float *keys, int64_t n, int64_t k, float *out) {
    return select_ctx<true>(c, reinterpret_cast<const int32_t *>(keys), n, k, reinterpret_cast<int32_t *>(out));
}

int kth_select_i32(const int32_t *keys, int64_t n, int64_t k, int32_t *out) {
    return select_oneshot<false>(keys, n, k, out);
}

int kth_select_f32(const float *keys, int64_t n, int64_t k, float *out) {
    return select_oneshot<true>(reinterpret_cast<const int32_t *>(keys), n, k, reinterpret_cast<int32_t *>(out));
}

int kth_select_multi_i32(const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out) {
    return multi_oneshot<false>(keys, n, ks, m, out);
}
int kth_select_multi_i32_ctx(kth_ctx *c, const int32_t *keys, int64_t n, const int64_t *ks, int m, int32_t *out) {
    return multi_ctx<false>(c, keys, n, ks, m, out);
}
int kth_select_multi_i32_async(kth_ctx *c, const int32_t *d_keys, int64_t n, const int64_t *ks, int m,
                               int32_t *d_out) {
    return multi_entry_async<false>(c, d_keys, n, ks, m, d_out);
}
int kth_select_multi_f32(const float *keys, int64_t n, const int64_t *ks, int m, float *out) {
    return multi_oneshot<true>(reinterpret_cast<const int32_t *>(keys), n, ks, m, reinterpret_cast<int32_t *>(out));
}
int kth_select_multi_f32_ctx(kth_ctx *c, const float *keys, int64_t n, const int64_t *ks, int m, float *out) {
    return multi_ctx<true>(c, reinterpret_cast<const int32_t *>(keys), n, ks, m, reinterpret_cast<int32_t *>(out));
}
int kth_select_multi_f32_async(kth_ctx *c, const float *d_keys, int64_t n, const int64_t *ks, int m, float *d_out) {
    return multi_entry_async<true>(c, reinterpret_cast<const int32_t *>(d_keys), n, ks, m,
                                   reinterpret_cast<int32_t *>(d_out));
}
int kth_ctx_reserve_multi(kth_ctx *c, int64_t n, int m) {
    if (!c || n < 0 || m < 1 || m > KTH_MULTI_MAX_RANKS) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    return reserve_multi(c, n, m);
}

int kth_select_k16(const void *keys, int64_t n, int64_t k, int kind, uint16_t *out) {
    return k16_oneshot(keys, n, &k, 1, kind, out);
}
int kth_select_k16_ctx(kth_ctx *c, const void *keys, int64_t n, int64_t k, int kind, uint16_t *out) {
    return k16_ctx(c, keys, n, &k, 1, kind, out);
}
int kth_select_k16_async(kth_ctx *c, const void *d_keys, int64_t n, int64_t k, int kind, uint16_t *d_out) {
    return k16_entry_async(c, d_keys, n, &k, 1, kind, d_out);
}
int kth_select_multi_k16(const void *keys, int64_t n, const int64_t *ks, int m, int kind, uint16_t *out) {
    return k16_oneshot(keys, n, ks, m, kind, out);
}
int kth_select_multi_k16_ctx(kth_ctx *c, const void *keys, int64_t n, const int64_t *ks, int m, int kind,
                             uint16_t *out) {
    return k16_ctx(c, keys, n, ks, m, kind, out);
}
int kth_select_multi_k16_async(kth_ctx *c, const void *d_keys, int64_t n, const int64_t *ks, int m, int kind,
                               uint16_t *d_out) {
    return k16_entry_async(c, d_keys, n, ks, m, kind, d_out);
}
int kth_ctx_reserve_k16(kth_ctx *c, int64_t n, int m) {
    if (!c || n < 0 || m < 1 || m > KTH_MULTI_MAX_RANKS) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    return reserve_k16(c);
}
uint16_t kth_k16_order_key(uint16_t bits, int kind) { return kth::k16_key_of_bits(bits, kind); }
uint16_t kth_k16_of_order_key(uint16_t key, int kind) { return kth::k16_bits_of_key(key, kind); }

uint32_t kth_f32_order_key(float x) {
    uint32_t b;
    memcpy(&b, &x, sizeof b);
    return kth::key_of_f32(b);
}

float kth_f32_of_order_key(uint32_t key) {
    const uint32_t b = kth::f32_of_key(key);
    float x;
    memcpy(&x, &b, sizeof x);
    return x;
}

int kth_ctx_coop(const kth_ctx *c) {
    if (!c) return KTH_EINVAL;
    return c->coop ? 1 : 0;
}

}  // extern "C"

namespace {

// The ctx's LastCall word, read from the device (synchronises the ctx stream).
int fetch_last(kth_ctx *c, LastCall *last) {
    KTH_TRY(set_device(c));
    HIP_TRY(hipMemcpyAsync(c->h_status + 2, d_last(c), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *last = last_of_word((uint32_t)c->h_status[2]);
    return KTH_OK;
}

// A selection state on the device as kth_stats (synchronises the ctx stream).
int fetch_stats(kth_ctx *c, const SelState *d_state, u64 capacity, bool f32, kth_stats *out) {
    KTH_TRY(set_device(c));
    HIP_TRY(hipMemcpyAsync(c->h_state, d_state, sizeof(SelState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const SelState &s = *c->h_state;
    memset(out, 0, sizeof *out);
    out->path = (int32_t)s.path;
    out->mode = (int32_t)s.mode;
    out->lo_key = s.lo;
    out->hi_key = s.hi;
    out->n = s.n;
    out->k = s.k;
    out->cnt_lt = s.cnt[kth::C_LT];
    out->cnt_eq_lo = s.cnt[kth::C_EQLO];
    out->cnt_eq_hi = s.cnt[kth::C_EQHI];
    out->candidates = s.cnt[kth::C_IN];
    out->capacity = capacity;
    out->answer = f32 ? (int32_t)kth::f32_of_key(s.answer) : (int32_t)(s.answer ^ 0x80000000u);
    out->error = (int32_t)s.error;
    return KTH_OK;
}

// Rank set j of the last 16-bit call (keys of `kind`): the window as order keys, the answer's bits.
int fetch_stats_k16(kth_ctx *c, int j, int kind, kth_stats *out) {
    KTH_TRY(set_device(c));
    kth::K16State *h = reinterpret_cast<kth::K16State *>(c->h_state);
    static_assert(sizeof(kth::K16State) <= sizeof(SelState), "the pinned state buffer holds either");
    HIP_TRY(hipMemcpyAsync(h, c->k16st.p + j, sizeof *h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->path = (int32_t)h->path;
    out->mode = (int32_t)h->mode;
    out->lo_key = kth::k16_key_of_ord(h->lo, kind);
    out->hi_key = kth::k16_key_of_ord(h->hi, kind);
    out->n = h->n;
    out->k = h->k;
    out->cnt_lt = h->cnt_lt;
    out->candidates = h->inside;
    out->answer = (int32_t)kth::k16_bits_of_ord(h->answer, kind);
    out->error = (int32_t)h->error;
    return KTH_OK;
}

// The final state LastCall names.
int last_stats(kth_ctx *c, const LastCall &last, kth_stats *out) {
    switch (last.form) {
    case LAST_K16: return fetch_stats_k16(c, last.index, last.k16_kind, out);
    case LAST_MULTI: return fetch_stats(c, c->mstate.p + 2 * (size_t)last.index, c->multi_cap, last.f32, out);
    case LAST_SINGLE: return fetch_stats(c, c->st + (last.index & 1), c->cand.count, last.f32, out);
    default: return KTH_EINVAL;  // no selection yet
    }
}

// Rank i of the multi or 16-bit call that ran last: the state of its set, a
// multi call's state 0.  The map from i to a set is the host's record of the
// last such call enqueued or captured here, so it serves only while what ran
// last on the device is a call of that form and key kind: KTH_EINVAL after a
// single select or a call of another kind (a replayed graph, for instance).
int multi_stats(kth_ctx *c, int i, kth_stats *out) {
    if (!c || !out || i < 0 || i >= c->multi_m) return KTH_EINVAL;
    LastCall last;
    KTH_TRY(fetch_last(c, &last));
    const LastCall mine = last_of_word(c->multi_word);
    if (last.form != mine.form || last.f32 != mine.f32 || last.k16_kind != mine.k16_kind) return KTH_EINVAL;
    last.index = c->multi_set[i];
    return last_stats(c, last, out);
}

}  // namespace

extern "C" {

int kth_ctx_multi_stats(kth_ctx *c, int i, kth_stats *out) { return multi_stats(c, i, out); }

int kth_ctx_last_stats(kth_ctx *c, kth_stats *out) {
    if (!c || !out) return KTH_EINVAL;
    LastCall last;
    KTH_TRY(fetch_last(c, &last));
    return last_stats(c, last, out);
}

int kth_ctx_last_finish_form(kth_ctx *c, int *form) {
    if (!c || !form) return KTH_EINVAL;
    LastCall last;
    KTH_TRY(fetch_last(c, &last));
    if (last.form == LAST_NONE) return KTH_EINVAL;  // no selection yet
    *form = (int)((uint32_t)c->h_status[2] >> kth::LAST_FORM_SHIFT & 7u);
    return KTH_OK;
}

int kth_ctx_enable_timing(kth_ctx *c, int on) {
    if (!c) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    if (on && c->ev_main.empty()) {
        c->ev_main.resize(MAX_EVENTS);
        c->ev_total.resize(MAX_EVENTS);
        for (auto &e : c->ev_main) HIP_TRY(hipEventCreate(&e));
        for (auto &e : c->ev_total) HIP_TRY(hipEventCreate(&e));
    }
    c->timing = on != 0;
    c->main_used = c->total_used = 0;
    return KTH_OK;
}

int kth_ctx_take_timing(kth_ctx *c, int64_t *n_sel, double *main_ms, double *total_ms) {
    if (!c || !n_sel || !main_ms || !total_ms) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double m = 0, t = 0;
    int64_t nm = 0;
    for (int i = 0; i + 1 < c->main_used; i += 2) {
        float a = 0;
        HIP_TRY(hipEventElapsedTime(&a, c->ev_main[i], c->ev_main[i + 1]));
        m += a;
        nm++;
    }
    for (int i = 0; i + 1 < c->total_used; i += 2) {
        float b = 0;
        HIP_TRY(hipEventElapsedTime(&b, c->ev_total[i], c->ev_total[i + 1]));
        t += b;
    }
    c->main_used = c->total_used = 0;
    *n_sel = nm;
    *main_ms = m;
    *total_ms = t;
    return KTH_OK;
}

int kth_select_rows_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int32_t k, int32_t *d_out) {
    return rows_entry<false, false>(c, d_keys, rows, cols, k, d_out);
}

int kth_select_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int32_t k, float *d_out) {
    return rows_entry<true, false>(c, d_keys, rows, cols, k, d_out);
}

int kth_topk_rows_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int32_t k, int largest,
                      int32_t *d_vals, int32_t *d_idx) {
    return rows_entry<false, true>(c, d_keys, rows, cols, k, nullptr, largest, d_vals, d_idx);
}

int kth_topk_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int32_t k, int largest,
                      float *d_vals, int32_t *d_idx) {
    return rows_entry<true, true>(c, d_keys, rows, cols, k, nullptr, largest, d_vals, d_idx);
}

int kth_select_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int32_t k, int kind,
                        uint16_t *d_out) {
    return rows16_entry<false>(c, d_keys, rows, cols, k, kind, d_out);
}

int kth_topk_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int32_t k, int largest, int kind,
                      uint16_t *d_vals, int32_t *d_idx) {
    return rows16_entry<true>(c, d_keys, rows, cols, k, kind, nullptr, largest, d_vals, d_idx);
}

int kth_select_wide_rows_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                             int32_t *d_out) {
    return wide_rows_entry<false, false>(c, d_keys, rows, cols, ld, k, d_out);
}

int kth_select_wide_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                             float *d_out) {
    return wide_rows_entry<true, false>(c, d_keys, rows, cols, ld, k, d_out);
}

int kth_topk_wide_rows_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                           int largest, int32_t *d_vals, int32_t *d_idx) {
    return wide_rows_entry<false, true>(c, d_keys, rows, cols, ld, k, nullptr, largest, d_vals, d_idx);
}

int kth_topk_wide_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                           int largest, float *d_vals, int32_t *d_idx) {
    return wide_rows_entry<true, true>(c, d_keys, rows, cols, ld, k, nullptr, largest, d_vals, d_idx);
}

int kth_ctx_reserve_wide_rows(kth_ctx *c, int64_t rows, int32_t cols) {
    if (!c || !wide_dims_ok(rows, cols)) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    // for the split form whatever the plan of (rows, cols) is: a forced plan then fits too
    return reserve_wide(c, std::min(std::max<int64_t>(rows, 1), WIDE_GROUP_MAX));
}

int kth_wide_rows_plan(int64_t rows, int32_t cols, int num_cu, int32_t *slices, int32_t *slice_keys,
                       int32_t *group_rows, int64_t *scratch_bytes) {
    return wide_plan_out(4, rows, cols, num_cu, slices, slice_keys, group_rows, scratch_bytes);
}

int kth_ctx_wide_rows_force(kth_ctx *c, int32_t slices, int32_t group_rows) {
    if (!c || slices < 0 || group_rows < 0 || slices > KTH_WIDE_MAX_SLICES) return KTH_EINVAL;
    c->wide_force_slices = slices;
    c->wide_force_group = group_rows;
    return KTH_OK;
}

int kth_select_wide_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                             int kind, uint16_t *d_out) {
    return wide16_rows_entry<false>(c, d_keys, rows, cols, ld, k, kind, d_out);
}

int kth_topk_wide_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld, int32_t k,
                           int largest, int kind, uint16_t *d_vals, int32_t *d_idx) {
    return wide16_rows_entry<true>(c, d_keys, rows, cols, ld, k, kind, nullptr, largest, d_vals, d_idx);
}

int kth_wide_rows_plan_k16(int64_t rows, int32_t cols, int num_cu, int32_t *slices, int32_t *slice_keys,
                           int32_t *group_rows, int64_t *scratch_bytes) {
    return wide_plan_out(2, rows, cols, num_cu, slices, slice_keys, group_rows, scratch_bytes);
}

int kth_select_wide_rows_var_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, int32_t *d_out) {
    return wide_rows_entry<false, false, true>(c, d_keys, rows, cols, ld, k, d_out, 0, nullptr, nullptr,
                                               kth::WideVar{d_lens, d_ks, nullptr});
}

int kth_select_wide_rows_var_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, float *d_out) {
    return wide_rows_entry<true, false, true>(c, d_keys, rows, cols, ld, k, d_out, 0, nullptr, nullptr,
                                              kth::WideVar{d_lens, d_ks, nullptr});
}

int kth_select_wide_rows_var_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                                 const int32_t *d_lens, const int32_t *d_ks, int32_t k, int kind, uint16_t *d_out) {
    return wide16_rows_entry<false, true>(c, d_keys, rows, cols, ld, k, kind, d_out, 0, nullptr, nullptr,
                                          kth::WideVar{d_lens, d_ks, nullptr});
}

int kth_topk_wide_rows_var_i32(kth_ctx *c, const int32_t *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, int32_t *d_vals,
                               int32_t *d_idx, int32_t *d_cnt) {
    return wide_rows_entry<false, true, true>(c, d_keys, rows, cols, ld, k, nullptr, largest, d_vals, d_idx,
                                              kth::WideVar{d_lens, d_ks, d_cnt});
}

int kth_topk_wide_rows_var_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, float *d_vals,
                               int32_t *d_idx, int32_t *d_cnt) {
    return wide_rows_entry<true, true, true>(c, d_keys, rows, cols, ld, k, nullptr, largest, d_vals, d_idx,
                                             kth::WideVar{d_lens, d_ks, d_cnt});
}

int kth_topk_wide_rows_var_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                               const int32_t *d_lens, const int32_t *d_ks, int32_t k, int largest, int kind,
                               uint16_t *d_vals, int32_t *d_idx, int32_t *d_cnt) {
    return wide16_rows_entry<true, true>(c, d_keys, rows, cols, ld, k, kind, nullptr, largest, d_vals, d_idx,
                                         kth::WideVar{d_lens, d_ks, d_cnt});
}

int kth_nucleus_wide_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                              const int32_t *d_lens, const float *d_ps, float p, const float *d_temps, float temp,
                              int32_t *d_n, float *d_thr) {
    return topp_entry<false>(c, d_keys, rows, cols, ld, d_lens, nullptr, 0, d_ps, p, d_temps, temp, -1, d_n, d_thr,
                             nullptr, nullptr, nullptr);
}

int kth_nucleus_wide_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                              const int32_t *d_lens, const float *d_ps, float p, const float *d_temps, float temp,
                              int kind, int32_t *d_n, uint16_t *d_thr) {
    if (kind < KTH_K16_I16 || kind > KTH_K16_BF16) return KTH_EINVAL;
    return topp_entry<false>(c, d_keys, rows, cols, ld, d_lens, nullptr, 0, d_ps, p, d_temps, temp, kind, d_n, d_thr,
                             nullptr, nullptr, nullptr);
}

int kth_topp_wide_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                           const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                           const float *d_temps, float temp, float *d_vals, int32_t *d_idx, int32_t *d_cnt) {
    return topp_entry<true>(c, d_keys, rows, cols, ld, d_lens, d_ks, k, d_ps, p, d_temps, temp, -1, nullptr, nullptr,
                            d_vals, d_idx, d_cnt);
}

int kth_topp_wide_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                           const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                           const float *d_temps, float temp, int kind, uint16_t *d_vals, int32_t *d_idx,
                           int32_t *d_cnt) {
    if (kind < KTH_K16_I16 || kind > KTH_K16_BF16) return KTH_EINVAL;
    return topp_entry<true>(c, d_keys, rows, cols, ld, d_lens, d_ks, k, d_ps, p, d_temps, temp, kind, nullptr, nullptr,
                            d_vals, d_idx, d_cnt);
}

int kth_ctx_reserve_topp_rows(kth_ctx *c, int64_t rows, int32_t cols) {
    if (!c || !wide_dims_ok(rows, cols)) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    // the split form of both sequences whatever the plan of (rows, cols) is: a forced plan then fits too
    KTH_TRY(reserve_topp(c, std::min(std::max<int64_t>(rows, 1), TP_GROUP_MAX)));
    KTH_TRY(c->tp_rank.reserve((u64)std::max<int64_t>(rows, 1)));
    return reserve_wide(c, std::min(std::max<int64_t>(rows, 1), WIDE_GROUP_MAX));
}

int kth_sample_wide_rows_f32(kth_ctx *c, const float *d_keys, int64_t rows, int32_t cols, int64_t ld,
                             const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                             const float *d_temps, float temp, const float *d_us, int32_t *d_tok, int32_t *d_cnt) {
    return sample_entry(c, d_keys, rows, cols, ld, d_lens, d_ks, k, d_ps, p, d_temps, temp, d_us, -1, d_tok, d_cnt);
}

int kth_sample_wide_rows_k16(kth_ctx *c, const void *d_keys, int64_t rows, int32_t cols, int64_t ld,
                             const int32_t *d_lens, const int32_t *d_ks, int32_t k, const float *d_ps, float p,
                             const float *d_temps, float temp, const float *d_us, int kind, int32_t *d_tok,
                             int32_t *d_cnt) {
    if (kind < KTH_K16_I16 || kind > KTH_K16_BF16) return KTH_EINVAL;
    return sample_entry(c, d_keys, rows, cols, ld, d_lens, d_ks, k, d_ps, p, d_temps, temp, d_us, kind, d_tok, d_cnt);
}

int kth_ctx_reserve_sample_rows(kth_ctx *c, int64_t rows, int32_t cols) {
    if (!c || !wide_dims_ok(rows, cols)) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    // the split form whatever the plan of (rows, cols) is: a forced plan then fits too
    return reserve_sample(c, std::min(std::max<int64_t>(rows, 1), SM_GROUP_MAX));
}

int kth_sort_topk_rows_i32(kth_ctx *c, int32_t *d_vals, int32_t *d_idx, int64_t rows, int32_t k, const int32_t *d_cnt,
                           int largest) {
    return sort_entry(c, d_vals, d_idx, rows, k, d_cnt, largest, -2);
}

int kth_sort_topk_rows_f32(kth_ctx *c, float *d_vals, int32_t *d_idx, int64_t rows, int32_t k, const int32_t *d_cnt,
                           int largest) {
    return sort_entry(c, d_vals, d_idx, rows, k, d_cnt, largest, -1);
}

int kth_sort_topk_rows_k16(kth_ctx *c, uint16_t *d_vals, int32_t *d_idx, int64_t rows, int32_t k, const int32_t *d_cnt,
                           int largest, int kind) {
    if (kind < KTH_K16_I16 || kind > KTH_K16_BF16) return KTH_EINVAL;
    return sort_entry(c, d_vals, d_idx, rows, k, d_cnt, largest, kind);
}

}  // extern "C"

namespace {

// Top-k of one array, either key kind.  float32 keys never take the staged
// variant (k_main<5/6>: its segments hold the caller's words and k_tk5_write
// copies them out): that k range goes through the row-word path (tf 3 / 4),
// which is exact for every k.
template <bool F32>
int topk_impl(kth_ctx *c, const int32_t *d_keys, int64_t n, int64_t k, int largest, int32_t *d_vals,
              int64_t *d_idx) {
    if (!c || !d_keys || (!d_vals && !d_idx) || n < 1 || k < 1 || k > n) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const u64 ntiles = ((u64)n + kth::TK_TILE - 1) / kth::TK_TILE;
    const u64 nblk = (ntiles + kth::TK_TILES_PER_BLOCK - 1) / kth::TK_TILES_PER_BLOCK;
    // k_main's tile geometry (its flags cover the full tiles after the unaligned head)
    u64 head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(d_keys) & 15u)) & 15u) >> 2;
    if (head > (u64)n) head = (u64)n;
    const u64 nfull = (((u64)n - head) >> 2) / ((u64)kth::BLK * kth::MAIN_UNROLL);
    // k_main's top-k records (only on the window path, n > RADIX_MAX_N):
    //   16-byte aligned keys: per wave-row counts + candidate rows, and the
    //   count pass loads no tile k_main covered (tf 3 / 4) -- unless k is so
    //   small that the rows holding output are a few per cent (k * 64 Ki <=
    //   n: one flag bit per row, the count pass loads only flagged tiles,
    //   tf 1 / 2; measured ~equal there, and it needs no alignment)
    //   and for n / 64 Ki < k <= n / 16 (16-byte aligned), every key on the
    //   kept side of the window's far edge staged in index order (tf 5 / 6):
    //   neither the count nor the write pass reads the input (KTH_TOPK_STAGE=0: tf 3 / 4)
    const bool aligned = (reinterpret_cast<uintptr_t>(d_keys) & 15u) == 0;
    const bool window = n > RADIX_MAX_N;
    const bool few = (u64)k * kth::TK_TILE * 64 <= (u64)n;
    const bool staged = !F32 && aligned && window && !few && (u64)k * TK_STAGE_MAX_FRAC <= (u64)n && c->topk_stage;
    const int tf = staged                                  ? (largest ? 6 : 5)
                   : (aligned && window && !few)           ? (largest ? 4 : 3)
                   : (u64)k * kth::TK_TILE <= (u64)n ? (largest ? 2 : 1)
                                                             : 0;
    const u64 ncov = tf >= 3 ? nfull * kth::MAIN_UNROLL : 0;  // tiles = k_main rows (head == 0)
    // tflags: the header and TF 1 / 2's flag bytes after 4 words, TF >= 3's
    // row words after TF_W0 in per-wave segments (kth::rw_index); 256-byte
    // aligned, so that a wave's group of 64 words fills one line
    const u64 Gm = (u64)c->main_grid[F32][tf];  // k_main<tf, F32>'s workgroups
    const kth::RowWords rwl{Gm, tf >= 3 ? kth::rw_seg_words(nfull, Gm) : kth::fl_seg_bytes(nfull, Gm)};
    const u64 fwords = tf >= 3 ? kth::TF_W0 + rwl.G * (kth::BLK / kth::WAVE) * rwl.seg
                               : 4 + rwl.G * (kth::BLK / kth::WAVE) * rwl.seg / 4;
    const u64 fw64 = (fwords + 1) / 2, before = (ntiles + 1) / 2 + ntiles + 4 * nblk + 2;
    const u64 words = before + fw64 + 32;
    KTH_TRY(c->topk.reserve(words));
    const u64 foff = (before + 31) & ~31ull;  // + fw64 <= words
    uint32_t *tflags = reinterpret_cast<uint32_t *>(c->topk.p + foff);
    HIP_TRY(hipMemsetAsync(tflags, 0, 16, c->stream));  // window header: not valid until k_main<TF> runs
    if (tf == 3 || tf == 4) KTH_TRY(reserve_cand(c, n, true));
    u64 seg_cap = 0;
    uint32_t nwin = 0;
    if (tf >= 5) {  // the staging segments: one per k_main wave, n / 16 entries in all
        const u64 nwaves = Gm * (kth::BLK / kth::WAVE);
        // entries: the k kept keys, the candidates (~0.6 % of n at 2^30) and the
        // waves' imbalance; a segment that overflows sends the top-k to the
        // input-reading path (exact)
        const u64 seg_total = std::max<u64>({1ull << 20, (u64)n / 16, (u64)k + (u64)k / 8 + (u64)n / 64});
        seg_cap = c->topk_seg_cap ? c->topk_seg_cap : (seg_total + nwaves - 1) / nwaves;
        seg_cap = (seg_cap + 3) & ~3ull;  // segments start 16-byte aligned (k_main<5/6> stores 4 entries a lane)
        KTH_TRY(reserve_cand(c, n));
        KTH_TRY(c->tk_segv.reserve(seg_cap * nwaves));
        KTH_TRY(c->tk_segp.reserve(seg_cap * nwaves));
        KTH_TRY(c->tk_wcnt.reserve(ncov * (kth::BLK / kth::WAVE) + 4));
        // per wave and window (TK5_WIN_TILES of its tiles): the entries staged before it
        nwin = (uint32_t)(((nfull + Gm - 1) / Gm + kth::TK5_WIN_TILES - 1) / kth::TK5_WIN_TILES);
        KTH_TRY(c->tk_wstart.reserve(nwaves * std::max(nwin, 1u)));
        // dense staging (k >= n / 32) stores the segments non-temporally: k_main<5> at k = 2^26 964-976
        // against 980-984 us, whole calls -0.5 to -2 %; at k = 2^24 k_main<5> gains ~6 us but
        // k_tk5_count, which then reads the entries from HBM, loses ~8; at 2^20 +0.8 %
        // (profiles/r6_topk_seg_store_ab.txt)
        const uint32_t nt = (u64)k * 32 >= (u64)n ? 1u : 0u;
        c->tk_seg = kth::TkSeg{c->tk_segv.p, c->tk_segp.p, (uint32_t)seg_cap, tflags + 3, c->tk_wstart.p, nwin, nt};
    }
    // the k-th smallest (largest: the (n-k+1)-th smallest) -> d_status[0], on the device
    int64_t rank = largest ? n - k + 1 : k;
    if (c->fault_topk_rank && n > 1) rank = rank < n ? rank + 1 : rank - 1;
    KTH_TRY(select_async<F32>(c, d_keys, n, rank, nullptr, c->d_status, tf, tflags));
    const uint32_t *keys = reinterpret_cast<const uint32_t *>(d_keys);
    const uint32_t flip = largest ? 0xFFFFFFFFu : 0u;
    u64 *toff = c->topk.p, *bsum = toff + ntiles, *bbase = bsum + 2 * nblk, *meta = bbase + 2 * nblk;
    uint32_t *tcnt = reinterpret_cast<uint32_t *>(meta + 2);
    const SelState *sel_st = c->st + c->last_state;
    // count and write passes: one wave per 64 tiles
    const int waves = kth::TK_BLOCK / kth::WAVE;
    const int g = (int)std::min<u64>((ntiles + waves * kth::WAVE - 1) / (waves * kth::WAVE), (u64)c->num_cu * 16);
    if (tf >= 5) {  // the staged entries (rows < ncov), then the ragged rows from the input
        auto tk5c = (u64)k * 64 >= (u64)n ? kth::k_tk5_count<true> : kth::k_tk5_count<false>;  // dense windows: chunked
        tk5c<<<(int)Gm * TK5_SPLIT, kth::TK_BLOCK, 0, c->stream>>>(
            c->tk_segv.p, seg_cap, c->tk_wstart.p, nwin, Gm, tflags, nfull, c->d_status, flip, c->tk_wcnt.p, tcnt);
        kth::k_topk_count<true, 2><<<g, kth::TK_BLOCK, 0, c->stream>>>(keys, (u64)n, ntiles, c->d_status, flip, tcnt,
                                                                       tflags, head, nfull, sel_st, ncov);
    } else if (tf >= 3) {  // candidates' share first (atomics into zeroed counts), then the rows' words
        HIP_TRY(hipMemsetAsync(tcnt, 0, ntiles * 4, c->stream));
        kth::k_topk_cands<<<c->num_cu * 8, kth::TK_BLOCK, 0, c->stream>>>(
            c->cand.p, c->cand_rows.p, cand_count(c), c->cand.count, c->d_status, flip, tcnt, tflags, sel_st);
        if (c->count_kept) {  // the per-level select left the count for the kernel above: nothing reads it now
            HIP_TRY(hipMemsetAsync(cand_count(c), 0, sizeof(u64), c->stream));
            c->count_kept = false;
        }
        kth::k_topk_count<true, 1, F32><<<g, kth::TK_BLOCK, 0, c->stream>>>(
            keys, (u64)n, ntiles, c->d_status, flip, tcnt, tflags, head, nfull, sel_st, ncov, rwl);
    } else if (aligned) {
        kth::k_topk_count<true, 0, F32><<<g, kth::TK_BLOCK, 0, c->stream>>>(
            keys, (u64)n, ntiles, c->d_status, flip, tcnt, tflags, head, nfull, sel_st, 0, rwl);
    } else {
        kth::k_topk_count<false, 0, F32><<<g, kth::TK_BLOCK, 0, c->stream>>>(
            keys, (u64)n, ntiles, c->d_status, flip, tcnt, tflags, head, nfull, sel_st, 0, rwl);
    }
    // tile offsets, block bases and need in one launch (a bracket failure --
    // counts that do not hold the k-th -- lands in the select's state, where
    // kth_ctx_last_stats reports it as .error)
    kth::k_topk_bases<<<(int)nblk, kth::TK_BLOCK, 0, c->stream>>>(
        tcnt, ntiles, toff, bsum, (u64)k, bbase, meta, c->st + c->last_state,
        reinterpret_cast<uint32_t *>(c->islots + BAR_OFF) + kth::BAR_TOPK_ARRIVE);
    if (tf >= 5) {
        auto tk5w = (u64)k * 32 <= (u64)n ? kth::k_tk5_write<kth::TK5_STAGE_SMALL> : kth::k_tk5_write<kth::TK5_STAGE_LARGE>;
        tk5w<<<(int)Gm * TK5_SPLIT, kth::TK_BLOCK, 0, c->stream>>>(
            c->tk_segv.p, c->tk_segp.p, seg_cap, c->tk_wstart.p, nwin, Gm, tflags, nfull, c->d_status, flip,
            c->tk_wcnt.p, tcnt, toff, bbase, meta, d_vals, d_idx);
        kth::k_topk_write<true, true><<<g, kth::TK_BLOCK, 0, c->stream>>>(keys, (u64)n, ntiles, c->d_status, flip,
                                                                          tcnt, toff, bbase, meta, d_vals, d_idx,
                                                                          tflags, ncov);
    } else if (aligned)
        kth::k_topk_write<true, false, F32><<<g, kth::TK_BLOCK, 0, c->stream>>>(
            keys, (u64)n, ntiles, c->d_status, flip, tcnt, toff, bbase, meta, d_vals, d_idx);
    else
        kth::k_topk_write<false, false, F32><<<g, kth::TK_BLOCK, 0, c->stream>>>(
            keys, (u64)n, ntiles, c->d_status, flip, tcnt, toff, bbase, meta, d_vals, d_idx);
    return launch_check();
}

// ---------------------------------------------------- top-k of 16-bit keys
// kth_topk_k16 (kth_topk16.hpp): the 16-bit select of rank k (largest: n - k +
// 1) with one rank and no output, then count, k_topk_bases and write.  One
// copy of the sequence, instantiated per ord transform and alignment.
// The flagged streaming pass (k16_main_tf) is taken for k <= n / 16384, the
// rule the 32-bit top-k's row flags started from scaled to this pass's
// geometry: were every output key alone in its 2048-key row, at most an eighth
// of the rows could hold output, and the count pass loads the rest of the
// input a second time above it for little.  (Not yet moved by a measurement:
// DESIGN.md "Top-k of one 16-bit array".)  Above it the unflagged k16_main
// runs and the count pass reads every tile.
constexpr u64 TK16_FLAG_FRAC = 16384;

struct Tk16Plan {
    u64 ntiles, nblk, pad, head, nfull;
    bool tf;
    u64 *toff, *bsum, *bbase, *meta, *nread;
    uint32_t *tcnt, *hdr;
};

template <int CV, bool ALIGNED>
int topk16_run(kth_ctx *c, const uint16_t *keys, int64_t n, int64_t k, int64_t rank, int largest, int kind,
               const Tk16Plan &p, uint16_t *d_vals, int64_t *d_idx) {
    int64_t dk[KTH_MULTI_MAX_RANKS];
    int first[KTH_MULTI_MAX_RANKS];
    const int D = distinct_ranks(c, &rank, 1, dk, first);  // one rank, set 0
    kth::K16Out out;
    memset(&out, 0, sizeof out);
    out.m = 1;
    out.kind = kind;
    out.set[0] = c->multi_set[0];
    const kth::K16Flags fl{p.hdr, largest ? 1u : 0u};
    KTH_TRY(run_k16<CV>(c, keys, n, dk, D, kind, out, p.tf ? &fl : nullptr));
    kth::K16State *st = c->k16st.p + c->multi_set[0];
    const uint32_t nl = kth::k16_nl(kind), top = kth::k16_top(kind);
    const kth::Tk16Args a{keys, (u64)n, p.pad, p.ntiles, st, largest ? 0xFFFFu : 0u, nl | nl << 16, top | top << 16, p.tcnt};
    const kth::Tk16Skip sk{p.hdr, p.head, p.nfull, p.tf && !c->k16_topk_noskip ? 1u : 0u, p.nread};
    const kth::Tk16Out o{p.toff, p.bbase, p.meta, st, kth::k16_float(kind) ? kth::k16_inf(kind) : 0xFFFFu,
                         (uint32_t)kth::k16_bits_of_ord(top, kind), d_vals, d_idx};
    // count and write passes: one wave per 64 tiles
    const int waves = kth::TK_BLOCK / kth::WAVE;
    const int g = (int)std::min<u64>((p.ntiles + waves * kth::WAVE - 1) / (waves * kth::WAVE), (u64)c->num_cu * 16);
    HIP_TRY(hipMemsetAsync(p.nread, 0, sizeof(u64), c->stream));
    kth::k16_topk_count<CV, ALIGNED><<<g, kth::TK_BLOCK, 0, c->stream>>>(a, sk);
    // (a null SelState: k16_topk_write carries a bracket failure to the 16-bit state)
    kth::k_topk_bases<<<(int)p.nblk, kth::TK_BLOCK, 0, c->stream>>>(
        p.tcnt, p.ntiles, p.toff, p.bsum, (u64)k, p.bbase, p.meta, nullptr,
        reinterpret_cast<uint32_t *>(c->islots + BAR_OFF) + kth::BAR_TOPK_ARRIVE);
    kth::k16_topk_write<CV, ALIGNED><<<g, kth::TK_BLOCK, 0, c->stream>>>(a, o);
    return launch_check();
}

int topk16_impl(kth_ctx *c, const void *d_keys, int64_t n, int64_t k, int largest, int kind, uint16_t *d_vals,
                int64_t *d_idx) {
    if (!c || !d_keys || (!d_vals && !d_idx) || n < 1 || k < 1 || k > n || kind < KTH_K16_I16 || kind > KTH_K16_BF16)
        return KTH_EINVAL;
    KTH_TRY(set_device(c));
    KTH_TRY(reserve_k16(c));
    const uint16_t *keys = static_cast<const uint16_t *>(d_keys);
    Tk16Plan p;
    // tiles in virtual indices: pad keys lie between the 16-byte boundary below d_keys and d_keys
    p.pad = (reinterpret_cast<uintptr_t>(keys) & 15u) >> 1;
    p.ntiles = ((u64)n + p.pad + kth::TK16_TILE - 1) / kth::TK16_TILE;
    p.nblk = (p.ntiles + kth::TK_TILES_PER_BLOCK - 1) / kth::TK_TILES_PER_BLOCK;
    // k16_main's geometry: its rows start after `head` unaligned keys
    p.head = std::min<u64>((8 - p.pad) & 7, (u64)n);
    p.nfull = (((u64)n - p.head) >> 3) / ((u64)kth::BLK * kth::K16_UNROLL);
    p.tf = n > kth::K16_SMALL_N && (u64)k * TK16_FLAG_FRAC <= (u64)n;
    // scratch (u64 words): offsets, block sums and bases, meta, the counts,
    // then the flag header and a 32-bit word per k16_main tile
    const u64 before = p.ntiles + 4 * p.nblk + 2 + (p.ntiles + 1) / 2;
    const u64 fw64 = (4 + p.nfull + 1) / 2;
    KTH_TRY(c->topk.reserve(before + fw64 + 2));
    KTH_TRY(c->tk16_nread.reserve(2));
    p.toff = c->topk.p;
    p.bsum = p.toff + p.ntiles;
    p.bbase = p.bsum + 2 * p.nblk;
    p.meta = p.bbase + 2 * p.nblk;
    p.nread = c->tk16_nread.p;
    p.tcnt = reinterpret_cast<uint32_t *>(p.meta + 2);
    p.hdr = reinterpret_cast<uint32_t *>(c->topk.p + before);
    if (c->k16_dirty) {
        HIP_TRY(hipMemsetAsync(c->k16.p, 0, c->k16.count * sizeof(u64), c->stream));
        c->k16_dirty = false;
    }
    // the k-th smallest (largest: the (n-k+1)-th smallest) -> K16State[0].answer, on the device
    int64_t rank = largest ? n - k + 1 : k;
    if (c->fault_topk_rank && n > 1) rank = rank < n ? rank + 1 : rank - 1;
    const bool aligned = p.pad == 0;
    ev_mark(c, c->ev_total, c->total_used);
    int rc;
    switch ((kind == KTH_K16_U16 ? 0 : kind == KTH_K16_I16 ? 1 : 2) * 2 + (aligned ? 1 : 0)) {
    case 0: rc = topk16_run<0, false>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    case 1: rc = topk16_run<0, true>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    case 2: rc = topk16_run<1, false>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    case 3: rc = topk16_run<1, true>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    case 4: rc = topk16_run<2, false>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    default: rc = topk16_run<2, true>(c, keys, n, k, rank, largest, kind, p, d_vals, d_idx); break;
    }
    ev_mark(c, c->ev_total, c->total_used);
    if (rc != KTH_OK) {
        c->k16_dirty = true;
        return rc;
    }
    c->tk16_tiles = p.ntiles;
    return KTH_OK;
}

}  // namespace

extern "C" {

int kth_topk_k16(kth_ctx *c, const void *d_keys, int64_t n, int64_t k, int largest, int kind, uint16_t *d_vals,
                 int64_t *d_idx) {
    return topk16_impl(c, d_keys, n, k, largest, kind, d_vals, d_idx);
}

int kth_ctx_last_topk_k16_tiles(kth_ctx *c, uint64_t *tiles, uint64_t *tiles_read) {
    if (!c || !tiles || !tiles_read || c->tk16_tiles == 0) return KTH_EINVAL;  // no kth_topk_k16 yet
    KTH_TRY(set_device(c));
    u64 *h = reinterpret_cast<u64 *>(c->h_state);  // pinned
    HIP_TRY(hipMemcpyAsync(h, c->tk16_nread.p, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *tiles = c->tk16_tiles;
    *tiles_read = *h;
    return KTH_OK;
}

int kth_topk_i32(kth_ctx *c, const int32_t *d_keys, int64_t n, int64_t k, int largest, int32_t *d_vals,
                 int64_t *d_idx) {
    return topk_impl<false>(c, d_keys, n, k, largest, d_vals, d_idx);
}

int kth_topk_f32(kth_ctx *c, const float *d_keys, int64_t n, int64_t k, int largest, float *d_vals, int64_t *d_idx) {
    return topk_impl<true>(c, reinterpret_cast<const int32_t *>(d_keys), n, k, largest,
                           reinterpret_cast<int32_t *>(d_vals), d_idx);
}

int kth_fill_synthetic(kth_ctx *c, int32_t *d_out, int64_t n, int64_t offset, int64_t n_total, int dist, uint64_t seed,
                       int32_t param) {
    if (!c || (!d_out && n > 0) || n < 0 || offset < 0 || dist < 0 || dist > 7) return KTH_EINVAL;
    if (n == 0) return KTH_OK;
    KTH_TRY(set_device(c));
    uint32_t step = 1;
    if (n_total > 0 && n_total <= (int64_t)0xFFFFFFFFll) {
        u64 s = (1ull << 32) / (u64)n_total;
        step = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (s ? (uint32_t)s : 1u);
    }
    const int g = (int)std::min<int64_t>((n + kth::BLK - 1) / kth::BLK, (int64_t)c->num_cu * 16);
    kth::k_fill<<<g, kth::BLK, 0, c->stream>>>(d_out, (u64)n, (u64)offset, step, dist, seed, param);
    return launch_check();
}

// ------------------------------------------------------- sharded protocol
int64_t kth_dist_sample_size(int64_t n) { return sample_size(n); }

int kth_sample_chunk(void) { return kth::SAMPLE_CHUNK; }

double kth_window_z(void) { return window_z(); }

int64_t kth_dist_cand_capacity(int64_t n_local) { return (int64_t)cand_capacity(std::max<int64_t>(n_local, 1)); }

int kth_window_slack64(void) { return (int)(HEAD_SLACK * 64); }

int kth_dist_begin(kth_ctx *c, uint64_t *d_slots, int64_t n_total, int64_t k) {
    if (!c || !d_slots || n_total < 1 || k < 1 || k > n_total) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    if (!c->h_dist) {  // level 0's DistStatus: host-visible memory the kernel writes, an event after it
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_dist), kth::DIST_STATUS_WORDS * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            c->h_dist = nullptr;
            return KTH_ENOMEM;
        }
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->d_dist), c->h_dist, 0));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_dist, hipEventDisableTiming));
    }
    coop_tick(c);
    c->uslots = reinterpret_cast<u64 *>(d_slots);
    c->dist_n = n_total;
    c->dist_k = k;
    c->dist_level_next = -1;  // kth_dist_scan first
    c->dist_levels = -1;
    c->dist_result_slot = -1;
    c->dist_early_out = nullptr;
    c->dist_zero = true;  // kth_dist_sample clears the slots inside its kernel
    // the ctx's own slots are left zeroed by every completed k_result; a
    // sequence cut short (dirty, or a dist selection never finished) re-zeroes,
    // and so does a cooperative single-GPU window select, which leaves its
    // count slot and candidate count for its next k_head to clear (the
    // streaming pass would append after a stale count, and the candidate
    // levels would histogram the previous select's keys)
    if (c->dirty || c->dist_open || c->counts_left || c->count_kept)
        HIP_TRY(hipMemsetAsync(c->islots, 0, SLOT_ALLOC_WORDS * sizeof(u64), c->stream));
    c->dirty = c->count_kept = false;
    c->counts_left = false;
    c->dist_open = true;
    return KTH_OK;
}

int kth_dist_sample(kth_ctx *c, const int32_t *d_keys, int64_t n_local, uint32_t *d_sample, int64_t s_local) {
    if (!c || !d_keys || !d_sample || s_local < 64 || s_local % 64 || n_local < s_local) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const u64 nchunks = ((u64)s_local + kth::SAMPLE_CHUNK - 1) / kth::SAMPLE_CHUNK;
    const u64 stride = (u64)n_local / nchunks;
    StepArgs a;
    memset(&a, 0, sizeof a);
    if (c->dist_zero && c->uslots) {
        a.stats_zero = c->uslots;
        a.zero_words = 3 * (u64)KTH_STATS_WORDS;
    }
    kth::k_gather<false><<<gather_grid(nchunks), kth::DENSE_BLK, 0, c->stream>>>(a, d_keys, (u64)n_local, stride, d_sample,
                                                                                (u64)s_local);
    KTH_TRY(launch_check());
    if (a.zero_words) c->dist_zero = false;
    return KTH_OK;
}

int kth_dist_window(kth_ctx *c, const uint32_t *d_sample, int64_t s_total) {
    if (!c || !d_sample || s_total < 1 || !c->uslots) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    if (c->dist_zero) {  // no kth_dist_sample since kth_dist_begin (samples from elsewhere)
        HIP_TRY(hipMemsetAsync(c->uslots, 0, 3 * (size_t)KTH_STATS_WORDS * 8, c->stream));
        c->dist_zero = false;
    }
    u64 r_lo, r_hi;
    window_ranks(c->dist_n, c->dist_k, s_total, &r_lo, &r_hi);
    if (c->coop && s_total % 64 == 0 && s_total < (1ll << 29)) {
        // one cooperative launch over the gathered sample (k_head without its
        // gather): the digits behind grid barriers, the early window; the state
        // is left resolved in st[0] for kth_dist_scan (ADV_CARRY).  Its slots
        // are cleared by kth_dist_result's k_result.
        Chain ch{c, c->islots, 2};
        StepArgs a = head_step(ch, c->dist_n, c->dist_k, s_total, r_lo, r_hi, false);
        kth::CoopArgs x = coop_args(c, HSLOT_OFF, nullptr, nullptr);
        x.sample_ready = 1;
        const int grid = (int)std::min<int64_t>(HEAD_GRID_MAX, std::max<int64_t>(1, s_total / HEAD_PER_WG));
        kth::k_head<false><<<grid, kth::DENSE_BLK, 0, c->stream>>>(a, x, nullptr, 0, 0,
                                                                  const_cast<uint32_t *>(d_sample), (u64)s_total);
        c->dist_coop_window = true;
        return launch_check();
    }
    c->dist_coop_window = false;
    // the three digits of the sample ranks, a launch each (steps 0 to 2;
    // kth_dist_scan's pass is step 3)
    Chain ch{c, c->islots};
    StepArgs a = ch.next(kth::ADV_INIT_SAMPLE, Chain::ACC | Chain::ZERO);
    init_rank(a, c->dist_n, c->dist_k, s_total, r_lo, r_hi);
    over_sample(a, d_sample, s_total);
    launch_level(c, a, true, level_grid((u64)s_total, DENSE_PER_WG));
    const int gs = level_grid((u64)s_total, sparse_wg(c));
    for (int digit = 2; digit <= 3; ++digit) {
        a = ch.next(kth::ADV_PICK);
        over_sample(a, d_sample, s_total);
        launch_level(c, a, false, gs);
    }
    return launch_check();
}

int kth_dist_scan(kth_ctx *c, const int32_t *d_keys, int64_t n_local) {
    if (!c || !d_keys || n_local < 0 || !c->uslots) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    KTH_TRY(reserve_cand(c, std::max<int64_t>(n_local, 1)));
    u64 *U0 = c->uslots;
    // step 3 of the window's chain over the ctx's slots (k_head resolved its
    // digits itself; the per-level window left the last one in islot(0)); the
    // counts go straight into the all-reduced slot 0 instead of islot(1)
    Chain ch{c, c->islots, 3};
    StepArgs a = c->dist_coop_window ? ch.next(kth::ADV_CARRY, Chain::NONE) : ch.next(kth::ADV_PICK, Chain::IN);
    a.stats_acc = U0;
    over_keys(a, d_keys, n_local);
    ev_main(c);
    launch_main<false>(c, a, 0, nullptr);
    ev_main(c);
    KTH_TRY(launch_check());
    // this rank's candidates' first digit into the same slot (one all-reduce
    // carries the counts and the digit)
    a = step(c, kth::ADV_CARRY, 1, 1, nullptr, U0, nullptr);
    a.min_per_wg = c->dscan_per_wg;
    kth::k_dscan_hist<kth::DENSE_BLK><<<level_grid(cand_capacity(std::max<int64_t>(n_local, 1)), c->dscan_per_wg),
                                        kth::DENSE_BLK, 0, c->stream>>>(a);
    KTH_TRY(launch_check());
    c->dist_level_next = 0;
    c->dist_levels = -1;
    return 0;
}

// Level l is step l of a chain over the bound slots (it accumulates into slot
// l+1 mod 3, which the caller all-reduces); level 0 also tells the host
// (DistStatus) how many level calls return a slot, so that level 1 can answer
// KTH_DIST_DONE without a collective.  Level 0 is enqueued without waiting
// for anything; level 1 waits for level 0 (the host reads the DistStatus) --
// while the all-reduce after level 0 is still queued on the device.
int kth_dist_level(kth_ctx *c, const int32_t *d_keys, int64_t n_local, int level) {
    if (!c || !d_keys || n_local < 0 || !c->uslots || level < 0 || level != c->dist_level_next) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    if (level >= 1 && c->dist_levels < 0) {
        HIP_TRY(hipEventSynchronize(c->ev_dist));
        const uint32_t *h = c->h_dist;
        const uint32_t levels = __atomic_load_n(&h[0], __ATOMIC_ACQUIRE), tag = __atomic_load_n(&h[3], __ATOMIC_ACQUIRE);
        if (tag != c->dist_tag || levels < 1 || levels > KTH_DIST_MAX_LEVELS) {
            c->dirty = true;
            return KTH_EINTERNAL;
        }
        c->dist_levels = (int)levels;
    }
    if (level >= 1 && level >= c->dist_levels) {
        c->dist_result_slot = level % 3;  // accumulated by level - 1
        c->dist_level_next = -1;
        return KTH_DIST_DONE;
    }
    StepArgs a = Chain{c, c->uslots, level}.next(level == 0 ? kth::ADV_DECIDE : kth::ADV_PICK);
    over_keys(a, d_keys, n_local);
    a.min_per_wg = sparse_wg(c);     // a digit under a resolved prefix: only that bin's keys
    a.dense_per_wg = DENSE_PER_WG;   // the fallback's first digit over the whole shard
    if (level == 0) {
        a.host_status = c->d_dist;
        a.tag = ++c->dist_tag;
    }
    // (the active workgroups follow the domain's size: candidates or the shard)
    kth::k_dlevel<kth::BLK><<<LEVEL_GRID_MAX, kth::BLK, 0, c->stream>>>(a);
    KTH_TRY(launch_check());
    if (level == 0) HIP_TRY(hipEventRecord(c->ev_dist, c->stream));
    c->dist_level_next = level + 1;
    return (level + 1) % 3;  // the slot it accumulated into
}

int kth_internal_slots_sum(uint64_t *const *slots, int P, int slot, void *stream) {
    static_assert(kth::SLOTS_SUM_MAX == KTH_LOCAL_MAX_SHARDS, "one limit");
    if (!slots || P < 1 || P > KTH_LOCAL_MAX_SHARDS || slot < 0 || slot > 2) return KTH_EINVAL;
    kth::SlotPtrs s{};
    for (int i = 0; i < P; ++i) {
        if (!slots[i]) return KTH_EINVAL;
        s.p[i] = reinterpret_cast<u64 *>(slots[i]) + (size_t)slot * KTH_STATS_WORDS;
    }
    constexpr int g = (KTH_STATS_WORDS + kth::BLK - 1) / kth::BLK;
    kth::k_slots_sum<<<g, kth::BLK, 0, reinterpret_cast<hipStream_t>(stream)>>>(s, P, (u64)KTH_STATS_WORDS);
    return launch_check();
}

void *kth_internal_ctx_stream(const kth_ctx *c) { return c ? reinterpret_cast<void *>(c->stream) : nullptr; }

int kth_internal_status_gather(kth_ctx *const *ctxs, int P, int32_t *d_dst, void *stream) {
    if (!ctxs || !d_dst || P < 1 || P > KTH_LOCAL_MAX_SHARDS) return KTH_EINVAL;
    kth::StatusPtrs p{};
    for (int i = 0; i < P; ++i) {
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) return KTH_EINVAL;
        p.p[i] = ctxs[i]->d_status;
    }
    KTH_TRY(set_device(ctxs[0]));
    kth::k_status_gather<<<1, kth::WAVE, 0, reinterpret_cast<hipStream_t>(stream)>>>(p, P, d_dst);
    return launch_check();
}

int kth_internal_dist_window_share(kth_ctx *src, kth_ctx *const *dst, int P) {
    if (!src || !dst || P < 0 || P > KTH_LOCAL_MAX_SHARDS) return KTH_EINVAL;
    if (!src->dist_coop_window) return 1;  // per-level window: its last pick is the scan's, nothing to copy
    kth::StatePtrs d{};
    for (int i = 0; i < P; ++i) {
        if (!dst[i] || dst[i]->device != src->device || !dst[i]->uslots) return KTH_EINVAL;
        d.p[i] = dst[i]->st;  // (the window's state is st[0], kth_dist_scan carries it)
    }
    if (P == 0) return KTH_OK;
    KTH_TRY(set_device(src));
    kth::k_state_bcast<<<1, kth::BLK, 0, src->stream>>>(src->st, d, P);
    KTH_TRY(launch_check());
    for (int i = 0; i < P; ++i) {
        dst[i]->dist_coop_window = true;
        dst[i]->dist_zero = false;
    }
    return KTH_OK;
}

// k_dresult after L levels: step L of their chain (state (L + 1) % 2 and slot L % 3 in, the other state out)
static int launch_dresult(kth_ctx *c, int L, int32_t *d_out, uint32_t early) {
    StepArgs a = Chain{c, c->uslots, L}.next(kth::ADV_PICK, Chain::IN);
    // (the islots and, right after them, k_head's slots of a cooperative window)
    static_assert(ISLOT_WORDS % 2 == 0, "k_dresult zeroes 16-byte words from the islots on");
    // (the sharded protocol is int32 only)
    kth::k_dresult<kth::BLK><<<16, kth::BLK, 0, c->stream>>>(a, d_out, c->d_status, c->islots,
                                                            ISLOT_WORDS + HSLOT_WORDS, early, d_last(c),
                                                            last_word(LAST_SINGLE, false, L % 2));
    c->last_state = L % 2;
    return launch_check();
}

int kth_dist_result_early(kth_ctx *c, int32_t *d_out) {
    // right after level 0's slot was all-reduced, before kth_dist_level(1):
    // the result as if level 0 were the last (it is whenever the window is at
    // most 2^24 values wide or decided by its counts)
    if (!c || !d_out || !c->uslots || c->dist_level_next != 1 || c->dist_levels >= 0) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    KTH_TRY(launch_dresult(c, 1, d_out, 1u));
    c->dist_early_out = d_out;
    return KTH_OK;
}

int kth_dist_result(kth_ctx *c, int32_t *d_out) {
    if (!c || !d_out || !c->uslots || c->dist_result_slot < 0) return KTH_EINVAL;
    KTH_TRY(set_device(c));
    const int L = c->dist_levels;  // levels enqueued: the last wrote state (L - 1) % 2
    if (!(L == 1 && c->dist_early_out == d_out))  // else the early result did it
        KTH_TRY(launch_dresult(c, L, d_out, 0u));
    c->dist_early_out = nullptr;
    c->dist_level_next = -1;
    c->dist_result_slot = -1;
    c->dist_open = false;
    return KTH_OK;
}

}  // extern "C"
