// kth_k16.hpp -- the one-array select for 16-bit keys (int16, uint16, float16,
// bfloat16) on gfx950.  Included by kth_api.hip after kth_kernels.hip; it uses
// that file's load_nt / BLK and kth_device.hpp's block scan and pick, and
// touches none of the 32-bit kernels.
//
// A 16-bit key has 65536 values, so every count here is an exact histogram
// count: there is no candidate buffer and no radix level.  All kernels work in
// "ord" space, a uint16 that is monotone in the public order key
// (kth_k16_order_key): for the integer kinds it is the order key, for the
// float kinds it is the order key moved down by the NL patterns the negative
// NaNs would take, with every NaN clamped to TOP = ord(+inf) + 1.  That makes
// the transform of two packed keys an arithmetic shift, an or, a xor, a
// subtract and a min on packed 16-bit halves (four instructions on gfx950,
// the or and the xor fuse), with no compare and no select.
//
// Loads: k16_main reads the input with 16-byte nontemporal loads (the < 8-key
// unaligned head and tail as 2-byte loads); k16_hist reads its sample, at most
// 2 MB, with one 2-byte load a thread and chunk.
// Launches of one call (kernel boundaries only, one chain, no grid barrier):
//   n <= K16_SMALL_N (32768):  k16_hist over every key, k16_pick writes the
//       answers from the full histogram.
//   above:  k16_hist over ~kth_dist_sample_size(n) sampled keys, k16_pick
//       publishes per distinct rank a closed window [lo, hi] of ords around the
//       sample ranks p*s -+ (z*sqrt(s*p*(1-p)) + 2), then K16_PASSES = 3 times
//       k16_main + k16_finish.  A pass counts, per rank, the keys below lo by
//       ballots and the keys inside [lo, hi] in an LDS histogram; k16_finish
//       scans it and either writes the answer or narrows the window for the
//       next pass.  Passes after the one that settled every rank return at
//       once (every workgroup reads the states and leaves).
// Window histogram.  A window may be wider than the LDS holds (float keys
// around zero: 43 % of all bfloat16 patterns lie between -2^-16 and +2^-16;
// the median window |x| < 0.006 of 2^30 randn keys spans ~30600 bfloat16
// patterns and ~15400 float16 ones), so its bins are: the C values at each
// end exactly (one bin a value), and the middle in K16_COARSE = 256 cells of 2^shift values.  A rank that lands in a
// fine bin is done; one that lands in a cell makes that cell (at most 256
// values, so all fine) the next window; one outside the window (the sample
// misled, ~6e-7, or KTH_HOOK_K16_MISS) takes everything below lo or above hi
// as the next window.  So the worst case reads the input three times (miss,
// cell, exact) beside the sample; the common case once.  C = 8192 / 4096 /
// 2048 / 1024 for 1 / 2 / 3-4 / 5-8 distinct ranks (16384 fine bins a
// workgroup in all).
// The LDS bins are 16-bit fields, two a word, added to with ds_add without
// return (the wave does not wait).  A field must not reach 65536: every wave
// counts the keys it has added to a window since it last flushed it, and once
// that count reaches K16_WAVE_BUDGET (checked after each tile, which adds at
// most 4096 keys) the wave alone swaps the words it may have touched out
// (atomic exchange, so the other waves' adds are neither lost nor counted
// twice) and adds them to the rank's global u64 bins.  A field holds only adds
// made since its word was last swapped, and every wave's last own flush is no
// later than that: at most 4 * (K16_WAVE_BUDGET + 4096) = 64384 keys.
// Keys of one wave slot that share a bin are added once with their count (up
// to K16_LEADER_ROUNDS leader adds, then one add a lane), so an all-equal
// input costs one LDS add per 64 keys, and the leader adds keep the range of
// fields a flush has to swap small.
#pragma once

namespace kth {

constexpr int K16_SMALL_N = 32768;     // at most this many keys: the full-histogram path
constexpr int K16_HIST_BLK = 1024;     // k16_hist / k16_pick / k16_finish workgroup
constexpr int K16_CHUNK = 1024;        // consecutive keys per sampled chunk
constexpr int K16_HIST_PER_WG = 16384; // sampled keys a k16_hist workgroup (a 16-bit field holds them)
constexpr int K16_VALUES = 65536;
constexpr int K16_COARSE = 256;        // coarse cells of a window's middle
constexpr int K16_FIELDS = 16384;      // fine bins of all windows of a workgroup
constexpr int K16_BINS_MAX = K16_FIELDS + K16_COARSE;  // bins of one window at most
constexpr int K16_RANK_WORDS = K16_BINS_MAX + 8;       // a rank's global set: bins, then [cnt_lt]
constexpr int K16_LDS_WORDS = (K16_FIELDS + MULTI_MAX * K16_COARSE) / 2;
constexpr int K16_PASSES = 3;
constexpr int K16_UNROLL = 8;          // 16-byte loads in flight per thread in k16_main
constexpr uint32_t K16_WAVE_BUDGET = 12000u;  // keys a wave adds to a window's LDS bins between its flushes
constexpr int K16_LEADER_ROUNDS = 8;
constexpr uint32_t K16_ERR_PASSES = 128;  // a rank unresolved after K16_PASSES passes (cannot happen)

enum : uint32_t { K16_IDLE = 0, K16_ACTIVE = 1, K16_DONE = 2 };

// ---- key kinds (include/kth.h KTH_K16_*): bits <-> order key <-> ord
__host__ __device__ __forceinline__ uint32_t k16_inf(int kind) { return kind == 2 ? 0x7C00u : 0x7F80u; }
__host__ __device__ __forceinline__ bool k16_float(int kind) { return kind == 2 || kind == 3; }

__host__ __device__ __forceinline__ uint16_t k16_key_of_bits(uint16_t b, int kind) {
    switch (kind) {
    case 0: return (uint16_t)(b ^ 0x8000u);
    case 1: return b;
    case 2:
    case 3:
        if ((uint32_t)(b & 0x7FFFu) > k16_inf(kind)) return 0xFFFFu;
        return (b & 0x8000u) ? (uint16_t)~b : (uint16_t)(b | 0x8000u);
    default: return 0;
    }
}
__host__ __device__ __forceinline__ uint16_t k16_bits_of_key(uint16_t key, int kind) {
    switch (kind) {
    case 0: return (uint16_t)(key ^ 0x8000u);
    case 1: return key;
    case 2:
    case 3:
        if (key == 0xFFFFu) return (uint16_t)(k16_inf(kind) | (kind == 2 ? 0x0200u : 0x0040u));
        return (key & 0x8000u) ? (uint16_t)(key & 0x7FFFu) : (uint16_t)~key;
    default: return 0;
    }
}
// NL: the keys below key(-inf) (the negative NaNs' patterns); TOP: the largest ord (float: every NaN)
__host__ __device__ __forceinline__ uint32_t k16_nl(int kind) { return k16_float(kind) ? 0xFFFFu - (k16_inf(kind) | 0x8000u) : 0u; }
__host__ __device__ __forceinline__ uint32_t k16_top(int kind) {
    return k16_float(kind) ? (k16_inf(kind) | 0x8000u) - k16_nl(kind) + 1u : 0xFFFFu;
}
__host__ __device__ __forceinline__ uint32_t k16_key_of_ord(uint32_t ord, int kind) {
    if (!k16_float(kind)) return ord & 0xFFFFu;
    return ord >= k16_top(kind) ? 0xFFFFu : ord + k16_nl(kind);
}
__host__ __device__ __forceinline__ uint16_t k16_bits_of_ord(uint32_t ord, int kind) {
    return k16_bits_of_key((uint16_t)k16_key_of_ord(ord, kind), kind);
}

typedef uint16_t k16_u2 __attribute__((ext_vector_type(2)));
typedef int16_t k16_i2 __attribute__((ext_vector_type(2)));

// Two packed keys -> two packed ords.  CV 0: uint16, 1: int16, 2: float16 /
// bfloat16 (nl2 / top2: NL and TOP in both halves).  Integer operations only.
template <int CV>
__device__ __forceinline__ uint32_t k16_ord2(uint32_t w, uint32_t nl2, uint32_t top2) {
    if constexpr (CV == 0) {
        return w;
    } else if constexpr (CV == 1) {
        return w ^ 0x80008000u;
    } else {
        const k16_i2 sg = __builtin_bit_cast(k16_i2, w) >> 15;  // 0xFFFF in a negative half
        const uint32_t r = w ^ (__builtin_bit_cast(uint32_t, sg) | 0x80008000u);
        k16_u2 d = __builtin_bit_cast(k16_u2, r) - __builtin_bit_cast(k16_u2, nl2);  // the negative NaNs wrap to the top
        d = __builtin_elementwise_min(d, __builtin_bit_cast(k16_u2, top2));
        return __builtin_bit_cast(uint32_t, d);
    }
}
template <int CV>
__device__ __forceinline__ uint4 k16_ord8(const uint4 &q, uint32_t nl2, uint32_t top2) {
    return make_uint4(k16_ord2<CV>(q.x, nl2, top2), k16_ord2<CV>(q.y, nl2, top2), k16_ord2<CV>(q.z, nl2, top2),
                      k16_ord2<CV>(q.w, nl2, top2));
}
template <int CV>
__device__ __forceinline__ uint32_t k16_ord1(uint16_t b, uint32_t nl2, uint32_t top2) {
    return k16_ord2<CV>((uint32_t)b, nl2, top2) & 0xFFFFu;
}

struct alignas(16) K16State {
    u64 n, k;
    u64 cnt_lt, inside;   // the last pass's counts: keys below lo, keys in [lo, hi]
    uint32_t lo, hi;      // the window, in ords (lo > hi: empty)
    uint32_t mode, pass;  // K16_*; passes finished
    uint32_t answer;      // done: the answer's ord
    uint32_t error, path, C;
};

// A window's bins, in rank order: [0, C) the values lo .. lo + C - 1, then
// K16_COARSE cells of 2^shift values, then [C + K16_COARSE, nb) the values
// hi - C + 1 .. hi; a window of at most 2 C values has one bin a value.
struct K16Lay {
    uint32_t lo, hi, C, shift, narrow, nb;
};
__host__ __device__ __forceinline__ K16Lay k16_layout(uint32_t lo, uint32_t hi, uint32_t C) {
    K16Lay l;
    l.lo = lo;
    l.hi = hi;
    l.C = C;
    const uint32_t width = hi >= lo ? hi - lo + 1u : 0u;
    l.narrow = width <= 2u * C;
    l.shift = 0;
    l.nb = width;
    if (!l.narrow) {
        const uint32_t mid = width - 2u * C;
        while (((mid - 1u) >> l.shift) >= (uint32_t)K16_COARSE) ++l.shift;
        l.nb = 2u * C + (uint32_t)K16_COARSE;
    }
    return l;
}
// the bin of ord x in [lo, hi]
__device__ __forceinline__ uint32_t k16_bin(const K16Lay &l, uint32_t x) {
    const uint32_t d = x - l.lo, e = l.hi - x;
    const uint32_t far = e < l.C ? l.C + (uint32_t)K16_COARSE + (l.C - 1u - e) : l.C + ((d - l.C) >> l.shift);
    return (l.narrow || d < l.C) ? d : far;
}

// Where the answers go: rank set j's bits to d_out[i] for every i with
// set[i] == j, and [bits, error] to d_status + 2 j (either may be null).
struct K16Out {
    int m, kind;
    int set[MULTI_MAX];
    uint16_t *d_out;
    int32_t *d_status;
};
__device__ __forceinline__ void k16_publish(const K16Out &o, int j, const K16State &s) {
    const uint16_t bits = k16_bits_of_ord(s.answer, o.kind);
    if (o.d_out && !s.error)
        for (int i = 0; i < o.m; ++i)
            if (o.set[i] == j) o.d_out[i] = bits;
    if (o.d_status) {
        o.d_status[2 * j] = (int32_t)bits;
        o.d_status[2 * j + 1] = (int32_t)s.error;
    }
}

// ------------------------------------------------------------------ k16_hist
// Adds the ords of s keys to the global 65536-bin histogram: key i of the s is
// keys[(i / K16_CHUNK) * stride + i % K16_CHUNK].  A workgroup counts its
// K16_HIST_PER_WG keys in 16-bit LDS fields (128 KiB) and adds the nonzero
// ones to the global bins.
template <int CV>
__global__ __launch_bounds__(K16_HIST_BLK) void k16_hist(const uint16_t *keys, u64 n, u64 s, u64 stride, uint32_t nl2,
                                                         uint32_t top2, uint32_t *shist) {
    extern __shared__ uint32_t k16_hl[];
    const int lane = threadIdx.x & (WAVE - 1);
    for (int i = threadIdx.x; i < K16_VALUES / 2; i += K16_HIST_BLK) k16_hl[i] = 0u;
    __syncthreads();
    for (int q = 0; q < K16_HIST_PER_WG / K16_CHUNK; ++q) {
        const u64 c = (u64)blockIdx.x * (K16_HIST_PER_WG / K16_CHUNK) + q;
        const u64 idx = c * stride + threadIdx.x;
        const bool ok = c * K16_CHUNK + threadIdx.x < s && idx < n;
        const uint32_t x = ok ? k16_ord1<CV>(keys[idx], nl2, top2) : 0u;
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
        if (!okm) continue;  // wave-uniform
        const int first = __builtin_ctzll(okm);
        const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)x, first);
        const unsigned long long eq = __builtin_amdgcn_ballot_w64(x == x0) & okm;
        if (eq == okm) {  // the wave's keys are all equal: one add of their count
            if (lane == first) atomicAdd(&k16_hl[x0 >> 1], (uint32_t)__popcll(eq) << (16u * (x0 & 1u)));
        } else if (ok) {
            atomicAdd(&k16_hl[x >> 1], 1u << (16u * (x & 1u)));
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < K16_VALUES / 2; w += K16_HIST_BLK) {
        const uint32_t t = k16_hl[w];
        if (t & 0xFFFFu) atomicAdd(&shist[2 * w], t & 0xFFFFu);
        if (t >> 16) atomicAdd(&shist[2 * w + 1], t >> 16);
    }
}

// ------------------------------------------------------------------ k16_pick
// One workgroup over the global histogram (and clears it).  small: the answer
// of every rank, exactly.  Otherwise the window of every rank: lo / hi = the
// ords holding sample ranks rlo / rhi (0: no lower bound, > s: no upper one);
// miss (KTH_HOOK_K16_MISS): an empty window instead, below which every key lies.
struct K16PickArgs {
    uint32_t *shist;
    K16State *st;
    int D, small, miss;
    u64 n;
    uint32_t C, top;
    u64 k[MULTI_MAX], rlo[MULTI_MAX], rhi[MULTI_MAX];
    K16Out out;
    uint32_t *last;       // the ctx's last-call word (kth_ctx_last_stats) ...
    uint32_t last_word;   // ... and what this call leaves there
};
__global__ __launch_bounds__(K16_HIST_BLK) void k16_pick(K16PickArgs a) {
    constexpr int PER = K16_VALUES / K16_HIST_BLK;  // 64 bins a thread: a wave reads them with one load
    static_assert(PER == WAVE && 2 * MULTI_MAX <= K16_HIST_BLK / WAVE, "one wave a target");
    __shared__ u64 scratch[K16_HIST_BLK / WAVE];
    __shared__ uint32_t res_bin[2 * MULTI_MAX], res_cnt[2 * MULTI_MAX], owner[2 * MULTI_MAX];
    __shared__ u64 res_below[2 * MULTI_MAX], owner_pre[2 * MULTI_MAX];
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    uint4 *mine = reinterpret_cast<uint4 *>(a.shist + (size_t)threadIdx.x * PER);
    u64 sum = 0;
#pragma unroll
    for (int i = 0; i < PER / 4; ++i) {
        const uint4 q = mine[i];
        sum += (u64)q.x + q.y + q.z + q.w;
    }
    u64 total;
    const u64 pre = block_exclusive_scan<K16_HIST_BLK>(sum, scratch, &total);
    const int T = 2 * a.D;
    auto target = [&](int t) -> u64 {
        const int j = t >> 1;
        return (t & 1) ? (a.small ? 0 : a.rhi[j]) : (a.small ? a.k[j] : a.rlo[j]);
    };
    if ((int)threadIdx.x < T) {
        res_bin[threadIdx.x] = target(threadIdx.x) == 0 ? 0u : a.top;  // a rank above the total keeps top
        res_cnt[threadIdx.x] = 0u;
        res_below[threadIdx.x] = 0;
        owner[threadIdx.x] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {  // the thread whose 64 bins hold target t
        const u64 r = target(t);
        if (r > pre && r <= pre + sum) {
            owner[t] = threadIdx.x;
            owner_pre[t] = pre;
        }
    }
    __syncthreads();
    if (wid < T && owner[wid] != 0xFFFFFFFFu) {  // wave t scans those bins, one a lane
        const u64 r = target(wid);
        const uint32_t hb = a.shist[(size_t)owner[wid] * PER + lane];
        const u64 inc = owner_pre[wid] + wave_incl_scan32(hb);
        if (inc >= r && inc - hb < r) {  // one lane
            res_bin[wid] = owner[wid] * PER + lane;
            res_cnt[wid] = hb;
            res_below[wid] = inc - hb;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER / 4; ++i) mine[i] = make_uint4(0, 0, 0, 0);
    if ((int)threadIdx.x < a.D) {
        const int j = threadIdx.x;
        K16State s;
        s.n = a.n;
        s.k = a.k[j];
        s.lo = res_bin[2 * j];
        s.hi = a.small ? s.lo : res_bin[2 * j + 1];
        s.cnt_lt = a.small ? res_below[2 * j] : 0;
        s.inside = a.small ? res_cnt[2 * j] : 0;
        s.mode = a.small ? K16_DONE : K16_ACTIVE;
        s.pass = 0;
        s.answer = s.lo;
        s.error = 0;
        s.path = 5;  // KTH_PATH_K16
        s.C = a.C;
        if (!a.small && a.miss) {
            s.lo = (uint32_t)K16_VALUES;
            s.hi = (uint32_t)K16_VALUES - 1u;
        }
        a.st[j] = s;
        if (a.small) k16_publish(a.out, j, s);
    }
    if (threadIdx.x == 0 && a.last) *a.last = a.last_word;
}

// ------------------------------------------------------------------ k16_main
struct K16Args {
    const uint16_t *keys;
    u64 n;
    int D;
    uint32_t nl2, top2;
    const K16State *st;
    u64 *bins;  // rank j's set at bins + j * K16_RANK_WORDS (zero on entry)
};
struct K16Win {
    K16Lay lay;
    uint32_t active, base;  // base: the window's first LDS word
};

__device__ __forceinline__ void k16_flush_word(u64 *gb, uint32_t f0, uint32_t t) {
    if (t & 0xFFFFu) atomicAdd(&gb[f0], (u64)(t & 0xFFFFu));
    if (t >> 16) atomicAdd(&gb[f0 + 1], (u64)(t >> 16));
}
// c keys into field f of an LDS histogram h (no return: the wave goes on)
__device__ __forceinline__ void k16_add_field(uint32_t *h, uint32_t f, uint32_t c) {
    (void)__hip_atomic_fetch_add(h + (f >> 1), c << (16u * (f & 1u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// k16_main_tf (kth_topk_k16's pass 0, D == 1) also records, for the top-k's
// count pass, which of its rows can hold output.  A row is one of a wave's U
// loads of a full tile, 8 * WAVE = 512 consecutive keys; wave w of the
// workgroup that streams tile t stores ONE byte, flags[t * NW + w] (one lane, a
// plain vector byte store), whose bit u says that some key of its load u lies
// at or below the window's upper edge hi (the ballot counts LT + N moved;
// largest: at or above lo, LT moved by less than the row's 512 keys).  Both
// counts are wave-uniform scalars already.  Workgroup 0 leaves the window the
// pass used and whether it ran in hdr[0..3) = [lo, hi, ran]: k16_finish narrows
// the state's window afterwards.  Every byte of a full tile is written by the
// pass that the count pass later trusts, so nothing is cleared between calls.
struct K16Flags {
    uint32_t *hdr;     // [lo, hi, ran, -], then the flag bytes
    uint32_t largest;  // the top-k's direction
};

#define K16_MAIN_TF 0
#include "kth_k16_main_body.hpp"
#undef K16_MAIN_TF
#define K16_MAIN_TF 1
#include "kth_k16_main_body.hpp"
#undef K16_MAIN_TF

// ---------------------------------------------------------------- k16_finish
// One workgroup per distinct rank, after a pass: scans the rank's bins (and
// clears them for the next pass or call); the rank's key lies in a fine bin ->
// the answer; in a coarse cell, below the window or above it -> the next
// pass's window.
struct K16FinArgs {
    K16State *st;
    u64 *bins;
    uint32_t top;
    K16Out out;
};
__global__ __launch_bounds__(K16_HIST_BLK) void k16_finish(K16FinArgs a) {
    __shared__ u64 scratch[K16_HIST_BLK / WAVE + 3];
    const int j = blockIdx.x;
    K16State s = a.st[j];
    if (s.mode != K16_ACTIVE) return;  // block-uniform
    u64 *gb = a.bins + (size_t)j * K16_RANK_WORDS;
    const K16Lay l = k16_layout(s.lo, s.hi, s.C);
    const int nb = (int)l.nb;
    const u64 cnt_lt = gb[K16_BINS_MAX];
    u64 mine = 0;
    for (int b = threadIdx.x; b < nb; b += K16_HIST_BLK) mine += gb[b];
    u64 inside;
    (void)block_exclusive_scan<K16_HIST_BLK>(mine, scratch, &inside);
    uint32_t bin = 0;
    u64 below = 0;
    bool ok = false;
    // (block_pick's "nb <= 2048" is its other callers' histogram size, not a
    // limit of its code: a thread takes ceil(nb / BLOCK) consecutive bins, here
    // up to 17 u64 bins read one after the other, once for its sum and once by
    // the one thread that holds the rank; ~16640 L2 reads a rank and pass)
    if (s.k > cnt_lt && s.k <= cnt_lt + inside)  // block-uniform
        ok = block_pick<K16_HIST_BLK>([&](int b) { return gb[b]; }, nb, s.k - cnt_lt, &bin, &below, scratch);
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += K16_HIST_BLK) gb[b] = 0;
    if (threadIdx.x != 0) return;
    gb[K16_BINS_MAX] = 0;
    s.cnt_lt = cnt_lt;
    s.inside = inside;
    const bool coarse = ok && !l.narrow && bin >= l.C && bin < l.C + (uint32_t)K16_COARSE;
    if (ok && !coarse) {
        s.answer = (l.narrow || bin < l.C) ? l.lo + bin : l.hi - (l.C - 1u - (bin - l.C - (uint32_t)K16_COARSE));
        s.mode = K16_DONE;
        s.path = s.pass == 0 ? 5 : 6;  // KTH_PATH_K16 / KTH_PATH_K16_FALLBACK
        k16_publish(a.out, j, s);
    } else {
        bool bad = false;
        if (coarse) {  // the cell becomes the window
            const uint32_t c0 = l.lo + l.C + ((bin - l.C) << l.shift), last = l.hi - l.C;
            s.lo = c0;
            s.hi = c0 + (1u << l.shift) - 1u < last ? c0 + (1u << l.shift) - 1u : last;
        } else if (s.k <= cnt_lt) {  // everything below the window
            bad = s.lo == 0u;
            s.hi = s.lo - 1u;
            s.lo = 0u;
        } else {  // everything above it
            bad = s.hi >= a.top;
            s.lo = s.hi + 1u;
            s.hi = a.top;
        }
        if (++s.pass >= (uint32_t)K16_PASSES || bad) {
            s.error = K16_ERR_PASSES;
            s.mode = K16_DONE;
            k16_publish(a.out, j, s);
        }
    }
    a.st[j] = s;
}

}  // namespace kth
