// kth_rows_wide.hpp -- per-row k-th selection and top-k for wide rows (up to
// 2^24 columns of int32 or float32 keys; include/kth.h "wide rows"): the shape
// between the one-array calls and the register / LDS rows kernels, a batch of
// 1 to a few thousand rows of 32 Ki to 1 Mi columns (the logits matrix).
//
// An exact radix select on the 32-bit order key, three digits at most
// (11 + 11 + 10 bits, <= 2048 bins), in two forms (kth_wide_rows_plan):
//
//   split (slices > 1): too few rows to fill the GPU, so `slices` workgroups
//     share a row (grid slices x group_rows).  Per digit, k_wide_count has each
//     workgroup histogram its slice in LDS and add its non-empty bins to the
//     row's 8 KiB histogram in scratch; k_wide_pick (one workgroup a row) picks
//     the digit after the kernel boundary, advances the row's state and clears
//     the histogram.  Every hand-off between workgroups is a kernel boundary: no
//     cooperative launch, no grid barrier, no in-launch flag.
//   fused (slices == 1): rows alone fill the GPU.  One workgroup per row runs
//     every digit in one launch, histogram and pick in LDS behind workgroup
//     barriers, no global atomics; the later digits re-read the row (from L2).
//
// Early end: every counting pass also takes the min and max of the keys that
// match the prefix.  When they are equal the picked bin holds one value (one
// key, or many equal ones) and that value is the answer: the remaining digits
// are skipped (their launches return at once in the split form).
//
// The first digit of a float row is sign + exponent + two mantissa bits: a
// randn row puts most keys into about ten bins, and a wave's LDS adds to one
// address serialise.  The remedy of k_rows_reg and the 16-bit rows, several
// histogram copies with the lane picking one, was measured here and lost
// (DESIGN.md "Wide rows"): a workgroup keeps one LDS histogram.
//
// Top-k: the select leaves the k-th key and the tie quota (k minus the keys
// strictly better).  Split: k_wide_tk_count writes (better, equal) per slice,
// k_wide_tk_write derives each workgroup's output offset and its share of the
// quota from the slices before it (<= 256 numbers) and compacts its slice in
// column order.  Fused: the one workgroup walks the row with a running offset.
// `flip` = 0xFFFFFFFF reverses the order key for the k largest.
//
// Loads: VEC = a 16-byte aligned base and ld % 4 == 0, so every row and every
// slice starts on a 16-byte boundary and is read with 16-byte loads, the last
// partial vector of a row by guarded 4-byte loads; otherwise guarded 4-byte
// loads throughout.  A word becomes an order key right after its load
// (WideKey: the one place that knows the key type).  The 16-bit wide rows are
// kernels of their own (kth_rows_wide16.hpp: two digits of packed 16-bit ords,
// 8 keys a load); they share the constants, WideState and the wave helpers of
// this file, and its scratch under the same rule.
// Included by kth_kernels.hip after kth_rows16.hpp.
#pragma once

namespace kth {

constexpr int WD_BLOCK = 256;    // split-form kernels
constexpr int WD_FBLOCK = 512;   // fused kernel: one workgroup per row
constexpr int WD_U = 4;          // 16-byte loads in flight per thread in the counting passes
constexpr int WD_MAX_SLICES = 256;
static_assert(WD_MAX_SLICES <= WD_BLOCK, "k_wide_tk_write reads one slice's counts per thread");

// The order key of a word and back (uint32, unsigned order = key order).
template <bool F32>
struct WideKey {
    static __device__ __forceinline__ uint32_t key(uint32_t bits) { return F32 ? key_of_f32(bits) : key_of_i32(bits); }
    static __device__ __forceinline__ uint32_t bits(uint32_t key) { return (uint32_t)out_word<F32>(key); }
};

// A row's selection state (split form; scratch).  nmn / mx accumulate max(~key)
// and max(key) of the keys matching the prefix: zero is the identity of both,
// and every pick leaves them zero.
struct WideState {
    uint32_t kk;      // remaining 1-based rank among the keys matching `prefix`; at the end the tie quota
    uint32_t prefix;  // the digits picked so far, right-aligned
    uint32_t done;
    uint32_t answer;  // the k-th key (flipped order key)
    uint32_t eqn;     // keys in the picked bin; at the end the keys equal to the answer
    uint32_t nmn, mx;
    uint32_t pad;
};
constexpr int WD_STATE_WORDS = sizeof(WideState) / 4;

// Ragged rows (include/kth.h "wide rows, ragged"): the device arrays of a var
// call, advanced to the group's first row; each may be null.  The kernels are
// in kth_rows_wide_kernels.hpp, whose text is compiled twice: WD_VAR 0 gives
// the uniform kernels (every row has `cols` keys and rank k: the tokens, and
// so the device code, they had before the var calls) and WD_VAR 1 their
// `_var` twins, which take a WideVar and read row r's length and rank from it,
// a workgroup-uniform read.
//
// New states of a var row, and how each kernel meets them:
//   a slice that begins at or past its row's end has no keys: the counting
//     kernels return before they touch LDS, the row histogram or nmn / mx;
//     k_wide_tk_count still writes its (0, 0), because k_wide_tk_write sums
//     the counts of the slices before it and the counts of an earlier, longer
//     call are still in scratch;
//   a row with nothing to select (length 0, or rank 0 in the top-k): the pick
//     of the first digit settles it -- done, quota 0, answer 0 -- having
//     cleared the histogram as always.  No order key is below 0 and the quota
//     of the keys equal to it is 0, so no later kernel keeps a key of the row.
struct WideVar {
    const int32_t *lens;  // clamped to [0, cols]; null: cols
    const int32_t *ks;    // null: the host's k
    int32_t *cnt;         // top-k: the entries written of each row; may be null
};

__device__ __forceinline__ uint32_t wd_row_len(const WideVar &v, u64 r, uint32_t cols) {
    if (!v.lens) return cols;
    const int32_t n = v.lens[r];
    return n < 0 ? 0u : (uint32_t)n < cols ? (uint32_t)n : cols;
}
// top-k: min(clamp(ks[r], 0, k), len); select: clamp(ks[r], 1, len), 0 for an empty row
__device__ __forceinline__ uint32_t wd_row_rank(const WideVar &v, u64 r, uint32_t k, uint32_t len, bool topk) {
    const int32_t q = v.ks ? v.ks[r] : (int32_t)k;
    uint32_t kr = q < 0 ? 0u : (uint32_t)q;
    if (topk) kr = kr < k ? kr : k;
    else kr = kr < 1u ? 1u : kr;
    return kr < len ? kr : len;
}
// The padding of a top-k row: entries [kr, k) of its k output slots, idx -1 and
// the zero word; cnt = kr.  WORD: the value type (uint32_t / uint16_t).
template <int BLOCK, class WORD>
__device__ __forceinline__ void wd_pad_row(const WideVar &v, u64 r, uint32_t kr, uint32_t k, WORD *__restrict__ vals,
                                           int32_t *__restrict__ idx) {
    for (uint32_t pos = kr + threadIdx.x; pos < k; pos += (uint32_t)BLOCK) {
        if (vals) vals[pos] = (WORD)0;
        if (idx) idx[pos] = -1;
    }
    if (threadIdx.x == 0 && v.cnt) v.cnt[r] = (int32_t)kr;
}

// digit `pass` of a key: bits [shift, shift + 11) (the last digit: the low 10)
__device__ __forceinline__ uint32_t wd_shift(int pass) { return pass == 0 ? 21u : pass == 1 ? 10u : 0u; }
__device__ __forceinline__ uint32_t wd_bins(int pass) { return pass == 2 ? 1024u : (uint32_t)NBINS; }

// The words of columns e .. e+3 of a row; columns at or past `end` read as 0
// and are never loaded.
template <bool VEC>
__device__ __forceinline__ uint4 wd_load4(const uint32_t *__restrict__ row, uint32_t e, uint32_t end) {
    if (VEC && e + 4u <= end) return *reinterpret_cast<const uint4 *>(row + e);
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (e < end) x.x = row[e];
    if (e + 1u < end) x.y = row[e + 1u];
    if (e + 2u < end) x.z = row[e + 2u];
    if (e + 3u < end) x.w = row[e + 3u];
    return x;
}

__device__ __forceinline__ void wd_add(uint32_t *h, uint32_t bin) {
    (void)__hip_atomic_fetch_add(h + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t wd_wave_max(uint32_t x) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, o, WAVE);
        x = y > x ? y : x;
    }
    return x;
}
__device__ __forceinline__ uint32_t wd_wave_sum(uint32_t x) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, WAVE);
    return x;
}

// Digit `pass` of the keys of columns [begin, end) that match `prefix`, counted
// into the workgroup's LDS histogram `hist`; smm[0 .. 1] take max(~key), max(key)
// of those keys.  The caller zeroes hist and smm before and synchronises after.
template <bool F32, bool VEC, int BLOCK>
__device__ __forceinline__ void wd_count_range(const uint32_t *__restrict__ row, uint32_t begin, uint32_t end,
                                               uint32_t flip, int pass, uint32_t prefix, uint32_t *hist,
                                               uint32_t *smm) {
    const uint32_t mshift = pass == 1 ? 21u : 10u, dshift = wd_shift(pass), dmask = wd_bins(pass) - 1u;
    uint32_t nmn = 0, mx = 0;
    for (uint32_t base = begin + threadIdx.x * 4u; base < end; base += (uint32_t)(BLOCK * 4 * WD_U)) {
        uint4 x[WD_U];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) x[u] = wd_load4<VEC>(row, base + (uint32_t)(u * BLOCK * 4), end);
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const uint32_t e = base + (uint32_t)(u * BLOCK * 4);
            const uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t kx = WideKey<F32>::key(w[j]) ^ flip;
                if (e + (uint32_t)j < end && (pass == 0 || (kx >> mshift) == prefix)) {
                    wd_add(hist, (kx >> dshift) & dmask);
                    nmn = ~kx > nmn ? ~kx : nmn;
                    mx = kx > mx ? kx : mx;
                }
            }
        }
    }
    nmn = wd_wave_max(nmn);
    mx = wd_wave_max(mx);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        (void)__hip_atomic_fetch_max(smm, nmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_max(smm + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

template <int BLOCK>
__device__ __forceinline__ void wd_zero_lds(uint32_t *hist, uint32_t *smm) {
    for (int i = threadIdx.x; i < NBINS; i += BLOCK) hist[i] = 0u;
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
}

// Ordered compaction of columns [begin, end): the keys below `answer`, and the
// first `quota` keys equal to it, go to outputs off, off + 1, ... in column
// order.  `want` = how many that is (the walk stops there); every store is
// bounded by k.  wsum: BLOCK / 64 words of LDS.
template <bool F32, bool VEC, int BLOCK>
__device__ __forceinline__ void wd_write_range(const uint32_t *__restrict__ row, uint32_t begin, uint32_t end,
                                               uint32_t flip, uint32_t answer, uint32_t quota, uint32_t off,
                                               uint32_t want, uint32_t k, uint32_t *__restrict__ vals,
                                               int32_t *__restrict__ idx, u64 *wsum) {
    uint32_t lt_run = 0, eq_run = 0;  // workgroup-uniform: kept-so-far counts
    for (uint32_t cb = begin; cb < end; cb += (uint32_t)(BLOCK * 4)) {
        if (lt_run + (eq_run < quota ? eq_run : quota) >= want) break;
        const uint32_t e = cb + threadIdx.x * 4u;
        const uint4 x = wd_load4<VEC>(row, e, end);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
        uint32_t kx[4], cl = 0, ce = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kx[j] = WideKey<F32>::key(w[j]) ^ flip;
            const bool in = e + (uint32_t)j < end;
            cl += (in && kx[j] < answer) ? 1u : 0u;
            ce += (in && kx[j] == answer) ? 1u : 0u;
        }
        u64 total;
        const u64 pre = block_exclusive_scan<BLOCK>((u64)cl | (u64)ce << 32, wsum, &total);
        uint32_t lt_b = lt_run + (uint32_t)pre, eq_b = eq_run + (uint32_t)(pre >> 32);
        if (cl | ce) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = e + (uint32_t)j < end;
                const bool is_lt = in && kx[j] < answer, is_eq = in && kx[j] == answer;
                if (is_lt || (is_eq && eq_b < quota)) {
                    const uint32_t pos = off + lt_b + (eq_b < quota ? eq_b : quota);
                    if (pos < k) {
                        if (vals) vals[pos] = WideKey<F32>::bits(kx[j] ^ flip);
                        if (idx) idx[pos] = (int32_t)(e + (uint32_t)j);
                    }
                }
                lt_b += is_lt ? 1u : 0u;
                eq_b += is_eq ? 1u : 0u;
            }
        }
        lt_run += (uint32_t)total;
        eq_run += (uint32_t)(total >> 32);
    }
}

// ---- the kernels, uniform and var (no include guard: see above)
#define WD_VAR 0
#include "kth_rows_wide_kernels.hpp"
#undef WD_VAR
#define WD_VAR 1
#include "kth_rows_wide_kernels.hpp"
#undef WD_VAR

}  // namespace kth
