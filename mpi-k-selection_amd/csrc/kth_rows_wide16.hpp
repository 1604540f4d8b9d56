// kth_rows_wide16.hpp -- per-row k-th selection and top-k for wide rows of
// 16-bit keys (up to 2^24 columns of int16, uint16, float16 or bfloat16;
// include/kth.h "wide rows, 16-bit keys"): kth_rows_wide.hpp's two forms, the
// split one (`slices` workgroups share a row, every hand-off a kernel
// boundary) and the fused one (one workgroup per row, one launch), on the keys
// as they are, 2 bytes each.
//
// Keys: a 16-byte load holds 8 keys as 4 packed pairs, k16_ord2<CV> turns a
// pair into two packed 16-bit ords (kth_k16.hpp; CV 0: uint16, 1: int16, 2:
// float16 / bfloat16 with nl2 / top2 as kernel arguments), `flip2` = 0xFFFF in
// both halves reverses them for the k largest.  Nothing is widened to 32 bits
// and a value leaves through k16_bits_of_ord.
//
// Digits: two, 11 + 5 bits of the ord.  The first keeps the 2048-bin LDS
// histogram, the row histogram in scratch and block_pick_vals<BLOCK, NBINS /
// BLOCK> of the 32-bit kernels; the second has 32 bins (the first 32 words of
// the same histograms).  So the select reads a row twice at 2 bytes a key (the
// 32-bit one: three times at 4 bytes) and the top-k three times.
//
// Early end: the first counting pass also takes the packed min and max of the
// ords.  When they are equal the row holds one value and the second digit is
// skipped (its launches return at once in the split form).  The second digit
// is the last, so its pass takes no min / max.
//
// Counts: a row can hold 2^24 equal keys, so every count, offset, quota and
// column is 32 bits wide; nothing packs a column beside an ord.
//
// Scratch: kth_rows_wide.hpp's (row histogram, WideState, per-slice counts),
// under its rule -- every launch sequence leaves the histogram zero and nmn /
// mx of the state zero -- so 32-bit and 16-bit calls alternate on one ctx.
//
// Loads: VEC = a 16-byte aligned base and ld % 8 == 0; slice_keys is a
// multiple of 8, so every row and slice starts on a 16-byte boundary.  The last
// partial vector of a row is read by guarded 2-byte loads, as is everything
// when VEC is false; nothing at or past `cols` of a row is loaded.
//
// Ragged rows: kth_rows_wide.hpp's WideVar and its rules for a slice past its
// row's end and a row with nothing to select; the kernels are the text of
// kth_rows_wide16_kernels.hpp compiled twice, uniform and `_var`.
// Included by kth_kernels.hip after kth_rows_wide.hpp.
#pragma once

namespace kth {

constexpr uint32_t W16_D1_BITS = 5, W16_D1_BINS = 1u << W16_D1_BITS;  // the second digit
static_assert(DIGIT + W16_D1_BITS == 16, "two digits cover a 16-bit ord");

// The packed pairs of columns e .. e+7 of a row (e % 8 == 0); columns at or
// past `end` read as 0 and are never loaded.
template <bool VEC>
__device__ __forceinline__ uint4 w16_load8(const uint16_t *__restrict__ row, uint32_t e, uint32_t end) {
    if (VEC && e + 8u <= end) return *reinterpret_cast<const uint4 *>(row + e);
    uint32_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = e + (uint32_t)j < end ? (uint32_t)row[e + (uint32_t)j] : 0u;
    return make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
}

__device__ __forceinline__ uint32_t w16_pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t,
                              __builtin_elementwise_max(__builtin_bit_cast(k16_u2, a), __builtin_bit_cast(k16_u2, b)));
}

// Digit PASS of the keys of columns [begin, end) (begin % 8 == 0), counted into
// the workgroup's LDS histogram `hist`.  PASS 0: every key, bin = ord >> 5, and
// smm[0 .. 1] take max(ord ^ 0xFFFF), max(ord); PASS 1: the keys whose first
// digit is `prefix`, bin = the low 5 bits.  The caller zeroes hist and smm
// before and synchronises after.
template <int CV, bool VEC, int BLOCK, int PASS>
__device__ __forceinline__ void w16_count_range(const uint16_t *__restrict__ row, uint32_t begin, uint32_t end,
                                                uint32_t flip2, uint32_t nl2, uint32_t top2, uint32_t prefix,
                                                uint32_t *hist, uint32_t *smm) {
    uint32_t nmn2 = 0, mx2 = 0;  // packed, from the whole vectors
    uint32_t nmn = 0, mx = 0;    // from a row's or slice's last partial vector
    for (uint32_t base = begin + threadIdx.x * 8u; base < end; base += (uint32_t)(BLOCK * 8 * WD_U)) {
        uint4 x[WD_U];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) x[u] = w16_load8<VEC>(row, base + (uint32_t)(u * BLOCK * 8), end);
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const uint32_t e = base + (uint32_t)(u * BLOCK * 8);
            const uint4 o = k16_ord8<CV>(x[u], nl2, top2);
            const uint32_t w[4] = {o.x ^ flip2, o.y ^ flip2, o.z ^ flip2, o.w ^ flip2};
            if (e + 8u <= end) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t lo = w[q] & 0xFFFFu, hi = w[q] >> 16;
                    if (PASS == 0) {
                        wd_add(hist, lo >> W16_D1_BITS);
                        wd_add(hist, hi >> W16_D1_BITS);
                        mx2 = w16_pk_max(mx2, w[q]);
                        nmn2 = w16_pk_max(nmn2, ~w[q]);
                    } else {
                        if ((lo >> W16_D1_BITS) == prefix) wd_add(hist, lo & (W16_D1_BINS - 1u));
                        if ((hi >> W16_D1_BITS) == prefix) wd_add(hist, hi & (W16_D1_BINS - 1u));
                    }
                }
            } else if (e < end) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t kx = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                    if (e + (uint32_t)j < end) {
                        if (PASS == 0) {
                            wd_add(hist, kx >> W16_D1_BITS);
                            nmn = (kx ^ 0xFFFFu) > nmn ? (kx ^ 0xFFFFu) : nmn;
                            mx = kx > mx ? kx : mx;
                        } else if ((kx >> W16_D1_BITS) == prefix) {
                            wd_add(hist, kx & (W16_D1_BINS - 1u));
                        }
                    }
                }
            }
        }
    }
    if (PASS == 0) {
        const uint32_t a = nmn2 & 0xFFFFu, b = nmn2 >> 16, c = mx2 & 0xFFFFu, d = mx2 >> 16;
        nmn = a > nmn ? a : nmn;
        nmn = b > nmn ? b : nmn;
        mx = c > mx ? c : mx;
        mx = d > mx ? d : mx;
        nmn = wd_wave_max(nmn);
        mx = wd_wave_max(mx);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            (void)__hip_atomic_fetch_max(smm, nmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_max(smm + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

template <int BLOCK, int PASS>
__device__ __forceinline__ void w16_zero_lds(uint32_t *hist, uint32_t *smm) {
    for (int i = threadIdx.x; i < (PASS == 0 ? NBINS : (int)W16_D1_BINS); i += BLOCK) hist[i] = 0u;
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
}

// (better, equal) of the 8 keys of packed ords w[0 .. 3] at columns e .. e+7
__device__ __forceinline__ void w16_cmp8(const uint32_t (&w)[4], uint32_t e, uint32_t end, uint32_t answer, uint32_t &lt,
                                         uint32_t &eq) {
    const bool whole = e + 8u <= end;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t kx = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        const bool in = whole || e + (uint32_t)j < end;
        lt += (in && kx < answer) ? 1u : 0u;
        eq += (in && kx == answer) ? 1u : 0u;
    }
}

// Ordered compaction of columns [begin, end) (begin % 8 == 0): the keys below
// `answer`, and the first `quota` keys equal to it, go to outputs off, off + 1,
// ... in column order.  `want` = how many that is (the walk stops there); every
// store is bounded by k.  wsum: BLOCK / 64 words of LDS.
template <int CV, bool VEC, int BLOCK>
__device__ __forceinline__ void w16_write_range(const uint16_t *__restrict__ row, uint32_t begin, uint32_t end,
                                                uint32_t flip2, uint32_t nl2, uint32_t top2, int kind, uint32_t answer,
                                                uint32_t quota, uint32_t off, uint32_t want, uint32_t k,
                                                uint16_t *__restrict__ vals, int32_t *__restrict__ idx, u64 *wsum) {
    uint32_t lt_run = 0, eq_run = 0;  // workgroup-uniform: kept-so-far counts
    for (uint32_t cb = begin; cb < end; cb += (uint32_t)(BLOCK * 8)) {
        if (lt_run + (eq_run < quota ? eq_run : quota) >= want) break;
        const uint32_t e = cb + threadIdx.x * 8u;
        const uint4 o = k16_ord8<CV>(w16_load8<VEC>(row, e, end), nl2, top2);
        const uint32_t w[4] = {o.x ^ flip2, o.y ^ flip2, o.z ^ flip2, o.w ^ flip2};
        uint32_t cl = 0, ce = 0;
        w16_cmp8(w, e, end, answer, cl, ce);
        u64 total;
        const u64 pre = block_exclusive_scan<BLOCK>((u64)cl | (u64)ce << 32, wsum, &total);
        uint32_t lt_b = lt_run + (uint32_t)pre, eq_b = eq_run + (uint32_t)(pre >> 32);
        if (cl | ce) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t kx = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                const bool in = e + (uint32_t)j < end;
                const bool is_lt = in && kx < answer, is_eq = in && kx == answer;
                if (is_lt || (is_eq && eq_b < quota)) {
                    const uint32_t pos = off + lt_b + (eq_b < quota ? eq_b : quota);
                    if (pos < k) {
                        if (vals) vals[pos] = k16_bits_of_ord((kx ^ flip2) & 0xFFFFu, kind);
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
#include "kth_rows_wide16_kernels.hpp"
#undef WD_VAR
#define WD_VAR 1
#include "kth_rows_wide16_kernels.hpp"
#undef WD_VAR

}  // namespace kth
