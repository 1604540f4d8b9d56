// kth_rows_topp16.hpp -- top-p (nucleus) selection per row for wide rows of
// float16 / bfloat16 keys (include/kth.h "wide rows, top-p"): the key traits
// that put kth_rows_topp.hpp's passes, picks and kernels on 2-byte keys.
//
// Keys: a 16-byte load holds 8 keys; k16_ord8<2> turns them into packed 16-bit
// ords as in kth_rows_wide16.hpp, and fk = ord ^ 0xFFFF (the k largest
// convention).  Digits: two, 11 + 5 bits of fk, so a row is read three times
// at 2 bytes a key (pass M and two weighted digits).  A key is converted to
// float32 once, from its own bits, for its weight; the order never goes
// through a float.
//
// Loads: VEC = a 16-byte aligned base and ld % 8 == 0; slice_keys is a multiple
// of 8.  The last partial vector of a row, and everything when VEC is false,
// is read by guarded 2-byte loads (w16_load8).
// Included by kth_kernels.hip after kth_rows_topp.hpp.
#pragma once

namespace kth {

template <bool BF>
struct TpK16 {
    using elem = uint16_t;
    static constexpr int PASSES = 2, PER = 8;
    static constexpr int KIND = BF ? 3 : 2;  // KTH_K16_BF16 / KTH_K16_F16
    static constexpr uint32_t MASK = 0xFFFFu;
    static __device__ __forceinline__ uint32_t dbits(int pass) { return pass == 0 ? (uint32_t)DIGIT : W16_D1_BITS; }
    static __device__ __forceinline__ uint32_t shift(int pass) { return pass == 0 ? W16_D1_BITS : 0u; }
    static __device__ __forceinline__ float val(uint32_t bits) {
        if (BF) return __uint_as_float(bits << 16);
        return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
    }
    static __device__ __forceinline__ uint32_t bits_of(uint32_t fk) { return k16_bits_of_ord((fk ^ MASK) & MASK, KIND); }
    // +inf is the ord below the top one, which is every NaN
    static __device__ __forceinline__ bool special(uint32_t fk) { return (fk ^ MASK) + 1u >= k16_top(KIND); }
    template <bool VEC>
    static __device__ __forceinline__ uint4 load(const elem *__restrict__ row, uint32_t e, uint32_t end) {
        return w16_load8<VEC>(row, e, end);
    }
    // f(fk, value) for each of the loaded columns e .. e+7 below `end`
    template <class F>
    static __device__ __forceinline__ void each(const uint4 &x, uint32_t e, uint32_t end, F f) {
        const uint32_t nl2 = k16_nl(KIND) * 0x10001u, top2 = k16_top(KIND) * 0x10001u;
        const uint4 o = k16_ord8<2>(x, nl2, top2);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w}, ow[4] = {~o.x, ~o.y, ~o.z, ~o.w};
        const bool whole = e + 8u <= end;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (whole || e + (uint32_t)j < end)
                f((ow[j >> 1] >> (16 * (j & 1))) & MASK, val((w[j >> 1] >> (16 * (j & 1))) & MASK));
    }
};

}  // namespace kth
