// kth_rows16.hpp -- batched per-row k-th selection and top-k for 16-bit keys
// (int16, uint16, float16, bfloat16; include/kth.h "16-bit rows"), one
// wavefront per row, the row in the wave's registers as packed pairs.
//
// A 16-byte load brings 8 keys: lane l holds the vectors j * 64 + l (j < KW / 4)
// of its row, i.e. columns (j * 64 + l) * 8 + {0..7}, two to a register, the
// lower column in the low half.  Every word becomes two "ords" right after its
// load (kth_k16.hpp: a uint16 monotone in the public order key; float kinds by
// k16_ord2<2>, four integer instructions a pair), xor 0xFFFF in both halves
// for the k largest; columns past `cols` are padded with 0xFFFF after that.
//
// An ord is exactly two 8-bit digits, so every row takes one path: a
// wave-private 256-bin LDS histogram of the high bytes, wave_pick, the same
// over the low bytes of the keys whose high byte matched, wave_pick: the
// answer is hi << 8 | lo.  Only valid columns are counted (the padding 0xFFFF
// is a real uint16 key, and flipped the smallest one): a count is the count of
// the row's keys, and `eqn`, the keys equal to the answer, holds no padding.
// Both digits count into R16_R0 histogram copies (lane % R16_R0 picks one, as
// k_rows_reg's first pass): the high byte of a bfloat16 is its sign and seven
// exponent bits, 29 % of a randn row share one, and LDS adds to one address
// serialise.
//
// Top-k: compaction from the registers in column order (vector-major, then
// lane, then half-word).  A key is kept when its ord is below the answer, or
// equal to it with a tie rank by column below the remaining rank; positions
// and tie ranks are ballot + mbcnt per half-word.  Rows that keep every key
// equal to the k-th (always, for distinct keys) take a shorter form: a lane
// notes its kept half-words of a vector in a bit mask, one wave scan of the
// lanes' counts places it, and it stores its few kept keys in a loop.  The
// kept (ord, column) pairs -- one word each, a column has 13 bits -- are staged
// in the wave's histogram words when k of them fit, then stored with
// consecutive lanes on consecutive outputs.
//
// VEC: a 16-byte aligned base and cols % 8 == 0, so every row starts on a
// 16-byte boundary and a vector lies inside the row or outside it; otherwise
// 2-byte guarded loads and a validity test per column.  Waves never wait for
// each other.  Four rows per 256-thread workgroup, one row per wave, no row
// loop.  Included by kth_kernels.hip after kth_rows.hpp (wave_pick, zero_hist,
// RW_STRIDE) and kth_k16.hpp (the ord transform).
#pragma once

namespace kth {

#ifndef KTH_ROWS16_R0
#define KTH_ROWS16_R0 4  // histogram copies per wave
#endif
constexpr int R16_R0 = KTH_ROWS16_R0;
constexpr int R16_WORDS = R16_R0 * RW_STRIDE;  // a wave's LDS words: the histogram copies, then the staged top-k
static_assert((R16_R0 & (R16_R0 - 1)) == 0, "lane % R16_R0 is a mask");
constexpr int R16_MAX_COLS = 8192;  // KW = 64: 128 keys a lane
static_assert(R16_MAX_COLS <= 1 << 16, "a staged pair keeps its column in 16 bits");

// Waves per SIMD the register budget is held to.  KW = 64: the top-k keeps the
// row's 64 words live through the compaction beside eight ballots, and the
// guarded loads keep a validity mask per vector: 2 waves, no scratch.
constexpr int r16_waves(int KW, bool VEC, bool TOPK) { return KW >= 64 && (TOPK || !VEC) ? 2 : 4; }

// How many columns of the 8-key vector starting at column e lie in the row:
// its half-word h is valid iff h < r16_valid (VEC: 8 or 0; else any number,
// negative past the row's end, above 8 inside it).
template <bool VEC>
__device__ __forceinline__ int r16_valid(uint32_t e, uint32_t cols) {
    if (VEC) return e < cols ? 8 : 0;
    return (int)cols - (int)e;
}

__device__ __forceinline__ void r16_add(uint32_t *h, uint32_t bin) {
    (void)__hip_atomic_fetch_add(h + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The kk-th smallest ord of the row's valid columns.  kk becomes its rank among
// the keys equal to it, eqn their number.
template <int KW, bool VEC>
__device__ __forceinline__ uint32_t r16_select(const uint32_t (&key)[KW], uint32_t *hist, int lane, uint32_t cols,
                                               uint32_t &kk, uint32_t &eqn) {
    uint32_t *mine = hist + (lane & (R16_R0 - 1)) * RW_STRIDE;
    uint32_t bin, below, cnt;
    // ---- digit 1: the high bytes
    zero_hist(hist, R16_R0, lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < KW / 4; ++j) {
        const int vm = r16_valid<VEC>((uint32_t)(j * WAVE + lane) * 8u, cols);
        if (vm > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t w = key[4 * j + q];
                if (VEC || (vm > 2 * q)) r16_add(mine, (w >> 8) & 0xFFu);
                if (VEC || (vm > 2 * q + 1)) r16_add(mine, w >> 24);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    wave_pick(hist, R16_R0, lane, kk, bin, below, cnt);
    kk -= below;
    const uint32_t hi = bin;
    __builtin_amdgcn_wave_barrier();  // the zeroing after every lane's histogram reads
    // ---- digit 2: the low bytes of the keys with that high byte
    zero_hist(hist, R16_R0, lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < KW / 4; ++j) {
        const int vm = r16_valid<VEC>((uint32_t)(j * WAVE + lane) * 8u, cols);
        if (vm > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t w = key[4 * j + q];
                if ((VEC || (vm > 2 * q)) && ((w >> 8) & 0xFFu) == hi) r16_add(mine, w & 0xFFu);
                if ((VEC || (vm > 2 * q + 1)) && (w >> 24) == hi) r16_add(mine, (w >> 16) & 0xFFu);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    wave_pick(hist, R16_R0, lane, kk, bin, below, cnt);
    kk -= below;
    eqn = cnt;
    __builtin_amdgcn_wave_barrier();  // the staged top-k after every lane's histogram reads
    return hi << 8 | bin;
}

// TOPK = false: out[r] = the bits of the k-th smallest of row r.
// TOPK = true: vals[r*k ..] / idx[r*k ..] = the k smallest keys of row r and
// their columns, in column order; of the keys equal to the k-th, the first
// ones by column.  flip = 0xFFFFFFFF selects the k largest (the ords reversed).
// FLT: float16 / bfloat16 (k16_ord2<2>); else int16 / uint16, whose ord is the
// word xor a constant (k16_ord2<1>'s 0x8000 in both halves for int16), folded
// into the xor of the flip.
template <bool FLT, int KW, bool VEC, bool TOPK>
__global__ __launch_bounds__(RW_BLOCK, r16_waves(KW, VEC, TOPK)) void k_rows16(const uint16_t *__restrict__ m, u64 rows,
                                                                          uint32_t cols, uint32_t k, int kind,
                                                                          uint32_t flip, uint16_t *__restrict__ out,
                                                                          uint16_t *__restrict__ vals,
                                                                          int32_t *__restrict__ idx) {
    static_assert(KW % 4 == 0 && KW * 2 * WAVE <= R16_MAX_COLS, "16-byte loads, columns in 13 bits");
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[RW_BLOCK / WAVE][R16_WORDS];
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    uint32_t *hist = hist_all[wid];
    const u64 r = (u64)blockIdx.x * (RW_BLOCK / WAVE) + wid;
    if (r >= rows) return;  // wave-uniform (no workgroup barrier anywhere)
    const uint16_t *row = m + r * (u64)cols;
    const uint32_t nl2 = k16_nl(kind) * 0x10001u, top2 = k16_top(kind) * 0x10001u;
    const uint32_t xr = flip ^ (kind == 0 ? 0x80008000u : 0u);
    uint32_t key[KW];
#pragma unroll
    for (int j = 0; j < KW / 4; ++j) {
        const uint32_t e = (uint32_t)(j * WAVE + lane) * 8u;  // first column of this lane's vector j
        const int vm = r16_valid<VEC>(e, cols);
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (VEC) {
            if (vm > 0) x = load_nt(reinterpret_cast<const uint4 *>(row + e));
        } else {
            uint32_t h[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = (vm > i) ? (uint32_t)row[e + i] : 0u;
            x = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
        }
        const uint32_t v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = FLT ? k16_ord2<2>(v[q], nl2, top2) ^ flip : v[q] ^ xr;
            const uint32_t pad = VEC ? (vm > 0 ? 0u : 0xFFFFFFFFu)
                                     : ((vm > 2 * q) ? 0u : 0x0000FFFFu) | ((vm > 2 * q + 1) ? 0u : 0xFFFF0000u);
            key[4 * j + q] = w | pad;
        }
        // guarded loads: a vector's eight 2-byte loads are packed before the next
        // vector's are issued (all at once they take 128 registers beside the keys)
        if (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t kk = k, eqn = 0;
    const uint32_t answer = r16_select<KW, VEC>(key, hist, lane, cols, kk, eqn);
    auto bits_of = [&](uint32_t ord) { return k16_bits_of_ord((ord ^ flip) & 0xFFFFu, kind); };
    if (!TOPK) {
        if (lane == 0) out[r] = bits_of(answer);
        return;
    }
    // ---- compaction in column order
    const u64 obase = r * (u64)k;
    const bool stage = k <= (uint32_t)R16_WORDS;  // the kept pairs fit the wave's histogram words
    const bool all_ties = kk == eqn;              // every key equal to the k-th is kept: one compare a key
    auto below_lane = [](unsigned long long b, uint32_t acc) {  // acc + the set bits of b in lanes below this one
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, acc));
    };
    uint32_t taken = 0;
    if (all_ties) {  // wave-uniform
        // The kept keys are exactly the valid ones <= answer.  A lane keeps few of
        // a vector's eight (k << cols) and mostly none: it notes them in a bit
        // mask, one wave scan of the lanes' counts gives its first position, and
        // a loop over the set bits stores them -- no ballot, mbcnt pair and
        // masked store per half-word.
#pragma unroll
        for (int j = 0; j < KW / 4; ++j) {
            if ((uint32_t)(j * WAVE * 8) < cols) {  // wave-uniform: some column of this vector slot is in the row
                const uint32_t e = (uint32_t)(j * WAVE + lane) * 8u;
                const int vm = r16_valid<VEC>(e, cols);
                // (opaque copies: a select among key[]'s elements by a lane's h
                // would be compiled as a lane-indexed load of key[] from scratch)
                uint32_t wv[4] = {key[4 * j], key[4 * j + 1], key[4 * j + 2], key[4 * j + 3]};
                asm volatile("" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]), "+v"(wv[3]));
                uint32_t mk = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t w = wv[q];
                    mk |= ((vm > 2 * q) && (w & 0xFFFFu) <= answer) ? 1u << (2 * q) : 0u;
                    mk |= ((vm > 2 * q + 1) && (w >> 16) <= answer) ? 2u << (2 * q) : 0u;
                }
                const uint32_t c = (uint32_t)__popc(mk);
                const uint32_t incl = wave_incl_scan(c);
                uint32_t pos = taken + incl - c;
                taken += lane_val(incl, WAVE - 1);
                while (mk) {  // (divergent: a lane's kept keys, in column order)
                    const uint32_t h = (uint32_t)__ffs((int)mk) - 1u;
                    mk &= mk - 1u;
                    uint32_t w01, w23, w;
                    const unsigned long long b1 = __ballot((h & 2u) != 0), b2 = __ballot((h & 4u) != 0);
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(w01) : "v"(wv[0]), "v"(wv[1]), "s"(b1));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(w23) : "v"(wv[2]), "v"(wv[3]), "s"(b1));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(w) : "v"(w01), "v"(w23), "s"(b2));
                    const uint32_t ord = (w >> ((h & 1u) * 16u)) & 0xFFFFu;
                    if (pos < k) {  // (exactly k keys are kept; the bound keeps every store inside the row's output)
                        if (stage) {
                            hist[pos] = ord | (e + h) << 16;
                        } else {
                            if (vals) vals[obase + pos] = bits_of(ord);
                            if (idx) idx[obase + pos] = (int32_t)(e + h);
                        }
                    }
                    ++pos;
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the vectors apart: no hoisting across them (VGPRs)
        }
    } else {
        // Ties at the k-th key: positions and tie ranks from ballot + mbcnt per
        // half-word (vector-major, then lane, then half-word = column order).
        uint32_t eq_seen = 0;
#pragma unroll
        for (int j = 0; j < KW / 4; ++j) {
            if ((uint32_t)(j * WAVE * 8) < cols) {  // wave-uniform
                const uint32_t e = (uint32_t)(j * WAVE + lane) * 8u;
                const int vm = r16_valid<VEC>(e, cols);
                uint32_t o[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[2 * q] = key[4 * j + q] & 0xFFFFu;
                    o[2 * q + 1] = key[4 * j + q] >> 16;
                }
                bool sel[8], eq[8];
                unsigned long long bs[8];
                uint32_t rank = eq_seen;
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    eq[h] = (vm > h) && o[h] == answer;
                    const unsigned long long be = __ballot(eq[h]);
                    rank = below_lane(be, rank);
                    eq_seen += (uint32_t)__popcll(be);
                }
#pragma unroll
                for (int h = 0; h < 8; ++h) {  // rank: the tie rank of this lane's next equal key
                    sel[h] = ((vm > h) && o[h] < answer) || (eq[h] && rank < kk);
                    rank += eq[h] ? 1u : 0u;
                    bs[h] = __ballot(sel[h]);
                }
                unsigned long long any = 0;
#pragma unroll
                for (int h = 0; h < 8; ++h) any |= bs[h];
                if (any) {  // wave-uniform
                    uint32_t pos = taken;
#pragma unroll
                    for (int h = 0; h < 8; ++h) pos = below_lane(bs[h], pos);
#pragma unroll
                    for (int h = 0; h < 8; ++h) {
                        if (sel[h] && pos < k) {  // (the bound: as above)
                            if (stage) {
                                hist[pos] = o[h] | (e + (uint32_t)h) << 16;
                            } else {
                                if (vals) vals[obase + pos] = bits_of(o[h]);
                                if (idx) idx[obase + pos] = (int32_t)(e + (uint32_t)h);
                            }
                        }
                        pos += sel[h] ? 1u : 0u;
                        taken += (uint32_t)__popcll(bs[h]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the vectors apart: no hoisting across them (VGPRs)
        }
    }
    if (stage) {  // consecutive lanes store consecutive outputs
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < k; i += WAVE) {
            const uint32_t p = hist[i];
            if (vals) vals[obase + i] = bits_of(p & 0xFFFFu);
            if (idx) idx[obase + i] = (int32_t)(p >> 16);
        }
    }
}

}  // namespace kth
