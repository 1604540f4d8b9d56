// kth_rows_sort.hpp -- a stable in-place sort of each row of a rows x k top-k
// output (include/kth.h "rows, sorted top-k"): the first n_r entries of row r,
// values and their int32 payloads, best first; equal keys keep their input
// order; entries [n_r, k) are neither read nor written.
//
// What is sorted is one composite word an entry: (order key, flipped for
// `largest`; input position).  Positions within a row are distinct, so the
// composites are, and a bitonic network over them is a stable sort of the keys.
// A row is padded to a power of two with a sentinel that sorts last.  The
// composite carries no value and no payload: once the composites stand sorted,
// slot j takes the value and the payload of the position its composite names,
// moved bit for bit (a NaN keeps its payload, which its order key has lost).
//   int32 / float32   u64: key << 32 | position            sentinel ~0
//   16-bit kinds      u32: key << 12 | position (< 4096)   sentinel ~0
//
// Two forms, by k' = the power of two at or above k:
//   wave, k' <= 64      One entry a lane, 64 / k' rows a wavefront, four
//          wavefronts a workgroup.  Every compare-exchange is a cross-lane move
//          (sort_xchg: DPP quad permutes for partners 1 and 2 lanes away,
//          ds_swizzle for 4 / 8 / 16, a permute for 32) -- no LDS memory.  The
//          values and payloads stay in the lane that loaded them and are
//          fetched by the sorted position with one permute each.  Lanes of rows
//          past the end, of rows with n_r <= 1 and of entries at or past n_r
//          load nothing and store nothing.
//   workgroup, k' <= 4096   One 256-thread workgroup a row, the composites in
//          LDS (k' words, dynamic: 32 KiB at most).  Each wavefront sorts
//          64-entry chunks in registers with the wave form's network (every
//          merge size up to 64 in one go), then per merge size the strides of
//          64 and more run over LDS, a pair a thread (consecutive lanes on
//          consecutive words: conflict-free 8-byte accesses), and the strides
//          below 64 again in registers, a chunk a wavefront.  The network runs
//          over n' = the power of two at or above n_r (64 at least), not k'.
//          Every thread then reads the values and payloads its output slots
//          take, a barrier, and only then the first store: the sort is in
//          place.
// Rows are taken in a grid-stride loop (rows is 64-bit, the grid is bounded).
// No scratch, no atomics, no cooperative launch, no in-launch flag.
// Included by kth_kernels.hip after kth_rows_sample.hpp.
#pragma once

namespace kth {

constexpr int SORT_BLOCK = 256;
constexpr int SORT_MAX_K = 4096;
constexpr int SORT_PER = SORT_MAX_K / SORT_BLOCK;  // output slots a thread of the workgroup form
constexpr int SORT_GRID_MAX = 1 << 16;

// ---- key kinds: the element, the composite, the order key
struct SortI32 {
    typedef uint32_t elem;
    typedef u64 comp;
    static __device__ __forceinline__ comp make(elem b, uint32_t flip, uint32_t pos, int) {
        return (u64)(key_of_i32(b) ^ flip) << 32 | pos;
    }
};
struct SortF32 {
    typedef uint32_t elem;
    typedef u64 comp;
    static __device__ __forceinline__ comp make(elem b, uint32_t flip, uint32_t pos, int) {
        return (u64)(key_of_f32(b) ^ flip) << 32 | pos;
    }
};
struct SortK16 {
    typedef uint16_t elem;
    typedef uint32_t comp;
    static __device__ __forceinline__ comp make(elem b, uint32_t flip, uint32_t pos, int kind) {
        return (((uint32_t)k16_key_of_bits(b, kind) ^ flip) & 0xFFFFu) << 12 | pos;
    }
};
static_assert(SORT_MAX_K <= 1 << 12, "a position fits the 16-bit kinds' composite");

template <class C>
__device__ __forceinline__ C sort_sentinel() {
    return (C)~(C)0;
}
// the input position a sorted composite names
__device__ __forceinline__ uint32_t sort_pos(u64 x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t sort_pos(uint32_t x) { return x & 0xFFFu; }

// ---- the value of the lane S lanes away (lane ^ S), S a power of two
template <int S>
__device__ __forceinline__ uint32_t sort_xchg(uint32_t x) {
    static_assert(S == 1 || S == 2 || S == 4 || S == 8 || S == 16 || S == 32, "a partner within the wavefront");
    if constexpr (S == 1)
        return dpp32<0xB1, 0xF>(x);  // quad_perm:[1,0,3,2]
    else if constexpr (S == 2)
        return dpp32<0x4E, 0xF>(x);  // quad_perm:[2,3,0,1]
    else if constexpr (S <= 16)      // bit-mask mode within 32 lanes: and 0x1F, or 0, xor S
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, (S << 10) | 0x1F);
    else
        return (uint32_t)__shfl_xor((int)x, 32, WAVE);
}
template <int S>
__device__ __forceinline__ u64 sort_xchg(u64 x) {
    const uint32_t lo = sort_xchg<S>((uint32_t)x), hi = sort_xchg<S>((uint32_t)(x >> 32));
    return (u64)hi << 32 | lo;
}

// The strides S, S / 2, ... 1 of one bitonic merge: entry e (its low bits are
// the lane's) keeps the lesser of the pair where it is the lower partner of an
// ascending merge or the upper one of a descending merge, else the greater.
template <class C, int S>
__device__ __forceinline__ void sort_merge(C &x, uint32_t e, bool asc) {
    const C y = sort_xchg<S>(x);
    const bool lesser = ((e & (uint32_t)S) == 0u) == asc;
    x = ((y < x) == lesser) ? y : x;
    if constexpr (S > 1) sort_merge<C, S / 2>(x, e, asc);
}
// Every merge size from SIZE to W (<= 64): entries [e & ~(W - 1), + W) end up
// ascending where (e & W) == 0, descending elsewhere.
template <class C, int SIZE, int W>
__device__ __forceinline__ void sort_lanes(C &x, uint32_t e) {
    sort_merge<C, SIZE / 2>(x, e, (e & (uint32_t)SIZE) == 0u);
    if constexpr (SIZE < W) sort_lanes<C, SIZE * 2, W>(x, e);
}

// n_r of row r
__device__ __forceinline__ uint32_t sort_row_n(const int32_t *__restrict__ cnt, u64 r, uint32_t k) {
    if (!cnt) return k;
    const int32_t c = cnt[r];
    return c <= 0 ? 0u : (uint32_t)c < k ? (uint32_t)c : k;
}

// ---- wave form: KP = k' lanes a row
template <class T, int KP>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_wave(typename T::elem *vals, int32_t *idx, u64 rows, uint32_t k,
                                                          const int32_t *__restrict__ cnt, uint32_t flip, int kind) {
    typedef typename T::comp C;
    constexpr uint32_t RPW = WAVE / KP;  // rows a wavefront
    const uint32_t lane = threadIdx.x & (WAVE - 1), p = lane & (KP - 1), first = lane & ~(uint32_t)(KP - 1);
    const u64 gw = (u64)blockIdx.x * (SORT_BLOCK / WAVE) + threadIdx.x / WAVE;
    const u64 nw = (u64)gridDim.x * (SORT_BLOCK / WAVE);
    for (u64 r0 = gw * RPW; r0 < rows; r0 += nw * RPW) {  // (wave-uniform)
        const u64 r = r0 + lane / KP;
        const uint32_t n = r < rows ? sort_row_n(cnt, r, k) : 0u;
        const bool act = n > 1u && p < n;  // this lane holds an entry that may move
        if (__builtin_amdgcn_ballot_w64(act) == 0) continue;  // (wave-uniform)
        const u64 at = r * k + p;
        typename T::elem v = 0;
        int32_t ix = 0;
        if (act) {
            v = vals[at];
            if (idx) ix = idx[at];
        }
        C x = act ? T::make(v, flip, p, kind) : sort_sentinel<C>();
        sort_lanes<C, 2, KP>(x, p);
        // slot p of an active row takes the entry at sort_pos(x) (< n: the sentinels stand last)
        const int src = (int)(first + (act ? sort_pos(x) : p));
        const uint32_t ov = (uint32_t)__shfl((int)(uint32_t)v, src, WAVE);
        const int32_t oi = __shfl(ix, src, WAVE);
        if (act) {
            vals[at] = (typename T::elem)ov;
            if (idx) idx[at] = oi;
        }
    }
}

// ---- workgroup form: one workgroup a row, kp * sizeof(comp) bytes of dynamic LDS
template <class T>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_wg(typename T::elem *vals, int32_t *idx, u64 rows, uint32_t k,
                                                        const int32_t *__restrict__ cnt, uint32_t flip, int kind) {
    typedef typename T::comp C;
    typedef typename T::elem E;
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
    C *comp = reinterpret_cast<C *>(sort_lds);
    const uint32_t lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    constexpr uint32_t NW = SORT_BLOCK / WAVE;
    for (u64 r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t n = sort_row_n(cnt, r, k);
        if (n <= 1u) continue;  // (workgroup-uniform)
        uint32_t np = WAVE;     // the network's size: n <= np <= k'
        while (np < n) np <<= 1;
        E *rv = vals + r * k;
        int32_t *ri = idx ? idx + r * k : nullptr;
        const uint32_t chunks = np / WAVE;
        // every merge size up to 64, a chunk a wavefront, straight from the row
        for (uint32_t c = wid; c < chunks; c += NW) {  // (wave-uniform)
            const uint32_t e = c * WAVE + lane;
            C x = sort_sentinel<C>();
            if (e < n) x = T::make(rv[e], flip, e, kind);
            sort_lanes<C, 2, WAVE>(x, e);
            comp[e] = x;
        }
        __syncthreads();
        for (uint32_t size = 2 * WAVE; size <= np; size <<= 1) {
            for (uint32_t stride = size / 2; stride >= (uint32_t)WAVE; stride >>= 1) {
                for (uint32_t t = threadIdx.x; t < np / 2; t += SORT_BLOCK) {
                    const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const C a = comp[i], b = comp[j];
                    if ((b < a) == ((i & size) == 0u)) comp[i] = b, comp[j] = a;
                }
                __syncthreads();
            }
            for (uint32_t c = wid; c < chunks; c += NW) {  // (wave-uniform) strides 32 ... 1
                const uint32_t e = c * WAVE + lane;
                C x = comp[e];
                sort_merge<C, WAVE / 2>(x, e, (e & size) == 0u);
                comp[e] = x;
            }
            __syncthreads();
        }
        // slot j takes the entry at sort_pos(comp[j]); all of the row is read before any of it is written
        E gv[SORT_PER];
        int32_t gi[SORT_PER];
#pragma unroll
        for (int q = 0; q < SORT_PER; ++q) {
            const uint32_t j = threadIdx.x + (uint32_t)q * SORT_BLOCK;
            gv[q] = 0, gi[q] = 0;
            if (j < n) {
                const uint32_t src = sort_pos(comp[j]);
                gv[q] = rv[src];
                if (ri) gi[q] = ri[src];
            }
        }
        // (the barrier alone does not wait for loads in flight: the compiler puts that wait before
        // the first use of a loaded register, which is after it)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SORT_PER; ++q) {
            const uint32_t j = threadIdx.x + (uint32_t)q * SORT_BLOCK;
            if (j < n) {
                rv[j] = gv[q];
                if (ri) ri[j] = gi[q];
            }
        }
    }
}

}  // namespace kth
