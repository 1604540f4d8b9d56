// kth_multi.hpp -- the streaming pass for several ranks of one array (gfx950).
// Included by kth_kernels.hip.
//
// kth_select_multi_* resolves up to MULTI_MAX ranks of the same keys: k_head
// runs once per rank (each into its own state and slots), then ONE launch of
// k_main_multi streams the input and serves every rank's window from each
// loaded tile, then k_finish runs once per rank over that rank's count slot
// and candidate buffer.  What a window leaves behind is exactly what k_main<0>
// leaves for a single select (counts C_LT / C_EQLO / C_EQHI / C_IN / C_OVF in
// its slot, candidates as order keys, the candidate count), so decide() and
// k_finish -- and their whole-input fallback -- are the single select's.
//
// Structure.  The load schedule is k_main<0>'s (16-byte nontemporal loads, one
// load, a wait, then the rest; ord_word right after the load; head / tail for
// unaligned pointers).  The windows are a RUNTIME loop over each loaded tile:
// the per-window state is wave-uniform and lives in LDS between tiles (the
// window bounds, the wave's staging fill and its four counts), so the kernel's
// registers and code size do not grow with the number of windows, a call with
// m windows does the work of m (not of the instantiation's maximum), and
// nothing is indexed dynamically in registers (no scratch).  Per key and window
// the counts are taken as ballots: #<lo is a compare into an SGPR pair plus a
// scalar popcount and add, and "in [lo, hi]" is the mask of x <= hi without it,
// so a key costs 2 VALU operations a window (two compares); the edges and the
// staging only run on the wave slots where some lane's key lies in the window,
// as in Stager::slot_near, and there too the masks are combined as scalars.
// The windows share ONE staging region per wave, MULTI_WREG = 1024 words split
// M ways (512 / 256 / 128 words a window for M = 2 / 4 / 8): ~17-19 KB of LDS a
// workgroup and 62 VGPRs, so eight workgroups fit a CU (k_main<0>: four); the
// pass is bound by the latency of its compare -> mask -> branch chains, not by
// HBM, and the waves hide it (2048 words and four workgroups: +14 %).  A
// region that fills is flushed by its wave with one reservation in that
// window's candidate buffer (the only global stores inside the tile loop).
#pragma once

namespace kth {

constexpr int MULTI_MAX = 8;  // == KTH_MULTI_MAX_RANKS
#ifndef KTH_MULTI_WREG
#define KTH_MULTI_WREG 1024
#endif
constexpr int MULTI_WREG = KTH_MULTI_WREG;  // a wave's staging words, split between the windows

struct MultiWin {
    const SelState *st_in;  // the window state k_head left (MODE_MAIN)
    SelState *st_out;       // ... carried to k_finish
    u64 *acc;               // the window's count slot (zero on entry)
    u64 *cand_count;        // its candidate count (zero on entry)
    uint32_t *cand;         // its candidate buffer
    u64 cap;                // ... and its capacity in keys
};
struct MultiArgs {
    const int32_t *keys;
    u64 n;
    int m;  // windows in use
    MultiWin w[MULTI_MAX];
};

// a window as the tile loop reads it from LDS (wave-uniform)
struct MultiLds {
    int32_t slo, shi;
    uint32_t active, pad;
    u64 *acc, *cand_count;
    uint32_t *cand;
    u64 cap;
};
enum : int { MW_LT = 0, MW_EQLO = 1, MW_EQHI = 2, MW_IN = 3, MW_FILL = 4, MW_WORDS = 5 };
static_assert(MW_LT == C_LT && MW_EQLO == C_EQLO && MW_EQHI == C_EQHI && MW_IN == C_IN, "a wave's counts in slot order");

// M: the most windows this instantiation serves (it sets the staging split).
template <int M, bool F32 = false>
__global__ __launch_bounds__(BLK) void k_main_multi(MultiArgs ma) {
    constexpr int U = MAIN_UNROLL, NW = BLK / WAVE, RW = MULTI_WREG / M;
    constexpr int SV = sizeof(SelState) / 16;
    static_assert(M <= MULTI_MAX && MULTI_WREG % M == 0 && RW >= 2 * WAVE, "a window's region holds two full wave slots");
    static_assert(MULTI_MAX * SV <= BLK && MULTI_MAX * 8 <= BLK, "states and counts move with one thread per word");
    __shared__ SelState ss[M];
    __shared__ MultiLds win[M];
    __shared__ __attribute__((aligned(16))) uint32_t region[NW][M][RW];
    __shared__ uint32_t wv[NW][M][MW_WORDS];  // a wave's counts and fill per window
    __shared__ u64 gbase[M];                  // the workgroup's final reservation per window
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ma.keys);
    const u64 n = ma.n;
    const int m = ma.m < M ? ma.m : M;
    u64 head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(p + head);
    const u64 nv = (n - head) >> 2, tail0 = head + (nv << 2);
    const u64 tile = (u64)BLK * U, nfull = nv / tile;
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;

    // the windows' states, one 16-byte word a thread; workgroup 0 carries them on
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int i = (int)threadIdx.x - j * SV;
        if (j < m && i >= 0 && i < SV) {
            const uint4 q = reinterpret_cast<const uint4 *>(ma.w[j].st_in)[i];
            reinterpret_cast<uint4 *>(&ss[j])[i] = q;
            if (blockIdx.x == 0) reinterpret_cast<uint4 *>(ma.w[j].st_out)[i] = q;
        }
    }
    for (int i = threadIdx.x; i < NW * M * MW_WORDS; i += BLK) (&wv[0][0][0])[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < M; ++j)
        if ((int)threadIdx.x == j) {
            MultiLds w;
            const bool on = j < m && ss[j].mode == MODE_MAIN;  // (else an error or a resolved state: k_finish reports it)
            w.slo = on ? i32_of_key(ss[j].lo) : 0;
            w.shi = on ? i32_of_key(ss[j].hi) : 0;
            w.active = on ? 1u : 0u;
            w.pad = 0u;
            w.acc = ma.w[j].acc;
            w.cand_count = ma.w[j].cand_count;
            w.cand = ma.w[j].cand;
            w.cap = ma.w[j].cap;
            win[j] = w;
        }
    __syncthreads();

    auto load_tile = [&](uint4 (&x)[U], u64 t) {  // k_main's schedule: one load, a wait, then the rest
        const uint4 *src = v + t * tile + threadIdx.x;
        x[0] = load_nt(src);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 1; u < U; ++u) x[u] = load_nt(src + u * BLK);
    };

    // One window's state while a wave scans a group of keys: all wave-uniform.
    struct WaveWin {
        int32_t slo, shi;
        uint32_t lt, eqlo, eqhi, in, fill;
    };
    auto flush = [&](const MultiLds &w, uint32_t *reg, WaveWin &s) __attribute__((always_inline)) {
        __builtin_amdgcn_wave_barrier();
        const u64 cap = w.cap;
        const u64 g = reserve_cands(w.cand_count, w.acc, cap, s.fill);
        for (uint32_t i = lane; i < s.fill; i += WAVE)
            if (g + i < cap) put_cand(&w.cand[g + i], reg[i]);
        __builtin_amdgcn_wave_barrier();
        s.fill = 0;
    };
    // (ballots are taken of plain compares only and combined as scalar masks:
    // a ballot of a compound condition is materialised per lane first)
    // a key slot some lane's key of which lies in the closed window (mask N)
    auto near_slot = [&](const MultiLds &w, uint32_t *reg, WaveWin &s, uint32_t xw, unsigned long long N) __attribute__((always_inline)) {
        const int32_t x = (int32_t)xw;
        const unsigned long long EL = __builtin_amdgcn_ballot_w64(x == s.slo) & N;
        const unsigned long long EH = __builtin_amdgcn_ballot_w64(x == s.shi) & N;
        const unsigned long long B = N & ~(EL | EH);  // strictly inside: the candidates
        s.eqlo += (uint32_t)__popcll(EL);
        s.eqhi += (uint32_t)__popcll(EH);
        if (B) {  // wave-uniform
            const uint32_t nb = (uint32_t)__popcll(B);
            if (s.fill + nb > (uint32_t)RW) flush(w, reg, s);
            const uint32_t below =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(B >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)B, 0u));
            // (the order key is made here, from a copy the compiler cannot see
            // through: it otherwise keeps all 32 flipped keys of the tile in
            // registers across the windows, 94 VGPRs instead of 62)
            uint32_t kx = xw;
            asm volatile("" : "+v"(kx));
            if ((B >> lane) & 1ull) reg[s.fill + below] = kx ^ 0x80000000u;
            s.fill += nb;
            s.in += nb;
        }
    };
    // (ballots are taken of plain compares only and combined as scalar masks:
    // a ballot of a compound condition is materialised per lane first)
    // one key slot of the masked groups (ragged tile, head, tail): ok = this lane holds a key
    auto key_slot = [&](const MultiLds &w, uint32_t *reg, WaveWin &s, uint32_t xw, bool ok) __attribute__((always_inline)) {
        const int32_t x = (int32_t)xw;
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
        // two compares a key: below the window, and not above it; the keys in
        // the closed window are the second mask without the first
        const unsigned long long LT = __builtin_amdgcn_ballot_w64(x < s.slo) & okm;
        const unsigned long long N = __builtin_amdgcn_ballot_w64(x <= s.shi) & okm & ~LT;
        s.lt += (uint32_t)__popcll(LT);
        if (__builtin_expect(N == 0, 1)) return;  // wave-uniform
        near_slot(w, reg, s, xw, N);
    };
    // Eight full keys at once: every compare first (16 independent VALU
    // operations back to back), then the scalar work and the near slots.  (A
    // compare, its scalar mask test and a branch per key in turn left each
    // wave waiting on the VALU -> SALU hand-off 32 times a window and tile:
    // ~3 % slower at m = 2 / 4 / 8.)
    auto key_group = [&](const MultiLds &w, uint32_t *reg, WaveWin &s, const uint4 &a, const uint4 &b) __attribute__((always_inline)) {
        const uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        unsigned long long LT[8], N[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            LT[i] = __builtin_amdgcn_ballot_w64((int32_t)k[i] < s.slo);
            N[i] = __builtin_amdgcn_ballot_w64((int32_t)k[i] <= s.shi);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s.lt += (uint32_t)__popcll(LT[i]);
            const unsigned long long n = N[i] & ~LT[i];
            if (__builtin_expect(n != 0, 0)) near_slot(w, reg, s, k[i], n);
        }
    };
    // every active window over one group of keys; the wave's counts and fill
    // come from its LDS words and go back there
    auto scan_windows = [&](auto &&keys_of_window) __attribute__((always_inline)) {
        for (int j = 0; j < m; ++j) {  // wave-uniform
            const MultiLds &w = win[j];
            if (!w.active) continue;
            uint32_t *cnt = wv[wid][j];
            WaveWin s;
            s.slo = __builtin_amdgcn_readfirstlane(w.slo);
            s.shi = __builtin_amdgcn_readfirstlane(w.shi);
            s.fill = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt[MW_FILL]);
            s.lt = s.eqlo = s.eqhi = s.in = 0u;
            keys_of_window(w, region[wid][j], s);
            if (lane == 0) {
                cnt[MW_LT] += s.lt;
                cnt[MW_EQLO] += s.eqlo;
                cnt[MW_EQHI] += s.eqhi;
                cnt[MW_IN] += s.in;
                cnt[MW_FILL] = s.fill;
            }
            __builtin_amdgcn_wave_barrier();  // (a wave's LDS accesses are in order)
        }
    };

    bool any = false;
    for (int j = 0; j < m; ++j) any |= win[j].active != 0u;
    if (!any) return;  // block-uniform

    for (u64 t = blockIdx.x; t < nfull; t += gridDim.x) {
        uint4 x[U];
        load_tile(x, t);
        if constexpr (F32) {
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = ord_word4<true>(x[u]);
        }
        scan_windows([&](const MultiLds &w, uint32_t *reg, WaveWin &s) {
            static_assert(U % 2 == 0, "key groups are two 16-byte loads");
#pragma unroll
            for (int u = 0; u < U; u += 2) key_group(w, reg, s, x[u], x[u + 1]);
        });
    }
    // ragged end: the last partial tile, masked, by one workgroup
    const u64 rem0 = nfull * tile;
    if (blockIdx.x == (uint32_t)(nfull % gridDim.x)) {
        uint4 x[U];
        uint32_t okm = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 i = rem0 + (u64)u * BLK + threadIdx.x;
            const bool in = i < nv;
            x[u] = ord_word4<F32>(in ? v[i] : make_uint4(0, 0, 0, 0));
            okm |= in ? 1u << u : 0u;
        }
        scan_windows([&](const MultiLds &w, uint32_t *reg, WaveWin &s) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = (okm >> u) & 1u;
                key_slot(w, reg, s, x[u].x, ok);
                key_slot(w, reg, s, x[u].y, ok);
                key_slot(w, reg, s, x[u].z, ok);
                key_slot(w, reg, s, x[u].w, ok);
            }
        });
    }
    if (blockIdx.x == 0) {  // the < 4-key unaligned head and tail
        const bool okh = threadIdx.x < head, okt = threadIdx.x < n - tail0;
        const uint32_t kh = ord_word<F32>(okh ? p[threadIdx.x] : 0u), kt = ord_word<F32>(okt ? p[tail0 + threadIdx.x] : 0u);
        scan_windows([&](const MultiLds &w, uint32_t *reg, WaveWin &s) {
            key_slot(w, reg, s, kh, okh);
            key_slot(w, reg, s, kt, okt);
        });
    }
    // counts: the waves' LDS words -> one atomic per workgroup, window and
    // counter; the waves' final fills are reserved together, one reservation
    // per workgroup and window
    __syncthreads();
    {
        const int j = threadIdx.x / 8, c = threadIdx.x % 8;
        if (j < m && c < MW_WORDS && win[j].active) {
            u64 sum = 0;
            for (int q = 0; q < NW; ++q) sum += wv[q][j][c];
            if (c == MW_FILL) {
                u64 g = 0;
                if (sum) {
                    g = atomicAdd(win[j].cand_count, sum);
                    if (g <= win[j].cap && g + sum > win[j].cap) atomicAdd(&win[j].acc[C_OVF], 1ull);
                }
                gbase[j] = g;
            } else if (sum) {
                atomicAdd(&win[j].acc[c], sum);  // (MW_* are the slot's C_* words)
            }
        }
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {  // this wave's final regions, at their share of the reservations
        const MultiLds &w = win[j];
        const uint32_t fill = wv[wid][j][MW_FILL];
        if (!w.active || fill == 0u) continue;
        u64 g = gbase[j];
        for (int q = 0; q < wid; ++q) g += wv[q][j][MW_FILL];
        const u64 cap = w.cap;
        const uint32_t *reg = region[wid][j];
        for (uint32_t i = lane; i < fill; i += WAVE)
            if (g + i < cap) put_cand(&w.cand[g + i], reg[i]);
    }
}

}  // namespace kth
