// kth_topk16.hpp -- top-k of one array of 16-bit keys (int16, uint16, float16,
// bfloat16), gfx950.  Included by kth_api.hip after kth_k16.hpp and
// kth_topk.hpp; it adds kernels and changes none.
//
// The k smallest (or largest) keys of n with their int64 indices, in index
// order; of the keys equal to the k-th, the first ones by index.  A 16-bit key
// has 65536 values, so the k-th value nearly always has a large tie group
// (2^30 uniform int16 keys: ~16384 copies of each value): the tie quota is
// the normal case here, not a corner.
// After the 16-bit select (kth_k16.hpp) has left the k-th key's ord v in
// K16State[0].answer, on 2048-key wave tiles (one wavefront each, no barriers):
//   k16_topk_count  per tile, #better-than-v | #equal << 16, in ord space on
//                   packed halves; tiles the select's streaming pass proved
//                   empty of output (k16_main_tf's row flags) are not loaded
//   k_topk_bases    kth_topk.hpp's, unchanged, with a null SelState
//   k16_topk_write  per tile that holds an output key: wave scan, pairs
//                   staged in the wave's LDS, coalesced copy-out of 2-byte
//                   values and int64 indices.  Its first thread carries a
//                   bracket failure (meta[1]) to K16State[0].error.
// A kept key's slot is (#better before it) + min(#equal before it, need).
//
// Tile: 2048 keys = 4 KiB = four 16-byte loads a lane, the bytes in flight of
// the 32-bit tile.  #better <= 2048 < 2^16 and #equal <= 2048 < 2^15, so the
// count word is kth_topk.hpp's (tk_better_of / tk_equal_of), and a
// k_topk_bases block of 4096 tiles holds 2^23 keys: its "per block < 2^32
// keys" note holds.
// Alignment: d_keys needs 2-byte alignment.  Tiles are cut in "virtual"
// indices j = i + pad, where pad < 8 is the number of keys between the 16-byte
// boundary below d_keys and d_keys itself, so every tile starts on a 16-byte
// boundary; the valid keys are j in [pad, n + pad).  A tile wholly inside that
// range is read with 16-byte loads; the first tile (pad != 0) and the last one
// (ragged) with guarded 2-byte loads, as k16_main reads its head and tail.
// ALIGNED instantiations have pad == 0 folded in.
#pragma once

namespace kth {

constexpr int TK16_TILE = 2048;               // keys per wave tile
constexpr int TK16_KPL = TK16_TILE / WAVE;    // 32 keys per lane
constexpr int TK16_WPL = TK16_KPL / 2;        // 16 packed words = four 16-byte loads per lane
constexpr u64 TK16_MAIN_ROW = (u64)BLK * 8;   // keys per k16_main row (one 16-byte load per thread)
static_assert(TK16_TILE < (1 << 15), "#equal fits tk_equal_of's 15 bits");
static_assert((u64)TK_TILES_PER_BLOCK * TK16_TILE < (1ull << 32), "k_topk_bases: per block < 2^32 keys");
static_assert(TK16_MAIN_ROW == (u64)TK16_TILE, "a tile spans at most two k16_main rows");
static_assert(BLK / WAVE == 4, "a k16_main tile's four flag bytes are one 32-bit word");

struct Tk16Args {
    const uint16_t *keys;
    u64 n, pad, ntiles;   // virtual keys [pad, n + pad), ntiles = ceil((n + pad) / TK16_TILE)
    const K16State *st;   // the select's state: answer = the k-th key's ord
    uint32_t flip;        // 0 for smallest, 0xFFFF for largest
    uint32_t nl2, top2;   // k16_ord2's constants
    uint32_t *tcnt;
};
// what the count pass needs to skip tiles (k16_main_tf ran as pass 0)
struct Tk16Skip {
    const uint32_t *hdr;  // K16Flags.hdr: [lo, hi, ran, -], then a 32-bit word of four flag bytes per k16_main tile
    u64 head, nfull;      // k16_main's geometry: unaligned keys before its rows, full tiles
    uint32_t use;         // 0: ignore the flags (the unflagged pass ran, or KTH_HOOK_K16_TOPK_NOSKIP)
    u64 *nread;           // += the tiles loaded from the input (kth_ctx_last_topk_k16_tiles)
};

// Two packed ords (already xor-ed with the direction's flip) against the k-th
// in both halves, v2: adds 1 to nb's half for a better key, 1 to nne's half for
// a key that differs.  Packed integer operations only: v - x saturates to 0
// unless x < v; min(.., 1) turns "nonzero" into 1.
__device__ __forceinline__ void tk16_acc(uint32_t x2, uint32_t v2, uint32_t &nb, uint32_t &nne) {
    const k16_u2 x = __builtin_bit_cast(k16_u2, x2), v = __builtin_bit_cast(k16_u2, v2);
    const k16_u2 one = {1, 1};
    const k16_u2 b = __builtin_elementwise_min(__builtin_elementwise_sub_sat(v, x), one);
    const k16_u2 d = __builtin_elementwise_min((k16_u2)(x ^ v), one);
    nb += __builtin_bit_cast(uint32_t, b);  // (at most TK16_WPL per half: no carry)
    nne += __builtin_bit_cast(uint32_t, d);
}

// bit r % 8 of any of the four waves' bytes of k16_main tile r / 8
__device__ __forceinline__ bool tk16_row_flagged(const uint32_t *fw, u64 r) {
    return (fw[r / K16_UNROLL] & (0x01010101u << (uint32_t)(r % K16_UNROLL))) != 0u;
}

// bits q of a lane's run of 32 virtual keys [j0, j0 + 32) that lie in [pad, end)
__device__ __forceinline__ uint32_t tk16_run_mask(u64 j0, u64 pad, u64 end) {
    auto below = [](u64 x) { return x >= 32 ? ~0u : (1u << (uint32_t)x) - 1u; };  // bits [0, x)
    const uint32_t lo = j0 >= pad ? 0u : below(pad - j0), hi = j0 >= end ? 0u : below(end - j0);
    return hi & ~lo;
}

// Pass 1: tile t = virtual keys [2048 t, 2048 t + 2048); tcnt[t] = #better |
// #equal << 16.  Lane l reads the 16-byte words l, l + 64, l + 128, l + 192 of
// its tile.  Each wave takes 64 tiles at a time: lane l tests tile tg + l's
// flags, the wave then streams only the tiles that may hold output
// (k_topk_count's scheme).  A tile is skipped, count 0 and no loads, when
//   - k16_main_tf ran in this call (hdr[2] == 1, sk.use) and the k-th key v
//     lies on the near side of the far edge of the window that pass used
//     (smallest: v <= hi0, largest: v >= lo0), so an unflagged row holds no
//     key <= v (>= v): a window that missed on the far side turns skipping off;
//   - every key of the tile lies in k16_main's full tiles (after `head`
//     unaligned keys, before the masked remainder and the tail), and
//   - the one or two rows it touches are unflagged in all four waves' bytes.
template <int CV, bool ALIGNED>
__global__ __launch_bounds__(TK_BLOCK) void k16_topk_count(Tk16Args a, Tk16Skip sk) {
    const uint32_t vo = a.st->answer;
    const uint32_t fv = (vo ^ a.flip) & 0xFFFFu, v2 = fv | fv << 16, flip2 = a.flip | a.flip << 16;
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 nw = (u64)gridDim.x * (TK_BLOCK / WAVE);
    const u64 pad = ALIGNED ? 0 : a.pad, end = a.n + pad;
    // the virtual array's 16-byte words (word 0 is dereferenced only when pad == 0)
    const uint4 *vw = reinterpret_cast<const uint4 *>(reinterpret_cast<uintptr_t>(a.keys) - 2 * pad);
    const bool skip_ok = sk.use != 0u && sk.hdr[2] == 1u && (a.flip == 0u ? vo <= sk.hdr[1] : vo >= sk.hdr[0]);
    const uint32_t *fw = sk.hdr + 4;
    uint32_t nread = 0;
    for (u64 tg = ((u64)blockIdx.x * (TK_BLOCK / WAVE) + threadIdx.x / WAVE) * WAVE; tg < a.ntiles; tg += nw * WAVE) {
        const u64 tl = tg + lane;
        bool act = tl < a.ntiles;
        if (act && skip_ok) {
            const u64 j0 = tl * TK16_TILE, jA = j0 > pad ? j0 : pad;
            const u64 jB = (j0 + TK16_TILE < end ? j0 + TK16_TILE : end) - 1;  // jA <= jB: j0 < end, pad < 8
            if (jA - pad >= sk.head) {
                const u64 ra = (jA - pad - sk.head) / TK16_MAIN_ROW, rb = (jB - pad - sk.head) / TK16_MAIN_ROW;
                if (rb / K16_UNROLL < sk.nfull && !tk16_row_flagged(fw, ra) && !tk16_row_flagged(fw, rb)) {
                    act = false;
                    a.tcnt[tl] = 0u;
                }
            }
        }
        u64 todo = __ballot(act);
        nread += (uint32_t)__popcll(todo);
        while (todo) {  // two tiles per round: 8 loads in flight per lane
            const u64 t1 = tg + __builtin_ctzll(todo);
            todo &= todo - 1;
            const bool two = todo != 0;
            const u64 t2 = two ? tg + __builtin_ctzll(todo) : t1;
            if (two) todo &= todo - 1;
            const u64 b1 = t1 * TK16_TILE, b2 = t2 * TK16_TILE;
            uint32_t c1, c2;
            if (b1 >= pad && b2 >= pad && b1 + TK16_TILE <= end && b2 + TK16_TILE <= end) {
                uint4 q[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    q[r] = load_nt(vw + b1 / 8 + r * WAVE + lane);
                    q[4 + r] = load_nt(vw + b2 / 8 + r * WAVE + lane);
                }
                uint32_t nb1 = 0, ne1 = 0, nb2 = 0, ne2 = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint4 o1 = k16_ord8<CV>(q[r], a.nl2, a.top2), o2 = k16_ord8<CV>(q[4 + r], a.nl2, a.top2);
                    tk16_acc(o1.x ^ flip2, v2, nb1, ne1);
                    tk16_acc(o1.y ^ flip2, v2, nb1, ne1);
                    tk16_acc(o1.z ^ flip2, v2, nb1, ne1);
                    tk16_acc(o1.w ^ flip2, v2, nb1, ne1);
                    tk16_acc(o2.x ^ flip2, v2, nb2, ne2);
                    tk16_acc(o2.y ^ flip2, v2, nb2, ne2);
                    tk16_acc(o2.z ^ flip2, v2, nb2, ne2);
                    tk16_acc(o2.w ^ flip2, v2, nb2, ne2);
                }
                c1 = ((nb1 & 0xFFFFu) + (nb1 >> 16)) | ((uint32_t)TK16_KPL - (ne1 & 0xFFFFu) - (ne1 >> 16)) << 16;
                c2 = ((nb2 & 0xFFFFu) + (nb2 >> 16)) | ((uint32_t)TK16_KPL - (ne2 & 0xFFFFu) - (ne2 >> 16)) << 16;
            } else {  // the first tile of unaligned keys, the ragged last tile: guarded 2-byte loads
                c1 = c2 = 0;
                auto one = [&](uint32_t &c, u64 j) {
                    if (j < pad || j >= end) return;
                    const uint32_t x = k16_ord1<CV>(a.keys[j - pad], a.nl2, a.top2) ^ a.flip;
                    c += x < fv ? 1u : 0u;
                    c += x == fv ? 0x10000u : 0u;
                };
#pragma unroll 4
                for (int j = 0; j < TK16_KPL; ++j) {
                    one(c1, b1 + (u64)j * WAVE + lane);
                    one(c2, b2 + (u64)j * WAVE + lane);
                }
            }
            c1 = wave_sum32(c1);
            c2 = wave_sum32(c2);
            if (lane == 0) {
                a.tcnt[t1] = c1;
                if (two) a.tcnt[t2] = c2;
            }
        }
    }
    if (lane == 0 && nread) atomicAdd(reinterpret_cast<unsigned long long *>(sk.nread), (unsigned long long)nread);
}

// Pass 3: ordered compaction, k_topk_write's scheme on 2048-key tiles.  Each
// wave looks at 64 tiles at once (one per lane) and visits only those that
// hold a better key, or an equal key while the tie quota before the tile is
// not exhausted (be < need).  Lane l owns the run of virtual keys [2048 t +
// 32 l, + 32) of tile t: its four 16-byte loads are the consecutive words
// 4 l .. 4 l + 3 of the tile, so key j of the run is half j & 1 of the lane's
// packed word j >> 1, and a wave scan of the per-lane counts gives index
// order.  With pb / pe the better / equal keys of the tile before a key and
// cap the ties the tile may still take, a better key goes to slot pb +
// min(pe, cap) of the tile's output range, a tie with pe < cap to pb + pe.
// The pairs (value bits, position in the tile) are staged in the wave's LDS
// and written out coalesced.  A NaN is written canonical.  vals or idx may be
// null.  The first thread carries a bracket failure to the select's state.
constexpr int TK16W_TILES = 4;  // tiles a wave loads together (16 loads in flight per lane, as k_topk_write)
struct Tk16Out {
    const u64 *toff, *bbase, *meta;
    K16State *st;
    uint32_t inf, canon;  // float kinds: bits & 0x7FFF > inf is a NaN, written as canon (integer kinds: inf = 0xFFFF)
    uint16_t *vals;
    int64_t *idx;
};
template <int CV, bool ALIGNED>
__global__ __launch_bounds__(TK_BLOCK) void k16_topk_write(Tk16Args a, Tk16Out o) {
    __shared__ uint16_t s_val[TK_BLOCK / WAVE][TK16_TILE];
    __shared__ uint16_t s_col[TK_BLOCK / WAVE][TK16_TILE];
    if (o.meta[1]) {  // grid-uniform: the counts do not bracket k
        if (blockIdx.x == 0 && threadIdx.x == 0) o.st->error = TK_ERR_BRACKET;
        return;
    }
    if (o.st->error) return;  // the select failed: nothing is written
    const u64 need = o.meta[0];
    const uint32_t fv = (a.st->answer ^ a.flip) & 0xFFFFu, flip2 = a.flip | a.flip << 16;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const u64 nw = (u64)gridDim.x * (TK_BLOCK / WAVE);
    const u64 pad = ALIGNED ? 0 : a.pad, end = a.n + pad;
    const uint4 *vw = reinterpret_cast<const uint4 *>(reinterpret_cast<uintptr_t>(a.keys) - 2 * pad);
    struct Round {
        int src[TK16W_TILES];  // lane (tile - tg) of each tile, -1 past the last
        uint32_t x[TK16W_TILES][TK16_WPL];
    };
    auto load_round = [&](Round &rd, u64 &todo, u64 tg) {
#pragma unroll
        for (int q = 0; q < TK16W_TILES; ++q) {
            const bool has = todo != 0;  // wave-uniform
            rd.src[q] = has ? __builtin_ctzll(todo) : -1;
            if (has) todo &= todo - 1;
            const u64 tb = (tg + (u64)(has ? rd.src[q] : 0)) * TK16_TILE;
            if (!has) {
#pragma unroll
                for (int j = 0; j < TK16_WPL; ++j) rd.x[q][j] = 0u;
            } else if (tb >= pad && tb + TK16_TILE <= end) {
#pragma unroll
                for (int r = 0; r < TK16_WPL / 4; ++r) {
                    const uint4 v4 = vw[tb / 8 + (u64)lane * (TK16_WPL / 4) + r];
                    rd.x[q][4 * r] = v4.x;
                    rd.x[q][4 * r + 1] = v4.y;
                    rd.x[q][4 * r + 2] = v4.z;
                    rd.x[q][4 * r + 3] = v4.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < TK16_WPL; ++j) {
                    const u64 j0 = tb + (u64)lane * TK16_KPL + 2 * j;
                    const uint32_t k0 = j0 >= pad && j0 < end ? a.keys[j0 - pad] : 0u;
                    const uint32_t k1 = j0 + 1 >= pad && j0 + 1 < end ? a.keys[j0 + 1 - pad] : 0u;
                    rd.x[q][j] = k0 | k1 << 16;
                }
            }
        }
    };
    for (u64 tg = ((u64)blockIdx.x * (TK_BLOCK / WAVE) + w) * WAVE; tg < a.ntiles; tg += nw * WAVE) {
        // lane l: tile tg + l's bases and whether it holds output keys
        const u64 tl = tg + lane;
        uint32_t c_l = 0;
        u64 bb_l = 0, be_l = 0;
        if (tl < a.ntiles) {
            c_l = a.tcnt[tl];
            const u64 off = o.toff[tl], blk = tl / TK_TILES_PER_BLOCK;
            bb_l = o.bbase[2 * blk] + (off & 0xFFFFFFFFull);
            be_l = o.bbase[2 * blk + 1] + (off >> 32);
        }
        const bool act = tk_better_of(c_l) != 0 || (tk_equal_of(c_l) != 0 && be_l < need);
        u64 todo = __ballot(act);
        while (todo) {
            Round cur;
            load_round(cur, todo, tg);
#pragma unroll
            for (int q = 0; q < TK16W_TILES; ++q) {
                const int src = cur.src[q];
                if (src < 0) break;  // wave-uniform
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)c_l, src);
                const u64 bb = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bb_l >> 32), src) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bb_l, src);
                const u64 be = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(be_l >> 32), src) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)be_l, src);
                const u64 ce = tk_equal_of(c);
                const u64 room = be >= need ? 0 : need - be;               // ties this tile may take
                const uint32_t cap = (uint32_t)(room < 0xFFFFu ? room : 0xFFFFu);
                const uint32_t total = tk_better_of(c) + (uint32_t)(room < ce ? room : ce);  // output keys
                const u64 start = bb + (be < need ? be : need);             // and where they go
                const u64 tb = (tg + (u64)src) * TK16_TILE;
                const bool full = tb >= pad && tb + TK16_TILE <= end;       // wave-uniform
                const uint32_t vm = full ? ~0u : tk16_run_mask(tb + (u64)lane * TK16_KPL, pad, end);
                uint32_t mb = 0, me = 0;  // bit j: this lane's key j is better / equal
#pragma unroll
                for (int i = 0; i < TK16_WPL; ++i) {
                    const uint32_t x2 = k16_ord2<CV>(cur.x[q][i], a.nl2, a.top2) ^ flip2;
                    const uint32_t x0 = x2 & 0xFFFFu, x1 = x2 >> 16;
                    mb |= (uint32_t)(x0 < fv) << (2 * i) | (uint32_t)(x1 < fv) << (2 * i + 1);
                    me |= (uint32_t)(x0 == fv) << (2 * i) | (uint32_t)(x1 == fv) << (2 * i + 1);
                }
                mb &= vm;
                me &= vm;
                const uint32_t mine = (uint32_t)__popc(mb) | ((uint32_t)__popc(me) << 16);
                const uint32_t p = wave_incl_scan32(mine) - mine;
                if (mb | me) {
                    uint32_t pb = p & 0xFFFFu, pe = p >> 16;
#pragma unroll
                    for (int j = 0; j < TK16_KPL; ++j) {
                        const uint32_t isb = (mb >> j) & 1u, ise = (me >> j) & 1u;
                        const uint32_t r = pb + min(pe, cap);
                        if (isb | (ise & (uint32_t)(pe < cap))) {
                            const uint32_t bits = (cur.x[q][j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                            s_val[w][r] = (uint16_t)((bits & 0x7FFFu) > o.inf ? o.canon : bits);
                            s_col[w][r] = (uint16_t)(lane * TK16_KPL + j);
                        }
                        pb += isb;
                        pe += ise;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                for (uint32_t r = lane; r < total; r += WAVE) {  // coalesced copy-out
                    if (o.vals) o.vals[start + r] = s_val[w][r];
                    if (o.idx) o.idx[start + r] = (int64_t)(tb + s_col[w][r] - pad);
                }
                __builtin_amdgcn_wave_barrier();  // copy-out reads before the next tile's staging
            }
        }
    }
}

}  // namespace kth
