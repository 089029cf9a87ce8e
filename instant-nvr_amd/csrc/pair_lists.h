// The layout of the per-part pair lists and winner lists, stated once for every kernel that produces or consumes them
// (k_lists.hip: k_pair_lists, k_winner_lists, k_all_lists; k_mlp.hip: k_part_rgb_all; k_composite.hip: MergedRaw; k_train.hip: k_merge_bwd).
//
//  * The survivor slots are cut into groups of PAIR_GROUP.  gcount[g][p] = the pairs of part p flagged in group g (the KNN counts them),
//    wcnt[g][p] = the winners among them.  The pairs of group g sit at [off_g, off_g + gcount[g][p]) of part p's list, off_g = the sum of
//    the gcount rows before g; its winners at wl[p][off_g ...), wcnt[g][p] of them.  No global offsets, no atomics.
//  * Inside a group a pair's position is its rank: inside the thread's 8 flag bytes, then the wave, then the workgroup — ascending slots.
//  * wsel[slot] says where the merged value of a survivor lives (the WSEL_ code below).
//  * Every part's list ends with one far-constant pair (far_* below).
#pragma once
#include "pipeline.h"

// ---- group geometry ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int last_group(int na) { return (max(na, 1) - 1) / PAIR_GROUP; }                  // the group of the last survivor (0 for an empty frame)
__device__ __forceinline__ int64_t group_row(int64_t g, int p) { return g * INVR_NUM_PARTS + p; }            // gcount / wcnt: [g][p]

// List offsets of group g = the sums of the gcount rows before it.  s_red: [BLOCK / 64][INVR_NUM_PARTS] ints of LDS.
// Contains ONE barrier: every thread of the workgroup must call it.
template <int BLOCK>
__device__ __forceinline__ void group_bases(const int32_t* gcount, int64_t g, int (*s_red)[INVR_NUM_PARTS], int* base) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int acc[INVR_NUM_PARTS] = {0, 0, 0, 0, 0};
    for (int64_t q = threadIdx.x; q < g; q += BLOCK)
#pragma unroll
        for (int p = 0; p < INVR_NUM_PARTS; ++p) acc[p] += gcount[group_row(q, p)];
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        acc[p] = __builtin_amdgcn_readlane(wave_incl_sum_i(acc[p]), 63);
        if (lane == 0) s_red[wv][p] = acc[p];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        base[p] = 0;
        for (int k = 0; k < BLOCK / 64; ++k) base[p] += s_red[k][p];
    }
}

// ---- a thread's 8 consecutive survivors: one byte each, byte k = slot s0 + k --------------------------------------------------
#define LIST_PER 8
// N byte arrays at once (the flag bytes and the far-flag bytes of the same survivors): one 8-byte load each, or the byte-wise ragged tail.
// The tail walks the arrays TOGETHER, byte by byte, as k_winner_lists always did: with one tail loop per array its 'mean' / 'dist' forms
// need 66 VGPRs instead of 62 and lose a wave of occupancy.
template <int N>
__device__ __forceinline__ void load_flags8(const uint8_t* const (&bytes)[N], int64_t s0, int na, unsigned long long (&out)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = 0ull;
    if (s0 + LIST_PER <= na) {
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = *reinterpret_cast<const unsigned long long*>(bytes[j] + s0);
    } else
        for (int k = 0; k < LIST_PER; ++k)
            if (s0 + k < na)
#pragma unroll
                for (int j = 0; j < N; ++j) out[j] |= (unsigned long long)bytes[j][s0 + k] << (8 * k);
}
__device__ __forceinline__ unsigned long long load_flags8(const uint8_t* bytes, int64_t s0, int na) {          // one array
    unsigned long long out[1];
    load_flags8<1>({bytes}, s0, na, out);
    return out[0];
}
__device__ __forceinline__ void store_bytes8(uint8_t* bytes, int64_t s0, int na, unsigned long long v) {
    if (s0 + LIST_PER <= na) *reinterpret_cast<unsigned long long*>(bytes + s0) = v;
    else for (int k = 0; k < LIST_PER; ++k) if (s0 + k < na) bytes[s0 + k] = (uint8_t)(v >> (8 * k));
}
__device__ __forceinline__ bool bit8(unsigned long long bits, int k, int p) { return (bits >> (8 * k + p)) & 1ull; }   // bit p of byte k

// The rank walk: for every part p, in part order, use(p, pos) with pos = the list position (relative to the group's offset when
// running[] starts at 0) of the thread's FIRST set bit p of `bits`; the thread's further bits p follow at pos + 1, ... in byte
// order.  running[p] advances by the workgroup's count.  s_cnt: [BLOCK / 64][INVR_NUM_PARTS] ints of LDS.  Contains ONE barrier
// (between the s_cnt write and read): every thread of the workgroup must call it, and the CALLER places a barrier before s_cnt is
// written again (the next call).
template <int BLOCK, class Use>
__device__ __forceinline__ void block_rank5(unsigned long long bits, int (*s_cnt)[INVR_NUM_PARTS], int* running, Use use) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int pre[INVR_NUM_PARTS];
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        const int mine = __popcll(bits & (0x0101010101010101ull << p));
        const int x = wave_incl_sum_i(mine);
        pre[p] = x - mine;
        if (lane == 63) s_cnt[wv][p] = x;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        int pos = running[p] + pre[p];
        for (int k = 0; k < BLOCK / 64; ++k) { const int c = s_cnt[k][p]; if (k < wv) pos += c; running[p] += c; }
        use(p, pos);
    }
}

// ---- wsel: the merge's choice per survivor ---------------------------------------------------------------------------------
// p = the listed pair of part p wins (its value is at rgbw[slot]); WSEL_FAR + p = the far constant of part p wins; WSEL_NONE = zeros
// (no flagged part, or an unflagged part 0 ties at 0).  The sum flows ('mean', 'dist') leave the merged value itself at rgbw[slot]
// and mark it WSEL_MERGED, which reads as "listed".
#define WSEL_FAR 8u
#define WSEL_NONE 255u
#define WSEL_MERGED 0u
__device__ __forceinline__ unsigned wsel_listed(int p) { return (unsigned)p; }
__device__ __forceinline__ unsigned wsel_far(int p) { return WSEL_FAR + (unsigned)p; }
__device__ __forceinline__ bool wsel_is_listed(unsigned sel) { return sel < (unsigned)INVR_NUM_PARTS; }
__device__ __forceinline__ bool wsel_is_far(unsigned sel) { return sel >= WSEL_FAR && sel < 2u * WSEL_FAR; }
__device__ __forceinline__ bool wsel_is_none(unsigned sel) { return sel >= 2u * WSEL_FAR; }
__device__ __forceinline__ unsigned wsel_far_part(unsigned sel) { return sel - WSEL_FAR; }                  // the part of a far code

// ---- the far constant of part p ------------------------------------------------------------------------------------------------
// Every far pair of a part takes one value: the field at zero weights.  It is evaluated once per frame as the LAST entry of the part's
// list (k_pair_lists appends it), whose survivor slot is the extra slot `cap` behind the real ones (cap = Workspace::cap, the largest
// number of survivors; per-slot arrays and lists hold lcap = cap + 1 entries), and its [rgb, occ] lands behind the per-slot results.
// MlpAllArgs::cap is lcap: k_part_rgb_all passes a.cap - 1 here.
__device__ __forceinline__ int far_list_index(const int32_t* counters, int p) { return counters[CNT_PAIRS + p] - 1; }
__device__ __forceinline__ int64_t far_slot(int64_t cap) { return cap; }
__device__ __forceinline__ int64_t far_result_index(int64_t cap, int64_t p) { return cap + 1 + p; }                 // in rgbw

// ---- cfg.aggr == 'dist': torch F.normalize(1.0 / (part_dist + 1e-5), dim=-1) over the five parts (L2, eps 1e-12) ----------------
__device__ __forceinline__ void dist_weights(const float* pdist_row, float* wgt) {
    float n2 = 0.0f;
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) { wgt[p] = 1.0f / (pdist_row[p] + 1e-5f); n2 += wgt[p] * wgt[p]; }
    const float den = fmaxf(sqrtf(n2), 1e-12f);
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) wgt[p] = wgt[p] / den;
}

// ---- the consumer side: a wave walks the winner tiles of one part ------------------------------------------------------------------
// A wave's unit of work is a tile of 32 winners (two 16-pair column blocks) of ONE segment (slot group); tile t of a
// part -> (segment, offset) through a wave-cooperative cursor: 64 segments per window (lane = segment), tile / pair prefix sums
// by wave scans, the window advanced as the wave's tile index grows — no per-part scan kernel, no LDS, any number of groups.
struct SegCursor {
    int g0, tiles_before, pairs_before;      // window start; tiles / pairs of the segments before it
    int wc, tl, ti, pe;                      // this lane's segment: winners, tiles, inclusive tile prefix, exclusive pair prefix
    int win_tiles, win_pairs;
};
__device__ __forceinline__ void seg_window(SegCursor& c, const int32_t* __restrict__ wcnt, const int32_t* __restrict__ gcount,
                                           int part, int g_last, int lane) {
    const int gi = c.g0 + lane;
    const bool ok = gi <= g_last;
    c.wc = ok ? wcnt[group_row(gi, part)] : 0;
    const int gc = ok ? gcount[group_row(gi, part)] : 0;
    c.tl = (c.wc + 31) >> 5;
    const int x = wave_incl_sum_i(c.tl), y = wave_incl_sum_i(gc);
    c.ti = x; c.pe = y - gc;
    c.win_tiles = __shfl(x, 63); c.win_pairs = __shfl(y, 63);
}
// -> first tile of the segment that holds tile T, the segment's offset in the lists and its winner count
__device__ __forceinline__ void seg_locate(SegCursor& c, int T, const int32_t* __restrict__ wcnt, const int32_t* __restrict__ gcount,
                                           int part, int g_last, int lane, int& seg_tile0, int& sb, int& sn) {
    while (T >= c.tiles_before + c.win_tiles && c.g0 + 64 <= g_last) {
        c.tiles_before += c.win_tiles; c.pairs_before += c.win_pairs; c.g0 += 64;
        seg_window(c, wcnt, gcount, part, g_last, lane);
    }
    const unsigned long long m = __ballot(c.tiles_before + c.ti > T);
    const int L = m ? __ffsll((long long)m) - 1 : 63;
    seg_tile0 = c.tiles_before + __shfl(c.ti - c.tl, L);
    sb = c.pairs_before + __shfl(c.pe, L);
    sn = __shfl(c.wc, L);
}
