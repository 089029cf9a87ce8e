// The list kernels of the render path: the KNN's per-survivor flag bytes -> per-part pair lists (k_pair_lists) -> per-part winner
// lists for the colour MLP (k_winner_lists, k_all_lists).  The layout they share is stated in pair_lists.h.
#include "pair_lists.h"

// The per-part pair lists from the flag bytes k_knn_pairs left per survivor: l_slot[p][0..count) = the survivors flagged for
// part p, ASCENDING (a deterministic order: consecutive pairs are neighbours in space, k_cull.hip); neighbours and weights stay
// where the KNN wrote them — at the survivor's slot.  One workgroup per group of PAIR_GROUP slots; its list offsets are the sums
// of the per-group counts the KNN accumulated (gcount) over the groups before it — no atomics here (device-scope atomics on one
// address serialise at tens of ns each on the 8-XCD part: 1167 claims per part cost this kernel 90 us).  The workgroup of the
// last group appends one zero-weight pair per part behind the real ones — its field value is the constant every far pair of
// that part takes (header comment); it lives in the extra slot `cap` — and exports the counters (no extra launches).
#define PL_BLOCK 256
__global__ __launch_bounds__(PL_BLOCK) void k_pair_lists(Workspace w, int32_t* __restrict__ stats) {
    __shared__ int s_cnt[PL_BLOCK / 64][INVR_NUM_PARTS];
    __shared__ int s_red[PL_BLOCK / 64][INVR_NUM_PARTS];
    const int na = w.counters[CNT_ACTIVE];
    const int64_t g = blockIdx.x, g_last = last_group(na);
    if (g > g_last) return;
    // list offsets of this group = counts of the groups before it
    int base[INVR_NUM_PARTS];
    group_bases<PL_BLOCK>(w.gcount, g, s_red, base);
    for (int64_t t0 = g * PAIR_GROUP; t0 < min((g + 1) * (int64_t)PAIR_GROUP, (int64_t)na); t0 += PL_BLOCK * LIST_PER) {
        // thread -> LIST_PER consecutive survivors (one 8-byte load of flag bytes); ranks: inside the thread, the wave, the block
        const int64_t s0 = t0 + (int64_t)threadIdx.x * LIST_PER;
        const unsigned long long fb = load_flags8(w.pflags, s0, na);
        block_rank5<PL_BLOCK>(fb, s_cnt, base, [&](int p, int pos) {
            for (int k = 0; k < LIST_PER; ++k)
                if (bit8(fb, k, p)) w.l_slot[p][pos++] = (int32_t)(s0 + k);
        });
        __syncthreads();                 // s_cnt is reused by the next tile
    }
    if (g != g_last) return;
    // epilogue: base[] = the totals
    if (threadIdx.x < INVR_NUM_PARTS) {
        const int p = threadIdx.x;
        int tot = 0;
#pragma unroll
        for (int q = 0; q < INVR_NUM_PARTS; ++q) if (q == p) tot = base[q];
        const int64_t fs = far_slot(w.cap);
        w.l_slot[p][tot] = (int32_t)fs;
        reinterpret_cast<int4*>(w.l_nn[p])[fs] = make_int4(0, 0, 0, 0);
        reinterpret_cast<float4*>(w.l_w[p])[fs] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.counters[CNT_PAIRS + p] = tot + 1;
        if (p == 0) w.active_idx[fs] = 0;
    }
    __syncthreads();
    if (stats && threadIdx.x < INVR_STATS_LEN) stats[threadIdx.x] = threadIdx.x < CNT_LEN ? w.counters[threadIdx.x] : 0;
}

int launch_pair_lists(const Workspace& w, int32_t* stats, hipStream_t st) {
    hipLaunchKernelGGL(k_pair_lists, dim3((unsigned)w.n_groups), dim3(PL_BLOCK), 0, st, w, stats);
    INVR_LAUNCH_CHECK();
    return 0;
}

// The merge of one survivor = arg-max of the occupancies over the five parts, zeros for unflagged parts, the first maximum wins
// (inb_part_network_multiassign.py:229-256 with cfg.aggr == ""), evaluated here from the phase-1 occupancies; the survivors whose
// winner is a LISTED pair are what the colour MLP still has to see.  One workgroup per group of PAIR_GROUP survivor slots — the
// layout of k_pair_lists: the pairs of group g sit at [off_g, off_g + gcount[g][p]) of part p's list, off_g = the counts of the
// groups before it — which writes its winners, ascending, to wl[p][off_g ...) and their number to wcnt[g][p]: no global offsets,
// no atomics; k_part_rgb_all walks the segments.  The last group appends the far-constant pair of every part.
//
// cfg.aggr == 'mean' (:236-239; InvrScene::aggr = INVR_AGGR_MEAN): the merged raw is the mean over the five parts of (rgb, occ), zeros
// for unflagged parts, so every listed pair needs its colour.  The phases then run as
//   k_part_occ_all -> k_all_lists (wl = identity, wcnt = gcount: every pair "wins") -> k_part_rgb_all ([rgb, occ] per PAIR to
//   feat[p][pair * 4]) -> k_winner_lists<true>: the same rank walk as the arg-max merge, but it sums the listed / far-constant
//   values of a survivor in part order, divides by 5 and writes rgbw[slot] (wsel = 0: "read rgbw[slot]").
#define WL_BLOCK 512         // x LIST_PER = PAIR_GROUP: one pass per group (the kernel is a chain of dependent round trips)
static_assert(WL_BLOCK * LIST_PER == PAIR_GROUP, "k_winner_lists walks a group in one pass");
// cfg.aggr == 'dist' (:240-244, MODE 2): the 'mean' flow with the parts weighted by F.normalize(1 / (part_dist + 1e-5)) (L2 over the five
// parts, eps 1e-12) instead of 1 / 5 — part_dist of every (slot, part) from k_knn_pdist.  cfg.aggr == 'mindist' (:245-251, MODE 3): the
// arg-max flow with the winner = the part of smallest part_dist (first minimum), whatever its occupancy — its listed pair, its far
// constant, or zeros when that part is not flagged for the survivor.
template <int MODE>          // 0 = max occupancy, 1 = mean, 2 = dist, 3 = mindist (InvrScene::aggr)
__global__ __launch_bounds__(WL_BLOCK) void k_winner_lists(Workspace w) {
    constexpr bool MEAN = MODE == 1 || MODE == 2;
    __shared__ int s_cnt[WL_BLOCK / 64][INVR_NUM_PARTS];
    __shared__ int s_red[WL_BLOCK / 64][INVR_NUM_PARTS];
    const int na = w.counters[CNT_ACTIVE];
    const int64_t g = blockIdx.x, g_last = last_group(na);
    if (g > g_last) return;
    int base[INVR_NUM_PARTS], wbase[INVR_NUM_PARTS], cidx[INVR_NUM_PARTS];
    group_bases<WL_BLOCK>(w.gcount, g, s_red, base);
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        wbase[p] = 0;                                          // winners of this group so far
        cidx[p] = far_list_index(w.counters, p);
    }
    const int pbase0[INVR_NUM_PARTS] = {base[0], base[1], base[2], base[3], base[4]};
    for (int64_t t0 = g * PAIR_GROUP; t0 < min((g + 1) * (int64_t)PAIR_GROUP, (int64_t)na); t0 += WL_BLOCK * LIST_PER) {
        const int64_t s0 = t0 + (int64_t)threadIdx.x * LIST_PER;
        unsigned long long fbs[2];
        load_flags8<2>({w.pflags, w.farflags}, s0, na, fbs);
        const unsigned long long fb = fbs[0], ffb = fbs[1];
        // list index of this thread's first pair of every part
        int pos[INVR_NUM_PARTS];
        block_rank5<WL_BLOCK>(fb, s_cnt, base, [&](int p, int q) { pos[p] = q; });
        __syncthreads();                 // s_cnt is reused below
        // the merge of the thread's LIST_PER survivors.  All occupancies are fetched first, unconditionally (an unflagged / far
        // (survivor, part) reads the part's far constant): loads under per-part conditions would be 40 serial round trips
        unsigned long long wb = 0ull, sel8 = 0ull;
        int widx[LIST_PER], pidx[LIST_PER][INVR_NUM_PARTS];
        float oc[LIST_PER][INVR_NUM_PARTS];
#pragma unroll
        for (int k = 0; k < LIST_PER; ++k)
#pragma unroll
            for (int p = 0; p < INVR_NUM_PARTS; ++p) {
                const bool listed = bit8(fb, k, p);
                pidx[k][p] = listed ? pos[p] : cidx[p];
                pos[p] += listed ? 1 : 0;
            }
        if (MEAN) {
            // raws.mean(dim=1) over (Na, P, 4) with zeros for unflagged parts: the per-pair values in part order, / P
#pragma unroll 2
            for (int k = 0; k < LIST_PER; ++k) {
                const unsigned fl = (unsigned)(fb >> (8 * k)) & 0xffu, ff = (unsigned)(ffb >> (8 * k)) & 0xffu;
                float4 v[INVR_NUM_PARTS];
#pragma unroll
                for (int p = 0; p < INVR_NUM_PARTS; ++p) v[p] = w.feat[p][(int64_t)pidx[k][p] * 4];      // (unflagged: the part's far constant, dropped below)
                float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
                if (MODE == 2) {
                    // torch.sum(raws * F.normalize(1.0 / (part_dist + 1e-5), dim=-1)[..., None], dim=1)
                    float wgt[INVR_NUM_PARTS];
                    const int64_t sl = min(s0 + k, (int64_t)na - 1);
                    dist_weights(w.pdist + sl * INVR_NUM_PARTS, wgt);
#pragma unroll
                    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
                        const float wp = wgt[p];
                        if ((fl | ff) & (1u << p)) { sum.x += v[p].x * wp; sum.y += v[p].y * wp; sum.z += v[p].z * wp; sum.w += v[p].w * wp; }
                    }
                    if (s0 + k < na) {
                        w.rgbw[s0 + k] = sum;
                        w.wsel[s0 + k] = ((fl | ff) & 0x1fu) ? (uint8_t)WSEL_MERGED : (uint8_t)WSEL_NONE;
                    }
                    continue;
                }
#pragma unroll
                for (int p = 0; p < INVR_NUM_PARTS; ++p)
                    if ((fl | ff) & (1u << p)) { sum.x += v[p].x; sum.y += v[p].y; sum.z += v[p].z; sum.w += v[p].w; }
                const float np = (float)INVR_NUM_PARTS;
                if (s0 + k < na) {
                    w.rgbw[s0 + k] = make_float4(sum.x / np, sum.y / np, sum.z / np, sum.w / np);
                    w.wsel[s0 + k] = ((fl | ff) & 0x1fu) ? (uint8_t)WSEL_MERGED : (uint8_t)WSEL_NONE;
                }
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < LIST_PER; ++k)
#pragma unroll
            for (int p = 0; p < INVR_NUM_PARTS; ++p) oc[k][p] = w.occp[p][pidx[k][p]];
#pragma unroll
        for (int k = 0; k < LIST_PER; ++k) {
            const unsigned fl = (unsigned)(fb >> (8 * k)) & 0xffu, ff = (unsigned)(ffb >> (8 * k)) & 0xffu;
            float best = 0.0f;
            unsigned bsel = WSEL_NONE;
            int bidx = 0;
            if (MODE == 3) {
                // part_dist.argmin(dim=1): the first minimum (a NaN, from a part with fewer than 4 vertices, wins as in torch)
                const int64_t sl = min(s0 + k, (int64_t)na - 1);
                int bp = 0;
                float bd = w.pdist[sl * INVR_NUM_PARTS];
#pragma unroll
                for (int p = 1; p < INVR_NUM_PARTS; ++p) {
                    const float d = w.pdist[sl * INVR_NUM_PARTS + p];
                    if (!(bd != bd) && (d < bd || d != d)) { bd = d; bp = p; }
                }
#pragma unroll
                for (int p = 0; p < INVR_NUM_PARTS; ++p)
                    if (p == bp) {
                        if (fl & (1u << p)) bsel = wsel_listed(p);
                        else if (ff & (1u << p)) bsel = wsel_far(p);
                        bidx = pidx[k][p];
                    }
            } else {
#pragma unroll
                for (int p = 0; p < INVR_NUM_PARTS; ++p) {
                    float c = 0.0f;
                    unsigned sel = WSEL_NONE;
                    if (fl & (1u << p)) { c = oc[k][p]; sel = wsel_listed(p); }
                    else if (ff & (1u << p)) { c = oc[k][p]; sel = wsel_far(p); }
                    if (p == 0 || c > best) { best = c; bsel = sel; bidx = pidx[k][p]; }
                }
            }
            widx[k] = bidx;
            sel8 |= (unsigned long long)bsel << (8 * k);
            if (wsel_is_listed(bsel)) wb |= 1ull << (8 * k + bsel);
        }
        store_bytes8(w.wsel, s0, na, sel8);
        // winner ranks, then the lists
        block_rank5<WL_BLOCK>(wb, s_cnt, wbase, [&](int p, int q) {
            q += pbase0[p];
#pragma unroll
            for (int k = 0; k < LIST_PER; ++k)
                if (bit8(wb, k, p)) w.wl[p][q++] = widx[k];
        });
        __syncthreads();                 // s_cnt is reused by the next tile
    }
    if (!MEAN && threadIdx.x < INVR_NUM_PARTS) {
        const int p = threadIdx.x;
        int nw = 0, off = 0, ci = 0;
#pragma unroll
        for (int q = 0; q < INVR_NUM_PARTS; ++q) if (q == p) { nw = wbase[q]; off = pbase0[q]; ci = cidx[q]; }
        if (g == g_last) w.wl[p][off + nw++] = ci;               // the far-constant pair: always evaluated
        w.wcnt[group_row(g, p)] = nw;
    }
}

int launch_winner_lists(const Workspace& w, int aggr, hipStream_t st) {
    const dim3 grid((unsigned)w.n_groups), block(WL_BLOCK);
    switch (aggr) {
        case INVR_AGGR_MEAN: hipLaunchKernelGGL(k_winner_lists<1>, grid, block, 0, st, w); break;
        case INVR_AGGR_DIST: hipLaunchKernelGGL(k_winner_lists<2>, grid, block, 0, st, w); break;
        case INVR_AGGR_MINDIST: hipLaunchKernelGGL(k_winner_lists<3>, grid, block, 0, st, w); break;
        default: hipLaunchKernelGGL(k_winner_lists<0>, grid, block, 0, st, w); break;
    }
    INVR_LAUNCH_CHECK();
    return 0;
}

// cfg.aggr == 'mean': every listed pair (and the far-constant pair that ends a part's list) goes through the colour MLP.
__global__ __launch_bounds__(256) void k_all_lists(Workspace w) {
    const int na = w.counters[CNT_ACTIVE];
    const int g_last = last_group(na);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        const int n = w.counters[CNT_PAIRS + p];
        for (int64_t i = t; i < n; i += nt) w.wl[p][i] = (int)i;
    }
    for (int64_t i = t; i < group_row(g_last + 1, 0); i += nt)
        w.wcnt[i] = w.gcount[i] + (i / INVR_NUM_PARTS == g_last ? 1 : 0);
}

int launch_all_lists(const Workspace& w, hipStream_t st) {
    int64_t lt = cdiv(w.lcap, 256);
    hipLaunchKernelGGL(k_all_lists, dim3((unsigned)(lt < 1024 ? (lt > 0 ? lt : 1) : 1024)), dim3(256), 0, st, w);
    INVR_LAUNCH_CHECK();
    return 0;
}
