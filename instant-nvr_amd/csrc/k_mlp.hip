// K6: the two tiny Softplus MLPs of one body part on the matrix cores.
// Replaces part_base_network.Network.forward after the encoder (part_base_network.py:44-63):
//   h   = occMLP(emb19)            19 -> 64 -> 17          (Softplus between linears)
//   occ = 1 - exp(-softplus(h[0])) ; feat = h[1:17]
//   rgb = sigmoid(rgbMLP([emb19, dirPE27, feat16, latent8]))   70 -> 64 (-> 64) -> 3
//
// fp32 parity (1e-4 per pixel) rules out plain bf16/fp16 MFMA inputs.  The occupancy MLP's layers run on
// v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains, MI355X_MICROARCH "Matrix cores"); the colour MLP's two 64-wide
// layers run on v_mfma_f32_16x16x32_bf16 as exact 3-way bf16 splits of weights and activations (six products per
// tile with fp32 accumulation: fp32 accuracy at 0.58x the time, see mlp_common.h).
// Orientation: D^T = W . X^T — weights are the A operand (M = 16 output features per tile),
// 16 (point,part) pairs are the N columns.  With that orientation the accumulator registers of
// one layer ARE the B operands of the next (lane group g = lane>>4 holds features 16*mt+4g+r of
// pair lane&15 in register r), provided the next layer's weights are stored in the matching
// K order — so activations never leave registers between layers.  Weights are re-ordered into
// that per-(k-step, m-tile, lane) order while they are staged into LDS (59 KB per part).
// The 1-wide / 3-wide heads (occupancy logit, rgb out) are 16-term VALU dot products plus two
// cross-lane adds instead of wasting 15/16 of an MFMA tile.
#include "pipeline.h"

#include "mlp_common.h"
#include "pair_lists.h"

// One 16-pair column block of a wave: inputs, activations and outputs stay in registers from the embedding to [rgb, occ].
struct MlpCol {
    float eb[EMB_STEPS];        // k-slots 4s+g of the (padded) 20-wide embedding of pair `col`
    float dv[3];                // canonical view direction
    f32x4 h[4];                 // hidden activations (log2 domain), feature 16 mt + 4 g + r
    f32x4 feat;                 // occ features 1..16 (true scale)
    float occ;
    float k5[11];               // rgb layer-1 k-slots 5..15: sin/cos (6), d (1), feat (4)
    mlp_bf16x8 sh[2], sm[2], sl[2];   // the 16 inputs of the next 64-wide layer (k-slots s = 8 kb + j) as bf16 hi / mid / lo terms
};

// One 64 -> 64 (or 64-slot -> 64) layer of a column block on the bf16 matrix pipe: six products per (m-tile, k-block), smallest first.
__device__ __forceinline__ void bf16x3_layer(const float* lds_w, const float* lds_b, int lane, int g, const MlpCol& c, f32x4* out) {
    const mlp_bf16x8* w = reinterpret_cast<const mlp_bf16x8*>(lds_w);
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) {
        out[mo] = bias4(lds_b, mo, g);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const mlp_bf16x8 ah = w[(0 * 8 + mo * 2 + kb) * 64 + lane], am = w[(1 * 8 + mo * 2 + kb) * 64 + lane], al = w[(2 * 8 + mo * 2 + kb) * 64 + lane];
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, c.sm[kb], out[mo], 0, 0, 0);
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, c.sl[kb], out[mo], 0, 0, 0);
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, c.sh[kb], out[mo], 0, 0, 0);
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, c.sm[kb], out[mo], 0, 0, 0);
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, c.sh[kb], out[mo], 0, 0, 0);
            out[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, c.sh[kb], out[mo], 0, 0, 0);
        }
    }
}
// the hidden activations c.h (k-slot s <-> h[s >> 2][s & 3]) as the split inputs of the next layer
__device__ __forceinline__ void bf16x3_split_h(MlpCol& c) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c.h[2 * kb + (j >> 2)][j & 3];
        bf16_split3x8(v, c.sh[kb], c.sm[kb], c.sl[kb]);
    }
}

// The stages of the two MLPs for ONE column block.  mlp_part runs two column blocks per wave SKEWED by one stage, so that in
// every scheduling region the matrix-core instructions of one block sit beside the vector instructions (activation, view-
// direction encoding, heads) of the other: a SIMD issues VALU in the shadow of a 32-cycle fp32 MFMA only if independent VALU
// work is available at that point of the (in-order) wave.
__device__ __forceinline__ void st_occ1(const float* lds, int lane, int g, MlpCol& c) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) c.h[mt] = bias4(lds + O_B_OCC1, mt, g);
#pragma unroll
    for (int s = 0; s < EMB_STEPS; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(lds + O_W_OCC1 + (s * 64 + lane) * 4);
        c.h[0] = mfma4(a.x, c.eb[s], c.h[0]); c.h[1] = mfma4(a.y, c.eb[s], c.h[1]);
        c.h[2] = mfma4(a.z, c.eb[s], c.h[2]); c.h[3] = mfma4(a.w, c.eb[s], c.h[3]);
    }
}
__device__ __forceinline__ void st_act(MlpCol& c) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) c.h[mt] = softplus4_log2(c.h[mt]);
}
// activation of a colour-MLP layer whose output feeds another 64-wide layer (rgb1 of the three-layer nets): + the bf16 split
__device__ __forceinline__ void st_act_split(MlpCol& c) {
    st_act(c);
    bf16x3_split_h(c);
}
__device__ __forceinline__ void st_occ2(const float* lds, int lane, int g, MlpCol& c) {       // features 1..16 on MFMA, logit 0 on VALU
    c.feat = bias4(lds + O_B_OCC2, 0, g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 a = *reinterpret_cast<const float4*>(lds + O_W_OCC2 + (q * 64 + lane) * 4);
        c.feat = mfma4(a.x, c.h[q][0], c.feat); c.feat = mfma4(a.y, c.h[q][1], c.feat);
        c.feat = mfma4(a.z, c.h[q][2], c.feat); c.feat = mfma4(a.w, c.h[q][3], c.feat);
    }
    const float lg = head_dot_s(c.h, lds + O_V_OCC, g) + lds[O_V_OCC + 64];
    c.occ = one_minus_exp_neg(softplus_f(lg));                    // 1 - exp(-softplus(h0))  (:52)
}
__device__ __forceinline__ void st_rgb_in(MlpCol& c, int g, float fmul) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float sn, cs;
        sincos_hw(c.dv[k] * fmul, &sn, &cs);
        c.k5[2 * k] = sn;
        c.k5[2 * k + 1] = cs;
    }
    c.k5[6] = g == 0 ? c.dv[0] : (g == 1 ? c.dv[1] : (g == 2 ? c.dv[2] : 0.0f));
#pragma unroll
    for (int r = 0; r < 4; ++r) c.k5[7 + r] = c.feat[r];
    // the 16 k-slots of rgb layer 1 (s < 5: embedding, s >= 5: k5) as split bf16 inputs
    float v0[8] = {c.eb[0], c.eb[1], c.eb[2], c.eb[3], c.eb[4], c.k5[0], c.k5[1], c.k5[2]};
    float v1[8] = {c.k5[3], c.k5[4], c.k5[5], c.k5[6], c.k5[7], c.k5[8], c.k5[9], c.k5[10]};
    bf16_split3x8(v0, c.sh[0], c.sm[0], c.sl[0]);
    bf16_split3x8(v1, c.sh[1], c.sm[1], c.sl[1]);
}
__device__ __forceinline__ void st_rgb1(const float* lds, int lane, int g, MlpCol& c) {
    bf16x3_layer(lds + O_W_RGB1, lds + O_B_RGB1, lane, g, c, c.h);
}
__device__ __forceinline__ void st_rgb2(const float* lds, int lane, int g, MlpCol& c) {
    f32x4 o[4];
    bf16x3_layer(lds + O_W_RGB2, lds + O_B_RGB2, lane, g, c, o);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) c.h[mt] = o[mt];
}
__device__ __forceinline__ float4 st_head(const float* lds, int g, const MlpCol& c) {          // rgb head 64 -> 3, sigmoid
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = sigmoid_f(head_dot_s(c.h, lds + O_V_OUT + k * 64, g) + lds[O_V_OUT + 3 * 64 + k]);
    return make_float4(o[0], o[1], o[2], c.occ);
}
#define MLP_FENCE() __builtin_amdgcn_sched_barrier(0)
// matrix / vector instruction mix of the colour-MLP regions below (bf16 x 3: 48 MFMAs of 16 cycles + the split of the next inputs)
#define RGB_MFMAS 48
#define RGB_V 3
// Interleave directive for one scheduling region (between two MLP_FENCEs): N_MFMA groups of {1 matrix instruction, V vector
// instructions} — the vector work of the other column block is issued in the shadows of this block's MFMAs (<= 5 single-issue
// VALU fit beside a 32-cycle fp32 MFMA; MI355X_MICROARCH.md).  LDS reads of the weights float freely.
template <int N_MFMA, int V>
__device__ __forceinline__ void mlp_interleave() {
#pragma unroll
    for (int i = 0; i < N_MFMA; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, V, 0);      // VALU
    }
}

// The skewed two-column schedule, stated once: each region between two MLP_FENCEs pairs the matrix work of one column block with the
// vector work of the other.  occ_stages: 19 -> 64 -> 17 of A and B.  RGB_FOLLOWS (the one-kernel form): the last region, B's second
// layer, also forms A's colour inputs; the occupancy phase alone closes it with B's MFMAs only.
template <bool RGB_FOLLOWS>
__device__ __forceinline__ void occ_stages(const float* lds, int lane, int g, float fmul, MlpCol& A, MlpCol& B) {
    st_occ1(lds, lane, g, A);
    MLP_FENCE();
    st_occ1(lds, lane, g, B); st_act(A);
    mlp_interleave<20, 4>();
    MLP_FENCE();
    st_occ2(lds, lane, g, A); st_act(B);
    mlp_interleave<16, 5>();
    MLP_FENCE();
    st_occ2(lds, lane, g, B);
    if (RGB_FOLLOWS) { st_rgb_in(A, g, fmul); mlp_interleave<16, 4>(); }
    MLP_FENCE();
}
// rgb_stages: 70 -> 64 (-> 64) -> 3 of A and B from their embedding, view direction, features and occupancy -> [rgb, occ].
// A_READY: A's colour inputs were formed by occ_stages<true>; the colour phase alone forms them in a region of their own.
template <int NRGB, bool A_READY>
__device__ __forceinline__ void rgb_stages(const float* lds, int lane, int g, float fmul, MlpCol& A, MlpCol& B, float4& rA, float4& rB) {
    if (!A_READY) { st_rgb_in(A, g, fmul); MLP_FENCE(); }
    st_rgb1(lds, lane, g, A); st_rgb_in(B, g, fmul);
    mlp_interleave<RGB_MFMAS, RGB_V>();
    MLP_FENCE();
    st_rgb1(lds, lane, g, B);
    if (NRGB == 3) st_act_split(A); else st_act(A);
    mlp_interleave<RGB_MFMAS, RGB_V>();
    MLP_FENCE();
    if (NRGB == 3) {
        st_rgb2(lds, lane, g, A); st_act_split(B);
        mlp_interleave<RGB_MFMAS, RGB_V>();
        MLP_FENCE();
        st_rgb2(lds, lane, g, B); st_act(A);
        mlp_interleave<RGB_MFMAS, 1>();
        MLP_FENCE();
    }
    rA = st_head(lds, g, A); st_act(B);
    MLP_FENCE();
    rB = st_head(lds, g, B);
}
// a column block takes the (pre-loaded) inputs of its next pair
template <bool DIRS>
__device__ __forceinline__ void set_in(MlpCol& c, const MlpIn& in) {
#pragma unroll
    for (int s = 0; s < EMB_STEPS; ++s) c.eb[s] = in.eb[s];
    if (DIRS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.dv[k] = in.dv[k];
    }
}

template <int NRGB>
__device__ __forceinline__ void mlp_part(float* lds, const PartMlpDev& pm, const float* __restrict__ emb,
                                         const float* __restrict__ ds, int64_t stride,
                                         int cnt, int64_t cap, float4* __restrict__ raw_direct, const int vblock, const int nblocks) {
    if ((int64_t)vblock * MLP_PAIRS_PER_WG >= cnt) return;
    __syncthreads();                                   // previous part's weights no longer in use
    stage_weights<NRGB, true>(pm, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const float fmul = (float)(1 << g);                          // frequency 2^g of this lane group

    const int64_t per_block = MLP_PAIRS_PER_WG, step = (int64_t)nblocks * per_block;
    auto load_in = [&](int64_t wbase, MlpIn (&in)[2]) {
        load_mlp_in<true>(in, emb, cap, ds, stride, {min(wbase + col, (int64_t)cnt - 1), min(wbase + 16 + col, (int64_t)cnt - 1)}, g);
    };
    int64_t wbase = (int64_t)vblock * per_block + (int64_t)wv * MLP_CB * 16;
    if (wbase >= cnt) return;
    MlpCol A, B;
    MlpIn nx[2];                                       // inputs of the NEXT tile: loaded a whole tile ahead
    load_in(wbase, nx);
    set_in<true>(A, nx[0]); set_in<true>(B, nx[1]);
    for (; wbase < cnt; wbase += step) {
        load_in(min(wbase + step, (int64_t)cnt - 1), nx);                 // (clamped: the values are unused past the last tile)
        occ_stages<true>(lds, lane, g, fmul, A, B);
        float4 rA, rB;
        rgb_stages<NRGB, true>(lds, lane, g, fmul, A, B, rA, rB);
        const int64_t pa = wbase + col, pb = wbase + 16 + col;
        if (g == 0) {
            if (pa < cnt) raw_direct[pa] = rA;
            if (pb < cnt) raw_direct[pb] = rB;
        }
        set_in<true>(A, nx[0]); set_in<true>(B, nx[1]);
    }
}


// One part's MLPs over a dense pair list, every pair fully evaluated: the stage-level entry points (invr_part_field_fwd /
// invr_part_mlp_fwd).  The render path runs the two phases below instead.
template <int NRGB>
__global__ __launch_bounds__(MLP_BLOCK, 3) void k_part_mlp(PartMlpDev pm, const float* __restrict__ emb,
                                                        const float* __restrict__ ds, int64_t stride,
                                                        const int32_t* __restrict__ count, int64_t cap,
                                                        float4* __restrict__ raw_direct) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    mlp_part<NRGB>(lds, pm, emb, ds, stride, *count, cap, raw_direct, (int)blockIdx.x, (int)gridDim.x);
}

// ---- render path -------------------------------------------------------------------------------------------------------
// TPoseHuman.forward keeps, per survivor, only the raw of the part with the largest occupancy (first maximum;
// inb_part_network_multiassign.py:253-256): the colour MLP of every other evaluated pair is dead work — 17.5 k (body, head) /
// 9.3 k (leg, arms) of a pair's 22.1 k / 14.0 kFLOP, for 49 % of the pairs of the bench frame.  So the part MLPs run in two
// phases with identical results:
//   k_part_occ_all    every listed pair: 19 -> 64 -> 17, occupancy to occp[p][pair], the 16 geometry features to feat[p][pair]
//   k_winner_lists    (k_lists.hip) per survivor the arg-max over {listed occupancies, far constants, 0 for unflagged parts} -> wsel[slot];
//                     the winning LISTED pairs (+ the far-constant pair of every part) as per-part lists, segmented by slot group
//   k_part_rgb_all    70 -> 64 (-> 64) -> 3 on the winners only; [rgb, occ] to rgbw[slot] (far constants: rgbw[lcap + p])
// A pair's arithmetic does not depend on its column or tile, so both phases reproduce the one-kernel results bit for bit.

#define OCC_LDS_FLOATS O_W_RGB1
__device__ __forceinline__ void occ_part(float* lds, const PartMlpDev& pm, const float* __restrict__ emb, int cnt, int64_t cap,
                                         float* __restrict__ occp, float4* __restrict__ feat, const int vblock, const int nblocks) {
    const int64_t per_block = MLP_PAIRS_PER_WG, step = (int64_t)nblocks * per_block;
    if ((int64_t)vblock * per_block >= cnt) return;
    __syncthreads();                                   // previous part's weights no longer in use
    stage_weights<2, true, 1>(pm, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    auto load_in = [&](int64_t wbase, MlpIn (&in)[2]) {
        load_mlp_in<false>(in, emb, cap, nullptr, 0, {min(wbase + col, (int64_t)cnt - 1), min(wbase + 16 + col, (int64_t)cnt - 1)}, g);
    };
    int64_t wbase = (int64_t)vblock * per_block + (int64_t)wv * MLP_CB * 16;
    if (wbase >= cnt) return;
    MlpCol A, B;
    MlpIn nx[2];                                       // inputs of the NEXT tile: loaded a whole tile ahead
    load_in(wbase, nx);
    set_in<false>(A, nx[0]); set_in<false>(B, nx[1]);
    for (; wbase < cnt; wbase += step) {
        load_in(min(wbase + step, (int64_t)cnt - 1), nx);
        occ_stages<false>(lds, lane, g, 0.0f, A, B);
        const int64_t pa = wbase + col, pb = wbase + 16 + col;
        if (pa < cnt) { feat[pa * 4 + g] = make_float4(A.feat[0], A.feat[1], A.feat[2], A.feat[3]); if (g == 0) occp[pa] = A.occ; }
        if (pb < cnt) { feat[pb * 4 + g] = make_float4(B.feat[0], B.feat[1], B.feat[2], B.feat[3]); if (g == 0) occp[pb] = B.occ; }
        set_in<false>(A, nx[0]); set_in<false>(B, nx[1]);
    }
}

// Every workgroup serves ONE part: the parts get contiguous ranges of workgroups in proportion to their (cost-weighted) tile
// counts (device-side counts), so a workgroup stages one LDS weight image instead of five and the per-part ceil() shares of a
// walk over all parts disappear.  A part too small for a range of its own is taken along by the workgroup where its range
// would start.  -> (vb, nb) of this workgroup inside part p's range, false if it does not serve p.
__device__ __forceinline__ bool part_range(const int64_t* tiles, int64_t total, int p, int b, int G, int& vb, int& nb) {
    int64_t cum = 0;
    for (int q = 0; q < p; ++q) cum += tiles[q];
    const int start = (int)(cum * G / total), end = (int)((cum + tiles[p]) * G / total);
    if (tiles[p] == 0) return false;
    if (end > start) { if (b < start || b >= end) return false; vb = b - start; nb = end - start; }
    else { if (b != min(start, G - 1)) return false; vb = 0; nb = 1; }
    return true;
}
// body(p, vb, nb) for every part p this workgroup serves, given the parts' (cost-weighted) tile counts
template <class Body>
__device__ __forceinline__ void for_my_parts(const int64_t* tiles, Body body) {
    const int G = (int)gridDim.x, b = (int)blockIdx.x;
    int64_t total = 0;
    for (int p = 0; p < INVR_NUM_PARTS; ++p) total += tiles[p];
    if (total == 0) return;
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        int vb, nb;
        if (!part_range(tiles, total, p, b, G, vb, nb)) continue;
        body(p, vb, nb);
    }
}

__global__ __launch_bounds__(MLP_BLOCK, 4) void k_part_occ_all(MlpAllArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[OCC_LDS_FLOATS];
    int64_t tiles[INVR_NUM_PARTS];
    for (int p = 0; p < INVR_NUM_PARTS; ++p) tiles[p] = (a.counts[p] + MLP_PAIRS_PER_WG - 1) / MLP_PAIRS_PER_WG;
    for_my_parts(tiles, [&](int p, int vb, int nb) { occ_part(lds, a.pm[p], a.emb[p], a.counts[p], a.cap, a.occp[p], a.feat[p], vb, nb); });
}

template <int NRGB, bool MEAN>
__device__ __forceinline__ void rgb_part(float* lds, const MlpAllArgs& a, const int part, const int g_last, const int total_tiles,
                                         const int vblock, const int nblocks) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    if (vblock * (MLP_BLOCK / 64) >= total_tiles) return;
    __syncthreads();                                   // previous part's weights no longer in use
    stage_weights<NRGB, true, 2>(a.pm[part], lds);
    __syncthreads();
    const float fmul = (float)(1 << g);                          // frequency 2^g of this lane group
    const float* __restrict__ emb = a.emb[part];
    const float* __restrict__ ds = a.ds[part];
    const float4* __restrict__ feat = a.feat[part];
    float4* featw = a.feat[part];                                // (aggr 'mean' writes the pair's result back into the pair's first float4:
                                                                 //  read by this wave a tile earlier, by no other wave)
    const float* __restrict__ occp = a.occp[part];
    const int32_t* __restrict__ l_slot = a.l_slot[part];
    const int32_t* __restrict__ wl = a.wl[part];
    const int64_t lcap = a.cap, cap = lcap - 1;                  // (MlpAllArgs::cap is the list capacity; cap as in Workspace and pair_lists.h)
    const int step = nblocks * (MLP_BLOCK / 64);
    int T = vblock * (MLP_BLOCK / 64) + wv;
    if (T >= total_tiles) return;
    SegCursor cur;
    cur.g0 = 0; cur.tiles_before = 0; cur.pairs_before = 0;
    seg_window(cur, a.wcnt, a.gcount, part, g_last, lane);
    // pair indices of tile T (-1 = column beyond the segment's winners; the loads then read the segment's last winner)
    auto tile_pairs = [&](int T_, int& ia, int& ib, bool& va, bool& vb_) {
        int t0, sb, sn;
        seg_locate(cur, T_, a.wcnt, a.gcount, part, g_last, lane, t0, sb, sn);
        const int ja = (T_ - t0) * 32 + col, jb = ja + 16;
        va = ja < sn; vb_ = jb < sn;
        ia = wl[sb + min(ja, sn - 1)]; ib = wl[sb + min(jb, sn - 1)];
    };
    auto load_in = [&](int pa, int pb, MlpIn (&in)[2]) {
        load_mlp_in<true>(in, emb, lcap, ds, a.stride, {(int64_t)pa, (int64_t)pb}, g);
        in[0].ft = feat[(int64_t)pa * 4 + g]; in[1].ft = feat[(int64_t)pb * 4 + g];
    };
    // software pipeline: inputs one tile ahead, pair indices two tiles ahead (a list read and the gathers it feeds are two
    // dependent round trips)
    int ia, ib, n_ia, n_ib, nn_ia = 0, nn_ib = 0;
    bool va, vb, n_va, n_vb, nn_va = false, nn_vb = false;
    MlpIn in[2], nx[2];
    tile_pairs(T, ia, ib, va, vb);
    load_in(ia, ib, in);
    n_ia = ia; n_ib = ib; n_va = n_vb = false;
    if (T + step < total_tiles) tile_pairs(T + step, n_ia, n_ib, n_va, n_vb);
    for (; T < total_tiles; T += step) {
        load_in(n_ia, n_ib, nx);                                  // (tile T + step; unused past the last tile)
        nn_ia = n_ia; nn_ib = n_ib; nn_va = nn_vb = false;
        if (T + 2 * step < total_tiles) tile_pairs(T + 2 * step, nn_ia, nn_ib, nn_va, nn_vb);
        const int slotA = l_slot[ia], slotB = l_slot[ib];         // consumed by the stores at the end of the tile
        const float occA = occp[ia], occB = occp[ib];
        MlpCol A, B;
        set_in<true>(A, in[0]); set_in<true>(B, in[1]);
        A.feat[0] = in[0].ft.x; A.feat[1] = in[0].ft.y; A.feat[2] = in[0].ft.z; A.feat[3] = in[0].ft.w;
        B.feat[0] = in[1].ft.x; B.feat[1] = in[1].ft.y; B.feat[2] = in[1].ft.z; B.feat[3] = in[1].ft.w;
        A.occ = occA; B.occ = occB;
        float4 rA, rB;
        rgb_stages<NRGB, false>(lds, lane, g, fmul, A, B, rA, rB);
        if (g == 0) {
            if (MEAN) {                                           // 'mean' / 'dist': per pair (k_winner_lists<1 / 2> sums them per survivor)
                if (va) featw[(int64_t)ia * 4] = rA;
                if (vb) featw[(int64_t)ib * 4] = rB;
            } else {                                              // the far-constant pair's result goes behind the per-slot ones
                if (va) a.rgbw[slotA == (int)far_slot(cap) ? far_result_index(cap, part) : (int64_t)slotA] = rA;
                if (vb) a.rgbw[slotB == (int)far_slot(cap) ? far_result_index(cap, part) : (int64_t)slotB] = rB;
            }
        }
        in[0] = nx[0]; in[1] = nx[1];
        ia = n_ia; ib = n_ib; va = n_va; vb = n_vb;
        n_ia = nn_ia; n_ib = nn_ib; n_va = nn_va; n_vb = nn_vb;
    }
}

#define RGB_WPS 2          // workgroups per CU the colour kernel is compiled / launched for (bf16 x 3: 59 KB of LDS each)
template <bool MEAN>
__global__ __launch_bounds__(MLP_BLOCK, RGB_WPS) void k_part_rgb_all(MlpAllArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ int s_tot[INVR_NUM_PARTS];
    const int lane = threadIdx.x & 63;
    const int g_last = last_group(a.n_active[0]);
    if (threadIdx.x < INVR_NUM_PARTS) s_tot[threadIdx.x] = 0;
    __syncthreads();
    {   // winner tiles per part (every workgroup sums the segment counts itself)
        int acc[INVR_NUM_PARTS] = {0, 0, 0, 0, 0};
        for (int q = threadIdx.x; q <= g_last; q += MLP_BLOCK)
#pragma unroll
            for (int p = 0; p < INVR_NUM_PARTS; ++p) acc[p] += (a.wcnt[group_row(q, p)] + 31) >> 5;
#pragma unroll
        for (int p = 0; p < INVR_NUM_PARTS; ++p) {
            acc[p] = __builtin_amdgcn_readlane(wave_incl_sum_i(acc[p]), 63);
            if (lane == 0 && acc[p]) atomicAdd(&s_tot[p], acc[p]);
        }
    }
    __syncthreads();
    int ntile[INVR_NUM_PARTS];
    int64_t tiles[INVR_NUM_PARTS];                     // tile counts weighted by the part's colour-MLP cost per pair (17.5 : 9.3 kFLOP)
    for (int p = 0; p < INVR_NUM_PARTS; ++p) {
        ntile[p] = s_tot[p];
        tiles[p] = (int64_t)((ntile[p] + (MLP_BLOCK / 64) - 1) / (MLP_BLOCK / 64)) * (a.pm[p].rgb.n_linear == 3 ? 15 : 8);
    }
    for_my_parts(tiles, [&](int p, int vb, int nb) {
        if (a.pm[p].rgb.n_linear == 3) rgb_part<3, MEAN>(lds, a, p, g_last, ntile[p], vb, nb);
        else rgb_part<2, MEAN>(lds, a, p, g_last, ntile[p], vb, nb);
    });
}

bool part_mlp_supported(const PartMlpDev& pm) {
    const MlpDev& o = pm.occ;
    const MlpDev& r = pm.rgb;
    const bool ok = o.n_linear == 2 && o.dims[0] == 19 && o.dims[1] == HID && o.dims[2] == 17 &&
                    (r.n_linear == 2 || r.n_linear == 3) && r.dims[0] == 70 && r.dims[1] == HID &&
                    r.dims[r.n_linear] == 3 && (r.n_linear == 2 || r.dims[2] == HID) &&
                    pm.n_freq == 4 && pm.latent_dim == 8 && pm.geo_dim == 16;
    if (!ok) invr_set_error("part MLP kernel supports occ 19-64-17 and rgb 70-64(-64)-3 with 4 view-dir frequencies, latent 8, geo feature 16");
    return ok;
}

int launch_part_mlp_all(const MlpAllArgs& a, const Workspace& w, hipStream_t st) {
    for (int p = 0; p < INVR_NUM_PARTS; ++p)
        if (!part_mlp_supported(a.pm[p])) return 1;
    int64_t tiles = cdiv(a.cap, (int64_t)MLP_PAIRS_PER_WG);
    unsigned grid_occ = (unsigned)(tiles < 256 * 4 ? (tiles > 0 ? tiles : 1) : 256 * 4);
    unsigned grid_rgb = (unsigned)(tiles < 256 * RGB_WPS ? (tiles > 0 ? tiles : 1) : 256 * RGB_WPS);
    hipLaunchKernelGGL(k_part_occ_all, dim3(grid_occ), dim3(MLP_BLOCK), 0, st, a);
    INVR_LAUNCH_CHECK();
    if (a.aggr == INVR_AGGR_MEAN || a.aggr == INVR_AGGR_DIST) {      // the sum flows: colour for every listed pair, then the merge
        if (launch_all_lists(w, st)) return 1;
        hipLaunchKernelGGL(k_part_rgb_all<true>, dim3(grid_rgb), dim3(MLP_BLOCK), 0, st, a);
        INVR_LAUNCH_CHECK();
        return launch_winner_lists(w, a.aggr, st);
    }
    if (launch_winner_lists(w, a.aggr, st)) return 1;                // the select flows: the merge, then colour for the winners
    hipLaunchKernelGGL(k_part_rgb_all<false>, dim3(grid_rgb), dim3(MLP_BLOCK), 0, st, a);
    INVR_LAUNCH_CHECK();
    return 0;
}

#define MLP_WPS 3          // workgroups per CU the single-part kernel is launched for
int launch_part_mlp(const PartMlpDev& pm, const float* emb, const float* d_soa, int64_t stride,
                    const int32_t* count, int64_t cap, float4* raw_direct, hipStream_t st) {
    if (!part_mlp_supported(pm)) return 1;
    int64_t tiles = cdiv(cap, (int64_t)MLP_PAIRS_PER_WG);
    unsigned grid = (unsigned)(tiles < 256 * MLP_WPS ? (tiles > 0 ? tiles : 1) : 256 * MLP_WPS);
    if (pm.rgb.n_linear == 3)
        hipLaunchKernelGGL(k_part_mlp<3>, dim3(grid), dim3(MLP_BLOCK), 0, st, pm, emb, d_soa, stride, count, cap, raw_direct);
    else
        hipLaunchKernelGGL(k_part_mlp<2>, dim3(grid), dim3(MLP_BLOCK), 0, st, pm, emb, d_soa, stride, count, cap, raw_direct);
    INVR_LAUNCH_CHECK();
    return 0;
}
