// The level rules of the multi-resolution hash grid (HashEmbedder.forward, lib/networks/embedders/part_base_embedder.py:106-174), each
// stated once: where a level's table starts, how many rows it has, which row a corner names, the trilinear weights, the normalisation
// of a world point into the box, the corners of a level.  Every kernel that touches a grid (k_encode.hip, k_warp.hip, front_bodies.h,
// grid_generic.h) and the host's table totals (invr_abi.hip) go through these.  The hash reducers and div_exact are common.h's.
#pragma once
#include "common.h"

// ---- tables --------------------------------------------------------------------------------------------------------------------------
// Start of level l's table: separate_dense keeps the dense levels back to back in `dense` (dense_off rows in front of level l) and
// T rows per hashed level in `hash`; otherwise ONE (L, T, F) table (:153-154).
// FC: the row width when the kernel fixes it (16 for the part grids, 2 for the deformer's), else g.F.
template <int FC = 0>
__device__ __forceinline__ const float* grid_level_table(const GridDev& g, int l, bool hashed) {      // hashed = l >= g.start_hash
    const int F = FC ? FC : g.F;
    return g.separate_dense ? (hashed ? g.hash + (int64_t)(l - g.start_hash) * g.T * F : g.dense + g.dense_off[l] * F)
                            : g.hash + (int64_t)l * g.T * F;
}
template <int FC = 0>
__device__ __forceinline__ const float* grid_level_table(const GridDev& g, int l) { return grid_level_table<FC>(g, l, l >= g.start_hash); }
// the same place in a (dense, hash) pair of arrays laid out as the tables — their gradients g_dense / g_hash; tab = grid_level_table(g, l)
template <typename T>
__device__ __forceinline__ T* grid_level_like(const GridDev& g, bool hashed, const float* tab, T* dense, T* hash) {
    return g.separate_dense ? (hashed ? hash + (tab - g.hash) : dense + (tab - g.dense)) : hash + (tab - g.hash);
}
// the same start in invr_grid_row_sums / rowgrad order, in rows: the dense rows, then T per hashed level (dense_rows = 0 for the single table)
__host__ __device__ __forceinline__ int64_t grid_level_rs_off(const GridDev& g, int l, bool hashed) {
    return g.separate_dense ? (hashed ? g.dense_rows + (int64_t)(l - g.start_hash) * g.T : g.dense_off[l]) : (int64_t)l * g.T;
}
__host__ __device__ __forceinline__ int64_t grid_level_rs_off(const GridDev& g, int l) { return grid_level_rs_off(g, l, l >= g.start_hash); }
// rows of level l: T when hashed, res^3 when dense (:124-129)
__host__ __device__ __forceinline__ int64_t grid_level_rows(const GridDev& g, int l) {
    return l >= g.start_hash ? g.T : (int64_t)g.res[l] * g.res[l] * g.res[l];
}
// rows of the two tables (dense_rows = 0 without separate_dense); their sum is the length of the row-sum table
__host__ __device__ __forceinline__ void grid_table_rows(const GridDev& g, int64_t& dense_rows, int64_t& hash_rows) {
    dense_rows = g.separate_dense ? g.dense_rows : 0;
    hash_rows = (int64_t)(g.separate_dense ? g.L - g.start_hash : g.L) * g.T;
}
// De-hashed vertex tables (GridDev.vertex_sums): a hashed level of at most max_rows vertices gets a dense (res^3,) table of the row sums
// its vertices name; the tables lie back to back in level order, two pad floats behind the last (the dense route of level_rowsum
// reads 8-byte z pairs).  GRID_VERTEX_MAX_ROWS bounds max_rows: res^3 <= 2^24 gives res <= 256, so every operand of that route's
// __umul24 (cx, cx res + cy < res^2 <= 2^16, res) is far below 2^24.  -> floats in all (0: no level qualifies); off[l] = -1 elsewhere.
#define GRID_VERTEX_MAX_ROWS (1ll << 24)          // = include/invr_vertex.h INVR_VERTEX_MAX_ROWS (invr_abi.hip asserts it)
__host__ __device__ __forceinline__ int64_t grid_vertex_layout(const GridDev& g, int64_t max_rows, int64_t* off) {
    int64_t total = 0;
    for (int l = 0; l < INVR_MAX_LEVELS; ++l) {
        const int64_t rows = (int64_t)g.res[l] * g.res[l] * g.res[l];
        const bool own = l >= g.start_hash && l < g.L && rows <= max_rows && max_rows <= GRID_VERTEX_MAX_ROWS;
        off[l] = own ? total : -1;
        if (own) total += rows;
    }
    return total ? total + 2 : 0;
}
// floats per encoded point
__host__ __device__ __forceinline__ int grid_out_dim(const GridDev& g) {
    return (g.sum ? (g.sum_over_features ? g.L : g.F) : g.L * g.F) + (g.include_input ? 3 : 0);
}

// ---- rows ----------------------------------------------------------------------------------------------------------------------------
// Row of corner (cx, cy, cz) relative to its level's table: hashed (cx * 1) ^ (cy * P1) ^ (cz * P2) mod T in 64 bits (:132-136), dense
// (cx res + cy) res + cz (:124-129; res^3 <= T < 2^31).  The pair form serves the two z corners of one (x, y) corner and forms the
// (x, y) part once.  (k_encode.hip:level_rowsum keeps reducers specialised for its table — same rows.)
// The spellings here are the ones that compile the timed kernels to the code of the hand-written copies (the z corners in front of
// cx, cy; a struct for the pair; `hashed` handed in; the row width a template constant): profiles/grid_level_rules.md.
struct GridRowPair { unsigned r0, r1; };
__device__ __forceinline__ GridRowPair grid_row_zpair(const GridDev& g, bool hashed, int res, int c0z, int c1z, int cx, int cy) {
    GridRowPair r;
    if (hashed) {
        const uint64_t hxy = (uint64_t)(uint32_t)cx ^ ((uint64_t)(uint32_t)cy * HASH_P1);
        r.r0 = grid_hash_mod(hxy ^ ((uint64_t)(uint32_t)c0z * HASH_P2), g);
        r.r1 = grid_hash_mod(hxy ^ ((uint64_t)(uint32_t)c1z * HASH_P2), g);
    } else {
        const unsigned rb = ((unsigned)cx * (unsigned)res + (unsigned)cy) * (unsigned)res;
        r.r0 = rb + (unsigned)c0z;
        r.r1 = rb + (unsigned)c1z;
    }
    return r;
}
__device__ __forceinline__ unsigned grid_row(const GridDev& g, bool hashed, int res, int cx, int cy, int cz) {
    if (hashed) return grid_hash_mod((uint64_t)(uint32_t)cx ^ ((uint64_t)(uint32_t)cy * HASH_P1) ^ ((uint64_t)(uint32_t)cz * HASH_P2), g);
    return ((unsigned)cx * (unsigned)res + (unsigned)cy) * (unsigned)res + (unsigned)cz;
}

// ---- weights -------------------------------------------------------------------------------------------------------------------------
// weight_k = prod_axis ((1-o) + (2o-1) t)  (:157-158) of corner k = offsets 000, 001, ..., 111 (x y z, z fastest, :81-88); u. = 1 - t.
__device__ __forceinline__ float trilinear_weight(int k, float tx, float ux, float ty, float uy, float tz, float uz) {
    return ((k & 4) ? tx : ux) * ((k & 2) ? ty : uy) * ((k & 1) ? tz : uz);
}

// ---- box -----------------------------------------------------------------------------------------------------------------------------
// world -> normalised coordinate (x - b0) / (b1 - b0) per axis (:112): one axis on the spot, or through the box read once (GridBox)
__device__ __forceinline__ float grid_norm(const GridDev& g, int a, float x) { return (x - g.bounds[a]) / (g.bounds[3 + a] - g.bounds[a]); }
struct GridBox { float b0[3], e[3]; };
__device__ __forceinline__ GridBox grid_box(const GridDev& g) {
    GridBox b;
#pragma unroll
    for (int a = 0; a < 3; ++a) b.b0[a] = g.bounds[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) b.e[a] = g.bounds[3 + a] - b.b0[a];
    return b;
}
__device__ __forceinline__ float grid_norm(const GridBox& b, int a, float x) { return (x - b.b0[a]) / b.e[a]; }

// ---- corners -------------------------------------------------------------------------------------------------------------------------
// Normalised coordinate -> per-axis clipped corners and fractional offsets of one level
// (part_base_embedder.py:115-118): f = x / cell; c0 = clip(trunc(f)), c1 = clip(trunc(f + 1));
// t = f - c0 (may leave [0,1] outside the box -> extrapolation).
// Three forms of the quotient, one clip: the IEEE division; common.h:div_exact (rcell = GridDev.rcell[l]); and div_by_rcp alone —
// FAST: the caller has established, once per tile of pairs, that every lane's three coordinates are in div_exact's proven range
// and that this level's reciprocal is usable (rcell != 0) — the three quotients then take the 5-instruction reciprocal form without
// div_exact's per-call range test + ballot + branch (nine wave-uniform branches per level pair of a tile otherwise).  Same bits.
__device__ __forceinline__ void level_corners_of(float f, int res, int& c0, int& c1, float& t) {
    int a = (int)f;              // v_cvt_i32_f32: truncates toward zero (torch .long())
    int b = (int)(f + 1.0f);
    c0 = min(max(a, 0), res - 1);
    c1 = min(max(b, 0), res - 1);
    t = f - (float)c0;
}
__device__ __forceinline__ void level_corners(float x, float cell, int res, int& c0, int& c1, float& t) {
    level_corners_of(x / cell, res, c0, c1, t);
}
__device__ __forceinline__ void level_corners(float x, float cell, float rcell, int res, int& c0, int& c1, float& t) {
    level_corners_of(div_exact(x, cell, rcell), res, c0, c1, t);
}
__device__ __forceinline__ void level_corners_fast(float x, float cell, float rcell, int res, int& c0, int& c1, float& t) {
    level_corners_of(div_by_rcp(x, cell, rcell), res, c0, c1, t);
}
