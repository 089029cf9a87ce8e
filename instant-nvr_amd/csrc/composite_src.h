// The compositing sources and wave scans shared by k_composite.hip and k_geomaps.hip: one definition of the merged per-survivor
// look-up (MergedRaw), the dense raw source and the DPP product scan / sum that render_weights is formed with.
#pragma once
#include "pair_lists.h"

// Wave-wide inclusive product scan and sum on the DPP network (row_shr 1 / 2 / 4 / 8 inside the 16-lane rows, then row_bcast:15 and
// row_bcast:31 across rows — the sequence LLVM's own wave scans use on gfx9): six full-rate VALU instructions per scan.  The
// __shfl_up form compiles to ds_bpermute_b32 — an LDS round trip per step, ~20 dependent ones per 128-sample ray — and the kernel
// was bound by exactly that latency at its occupancy.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float identity, float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_incl_prod(float x, int) {
    x *= dpp_f<0x111, 0xF>(1.0f, x);          // row_shr:1
    x *= dpp_f<0x112, 0xF>(1.0f, x);          // row_shr:2
    x *= dpp_f<0x114, 0xF>(1.0f, x);          // row_shr:4
    x *= dpp_f<0x118, 0xF>(1.0f, x);          // row_shr:8
    x *= dpp_f<0x142, 0xA>(1.0f, x);          // row_bcast:15 -> rows 1 and 3
    x *= dpp_f<0x143, 0xC>(1.0f, x);          // row_bcast:31 -> rows 2 and 3
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {           // total in every lane that reads lane 63's value: returned broadcast
    x += dpp_f<0x111, 0xF>(0.0f, x);
    x += dpp_f<0x112, 0xF>(0.0f, x);
    x += dpp_f<0x114, 0xF>(0.0f, x);
    x += dpp_f<0x118, 0xF>(0.0f, x);
    x += dpp_f<0x142, 0xA>(0.0f, x);
    x += dpp_f<0x143, 0xC>(0.0f, x);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

struct DenseRaw {      // raw (R,S,4) given
    const float4* raw;
    __device__ __forceinline__ float4 get(int64_t i) const { return raw[i]; }
};
struct MergedRaw {     // merge per-part results of the survivor slot of sample i
    const unsigned long long* mask;      // survivor bit of sample i: bit i&63 of word i>>6
    const int32_t* word_off;             // rank of the first survivor of every word (ray-major order)
    const int32_t* byte_off;             // windowed order (Workspace::ord_rows > 0): rank of the first survivor of every mask byte; else NULL
    const uint8_t* wsel;                 // the merge's choice per survivor (k_winner_lists)
    const float4* rgbw;                  // [rgb, occ] of the winning listed pair at the survivor's slot; far constants at [lcap + p]
    int64_t const_slot;                  // Workspace::cap (pair_lists.h: the far-constant rule)
    __device__ __forceinline__ float4 get(int64_t i) const { return get_m(i, mask[i >> 6]); }
    __device__ __forceinline__ float4 get_m(int64_t i, unsigned long long m) const {          // m = mask[i >> 6]
        const int bit = (int)(i & 63);
        int slot = -1;
        if ((m >> bit) & 1ull) {
            if (byte_off) slot = byte_off[i >> 3] + __popc((unsigned)(m >> (bit & ~7)) & ((1u << (bit & 7)) - 1u));
            else slot = word_off[i >> 6] + __popcll(m & ((1ull << bit) - 1ull));
        }
        if (slot >= const_slot) slot = -1;                   // survivor beyond max_active (reported in stats[6])
        float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
        if (slot >= 0) {
            // argmax over the 5 parts with zeros for unflagged parts, first maximum wins (:253-255): decided by k_winner_lists
            const unsigned sel = wsel[slot];
            if (wsel_is_listed(sel)) best = rgbw[slot];
            else if (!wsel_is_none(sel)) best = rgbw[far_result_index(const_slot, wsel_far_part(sel))];      // far pair: per-part constant
        }
        return best;
    }
};
