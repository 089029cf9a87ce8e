// K7 + K8: max-occupancy part merge and alpha compositing along the ray.
// Replaces TPoseHuman.forward's merge (inb_part_network_multiassign.py:229-256, cfg.aggr == ""),
// the scatter into full-size raw/occ (:156-159) and volume_rendering / render_weights
// (lib/utils/net_utils.py:12-44 as called at inb_renderer.py:72, i.e. epsilon = 0, no background).
//
// Lane = sample, 64 samples per pass, a wave walks the passes of a ray (k_composite: one wave per ray; k_composite_words, the merged
// source with S a multiple of 64: one wave per CMP_GROUP rays, live passes only): transmittance is an exclusive product
// scan done with 6 wave shuffles, rgb/acc are wave reductions.  The merge is done on the fly from
// the per-(slot,part) results, so the (N,4) raw tensor is only written when the caller wants it.
#include "composite_src.h"

#define CMP_BLOCK 256
typedef float cmp_v4 __attribute__((ext_vector_type(4)));

template <class Src>
__global__ __launch_bounds__(CMP_BLOCK) void k_composite(Src src, int64_t R, int S, float eps, float* __restrict__ weights,
                                                         float* __restrict__ rgb_map, float* __restrict__ acc_map,
                                                         float4* __restrict__ raw_out, float* __restrict__ occ_out) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (CMP_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;
    float T_run = 1.0f, ar = 0.f, ag = 0.f, ab = 0.f, aw = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool live = s < S;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            v = src.get(ray * S + s);
            // raw is the frame's largest output (16 B per ray-sample, 93 % zeros) and nothing on the device reads it again: stored
            // nontemporal so that its 0.5 GB per frame do not displace the row-sum tables and pair arrays of the frames in flight
            // from the L2 / Infinity Cache
            if (raw_out) __builtin_nontemporal_store((cmp_v4){v.x, v.y, v.z, v.w}, reinterpret_cast<cmp_v4*>(raw_out) + (ray * S + s));
            if (occ_out) occ_out[ray * S + s] = v.w;
        }
        const float alpha = v.w;
        const float incl = wave_incl_prod(live ? 1.0f - alpha + eps : 1.0f, lane);      // cumprod(1 - alpha + epsilon); eps = 0 (1 with cfg.random_bg)
        const float excl = dpp_f<0x138, 0xF>(1.0f, incl);                // wave_shr:1 (lane 0 keeps the identity)
        const float wgt = alpha * (T_run * excl);                        // render_weights (:12-15)
        if (live && weights) weights[ray * S + s] = wgt;
        ar = fmaf(wgt, v.x, ar); ag = fmaf(wgt, v.y, ag); ab = fmaf(wgt, v.z, ab); aw += wgt;
        T_run *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
    }
    ar = wave_sum(ar); ag = wave_sum(ag); ab = wave_sum(ab); aw = wave_sum(aw);
    if (lane == 0) {
        rgb_map[ray * 3] = ar; rgb_map[ray * 3 + 1] = ag; rgb_map[ray * 3 + 2] = ab;
        acc_map[ray] = aw;
    }
}

// The merged source when S is a multiple of 64: every 64-sample pass of a ray is exactly one aligned word of the survivor mask, owned
// by one wave alone, so the wave reads the word once, as a wave-uniform value, and decides per pass what the pass needs.
//  * A pass without a survivor (and epsilon 0) contributes nothing: its factors are 1 - 0 + 0 = 1 exactly, fmaf(0, 0, acc) and
//    acc + 0 are exact, so the look-ups, the scan and the accumulation are skipped and the results keep their bits.  A ray without any
//    survivor gets its zero map entries and nothing else.  (With epsilon != 0 — cfg.random_bg — an empty pass is not the identity: computed.)
//  * TRACKED (invr_render_fwd_tracked): `dirty` holds one bit per row of the caller's raw buffer, clear = the row holds four +0.0f.  93 %
//    of a frame's rows are zeros the cull dropped, the same zeros the frame before stored: only the rows of `cur | prev` are stored (zeros
//    where only `prev` is set) and lane 0 brings the dirty word to `cur`.  The dirty word of a pass is as aligned and as private as its
//    mask word.  Survivors beyond max_active (zero value, mask bit set) count as dirty.
//  * One wave takes CMP_GROUP consecutive rays (while their words fit its 64 lanes): lane j fetches the mask and dirty words of the group's
//    j-th pass in one load each, a ballot says which passes need anything at all, and the wave walks only those, in order, carrying the
//    ray's transmittance and sums from pass to pass and writing the maps when the ray changes.  Most of a frame's rays
//    have no survivor, and a wave of their own each cost them a launch and the latency of a first load: with no raw to store at all
//    one wave per ray took 66 us at 512 x 512 x 128, eight rays per wave take 43 (4: 40, 16: 52, 32: 89 — the live passes of a wave
//    are walked one after the other, each behind its own chain of look-ups; profiles/composite_tracked_raw.md).
#define CMP_GROUP 8
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long x, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
static int composite_group(int S) { const int npass = S >> 6; return npass >= 64 ? 1 : (64 / npass < CMP_GROUP ? 64 / npass : CMP_GROUP); }       // rays per wave

template <bool TRACKED>
__global__ __launch_bounds__(CMP_BLOCK) void k_composite_words(MergedRaw src, int64_t R, int S, int G, float eps, float* __restrict__ weights,
                                                               float* __restrict__ rgb_map, float* __restrict__ acc_map,
                                                               float4* __restrict__ raw_out, float* __restrict__ occ_out,
                                                               unsigned long long* __restrict__ dirty) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * (CMP_BLOCK / 64) + (threadIdx.x >> 6)) * G;          // the wave's rays: [r0, r0 + nr)
    if (r0 >= R) return;
    const int npass = S >> 6;
    const int nr = (int)min((int64_t)G, R - r0);
    const int64_t w0 = r0 * npass;                        // ... and their words: [w0, w0 + nw)
    const int nw = nr * npass;
    const bool skip_empty = eps == 0.0f;
    // passes that are walked whatever their words say: an output that is written densely, or arithmetic that is not the identity
    const bool every = !skip_empty || occ_out != nullptr || weights != nullptr || (!TRACKED && raw_out != nullptr);
    const cmp_v4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float T_run = 1.0f, ar = 0.f, ag = 0.f, ab = 0.f, aw = 0.f;
    int cur_ray = -1;                                     // the ray (of the group) whose passes are being walked
    bool any = false;                                     // ... has contributed something
    unsigned long long seen = 0ull;                       // rays of the group whose maps are written
    for (int c0 = 0; c0 < nw; c0 += 64) {
        const bool valid = c0 + lane < nw;
        unsigned long long mw = 0ull, dw = 0ull;
        if (valid) {
            mw = src.mask[w0 + c0 + lane];
            if (TRACKED) dw = dirty[w0 + c0 + lane];
        }
        unsigned long long act = __ballot(valid && (every || (mw | dw) != 0ull));
        while (act != 0ull) {
            const int p = __ffsll((long long)act) - 1;
            act &= act - 1ull;
            const int g = (c0 + p) / npass;
            if (g != cur_ray) {
                if (cur_ray >= 0) {
                    if (any) { ar = wave_sum(ar); ag = wave_sum(ag); ab = wave_sum(ab); aw = wave_sum(aw); }
                    if (lane == 0) {
                        const int64_t ray = r0 + cur_ray;
                        rgb_map[ray * 3] = ar; rgb_map[ray * 3 + 1] = ag; rgb_map[ray * 3 + 2] = ab;
                        acc_map[ray] = aw;
                    }
                    seen |= 1ull << cur_ray;
                }
                cur_ray = g; any = false;
                T_run = 1.0f; ar = ag = ab = aw = 0.f;
            }
            const unsigned long long cur = readlane_u64(mw, p);
            const unsigned long long prev = TRACKED ? readlane_u64(dw, p) : 0ull;
            const unsigned long long st = TRACKED ? (cur | prev) : (raw_out ? ~0ull : 0ull);      // rows of this pass to store
            const int64_t wi = w0 + c0 + p, row = wi * 64 + lane;
            if (cur == 0ull && skip_empty) {
                if ((st >> lane) & 1ull) __builtin_nontemporal_store(zero4, reinterpret_cast<cmp_v4*>(raw_out) + row);
                if (occ_out) occ_out[row] = 0.0f;
                if (weights) weights[row] = 0.0f;
                if (TRACKED && prev != 0ull && lane == 0) dirty[wi] = 0ull;
                continue;
            }
            any = true;
            const float4 v = src.get_m(row, cur);
            // raw is the frame's largest output and nothing on the device reads it again: stored nontemporal (see k_composite)
            if ((st >> lane) & 1ull) __builtin_nontemporal_store((cmp_v4){v.x, v.y, v.z, v.w}, reinterpret_cast<cmp_v4*>(raw_out) + row);
            if (occ_out) occ_out[row] = v.w;
            if (TRACKED && cur != prev && lane == 0) dirty[wi] = cur;
            const float alpha = v.w;
            const float incl = wave_incl_prod(1.0f - alpha + eps, lane);
            const float excl = dpp_f<0x138, 0xF>(1.0f, incl);
            const float wgt = alpha * (T_run * excl);
            if (weights) weights[row] = wgt;
            ar = fmaf(wgt, v.x, ar); ag = fmaf(wgt, v.y, ag); ab = fmaf(wgt, v.z, ab); aw += wgt;
            T_run *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
        }
    }
    if (cur_ray >= 0) {
        if (any) { ar = wave_sum(ar); ag = wave_sum(ag); ab = wave_sum(ab); aw = wave_sum(aw); }
        if (lane == 0) {
            const int64_t ray = r0 + cur_ray;
            rgb_map[ray * 3] = ar; rgb_map[ray * 3 + 1] = ag; rgb_map[ray * 3 + 2] = ab;
            acc_map[ray] = aw;
        }
        seen |= 1ull << cur_ray;
    }
    if (lane < nr && !((seen >> lane) & 1ull)) {          // rays none of whose passes was walked: nothing survived on them
        const int64_t ray = r0 + lane;
        rgb_map[ray * 3] = 0.f; rgb_map[ray * 3 + 1] = 0.f; rgb_map[ray * 3 + 2] = 0.f;
        acc_map[ray] = 0.f;
    }
}

// S not a multiple of 64: mask words straddle rays (waves), the stores stay dense, and the dirty words of [0, N) follow the frame's mask
// in a launch of their own; the bits at or beyond N in the last word are the caller's and stay.
__global__ __launch_bounds__(256) void k_dirty_from_mask(const unsigned long long* __restrict__ mask, int64_t N, unsigned long long* __restrict__ dirty) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ((N + 63) >> 6)) return;
    unsigned long long m = mask[i];
    const int64_t left = N - i * 64;
    if (left < 64) {
        const unsigned long long valid = (1ull << left) - 1ull;
        m = (m & valid) | (dirty[i] & ~valid);
    }
    dirty[i] = m;
}

// (k_composite, dense stores: one workgroup per four rays; a fixed grid of 4096 workgroups walking the rays measured the same 135 us —
// with 16 B / sample of output that kernel is bound by its store stream, not by dispatch.  k_composite_words, which stores a fourteenth
// of that or nothing, is not: see its header)
static unsigned composite_grid(int64_t n_rays) { return (unsigned)cdiv(n_rays, CMP_BLOCK / 64); }

int launch_composite(const float* raw, int64_t n_rays, int S, float eps, float* weights, float* rgb_map, float* acc_map, hipStream_t st) {
    if (n_rays == 0) return 0;
    DenseRaw src{reinterpret_cast<const float4*>(raw)};
    hipLaunchKernelGGL(k_composite<DenseRaw>, dim3(composite_grid(n_rays)), dim3(CMP_BLOCK), 0, st,
                       src, n_rays, S, eps, weights, rgb_map, acc_map, (float4*)nullptr, (float*)nullptr);
    INVR_LAUNCH_CHECK();
    return 0;
}

int launch_merge_composite(const RenderArgs& a, const Workspace& w, float* rgb_map, float* acc_map, float* raw,
                           float* occ, float* weights, hipStream_t st, unsigned long long* raw_dirty) {
    if (a.R == 0) return 0;
    MergedRaw src{w.mask, w.word_off, w.ord_rows > 0 ? w.byte_off : nullptr, w.wsel, w.rgbw, w.cap};
    if ((a.S & 63) == 0) {
        const int G = composite_group(a.S);
        if (raw_dirty)
            hipLaunchKernelGGL(k_composite_words<true>, dim3(composite_grid(cdiv(a.R, G))), dim3(CMP_BLOCK), 0, st,
                               src, a.R, a.S, G, a.scene.comp_eps, weights, rgb_map, acc_map, reinterpret_cast<float4*>(raw), occ, raw_dirty);
        else
            hipLaunchKernelGGL(k_composite_words<false>, dim3(composite_grid(cdiv(a.R, G))), dim3(CMP_BLOCK), 0, st,
                               src, a.R, a.S, G, a.scene.comp_eps, weights, rgb_map, acc_map, reinterpret_cast<float4*>(raw), occ, (unsigned long long*)nullptr);
        INVR_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(k_composite<MergedRaw>, dim3(composite_grid(a.R)), dim3(CMP_BLOCK), 0, st,
                       src, a.R, a.S, a.scene.comp_eps, weights, rgb_map, acc_map, reinterpret_cast<float4*>(raw), occ);
    INVR_LAUNCH_CHECK();
    if (raw_dirty) {
        hipLaunchKernelGGL(k_dirty_from_mask, dim3((unsigned)cdiv(cdiv(a.N, (int64_t)64), (int64_t)256)), dim3(256), 0, st, w.mask, a.N, raw_dirty);
        INVR_LAUNCH_CHECK();
    }
    return 0;
}

// ---- distortion regulariser (inb_renderer.py:96-103), O(S) per ray with running prefix sums -------
// sum_ij w_i w_j |m_i - m_j| = 2 * sum_i w_i (m_i * W_<i - M_<i) for ascending m (z is ascending);
// evaluated in the reference's O(S^2) form when S <= 64 is not needed: both agree to fp32 rounding.
__global__ __launch_bounds__(CMP_BLOCK) void k_distortion(const float* __restrict__ weights, const float* __restrict__ z,
                                                          int64_t R, int S, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (CMP_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;
    const float* wr = weights + ray * S;
    const float* zr = z + ray * S;
    // direct double loop split over lanes (S is 64..128 in practice): lane i accumulates row i
    float acc = 0.0f;
    for (int i = lane; i < S; i += 64) {
        const float mi = (zr[i] + zr[min(i + 1, S - 1)]) / 2.0f;
        const float wi = wr[i];
        float row = 0.0f;
        for (int j = 0; j < S; ++j) {
            const float mj = (zr[j] + zr[min(j + 1, S - 1)]) / 2.0f;
            row += (wi * wr[j]) * fabsf(mi - mj);
        }
        acc += row;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[ray] = acc;
}

int launch_distortion(const float* weights, const float* z, int64_t n_rays, int S, float* out, hipStream_t st) {
    if (n_rays == 0) return 0;
    hipLaunchKernelGGL(k_distortion, dim3((unsigned)cdiv(n_rays, CMP_BLOCK / 64)), dim3(CMP_BLOCK), 0, st, weights, z, n_rays, S, out);
    INVR_LAUNCH_CHECK();
    return 0;
}

// ---- backward of the compositing (net_utils.py:12-44 under autograd) ------------------------------
// (written for epsilon = 0; with the epsilon of render_weights every factor 1-a_j below is 1-a_j+eps.)
// w_k = a_k T_k, T_k = prod_{j<k}(1-a_j).  With G_k = dL/dw_k (from rgb_map, acc_map and any direct
// weight gradient):
//     dL/da_i = T_i (G_i - Q_i),   Q_i = sum_{k>i} G_k a_k prod_{i<j<k}(1-a_j)
// (the product EXCLUDES factor i, so nothing is divided by 1-a_i: alpha == 1 — reachable, 1-exp(-softplus(h))
// rounds to 1 for h >~ 17 — gives the finite gradient torch's zero-aware cumprod backward gives, and alpha close to 1
// has no cancellation).  Q obeys the backward recurrence Q_i = G_{i+1} a_{i+1} + (1-a_{i+1}) Q_{i+1}, Q_{S-1} = 0:
// a composition of affine maps f_k(x) = b_k + m_k x, which is associative -> one wave suffix scan over (m, b) pairs per
// 64-sample pass, passes walked back to front with a carried Q.  dL/drgb_i = w_i * g_rgb.
struct Affine { float m, b; };
__device__ __forceinline__ Affine wave_suffix_compose(Affine f, int lane) {     // F_l = f_l o f_{l+1} o ... o f_63
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float m2 = __shfl_down(f.m, d), b2 = __shfl_down(f.b, d);
        if (lane + d < 64) { f.b = fmaf(f.m, b2, f.b); f.m *= m2; }
    }
    return f;
}

__global__ __launch_bounds__(CMP_BLOCK) void k_composite_bwd(const float4* __restrict__ raw, const float* __restrict__ g_rgb,
                                                             const float* __restrict__ g_acc, const float* __restrict__ g_w,
                                                             int64_t R, int S, float eps, float4* __restrict__ g_raw) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (CMP_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;
    const float gr = g_rgb[ray * 3], gg = g_rgb[ray * 3 + 1], gb = g_rgb[ray * 3 + 2];
    const float ga = g_acc ? g_acc[ray] : 0.0f;
    const int npass = (S + 63) / 64;
    float carry = 0.0f;     // Q of the last sample of the current pass
    for (int ps = npass - 1; ps >= 0; --ps) {
        // transmittance at the start of this pass: product over the earlier passes (recomputed per pass — S is a
        // few passes at most, and no per-thread array bounds the sample count)
        float T0 = 1.0f;
        for (int q = 0; q < ps; ++q) {
            const float aq = raw[ray * S + q * 64 + lane].w;
            T0 *= __shfl(wave_incl_prod(1.0f - aq + eps, lane), 63);
        }
        const int s = ps * 64 + lane;
        const bool live = s < S;
        float4 v = live ? raw[ray * S + s] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float a = v.w;
        const float incl = wave_incl_prod(live ? 1.0f - a + eps : 1.0f, lane);
        float excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0f;
        const float T = T0 * excl;
        const float wgt = a * T;
        const float G = live ? (gr * v.x + gg * v.y + gb * v.z + ga + (g_w ? g_w[ray * S + s] : 0.0f)) : 0.0f;
        const Affine F = wave_suffix_compose(Affine{live ? 1.0f - a + eps : 1.0f, G * a}, lane);       // dead lanes: identity map
        float Mn = __shfl_down(F.m, 1), Bn = __shfl_down(F.b, 1);
        if (lane == 63) { Mn = 1.0f; Bn = 0.0f; }
        const float Q = fmaf(Mn, carry, Bn);
        if (live) {
            float4 o;
            o.x = wgt * gr; o.y = wgt * gg; o.z = wgt * gb;
            o.w = T * (G - Q);
            g_raw[ray * S + s] = o;
        }
        carry = fmaf(__shfl(F.m, 0), carry, __shfl(F.b, 0));
    }
}

int launch_composite_bwd(const float* raw, const float* g_rgb, const float* g_acc, const float* g_w, int64_t n_rays, int S, float eps,
                         float* g_raw, hipStream_t st) {
    if (n_rays == 0) return 0;
    hipLaunchKernelGGL(k_composite_bwd, dim3((unsigned)cdiv(n_rays, CMP_BLOCK / 64)), dim3(CMP_BLOCK), 0, st,
                       reinterpret_cast<const float4*>(raw), g_rgb, g_acc, g_w, n_rays, S, eps, reinterpret_cast<float4*>(g_raw));
    INVR_LAUNCH_CHECK();
    return 0;
}
