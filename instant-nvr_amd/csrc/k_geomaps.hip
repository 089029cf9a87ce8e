// Per-ray geometry maps (include/invr_geomaps.h): the expected depth sum_i w_i z_i (nerf_net_utils.py:28 of the reference: depth_map =
// sum(weights * z_vals, -1)), the first sample whose occupancy reaches a level with the interpolated depth of that crossing, the
// six-point stencil around the surface point and the normal from the field's central differences (what lib/visualizers/if_nerf.py
// reads as depth_map / surf_normal / surf_mask).
//
// The depth is a second pass over what the compositing read, not a change to the compositing kernels: it takes the same two sources
// (a dense occupancy, or the merged per-survivor results the render left in the workspace), forms render_weights with the same scan
// (composite_src.h: one definition) and stores three values per ray and nothing per sample.  Lane = sample, 64 samples per pass:
// k_geo_depth, one wave per ray (the dense source; the merged one when S is no multiple of 64), and k_geo_depth_words, the merged source
// with S a multiple of 64, where a pass is one aligned word of the survivor mask: with epsilon 0 an empty word contributes nothing
// (factors 1, weights 0, no crossing) and is skipped.
#include <math.h>
#include "composite_src.h"
#include "pipeline.h"
#include "../../include/invr_geomaps.h"

#define GEO_BLOCK 256

struct DenseOcc {      // occ (R,S) given
    const float* occ;
    __device__ __forceinline__ float4 get(int64_t i) const { return make_float4(0.f, 0.f, 0.f, occ[i]); }
};

// depth of sample s of the ray: the caller's z_vals row, or the renderer's own formula
__device__ __forceinline__ float geo_z(const float* zrow, float near, float far, int s, int S) {
    return zrow ? zrow[s] : sample_z(near, far, s, S, nullptr);
}

template <class Src>
__global__ __launch_bounds__(GEO_BLOCK) void k_geo_depth(Src src, const float* __restrict__ near, const float* __restrict__ far,
                                                         const float* __restrict__ z_vals, int64_t R, int S, float eps, float level,
                                                         float* __restrict__ depth_map, int32_t* __restrict__ surf_index,
                                                         float* __restrict__ surf_depth) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (GEO_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;
    const float* zrow = z_vals ? z_vals + ray * S : nullptr;
    const float zn = zrow ? 0.0f : near[ray], zf = zrow ? 0.0f : far[ray];
    float T_run = 1.0f, acc = 0.0f;
    float prev_last = 0.0f;          // occupancy of the sample in front of this pass (wave-uniform)
    bool found = false;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool live = s < S;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = src.get(ray * S + s);
        const float alpha = v.w;
        const float incl = wave_incl_prod(live ? 1.0f - alpha + eps : 1.0f, lane);      // as k_composite forms it
        const float excl = dpp_f<0x138, 0xF>(1.0f, incl);                // wave_shr:1 (lane 0 keeps the identity)
        const float wgt = alpha * (T_run * excl);                        // render_weights
        const float z = live ? geo_z(zrow, zn, zf, s, S) : 0.0f;
        acc = fmaf(wgt, z, acc);
        T_run *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
        const float before = dpp_f<0x138, 0xF>(prev_last, alpha);        // occupancy of sample s - 1 (lane 0: the pass in front)
        prev_last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(alpha), 63));
        if (!found) {
            const unsigned long long hit = __ballot(live && alpha >= level);
            if (hit != 0ull) {
                found = true;
                if (lane == __ffsll((long long)hit) - 1) {
                    float zs = z;
                    if (s > 0) {
                        const float o0 = before == before ? before : 0.0f;       // a NaN interpolates as 0
                        const float z0 = geo_z(zrow, zn, zf, s - 1, S);
                        const float t = (level - o0) / (alpha - o0);
                        zs = z0 + t * (z - z0);
                    }
                    if (surf_index) surf_index[ray] = s;
                    if (surf_depth) surf_depth[ray] = zs;
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (depth_map) depth_map[ray] = acc;
        if (!found) {
            if (surf_index) surf_index[ray] = -1;
            if (surf_depth) surf_depth[ray] = 0.0f;
        }
    }
}

// The merged source when S is a multiple of 64, laid out as k_composite_words: one wave takes GEO_GROUP consecutive rays (while their
// mask words fit its 64 lanes), lane j fetches the word of the group's j-th pass, a ballot says which passes hold a survivor (with
// epsilon != 0: all of them, an empty pass is not the identity then) and the wave walks only those, in order, carrying the ray's
// transmittance, sum and last occupancy from pass to pass.  Most rays of a frame have no survivor at all: a wave of their own each
// cost them a launch and the latency of a first load (one wave per ray: 80 us for the depth pass at 512 x 512 x 128,
// profiles/geometry_maps.md).  The arithmetic of a walked pass is k_geo_depth's, so the maps keep their bits.
#define GEO_GROUP 8
__device__ __forceinline__ unsigned long long geo_readlane_u64(unsigned long long x, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
static int geo_group(int S) { const int npass = S >> 6; return npass >= 64 ? 1 : (64 / npass < GEO_GROUP ? 64 / npass : GEO_GROUP); }       // rays per wave

__global__ __launch_bounds__(GEO_BLOCK) void k_geo_depth_words(MergedRaw src, const float* __restrict__ near, const float* __restrict__ far,
                                                               const float* __restrict__ z_vals, int64_t R, int S, int G, float eps, float level,
                                                               float* __restrict__ depth_map, int32_t* __restrict__ surf_index,
                                                               float* __restrict__ surf_depth) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * (GEO_BLOCK / 64) + (threadIdx.x >> 6)) * G;          // the wave's rays: [r0, r0 + nr)
    if (r0 >= R) return;
    const int npass = S >> 6;
    const int nr = (int)min((int64_t)G, R - r0);
    const int64_t w0 = r0 * npass;                        // ... and their words: [w0, w0 + nw)
    const int nw = nr * npass;
    const bool every = eps != 0.0f;
    float T_run = 1.0f, acc = 0.0f, prev_last = 0.0f, zn = 0.0f, zf = 0.0f;
    const float* zrow = nullptr;
    int cur_ray = -1, last_q = -1;                        // the ray (of the group) whose passes are being walked, and its last walked pass
    bool found = false;
    unsigned long long seen = 0ull;                       // rays of the group whose maps are written
    for (int c0 = 0; c0 < nw; c0 += 64) {
        const bool valid = c0 + lane < nw;
        const unsigned long long mw = valid ? src.mask[w0 + c0 + lane] : 0ull;
        unsigned long long act = __ballot(valid && (every || mw != 0ull));
        while (act != 0ull) {
            const int p = __ffsll((long long)act) - 1;
            act &= act - 1ull;
            const int g = (c0 + p) / npass, q = (c0 + p) - g * npass;
            if (g != cur_ray) {
                if (cur_ray >= 0) {
                    acc = wave_sum(acc);
                    if (lane == 0) {
                        const int64_t ray = r0 + cur_ray;
                        if (depth_map) depth_map[ray] = acc;
                        if (!found) {
                            if (surf_index) surf_index[ray] = -1;
                            if (surf_depth) surf_depth[ray] = 0.0f;
                        }
                    }
                    seen |= 1ull << cur_ray;
                }
                cur_ray = g; last_q = -1; found = false;
                T_run = 1.0f; acc = 0.0f; prev_last = 0.0f;
                zrow = z_vals ? z_vals + (r0 + g) * S : nullptr;
                zn = zrow ? 0.0f : near[r0 + g]; zf = zrow ? 0.0f : far[r0 + g];
            }
            if (q != last_q + 1) prev_last = 0.0f;          // empty passes in between: the sample in front of this pass was culled
            last_q = q;
            const unsigned long long cur = geo_readlane_u64(mw, p);
            const int64_t ray = r0 + g, row = (w0 + c0 + p) * 64 + lane;
            const int s = q * 64 + lane;
            const float4 v = src.get_m(row, cur);
            const float alpha = v.w;
            const float incl = wave_incl_prod(1.0f - alpha + eps, lane);
            const float excl = dpp_f<0x138, 0xF>(1.0f, incl);
            const float wgt = alpha * (T_run * excl);
            const float z = geo_z(zrow, zn, zf, s, S);
            acc = fmaf(wgt, z, acc);
            T_run *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
            const float before = dpp_f<0x138, 0xF>(prev_last, alpha);
            prev_last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(alpha), 63));
            if (!found) {
                const unsigned long long hit = __ballot(alpha >= level);
                if (hit != 0ull) {
                    found = true;
                    if (lane == __ffsll((long long)hit) - 1) {
                        float zs = z;
                        if (s > 0) {
                            const float o0 = before == before ? before : 0.0f;
                            const float z0 = geo_z(zrow, zn, zf, s - 1, S);
                            const float t = (level - o0) / (alpha - o0);
                            zs = z0 + t * (z - z0);
                        }
                        if (surf_index) surf_index[ray] = s;
                        if (surf_depth) surf_depth[ray] = zs;
                    }
                }
            }
        }
    }
    if (cur_ray >= 0) {
        acc = wave_sum(acc);
        if (lane == 0) {
            const int64_t ray = r0 + cur_ray;
            if (depth_map) depth_map[ray] = acc;
            if (!found) {
                if (surf_index) surf_index[ray] = -1;
                if (surf_depth) surf_depth[ray] = 0.0f;
            }
        }
        seen |= 1ull << cur_ray;
    }
    if (lane < nr && !((seen >> lane) & 1ull)) {          // rays none of whose passes was walked: nothing survived on them
        const int64_t ray = r0 + lane;
        if (depth_map) depth_map[ray] = 0.0f;
        if (surf_index) surf_index[ray] = -1;
        if (surf_depth) surf_depth[ray] = 0.0f;
    }
}

// one thread per stencil point: 6 per listed ray
__global__ __launch_bounds__(GEO_BLOCK) void k_surface_stencil(const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                               const float* __restrict__ surf_depth, const int32_t* __restrict__ rows,
                                                               int64_t n, float h, float* __restrict__ pts, float* __restrict__ dirs) {
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= n * 6) return;
    const int64_t j = i / 6;
    const int k = (int)(i - j * 6);
    const int64_t row = rows[j];
    const float z = surf_depth[row];
    const float step = (k & 1) ? -h : h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = ray_d[row * 3 + c];
        float x = fmaf(z, d, ray_o[row * 3 + c]);
        if (c == (k >> 1)) x += step;
        pts[i * 3 + c] = x;
        dirs[i * 3 + c] = d;
    }
}

// one thread per listed ray
__global__ __launch_bounds__(GEO_BLOCK) void k_stencil_normals(const float* __restrict__ occ6, const int32_t* __restrict__ rows, int64_t n,
                                                               float* __restrict__ surf_normal, uint8_t* __restrict__ surf_mask) {
    const int64_t j = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (j >= n) return;
    const float* o = occ6 + j * 6;
    const float gx = o[0] - o[1], gy = o[2] - o[3], gz = o[4] - o[5];
    const float n2 = (gx * gx + gy * gy) + gz * gz;
    const int64_t row = rows[j];
    const bool ok = n2 > 0.0f && n2 <= 3.402823466e+38f;       // not 0, not infinite, not a NaN
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (ok) {
        const float len = sqrtf(n2);
        nx = -gx / len; ny = -gy / len; nz = -gz / len;         // the field rises inwards
    }
    surf_normal[row * 3] = nx; surf_normal[row * 3 + 1] = ny; surf_normal[row * 3 + 2] = nz;
    surf_mask[row] = ok ? 1 : 0;
}

static unsigned geo_depth_grid(int64_t n_rays) { return (unsigned)cdiv(n_rays, GEO_BLOCK / 64); }

int launch_geo_depth_merged(const RenderArgs& a, const Workspace& w, const float* z_vals, float level, float* depth_map,
                            int32_t* surf_index, float* surf_depth, hipStream_t st) {
    if (a.R == 0 || !(depth_map || surf_index || surf_depth)) return 0;
    MergedRaw src{w.mask, w.word_off, w.ord_rows > 0 ? w.byte_off : nullptr, w.wsel, w.rgbw, w.cap};
    if ((a.S & 63) == 0) {
        const int G = geo_group(a.S);
        hipLaunchKernelGGL(k_geo_depth_words, dim3(geo_depth_grid(cdiv(a.R, G))), dim3(GEO_BLOCK), 0, st,
                           src, a.near, a.far, z_vals, a.R, a.S, G, a.scene.comp_eps, level, depth_map, surf_index, surf_depth);
        INVR_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(k_geo_depth<MergedRaw>, dim3(geo_depth_grid(a.R)), dim3(GEO_BLOCK), 0, st,
                       src, a.near, a.far, z_vals, a.R, a.S, a.scene.comp_eps, level, depth_map, surf_index, surf_depth);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_depth_fwd(const float* occ, const float* near, const float* far, const float* z_vals, int64_t n_rays, int32_t n_samples,
                              float eps, float level, float* depth_map, int32_t* surf_index, float* surf_depth, void* stream) {
    INVR_CHECK(n_rays >= 0 && n_samples >= 2, "invr_depth_fwd: need n_rays >= 0 and n_samples >= 2");
    INVR_CHECK(isfinite(level) && isfinite(eps), "invr_depth_fwd: level and eps must be finite");
    if (n_rays == 0) return 0;
    INVR_CHECK(occ && (z_vals || (near && far)), "invr_depth_fwd: null occ, or neither z_vals nor near / far");
    INVR_CHECK(n_rays * (int64_t)n_samples < (1ll << 40), "invr_depth_fwd: n_rays * n_samples out of range");
    INVR_CHECK(cdiv(n_rays, GEO_BLOCK / 64) < (1ll << 31), "invr_depth_fwd: too many rays for one launch");
    if (!(depth_map || surf_index || surf_depth)) return 0;
    hipLaunchKernelGGL(k_geo_depth<DenseOcc>, dim3(geo_depth_grid(n_rays)), dim3(GEO_BLOCK), 0, (hipStream_t)stream,
                       DenseOcc{occ}, near, far, z_vals, n_rays, (int)n_samples, eps, level, depth_map, surf_index, surf_depth);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_surface_stencil(const float* ray_o, const float* ray_d, const float* surf_depth, const int32_t* rows, int64_t n, float h,
                                    float* pts, float* dirs, void* stream) {
    INVR_CHECK(n >= 0 && n < (1ll << 31), "invr_surface_stencil: n out of range");
    INVR_CHECK(isfinite(h) && h > 0.0f, "invr_surface_stencil: h must be finite and > 0");
    if (n == 0) return 0;
    INVR_CHECK(ray_o && ray_d && surf_depth && rows && pts && dirs, "invr_surface_stencil: null pointer");
    hipLaunchKernelGGL(k_surface_stencil, dim3((unsigned)cdiv(n * 6, GEO_BLOCK)), dim3(GEO_BLOCK), 0, (hipStream_t)stream,
                       ray_o, ray_d, surf_depth, rows, n, h, pts, dirs);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_stencil_normals(const float* occ6, const int32_t* rows, int64_t n, float* surf_normal, uint8_t* surf_mask, void* stream) {
    INVR_CHECK(n >= 0 && n < (1ll << 31), "invr_stencil_normals: n out of range");
    if (n == 0) return 0;
    INVR_CHECK(occ6 && rows && surf_normal && surf_mask, "invr_stencil_normals: null pointer");
    hipLaunchKernelGGL(k_stencil_normals, dim3((unsigned)cdiv(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, (hipStream_t)stream,
                       occ6, rows, n, surf_normal, surf_mask);
    INVR_LAUNCH_CHECK();
    return 0;
}
