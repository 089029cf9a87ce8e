// The Evaluator's LPIPS (v0.1, net='vgg') on the device (include/invr_lpips.h): the scaling layer, the 13 convolutions of a VGG16 with
// their ReLUs and pools, the five per-tap distances and their sum, for the predicted and the target frame at once.
//
//   k_lp_scale -> conv1_1 -> conv1_2 -> k_lp_dist -> k_lp_pool -> conv2_1 -> conv2_2 -> k_lp_dist -> ... -> conv5_3 -> k_lp_dist -> k_lp_final
//
// The convolution is the implicit GEMM D^T = W . X^T of k_perceptual.hip on v_mfma_f32_16x16x4_f32 (exact fp32), blocked for full
// frames.  A STRIP is 16 pixels, SW x SH of them with SW = min(16, the map's width rounded up to a power of two): narrow late maps
// (conv5 of a 16 x 16 frame is 1 x 1) fold their strips vertically instead of idling 15 of 16 columns.  A workgroup of 4 waves owns a
// tile of 8 strips stacked vertically (16 x 8 pixels on a wide map) and 64 output channels; the input tile with its halo, both images,
// is staged in LDS 16 input channels at a time (the out-of-image halo as true zeros: the padding), and every wave runs 2 images x 2
// strips x 4 channel tiles = 16 MFMAs per K step on 4 weight loads (one packed stream, shared by both images and all strips) and 4
// LDS reads: 0.5 operand fetches per MFMA, 64 accumulator registers.  The small late layers trade some of that blocking for
// workgroups (LP_SPW / LP_CTL below).  K runs over (16-channel chunk, tap, 4-channel step) in the same order for every output
// element, and both images go through identical arithmetic: where they agree on a unit's receptive field the two features are
// bit-identical.  A strip wholly below the image is skipped by its wave (wave-uniform).  K is not split across waves.
// No floating-point atomics: per-workgroup partial sums in float64 at fixed slots, one final pass adding them in a fixed order.
#include "common.h"
#include "../../include/invr_lpips.h"

typedef float lp_f32x4 __attribute__((ext_vector_type(4)));

#define LP_BLOCK 256
#define LP_WAVES (LP_BLOCK / INVR_WAVE)
#define LP_NLAYER 13
#define LP_NTAP 5
// 64-lane rounds that cover the largest staged plane.  With the LP_SPW table below: 2 strips per wave only in blocks 1..3, whose maps are
// at least 4 wide (SW 4: 6 x 34 = 204 positions; SW 8, 16: 180); 1 strip per wave in blocks 4, 5 (SW 1: 3 x 66 = 198; wider: at most 136).
// lp_launch_conv refuses a geometry beyond it.
#define LP_NIT 4
#define LP_DPIX 16           // pixels per workgroup of the distance pass
#define LP_DGRP (LP_BLOCK / LP_DPIX)

static const int LP_CIN[LP_NLAYER] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int LP_COUT[LP_NLAYER] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int LP_BLK[LP_NLAYER] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
static const int LP_TAP[LP_NTAP] = {1, 3, 6, 9, 12};          // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
// Blocking per layer: strips per wave (a workgroup tile is 4 waves x that many strips) and 16-channel tiles per wave.  Blocks 1..3 take
// the full 2 x 4 (with both images 16 MFMAs per K step on 8 operand fetches).  The maps of blocks 4 and 5 are small and their K is long
// (a 512 x 512 frame: 64 x 64 and 32 x 32 pixels x 512 channels): full blocking leaves them 256 and 64 workgroups for 256 CUs, so block 4
// halves the tile and block 5 also halves the channel group — 512 and 256 workgroups — at 0.75 and 1 fetch per MFMA.  The table is
// per layer, not per size, so that every frame size runs every blocking.
static const int LP_SPW[LP_NLAYER] = {2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1};
static const int LP_CTL[LP_NLAYER] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 2, 2, 2};

static inline int lp_cc(int l) { return l == 0 ? 4 : 16; }                         // input channels per staged chunk (conv1_1: 3 padded to 4)
static inline int lp_cin_pad(int l) { return l == 0 ? 4 : LP_CIN[l]; }
static inline int64_t lp_ksteps(int l) { return 9 * (int64_t)lp_cin_pad(l) / 4; }

struct LpPacked { int64_t w[LP_NLAYER], bias[LP_NLAYER], lin[LP_NTAP], shift, scale, total; };      // float offsets into the packed image

static LpPacked lp_packed() {
    LpPacked p;
    int64_t off = 0;
    for (int l = 0; l < LP_NLAYER; ++l) { p.w[l] = off; off += lp_ksteps(l) * (LP_COUT[l] / 16) * 64; }
    for (int l = 0; l < LP_NLAYER; ++l) { p.bias[l] = off; off += LP_COUT[l]; }
    for (int t = 0; t < LP_NTAP; ++t) { p.lin[t] = off; off += LP_COUT[LP_TAP[t]]; }
    p.shift = off; off += 3;
    p.scale = off; off += 3;
    p.total = off;
    return p;
}

// geometry of the convolution's tiles on an h x w map
struct LpGeom { int swl, th, npos, cs, tiles_x, tiles_y; };

static LpGeom lp_geom(int h, int w, int spw) {
    LpGeom g;
    g.swl = 0;
    while ((1 << g.swl) < w && g.swl < 4) ++g.swl;
    const int sw = 1 << g.swl, sh = 16 >> g.swl;
    g.th = sh * LP_WAVES * spw;
    g.npos = (sw + 2) * (g.th + 2);                        // staged positions of one (image, channel) plane: at most 204 <= 64 LP_NIT
    g.cs = (g.npos - 16 + 63) / 64 * 64 + 16;              // plane stride = 16 (mod 32): the four k rows of a ds_read_b32 group fall on distinct banks
    g.tiles_x = (int)cdiv(w, sw);
    g.tiles_y = (int)cdiv(h, g.th);
    return g;
}

static inline int64_t lp_dist_blocks(int64_t hw) { return cdiv(hw, LP_DPIX); }

static void lp_layout(int H, int W, int keep, InvrLpipsLayout* L) {
    size_t off = 0;
    auto take = [&](int64_t count, size_t elem) { const size_t o = off; off = align_up(off + (size_t)count * elem, 256); return (int64_t)o; };
    const int64_t P = (int64_t)H * W;
    L->scaled = take(2 * 3 * P, 4);
    if (keep) {
        for (int l = 0; l < LP_NLAYER; ++l) {
            const int b = LP_BLK[l];
            if (l > 0 && LP_BLK[l - 1] != b) L->pool[b - 1] = take(2 * (int64_t)LP_CIN[l] * (H >> b) * (W >> b), 4);
            L->act[l] = take(2 * (int64_t)LP_COUT[l] * (H >> b) * (W >> b), 4);
        }
    } else {                                               // two buffers of the largest array (64 channels at full size); every stage writes the other one
        const int64_t buf[2] = {take(2 * 64 * P, 4), take(2 * 64 * P, 4)};
        int at = 0;
        for (int l = 0; l < LP_NLAYER; ++l) {
            const int b = LP_BLK[l];
            if (l > 0 && LP_BLK[l - 1] != b) { L->pool[b - 1] = buf[at]; at ^= 1; }
            L->act[l] = buf[at];
            at ^= 1;
        }
    }
    int64_t n = 0;
    for (int t = 0; t < LP_NTAP; ++t) {
        const int b = LP_BLK[LP_TAP[t]];
        L->part_off[t] = n;
        L->n_part[t] = lp_dist_blocks((int64_t)(H >> b) * (W >> b));
        n += L->n_part[t];
    }
    L->n_partial = n;
    L->partial = take(n, 8);
    L->bytes = (int64_t)off;
}

// ---- packing --------------------------------------------------------------------------------------------------------------------
// A-operand stream of a convolution staged CC input channels at a time: element ((ks * tiles + tile) * 64 + lane) is the weight of
// output channel tile * 16 + lane % 16, tap (ks / (CC / 4)) % 9 and input channel (ks / (9 CC / 4)) * CC + 4 (ks % (CC / 4)) + lane / 16
// (0 for conv1_1's padded fourth channel) of torch's (out, in, 3, 3) w.
__global__ void __launch_bounds__(LP_BLOCK) k_lp_pack(const float* __restrict__ w, float* __restrict__ out, int cin, int cc, int tiles, int64_t total) {
    const int spt = cc / 4;
    for (int64_t e = (int64_t)blockIdx.x * LP_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * LP_BLOCK) {
        const int lane = (int)(e & 63);
        const int64_t st = e >> 6;
        const int tile = (int)(st % tiles), ks = (int)(st / tiles);
        const int s = ks % spt, tap = (ks / spt) % 9, chunk = ks / (spt * 9);
        const int ci = chunk * cc + 4 * s + (lane >> 4), o = tile * 16 + (lane & 15);
        out[e] = ci < cin ? w[((int64_t)o * cin + ci) * 9 + tap] : 0.0f;
    }
}

__global__ void __launch_bounds__(LP_BLOCK) k_lp_copy(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- the scaling layer: interleaved (H, W, 3) -> planar [2][3][P] ----------------------------------------------------------------------
__global__ void __launch_bounds__(LP_BLOCK) k_lp_scale(const float* __restrict__ img_pred, const float* __restrict__ img_gt,
                                                       const float* __restrict__ shift, const float* __restrict__ scale, int64_t P,
                                                       float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * LP_BLOCK + threadIdx.x;
    if (pix >= P) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sh = shift[c], sc = scale[c];
        out[(0 * 3 + c) * P + pix] = (img_pred[pix * 3 + c] - sh) / sc;
        out[(1 * 3 + c) * P + pix] = (img_gt[pix * 3 + c] - sh) / sc;
    }
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------
struct LpConvArgs {
    const float* in;         // [2][cin][H*W]
    const float* wp;         // packed A-operand stream
    const float* bias;       // [cout]
    float* out;              // [2][cout][H*W]
    int H, W, cin, cout;
    int swl, spw, npos, cs, tiles_x;
};

// the K steps of one staged chunk for NQ strips of this wave
template <int CC, int CT, int NQ>
__device__ __forceinline__ void lp_chunk(lp_f32x4 (&acc)[2][2][CT], const float* __restrict__ wp, const float* lb, int64_t tiles, int cs,
                                         int lw, int qstride) {
    constexpr int SPT = CC / 4;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const float* lt = lb + (tap / 3) * lw + tap % 3;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            float w[CT], b[2][NQ];
#pragma unroll
            for (int t = 0; t < CT; ++t) w[t] = wp[((int64_t)(tap * SPT + s) * tiles + t) * 64];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int q = 0; q < NQ; ++q) b[n][q] = lt[(n * CC + 4 * s) * cs + q * qstride];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[n][q][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], b[n][q], acc[n][q][t], 0, 0, 0);
        }
    }
}

// CC input channels per staged chunk, CT 16-channel tiles per wave, spw strips per wave (1 or 2).
// grid: (tiles_x * tiles_y, cout / (16 CT)); dynamic LDS: 2 * CC * cs floats
template <int CC, int CT>
__global__ void __launch_bounds__(LP_BLOCK) k_lp_conv(const LpConvArgs a) {
    extern __shared__ float lp_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int sw = 1 << a.swl, sh = 16 >> a.swl, lw = sw + 2;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x), cg = (int)blockIdx.y;
    const int x0 = tx * sw, y0 = ty * (sh * LP_WAVES * a.spw);
    const int64_t HW = (int64_t)a.H * a.W;
    const int tiles = a.cout / 16;
    const int lx = j & (sw - 1), ly = j >> a.swl;
    const int sy0 = y0 + a.spw * wave * sh;                // first row of this wave's strips spw wave (, spw wave + 1)
    const int nact = sy0 >= a.H ? 0 : ((a.spw == 2 && sy0 + sh < a.H) ? 2 : 1);      // (wave-uniform) strips that hold a pixel of the image

    // where this lane's staged positions come from: the same for every plane
    int goff[LP_NIT];
#pragma unroll
    for (int it = 0; it < LP_NIT; ++it) {
        const int pos = it * 64 + lane, ry = pos / lw, rx = pos - ry * lw;
        const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
        goff[it] = (pos < a.npos && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? gy * a.W + gx : -1;
    }

    lp_f32x4 acc[2][2][CT];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[n][q][t][r] = a.bias[(cg * CT + t) * 16 + 4 * kq + r];

    const int nchunk = (a.cin + CC - 1) / CC;
    const float* lb = lp_lds + kq * a.cs + (a.spw * wave * sh + ly) * lw + lx;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();                                   // (the previous chunk has been read)
        for (int p = wave; p < 2 * CC; p += LP_WAVES) {    // plane p = (image, channel of the chunk): out-of-image positions and padded channels are zeros
            const int n = p / CC, ci = chunk * CC + p % CC;
            const bool chan = ci < a.cin;
            const float* src = a.in + (chan ? ((int64_t)n * a.cin + ci) * HW : 0);
            float* dst = lp_lds + p * a.cs;
#pragma unroll
            for (int it = 0; it < LP_NIT; ++it) {
                const int pos = it * 64 + lane;
                if (pos < a.npos) dst[pos] = (chan && goff[it] >= 0) ? src[goff[it]] : 0.0f;
            }
        }
        __syncthreads();
        const float* wp = a.wp + ((int64_t)chunk * 9 * (CC / 4) * tiles + cg * CT) * 64 + lane;
        if (nact == 2) lp_chunk<CC, CT, 2>(acc, wp, lb, tiles, a.cs, lw, sh * lw);
        else if (nact == 1) lp_chunk<CC, CT, 1>(acc, wp, lb, tiles, a.cs, lw, sh * lw);
    }

    // lane (j, kq) holds channels tile * 16 + 4 kq + r of pixel j of each strip
    const int x = x0 + lx;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int y = sy0 + q * sh + ly;
        if (q >= nact || y >= a.H || x >= a.W) continue;  // (q >= nact: with one strip per wave the rows below belong to the next wave)
        const int64_t pix = (int64_t)y * a.W + x;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = (cg * CT + t) * 16 + 4 * kq + r;
                    const float v = acc[n][q][t][r];
                    a.out[((int64_t)n * a.cout + co) * HW + pix] = v > 0.0f ? v : 0.0f;
                }
    }
}

// ---- 2x2 max-pool (floor), both images -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LP_BLOCK) k_lp_pool(const float* __restrict__ in, float* __restrict__ out, int H, int W, int64_t total) {
    const int h = H / 2, w = W / 2;
    for (int64_t e = (int64_t)blockIdx.x * LP_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * LP_BLOCK) {
        const int xx = (int)(e % w), yy = (int)((e / w) % h);
        const int64_t plane = e / ((int64_t)w * h);
        const float* s = in + plane * H * W + (int64_t)(2 * yy) * W + 2 * xx;
        out[e] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
    }
}

// ---- the distance of one tap, float64 ---------------------------------------------------------------------------------------------------
// A workgroup owns LP_DPIX pixels; thread (pixel, group) takes the channels group, group + 16, ... of its pixel (the late taps have few
// pixels and 512 channels: a pixel per thread leaves the chip idle behind a chain of 512 divisions).  The groups' sums meet in LDS and are
// added in the order of the groups; one slot per workgroup.
__global__ void __launch_bounds__(LP_BLOCK) k_lp_dist(const float* __restrict__ feat, const float* __restrict__ lin, int C, int64_t hw,
                                                      double* __restrict__ partial) {
    __shared__ double s_s[2][LP_DGRP][LP_DPIX];
    __shared__ double s_d[LP_DGRP][LP_DPIX];
    const int px = threadIdx.x % LP_DPIX, grp = threadIdx.x / LP_DPIX;
    const int64_t pix = (int64_t)blockIdx.x * LP_DPIX + px;
    const bool valid = pix < hw;
    const float* f0 = feat + (valid ? pix : 0);
    const float* f1 = f0 + (int64_t)C * hw;
    double s0 = 0.0, s1 = 0.0;
    if (valid)
        for (int c = grp; c < C; c += LP_DGRP) {
            const double x0 = (double)f0[(int64_t)c * hw], x1 = (double)f1[(int64_t)c * hw];
            s0 += x0 * x0;
            s1 += x1 * x1;
        }
    s_s[0][grp][px] = s0;
    s_s[1][grp][px] = s1;
    __syncthreads();
    s0 = s1 = 0.0;
    for (int g = 0; g < LP_DGRP; ++g) { s0 += s_s[0][g][px]; s1 += s_s[1][g][px]; }
    const double r0 = sqrt(s0) + (double)1e-10f, r1 = sqrt(s1) + (double)1e-10f;
    double d = 0.0;
    if (valid)
        for (int c = grp; c < C; c += LP_DGRP) {
            const double n0 = (double)f0[(int64_t)c * hw] / r0, n1 = (double)f1[(int64_t)c * hw] / r1;
            const double df = n0 - n1;
            d += (double)lin[c] * (df * df);
        }
    s_d[grp][px] = d;
    __syncthreads();
    if (threadIdx.x < LP_DPIX) {
        d = 0.0;
        for (int g = 0; g < LP_DGRP; ++g) d += s_d[g][threadIdx.x];
        s_d[0][threadIdx.x] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        d = 0.0;
        for (int p = 0; p < LP_DPIX; ++p) d += s_d[0][p];
        partial[blockIdx.x] = d;
    }
}

// ---- the sums -> out8 (one workgroup) ----------------------------------------------------------------------------------------------------
struct LpFinalArgs { int64_t off[LP_NTAP], n[LP_NTAP], hw[LP_NTAP]; };

__global__ void __launch_bounds__(LP_BLOCK) k_lp_final(const double* __restrict__ partial, const LpFinalArgs a, double* __restrict__ out8) {
    __shared__ double s_red[LP_WAVES];
    double layer[LP_NTAP];
#pragma unroll
    for (int t = 0; t < LP_NTAP; ++t) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < a.n[t]; i += LP_BLOCK) s += partial[a.off[t] + i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        __syncthreads();                                   // (s_red of the previous tap has been read)
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
        __syncthreads();
        s = 0.0;
        for (int k = 0; k < LP_WAVES; ++k) s += s_red[k];
        layer[t] = s / (double)a.hw[t];
    }
    if (threadIdx.x == 0) {
        out8[0] = (((layer[0] + layer[1]) + layer[2]) + layer[3]) + layer[4];
#pragma unroll
        for (int t = 0; t < LP_NTAP; ++t) out8[1 + t] = layer[t];
        out8[6] = 0.0;
        out8[7] = 0.0;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned lp_grid(int64_t n) { const int64_t b = cdiv(n > 0 ? n : 1, LP_BLOCK); return (unsigned)(b < 4096 ? b : 4096); }
template <class T> static inline T* lp_at(void* ws, int64_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

extern "C" int64_t invr_lpips_packed_floats(void) { return lp_packed().total; }

extern "C" int invr_lpips_pack_weights(const float* const* w, const float* const* b, const float* const* lin, const float* shift3,
                                       const float* scale3, float* packed, void* stream) {
    INVR_CHECK(w && b && lin && shift3 && scale3 && packed, "invr_lpips_pack_weights: null pointer");
    for (int l = 0; l < LP_NLAYER; ++l) INVR_CHECK(w[l] && b[l], "invr_lpips_pack_weights: null weight / bias pointer of layer %d", l);
    for (int t = 0; t < LP_NTAP; ++t) INVR_CHECK(lin[t], "invr_lpips_pack_weights: null lin pointer of tap %d", t);
    const LpPacked p = lp_packed();
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < LP_NLAYER; ++l) {
        const int64_t nf = lp_ksteps(l) * (LP_COUT[l] / 16) * 64;
        hipLaunchKernelGGL(k_lp_pack, dim3(lp_grid(nf)), dim3(LP_BLOCK), 0, st, w[l], packed + p.w[l], LP_CIN[l], lp_cc(l), LP_COUT[l] / 16, nf);
        INVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_lp_copy, dim3(lp_grid(LP_COUT[l])), dim3(LP_BLOCK), 0, st, b[l], packed + p.bias[l], LP_COUT[l]);
        INVR_LAUNCH_CHECK();
    }
    for (int t = 0; t < LP_NTAP; ++t) {
        const int c = LP_COUT[LP_TAP[t]];
        hipLaunchKernelGGL(k_lp_copy, dim3(lp_grid(c)), dim3(LP_BLOCK), 0, st, lin[t], packed + p.lin[t], c);
        INVR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_lp_copy, dim3(1), dim3(LP_BLOCK), 0, st, shift3, packed + p.shift, 3);
    INVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lp_copy, dim3(1), dim3(LP_BLOCK), 0, st, scale3, packed + p.scale, 3);
    INVR_LAUNCH_CHECK();
    return 0;
}

static inline bool lp_size_ok(int32_t H, int32_t W) {
    return H >= INVR_LPIPS_MIN_SIDE && W >= INVR_LPIPS_MIN_SIDE && H <= INVR_LPIPS_MAX_SIDE && W <= INVR_LPIPS_MAX_SIDE;
}

extern "C" size_t invr_lpips_workspace_bytes(int32_t H, int32_t W, int32_t keep) {
    if (!lp_size_ok(H, W)) return 0;
    InvrLpipsLayout L;
    lp_layout(H, W, keep, &L);
    if (keep && L.bytes > INVR_LPIPS_KEEP_MAX_BYTES) return 0;
    return (size_t)L.bytes;
}

extern "C" int invr_lpips_workspace_layout(int32_t H, int32_t W, int32_t keep, InvrLpipsLayout* layout) {
    INVR_CHECK(layout, "invr_lpips_workspace_layout: null layout");
    INVR_CHECK(lp_size_ok(H, W), "invr_lpips_workspace_layout: H, W must be in [%d, %d] (got %d x %d)", INVR_LPIPS_MIN_SIDE, INVR_LPIPS_MAX_SIDE,
               H, W);
    InvrLpipsLayout L;
    lp_layout(H, W, keep, &L);
    INVR_CHECK(!keep || L.bytes <= INVR_LPIPS_KEEP_MAX_BYTES, "invr_lpips_workspace_layout: a keep = 1 layout of %d x %d exceeds %lld bytes", H, W,
               (long long)INVR_LPIPS_KEEP_MAX_BYTES);
    *layout = L;
    return 0;
}

static int lp_launch_conv(int l, const float* packed, const LpPacked& pk, const float* in, float* out, int h, int w, hipStream_t st) {
    const LpGeom g = lp_geom(h, w, LP_SPW[l]);
    LpConvArgs a;
    a.in = in; a.wp = packed + pk.w[l]; a.bias = packed + pk.bias[l]; a.out = out;
    a.H = h; a.W = w; a.cin = LP_CIN[l]; a.cout = LP_COUT[l];
    INVR_CHECK(g.npos <= 64 * LP_NIT, "invr_lpips_fwd: layer %d stages %d positions per plane, the kernel covers %d", l, g.npos, 64 * LP_NIT);
    a.swl = g.swl; a.spw = LP_SPW[l]; a.npos = g.npos; a.cs = g.cs; a.tiles_x = g.tiles_x;
    const dim3 grid((unsigned)(g.tiles_x * g.tiles_y), (unsigned)(LP_COUT[l] / (16 * LP_CTL[l])));
    if (l == 0) hipLaunchKernelGGL((k_lp_conv<4, 4>), grid, dim3(LP_BLOCK), (size_t)2 * 4 * g.cs * sizeof(float), st, a);
    else if (LP_CTL[l] == 4) hipLaunchKernelGGL((k_lp_conv<16, 4>), grid, dim3(LP_BLOCK), (size_t)2 * 16 * g.cs * sizeof(float), st, a);
    else hipLaunchKernelGGL((k_lp_conv<16, 2>), grid, dim3(LP_BLOCK), (size_t)2 * 16 * g.cs * sizeof(float), st, a);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_lpips_fwd(const float* packed, const float* img_pred, const float* img_gt, int32_t H, int32_t W, int32_t keep, void* workspace,
                              size_t workspace_bytes, double* out8, void* stream) {
    INVR_CHECK(lp_size_ok(H, W), "invr_lpips_fwd: H, W must be in [%d, %d] (got %d x %d)", INVR_LPIPS_MIN_SIDE, INVR_LPIPS_MAX_SIDE, H, W);
    INVR_CHECK(packed && img_pred && img_gt && workspace && out8, "invr_lpips_fwd: null packed weights / image / workspace / out8 pointer");
    INVR_CHECK(((uintptr_t)workspace & 255) == 0, "invr_lpips_fwd: the workspace must be 256-byte aligned");
    const size_t need = invr_lpips_workspace_bytes(H, W, keep);
    INVR_CHECK(need > 0, "invr_lpips_fwd: a keep = 1 layout of %d x %d exceeds %lld bytes", H, W, (long long)INVR_LPIPS_KEEP_MAX_BYTES);
    INVR_CHECK(workspace_bytes >= need, "invr_lpips_fwd: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    InvrLpipsLayout L;
    lp_layout(H, W, keep, &L);
    const LpPacked pk = lp_packed();
    const int64_t P = (int64_t)H * W;
    double* partial = lp_at<double>(workspace, L.partial);
    hipLaunchKernelGGL(k_lp_scale, dim3((unsigned)cdiv(P, LP_BLOCK)), dim3(LP_BLOCK), 0, st, img_pred, img_gt, packed + pk.shift, packed + pk.scale, P,
                       lp_at<float>(workspace, L.scaled));
    INVR_LAUNCH_CHECK();
    LpFinalArgs fa;
    const float* cur = lp_at<float>(workspace, L.scaled);
    int tap = 0;
    for (int l = 0; l < LP_NLAYER; ++l) {
        const int b = LP_BLK[l], h = H >> b, w = W >> b;
        if (l > 0 && LP_BLK[l - 1] != b) {
            float* pooled = lp_at<float>(workspace, L.pool[b - 1]);
            const int64_t total = 2 * (int64_t)LP_CIN[l] * h * w;
            hipLaunchKernelGGL(k_lp_pool, dim3(lp_grid(total)), dim3(LP_BLOCK), 0, st, cur, pooled, H >> (b - 1), W >> (b - 1), total);
            INVR_LAUNCH_CHECK();
            cur = pooled;
        }
        float* out = lp_at<float>(workspace, L.act[l]);
        if (lp_launch_conv(l, packed, pk, cur, out, h, w, st)) return 1;
        cur = out;
        if (l == LP_TAP[tap]) {
            const int64_t hw = (int64_t)h * w;
            hipLaunchKernelGGL(k_lp_dist, dim3((unsigned)lp_dist_blocks(hw)), dim3(LP_BLOCK), 0, st, cur, packed + pk.lin[tap], LP_COUT[l], hw,
                               partial + L.part_off[tap]);
            INVR_LAUNCH_CHECK();
            fa.off[tap] = L.part_off[tap]; fa.n[tap] = L.n_part[tap]; fa.hw[tap] = hw;
            ++tap;
        }
    }
    hipLaunchKernelGGL(k_lp_final, dim3(1), dim3(LP_BLOCK), 0, st, partial, fa, out8);
    INVR_LAUNCH_CHECK();
    return 0;
}
