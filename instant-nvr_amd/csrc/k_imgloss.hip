// The SSIM (cfg.use_ssim) and total-variation (cfg.use_tv_image) image terms of the training objective (include/invr_imgloss.h): the
// term's forward over the patch re-assembled from mask_at_box, its backward to the predicted patch only, gathered back to the rays.
//
//   SSIM forward : launch_patch_assemble -> k_ssim_map (five moments, S, p / q / r, per-workgroup sums of S) -> k_imgloss_final
//        backward: k_ssim_grad ((G*p) + 2 x (G*q) + y (G*r), scattered to the rays)
//   TV   forward : launch_patch_assemble -> k_tv_max (mask_gt + the target's maxima) -> k_tv_sum -> k_imgloss_final
//        backward: k_tv_grad (a gather over the four differences a pixel takes part in)
//   the objective's twins run k_train_loss_term in the place of k_imgloss_final (the same final sums, then k_train_loss's arithmetic)
//   and hand their backward kernel the regularisers' gradients to write as well: 3 + 1 launches for SSIM, 4 + 1 for TV.
//
// The Gaussian window is separable: a workgroup owns a 16 x 16 tile of one channel, stages the tile with its halo of w / 2 in LDS,
// filters the rows of all five moments from the two staged images (the products x^2, y^2, xy are formed on the fly: no round trip per
// map), then the columns.  A 64 x 64 x 3 patch is 48 workgroups; every array is L2-resident and the pass is launch-latency bound.
// No floating-point atomics: per-workgroup partial sums in float64 at fixed slots of the workspace, added in a fixed order.
#include "common.h"
#include "train.h"
#include "../../include/invr_imgloss.h"

#define IL_TS 16                                        // side of a workgroup's output tile
#define IL_HMAX (INVR_IMGLOSS_MAX_WINDOW / 2)
#define IL_R (IL_TS + 2 * IL_HMAX)                      // rows / columns of a staged tile with the widest halo
#define IL_RS (IL_R + 1)                                // its row stride in LDS
#define IL_BLOCK 256
#define IL_WAVES (IL_BLOCK / INVR_WAVE)
#define IL_TV_MAX_BLOCKS 1024
#define IL_C1 ((float)(0.01 * 0.01))
#define IL_C2 ((float)(0.03 * 0.03))

enum { IL_SSIM = 0, IL_TV = 1 };

static inline bool il_size_ok(int32_t H, int32_t W, int32_t w) {
    return H >= 2 && W >= 2 && H <= INVR_IMGLOSS_MAX_SIDE && W <= INVR_IMGLOSS_MAX_SIDE && w >= 1 && w <= INVR_IMGLOSS_MAX_WINDOW && (w & 1);
}

static void il_layout(int H, int W, InvrImglossLayout* L) {
    const int64_t P = (int64_t)H * W;
    size_t off = 0;
    auto take = [&](int64_t count, size_t elem) { const size_t o = off; off = align_up(off + (size_t)count * elem, 256); return (int64_t)o; };
    L->n_ssim = cdiv(W, IL_TS) * cdiv(H, IL_TS) * 3;
    L->n_tv = cdiv(P, IL_BLOCK) < IL_TV_MAX_BLOCKS ? cdiv(P, IL_BLOCK) : IL_TV_MAX_BLOCKS;
    L->n_partial = (L->n_ssim > 4 * L->n_tv ? L->n_ssim : 4 * L->n_tv) + 2;
    L->rank = take(P, 4);
    L->img = take(2 * 3 * P, 4);
    L->mom = take(5 * 3 * P, 4);
    L->smap = take(3 * P, 4);
    L->pqr = take(3 * 3 * P, 4);
    L->occ = take(P, 1);
    L->tvmax = take(2 * L->n_tv, 4);
    L->partial = take(L->n_partial, 8);
    L->out8 = take(8, 4);
    L->gimg = take(3 * P, 4);
    L->bytes = (int64_t)off;
}

// the regularisers' share of the objective's backward (k_train_loss_bwd's g_dist / g_terms), written by the term's backward kernel
struct IlReg {
    const float* terms;
    float* g_dist;
    float* g_terms;          // NULL: the term alone
    int64_t n;
    float w_pair, w_dist, w_off;
    int use_pair;
};

__device__ __forceinline__ void il_reg_bwd(const IlReg& r, float gl, int64_t block, int64_t blocks) {
    if (!r.g_terms) return;
    const float k_dist = r.n > 0 ? gl * r.w_dist / (float)r.n : 0.0f;
    if (r.g_dist)
        for (int64_t i = block * IL_BLOCK + threadIdx.x; i < r.n; i += blocks * IL_BLOCK) r.g_dist[i] = k_dist;
    if (block == 0 && threadIdx.x < TERM_LEN) {
        float g = 0.0f;
        if (threadIdx.x == TERM_OFFSET_SUM) g = gl * r.w_off / fmaxf(r.terms[TERM_OFFSET_ROWS], 1.0f);
        if (threadIdx.x == TERM_PAIR_SUM && r.use_pair) g = gl * r.w_pair / fmaxf(r.terms[TERM_PAIR_ROWS], 1.0f);
        r.g_terms[threadIdx.x] = g;
    }
}

// sum over the workgroup (every thread takes part; blockDim.x a multiple of 64, at most 1024) -> the total in every thread
__device__ __forceinline__ double il_block_sum(double s, double* s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    __syncthreads();                                       // (s_red of the previous sum has been read)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
    __syncthreads();
    s = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += s_red[k];
    return s;
}

__device__ __forceinline__ float il_block_max(float m, float* s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) m = fmaxf(m, s_red[k]);
    return m;
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------
// stage the R x R tile (R = 16 + 2 h) of PLANES maps around the workgroup's tile, zeros outside the image
template <int PLANES>
__device__ __forceinline__ void il_stage(const float* const* src, float* s_in, int h, int x0, int y0, int H, int W) {
    const int R = IL_TS + 2 * h;
    for (int e = threadIdx.x; e < R * R; e += IL_BLOCK) {
        const int ry = e / R, rx = e - ry * R, yy = y0 + ry - h, xx = x0 + rx - h;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = in ? (int64_t)yy * W + xx : 0;
#pragma unroll
        for (int m = 0; m < PLANES; ++m) s_in[m * (IL_R * IL_RS) + ry * IL_RS + rx] = in ? src[m][o] : 0.0f;
    }
}

// img [2][3][P] -> mom [5][3][P], smap [3][P], pqr [3][3][P], partial[workgroup] = the tile's sum of S.  grid (tiles x, tiles y, 3)
__global__ void __launch_bounds__(IL_BLOCK) k_ssim_map(const float* __restrict__ img, const float* __restrict__ taps, int w, int H, int W,
                                                       float* __restrict__ mom, float* __restrict__ smap, float* __restrict__ pqr,
                                                       double* __restrict__ partial) {
    __shared__ float s_g[INVR_IMGLOSS_MAX_WINDOW + 1];
    __shared__ float s_in[2 * IL_R * IL_RS];
    __shared__ float s_row[5][IL_R * IL_TS];
    __shared__ double s_red[IL_WAVES];
    const int tid = threadIdx.x, h = w >> 1, R = IL_TS + 2 * h;
    const int c = blockIdx.z, x0 = blockIdx.x * IL_TS, y0 = blockIdx.y * IL_TS;
    const int64_t P = (int64_t)H * W;
    if (tid < w) s_g[tid] = taps[tid];
    const float* src[2] = {img + (int64_t)c * P, img + (int64_t)(3 + c) * P};
    il_stage<2>(src, s_in, h, x0, y0, H, W);
    __syncthreads();
    for (int e = tid; e < R * IL_TS; e += IL_BLOCK) {             // rows: the five moments of row ry at the tile's 16 columns
        const int ry = e / IL_TS, tx = e % IL_TS;
        const float* px = s_in + ry * IL_RS + tx;
        const float* py = px + IL_R * IL_RS;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f;
        for (int k = 0; k < w; ++k) {
            const float g = s_g[k], x = px[k], y = py[k];
            a0 = fmaf(g, x, a0);
            a1 = fmaf(g, y, a1);
            a2 = fmaf(g, x * x, a2);
            a3 = fmaf(g, y * y, a3);
            a4 = fmaf(g, x * y, a4);
        }
        s_row[0][e] = a0; s_row[1][e] = a1; s_row[2][e] = a2; s_row[3][e] = a3; s_row[4][e] = a4;
    }
    __syncthreads();
    const int ty = tid / IL_TS, tx = tid % IL_TS, yy = y0 + ty, xx = x0 + tx;
    float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < w; ++k) {                                 // columns
        const float g = s_g[k];
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] = fmaf(g, s_row[j][(ty + k) * IL_TS + tx], m[j]);
    }
    double sum = 0.0;
    if (yy < H && xx < W) {
        const float a = m[0], b = m[1];
        const float ab = a * b, aa = a * a, bb = b * b;
        const float n1 = 2.0f * ab + IL_C1, n2 = 2.0f * (m[4] - ab) + IL_C2;
        const float d1 = (aa + bb) + IL_C1, d2 = ((m[2] - aa) + (m[3] - bb)) + IL_C2;
        const float den = d1 * d2;
        const float S = (n1 * n2) / den;
        const float p = ((2.0f * b) * (n2 - n1)) / den + ((2.0f * a) * S) * (1.0f / d2 - 1.0f / d1);
        const float q = -(S / d2);
        const float r = (2.0f * n1) / den;
        const int64_t o = (int64_t)c * P + (int64_t)yy * W + xx;
#pragma unroll
        for (int j = 0; j < 5; ++j) mom[(int64_t)j * 3 * P + o] = m[j];
        smap[o] = S;
        pqr[o] = p;
        pqr[3 * P + o] = q;
        pqr[6 * P + o] = r;
        sum = (double)S;
    }
    sum = il_block_sum(sum, s_red);
    if (tid == 0) partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

// gimg = ((G*p) + 2 x (G*q) + y (G*r)) * g_loss * scale / (3 P); g_rgb[rank] = gimg (+ the MSE's gradient when k_mse2: the objective)
__global__ void __launch_bounds__(IL_BLOCK) k_ssim_grad(const float* __restrict__ img, const float* __restrict__ pqr, const float* __restrict__ taps,
                                                        int w, int H, int W, const int32_t* __restrict__ rank, const float* __restrict__ g_loss,
                                                        float scale, int with_mse, float* __restrict__ gimg, float* __restrict__ g_rgb,
                                                        const IlReg reg) {
    __shared__ float s_g[INVR_IMGLOSS_MAX_WINDOW + 1];
    __shared__ float s_in[3 * IL_R * IL_RS];
    __shared__ float s_row[3][IL_R * IL_TS];
    const int tid = threadIdx.x, h = w >> 1, R = IL_TS + 2 * h;
    const int c = blockIdx.z, x0 = blockIdx.x * IL_TS, y0 = blockIdx.y * IL_TS;
    const int64_t P = (int64_t)H * W;
    const float gl = g_loss[0];
    il_reg_bwd(reg, gl, ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, (int64_t)gridDim.x * gridDim.y * gridDim.z);
    if (tid < w) s_g[tid] = taps[tid];
    const float* src[3] = {pqr + (int64_t)c * P, pqr + (int64_t)(3 + c) * P, pqr + (int64_t)(6 + c) * P};
    il_stage<3>(src, s_in, h, x0, y0, H, W);
    __syncthreads();
    for (int e = tid; e < R * IL_TS; e += IL_BLOCK) {
        const int ry = e / IL_TS, tx = e % IL_TS;
        const float* pp = s_in + ry * IL_RS + tx;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int k = 0; k < w; ++k) {
            const float g = s_g[k];
            a0 = fmaf(g, pp[k], a0);
            a1 = fmaf(g, pp[IL_R * IL_RS + k], a1);
            a2 = fmaf(g, pp[2 * IL_R * IL_RS + k], a2);
        }
        s_row[0][e] = a0; s_row[1][e] = a1; s_row[2][e] = a2;
    }
    __syncthreads();
    const int ty = tid / IL_TS, tx = tid % IL_TS, yy = y0 + ty, xx = x0 + tx;
    float m[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < w; ++k) {
        const float g = s_g[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j] = fmaf(g, s_row[j][(ty + k) * IL_TS + tx], m[j]);
    }
    if (yy < H && xx < W) {
        const int64_t pix = (int64_t)yy * W + xx, o = (int64_t)c * P + pix;
        const float x = img[o], y = img[3 * P + o];
        const float kk = (gl * scale) / (float)(3 * P);
        const float g = ((m[0] + (2.0f * x) * m[1]) + y * m[2]) * kk;
        gimg[o] = g;
        const int32_t rk = rank[pix];
        if (rk >= 0) {
            const float k_img = reg.n > 0 ? gl * 2.0f / (float)(3 * reg.n) : 0.0f;
            g_rgb[(int64_t)rk * 3 + c] = with_mse ? k_img * (x - y) + g : g;
        }
    }
}

// ---- TV ------------------------------------------------------------------------------------------------------------------------------
// mask_gt (a gather through the rank array) and the per-workgroup maxima of the target's squared differences
__global__ void __launch_bounds__(IL_BLOCK) k_tv_max(const float* __restrict__ img, const int32_t* __restrict__ rank, const uint8_t* __restrict__ occupancy,
                                                     int H, int W, uint8_t* __restrict__ occ, float* __restrict__ tvmax) {
    __shared__ float s_red[IL_WAVES];
    const int64_t P = (int64_t)H * W;
    const float* gt = img + 3 * P;
    float mx = 0.0f, my = 0.0f;
    for (int64_t pix = (int64_t)blockIdx.x * IL_BLOCK + threadIdx.x; pix < P; pix += (int64_t)gridDim.x * IL_BLOCK) {
        const int32_t rk = rank[pix];
        occ[pix] = (rk >= 0 && occupancy[rk] != 0) ? 1 : 0;
        const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = gt[c * P + pix];
            if (y < H - 1) { const float d = v - gt[c * P + pix + W]; mx = fmaxf(mx, d * d); }
            if (x < W - 1) { const float d = v - gt[c * P + pix + 1]; my = fmaxf(my, d * d); }
        }
    }
    mx = il_block_max(mx, s_red);
    my = il_block_max(my, s_red);
    if (threadIdx.x == 0) { tvmax[blockIdx.x] = mx; tvmax[gridDim.x + blockIdx.x] = my; }
}

// eps_x, eps_y = the maxima over the n workgroups of k_tv_max (a maximum does not depend on the order)
__device__ __forceinline__ void il_tv_eps(const float* __restrict__ tvmax, int64_t n, float* s_red, float* ex, float* ey) {
    float mx = 0.0f, my = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) { mx = fmaxf(mx, tvmax[i]); my = fmaxf(my, tvmax[n + i]); }
    *ex = il_block_max(mx, s_red);
    *ey = il_block_max(my, s_red);
}

__global__ void __launch_bounds__(IL_BLOCK) k_tv_sum(const float* __restrict__ img, const uint8_t* __restrict__ occ, const float* __restrict__ tvmax,
                                                     int H, int W, double* __restrict__ partial) {
    __shared__ float s_redf[IL_WAVES];
    __shared__ double s_red[IL_WAVES];
    const int64_t P = (int64_t)H * W, nb = gridDim.x;
    float ex, ey;
    il_tv_eps(tvmax, nb, s_redf, &ex, &ey);
    double sx = 0.0, sy = 0.0, kx = 0.0, ky = 0.0;
    for (int64_t pix = (int64_t)blockIdx.x * IL_BLOCK + threadIdx.x; pix < P; pix += nb * IL_BLOCK) {
        if (!occ[pix]) continue;
        const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
        if (y < H - 1) kx += 1.0;
        if (x < W - 1) ky += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = img[c * P + pix];
            if (y < H - 1) { const float d = v - img[c * P + pix + W]; const float t = d * d - ex; if (t > 0.0f) sx += (double)t; }
            if (x < W - 1) { const float d = v - img[c * P + pix + 1]; const float t = d * d - ey; if (t > 0.0f) sy += (double)t; }
        }
    }
    sx = il_block_sum(sx, s_red);
    sy = il_block_sum(sy, s_red);
    kx = il_block_sum(kx, s_red);
    ky = il_block_sum(ky, s_red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sx; partial[nb + blockIdx.x] = sy; partial[2 * nb + blockIdx.x] = kx; partial[3 * nb + blockIdx.x] = ky;
    }
}

// out8 of the workspace = {tv, mean_x, mean_y, eps_x, eps_y, k_x, k_y, 0}: a pixel's gradient gathers the (up to) four differences it is in
__global__ void __launch_bounds__(IL_BLOCK) k_tv_grad(const float* __restrict__ img, const uint8_t* __restrict__ occ, const float* __restrict__ out_ws,
                                                      int H, int W, const int32_t* __restrict__ rank, const float* __restrict__ g_loss, float scale,
                                                      int with_mse, float* __restrict__ gimg, float* __restrict__ g_rgb, const IlReg reg) {
    const int64_t P = (int64_t)H * W;
    const float gl = g_loss[0];
    il_reg_bwd(reg, gl, blockIdx.x, gridDim.x);
    const float ex = out_ws[3], ey = out_ws[4];
    const float cx = (gl * scale) / (3.0f * out_ws[5]), cy = (gl * scale) / (3.0f * out_ws[6]);      // (inf when k = 0: never used then)
    const float k_img = reg.n > 0 ? gl * 2.0f / (float)(3 * reg.n) : 0.0f;
    for (int64_t pix = (int64_t)blockIdx.x * IL_BLOCK + threadIdx.x; pix < P; pix += (int64_t)gridDim.x * IL_BLOCK) {
        const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
        const bool here = occ[pix] != 0, up = y > 0 && occ[pix - W] != 0, left = x > 0 && occ[pix - 1] != 0;
        const int32_t rk = rank[pix];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = img + c * P + pix;
            const float v = p[0];
            float g = 0.0f;
            if (here && y < H - 1) { const float d = v - p[W]; if (d * d - ex > 0.0f) g = g + cx * d; }
            if (up) { const float d = p[-W] - v; if (d * d - ex > 0.0f) g = g - cx * d; }
            if (here && x < W - 1) { const float d = v - p[1]; if (d * d - ey > 0.0f) g = g + cy * d; }
            if (left) { const float d = p[-1] - v; if (d * d - ey > 0.0f) g = g - cy * d; }
            gimg[c * P + pix] = g;
            if (rk >= 0) g_rgb[(int64_t)rk * 3 + c] = with_mse ? k_img * (v - p[3 * P]) + g : g;
        }
    }
}

// ---- the final sums --------------------------------------------------------------------------------------------------------------------
// every thread of the workgroup takes part; the term's out8 goes to the workspace (and to out8 when given); -> the term in every thread
__device__ __forceinline__ float il_finish(int mode, const double* __restrict__ partial, const float* __restrict__ tvmax, int64_t n, int64_t P,
                                           double* s_red, float* s_redf, float* __restrict__ out_ws, float* __restrict__ out8) {
    float o[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int groups = mode == IL_SSIM ? 1 : 4;
    for (int k = 0; k < groups; ++k) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += partial[k * n + i];
        acc[k] = il_block_sum(s, s_red);
    }
    if (mode == IL_SSIM) {
        o[0] = (float)(acc[0] / (double)(3 * P));               // the mean in float64, rounded to fp32 once
        o[1] = 1.0f - o[0];
    } else {
        float ex, ey;
        il_tv_eps(tvmax, n, s_redf, &ex, &ey);
        const double mx = acc[0] / (3.0 * acc[2]), my = acc[1] / (3.0 * acc[3]);      // 0 / 0 = NaN: the mean of an empty selection
        o[0] = (float)((mx + my) / 2.0); o[1] = (float)mx; o[2] = (float)my; o[3] = ex; o[4] = ey; o[5] = (float)acc[2]; o[6] = (float)acc[3];
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 8; ++k) {
            out_ws[k] = o[k];
            if (out8) out8[k] = o[k];
        }
    return o[0];
}

__global__ void __launch_bounds__(IL_BLOCK) k_imgloss_final(int mode, const double* __restrict__ partial, const float* __restrict__ tvmax, int64_t n,
                                                            int64_t P, float* __restrict__ out_ws, float* __restrict__ out8) {
    __shared__ double s_red[IL_WAVES];
    __shared__ float s_redf[IL_WAVES];
    il_finish(mode, partial, tvmax, n, P, s_red, s_redf, out_ws, out8);
}

// the whole objective's scalar part: k_train_loss of k_train.hip (the same loops, the same arithmetic for out[1..5]) with the term added
// as the reference adds it: loss += (0.1 (1 - ssim) + img_loss) | (0.01 tv + img_loss).  out[6] = 1 - ssim | tv
__global__ __launch_bounds__(1024) void k_train_loss_term(int mode, const double* __restrict__ partial, const float* __restrict__ tvmax, int64_t np,
                                                          int64_t P, float* __restrict__ out_ws, const float* __restrict__ rgb,
                                                          const float* __restrict__ gt, const float* __restrict__ dist, const float* __restrict__ terms,
                                                          int64_t n, float w_pair, float w_dist, float w_off, int use_pair, float* __restrict__ out,
                                                          float* __restrict__ err) {
    __shared__ double red[2][1024 / 64];
    __shared__ double s_red[1024 / 64];
    __shared__ float s_redf[1024 / 64];
    const float term = il_finish(mode, partial, tvmax, np, P, s_red, s_redf, out_ws, nullptr);
    double s2 = 0.0, sd = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        float e = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float d = rgb[i * 3 + c] - gt[i * 3 + c]; s2 += (double)(d * d); e += fabsf(d); }
        if (err) err[i] = e;
        if (dist) sd += (double)dist[i];
    }
    for (int d = 32; d >= 1; d >>= 1) { s2 += __shfl_xor(s2, d); sd += __shfl_xor(sd, d); }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[0][wv] = s2; red[1][wv] = sd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s2 = sd = 0.0;
        for (int k = 0; k < 1024 / 64; ++k) { s2 += red[0][k]; sd += red[1][k]; }
        const float img = n > 0 ? (float)(s2 / (double)(3 * n)) : 0.0f;
        const float rd = (dist && n > 0) ? (float)(sd / (double)n) : 0.0f;
        const float off = terms[TERM_OFFSET_SUM] / fmaxf(terms[TERM_OFFSET_ROWS], 1.0f);
        const float pair = use_pair ? terms[TERM_PAIR_SUM] / fmaxf(terms[TERM_PAIR_ROWS], 1.0f) : 0.0f;
        const float t = mode == IL_SSIM ? 1.0f - term : term;
        float loss = 0.0f;
        if (use_pair) loss = loss + w_pair * pair;
        if (dist) loss = loss + w_dist * rd;
        loss = loss + w_off * off;
        loss = loss + ((mode == IL_SSIM ? 0.1f : 0.01f) * t + img);
        out[0] = loss; out[1] = img; out[2] = -10.0f * logf(img) / 2.302585092994046f; out[3] = rd; out[4] = off; out[5] = pair;
        out[6] = t; out[7] = 0.0f;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
template <class T> static inline T* il_at(void* ws, int64_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

extern "C" size_t invr_imgloss_workspace_bytes(int32_t H, int32_t W, int32_t window) {
    if (!il_size_ok(H, W, window)) return 0;
    InvrImglossLayout L;
    il_layout(H, W, &L);
    return (size_t)L.bytes;
}

extern "C" int invr_imgloss_workspace_layout(int32_t H, int32_t W, int32_t window, InvrImglossLayout* layout) {
    INVR_CHECK(layout, "invr_imgloss_workspace_layout: null layout");
    INVR_CHECK(il_size_ok(H, W, window), "invr_imgloss_workspace_layout: H, W must be in [2, %d] and the window odd, at most %d (got %d x %d, %d)",
               INVR_IMGLOSS_MAX_SIDE, INVR_IMGLOSS_MAX_WINDOW, H, W, window);
    il_layout(H, W, layout);
    return 0;
}

static int il_check(const char* who, const uint8_t* mask, int32_t window, int64_t n_rays, int32_t H, int32_t W, const void* ws, size_t ws_bytes) {
    INVR_CHECK(il_size_ok(H, W, 1), "%s: H, W must be in [2, %d] (got %d x %d)", who, INVR_IMGLOSS_MAX_SIDE, H, W);
    INVR_CHECK(il_size_ok(H, W, window), "%s: the window must be odd and in [1, %d] (got %d)", who, INVR_IMGLOSS_MAX_WINDOW, window);
    INVR_CHECK(n_rays >= 0 && n_rays <= (int64_t)H * W, "%s: n_rays must be in [0, H*W] (got %lld)", who, (long long)n_rays);
    INVR_CHECK(mask && ws, "%s: null mask / workspace", who);
    INVR_CHECK(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    INVR_CHECK(ws_bytes >= invr_imgloss_workspace_bytes(H, W, window), "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes,
               invr_imgloss_workspace_bytes(H, W, window));
    return 0;
}

struct IlObjective {          // the objective around the term (NULL terms: the term alone)
    const float* dist; const float* terms; float w_pair, w_dist, w_off; int use_pair; float* err;
};

static inline dim3 il_tiles(int H, int W) { return dim3((unsigned)cdiv(W, IL_TS), (unsigned)cdiv(H, IL_TS), 3); }

static int il_final(int mode, const InvrImglossLayout& L, const float* rgb, const float* gt, int64_t n_rays, int64_t P, void* ws,
                    const IlObjective* ob, float* out8, hipStream_t st) {
    const int64_t np = mode == IL_SSIM ? L.n_ssim : L.n_tv;
    if (ob)
        hipLaunchKernelGGL(k_train_loss_term, dim3(1), dim3(1024), 0, st, mode, il_at<double>(ws, L.partial), il_at<float>(ws, L.tvmax), np, P,
                           il_at<float>(ws, L.out8), rgb, gt, ob->dist, ob->terms, n_rays, ob->w_pair, ob->w_dist, ob->w_off, ob->use_pair, out8,
                           ob->err);
    else
        hipLaunchKernelGGL(k_imgloss_final, dim3(1), dim3(IL_BLOCK), 0, st, mode, il_at<double>(ws, L.partial), il_at<float>(ws, L.tvmax), np, P,
                           il_at<float>(ws, L.out8), out8);
    INVR_LAUNCH_CHECK();
    return 0;
}

static int il_ssim_forward(const float* rgb, const float* gt, const uint8_t* mask, const float* taps, int w, int64_t n_rays, int H, int W,
                           void* ws, const IlObjective* ob, float* out8, hipStream_t st) {
    InvrImglossLayout L;
    il_layout(H, W, &L);
    const int64_t P = (int64_t)H * W;
    double* partial = il_at<double>(ws, L.partial);
    if (launch_patch_assemble(rgb, gt, mask, n_rays, P, il_at<int32_t>(ws, L.rank), il_at<float>(ws, L.img), partial + L.n_partial - 2, st)) return 1;
    hipLaunchKernelGGL(k_ssim_map, il_tiles(H, W), dim3(IL_BLOCK), 0, st, il_at<float>(ws, L.img), taps, w, H, W, il_at<float>(ws, L.mom),
                       il_at<float>(ws, L.smap), il_at<float>(ws, L.pqr), partial);
    INVR_LAUNCH_CHECK();
    return il_final(IL_SSIM, L, rgb, gt, n_rays, P, ws, ob, out8, st);
}

static int il_ssim_backward(const float* taps, int w, int H, int W, void* ws, const float* g_loss, float scale, const IlReg& reg, float* g_rgb,
                            hipStream_t st) {
    InvrImglossLayout L;
    il_layout(H, W, &L);
    hipLaunchKernelGGL(k_ssim_grad, il_tiles(H, W), dim3(IL_BLOCK), 0, st, il_at<float>(ws, L.img), il_at<float>(ws, L.pqr), taps, w, H, W,
                       il_at<int32_t>(ws, L.rank), g_loss, scale, reg.g_terms ? 1 : 0, il_at<float>(ws, L.gimg), g_rgb, reg);
    INVR_LAUNCH_CHECK();
    return 0;
}

static int il_tv_forward(const float* rgb, const float* gt, const uint8_t* occupancy, const uint8_t* mask, int64_t n_rays, int H, int W, void* ws,
                         const IlObjective* ob, float* out8, hipStream_t st) {
    InvrImglossLayout L;
    il_layout(H, W, &L);
    const int64_t P = (int64_t)H * W;
    double* partial = il_at<double>(ws, L.partial);
    if (launch_patch_assemble(rgb, gt, mask, n_rays, P, il_at<int32_t>(ws, L.rank), il_at<float>(ws, L.img), partial + L.n_partial - 2, st)) return 1;
    hipLaunchKernelGGL(k_tv_max, dim3((unsigned)L.n_tv), dim3(IL_BLOCK), 0, st, il_at<float>(ws, L.img), il_at<int32_t>(ws, L.rank), occupancy, H, W,
                       il_at<uint8_t>(ws, L.occ), il_at<float>(ws, L.tvmax));
    INVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tv_sum, dim3((unsigned)L.n_tv), dim3(IL_BLOCK), 0, st, il_at<float>(ws, L.img), il_at<uint8_t>(ws, L.occ),
                       il_at<float>(ws, L.tvmax), H, W, partial);
    INVR_LAUNCH_CHECK();
    return il_final(IL_TV, L, rgb, gt, n_rays, P, ws, ob, out8, st);
}

static int il_tv_backward(int H, int W, void* ws, const float* g_loss, float scale, const IlReg& reg, float* g_rgb, hipStream_t st) {
    InvrImglossLayout L;
    il_layout(H, W, &L);
    hipLaunchKernelGGL(k_tv_grad, dim3((unsigned)L.n_tv), dim3(IL_BLOCK), 0, st, il_at<float>(ws, L.img), il_at<uint8_t>(ws, L.occ),
                       il_at<float>(ws, L.out8), H, W, il_at<int32_t>(ws, L.rank), g_loss, scale, reg.g_terms ? 1 : 0, il_at<float>(ws, L.gimg),
                       g_rgb, reg);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_ssim_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, const float* taps, int32_t window,
                             int64_t n_rays, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream) {
    if (il_check("invr_ssim_fwd", mask_at_box, window, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(taps && out8 && (n_rays == 0 || (rgb_map && rgb_gt)), "invr_ssim_fwd: null rgb / taps / out8 pointer");
    return il_ssim_forward(rgb_map, rgb_gt, mask_at_box, taps, window, n_rays, H, W, workspace, nullptr, out8, (hipStream_t)stream);
}

extern "C" int invr_ssim_bwd(const uint8_t* mask_at_box, const float* taps, int32_t window, int64_t n_rays, int32_t H, int32_t W, void* workspace,
                             size_t workspace_bytes, const float* g_loss, float* g_rgb, void* stream) {
    if (il_check("invr_ssim_bwd", mask_at_box, window, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(taps && g_loss && (n_rays == 0 || g_rgb), "invr_ssim_bwd: null taps / g_loss / g_rgb pointer");
    if (n_rays == 0) return 0;
    IlReg reg = {};
    return il_ssim_backward(taps, window, H, W, workspace, g_loss, 1.0f, reg, g_rgb, (hipStream_t)stream);
}

extern "C" int invr_tv_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* occupancy, const uint8_t* mask_at_box, int64_t n_rays,
                           int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream) {
    if (il_check("invr_tv_fwd", mask_at_box, 1, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(out8 && (n_rays == 0 || (rgb_map && rgb_gt && occupancy)), "invr_tv_fwd: null rgb / occupancy / out8 pointer");
    return il_tv_forward(rgb_map, rgb_gt, occupancy, mask_at_box, n_rays, H, W, workspace, nullptr, out8, (hipStream_t)stream);
}

extern "C" int invr_tv_bwd(const uint8_t* mask_at_box, int64_t n_rays, int32_t H, int32_t W, void* workspace, size_t workspace_bytes,
                           const float* g_loss, float* g_rgb, void* stream) {
    if (il_check("invr_tv_bwd", mask_at_box, 1, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(g_loss && (n_rays == 0 || g_rgb), "invr_tv_bwd: null g_loss / g_rgb pointer");
    if (n_rays == 0) return 0;
    IlReg reg = {};
    return il_tv_backward(H, W, workspace, g_loss, 1.0f, reg, g_rgb, (hipStream_t)stream);
}

extern "C" int invr_train_loss_ssim_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, const float* taps, int32_t window,
                                        const float* dist, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist,
                                        float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err,
                                        void* stream) {
    if (il_check("invr_train_loss_ssim_fwd", mask_at_box, window, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(taps && terms && out8 && (n_rays == 0 || (rgb_map && rgb_gt)), "invr_train_loss_ssim_fwd: null pointer");
    const IlObjective ob = {dist, terms, w_pair, w_dist, w_off, use_pair, err};
    return il_ssim_forward(rgb_map, rgb_gt, mask_at_box, taps, window, n_rays, H, W, workspace, &ob, out8, (hipStream_t)stream);
}

extern "C" int invr_train_loss_ssim_bwd(const uint8_t* mask_at_box, const float* taps, int32_t window, const float* terms, int64_t n_rays,
                                        int32_t H, int32_t W, float w_pair, float w_dist, float w_off, int32_t use_pair, void* workspace,
                                        size_t workspace_bytes, const float* g_loss, float* g_rgb, float* g_dist, float* g_terms, void* stream) {
    if (il_check("invr_train_loss_ssim_bwd", mask_at_box, window, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(taps && terms && g_loss && g_terms && (n_rays == 0 || g_rgb), "invr_train_loss_ssim_bwd: null pointer");
    const IlReg reg = {terms, g_dist, g_terms, n_rays, w_pair, w_dist, w_off, use_pair};
    return il_ssim_backward(taps, window, H, W, workspace, g_loss, -0.1f, reg, g_rgb, (hipStream_t)stream);      // d loss / d ssim = -0.1
}

extern "C" int invr_train_loss_tv_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* occupancy, const uint8_t* mask_at_box,
                                      const float* dist, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist,
                                      float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err, void* stream) {
    if (il_check("invr_train_loss_tv_fwd", mask_at_box, 1, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(terms && out8 && (n_rays == 0 || (rgb_map && rgb_gt && occupancy)), "invr_train_loss_tv_fwd: null pointer");
    const IlObjective ob = {dist, terms, w_pair, w_dist, w_off, use_pair, err};
    return il_tv_forward(rgb_map, rgb_gt, occupancy, mask_at_box, n_rays, H, W, workspace, &ob, out8, (hipStream_t)stream);
}

extern "C" int invr_train_loss_tv_bwd(const uint8_t* mask_at_box, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair,
                                      float w_dist, float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, const float* g_loss,
                                      float* g_rgb, float* g_dist, float* g_terms, void* stream) {
    if (il_check("invr_train_loss_tv_bwd", mask_at_box, 1, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(terms && g_loss && g_terms && (n_rays == 0 || g_rgb), "invr_train_loss_tv_bwd: null pointer");
    const IlReg reg = {terms, g_dist, g_terms, n_rays, w_pair, w_dist, w_off, use_pair};
    return il_tv_backward(H, W, workspace, g_loss, 0.01f, reg, g_rgb, (hipStream_t)stream);
}
