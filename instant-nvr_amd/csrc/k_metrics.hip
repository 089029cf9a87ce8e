// Per-frame image metrics of the reference's Evaluator (lib/evaluators/if_nerf.py) on the device, in float64, without a host
// round trip:
//   invr_image_assemble : img[mask] = values (:39-42, :85-89), cv2.boundingRect(mask) (:68), the 8-bit B,G,R image cv2.imwrite
//                         stores (:58-65, :106-107)            — k_mask_count -> k_mask_scan -> k_mask_scatter
//   invr_image_metrics  : sum (pred - gt)^2 (:112, :137), sum gt (:134), and scikit-image's structural_similarity with its defaults
//                         (:72, :126: uniform 7x7 window, K1 0.01, K2 0.03, sample covariance, data_range 2)
//                                                              — k_image_metrics -> k_metrics_final
// Every hand-off between workgroups is a kernel boundary.  No floating-point atomics: per-lane sums in a fixed order, a shuffle tree
// per wave, the waves of a workgroup in order, per-workgroup partials in the workspace, one workgroup adding those in a fixed
// order — the same inputs give the same bits in every run.
#include "common.h"

#define MET_BLOCK 256
#define MET_WAVES (MET_BLOCK / INVR_WAVE)
#define MET_PIX_ITERS 4                                   // a rank workgroup covers MET_BLOCK * MET_PIX_ITERS consecutive pixels
#define MET_PIX_PER_BLOCK (MET_BLOCK * MET_PIX_ITERS)
#define MET_TW 32                                         // window positions per tile: 32 columns x 16 rows
#define MET_TH 16
#define MET_WIN 7
#define MET_AW (MET_TW + MET_WIN - 1)                     // tile + apron: 38 x 22 pixels
#define MET_AH (MET_TH + MET_WIN - 1)

// result block (INVR_EVAL_RESULT_BYTES): double[3] at byte 0, int32[8] at byte 24
__device__ __forceinline__ double* res_f64(void* r) { return reinterpret_cast<double*>(r); }
__device__ __forceinline__ int32_t* res_i32(void* r) { return reinterpret_cast<int32_t*>(reinterpret_cast<char*>(r) + 24); }

struct MetWs {                 // carve of the caller's workspace
    int32_t* block_count;      // [n_rank_blocks] set pixels per rank workgroup, then their exclusive prefix
    int32_t* block_rect;       // [n_rank_blocks][4] min x, max x, min y, max y of the workgroup's set pixels
    double* partial;           // [n_tiles][3] sum S, sum (pred - gt)^2, sum gt per tile
    int64_t n_rank_blocks, n_tiles;
    size_t bytes;
};

static MetWs met_carve(void* ws, int H, int W) {
    MetWs m;
    const int64_t npix = (int64_t)H * W;
    m.n_rank_blocks = cdiv(npix, MET_PIX_PER_BLOCK);
    m.n_tiles = cdiv(W, MET_TW) * cdiv(H, MET_TH);
    char* base = reinterpret_cast<char*>(ws);
    size_t off = 0;
    m.block_count = reinterpret_cast<int32_t*>(base + off); off = align_up(off + (size_t)m.n_rank_blocks * sizeof(int32_t), 256);
    m.block_rect = reinterpret_cast<int32_t*>(base + off); off = align_up(off + (size_t)m.n_rank_blocks * 4 * sizeof(int32_t), 256);
    m.partial = reinterpret_cast<double*>(base + off); off = align_up(off + (size_t)m.n_tiles * 3 * sizeof(double), 256);
    m.bytes = off + 256;
    return m;
}

size_t eval_workspace_bytes(int H, int W) { return met_carve(nullptr, H, W).bytes; }

// ---- rank: set pixels per workgroup + their bounding rectangle ------------------------------------------------------------------
__global__ void __launch_bounds__(MET_BLOCK) k_mask_count(const uint8_t* __restrict__ mask, int64_t npix, int W,
                                                          int32_t* __restrict__ block_count, int32_t* __restrict__ block_rect) {
    __shared__ int s_cnt, s_rect[4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { s_cnt = 0; s_rect[0] = 0x7fffffff; s_rect[1] = -1; s_rect[2] = 0x7fffffff; s_rect[3] = -1; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * MET_PIX_PER_BLOCK;
    int cnt = 0, lo_x = 0x7fffffff, hi_x = -1, lo_y = 0x7fffffff, hi_y = -1;
#pragma unroll
    for (int it = 0; it < MET_PIX_ITERS; ++it) {
        const int64_t pix = base + it * MET_BLOCK + tid;
        const bool set = pix < npix && mask[pix] != 0;
        const unsigned long long b = __ballot(set);
        if (lane == 0) cnt += __popcll(b);
        if (set) {
            const int x = (int)(pix % W), y = (int)(pix / W);
            lo_x = min(lo_x, x); hi_x = max(hi_x, x); lo_y = min(lo_y, y); hi_y = max(hi_y, y);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                    // the wave's rectangle, then one LDS atomic per wave and bound
        lo_x = min(lo_x, __shfl_xor(lo_x, d)); hi_x = max(hi_x, __shfl_xor(hi_x, d));
        lo_y = min(lo_y, __shfl_xor(lo_y, d)); hi_y = max(hi_y, __shfl_xor(hi_y, d));
    }
    if (lane == 0 && hi_x >= 0) {
        atomicMin(&s_rect[0], lo_x); atomicMax(&s_rect[1], hi_x);
        atomicMin(&s_rect[2], lo_y); atomicMax(&s_rect[3], hi_y);
    }
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) block_count[blockIdx.x] = s_cnt;
    if (tid < 4) block_rect[blockIdx.x * 4 + tid] = s_rect[tid];
}

// one workgroup: exclusive prefix of the workgroup counts (in place), the frame's rectangle and the status word
__global__ void __launch_bounds__(MET_BLOCK) k_mask_scan(int32_t* __restrict__ block_count, const int32_t* __restrict__ block_rect,
                                                         int64_t n_blocks, int64_t n_expected, void* __restrict__ result) {
    __shared__ int s_wave[MET_WAVES], s_rect[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_rect[0] = 0x7fffffff; s_rect[1] = -1; s_rect[2] = 0x7fffffff; s_rect[3] = -1; }
    int carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += MET_BLOCK) {
        const int64_t b = b0 + tid;
        const int v = b < n_blocks ? block_count[b] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        __syncthreads();                                   // (s_wave of the previous chunk has been read; s_rect is initialised)
        if (lane == 63) s_wave[wave] = incl;
        if (b < n_blocks && v > 0) {
            atomicMin(&s_rect[0], block_rect[b * 4 + 0]); atomicMax(&s_rect[1], block_rect[b * 4 + 1]);
            atomicMin(&s_rect[2], block_rect[b * 4 + 2]); atomicMax(&s_rect[3], block_rect[b * 4 + 3]);
        }
        __syncthreads();
        int before = carry, total = carry;
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (b < n_blocks) block_count[b] = before + incl - v;
        carry = total;
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* ri = res_i32(result);
        const bool any = carry > 0;
        ri[INVR_EVAL_I_X] = any ? s_rect[0] : 0;
        ri[INVR_EVAL_I_Y] = any ? s_rect[2] : 0;
        ri[INVR_EVAL_I_W] = any ? s_rect[1] - s_rect[0] + 1 : 0;
        ri[INVR_EVAL_I_H] = any ? s_rect[3] - s_rect[2] + 1 : 0;
        ri[INVR_EVAL_I_NSET] = carry;
        ri[INVR_EVAL_I_STATUS] = (int64_t)carry != n_expected ? 1 : 0;
        ri[INVR_EVAL_I_WINDOWS] = 0;
        ri[7] = 0;
    }
}

// cv2.imwrite of a float64 image: saturate_cast<uchar>(double) = round half to even, then clamp (a NaN becomes 0)
__device__ __forceinline__ uint8_t to_u8(float v) {
    const double r = rint((double)v * 255.0);
    return !(r > 0.0) ? 0 : (r > 255.0 ? 255 : (uint8_t)r);
}

// img[mask] = values: the k-th set pixel (row-major) takes row k; every pixel of the outputs is written
__global__ void __launch_bounds__(MET_BLOCK) k_mask_scatter(const uint8_t* __restrict__ mask, const float* __restrict__ pred,
                                                            const float* __restrict__ gt, int64_t n, int64_t npix,
                                                            const int32_t* __restrict__ block_off, float* __restrict__ img_pred,
                                                            float* __restrict__ img_gt, uint8_t* __restrict__ u8_pred,
                                                            uint8_t* __restrict__ u8_gt) {
    __shared__ int s_cnt[MET_PIX_ITERS * MET_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * MET_PIX_PER_BLOCK;
    bool set[MET_PIX_ITERS];
    int below[MET_PIX_ITERS];
#pragma unroll
    for (int it = 0; it < MET_PIX_ITERS; ++it) {
        const int64_t pix = base + it * MET_BLOCK + tid;
        set[it] = pix < npix && mask[pix] != 0;
        const unsigned long long b = __ballot(set[it]);
        below[it] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[it * MET_WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    const int64_t off = block_off[blockIdx.x];
    int seg = 0;                                          // set pixels of this workgroup in front of segment (it, wave)
#pragma unroll
    for (int it = 0; it < MET_PIX_ITERS; ++it) {
        int mine = seg;
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) {
            if (w < wave) mine += s_cnt[it * MET_WAVES + w];
            seg += s_cnt[it * MET_WAVES + w];
        }
        const int64_t pix = base + it * MET_BLOCK + tid;
        if (pix >= npix) continue;
        const int64_t rank = off + mine + below[it];
        float p[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
        if (set[it] && rank < n) {                        // (rank >= n: more set pixels than rows — the status word says so)
#pragma unroll
            for (int c = 0; c < 3; ++c) { p[c] = pred[rank * 3 + c]; g[c] = gt[rank * 3 + c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { img_pred[pix * 3 + c] = p[c]; img_gt[pix * 3 + c] = g[c]; }
        if (u8_pred) {
#pragma unroll
            for (int c = 0; c < 3; ++c) u8_pred[pix * 3 + c] = to_u8(p[2 - c]);
        }
        if (u8_gt) {
#pragma unroll
            for (int c = 0; c < 3; ++c) u8_gt[pix * 3 + c] = to_u8(g[2 - c]);
        }
    }
}

// ---- metrics ------------------------------------------------------------------------------------------------------------------------
// fixed-order sum of one double per work-item over the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* s_red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) t += s_red[w];
    }
    return t;
}

// One tile of the region (the whole frame, or the mask's rectangle read from the result block): 32 x 16 window positions and the same
// 32 x 16 pixels for the two plain sums.  Per channel: tile + apron into LDS, the five 7-tap row sums (x, y, xx, yy, xy) in
// float64, then the 7-tap column sums, S per window.
__global__ void __launch_bounds__(MET_BLOCK) k_image_metrics(const float* __restrict__ img_pred, const float* __restrict__ img_gt,
                                                             int H, int W, int crop, const void* __restrict__ result,
                                                             double* __restrict__ partial) {
    __shared__ float s_p[MET_AH][MET_AW], s_g[MET_AH][MET_AW];
    __shared__ double s_row[5][MET_AH][MET_TW];
    __shared__ double s_red[MET_WAVES];
    const int tid = threadIdx.x;
    int x0 = 0, y0 = 0, rw = W, rh = H;
    if (crop) {
        const int32_t* ri = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(result) + 24);
        x0 = ri[INVR_EVAL_I_X]; y0 = ri[INVR_EVAL_I_Y]; rw = ri[INVR_EVAL_I_W]; rh = ri[INVR_EVAL_I_H];
        if (x0 < 0 || y0 < 0 || rw < 0 || rh < 0 || x0 + rw > W || y0 + rh > H) { x0 = y0 = rw = rh = 0; }      // (never read out of the image)
    }
    const int ox = blockIdx.x * MET_TW, oy = blockIdx.y * MET_TH;          // tile origin inside the region
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (ox >= rw || oy >= rh) {                                            // (uniform for the workgroup)
        if (tid < 3) partial[tile * 3 + tid] = 0.0;
        return;
    }
    const double C1 = 4e-4, C2 = 3.6e-3, cov_norm = 49.0 / 48.0;           // (K1 * 2)^2, (K2 * 2)^2, NP / (NP - 1)
    double acc_s = 0.0, acc_sse = 0.0, acc_gt = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < MET_AH * MET_AW; i += MET_BLOCK) {
            const int r = i / MET_AW, q = i % MET_AW;
            float p = 0.0f, g = 0.0f;
            if (oy + r < rh && ox + q < rw) {
                const int64_t at = ((int64_t)(y0 + oy + r) * W + (x0 + ox + q)) * 3 + c;
                p = img_pred[at]; g = img_gt[at];
                if (r < MET_TH && q < MET_TW) {
                    const double d = (double)p - (double)g;
                    acc_sse += d * d;
                    acc_gt += (double)g;
                }
            }
            s_p[r][q] = p; s_g[r][q] = g;
        }
        __syncthreads();
        for (int i = tid; i < MET_AH * MET_TW; i += MET_BLOCK) {
            const int r = i / MET_TW, x = i % MET_TW;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int k = 0; k < MET_WIN; ++k) {
                const double a = (double)s_p[r][x + k], b = (double)s_g[r][x + k];
                sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
            }
            s_row[0][r][x] = sx; s_row[1][r][x] = sy; s_row[2][r][x] = sxx; s_row[3][r][x] = syy; s_row[4][r][x] = sxy;
        }
        __syncthreads();
        for (int i = tid; i < MET_TH * MET_TW; i += MET_BLOCK) {
            const int y = i / MET_TW, x = i % MET_TW;
            if (oy + y + MET_WIN <= rh && ox + x + MET_WIN <= rw) {        // the window lies fully inside the region
                double m[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < MET_WIN; ++k) t += s_row[j][y + k][x];
                    m[j] = t / 49.0;
                }
                const double ux = m[0], uy = m[1];
                const double vx = cov_norm * (m[2] - ux * ux), vy = cov_norm * (m[3] - uy * uy), vxy = cov_norm * (m[4] - ux * uy);
                const double num = (2.0 * ux * uy + C1) * (2.0 * vxy + C2);
                const double den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                acc_s += num / den;
            }
        }
        __syncthreads();                                   // (the next channel overwrites the tile)
    }
    const double ts = block_sum_f64(acc_s, s_red);
    const double te = block_sum_f64(acc_sse, s_red);
    const double tg = block_sum_f64(acc_gt, s_red);
    if (tid == 0) { partial[tile * 3 + 0] = ts; partial[tile * 3 + 1] = te; partial[tile * 3 + 2] = tg; }
}

// one workgroup: the tiles' partials in a fixed order -> the result block
__global__ void __launch_bounds__(MET_BLOCK) k_metrics_final(const double* __restrict__ partial, int64_t n_tiles, int H, int W, int crop,
                                                             void* __restrict__ result) {
    __shared__ double s_red[MET_WAVES];
    const int tid = threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t t = tid; t < n_tiles; t += MET_BLOCK) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] += partial[t * 3 + j];
    }
    const double ts = block_sum_f64(a[0], s_red);
    const double te = block_sum_f64(a[1], s_red);
    const double tg = block_sum_f64(a[2], s_red);
    if (tid == 0) {
        int32_t* ri = res_i32(result);
        int rw = W, rh = H;
        if (crop) {
            rw = ri[INVR_EVAL_I_W]; rh = ri[INVR_EVAL_I_H];
            if (ri[INVR_EVAL_I_X] < 0 || ri[INVR_EVAL_I_Y] < 0 || rw < 0 || rh < 0 || ri[INVR_EVAL_I_X] + rw > W || ri[INVR_EVAL_I_Y] + rh > H) rw = rh = 0;
        }
        double* rd = res_f64(result);
        rd[INVR_EVAL_F_SSE] = te; rd[INVR_EVAL_F_SUM_GT] = tg; rd[INVR_EVAL_F_SUM_S] = ts;
        ri[INVR_EVAL_I_WINDOWS] = (rw >= MET_WIN && rh >= MET_WIN) ? (rw - MET_WIN + 1) * (rh - MET_WIN + 1) : 0;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
int launch_image_assemble(const float* pred, const float* gt, const uint8_t* mask, int64_t n, int H, int W, float* img_pred,
                          float* img_gt, uint8_t* u8_pred, uint8_t* u8_gt, void* result, void* ws, hipStream_t st) {
    const MetWs m = met_carve(ws, H, W);
    const int64_t npix = (int64_t)H * W;
    if (npix > 0) {
        hipLaunchKernelGGL(k_mask_count, dim3((unsigned)m.n_rank_blocks), dim3(MET_BLOCK), 0, st, mask, npix, W, m.block_count, m.block_rect);
        INVR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(MET_BLOCK), 0, st, m.block_count, m.block_rect, m.n_rank_blocks, n, result);
    INVR_LAUNCH_CHECK();
    if (npix > 0) {
        hipLaunchKernelGGL(k_mask_scatter, dim3((unsigned)m.n_rank_blocks), dim3(MET_BLOCK), 0, st, mask, pred, gt, n, npix, m.block_count,
                           img_pred, img_gt, u8_pred, u8_gt);
        INVR_LAUNCH_CHECK();
    }
    return 0;
}

int launch_image_metrics(const float* img_pred, const float* img_gt, int H, int W, int crop, void* result, void* ws, hipStream_t st) {
    const MetWs m = met_carve(ws, H, W);
    if (m.n_tiles > 0) {
        hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)cdiv(W, MET_TW), (unsigned)cdiv(H, MET_TH)), dim3(MET_BLOCK), 0, st,
                           img_pred, img_gt, H, W, crop, result, m.partial);
        INVR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_metrics_final, dim3(1), dim3(MET_BLOCK), 0, st, m.partial, m.n_tiles, H, W, crop, result);
    INVR_LAUNCH_CHECK();
    return 0;
}
