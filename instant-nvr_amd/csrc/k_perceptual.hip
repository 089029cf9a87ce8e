// The perceptual (cfg.use_lpips) image term of the training objective (include/invr_perceptual.h): forward of the frozen VGG19 prefix
// for the predicted and the target patch, backward to the predicted patch only.
//
//   forward : k_perc_assemble -> conv1_1 -> conv1_2 (+ sum |relu1_2 difference|) -> k_perc_pool -> conv2_1 -> conv2_2 (+ sum |relu2_2
//             difference|) -> k_perc_final
//   backward: k_perc_g22 -> conv2_2^T -> conv2_1^T -> k_perc_g12 (pool routing + sign term) -> conv1_2^T -> conv1_1^T (+ the image's
//             sign and MSE terms, scattered to the rays)
//
// Every 3x3 convolution is the implicit GEMM D^T = W . X^T on v_mfma_f32_16x16x4_f32 (exact fp32): a wave owns 16 consecutive pixels
// (row-major, across row ends) and CT tiles of 16 output channels; K runs over (tap, input channel) in steps of 4, the halo is a
// predicated load (zero padding), and the weights come as a packed A-operand stream built once per weight version.  The
// data-gradient of a convolution is the same kernel on the 180-degree-rotated, in/out-transposed weights.  In the forward pass a wave
// computes BOTH images' tiles with one weight stream: identical arithmetic per element, so where the two images agree on a unit's
// receptive field the two features are bit-identical and their difference is exactly 0.
// At 64 x 64 every array here is at most 2 MB: the convolutions read their operands straight from L2 / L1, there is no LDS staging
// and therefore no hand-off between lanes.  No floating-point atomics: per-wave partial sums in float64 at fixed slots of the
// workspace, one final pass adding them in a fixed order.
#include "common.h"
#include "train.h"
#include "../../include/invr_perceptual.h"

typedef float pc_f32x4 __attribute__((ext_vector_type(4)));

#define PC_BLOCK 256
#define PC_WAVES (PC_BLOCK / INVR_WAVE)
#define PC_NLAYER 4

static const int PC_CIN[PC_NLAYER] = {3, 64, 64, 128}, PC_COUT[PC_NLAYER] = {64, 64, 128, 128};

static inline int64_t pc_ksteps(int cin) { return (9 * cin + 3) / 4; }
static inline int64_t pc_pad16(int c) { return (c + 15) / 16 * 16; }

struct PcPacked { int64_t fwd[PC_NLAYER], bwd[PC_NLAYER], bias[PC_NLAYER], total; };      // float offsets into the packed image

static PcPacked pc_packed() {
    PcPacked p;
    int64_t off = 0;
    for (int l = 0; l < PC_NLAYER; ++l) { p.fwd[l] = off; off += pc_ksteps(PC_CIN[l]) * (PC_COUT[l] / 16) * 64; }
    for (int l = 0; l < PC_NLAYER; ++l) { p.bwd[l] = off; off += pc_ksteps(PC_COUT[l]) * (pc_pad16(PC_CIN[l]) / 16) * 64; }
    for (int l = 0; l < PC_NLAYER; ++l) { p.bias[l] = off; off += PC_COUT[l]; }
    p.total = off;
    return p;
}

static inline int64_t pc_conv_waves(int64_t npix, int cout_pad, int ct) { return cdiv(npix, 16) * (cout_pad / (16 * ct)); }
static inline int64_t pc_conv_blocks(int64_t npix, int cout_pad, int ct) { return cdiv(pc_conv_waves(npix, cout_pad, ct), PC_WAVES); }

#define PC_FWD_CT 1          // forward: 2 images x 1 channel tile per wave; backward: 1 image x 2 channel tiles
#define PC_BWD_CT 2

static void pc_layout(int H, int W, InvrPerceptualLayout* L) {
    const int64_t P = (int64_t)H * W, p = (int64_t)(H / 2) * (W / 2);
    size_t off = 0;
    auto take = [&](int64_t count, size_t elem) { const size_t o = off; off = align_up(off + (size_t)count * elem, 256); return (int64_t)o; };
    L->rank = take(P, 4);
    L->img = take(2 * 3 * P, 4);
    L->a11 = take(2 * 64 * P, 4);
    L->a12 = take(2 * 64 * P, 4);
    L->pool = take(2 * 64 * p, 4);
    L->a21 = take(2 * 128 * p, 4);
    L->a22 = take(2 * 128 * p, 4);
    L->n_part1 = pc_conv_blocks(P, 64, PC_FWD_CT) * PC_WAVES;
    L->n_part2 = pc_conv_blocks(p, 128, PC_FWD_CT) * PC_WAVES;
    L->n_partial = L->n_part1 + L->n_part2 + 2;
    L->partial = take(L->n_partial, 8);
    L->out8 = take(8, 4);
    L->g22 = take(128 * p, 4);
    L->gm22 = take(128 * p, 4);
    L->g21 = take(128 * p, 4);
    L->gm21 = take(128 * p, 4);
    L->gpool = take(64 * p, 4);
    L->g12 = take(64 * P, 4);
    L->gm12 = take(64 * P, 4);
    L->g11 = take(64 * P, 4);
    L->gm11 = take(64 * P, 4);
    L->gimg = take(3 * P, 4);
    L->bytes = (int64_t)off;
}

// ---- packing --------------------------------------------------------------------------------------------------------------------
// A-operand stream of a convolution with `cin` input and `cout` (padded to cout_pad) output channels: element ((s * cout_pad / 16 + tile)
// * 64 + lane) is the weight of output channel tile * 16 + lane % 16 at K index k = 4 s + lane / 16, k = tap * cin + ci (0 beyond 9 cin
// and for padded channels).  transposed: the data-gradient's weights Wb[o][i][ky][kx] = w[i][o][2 - ky][2 - kx] of torch's (out, in, 3, 3) w.
__global__ void __launch_bounds__(PC_BLOCK) k_perc_pack(const float* __restrict__ w, float* __restrict__ out, int cin, int cout, int cout_pad,
                                                        int transposed, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * PC_BLOCK) {
        const int lane = (int)(e & 63);
        const int64_t st = e >> 6;
        const int tiles = cout_pad / 16, tile = (int)(st % tiles);
        const int k = (int)(st / tiles) * 4 + (lane >> 4), o = tile * 16 + (lane & 15);
        float v = 0.0f;
        if (k < 9 * cin && o < cout) {
            const int tap = k / cin, ci = k % cin;
            v = transposed ? w[((int64_t)ci * cout + o) * 9 + (8 - tap)] : w[((int64_t)o * cin + ci) * 9 + tap];
        }
        out[e] = v;
    }
}

__global__ void __launch_bounds__(PC_BLOCK) k_perc_copy(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- patch assembly + the image's L1 / MSE sums (one workgroup) --------------------------------------------------------------------
// rank of a pixel = number of set mask bytes before it; img[mask] = rgb, zeros elsewhere (inb_trainer.py:196-203)
__global__ void __launch_bounds__(1024) k_perc_assemble(const float* __restrict__ rgb, const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                        int64_t n_rays, int64_t P, int32_t* __restrict__ rank, float* __restrict__ img,
                                                        double* __restrict__ img_sums) {
    __shared__ int s_wave[1024 / 64];
    __shared__ double s_red[2][1024 / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p0 = 0; p0 < P; p0 += 1024) {
        const int64_t pix = p0 + tid;
        const bool set = pix < P && mask[pix] != 0;
        const unsigned long long b = __ballot(set);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();                                   // (s_wave of the previous chunk has been read)
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int64_t r = carry + before, total = carry;
#pragma unroll
        for (int w = 0; w < 1024 / 64; ++w) {
            if (w < wave) r += s_wave[w];
            total += s_wave[w];
        }
        carry = total;
        if (pix < P) {
            const bool use = set && r < n_rays;
            rank[pix] = use ? (int32_t)r : -1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = use ? rgb[r * 3 + c] : 0.0f, t = use ? gt[r * 3 + c] : 0.0f;
                img[(0 * 3 + c) * P + pix] = a;
                img[(1 * 3 + c) * P + pix] = t;
                const float d = a - t;
                s1 += (double)fabsf(d);
                s2 += (double)(d * d);
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d); }
    if (lane == 0) { s_red[0][wave] = s1; s_red[1][wave] = s2; }
    __syncthreads();
    if (tid == 0) {
        s1 = s2 = 0.0;
        for (int k = 0; k < 1024 / 64; ++k) { s1 += s_red[0][k]; s2 += s_red[1][k]; }
        img_sums[0] = s1;
        img_sums[1] = s2;
    }
}

// the one statement of the patch assembly for every image term (k_imgloss.hip launches it too): img_sums[2] = sum |d|, sum d^2
int launch_patch_assemble(const float* rgb, const float* gt, const uint8_t* mask, int64_t n_rays, int64_t P, int32_t* rank, float* img,
                          double* img_sums, hipStream_t st) {
    hipLaunchKernelGGL(k_perc_assemble, dim3(1), dim3(1024), 0, st, rgb, gt, mask, n_rays, P, rank, img, img_sums);
    INVR_LAUNCH_CHECK();
    return 0;
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------
enum { PC_EP_FWD = 0, PC_EP_FWD_SUM = 1, PC_EP_BWD_MASK = 2, PC_EP_BWD_PLAIN = 3, PC_EP_BWD_IMG = 4 };

struct PcConvArgs {
    const float* in;         // [NB][CIN][H*W]
    const float* wp;         // packed A-operand stream
    const float* bias;       // forward: [COUT]
    float* out;              // forward: activations [NB][COUT][H*W]; backward: the gradient arriving at the output's layer [COUT][H*W]
    float* out_masked;       // PC_EP_BWD_MASK: out where act > 0, else 0
    const float* act;        // PC_EP_BWD_MASK: stored activation of the layer the gradient arrives at [COUT][H*W]
    double* partial;         // PC_EP_FWD_SUM: one slot per launched wave
    // PC_EP_BWD_IMG: the image's own terms and the scatter to the rays
    const float* img;        // [2][3][H*W]
    const int32_t* rank;
    const float* g_loss;
    float* g_rgb;
    int H, W;
};

// NB images x CT channel tiles per wave.  COUT is the padded channel count (a multiple of 16 CT); COUT_REAL channels are stored.
template <int CIN, int COUT, int COUT_REAL, int NB, int CT, int EP>
__global__ void __launch_bounds__(PC_BLOCK) k_perc_conv(const PcConvArgs a) {
    constexpr int K = 9 * CIN, KS = (K + 3) / 4, TILES = COUT / 16, NG = TILES / CT;
    static_assert(TILES % CT == 0, "channel tiles per wave");
    const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
    const int64_t gw = (int64_t)blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    const int64_t HW = (int64_t)a.H * a.W, strip = gw / NG;
    const int cg = (int)(gw % NG);
    if (strip * 16 >= HW) {                               // (the whole wave: a slot of the last workgroup beyond the image)
        if (EP == PC_EP_FWD_SUM && lane == 0) a.partial[gw] = 0.0;
        return;
    }
    const int64_t pix = strip * 16 + j;
    const bool valid = pix < HW;
    const int y = valid ? (int)(pix / a.W) : 0, x = valid ? (int)(pix % a.W) : 0;

    pc_f32x4 acc[NB][CT];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[n][t][r] = (EP == PC_EP_FWD || EP == PC_EP_FWD_SUM) ? a.bias[(cg * CT + t) * 16 + 4 * kq + r] : 0.0f;

    const float* wp = a.wp + ((int64_t)cg * CT) * 64 + lane;
    if constexpr (CIN % 4 == 0) {
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool inb = valid && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            const float* src = a.in + (int64_t)kq * HW + (inb ? (int64_t)yy * a.W + xx : 0);
#pragma unroll 4
            for (int s = 0; s < CIN / 4; ++s) {
                float b[NB], w[CT];
#pragma unroll
                for (int n = 0; n < NB; ++n) b[n] = inb ? src[((int64_t)n * CIN + 4 * s) * HW] : 0.0f;
#pragma unroll
                for (int t = 0; t < CT; ++t) w[t] = wp[((int64_t)(tap * (CIN / 4) + s) * TILES + t) * 64];
#pragma unroll
                for (int n = 0; n < NB; ++n)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[n][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], b[n], acc[n][t], 0, 0, 0);
            }
        }
    } else {                                              // conv1_1: K = 27 padded to 28, (tap, channel) differ per lane
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + kq, tap = k / CIN, ci = k % CIN;
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool inb = valid && k < K && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            float b[NB], w[CT];
#pragma unroll
            for (int n = 0; n < NB; ++n) b[n] = inb ? a.in[((int64_t)n * CIN + ci) * HW + (int64_t)yy * a.W + xx] : 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t) w[t] = wp[((int64_t)s * TILES + t) * 64];
#pragma unroll
            for (int n = 0; n < NB; ++n)
#pragma unroll
                for (int t = 0; t < CT; ++t) acc[n][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], b[n], acc[n][t], 0, 0, 0);
        }
    }

    // lane (j, kq) holds channels tile * 16 + 4 kq + r of pixel j
    double sum = 0.0;
    float k_l1 = 0.0f, k_mse = 0.0f;
    if (EP == PC_EP_BWD_IMG) {
        const float gl = a.g_loss[0], numel = (float)(3 * HW);
        k_l1 = gl / numel;
        k_mse = gl * 2.0f / numel;
    }
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = (cg * CT + t) * 16 + 4 * kq + r;
            if (!valid || co >= COUT_REAL) continue;
            const int64_t o = (int64_t)co * HW + pix;
            if (EP == PC_EP_FWD || EP == PC_EP_FWD_SUM) {
                float v[NB];
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    v[n] = acc[n][t][r] > 0.0f ? acc[n][t][r] : 0.0f;
                    a.out[(int64_t)n * COUT_REAL * HW + o] = v[n];
                }
                if (EP == PC_EP_FWD_SUM) sum += (double)fabsf(v[0] - v[NB - 1]);
            } else if (EP == PC_EP_BWD_MASK) {
                const float g = acc[0][t][r];
                a.out[o] = g;
                a.out_masked[o] = a.act[o] > 0.0f ? g : 0.0f;
            } else if (EP == PC_EP_BWD_PLAIN) {
                a.out[o] = acc[0][t][r];
            } else {                                      // d lpips / d image = conv^T + k_l1 sign(d) + k_mse d, then to the pixel's ray
                const float d = a.img[o] - a.img[3 * HW + o];
                const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                const float g = (acc[0][t][r] + k_l1 * sg) + k_mse * d;
                a.out[o] = g;
                const int32_t rk = a.rank[pix];
                if (rk >= 0) a.g_rgb[(int64_t)rk * 3 + co] = g;
            }
        }
    if (EP == PC_EP_FWD_SUM) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) a.partial[gw] = sum;
    }
}

// ---- 2x2 max-pool (floor), both images -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PC_BLOCK) k_perc_pool(const float* __restrict__ a12, float* __restrict__ pool, int H, int W, int64_t total) {
    const int h = H / 2, w = W / 2;
    for (int64_t e = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * PC_BLOCK) {
        const int xx = (int)(e % w), yy = (int)((e / w) % h);
        const int64_t plane = e / ((int64_t)w * h);
        const float* s = a12 + plane * H * W + (int64_t)(2 * yy) * W + 2 * xx;
        pool[e] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
    }
}

// ---- the sums -> out8 (one workgroup) ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pc_block_sum(const double* __restrict__ v, int64_t n, double* s_red) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += PC_BLOCK) s += v[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    __syncthreads();                                       // (s_red of the previous sum has been read)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
    __syncthreads();
    s = 0.0;
    for (int k = 0; k < PC_WAVES; ++k) s += s_red[k];
    return s;
}

__global__ void __launch_bounds__(PC_BLOCK) k_perc_final(const double* __restrict__ partial, int64_t n1, int64_t n2, int64_t P, int64_t p,
                                                         float* __restrict__ out_ws, float* __restrict__ out8) {
    __shared__ double s_red[PC_WAVES];
    const double f1 = pc_block_sum(partial, n1, s_red), f2 = pc_block_sum(partial + n1, n2, s_red);
    if (threadIdx.x == 0) {
        // the four means and their sum (perceptual_loss.py:64-65's order) in float64, each rounded to fp32 once
        const double l1 = f1 / (double)(64 * P), l2 = f2 / (double)(128 * p);
        const double li = partial[n1 + n2] / (double)(3 * P), mse = partial[n1 + n2 + 1] / (double)(3 * P);
        const double lp = ((l1 + l2) / 2.0 + li) + mse;
        const float o[8] = {(float)lp, (float)l1, (float)l2, (float)li, (float)mse, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 8; ++k) {
            out_ws[k] = o[k];
            if (out8) out8[k] = o[k];
        }
    }
}

// ---- backward: elementwise stages ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pc_sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// gradient arriving at relu2_2 of the predicted image: g_loss / (2 numel) * sign(a22 - target's a22)
__global__ void __launch_bounds__(PC_BLOCK) k_perc_g22(const float* __restrict__ a22, const float* __restrict__ g_loss, int64_t numel,
                                                       float* __restrict__ g22, float* __restrict__ gm22) {
    const float k = g_loss[0] / (2.0f * (float)numel);
    for (int64_t e = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x; e < numel; e += (int64_t)gridDim.x * PC_BLOCK) {
        const float av = a22[e], g = k * pc_sign(av - a22[numel + e]);
        g22[e] = g;
        gm22[e] = av > 0.0f ? g : 0.0f;
    }
}

// gradient arriving at relu1_2 of the predicted image: the pool's gradient at the FIRST maximum of each window (row-major; the last
// row / column of an odd size feeds no pooled unit) + g_loss / (2 numel) * sign(a12 - target's a12)
__global__ void __launch_bounds__(PC_BLOCK) k_perc_g12(const float* __restrict__ a12, const float* __restrict__ gpool, const float* __restrict__ g_loss,
                                                       int H, int W, int64_t numel, float* __restrict__ g12, float* __restrict__ gm12) {
    const float k = g_loss[0] / (2.0f * (float)numel);
    const int h = H / 2, w = W / 2;
    for (int64_t e = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x; e < numel; e += (int64_t)gridDim.x * PC_BLOCK) {
        const int x = (int)(e % W), y = (int)((e / W) % H);
        const int64_t c = e / ((int64_t)W * H);
        const float av = a12[e];
        float gp = 0.0f;
        if (y < 2 * h && x < 2 * w) {
            const float* s = a12 + c * H * W + (int64_t)(y & ~1) * W + (x & ~1);
            const float v0 = s[0], v1 = s[1], v2 = s[W], v3 = s[W + 1];
            const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
            const int first = v0 == m ? 0 : (v1 == m ? 1 : (v2 == m ? 2 : 3));
            if (first == (y & 1) * 2 + (x & 1)) gp = gpool[(c * h + y / 2) * w + x / 2];
        }
        const float g = gp + k * pc_sign(av - a12[numel + e]);
        g12[e] = g;
        gm12[e] = av > 0.0f ? g : 0.0f;
    }
}

// ---- the whole objective's scalar part (k_train_loss of k_train.hip with lpips in the place of the MSE in the sum) ---------------------
// out[8] = {loss, img_loss, psnr, reg_dist, offset_loss, pair_loss, lpips, 0}
__global__ __launch_bounds__(1024) void k_train_loss_lpips(const float* __restrict__ rgb, const float* __restrict__ gt, const float* __restrict__ dist,
                                                           const float* __restrict__ terms, const float* __restrict__ perc_out, int64_t n,
                                                           float w_pair, float w_dist, float w_off, int use_pair, float* __restrict__ out,
                                                           float* __restrict__ err) {
    __shared__ double red[2][1024 / 64];
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
        const float lp = perc_out[0];
        float loss = 0.0f;
        if (use_pair) loss = loss + w_pair * pair;
        if (dist) loss = loss + w_dist * rd;
        loss = loss + w_off * off;
        loss = loss + lp;
        out[0] = loss; out[1] = img; out[2] = -10.0f * logf(img) / 2.302585092994046f; out[3] = rd; out[4] = off; out[5] = pair;
        out[6] = lp; out[7] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_train_loss_lpips_bwd(const float* __restrict__ terms, int64_t n, float w_pair, float w_dist, float w_off,
                                                              int use_pair, const float* __restrict__ g_loss, float* __restrict__ g_dist,
                                                              float* __restrict__ g_terms) {
    const float gl = g_loss[0];
    const float k_dist = n > 0 ? gl * w_dist / (float)n : 0.0f;
    if (g_dist)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g_dist[i] = k_dist;
    if (blockIdx.x == 0 && threadIdx.x < TERM_LEN) {
        float g = 0.0f;
        if (threadIdx.x == TERM_OFFSET_SUM) g = gl * w_off / fmaxf(terms[TERM_OFFSET_ROWS], 1.0f);
        if (threadIdx.x == TERM_PAIR_SUM && use_pair) g = gl * w_pair / fmaxf(terms[TERM_PAIR_ROWS], 1.0f);
        g_terms[threadIdx.x] = g;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned pc_grid(int64_t n) { const int64_t b = cdiv(n > 0 ? n : 1, PC_BLOCK); return (unsigned)(b < 2048 ? b : 2048); }
template <class T> static inline T* pc_at(void* ws, int64_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

extern "C" int64_t invr_perceptual_packed_floats(void) { return pc_packed().total; }

extern "C" int invr_perceptual_pack_weights(const float* const* w, const float* const* b, float* packed, void* stream) {
    INVR_CHECK(w && b && packed, "invr_perceptual_pack_weights: null pointer");
    for (int l = 0; l < PC_NLAYER; ++l) INVR_CHECK(w[l] && b[l], "invr_perceptual_pack_weights: null weight / bias pointer of layer %d", l);
    const PcPacked p = pc_packed();
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < PC_NLAYER; ++l) {
        const int64_t nf = pc_ksteps(PC_CIN[l]) * (PC_COUT[l] / 16) * 64, nb = pc_ksteps(PC_COUT[l]) * (pc_pad16(PC_CIN[l]) / 16) * 64;
        hipLaunchKernelGGL(k_perc_pack, dim3(pc_grid(nf)), dim3(PC_BLOCK), 0, st, w[l], packed + p.fwd[l], PC_CIN[l], PC_COUT[l], PC_COUT[l], 0, nf);
        INVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_perc_pack, dim3(pc_grid(nb)), dim3(PC_BLOCK), 0, st, w[l], packed + p.bwd[l], PC_COUT[l], PC_CIN[l],
                           (int)pc_pad16(PC_CIN[l]), 1, nb);
        INVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_perc_copy, dim3(pc_grid(PC_COUT[l])), dim3(PC_BLOCK), 0, st, b[l], packed + p.bias[l], PC_COUT[l]);
        INVR_LAUNCH_CHECK();
    }
    return 0;
}

static inline bool pc_size_ok(int32_t H, int32_t W) { return H >= 2 && W >= 2 && H <= INVR_PERCEPTUAL_MAX_SIDE && W <= INVR_PERCEPTUAL_MAX_SIDE; }

extern "C" size_t invr_perceptual_workspace_bytes(int32_t H, int32_t W) {
    if (!pc_size_ok(H, W)) return 0;
    InvrPerceptualLayout L;
    pc_layout(H, W, &L);
    return (size_t)L.bytes;
}

extern "C" int invr_perceptual_workspace_layout(int32_t H, int32_t W, InvrPerceptualLayout* layout) {
    INVR_CHECK(layout, "invr_perceptual_workspace_layout: null layout");
    INVR_CHECK(pc_size_ok(H, W), "invr_perceptual_workspace_layout: H, W must be in [2, %d] (got %d x %d)", INVR_PERCEPTUAL_MAX_SIDE, H, W);
    pc_layout(H, W, layout);
    return 0;
}

static int pc_check(const char* who, const float* packed, const uint8_t* mask, int64_t n_rays, int32_t H, int32_t W, const void* ws,
                    size_t ws_bytes) {
    INVR_CHECK(pc_size_ok(H, W), "%s: H, W must be in [2, %d] (got %d x %d)", who, INVR_PERCEPTUAL_MAX_SIDE, H, W);
    INVR_CHECK(n_rays >= 0 && n_rays <= (int64_t)H * W, "%s: n_rays must be in [0, H*W] (got %lld)", who, (long long)n_rays);
    INVR_CHECK(packed && mask && ws, "%s: null packed weights / mask / workspace", who);
    INVR_CHECK(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    INVR_CHECK(ws_bytes >= invr_perceptual_workspace_bytes(H, W), "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes,
               invr_perceptual_workspace_bytes(H, W));
    return 0;
}

template <int CIN, int COUT, int COUT_REAL, int NB, int CT, int EP>
static int pc_launch_conv(const PcConvArgs& a, hipStream_t st) {
    const int64_t blocks = pc_conv_blocks((int64_t)a.H * a.W, COUT, CT);
    hipLaunchKernelGGL((k_perc_conv<CIN, COUT, COUT_REAL, NB, CT, EP>), dim3((unsigned)blocks), dim3(PC_BLOCK), 0, st, a);
    INVR_LAUNCH_CHECK();
    return 0;
}

static int pc_forward(const float* packed, const float* rgb, const float* gt, const uint8_t* mask, int64_t n_rays, int H, int W, void* ws,
                      float* out8, hipStream_t st) {
    InvrPerceptualLayout L;
    pc_layout(H, W, &L);
    const PcPacked pk = pc_packed();
    const int64_t P = (int64_t)H * W;
    const int h = H / 2, w = W / 2;
    const int64_t p = (int64_t)h * w;
    double* partial = pc_at<double>(ws, L.partial);
    if (launch_patch_assemble(rgb, gt, mask, n_rays, P, pc_at<int32_t>(ws, L.rank), pc_at<float>(ws, L.img), partial + L.n_part1 + L.n_part2, st)) return 1;
    PcConvArgs a = {};
    a.H = H; a.W = W;
    a.in = pc_at<float>(ws, L.img); a.wp = packed + pk.fwd[0]; a.bias = packed + pk.bias[0]; a.out = pc_at<float>(ws, L.a11);
    if (pc_launch_conv<3, 64, 64, 2, PC_FWD_CT, PC_EP_FWD>(a, st)) return 1;
    a.in = pc_at<float>(ws, L.a11); a.wp = packed + pk.fwd[1]; a.bias = packed + pk.bias[1]; a.out = pc_at<float>(ws, L.a12); a.partial = partial;
    if (pc_launch_conv<64, 64, 64, 2, PC_FWD_CT, PC_EP_FWD_SUM>(a, st)) return 1;
    hipLaunchKernelGGL(k_perc_pool, dim3(pc_grid(2 * 64 * p)), dim3(PC_BLOCK), 0, st, pc_at<float>(ws, L.a12), pc_at<float>(ws, L.pool), H, W,
                       2 * 64 * p);
    INVR_LAUNCH_CHECK();
    a.H = h; a.W = w; a.partial = nullptr;
    a.in = pc_at<float>(ws, L.pool); a.wp = packed + pk.fwd[2]; a.bias = packed + pk.bias[2]; a.out = pc_at<float>(ws, L.a21);
    if (pc_launch_conv<64, 128, 128, 2, PC_FWD_CT, PC_EP_FWD>(a, st)) return 1;
    a.in = pc_at<float>(ws, L.a21); a.wp = packed + pk.fwd[3]; a.bias = packed + pk.bias[3]; a.out = pc_at<float>(ws, L.a22);
    a.partial = partial + L.n_part1;
    if (pc_launch_conv<128, 128, 128, 2, PC_FWD_CT, PC_EP_FWD_SUM>(a, st)) return 1;
    hipLaunchKernelGGL(k_perc_final, dim3(1), dim3(PC_BLOCK), 0, st, partial, L.n_part1, L.n_part2, P, p, pc_at<float>(ws, L.out8), out8);
    INVR_LAUNCH_CHECK();
    return 0;
}

static int pc_backward(const float* packed, int64_t n_rays, int H, int W, void* ws, const float* g_loss, float* g_rgb, hipStream_t st) {
    if (n_rays == 0) return 0;
    InvrPerceptualLayout L;
    pc_layout(H, W, &L);
    const PcPacked pk = pc_packed();
    const int64_t P = (int64_t)H * W;
    const int h = H / 2, w = W / 2;
    const int64_t p = (int64_t)h * w;
    hipLaunchKernelGGL(k_perc_g22, dim3(pc_grid(128 * p)), dim3(PC_BLOCK), 0, st, pc_at<float>(ws, L.a22), g_loss, 128 * p, pc_at<float>(ws, L.g22),
                       pc_at<float>(ws, L.gm22));
    INVR_LAUNCH_CHECK();
    PcConvArgs a = {};
    a.H = h; a.W = w;
    a.in = pc_at<float>(ws, L.gm22); a.wp = packed + pk.bwd[3]; a.out = pc_at<float>(ws, L.g21); a.out_masked = pc_at<float>(ws, L.gm21);
    a.act = pc_at<float>(ws, L.a21);
    if (pc_launch_conv<128, 128, 128, 1, PC_BWD_CT, PC_EP_BWD_MASK>(a, st)) return 1;
    a.in = pc_at<float>(ws, L.gm21); a.wp = packed + pk.bwd[2]; a.out = pc_at<float>(ws, L.gpool); a.out_masked = nullptr; a.act = nullptr;
    if (pc_launch_conv<128, 64, 64, 1, PC_BWD_CT, PC_EP_BWD_PLAIN>(a, st)) return 1;
    hipLaunchKernelGGL(k_perc_g12, dim3(pc_grid(64 * P)), dim3(PC_BLOCK), 0, st, pc_at<float>(ws, L.a12), pc_at<float>(ws, L.gpool), g_loss, H, W,
                       64 * P, pc_at<float>(ws, L.g12), pc_at<float>(ws, L.gm12));
    INVR_LAUNCH_CHECK();
    a.H = H; a.W = W;
    a.in = pc_at<float>(ws, L.gm12); a.wp = packed + pk.bwd[1]; a.out = pc_at<float>(ws, L.g11); a.out_masked = pc_at<float>(ws, L.gm11);
    a.act = pc_at<float>(ws, L.a11);
    if (pc_launch_conv<64, 64, 64, 1, PC_BWD_CT, PC_EP_BWD_MASK>(a, st)) return 1;
    a.in = pc_at<float>(ws, L.gm11); a.wp = packed + pk.bwd[0]; a.out = pc_at<float>(ws, L.gimg); a.out_masked = nullptr; a.act = nullptr;
    a.img = pc_at<float>(ws, L.img); a.rank = pc_at<int32_t>(ws, L.rank); a.g_loss = g_loss; a.g_rgb = g_rgb;
    if (pc_launch_conv<64, 16, 3, 1, 1, PC_EP_BWD_IMG>(a, st)) return 1;
    return 0;
}

extern "C" int invr_perceptual_fwd(const float* packed, const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, int64_t n_rays,
                                   int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream) {
    if (pc_check("invr_perceptual_fwd", packed, mask_at_box, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(out8 && (n_rays == 0 || (rgb_map && rgb_gt)), "invr_perceptual_fwd: null rgb / out8 pointer");
    return pc_forward(packed, rgb_map, rgb_gt, mask_at_box, n_rays, H, W, workspace, out8, (hipStream_t)stream);
}

extern "C" int invr_perceptual_bwd(const float* packed, const uint8_t* mask_at_box, int64_t n_rays, int32_t H, int32_t W, void* workspace,
                                   size_t workspace_bytes, const float* g_loss, float* g_rgb, void* stream) {
    if (pc_check("invr_perceptual_bwd", packed, mask_at_box, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(g_loss && (n_rays == 0 || g_rgb), "invr_perceptual_bwd: null g_loss / g_rgb pointer");
    return pc_backward(packed, n_rays, H, W, workspace, g_loss, g_rgb, (hipStream_t)stream);
}

extern "C" int invr_train_loss_lpips_fwd(const float* packed, const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box,
                                         const float* dist, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist,
                                         float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err,
                                         void* stream) {
    if (pc_check("invr_train_loss_lpips_fwd", packed, mask_at_box, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(terms && out8 && (n_rays == 0 || (rgb_map && rgb_gt)), "invr_train_loss_lpips_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (pc_forward(packed, rgb_map, rgb_gt, mask_at_box, n_rays, H, W, workspace, nullptr, st)) return 1;
    InvrPerceptualLayout L;
    pc_layout(H, W, &L);
    hipLaunchKernelGGL(k_train_loss_lpips, dim3(1), dim3(1024), 0, st, rgb_map, rgb_gt, dist, terms, pc_at<float>(workspace, L.out8), n_rays,
                       w_pair, w_dist, w_off, use_pair, out8, err);
    INVR_LAUNCH_CHECK();
    return 0;
}

extern "C" int invr_train_loss_lpips_bwd(const float* packed, const uint8_t* mask_at_box, const float* terms, int64_t n_rays, int32_t H,
                                         int32_t W, float w_pair, float w_dist, float w_off, int32_t use_pair, void* workspace,
                                         size_t workspace_bytes, const float* g_loss, float* g_rgb, float* g_dist, float* g_terms, void* stream) {
    if (pc_check("invr_train_loss_lpips_bwd", packed, mask_at_box, n_rays, H, W, workspace, workspace_bytes)) return 1;
    INVR_CHECK(terms && g_loss && g_terms && (n_rays == 0 || g_rgb), "invr_train_loss_lpips_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = cdiv(n_rays > 0 ? n_rays : 1, 256);
    hipLaunchKernelGGL(k_train_loss_lpips_bwd, dim3((unsigned)(tiles < 256 ? tiles : 256)), dim3(256), 0, st, terms, n_rays, w_pair, w_dist, w_off,
                       use_pair, g_loss, g_dist, g_terms);
    INVR_LAUNCH_CHECK();
    return pc_backward(packed, n_rays, H, W, workspace, g_loss, g_rgb, st);
}
