// One training patch from a device-resident frame (include/invr_batch.h states the contract): the rays of a window, the ones that meet
// the body's box compacted in pixel order, the frame's pixels and mask gathered for them.
//
// ONE workgroup per call: a patch is at most 256 x 256 pixels, typically 56 x 56 or 64 x 64, and its compaction is ordered — the
// workgroup walks the window in rounds of PATCH_BLOCK pixels and carries the number of rows written so far from round to round, so
// there is nothing to exchange between workgroups.  In a round every wave ballots its inside pixels (k_cull.hip's idiom: the lane's rank
// is the popcount of the lower lanes' bits), the wave totals meet in LDS and every thread sums the totals of the waves below its own.
// The totals are double-buffered by round parity: one barrier per round (a wave can write round r + 2's totals only after every wave
// has passed round r + 1's barrier, i.e. has read round r's).
#include "ray_body.h"
#include "../../include/invr_batch.h"

#define PATCH_BLOCK 1024
#define PATCH_WAVES (PATCH_BLOCK / 64)

struct PatchCam {
    float kinv[9];
    RayPose p;
};

__global__ __launch_bounds__(PATCH_BLOCK) void k_patch_batch(PatchCam c, const float* __restrict__ img, const uint8_t* __restrict__ msk, int W,
                                                             int x0, int y0, int w, int h, float* __restrict__ ray_d, float* __restrict__ near,
                                                             float* __restrict__ far, float* __restrict__ rgb, uint8_t* __restrict__ occupancy,
                                                             uint8_t* __restrict__ coord, uint8_t* __restrict__ mask_at_box,
                                                             int32_t* __restrict__ count) {
    __shared__ int wsum[2][PATCH_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = w * h, rounds = (n + PATCH_BLOCK - 1) / PATCH_BLOCK;
    int base = 0;                                              // rows written by the rounds before this one (workgroup-uniform)
    for (int r = 0; r < rounds; ++r) {
        const int p = r * PATCH_BLOCK + (int)threadIdx.x;
        const bool valid = p < n;
        const int y = valid ? p / w : 0, x = valid ? p - y * w : 0;
        const float i = (float)x, j = (float)y;              // meshgrid(arange(w), arange(h)) float32
        double pc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pc[a] = (double)((i * c.kinv[a * 3] + j * c.kinv[a * 3 + 1]) + c.kinv[a * 3 + 2]);   // xy1 @ inv(K32).T in float32
        float rd[3], tn, tf;
        const bool m = ray_from_pixel_camera(pc, c.p, rd, tn, tf) && valid;
        const unsigned long long bal = __ballot(m);
        if (lane == 0) wsum[r & 1][wv] = __popcll(bal);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int k = 0; k < PATCH_WAVES; ++k) {
            const int s = wsum[r & 1][k];
            woff += k < wv ? s : 0;
            total += s;
        }
        if (valid) mask_at_box[p] = m ? 1 : 0;
        if (m) {
            const int row = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
            const int64_t fp = (int64_t)(y0 + y) * W + (x0 + x);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                ray_d[row * 3 + a] = rd[a];
                rgb[row * 3 + a] = img[fp * 3 + a];
            }
            near[row] = tn;
            far[row] = tf;
            occupancy[row] = msk[fp] > 0 ? 1 : 0;
            coord[row * 2] = (uint8_t)x;
            coord[row * 2 + 1] = (uint8_t)y;
        }
        base += total;
    }
    if (threadIdx.x == 0) count[0] = base;
}

extern "C" int invr_patch_batch(const float* img, const uint8_t* msk, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
                                const float* k_inv, const double* R, const double* T, const double* cam_o, const float* bounds, float* ray_d,
                                float* near, float* far, float* rgb, uint8_t* occupancy, uint8_t* coord, uint8_t* mask_at_box, int32_t* count,
                                void* stream) {
    INVR_CHECK(img && msk, "invr_patch_batch: null img / msk");
    INVR_CHECK(k_inv && R && T && cam_o && bounds, "invr_patch_batch: null k_inv / R / T / cam_o / bounds");
    INVR_CHECK(ray_d && near && far && rgb && occupancy && coord && mask_at_box && count, "invr_patch_batch: null output");
    INVR_CHECK(H >= 1 && W >= 1, "invr_patch_batch: the frame must be at least 1 x 1 (got H = %d, W = %d)", H, W);
    INVR_CHECK(w >= 1 && w <= INVR_PATCH_MAX_SIDE && h >= 1 && h <= INVR_PATCH_MAX_SIDE, "invr_patch_batch: w and h must be in 1..%d (got %d x %d)",
               INVR_PATCH_MAX_SIDE, w, h);
    INVR_CHECK(x0 >= 0 && y0 >= 0 && (int64_t)x0 + w <= W && (int64_t)y0 + h <= H,
               "invr_patch_batch: the window [%d, %lld) x [%d, %lld) leaves the %d x %d frame", x0, (long long)x0 + w, y0, (long long)y0 + h, W, H);
    PatchCam c;
    for (int k = 0; k < 9; ++k) c.kinv[k] = k_inv[k];
    ray_pose_from_host(&c.p, R, T, cam_o, bounds);
    hipLaunchKernelGGL(k_patch_batch, dim3(1), dim3(PATCH_BLOCK), 0, (hipStream_t)stream, c, img, msk, W, x0, y0, w, h, ray_d, near, far, rgb,
                       occupancy, coord, mask_at_box, count);
    INVR_LAUNCH_CHECK();
    return 0;
}
