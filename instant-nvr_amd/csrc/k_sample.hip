// One plain N_rand ray batch from a device-resident frame (include/invr_sample.h states the contract): every ray names its pixel as
// the k-th member of a pixel class; the kernel finds the pixel in the class's bit plane and writes its ray, near / far, the frame's
// pixel and the occupancy byte.
//
// ONE thread per ray, no LDS, no atomics, no cross-lane operation: the rays of a batch are independent draws (duplicates included), so
// there is nothing to share.  The select is three bounded steps: a binary search of the class's row prefix counts (ceil(log2 H)
// probes of an array that stays in cache), a walk over the row's words subtracting popcounts (at most ceil(W / 64) words), and a
// six-step popcount bisection inside the word.  At 1024 rays the launch is 4 workgroups: it is latency, not throughput, and it
// runs on the set's side stream behind the training step.
#include "ray_body.h"
#include "../../include/invr_sample.h"

#define SAMPLE_BLOCK 256

struct SampleCam {
    double kinv[9];
    RayPose p;
};

// index of the r-th (0-based) set bit of w, for r < popcount(w): halve the window six times, stepping over the lower half when it
// holds r bits or fewer
__device__ __forceinline__ int select_bit(uint64_t w, int r) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const int c = __popcll((w >> pos) & ((1ull << width) - 1ull));
        if (r >= c) {
            r -= c;
            pos += width;
        }
    }
    return pos;
}

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_ray_batch(SampleCam c, const float* __restrict__ img, const uint8_t* __restrict__ occ_msk,
                                                            const uint64_t* __restrict__ planes, const int32_t* __restrict__ row_prefix, int H,
                                                            int W, const int32_t* __restrict__ sel, int n, float* __restrict__ ray_d,
                                                            float* __restrict__ near, float* __restrict__ far, float* __restrict__ rgb,
                                                            uint8_t* __restrict__ occupancy, int64_t* __restrict__ coord) {
    const int i = (int)(blockIdx.x * SAMPLE_BLOCK + threadIdx.x);
    if (i >= n) return;
    const int cls = sel[2 * i], k = sel[2 * i + 1];
    const int wr = (W + 63) >> 6;
    // row: the last y with prefix[y] <= k (rows without a member repeat their prefix: the last of equal entries is the row that has one)
    const int32_t* __restrict__ pre = row_prefix + (int64_t)cls * (H + 1);
    int lo = 0, hi = H - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    const int y = lo;
    // word: walk the row, leaving the members of the words before
    const uint64_t* __restrict__ row = planes + ((int64_t)cls * H + y) * wr;
    int r = k - pre[y], j = 0;
    uint64_t w = row[0];
    for (int cnt = __popcll(w); r >= cnt && j + 1 < wr; cnt = __popcll(w)) {
        r -= cnt;
        w = row[++j];
    }
    const int x = (j << 6) + select_bit(w, r);
    const double fi = (double)(float)x, fj = (double)(float)y;                   // meshgrid(arange(W), arange(H)) float32
    double pc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = fi * c.kinv[a * 3] + fj * c.kinv[a * 3 + 1] + c.kinv[a * 3 + 2];   // xy1 @ inv(K).T
    float rd[3], tn, tf;
    ray_from_pixel_camera_f64(pc, c.p, rd, tn, tf);
    const int64_t fp = (int64_t)y * W + x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ray_d[(int64_t)i * 3 + a] = rd[a];
        rgb[(int64_t)i * 3 + a] = img[fp * 3 + a];
    }
    near[i] = tn;
    far[i] = tf;
    occupancy[i] = occ_msk[fp];
    coord[(int64_t)i * 2] = y;
    coord[(int64_t)i * 2 + 1] = x;
}

extern "C" int invr_ray_batch(const float* img, const uint8_t* occ_msk, const uint64_t* planes, const int32_t* row_prefix, int32_t H,
                              int32_t W, const int32_t* sel, int32_t n, const double* k_inv, const double* R, const double* T,
                              const double* cam_o, const float* bounds, float* ray_d, float* near, float* far, float* rgb,
                              uint8_t* occupancy, int64_t* coord, void* stream) {
    INVR_CHECK(img && occ_msk, "invr_ray_batch: null img / occ_msk");
    INVR_CHECK(planes && row_prefix && sel, "invr_ray_batch: null planes / row_prefix / sel");
    INVR_CHECK(k_inv && R && T && cam_o && bounds, "invr_ray_batch: null k_inv / R / T / cam_o / bounds");
    INVR_CHECK(ray_d && near && far && rgb && occupancy && coord, "invr_ray_batch: null output");
    INVR_CHECK(H >= 1 && W >= 1, "invr_ray_batch: the frame must be at least 1 x 1 (got H = %d, W = %d)", H, W);
    INVR_CHECK(n >= 1 && n <= INVR_RAY_BATCH_MAX, "invr_ray_batch: n must be in 1..%d (got %d)", INVR_RAY_BATCH_MAX, n);
    SampleCam c;
    for (int k = 0; k < 9; ++k) c.kinv[k] = k_inv[k];
    ray_pose_from_host(&c.p, R, T, cam_o, bounds);
    hipLaunchKernelGGL(k_ray_batch, dim3((unsigned)((n + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK)), dim3(SAMPLE_BLOCK), 0, (hipStream_t)stream, c, img,
                       occ_msk, planes, row_prefix, H, W, sel, n, ray_d, near, far, rgb, occupancy, coord);
    INVR_LAUNCH_CHECK();
    return 0;
}
