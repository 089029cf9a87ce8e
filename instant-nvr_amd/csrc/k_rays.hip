// Row f2: ray generation on the device — get_rays + get_near_far of the reference's dataset code
// (lib/utils/if_nerf/if_nerf_data_utils.py:24-38, 92-107, 313-327), which runs in NumPy on the host
// per frame: pixel -> camera -> world in float64, normalise, cast to float32, then the ray / AABB
// slab test in float32.  One thread per pixel; full-frame outputs + the mask_at_box byte mask (the
// caller compacts).  inv(K), R, T and the camera centre are tiny host-side float64 values (the
// Python wrapper forms them with NumPy exactly as the reference does).  The body from pixel_camera on is ray_body.h's.
#include "ray_body.h"

struct RayCam {
    double kinv[9];
    RayPose p;
};

__global__ void k_generate_rays(RayCam c, int H, int W, float* __restrict__ ray_d, float* __restrict__ near,
                                float* __restrict__ far, uint8_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    const double i = (double)(float)(idx % W), j = (double)(float)(idx / W);     // meshgrid(arange(W), arange(H)) float32
    double pc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = i * c.kinv[a * 3] + j * c.kinv[a * 3 + 1] + c.kinv[a * 3 + 2];   // xy1 @ inv(K).T
    float rd[3], tn, tf;
    const bool m = ray_from_pixel_camera(pc, c.p, rd, tn, tf);
#pragma unroll
    for (int a = 0; a < 3; ++a) ray_d[idx * 3 + a] = rd[a];
    mask[idx] = m ? 1 : 0;
    near[idx] = tn;
    far[idx] = tf;
}

int launch_generate_rays(const double* kinv, const double* r, const double* t, const double* o, const float* bounds,
                         int H, int W, float* ray_d, float* near, float* far, uint8_t* mask, hipStream_t st) {
    RayCam c;
    for (int k = 0; k < 9; ++k) c.kinv[k] = kinv[k];
    ray_pose_from_host(&c.p, r, t, o, bounds);
    const int64_t n = (int64_t)H * W;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_generate_rays, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, c, H, W, ray_d, near, far, mask);
    INVR_LAUNCH_CHECK();
    return 0;
}
