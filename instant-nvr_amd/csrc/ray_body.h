// One pixel's ray from its camera-space point: the part of get_rays + get_near_far of the reference's dataset code
// (lib/utils/if_nerf/if_nerf_data_utils.py:33-38, 92-107) that k_generate_rays (full frames, pixel_camera in float64) and
// k_patch_batch (training patches, pixel_camera in float32) share.  Stated once so that both kernels round alike.
#pragma once
#include "common.h"

struct RayPose {
    double r[9], t[3], o[3];          // camera rotation (row-major), translation, centre -R^T T
    float bounds[6];                  // world AABB, (2,3)
};

// pc = pixel_camera promoted to double.  (pc - T) @ R, minus the camera centre, normalised in double, cast to float32 (rd); then the
// ray / AABB slab test in float32 against the float32 camera centre.  near / far are the values the reference keeps for a ray inside
// the box (t / |d|); the return value is mask_at_box.
__device__ __forceinline__ bool ray_from_pixel_camera(const double pc[3], const RayPose& c, float rd[3], float& near, float& far) {
    double pw[3], d[3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
        pw[b] = (pc[0] - c.t[0]) * c.r[b] + (pc[1] - c.t[1]) * c.r[3 + b] + (pc[2] - c.t[2]) * c.r[6 + b];   // (pc - T) @ R
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = pw[a] - c.o[a];
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    float ro[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { rd[a] = (float)(d[a] / nrm); ro[a] = (float)c.o[a]; }
    // get_near_far in float32
    const float norm_d = sqrtf(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]);
    float tn = -__builtin_inff(), tf = __builtin_inff();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v = rd[a] / norm_d;
        if (v < 1e-5f && v > -1e-10f) v = 1e-5f;
        if (v > -1e-5f && v < 1e-10f) v = -1e-5f;
        const float t0 = (c.bounds[a] - ro[a]) / v, t1 = (c.bounds[3 + a] - ro[a]) / v;
        tn = fmaxf(tn, fminf(t0, t1));
        tf = fminf(tf, fmaxf(t0, t1));
    }
    near = tn / norm_d;
    far = tf / norm_d;
    return tn < tf;
}

static inline void ray_pose_from_host(RayPose* c, const double* r, const double* t, const double* o, const float* bounds) {
    for (int k = 0; k < 9; ++k) c->r[k] = r[k];
    for (int k = 0; k < 3; ++k) { c->t[k] = t[k]; c->o[k] = o[k]; }
    for (int k = 0; k < 6; ++k) c->bounds[k] = bounds[k];
}
