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

// The same ray with the slab test kept in float64: what sample_ray_h36m (:276-280) computes, which hands get_near_far the float64
// rays of get_rays and the float64 camera centre (bounds stay float32 and are promoted).  Nothing is rounded to float32 before the
// stores: rd = (float)u, near = (float)(tn / |u|), far = (float)(tf / |u|), where ray_from_pixel_camera above rounds u first and
// runs every later operation in float32.  The return value is near < far of the float64 values.
__device__ __forceinline__ bool ray_from_pixel_camera_f64(const double pc[3], const RayPose& c, float rd[3], float& near, float& far) {
    double pw[3], d[3], u[3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
        pw[b] = (pc[0] - c.t[0]) * c.r[b] + (pc[1] - c.t[1]) * c.r[3 + b] + (pc[2] - c.t[2]) * c.r[6 + b];   // (pc - T) @ R
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = pw[a] - c.o[a];
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) { u[a] = d[a] / nrm; rd[a] = (float)u[a]; }
    // get_near_far in float64
    const double norm_d = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double tn = -__builtin_inf(), tf = __builtin_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double v = u[a] / norm_d;
        if (v < 1e-5 && v > -1e-10) v = 1e-5;
        if (v > -1e-5 && v < 1e-10) v = -1e-5;
        const double t0 = ((double)c.bounds[a] - c.o[a]) / v, t1 = ((double)c.bounds[3 + a] - c.o[a]) / v;
        tn = fmax(tn, fmin(t0, t1));
        tf = fmin(tf, fmax(t0, t1));
    }
    near = (float)(tn / norm_d);
    far = (float)(tf / norm_d);
    return tn < tf;
}

static inline void ray_pose_from_host(RayPose* c, const double* r, const double* t, const double* o, const float* bounds) {
    for (int k = 0; k < 9; ++k) c->r[k] = r[k];
    for (int k = 0; k < 3; ++k) { c->t[k] = t[k]; c->o[k] = o[k]; }
    for (int k = 0; k < 6; ++k) c->bounds[k] = bounds[k];
}
