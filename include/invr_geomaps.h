/* libinvr — per-ray geometry maps of a render (depth, first surface crossing, surface normal), entry points of libinvr.so next to
 * include/invr.h.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers;
 * `stream` is a hipStream_t.  The calls allocate nothing, read nothing back, launch on `stream` only and can be captured in a
 * hipGraph.  Zero rays / rows is a no-op that returns 0.
 *
 * THE CONTRACT
 *
 * Depth.  Per ray r of n_samples samples with occupancies occ_i and sample depths z_i:
 *     depth_map[r]  = sum_i w_i * z_i (fp32), w = render_weights as the compositing forms it (lib/utils/net_utils.py:12-15 of the
 *                     reference): w_i = occ_i * prod_{j<i} (1 - occ_j + eps), the same scan, bit for bit the `weights` of the render;
 *     surf_index[r] = the first sample i with occ_i >= level (an fp32 comparison; a NaN is not a crossing), or -1 if there is none;
 *     surf_depth[r] = crossing at i > 0: z_{i-1} + t * (z_i - z_{i-1}) with t = (level - occ_{i-1}) / (occ_i - occ_{i-1}), all fp32
 *                     (a culled sample has occupancy 0; a NaN occ_{i-1} interpolates as 0, as in include/invr_mesh.h);
 *                     crossing at i = 0: z_0;  no crossing: +0.0f.
 * z_i = near + (far - near) * i / (n_samples - 1) in the renderer's fp32 form (the z_vals of an unjittered invr_render_fwd), or
 * z_vals[r][i] where a z_vals (n_rays, n_samples) pointer is given (renders with jitter).  Every one of the n_rays entries of every
 * output that is not NULL is written, and nothing else.  A ray without survivors gets 0, -1, 0.
 *
 * Stencil.  For the j-th listed ray row = rows[j] (int32, ascending, each with surf_index >= 0): x = fmaf(surf_depth[row],
 * ray_d[row], ray_o[row]) per component; pts[6 j + k] = x + h e_x, x - h e_x, x + h e_y, x - h e_y, x + h e_z, x - h e_z for
 * k = 0..5 (one fp32 addition on the moved coordinate), dirs[6 j + k] = ray_d[row].  pts and dirs are (6 n, 3).
 *
 * Normals.  occ6 (n, 6) = the field's occupancy at the six points of every listed ray.  g = (o[0] - o[1], o[2] - o[3],
 * o[4] - o[5]), |g|^2 = (gx^2 + gy^2) + gz^2 in fp32; surf_normal[row] = -g / sqrt(|g|^2) (the field rises inwards) and
 * surf_mask[row] = 1.  Where |g|^2 is 0 or not finite the normal is three +0.0f and the mask 0.  Rows that are not listed are not
 * written: the caller clears surf_normal (n_rays, 3) and surf_mask (n_rays, uint8) first.
 *
 * Not here: gradients of the maps, and a normal from the field's analytic gradient.
 */
#ifndef INVR_GEOMAPS_H
#define INVR_GEOMAPS_H
#include <stddef.h>
#include <stdint.h>
#include "invr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_SIZEOF_GEO_OUT 10      /* invr_sizeof(INVR_SIZEOF_GEO_OUT) = sizeof(InvrGeoOut) */

/* The geometry outputs of invr_render_fwd_geo; any pointer may be NULL (that map is not formed). */
typedef struct InvrGeoOut {
    float level;             /* the crossing level; finite */
    float* depth_map;        /* (n_rays) */
    int32_t* surf_index;     /* (n_rays) */
    float* surf_depth;       /* (n_rays) */
} InvrGeoOut;

/* The dense form: occ (n_rays, n_samples), near / far (n_rays) or z_vals (n_rays, n_samples) — near and far may be NULL when z_vals
 * is given.  eps is render_weights' epsilon (0 for the INB call, 1 under cfg.random_bg). */
int invr_depth_fwd(const float* occ, const float* near, const float* far, const float* z_vals, int64_t n_rays, int32_t n_samples,
                   float eps, float level, float* depth_map, int32_t* surf_index, float* surf_depth, void* stream);

/* invr_render_fwd (raw_dirty NULL: raw_rows is ignored) or invr_render_fwd_tracked (raw_dirty given) with the depth pass behind the
 * compositing, reading the frame's merged per-survivor results in the workspace: the render's outputs keep their bits.  eps is
 * InvrScene::composite_eps.  A call with jitter needs z_vals (the depths it writes are the ones the maps are formed with).
 * geo NULL: the plain render. */
int invr_render_fwd_geo(const InvrScene* scene, const InvrModel* model,
                        const float* ray_o, const float* ray_d, const float* near, const float* far,
                        const float* jitter, int64_t n_rays, int32_t n_samples,
                        float* rgb_map, float* acc_map, float* raw, float* occ, float* weights,
                        float* z_vals, int32_t* stats,
                        void* workspace, size_t workspace_bytes, int64_t max_active, void* stream,
                        uint64_t* raw_dirty, int64_t raw_rows, const InvrGeoOut* geo);

/* h > 0 and finite. */
int invr_surface_stencil(const float* ray_o, const float* ray_d, const float* surf_depth, const int32_t* rows, int64_t n, float h,
                         float* pts, float* dirs, void* stream);

int invr_stencil_normals(const float* occ6, const int32_t* rows, int64_t n, float* surf_normal, uint8_t* surf_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
