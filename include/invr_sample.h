/* libinvr — one plain N_rand ray batch from a device-resident frame, entry point of libinvr.so next to include/invr.h.
 *
 * The plain branch of the reference's dataset (lib/datasets/h36m/tpose_dataset.py:442-450 -> sample_ray_h36m,
 * lib/utils/if_nerf/if_nerf_data_utils.py:228-297) after its host-side draw: every ray of the batch names a pixel of the frame as the
 * k-th member, in row-major order, of one of three pixel classes (body, face, bound); the call resolves the pixel and writes its ray
 * (get_rays :24-38), its near / far (get_near_far :92-107, in float64 as that function is handed float64 rays there), the frame's
 * pixel and the byte of the occupancy mask — in one launch, from an image, a mask and three bit planes that stay on the device.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; the function returns 0 on success, else a status with the message
 * in invr_last_error(); arguments are checked ahead of the launch (null pointers, H / W < 1, n outside 1..INVR_RAY_BATCH_MAX).  `img`,
 * `occ_msk`, `planes`, `row_prefix`, `sel` and every output are DEVICE pointers; `k_inv`, `R`, `T`, `cam_o` and `bounds` are HOST
 * arrays read during the call; `stream` is a hipStream_t.  The call allocates nothing, reads nothing back, launches one kernel on
 * `stream` only and can be captured in a hipGraph.
 *
 * THE CONTRACT
 *
 * Frame.  img[H][W][3] fp32 and occ_msk[H][W] bytes.
 *
 * Classes.  Wr = (W + 63) / 64.  planes[3][H][Wr] are 64-bit words: bit b of word j of row y of class c is set iff pixel (x = 64 j + b, y)
 * belongs to class c; bits at x >= W are zero.  row_prefix[3][H + 1] int32: row_prefix[c][y] = the number of members of class c in the
 * rows before y, so row_prefix[c][0] = 0 and row_prefix[c][H] = the size of the class.  The members of a class are ranked in row-major
 * order (y, then x): rank 0 is the first.
 *
 * Selection.  sel[n][2] int32 = (class, rank) per ray.  Ray i resolves to the pixel (x, y) that is member `rank` of class `class`.
 * sel is device data and is not checked: a class outside {0, 1, 2} or a rank outside 0 .. size - 1 is the caller's error and the
 * result of such a row is undefined (the kernel neither clamps nor reports it).  Duplicates are fine.
 *
 * Ray of a pixel.  k_inv (3,3) row-major is the float64 inverse of the frame's float64 intrinsic matrix.  With i = (double)(float)x,
 * j = (double)(float)y, every operation in double, left to right, no contraction:
 *     pc[a] = (i * k_inv[a][0] + j * k_inv[a][1]) + k_inv[a][2]
 *     d     = (pc - T) @ R - cam_o,   u = d / |d|                    (as invr_generate_rays)
 * and the slab test stays in double: norm = |u|, v = u / norm with v in (-1e-10, 1e-5) replaced by 1e-5 and then v in (-1e-5, 1e-10)
 * by -1e-5; t0 = (bounds[0] - cam_o) / v, t1 = (bounds[1] - cam_o) / v with bounds promoted from float32; tn = max over the axes of
 * min(t0, t1), tf = min over the axes of max(t0, t1).  Only the stores round to float32:
 *     ray_d = (float)u,   near = (float)(tn / norm),   far = (float)(tf / norm)
 * No ray is dropped: whether tn < tf is the caller's to know (the host decides it before it selects a rank).
 *
 * Outputs.  Row i, for every i < n and no other: ray_d (n,3); near, far (n); rgb (n,3) = the three floats of img at the pixel, bit for
 * bit; occupancy (n) = the byte of occ_msk at the pixel; coord (n,2) int64 = (y, x).
 *
 * Determinism.  The same inputs give the same bits over any dirty buffers; there are no atomics.
 */
#ifndef INVR_SAMPLE_H
#define INVR_SAMPLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_RAY_BATCH_MAX 1048576

int invr_ray_batch(const float* img, const uint8_t* occ_msk, const uint64_t* planes, const int32_t* row_prefix,
                   int32_t H, int32_t W, const int32_t* sel, int32_t n,
                   const double* k_inv, const double* R, const double* T, const double* cam_o, const float* bounds,
                   float* ray_d, float* near, float* far, float* rgb, uint8_t* occupancy, int64_t* coord, void* stream);

#ifdef __cplusplus
}
#endif
#endif
