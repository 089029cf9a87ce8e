/* libinvr — one training patch from a device-resident frame, entry point of libinvr.so next to include/invr.h.
 *
 * The patch branch of the reference's dataset (lib/datasets/h36m/tpose_dataset.py:421-441) after its host-side window draw: the rays
 * of a w x h window of a frame (get_rays_coord + get_near_far, lib/utils/if_nerf/if_nerf_data_utils.py:41-59, 92-107), the rays
 * that meet the body's box compacted in pixel order, and the frame's pixels and mask gathered for them — in one launch, from an image
 * and a mask that stay on the device.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; the function returns 0 on success, else a status with the message
 * in invr_last_error(); arguments are checked ahead of the launch (null pointers, H / W < 1, w / h outside 1..INVR_PATCH_MAX_SIDE, a
 * window that leaves the frame).  `img`, `msk` and every output are DEVICE pointers; `k_inv`, `R`, `T`, `cam_o` and `bounds` are HOST
 * arrays read during the call; `stream` is a hipStream_t.  The call allocates nothing, reads nothing back, launches one kernel on
 * `stream` only and can be captured in a hipGraph.
 *
 * THE CONTRACT
 *
 * Frame and window.  img[H][W][3] fp32 and msk[H][W] bytes.  The window's local pixel (x, y), 0 <= x < w, 0 <= y < h, is the frame's
 * pixel (x0 + x, y0 + y).  Pixels run over the window in row-major order: p = y * w + x.
 *
 * Ray of a pixel.  k_inv (3,3) row-major is the float32 inverse of the window's float32 intrinsic matrix (the reference has cast K
 * to float32 by then, so its pixel_camera is float32).  With i = (float)x, j = (float)y, every operation rounded to float32, left to
 * right, no contraction:
 *     pc[a] = (i * k_inv[a][0] + j * k_inv[a][1]) + k_inv[a][2]
 * From there on in double, as invr_generate_rays: d = (pc - T) @ R - cam_o, ray_d = (float)(d / |d|); then in float32 the slab test
 * of ray_d against bounds (2,3) from the float32 camera centre: near, far, and inside := near < far.
 *
 * Outputs.  mask_at_box[p] = inside(p) as 0 / 1, written for every pixel of the window.  The k-th inside pixel in pixel order writes
 * row k of the compact arrays: ray_d (.,3); near, far (.); rgb (.,3) = the three floats of img at the frame pixel, bit for bit;
 * occupancy (.) = (msk at the frame pixel > 0) as 0 / 1; coord (.,2) = (uint8)x, (uint8)y.  count[0] = the number of inside pixels.
 * Rows at or past count are not written: every compact array holds w * h rows at the caller's.
 *
 * Determinism.  The same inputs give the same bits over any dirty buffers; there are no atomics.
 */
#ifndef INVR_BATCH_H
#define INVR_BATCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_PATCH_MAX_SIDE 256

int invr_patch_batch(const float* img, const uint8_t* msk, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
                     const float* k_inv, const double* R, const double* T, const double* cam_o, const float* bounds, float* ray_d,
                     float* near, float* far, float* rgb, uint8_t* occupancy, uint8_t* coord, uint8_t* mask_at_box, int32_t* count,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
