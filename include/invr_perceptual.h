/* libinvr — the perceptual (cfg.use_lpips) image term of the training objective, entry points of libinvr.so next to include/invr.h.
 *
 * The reference's PerceptualLoss (lib/train/trainers/loss/perceptual_loss.py:45-68) on the patch re-assembled from mask_at_box
 * (inb_trainer.py:188-214):
 *
 *     lpips = (L1(relu1_2) + L1(relu2_2)) / 2 + L1(image) + MSE(image)
 *
 * over the frozen prefix conv3-64, relu, conv64-64, relu, maxpool 2x2, conv64-128, relu, conv128-128, relu of a VGG19, forward for
 * the predicted and the target image and backward to the predicted image only (the weights get no gradient).
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `stream` is a hipStream_t.  The calls allocate nothing, read nothing back, launch on `stream` only, use no
 * floating-point atomics (the same inputs give the same bits in every run) and can be captured in a hipGraph.
 *
 * Discrete rules (torch's): ReLU' = 1 where the stored activation is > 0; sign(0) = 0; the pool's gradient goes to the first
 * maximum of its window in row-major order.
 */
#ifndef INVR_PERCEPTUAL_H
#define INVR_PERCEPTUAL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_PERCEPTUAL_MAX_SIDE 2048

/* Arrays of one forward + backward in the caller's workspace: BYTE offsets.  P = H*W, p = (H/2)*(W/2); every float array of two
 * images is [image (0 predicted, 1 target)][channel][row][column]. */
typedef struct InvrPerceptualLayout {
    int64_t rank;      /* int32 [P]        : row of rgb_map / rgb_gt a pixel takes its value from, -1 where mask_at_box is 0 */
    int64_t img;       /* float [2][3][P]  : the assembled images (zeros; img[mask] = rgb) */
    int64_t a11;       /* float [2][64][P] : relu(conv1_1) */
    int64_t a12;       /* float [2][64][P] : relu(conv1_2) = relu1_2 */
    int64_t pool;      /* float [2][64][p] : maxpool 2x2 of a12 */
    int64_t a21;       /* float [2][128][p]: relu(conv2_1) */
    int64_t a22;       /* float [2][128][p]: relu(conv2_2) = relu2_2 */
    int64_t partial;   /* double[n_partial]: per-wave sums of |relu1_2 difference| (n_part1), then of |relu2_2 difference| (n_part2),
                          then the image's sum |d| and sum d^2 */
    int64_t out8;      /* float [8]        : invr_perceptual_fwd's out8 of the last forward */
    int64_t g22;       /* float [128][p]   : gradient arriving at a22 (predicted image) = g_loss / (2 numel) * sign(difference) */
    int64_t gm22;      /* float [128][p]   : g22 where a22 > 0, else 0 */
    int64_t g21;       /* float [128][p]   : gradient arriving at a21 */
    int64_t gm21;      /* float [128][p]   */
    int64_t gpool;     /* float [64][p]    : gradient arriving at the pooled map */
    int64_t g12;       /* float [64][P]    : gradient arriving at a12 = pool routing + g_loss / (2 numel) * sign(difference) */
    int64_t gm12;      /* float [64][P]    */
    int64_t g11;       /* float [64][P]    : gradient arriving at a11 */
    int64_t gm11;      /* float [64][P]    */
    int64_t gimg;      /* float [3][P]     : gradient of the assembled predicted image */
    int64_t n_part1, n_part2, n_partial;
    int64_t bytes;
} InvrPerceptualLayout;

/* Packed weight image: for each of the four convolutions the MFMA A-operand stream of the forward pass and of the data-gradient
 * pass (the 180-degree-rotated, in/out-transposed weights), then the four biases.  Build it once per version of the weights. */
int64_t invr_perceptual_packed_floats(void);
/* w[4], b[4]: HOST arrays of device pointers to torch's (out, in, 3, 3) weights / (out) biases of conv1_1, conv1_2, conv2_1, conv2_2. */
int invr_perceptual_pack_weights(const float* const* w, const float* const* b, float* packed, void* stream);

size_t invr_perceptual_workspace_bytes(int32_t H, int32_t W);      /* 0 for sizes outside [2, INVR_PERCEPTUAL_MAX_SIDE] */
int invr_perceptual_workspace_layout(int32_t H, int32_t W, InvrPerceptualLayout* layout);

/* rgb_map, rgb_gt (n_rays, 3): the values of the set bytes of mask_at_box (uint8, H*W) in row-major order; set bytes beyond
 * n_rays are treated as unset.  out8 = {lpips, L1(relu1_2), L1(relu2_2), L1(image), MSE(image), 0, 0, 0}.  The workspace
 * (256-byte aligned) keeps everything the backward needs. */
int invr_perceptual_fwd(const float* packed, const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, int64_t n_rays,
                        int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream);
/* After invr_perceptual_fwd on the same workspace.  g_loss: 1 float on the device.  g_rgb (n_rays, 3) = d lpips / d rgb_map * g_loss;
 * gradients of masked-out pixels are dropped; nothing is written when n_rays == 0. */
int invr_perceptual_bwd(const float* packed, const uint8_t* mask_at_box, int64_t n_rays, int32_t H, int32_t W, void* workspace,
                        size_t workspace_bytes, const float* g_loss, float* g_rgb, void* stream);

/* NetworkWrapper's objective with the perceptual image term (inb_trainer.py:45-98, 206-214): invr_train_loss_fwd / _bwd of
 * include/invr.h with lpips in the place of the MSE in the sum, added in the same order: pair, distortion, offset, image term.
 * out8 = {loss, img_loss (MSE of the rays, a statistic), psnr, reg_dist, offset_loss, pair_loss, lpips, 0}; err (n_rays) = sum_c |rgb - gt|
 * or NULL.  g_rgb carries only the perceptual gradient. */
int invr_train_loss_lpips_fwd(const float* packed, const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, const float* dist,
                              const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist, float w_off,
                              int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err, void* stream);
int invr_train_loss_lpips_bwd(const float* packed, const uint8_t* mask_at_box, const float* terms, int64_t n_rays, int32_t H, int32_t W,
                              float w_pair, float w_dist, float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes,
                              const float* g_loss, float* g_rgb, float* g_dist, float* g_terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif
