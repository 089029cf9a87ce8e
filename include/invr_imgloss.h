/* libinvr — the SSIM (cfg.use_ssim) and total-variation (cfg.use_tv_image) image terms of the training objective, entry points of
 * libinvr.so next to include/invr.h.
 *
 * Both terms work on the patch re-assembled from mask_at_box (inb_trainer.py:196-207): img = zeros(H, W, 3); img[mask_at_box] = values
 * for the prediction and the target, and for TV mask_gt = zeros(H, W, bool); mask_gt[mask_at_box] = occupancy.  The assembly is the one
 * of include/invr_perceptual.h (k_perc_assemble's rank array: the row a pixel takes its value from, -1 where the mask is 0; set bytes
 * beyond n_rays are treated as unset); mask_gt is a gather through that array.
 *
 * SSIM (lib/utils/loss_utils.py:7-37, SSIM(window_size = w), size_average = True): taps g (w floats on the device, w odd, <= 31;
 * the reference's are exp(-(k - w/2)^2 / (2 1.5^2)) normalised, formed as torch forms them: invr.losses.gaussian_taps), window g g^T per
 * channel with zero padding w/2, evaluated separably (rows, then columns: the reference's 2-D fp32 window up to rounding).  Five filtered
 * maps per channel: mu1 = G*x, mu2 = G*y, e11 = G*x^2, e22 = G*y^2, e12 = G*xy (x the prediction, y the target); C1 = 0.01^2, C2 = 0.03^2;
 *
 *     N1 = 2 mu1 mu2 + C1    N2 = 2 (e12 - mu1 mu2) + C2    D1 = mu1^2 + mu2^2 + C1    D2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
 *     S = N1 N2 / (D1 D2)    ssim = mean(S) over 3 H W
 *
 * Backward, to the prediction only: p = dS/dmu1 (the e maps held fixed) = 2 mu2 (N2 - N1) / (D1 D2) + 2 mu1 S (1 / D2 - 1 / D1),
 * q = dS/de11 = -S / D2, r = dS/de12 = 2 N1 / (D1 D2); d ssim / d x = ((G*p) + 2 x (G*q) + y (G*r)) / (3 H W) — G is symmetric, so the
 * same zero-padded filter is its own adjoint — gathered back to the rays through the rank array; gradients of masked-out pixels are dropped.
 *
 * TV (lib/train/trainers/loss/tv_image_loss.py:11-21): dx = (img[:-1] - img[1:])^2 (H-1, W, 3), dy = (img[:, :-1] - img[:, 1:])^2
 * (H, W-1, 3); eps_x, eps_y = the maxima of the TARGET's dx, dy over all elements, zero-filled pixels included;
 *
 *     tv = (mean(relu(dx_pred - eps_x)[mask_gt[:-1, :]]) + mean(relu(dy_pred - eps_y)[mask_gt[:, :-1]])) / 2
 *
 * each mean over 3 k elements, k = the set pixels of mask_gt in that selection (the last row / column is in neither first operand).
 * relu'(0) = 0; the target carries no gradient.  k = 0: the mean of an empty selection is NaN, as in the reference, and so are tv and
 * the objective; that selection contributes nothing to the gradient.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `stream` is a hipStream_t.  The calls allocate nothing, read nothing back, launch on `stream` only, use no
 * floating-point atomics (means are fixed-order sums of float64 partials: the same inputs give the same bits in every run) and can be
 * captured in a hipGraph.
 */
#ifndef INVR_IMGLOSS_H
#define INVR_IMGLOSS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_IMGLOSS_MAX_SIDE 2048
#define INVR_IMGLOSS_MAX_WINDOW 31

/* Arrays of one forward + backward in the caller's workspace: BYTE offsets.  P = H*W; every float map is [channel][row][column].  One
 * workspace serves either term; a forward of one term overwrites what the other shares with it (rank, img, partial, out8, gimg). */
typedef struct InvrImglossLayout {
    int64_t rank;      /* int32 [P]        : row of rgb_map / rgb_gt a pixel takes its value from, -1 where mask_at_box is 0 */
    int64_t img;       /* float [2][3][P]  : the assembled images (0 predicted, 1 target) */
    int64_t mom;       /* float [5][3][P]  : SSIM: mu1, mu2, e11, e22, e12 */
    int64_t smap;      /* float [3][P]     : SSIM: S */
    int64_t pqr;       /* float [3][3][P]  : SSIM: p, q, r */
    int64_t occ;       /* uint8 [P]        : TV: mask_gt */
    int64_t tvmax;     /* float [2][n_tv]  : TV: per-workgroup maxima of the target's dx, then of its dy */
    int64_t partial;   /* double[n_partial]: SSIM: per-workgroup sums of S (n_ssim).  TV: per-workgroup sums of relu(dx - eps_x), then of
                          relu(dy - eps_y), then the two counts k_x, k_y (n_tv each).  The last two: the assembly's sum |d|, sum d^2 */
    int64_t out8;      /* float [8]        : invr_ssim_fwd's / invr_tv_fwd's out8 of the last forward */
    int64_t gimg;      /* float [3][P]     : gradient of the term w.r.t. the assembled predicted image (times g_loss) */
    int64_t n_ssim, n_tv, n_partial;
    int64_t bytes;
} InvrImglossLayout;

/* window: the SSIM window the workspace is to serve (odd, 1 .. INVR_IMGLOSS_MAX_WINDOW; TV ignores it).  0 bytes for a side outside
 * [2, INVR_IMGLOSS_MAX_SIDE] or such a window. */
size_t invr_imgloss_workspace_bytes(int32_t H, int32_t W, int32_t window);
int invr_imgloss_workspace_layout(int32_t H, int32_t W, int32_t window, InvrImglossLayout* layout);

/* rgb_map, rgb_gt (n_rays, 3): the values of the set bytes of mask_at_box (uint8, H*W) in row-major order.  taps: `window` floats.
 * out8 = {ssim, 1 - ssim, 0, 0, 0, 0, 0, 0}.  The workspace (256-byte aligned) keeps everything the backward needs. */
int invr_ssim_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, const float* taps, int32_t window, int64_t n_rays,
                  int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream);
/* After invr_ssim_fwd on the same workspace.  g_loss: 1 float on the device.  g_rgb (n_rays, 3) = d ssim / d rgb_map * g_loss; nothing is
 * written when n_rays == 0. */
int invr_ssim_bwd(const uint8_t* mask_at_box, const float* taps, int32_t window, int64_t n_rays, int32_t H, int32_t W, void* workspace,
                  size_t workspace_bytes, const float* g_loss, float* g_rgb, void* stream);

/* occupancy (n_rays): one uint8 per ray, mask_gt[mask_at_box] = occupancy != 0.
 * out8 = {tv, mean_x, mean_y, eps_x, eps_y, k_x, k_y, 0} (the two means, the target's two maxima, the two counts of selected pixels). */
int invr_tv_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* occupancy, const uint8_t* mask_at_box, int64_t n_rays, int32_t H,
                int32_t W, void* workspace, size_t workspace_bytes, float* out8, void* stream);
/* After invr_tv_fwd on the same workspace.  g_rgb (n_rays, 3) = d tv / d rgb_map * g_loss; nothing is written when n_rays == 0. */
int invr_tv_bwd(const uint8_t* mask_at_box, int64_t n_rays, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, const float* g_loss,
                float* g_rgb, void* stream);

/* NetworkWrapper's objective with the term in place (inb_trainer.py:45-98, 215-226): invr_train_loss_fwd / _bwd of include/invr.h with,
 * added in the reference's order — pair, distortion, offset, then (0.1 (1 - ssim) + img_loss) or (0.01 tv + img_loss).
 * out8 = {loss, img_loss, psnr, reg_dist, offset_loss, pair_loss, ssim_loss = 1 - ssim | tv_loss = tv, 0}; err (n_rays) = sum_c |rgb - gt|
 * or NULL.  g_rgb carries the MSE gradient plus the term's; g_dist and g_terms as in invr_train_loss_bwd. */
int invr_train_loss_ssim_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* mask_at_box, const float* taps, int32_t window,
                             const float* dist, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist,
                             float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err, void* stream);
int invr_train_loss_ssim_bwd(const uint8_t* mask_at_box, const float* taps, int32_t window, const float* terms, int64_t n_rays, int32_t H,
                             int32_t W, float w_pair, float w_dist, float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes,
                             const float* g_loss, float* g_rgb, float* g_dist, float* g_terms, void* stream);
int invr_train_loss_tv_fwd(const float* rgb_map, const float* rgb_gt, const uint8_t* occupancy, const uint8_t* mask_at_box, const float* dist,
                           const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist, float w_off,
                           int32_t use_pair, void* workspace, size_t workspace_bytes, float* out8, float* err, void* stream);
int invr_train_loss_tv_bwd(const uint8_t* mask_at_box, const float* terms, int64_t n_rays, int32_t H, int32_t W, float w_pair, float w_dist,
                           float w_off, int32_t use_pair, void* workspace, size_t workspace_bytes, const float* g_loss, float* g_rgb,
                           float* g_dist, float* g_terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif
