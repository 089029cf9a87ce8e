/* libinvr — the Evaluator's LPIPS (v0.1, net='vgg', spatial=False, eval mode) on the device, entry points of libinvr.so next to
 * include/invr.h.
 *
 * The reference's evaluator (lib/evaluators/if_nerf.py:23, 118-122) calls lpips.LPIPS(net='vgg') on the two re-assembled H x W images
 * WITHOUT normalize=True: the [0, 1] images go in as they are.  So do they here:
 *
 *     x_c      = (img_c - shift_c) / scale_c                          fp32, one subtraction and one division, each rounded once
 *     features = VGG16: 3x3 convolutions (padding 1 of true zeros on the scaled tensor, stride 1, bias), ReLU (v > 0 ? v : 0) after
 *                each, channel plan 3-64, 64-64 | 64-128, 128-128 | 128-256, 256-256 x2 | 256-512, 512-512 x2 | 512-512 x3, a 2x2
 *                stride-2 floor max-pool in front of blocks 2..5; taps at relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
 *     per tap, in double from the stored fp32 features, per pixel:
 *                S_k = sum_c x_k,c^2,  n_k,c = x_k,c / (sqrt(S_k) + (double)1e-10f),  d = sum_c lin_c (n_0,c - n_1,c)^2
 *     layer_l  = sum_pixels d / (h_l w_l)
 *     lpips    = ((((layer_0 + layer_1) + layer_2) + layer_3) + layer_4)
 *
 * Every convolution is an implicit GEMM of exact fp32 products accumulated in fp32 (v_mfma_f32_16x16x4_f32); both images of a frame
 * go through identical arithmetic per element, so where they agree on a unit's receptive field their features are bit-equal.
 *
 * Rules, as include/invr.h states them: plain pointers and sizes; every function returning int returns 0 on success, else a status
 * with the message in invr_last_error(); arguments are checked ahead of any launch.  All data pointers are device pointers unless
 * said otherwise; `stream` is a hipStream_t.  The calls allocate nothing, read nothing back, launch on `stream` only, use no
 * floating-point atomics (partial sums of 16 pixels each at fixed slots, formed and then added in a fixed order by one final pass:
 * the same inputs give the same bits in every run) and can be captured in a hipGraph.
 */
#ifndef INVR_LPIPS_H
#define INVR_LPIPS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVR_LPIPS_MIN_SIDE 16          /* below it the relu5_3 map is empty */
#define INVR_LPIPS_MAX_SIDE 2048
#define INVR_LPIPS_KEEP_MAX_BYTES 2147483648ll          /* a keep = 1 layout beyond 2 GiB is refused (keep = 1 is for tests) */

/* Arrays of one forward in the caller's workspace: BYTE offsets.  Layer l of the 13 convolutions has C_l output channels on the
 * h_l x w_l map of its block (block b: H >> b, W >> b); every float array is [image (0 predicted, 1 target)][channel][row][column].
 * With keep = 1 every array has a place of its own; with keep = 0 the activations and pooled maps rotate through two buffers (a
 * tap is consumed by its distance pass before it is overwritten) and the offsets say where each array WAS while it lived. */
typedef struct InvrLpipsLayout {
    int64_t scaled;          /* float [2][3][H*W]      : the scaling layer's output, planar */
    int64_t act[13];         /* float [2][C_l][h_l w_l]: relu(conv_l) */
    int64_t pool[4];         /* float [2][C][h w]      : the pooled map in front of block 2..5 */
    int64_t partial;         /* double[n_partial]      : sums of d over 16 pixels each (one slot per workgroup), tap after tap */
    int64_t part_off[5];     /* first slot of tap l in `partial` */
    int64_t n_part[5];       /* slots of tap l */
    int64_t n_partial;
    int64_t bytes;
} InvrLpipsLayout;

/* Packed weight image: for each of the 13 convolutions the MFMA A-operand stream and its bias, then the five lin vectors, then
 * shift and scale.  Build it once per version of the weights. */
int64_t invr_lpips_packed_floats(void);
/* w[13], b[13], lin[5]: HOST arrays of device pointers to torch's (out, in, 3, 3) weights, (out) biases and the (C) weights of the
 * bias-free 1x1 lin layers; shift3, scale3: 3 floats each on the device. */
int invr_lpips_pack_weights(const float* const* w, const float* const* b, const float* const* lin, const float* shift3, const float* scale3,
                            float* packed, void* stream);

/* 0 for sizes outside [INVR_LPIPS_MIN_SIDE, INVR_LPIPS_MAX_SIDE] and for a keep = 1 layout beyond INVR_LPIPS_KEEP_MAX_BYTES */
size_t invr_lpips_workspace_bytes(int32_t H, int32_t W, int32_t keep);
int invr_lpips_workspace_layout(int32_t H, int32_t W, int32_t keep, InvrLpipsLayout* layout);

/* img_pred, img_gt (H, W, 3) float32, interleaved, as invr_image_assemble leaves them.  out8 (8 doubles on the device) =
 * {lpips, layer_0 .. layer_4, 0, 0}.  The workspace is 256-byte aligned. */
int invr_lpips_fwd(const float* packed, const float* img_pred, const float* img_gt, int32_t H, int32_t W, int32_t keep, void* workspace,
                   size_t workspace_bytes, double* out8, void* stream);

#ifdef __cplusplus
}
#endif
#endif
