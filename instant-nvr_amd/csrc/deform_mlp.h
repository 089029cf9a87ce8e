// The residual deformer (uv_deformer.py:23-45: UV-volume trilinear -> (u,v,t) -> 8-level F=2 grid encoder -> 19-32-32-3 Softplus
// MLP -> 0.05 * tanh), stated once per form:
//   scalar : deform_fwd_act<BWD>, one thread per point, weights through any pointers (k_warp.hip: k_warp_dense, k_deform_points;
//            k_train.hip: k_pair_term_fwd, k_deform_bwd), with stage_deform_weights for the kernels that read them from LDS
//   MFMA   : the DF_O_* weight image in matrix-core operand order, log2-domain scales folded in (k_warp.hip: k_deform_pairs, which
//            stages it and is the one statement of this form)
#pragma once
#include "pipeline.h"
#include "grid_generic.h"
#include "mlp_common.h"

// ---- thread-per-point form, forward with kept activations ----------------------------------------------------------------
// (BWD: the backward's recompute — activations AND their derivative factors softplus'(z) = sigmoid(z) formed from the pre-activation
// (sigmoid_acc: ~3 ulp RELATIVE for every z).  The earlier form 1 - exp(-softplus(z)) is a cancellation for z < 0: 6e-8 ABSOLUTE error on a
// factor ~e^z, and with Adam's eps = 1e-15 every extra bit of gradient noise flips the sign of more rounding-level steps — the
// deformer's first layer agreed with the float32 oracle on 0.67-0.94 of its elements after three steps, 0.99 now
// (tests/test_gpu_training.py::test_configs3_real_shape_three_steps_vs_oracle_autograd))
// th = tanh of the head: the residual is 0.05 * th (the backward needs th itself)
template <bool BWD> struct DeformActT { float feat[19]; float h1[32]; float h2[32]; float th[3]; float s1[BWD ? 32 : 1]; float s2[BWD ? 32 : 1]; };
typedef DeformActT<false> DeformAct;

// (the weights through any pointers: the MlpDev's global tensors, or a workgroup's LDS copy — same operations, same order)
template <bool BWD>
__device__ __forceinline__ void deform_fwd_act_w(const SceneDev& s, const GridDev& dg, const float* W0, const float* B0, const float* W1,
                                                 const float* B1, const float* W2, const float* B2, const float* xb, float* uvt,
                                                 DeformActT<BWD>& a) {
    sample_volume_dev<2>(s.tuv, 0, xb[0], xb[1], xb[2], uvt);
    uvt[2] = s.frame_dim[0];
    grid_encode_concat<8, 2>(dg, uvt, a.feat);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        float acc = B0[j];
#pragma unroll
        for (int i = 0; i < 19; ++i) acc = fmaf(W0[j * 19 + i], a.feat[i], acc);
        a.h1[j] = softplus_f(acc);
        if (BWD) a.s1[j] = sigmoid_acc(acc);
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // (keeps the weight loads of later neurons from being hoisted: registers)
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        float acc = B1[j];
#pragma unroll
        for (int i = 0; i < 32; ++i) acc = fmaf(W1[j * 32 + i], a.h1[i], acc);
        a.h2[j] = softplus_f(acc);
        if (BWD) a.s2[j] = sigmoid_acc(acc);
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float acc = B2[j];
#pragma unroll
        for (int i = 0; i < 32; ++i) acc = fmaf(W2[j * 32 + i], a.h2[i], acc);
        a.th[j] = tanhf(acc);
    }
}
template <bool BWD>
__device__ __forceinline__ void deform_fwd_act(const SceneDev& s, const GridDev& dg, const MlpDev& dm, const float* xb, float* uvt,
                                               DeformActT<BWD>& a) {
    deform_fwd_act_w<BWD>(s, dg, dm.w[0], dm.b[0], dm.w[1], dm.b[1], dm.w[2], dm.b[2], xb, uvt, a);
}

// ---- the weights as a row-major LDS image (they are ~1100 wave-uniform vector loads per thread when read from global memory) ----
#define DM_O_W0 0                       // 32 x 19
#define DM_O_B0 (DM_O_W0 + 32 * 19)
#define DM_O_W1 (DM_O_B0 + 32)          // 32 x 32
#define DM_O_B1 (DM_O_W1 + 32 * 32)
#define DM_O_W2 (DM_O_B1 + 32)          // 3 x 32
#define DM_O_B2 (DM_O_W2 + 3 * 32)
#define DM_LDS (DM_O_B2 + 4)
// block-cooperative (block >= 96 threads = the caller's workgroup size); the caller's __syncthreads follows, then
// deform_fwd_act_w reads the image through lw + DM_O_*
__device__ __forceinline__ void stage_deform_weights(float* lw, const MlpDev& dm, const int block) {
    for (int k = threadIdx.x; k < 32 * 19; k += block) lw[DM_O_W0 + k] = dm.w[0][k];
    for (int k = threadIdx.x; k < 32 * 32; k += block) lw[DM_O_W1 + k] = dm.w[1][k];
    if (threadIdx.x < 96) lw[DM_O_W2 + threadIdx.x] = dm.w[2][threadIdx.x];
    if (threadIdx.x < 32) { lw[DM_O_B0 + threadIdx.x] = dm.b[0][threadIdx.x]; lw[DM_O_B1 + threadIdx.x] = dm.b[1][threadIdx.x]; }
    if (threadIdx.x < 3) lw[DM_O_B2 + threadIdx.x] = dm.b[2][threadIdx.x];
}

// ---- the weights in MFMA operand order (D^T = W . X^T as in k_part_mlp: 16 pairs = the N columns of v_mfma_f32_16x16x4_f32) ----
// In a 16-pair tile lane (g = lane>>4, col = lane&15) encodes levels 2g and 2g+1 of pair col, so the K order of layer 1 is permuted
// to match: k-slot (s<4, g) = feature 3 + 2*(2g + s/2) + s%2, (4, g) = uvt[g].
// The hidden activations are kept in the log2 domain, u = log2(1 + exp2(z log2e)) = softplus(z) / ln2 (mlp_common.h:
// softplus4_log2), with the two scale factors folded into the staged weights as in the part MLPs: a layer that feeds a Softplus is
// scaled by log2e (weights and bias), a layer that consumes Softplus outputs by ln2 — for the hidden-to-hidden layer the two cancel,
// only its bias is scaled.  {min, exp2, add, log2} = 4 instructions per value instead of the 7 of softplus_f; 64 values per pair.
#define DF_BLOCK 256
#define DF_O_W1 0                       // 5 k-steps * 2 m-tiles * 64 lanes
#define DF_O_W2 (DF_O_W1 + 5 * 2 * 64)  // 8 * 2 * 64
#define DF_O_B1 (DF_O_W2 + 8 * 2 * 64)  // 32
#define DF_O_B2 (DF_O_B1 + 32)          // 32
#define DF_O_V (DF_O_B2 + 32)           // 3 * 32, slot order [c][g*8 + mt*4 + r]
#define DF_O_B3 (DF_O_V + 96)           // 3 (+1)
#define DF_LDS (DF_O_B3 + 4)

__device__ __forceinline__ int df_col(int s, int g) { return s < 4 ? 3 + 2 * (2 * g + (s >> 1)) + (s & 1) : (g < 3 ? g : -1); }
