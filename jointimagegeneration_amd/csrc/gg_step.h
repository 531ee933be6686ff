// Reverse step of the LDM samplers on ONE element, each formula written once.  All fp32, every product and sum rounded on its own (no
// FMA contraction), IEEE division and square root; the torch restatements of the tests (tests/vq_ref.py, tests/progressive_ref.py) encode
// this order.
//   DDIM (ddim.py:190-204), scalar row {a_t, a_prev, sigma_t, sqrt(1 - a_t)[, noise coefficient]}:
//     pred_x0 = (x - sqrt(1 - a_t) * e) / sqrt(a_t) ;  x_prev = sqrt(a_prev) * pred_x0 + dir * e [+ coefficient * noise],
//     dir = sqrt(1 - a_prev - sigma_t^2) on sigma_t itself, not on the sigma_t * temperature that may scale the noise
//   ancestral (LatentDiffusion.p_sample, ddpm.py:1072-1083, 1109-1120), scalar row {sqrt_recip_alphas_cumprod[t],
//   sqrt_recipm1_alphas_cumprod[t], posterior_mean_coef1[t], posterior_mean_coef2[t], (t > 0) * exp(0.5 * posterior_log_variance_clipped[t])}:
//     x_recon = a * x - b * out  (out itself under GG_DDPM_PREDICTS_X0; clamped to [-1, 1] under GG_DDPM_CLIP)
//     x_prev = c1 * x_recon + c2 * x [+ sg * noise]
//   DPM-Solver++ (2M) in data prediction (Lu et al. 2022, Algorithm 2), scalar row {alpha_s, sigma_s, k_x, k_d, c0, c1} for the step
//   from the point s to the point t (alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda_t - lambda_s):
//     p = (x - sigma_s * out) / alpha_s  (out itself under GG_DDPM_PREDICTS_X0; clamped to [-1, 1] under GG_DDPM_CLIP)
//     D = p on a first-order step (c1 == 0), else c0 * p + c1 * hist, hist being the previous step's p
//     x_next = k_x * x + k_d * D,  k_x = sigma_t / sigma_s,  k_d = -alpha_t * expm1(-h)
//   inpainting blend (ddim.py:144-148, plms.py:147-150, ddpm.py:1212-1214), the reference's operation order:
//     o = a * x0 + b * noise  (q_sample, ddpm.py:275-278) ;  x <- o * mask + (1 - mask) * x
// Callers: the pointwise step kernels and the inpainting kernels of gg_sampler.hip (gg_ddim_step, gg_ddpm_step, gg_ddpm_step_x0,
// gg_dpm_solver_step, the codebook-free gg_ddim_step_vq, gg_inpaint_blend), both step modes of vq_kernel in gg_vq.hip (which quantises the prediction of x_0
// between the two halves of a step), and the fused DDIM epilogue of the UNet head conv in gg_conv_box_kernel.h.  They agree bit for bit
// because they run these expressions.
#pragma once
#include "gg_common.h"

__device__ __forceinline__ void ddim_roots(float a_t, float a_prev, float sigma, float &sqrt_at, float &sqrt_ap, float &dirc)
{
#pragma clang fp contract(off)
    sqrt_at = sqrtf(a_t);
    sqrt_ap = sqrtf(a_prev);
    dirc = sqrtf(1.0f - a_prev - sigma * sigma);
}

__device__ __forceinline__ float ddim_pred_x0(float xv, float e, float s1m, float sqrt_at)
{
#pragma clang fp contract(off)
    return (xv - s1m * e) / sqrt_at;
}

// px0: the prediction of x_0, or its quantised value
__device__ __forceinline__ float ddim_x_prev(float px0, float e, float sqrt_ap, float dirc)
{
#pragma clang fp contract(off)
    return sqrt_ap * px0 + dirc * e;
}

__device__ __forceinline__ float ddpm_x_recon(float xv, float ov, float a, float b, int flags)
{
#pragma clang fp contract(off)
    float xr = a * xv - b * ov;
    if (flags & GG_DDPM_PREDICTS_X0) xr = ov;
    if (flags & GG_DDPM_CLIP) xr = fminf(fmaxf(xr, -1.0f), 1.0f);
    return xr;
}

// xr: x_recon, or its quantised value
__device__ __forceinline__ float ddpm_mean(float xr, float xv, float c1, float c2)
{
#pragma clang fp contract(off)
    return c1 * xr + c2 * xv;
}

// the noise term of either update
__device__ __forceinline__ float step_add_noise(float xn, float coef, float nz)
{
#pragma clang fp contract(off)
    return xn + coef * nz;
}

// DPM-Solver++ (2M) prediction of x_0 at the current point s: DDIM's expression on {sigma_s, alpha_s}, the model's output itself under
// GG_DDPM_PREDICTS_X0, clamped to [-1, 1] under GG_DDPM_CLIP
__device__ __forceinline__ float dpm_pred_x0(float xv, float ov, float sigma_s, float alpha_s, int flags)
{
#pragma clang fp contract(off)
    float p = ddim_pred_x0(xv, ov, sigma_s, alpha_s);
    if (flags & GG_DDPM_PREDICTS_X0) p = ov;
    if (flags & GG_DDPM_CLIP) p = fminf(fmaxf(p, -1.0f), 1.0f);
    return p;
}

// the second-order combination of this step's prediction with the previous one; a first-order step (c1 == 0) does not call it
__device__ __forceinline__ float dpm_combine(float p, float hist, float c0, float c1)
{
#pragma clang fp contract(off)
    return c0 * p + c1 * hist;
}

// D: the prediction of x_0, or its combination
__device__ __forceinline__ float dpm_x_next(float xv, float D, float k_x, float k_d)
{
#pragma clang fp contract(off)
    return k_x * xv + k_d * D;
}

__device__ __forceinline__ float inpaint_blend_one(float xv, float x0v, float nv, float mv, float a, float b)
{
#pragma clang fp contract(off)
    const float t1 = a * x0v;
    const float t2 = b * nv;
    const float o = t1 + t2;
    const float p = o * mv;
    const float q = (1.0f - mv) * xv;
    return p + q;
}
