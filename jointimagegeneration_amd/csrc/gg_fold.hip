// Patch-wise evaluation (LatentDiffusion.split_input_params, ddpm.py:573-660): cut a channels-last tensor into overlapping crops
// (gg_unfold_cl) and re-assemble crop results by a weighted overlap-add (gg_fold_weighted_cl).
//
// Geometry (torch.nn.Unfold / Fold with dilation 1, padding 0): Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1, crop l = ly * Lx + lx
// starts at (ly * sy, lx * sx); crop l of sample n is row l * N + n of the crop batch (the reference stacks the crops of a batch on a
// trailing axis and evaluates them one l at a time: a batch of L * N with l outermost is that loop as one call).
//
// gg_unfold_cl is a pure copy (optionally fp32 -> bf16 with the cast the step kernels use for their unet_in rows).  One thread moves one
// channel quad of one destination pixel: 16-byte loads / 16- or 8-byte stores where the quad is whole and the addresses are aligned,
// element-wise otherwise.  Lanes outside [c_offset, c_offset + C) of a destination row are not written.
//
// gg_fold_weighted_cl is the gather form of fold(o * w) / fold(w): one thread owns a channel quad (16 bytes) of one output pixel and
// walks the crops that cover it -- no atomics, so the result does not depend on the schedule.  Evaluation order (all fp32, no
// contraction: every product and every sum is rounded on its own):
//   w   = Wt[ky, kx]                       or  Wt[ky, kx] * Tt[l], rounded first (get_weighting forms that product as a tensor)
//   num = 0;  den = 0
//   for ly descending, lx descending over the covering crops:   num = num + o[l] * w;   den = den + w
//   out = num / den                        IEEE division
// Descending l is the order in which ATen's CPU col2im adds (ascending kernel offset = descending crop index at a fixed pixel), so with
// the same fp32 crops the result equals the reference's fold(o * weighting) / normalization bit for bit.
#include "gg_common.h"

namespace {

struct FoldGeom {
    int N, H, W, kh, kw, sy, sx, Ly, Lx;
};

template <class S, class D>
__global__ __launch_bounds__(256) void unfold_kernel(const S *__restrict__ src, int src_stride, D *__restrict__ dst, int dst_stride,
                                                     int c_offset, int C, FoldGeom g, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned Q = (unsigned)(C + 3) >> 2;
    const unsigned q = i % Q;
    unsigned p = i / Q;
    const unsigned kx = p % (unsigned)g.kw;
    p /= (unsigned)g.kw;
    const unsigned ky = p % (unsigned)g.kh;
    p /= (unsigned)g.kh;                               // row of the crop batch = l * N + n
    const unsigned n = p % (unsigned)g.N, l = p / (unsigned)g.N;
    const unsigned ly = l / (unsigned)g.Lx, lx = l % (unsigned)g.Lx;
    const long long spix = ((long long)n * g.H + (ly * g.sy + ky)) * g.W + (lx * g.sx + kx);
    const long long dpix = ((long long)p * g.kh + ky) * g.kw + kx;
    const S *s = src + spix * src_stride + 4 * q;
    D *d = dst + dpix * dst_stride + c_offset + 4 * q;
    const int nc = min(4, C - 4 * (int)q);
    if (nc == 4 && ((uintptr_t)s & (4 * sizeof(S) - 1)) == 0 && ((uintptr_t)d & (4 * sizeof(D) - 1)) == 0) {
        typedef __attribute__((ext_vector_type(4))) S SV;
        typedef __attribute__((ext_vector_type(4))) D DV;
        const SV v = *(const SV *)s;
        DV o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = (D)v[c];
        *(DV *)d = o;
        return;
    }
    for (int c = 0; c < nc; ++c) d[c] = (D)s[c];
}

__global__ __launch_bounds__(256) void fold_kernel(const float *__restrict__ crops, int crop_stride, const float *__restrict__ Wt,
                                                   const float *__restrict__ Tt, float *__restrict__ out, int out_stride, int C, FoldGeom g,
                                                   unsigned total)
{
    // contract(off) covers the expressions written in this body: products and sums below are separate statements on purpose, and the
    // header's __fmul_rn / __fadd_rn are NOT used (inlined from outside this region they carry the file's contraction setting and the
    // backend fuses them into v_fma: 1-ulp differences against the reference order were measured with them)
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned Q = (unsigned)(C + 3) >> 2;
    const unsigned q = i % Q;
    unsigned p = i / Q;                                // output pixel (n, y, x)
    const int x = (int)(p % (unsigned)g.W);
    const unsigned t = p / (unsigned)g.W;
    const int y = (int)(t % (unsigned)g.H);
    const int n = (int)(t / (unsigned)g.H);
    // crops covering y: ly * sy <= y < ly * sy + kh
    const int ly_hi = min(y / g.sy, g.Ly - 1), ly_lo = y < g.kh ? 0 : (y - g.kh + g.sy) / g.sy;
    const int lx_hi = min(x / g.sx, g.Lx - 1), lx_lo = x < g.kw ? 0 : (x - g.kw + g.sx) / g.sx;
    const int nc = min(4, C - 4 * (int)q);
    float num[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float den = 0.0f;
    for (int ly = ly_hi; ly >= ly_lo; --ly) {
        const int ky = y - ly * g.sy;
        for (int lx = lx_hi; lx >= lx_lo; --lx) {
            const int kx = x - lx * g.sx;
            const int l = ly * g.Lx + lx;
            float w = Wt[ky * g.kw + kx];
            if (Tt) w = w * Tt[l];
            const float *o = crops + ((((long long)l * g.N + n) * g.kh + ky) * g.kw + kx) * crop_stride + 4 * q;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (nc == 4 && ((uintptr_t)o & 15) == 0) {
                const f32x4 vv = *(const f32x4 *)o;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = vv[c];
            } else {
                for (int c = 0; c < nc; ++c) v[c] = o[c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float prod = v[c] * w;
                num[c] = num[c] + prod;
            }
            den = den + w;
        }
    }
    float *d = out + (long long)p * out_stride + 4 * q;
    if (nc == 4 && ((uintptr_t)d & 15) == 0) {
        f32x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = num[c] / den;
        *(f32x4 *)d = r;
        return;
    }
    for (int c = 0; c < nc; ++c) d[c] = num[c] / den;
}

int fold_geom(const char *what, int N, int H, int W, int kh, int kw, int sy, int sx, int C, FoldGeom *g)
{
    if (N < 1 || H < 1 || W < 1 || C < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: N=%d H=%d W=%d C=%d", what, N, H, W, C);
    if (kh < 1 || kw < 1 || sy < 1 || sx < 1 || kh > H || kw > W)
        GG_FAIL(GG_ERR_BAD_SHAPE, "%s: crop %dx%d stride %dx%d on %dx%d", what, kh, kw, sy, sx, H, W);
    *g = FoldGeom{N, H, W, kh, kw, sy, sx, (H - kh) / sy + 1, (W - kw) / sx + 1};
    return GG_OK;
}

}  // namespace

extern "C" int gg_unfold_cl(const void *src, int32_t src_dtype, int32_t N, int32_t H, int32_t W, int32_t src_stride, int32_t C, void *dst,
                            int32_t dst_dtype, int32_t dst_stride, int32_t dst_c_offset, int32_t kh, int32_t kw, int32_t sy, int32_t sx,
                            void *stream_)
{
    if (!src || !dst) GG_FAIL(GG_ERR_BAD_SHAPE, "unfold_cl: null pointer");
    FoldGeom g;
    const int rc = fold_geom("unfold_cl", N, H, W, kh, kw, sy, sx, C, &g);
    if (rc != GG_OK) return rc;
    if (src_stride < C || dst_c_offset < 0 || dst_stride < dst_c_offset + C)
        GG_FAIL(GG_ERR_BAD_SHAPE, "unfold_cl: C=%d does not fit the rows (src stride %d, dst stride %d at offset %d)", C, src_stride, dst_stride,
                dst_c_offset);
    const bool sf = src_dtype == GG_F32, df = dst_dtype == GG_F32;
    if ((!sf && src_dtype != GG_BF16) || (!df && dst_dtype != GG_BF16) || (!sf && df))
        GG_FAIL(GG_ERR_UNSUPPORTED, "unfold_cl: dtypes %d -> %d (fp32 -> fp32 | bf16, bf16 -> bf16)", src_dtype, dst_dtype);
    const long long total = (long long)g.Ly * g.Lx * N * kh * kw * ((C + 3) / 4);
    if (total > 0x7fffffffLL || (long long)N * H * W > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "unfold_cl: %lld work items exceed the grid", total);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipStream_t stream = (hipStream_t)stream_;
    if (sf && df)
        hipLaunchKernelGGL((unfold_kernel<float, float>), grid, block, 0, stream, (const float *)src, src_stride, (float *)dst, dst_stride,
                           dst_c_offset, C, g, (unsigned)total);
    else if (sf)
        hipLaunchKernelGGL((unfold_kernel<float, bf16_t>), grid, block, 0, stream, (const float *)src, src_stride, (bf16_t *)dst, dst_stride,
                           dst_c_offset, C, g, (unsigned)total);
    else
        hipLaunchKernelGGL((unfold_kernel<bf16_t, bf16_t>), grid, block, 0, stream, (const bf16_t *)src, src_stride, (bf16_t *)dst, dst_stride,
                           dst_c_offset, C, g, (unsigned)total);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_fold_weighted_cl(const float *crops, int32_t crop_stride, const float *weight, const float *tie, float *out,
                                   int32_t out_stride, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t sy,
                                   int32_t sx, void *stream_)
{
    if (!crops || !weight || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "fold_weighted_cl: null pointer");
    FoldGeom g;
    const int rc = fold_geom("fold_weighted_cl", N, H, W, kh, kw, sy, sx, C, &g);
    if (rc != GG_OK) return rc;
    if (crop_stride < C || out_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "fold_weighted_cl: stride < C=%d", C);
    // every output pixel needs a covering crop: else its weight sum is 0 and the result 0 / 0
    if ((H - kh) % sy != 0 || (W - kw) % sx != 0 || (g.Ly > 1 && sy > kh) || (g.Lx > 1 && sx > kw))
        GG_FAIL(GG_ERR_BAD_SHAPE, "fold_weighted_cl: crops %dx%d at stride %dx%d leave pixels of %dx%d uncovered", kh, kw, sy, sx, H, W);
    const long long total = (long long)N * H * W * ((C + 3) / 4);
    if (total > 0x7fffffffLL || (long long)g.Ly * g.Lx * N * kh * kw > 0x7fffffffLL)
        GG_FAIL(GG_ERR_UNSUPPORTED, "fold_weighted_cl: %lld work items exceed the grid", total);
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, crops, crop_stride, weight, tie,
                       out, out_stride, C, g, (unsigned)total);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
