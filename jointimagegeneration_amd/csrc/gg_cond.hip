// Conditioning stages (include/guidegen_hip.h "cond stages"): what ClassEmbedder, TransformerEmbedder / BERTEmbedder and SpatialRescaler
// (ldm/modules/encoders/modules.py:22-136) need beyond the conv, attention and LayerNorm kernels.
//
//   embed_rows_kernel       out[r, d] = tok[ids[r], d] (+ pos[r % T, d]): nn.Embedding, and token + absolute positional embedding
//                           (x_transformer.py:25-36,609-610), as fp32 rows or as the bf16 channels-last token rows the convs read
//   bert_embed_kernel       LayerNorm(word[ids] + type[tt] + pos[t]) of transformers' BertEmbeddings as bf16 token rows, one launch
//   gelu_kernel             erf-form GELU (nn.GELU) between the two Linears of x_transformer.FeedForward (x_transformer.py:194-211)
//   layernorm_rows_kernel   LayerNorm over the C logical lanes of rows `stride` lanes apart (gg_layernorm normalises whole rows: C == stride)
//   interpolate2d_kernel    F.interpolate(x, scale_factor=s, mode=nearest | bilinear | bicubic | area) on NCHW fp32 planes
//
// A cond stage runs once per sample, before the chain: these are plain memory-bound kernels, one work item per output element.
#include "gg_norm.h"

// ------------------------------------------------------------------------------------------------------------ embedding rows
template <class T>
__global__ __launch_bounds__(256) void embed_rows_kernel(const int32_t *__restrict__ ids, long long rows, int T_len, const float *__restrict__ tok,
                                                         int V, int D, const float *__restrict__ pos, T *__restrict__ out, int stride)
{
    const long long total = rows * stride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / stride;
        const int d = (int)(i - r * stride);
        float v = 0.f;
        if (d < D) {
            const int id = ids[r];
            if (id >= 0 && id < V) {                       // an id outside the table: a zero row, nothing is read
                v = tok[(long long)id * D + d];
                if (pos) v += pos[(r % T_len) * D + d];    // fp32 add, then ONE rounding to the output type
            }
        }
        out[i] = (T)v;
    }
}

extern "C" int gg_embed_rows(const int32_t *ids, int64_t rows, int32_t T, const float *tok, int32_t V, int32_t D, const float *pos, int32_t P,
                             void *out, int32_t out_dtype, int32_t out_stride, void *stream_)
{
    if (out_dtype != GG_BF16 && out_dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "embed_rows: out_dtype must be GG_BF16 or GG_F32");
    if (rows <= 0 || T <= 0 || rows % T) GG_FAIL(GG_ERR_BAD_SHAPE, "embed_rows: %lld rows are not whole sequences of %d", (long long)rows, T);
    if (V <= 0 || D <= 0 || out_stride < D) GG_FAIL(GG_ERR_BAD_SHAPE, "embed_rows: bad table [%d, %d] or row stride %d", V, D, out_stride);
    if (pos && T > P) GG_FAIL(GG_ERR_BAD_SHAPE, "embed_rows: sequence length %d exceeds the %d positions of the table", T, P);
    if (!ids || !tok || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "embed_rows: null pointer");
    const long long total = (long long)rows * out_stride;
    const unsigned blocks = gg_blocks256(total, 8192);
    const dim3 g(blocks), b(256);
    if (out_dtype == GG_BF16)
        hipLaunchKernelGGL(embed_rows_kernel<bf16_t>, g, b, 0, (hipStream_t)stream_, ids, (long long)rows, T, tok, V, D, pos, (bf16_t *)out, out_stride);
    else
        hipLaunchKernelGGL(embed_rows_kernel<float>, g, b, 0, (hipStream_t)stream_, ids, (long long)rows, T, tok, V, D, pos, (float *)out, out_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------ BERT embeddings
// out[r, :] = LayerNorm(word[ids[r]] + type[tt[r]] + pos[r % T]) (transformers' BertEmbeddings, in its order of additions): one wave per
// row, four rows per workgroup, the statistics of layernorm_rows_kernel (mean, then the centred sum of squares, biased variance) on the
// fp32 sums, ONE rounding to bf16.  The three table rows are re-read per pass (they are in L2; the kernel runs once per text).
// An id outside its table: a zero row, nothing is read.
__global__ __launch_bounds__(256) void bert_embed_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ tts, long long rows, int T_len,
                                                         const float *__restrict__ word, int V, const float *__restrict__ pos,
                                                         const float *__restrict__ type, int NT, int D, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float eps, bf16_t *__restrict__ out, int stride)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                               // whole waves leave: the shuffles below see full waves
    bf16_t *orow = out + row * stride;
    const int id = ids[row], tt = tts ? tts[row] : 0;
    if (id < 0 || id >= V || tt < 0 || tt >= NT) {         // wave-uniform
        for (int c = lane; c < stride; c += 64) orow[c] = (bf16_t)0.f;
        return;
    }
    const float *w = word + (long long)id * D, *ty = type + (long long)tt * D, *po = pos + (row % T_len) * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += (w[c] + ty[c]) + po[c];
    const float mean = gg_wave_sum_f32(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = ((w[c] + ty[c]) + po[c]) - mean; q += d * d; }
    const float rstd = rsqrtf(gg_wave_sum_f32(q) / (float)D + eps);
    for (int c = lane; c < stride; c += 64)
        orow[c] = c < D ? (bf16_t)ln_normalise((w[c] + ty[c]) + po[c], mean, rstd, gamma[c], beta[c]) : (bf16_t)0.f;
}

extern "C" int gg_bert_embed(const int32_t *ids, const int32_t *type_ids, int64_t rows, int32_t T, const float *word, int32_t V,
                             const float *pos, int32_t P, const float *type, int32_t NT, int32_t D, const float *gamma, const float *beta,
                             float eps, void *out, int32_t out_stride, const int32_t *ids_host, const int32_t *type_ids_host, void *stream_)
{
    if (rows <= 0 || T <= 0 || rows % T) GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: %lld rows are not whole sequences of %d", (long long)rows, T);
    if (V <= 0 || NT <= 0 || D <= 0 || out_stride < D) GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: bad tables [%d | %d, %d] or row stride %d", V, NT, D, out_stride);
    if (T > P) GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: sequence length %d exceeds the %d positions of the table", T, P);
    if (!ids || !word || !pos || !type || !gamma || !beta || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: null pointer");
    // the caller's HOST copies of the ids (they come from a host tokenizer): checked here, the device copies are never read back
    for (int64_t r = 0; ids_host && r < rows; ++r)
        if (ids_host[r] < 0 || ids_host[r] >= V) GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: token id %d at row %lld is outside the table's [0, %d)", ids_host[r], (long long)r, V);
    for (int64_t r = 0; type_ids_host && r < rows; ++r)
        if (type_ids_host[r] < 0 || type_ids_host[r] >= NT)
            GG_FAIL(GG_ERR_BAD_SHAPE, "bert_embed: token type %d at row %lld is outside the table's [0, %d)", type_ids_host[r], (long long)r, NT);
    hipLaunchKernelGGL(bert_embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, ids, type_ids, (long long)rows, T,
                       word, V, pos, type, NT, D, gamma, beta, eps, (bf16_t *)out, out_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------ GELU
// 0.5 x (1 + erf(x / sqrt 2)) written as 0.5 x erfc(-x / sqrt 2): the same function, but the left tail keeps its relative accuracy
// (1 + erf(z) cancels to 0 below z = -3.9 in fp32, where the true value is still a normal bf16 number).
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * erfcf(-x * 0.70710678118654752f); }

__global__ __launch_bounds__(256) void gelu_kernel(const bf16_t *__restrict__ x, long long n, bf16_t *__restrict__ out)
{
    const long long groups = (n + 7) / 8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long long)gridDim.x * 256) {
        const long long e0 = i * 8;
        if (e0 + 8 <= n) {
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(x + e0);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (bf16_t)gelu_erf((float)v[j]);
            *reinterpret_cast<bf16x8 *>(out + e0) = o;
        } else {
            for (long long e = e0; e < n; ++e) out[e] = (bf16_t)gelu_erf((float)x[e]);
        }
    }
}

extern "C" int gg_gelu(const void *x, int64_t n, void *out, void *stream_)
{
    if (n <= 0) GG_FAIL(GG_ERR_BAD_SHAPE, "gelu: n = %lld", (long long)n);
    if (!x || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "gelu: null pointer");
    if (((uintptr_t)x | (uintptr_t)out) & 15) GG_FAIL(GG_ERR_BAD_SHAPE, "gelu: x and out must be 16-byte aligned");
    const unsigned blocks = gg_blocks256((n + 7) / 8, 8192);
    hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, (const bf16_t *)x, (long long)n, (bf16_t *)out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------ LayerNorm of padded rows
// One wave per row, four rows per workgroup; the arithmetic of layernorm_kernel (gg_norm.hip): mean, then the centred sum of squares, fp32.
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const bf16_t *__restrict__ x, long long rows, int C, int stride,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                             bf16_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                               // whole waves leave: the shuffles below see full waves
    const bf16_t *xr = x + row * stride;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += (float)xr[c];
    const float mean = gg_wave_sum_f32(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = (float)xr[c] - mean; q += d * d; }
    const float rstd = rsqrtf(gg_wave_sum_f32(q) / (float)C + eps);
    bf16_t *orow = out + row * stride;
    for (int c = lane; c < stride; c += 64)
        orow[c] = c < C ? (bf16_t)ln_normalise((float)xr[c], mean, rstd, gamma[c], beta[c]) : (bf16_t)0.f;
}

extern "C" int gg_layernorm_rows(const void *x, int64_t rows, int32_t C, int32_t stride, const float *gamma, const float *beta, float eps,
                                 void *out, void *stream_)
{
    if (C <= 0 || stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "layernorm_rows: C = %d, stride = %d", C, stride);
    if (rows <= 0) GG_FAIL(GG_ERR_BAD_SHAPE, "layernorm_rows: rows = %lld", (long long)rows);
    if (!x || !gamma || !beta || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "layernorm_rows: null pointer");
    if (x == out) GG_FAIL(GG_ERR_BAD_SHAPE, "layernorm_rows: in place is not supported");
    hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, (const bf16_t *)x,
                       (long long)rows, C, stride, gamma, beta, eps, (bf16_t *)out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------ interpolate
// torch.nn.functional.interpolate(x, scale_factor=s, mode=...) with align_corners=False and no recompute_scale_factor, as ATen's CPU
// kernels compute it in fp32 (aten/src/ATen/native/UpSample.h, cpu/UpSampleKernel.cpp, AdaptiveAvgPoolKernel.cpp).  `scale` is
// float(1.0 / s), the value ATen uses when a scale factor is given -- not in / out.  Every source index is clamped to [0, in - 1].
enum { GG_INTERP_NEAREST = 0, GG_INTERP_BILINEAR = 1, GG_INTERP_BICUBIC = 2, GG_INTERP_AREA = 3 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bilinear: src = scale (dst + 0.5) - 0.5 clamped below at 0; i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1)
__device__ __forceinline__ void linear_taps(float scale, int dst, int in, int &i0, int &i1, float &l0, float &l1)
{
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = clampi((int)src, 0, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}

// cubic convolution coefficients, A = -0.75 (UpSample.h: cubic_convolution1 / 2, get_cubic_upsample_coefficients)
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
__device__ __forceinline__ void cubic_taps(float scale, int dst, int in, int idx[4], float w[4])
{
    const float src = scale * ((float)dst + 0.5f) - 0.5f;                  // not clamped
    int i = (int)floorf(src);
    if (i > in - 1) i = in - 1;
    const float t = fminf(fmaxf(src - (float)i, 0.f), 1.f);
    const float A = -0.75f;
    w[0] = cubic2(t + 1.f, A);
    w[1] = cubic1(t, A);
    w[2] = cubic1(1.f - t, A);
    w[3] = cubic2((1.f - t) + 1.f, A);
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = clampi(i - 1 + j, 0, in - 1);
}

template <int MODE>
__global__ __launch_bounds__(256) void interpolate2d_kernel(const float *__restrict__ src, int H, int W, int Ho, int Wo, float sh, float sw,
                                                            long long total, float *__restrict__ dst)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r = i;
        const int ow = (int)(r % Wo); r /= Wo;
        const int oh = (int)(r % Ho);
        const long long plane = r / Ho;
        const float *p = src + plane * (long long)H * W;
        float o;
        if (MODE == GG_INTERP_NEAREST) {
            const int ih = clampi((int)floorf((float)oh * sh), 0, H - 1), iw = clampi((int)floorf((float)ow * sw), 0, W - 1);
            o = p[(long long)ih * W + iw];
        } else if (MODE == GG_INTERP_BILINEAR) {
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            linear_taps(sh, oh, H, y0, y1, ly0, ly1);
            linear_taps(sw, ow, W, x0, x1, lx0, lx1);
            const float *r0 = p + (long long)y0 * W, *r1 = p + (long long)y1 * W;
            float a = r0[x0] * lx0; a += r0[x1] * lx1;
            float b = r1[x0] * lx0; b += r1[x1] * lx1;
            o = a * ly0; o += b * ly1;
        } else if (MODE == GG_INTERP_BICUBIC) {
            int iy[4], ix[4];
            float wy[4], wx[4];
            cubic_taps(sh, oh, H, iy, wy);
            cubic_taps(sw, ow, W, ix, wx);
            o = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float *rr = p + (long long)iy[j] * W;
                float a = rr[ix[0]] * wx[0];
#pragma unroll
                for (int k = 1; k < 4; ++k) a += rr[ix[k]] * wx[k];
                o = j == 0 ? a * wy[0] : o + a * wy[j];
            }
        } else {                                                            // adaptive average pool: [floor(i in / out), ceil((i + 1) in / out))
            const int h0 = (int)(((long long)oh * H) / Ho), w0 = (int)(((long long)ow * W) / Wo);
            int h1 = (int)((((long long)oh + 1) * H + Ho - 1) / Ho), w1 = (int)((((long long)ow + 1) * W + Wo - 1) / Wo);
            if (h1 > H) h1 = H;
            if (w1 > W) w1 = W;
            float s = 0.f;
            for (int ih = h0; ih < h1; ++ih)
                for (int iw = w0; iw < w1; ++iw) s += p[(long long)ih * W + iw];
            o = s / (float)(h1 - h0) / (float)(w1 - w0);                 // ATen: sum / kh / kw, two IEEE divisions
        }
        dst[i] = o;
    }
}

extern "C" int gg_interpolate2d_f32(const float *src, int64_t planes, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float scale_h, float scale_w,
                                    int32_t mode, float *dst, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (planes <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        GG_FAIL(GG_ERR_BAD_SHAPE, "interpolate2d: empty extent (%lld planes, %d x %d -> %d x %d)", (long long)planes, H, W, Ho, Wo);
    if (mode < GG_INTERP_NEAREST || mode > GG_INTERP_AREA) GG_FAIL(GG_ERR_BAD_SHAPE, "interpolate2d: mode %d outside 0..3 (nearest, bilinear, bicubic, area)", mode);
    if (mode != GG_INTERP_AREA && !(scale_h > 0.f && scale_w > 0.f && scale_h < 3.0e38f && scale_w < 3.0e38f))
        GG_FAIL(GG_ERR_BAD_SHAPE, "interpolate2d: coordinate scales must be positive and finite");
    if ((long long)H * W >= (1LL << 31) || (long long)Ho * Wo >= (1LL << 31)) GG_FAIL(GG_ERR_BAD_SHAPE, "interpolate2d: a plane of 2^31 elements or more");
    if (!src || !dst) GG_FAIL(GG_ERR_BAD_SHAPE, "interpolate2d: null pointer");
    const long long total = (long long)planes * Ho * Wo;
    const unsigned blocks = gg_blocks256(total, 16384);
    const dim3 g(blocks), b(256);
    switch (mode) {
    case GG_INTERP_NEAREST: hipLaunchKernelGGL(interpolate2d_kernel<GG_INTERP_NEAREST>, g, b, 0, stream, src, H, W, Ho, Wo, scale_h, scale_w, total, dst); break;
    case GG_INTERP_BILINEAR: hipLaunchKernelGGL(interpolate2d_kernel<GG_INTERP_BILINEAR>, g, b, 0, stream, src, H, W, Ho, Wo, scale_h, scale_w, total, dst); break;
    case GG_INTERP_BICUBIC: hipLaunchKernelGGL(interpolate2d_kernel<GG_INTERP_BICUBIC>, g, b, 0, stream, src, H, W, Ho, Wo, scale_h, scale_w, total, dst); break;
    default: hipLaunchKernelGGL(interpolate2d_kernel<GG_INTERP_AREA>, g, b, 0, stream, src, H, W, Ho, Wo, scale_h, scale_w, total, dst); break;
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}
