// Three-view LPIPS of CT volumes (ldm/modules/losses/lpips.py, latentdiffusion/sample_diffusion.py:437-475): the three kernels around the
// VGG16 convolutions, which run on the project's channels-last 3x3 kernels as they are.
//
//   gg_volume_views_cl  fp32 volume [B, D, H, W] -> channels-last rows [n, 1, h, w, 32] of one axis view, channels 0..2 =
//                       (x - shift_c) / scale_c (ScalingLayer on a 1-channel slice: one value, three differently scaled channels)
//   gg_relu_cl          in-place ReLU on channels-last rows (the 8 convolutions that no tap follows)
//   gg_lpips_tap        pre-ReLU conv outputs of both images at a tap -> per-image LPIPS term + the 2x2 max-pooled ReLU'd rows
//
// Mapping of gg_volume_views_cl.  A thread writes one 16-byte piece of a 32-channel row (bf16: 4 pieces, fp32: 8); a wave writes 1 KiB
// of consecutive output.  Only piece 0 carries values, so one lane in 4 (8) reads x.  Views 0 (images along D) and 1 (along H) keep W
// as the image's inner axis: consecutive pixels read consecutive floats (direct kernel, one workgroup row per image line).  View 2
// (images along W, pixel (d, h)) has the image's inner axis at stride W in x, and W consecutive IMAGES on one cache line: a direct
// mapping would fetch a 128-byte line per 4 bytes used.  There a workgroup stages a tile of 32 images x 32 pixels through LDS
// ([32][33] floats): the read runs along w (128 B per 32 lanes), the write along h (32 pixels = 2 KiB of one image, consecutive).
// The LDS read of lane (pixel j, piece p) is tile[j][image]: 16 (8) distinct j per wave at row pitch 33 -> distinct banks.
//
// Mapping of gg_lpips_tap.  The unit of work is a 2x2 quad of pixels of one image (what one pooled pixel needs); L = min(64, C / vec)
// lanes own a quad, lane s the 16-byte channel pieces s, s + L, ...  (vec = 8 bf16 or 4 fp32 per piece; ITERS pieces per lane, held in
// registers so that each tap tensor is read once).  Per pixel: ReLU, sum of squares of both rows reduced over the L lanes with an xor
// butterfly (every lane ends with the same bits), then sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 reduced the same way.
// Lane 0 of the group adds the pixel's term to its running fp32 sum.  grid = (nb, n): a workgroup strides over the quads of ONE
// image; its 256 / L group sums are reduced through LDS in a fixed tree -> partial[n][block].  The second kernel adds the nb partials
// of an image in index order and divides by h * w.  No floating-point atomics; nb depends on (h, w, C, dtype) alone, so the bits of an
// image's value do not depend on the batch it is in.
#include "gg_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_BLOCKS = 128;          // partials per image
constexpr int LP_TILE = 32;

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };

// image n (global index within the view) = (b, m) with m < per_b; pixel (i, j), channel c reads x[b * sB + m * sN + i * sI + j * sJ + c * sC]
struct ViewGeom {
    long long sB, sN, sI, sJ, sC;
    int per_b, hh, ww;
};

template <typename T>
__device__ __forceinline__ typename Vec16<T>::type scaled_piece(const float *p, long long sC, const float *shift, const float *scale)
{
    typename Vec16<T>::type v;
#pragma unroll
    for (int c = 0; c < Vec16<T>::N; ++c) v[c] = (T)0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (T)((p[c * sC] - shift[c]) / scale[c]);       // fp32 subtract, IEEE fp32 divide, one rounding to T
    return v;
}

// views whose inner image axis is contiguous in x (sJ == 1).  grid = (image lines of the chunk, column blocks)
template <typename T>
__global__ __launch_bounds__(LP_THREADS) void views_direct_kernel(const float *__restrict__ x, ViewGeom g, long long n0, const float *__restrict__ shift,
                                                                  const float *__restrict__ scale, T *__restrict__ out)
{
    constexpr int V = Vec16<T>::N, P = 32 / V;
    typedef typename Vec16<T>::type VT;
    const int t = (int)blockIdx.y * LP_THREADS + (int)threadIdx.x;
    if (t >= g.ww * P) return;
    const long long line = blockIdx.x;                   // (image within the chunk) * hh + i
    const int i = (int)(line % g.hh);
    const long long n = n0 + line / g.hh;
    const int j = t / P, piece = t % P;
    VT v;
#pragma unroll
    for (int c = 0; c < V; ++c) v[c] = (T)0.0f;
    if (piece == 0) v = scaled_piece<T>(x + (n / g.per_b) * g.sB + (n % g.per_b) * g.sN + i * g.sI + j * g.sJ, g.sC, shift, scale);
    *(VT *)(out + ((line * g.ww + j) * 32 + piece * V)) = v;
}

// views whose IMAGE axis is contiguous in x (sN == 1): 32 images x 32 pixels of one image line through LDS.
// grid = (hh * column tiles, image tiles)
template <typename T>
__global__ __launch_bounds__(LP_THREADS) void views_transposed_kernel(const float *__restrict__ x, ViewGeom g, long long n0, long long n1,
                                                                      const float *__restrict__ shift, const float *__restrict__ scale, T *__restrict__ out)
{
    constexpr int V = Vec16<T>::N, P = 32 / V;
    typedef typename Vec16<T>::type VT;
    __shared__ float tile[LP_TILE][LP_TILE + 1];
    const int jt = (g.ww + LP_TILE - 1) / LP_TILE;
    const int i = (int)blockIdx.x / jt;
    const int j0 = ((int)blockIdx.x % jt) * LP_TILE;
    const long long nt0 = n0 + (long long)blockIdx.y * LP_TILE;
    const int tx = threadIdx.x % LP_TILE, ty = threadIdx.x / LP_TILE;
    {
        const long long n = nt0 + tx;
#pragma unroll
        for (int r = 0; r < LP_TILE / (LP_THREADS / LP_TILE); ++r) {
            const int jl = ty + r * (LP_THREADS / LP_TILE);
            if (n < n1 && j0 + jl < g.ww) tile[jl][tx] = x[(n / g.per_b) * g.sB + (n % g.per_b) * g.sN + i * g.sI + (j0 + jl) * g.sJ];
        }
    }
    __syncthreads();
    const float s0 = shift[0], s1 = shift[1], s2 = shift[2], c0 = scale[0], c1 = scale[1], c2 = scale[2];
    for (int it = threadIdx.x; it < LP_TILE * LP_TILE * P; it += LP_THREADS) {
        const int piece = it % P, jl = (it / P) % LP_TILE, nl = it / (P * LP_TILE);
        if (nt0 + nl >= n1 || j0 + jl >= g.ww) continue;
        VT v;
#pragma unroll
        for (int c = 0; c < V; ++c) v[c] = (T)0.0f;
        if (piece == 0) {
            const float xv = tile[jl][nl];
            v[0] = (T)((xv - s0) / c0);
            v[1] = (T)((xv - s1) / c1);
            v[2] = (T)((xv - s2) / c2);
        }
        const long long pix = ((nt0 + nl - n0) * g.hh + i) * g.ww + (j0 + jl);
        *(VT *)(out + (pix * 32 + piece * V)) = v;
    }
}

template <typename T>
__global__ __launch_bounds__(LP_THREADS) void relu_kernel(T *x, long long nvec)
{
    constexpr int V = Vec16<T>::N;
    typedef typename Vec16<T>::type VT;
    const long long idx = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (idx >= nvec) return;
    VT v = ((VT *)x)[idx];
#pragma unroll
    for (int c = 0; c < V; ++c)
        if ((float)v[c] < 0.0f) v[c] = (T)0.0f;          // a NaN stays a NaN, as in torch
    ((VT *)x)[idx] = v;
}

template <typename T, int ITERS>
__global__ __launch_bounds__(LP_THREADS) void lpips_tap_kernel(const T *__restrict__ a, const T *__restrict__ b, const float *__restrict__ wlin, int h, int w,
                                                               int C, int L, int lshift, T *__restrict__ pa, T *__restrict__ pb,
                                                               float *__restrict__ partial)
{
    constexpr int V = Vec16<T>::N;
    typedef typename Vec16<T>::type VT;
    __shared__ float red[LP_THREADS];
    const int tid = threadIdx.x;
    const int sub = tid & (L - 1), grp = tid >> lshift, G = LP_THREADS >> lshift;
    const int n = blockIdx.y;
    const int qw = (w + 1) >> 1, Q = ((h + 1) >> 1) * qw, ho = h >> 1, wo = w >> 1;
    const long long img = (long long)n * h * w;
    float wv[ITERS][V];
    bool cok[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * L + sub) * V;
        cok[it] = c < C;
#pragma unroll
        for (int e = 0; e < V; ++e) wv[it][e] = cok[it] ? wlin[c + e] : 0.0f;
    }
    float acc = 0.0f;
    for (int q0 = (int)blockIdx.x * G; q0 < Q; q0 += (int)gridDim.x * G) {          // the same trip count for every thread of the workgroup
        const int q = q0 + grp;
        const bool qv = q < Q;
        const int qy = q / qw, qx = q - qy * qw;
        float ma[ITERS][V], mb[ITERS][V];
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
#pragma unroll
            for (int e = 0; e < V; ++e) ma[it][e] = mb[it][e] = 0.0f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * qy + (p >> 1), xx = 2 * qx + (p & 1);
            const bool pv = qv && y < h && xx < w;       // a pixel outside the image (odd extents, a group past the last quad) is read nowhere
            const long long row = (img + (long long)y * w + xx) * C;
            float va[ITERS][V], vb[ITERS][V];
            float sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int c = (it * L + sub) * V;
                VT ra, rb;
#pragma unroll
                for (int e = 0; e < V; ++e) ra[e] = rb[e] = (T)0.0f;
                if (pv && cok[it]) {
                    ra = *(const VT *)(a + row + c);
                    rb = *(const VT *)(b + row + c);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float fa = (float)ra[e], fb = (float)rb[e];
                    va[it][e] = fa < 0.0f ? 0.0f : fa;
                    vb[it][e] = fb < 0.0f ? 0.0f : fb;
                    sa += va[it][e] * va[it][e];
                    sb += vb[it][e] * vb[it][e];
                    ma[it][e] = fmaxf(ma[it][e], va[it][e]);
                    mb[it][e] = fmaxf(mb[it][e], vb[it][e]);
                }
            }
            for (int m = L >> 1; m >= 1; m >>= 1) {      // xor butterfly inside the group: every lane ends with the same sum
                sa += __shfl_xor(sa, m, GG_WAVE);
                sb += __shfl_xor(sb, m, GG_WAVE);
            }
            const float ia = 1.0f / (sqrtf(sa) + 1e-10f), ib = 1.0f / (sqrtf(sb) + 1e-10f);      // an all-zero row: 0 * 1e10 = 0
            float d = 0.0f;
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float t = va[it][e] * ia - vb[it][e] * ib;
                    d += wv[it][e] * (t * t);
                }
            for (int m = L >> 1; m >= 1; m >>= 1) d += __shfl_xor(d, m, GG_WAVE);
            if (pv) acc += d;
        }
        if (pa && qv && qy < ho && qx < wo) {            // MaxPool2d(2, 2): floor semantics, the odd last line / column has no output
            const long long prow = (((long long)n * ho + qy) * wo + qx) * C;
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                if (!cok[it]) continue;
                const int c = (it * L + sub) * V;
                VT oa, ob;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    oa[e] = (T)ma[it][e];                // exact: the maximum of values that came from T
                    ob[e] = (T)mb[it][e];
                }
                *(VT *)(pa + prow + c) = oa;
                *(VT *)(pb + prow + c) = ob;
            }
        }
    }
    red[tid] = sub == 0 ? acc : 0.0f;
    __syncthreads();
    for (int s = LP_THREADS / 2; s >= 1; s >>= 1) {      // fixed tree
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[(long long)n * gridDim.x + blockIdx.x] = red[0];
}

__global__ void lpips_tap_finish_kernel(const float *__restrict__ partial, int nb, int n, float hw, float *__restrict__ tap_out, float *total, int accumulate)
{
    const int i = (int)blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int k = 0; k < nb; ++k) s += partial[(long long)i * nb + k];           // index order
    const float v = s / hw;
    if (tap_out) tap_out[i] = v;
    if (total) total[i] = accumulate ? total[i] + v : v;
}

struct TapPlan {
    int L, lshift, iters, nb;
};

// lanes per quad, pieces per lane and workgroups per image: functions of (h, w, C, dtype) alone
bool tap_plan(int h, int w, int C, int dtype, TapPlan *p)
{
    const int vec = dtype == GG_F32 ? 4 : 8;
    int L = 1, ls = 0;
    while (L * 2 <= 64 && L * 2 * vec <= C) {
        L *= 2;
        ++ls;
    }
    const int iters = (C + L * vec - 1) / (L * vec);
    if (iters != 1 && iters != 2 && iters != 4) return false;
    const long long Q = (long long)((h + 1) / 2) * ((w + 1) / 2);
    const int G = LP_THREADS / L;
    const long long nb = (Q + G - 1) / G;
    p->L = L;
    p->lshift = ls;
    p->iters = iters;
    p->nb = (int)(nb < LP_MAX_BLOCKS ? nb : LP_MAX_BLOCKS);
    return true;
}

int tap_check(int n, int h, int w, int C, int dtype, TapPlan *p)
{
    if (dtype != GG_BF16 && dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "lpips_tap: dtype %d", dtype);
    if (n < 1 || n > 65535 || h < 1 || w < 1 || (long long)h * w > (1LL << 30)) GG_FAIL(GG_ERR_BAD_SHAPE, "lpips_tap: n=%d h=%d w=%d", n, h, w);
    if (C < 32 || C % 32) GG_FAIL(GG_ERR_BAD_SHAPE, "lpips_tap: C=%d is not a positive multiple of 32", C);
    if (!tap_plan(h, w, C, dtype, p)) GG_FAIL(GG_ERR_UNSUPPORTED, "lpips_tap: C=%d needs more than 4 pieces per lane", C);
    return GG_OK;
}

template <typename T>
void tap_launch(const TapPlan &p, dim3 grid, hipStream_t s, const void *a, const void *b, const float *wl, int h, int w, int C, void *pa, void *pb, float *part)
{
#define LP_CASE(I)                                                                                                                          \
    case I:                                                                                                                                 \
        hipLaunchKernelGGL((lpips_tap_kernel<T, I>), grid, dim3(LP_THREADS), 0, s, (const T *)a, (const T *)b, wl, h, w, C, p.L, p.lshift, \
                           (T *)pa, (T *)pb, part);                                                                                        \
        break;
    switch (p.iters) {
        LP_CASE(1) LP_CASE(2) LP_CASE(4)
    }
#undef LP_CASE
}

}  // namespace

extern "C" int gg_volume_views_cl(const float *x, int32_t B, int32_t D, int32_t H, int32_t W, int32_t view, int64_t n0, int64_t n1,
                                  const float *shift, const float *scale, void *out, int32_t out_dtype, void *stream_)
{
    if (!x || !shift || !scale || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "volume_views_cl: null pointer");
    if (out_dtype != GG_BF16 && out_dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "volume_views_cl: out_dtype %d", out_dtype);
    if (B < 1 || D < 1 || H < 1 || W < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "volume_views_cl: B=%d D=%d H=%d W=%d", B, D, H, W);
    if (view < 0 || view > 3) GG_FAIL(GG_ERR_BAD_SHAPE, "volume_views_cl: view %d outside 0..3", view);
    if (view == 3 && D != 3) GG_FAIL(GG_ERR_BAD_SHAPE, "volume_views_cl: view 3 reads [B, 3, H, W] images, got %d channels", D);
    const long long HW = (long long)H * W;
    ViewGeom g;
    g.sB = (long long)D * HW;
    g.sC = 0;
    long long images;
    switch (view) {
    case 0: g.per_b = D; g.hh = H; g.ww = W; g.sN = HW; g.sI = W; g.sJ = 1; break;               // (b d) 1 h w
    case 1: g.per_b = H; g.hh = D; g.ww = W; g.sN = W; g.sI = HW; g.sJ = 1; break;               // (b h) 1 d w
    case 2: g.per_b = W; g.hh = D; g.ww = H; g.sN = 1; g.sI = HW; g.sJ = W; break;               // (b w) 1 d h
    default: g.per_b = 1; g.hh = H; g.ww = W; g.sN = 0; g.sI = W; g.sJ = 1; g.sC = HW; break;    // b 3 h w
    }
    images = (long long)B * g.per_b;
    if (n0 < 0 || n1 <= n0 || n1 > images) GG_FAIL(GG_ERR_BAD_SHAPE, "volume_views_cl: images [%lld, %lld) outside the view's %lld", (long long)n0, (long long)n1, images);
    hipStream_t stream = (hipStream_t)stream_;
    const long long cnt = n1 - n0;
    if (view == 2) {
        const long long gx = (long long)g.hh * ((g.ww + LP_TILE - 1) / LP_TILE), gy = (cnt + LP_TILE - 1) / LP_TILE;
        if (gx > 0x7fffffffLL || gy > 65535) GG_FAIL(GG_ERR_UNSUPPORTED, "volume_views_cl: %lld images of %d x %d exceed the grid", cnt, g.hh, g.ww);
        const dim3 grid((unsigned)gx, (unsigned)gy);
        if (out_dtype == GG_F32)
            hipLaunchKernelGGL(views_transposed_kernel<float>, grid, dim3(LP_THREADS), 0, stream, x, g, (long long)n0, (long long)n1, shift, scale, (float *)out);
        else
            hipLaunchKernelGGL(views_transposed_kernel<bf16_t>, grid, dim3(LP_THREADS), 0, stream, x, g, (long long)n0, (long long)n1, shift, scale, (bf16_t *)out);
    } else {
        const int P = out_dtype == GG_F32 ? 8 : 4;
        const long long gx = cnt * g.hh, gy = ((long long)g.ww * P + LP_THREADS - 1) / LP_THREADS;
        if (gx > 0x7fffffffLL || gy > 65535) GG_FAIL(GG_ERR_UNSUPPORTED, "volume_views_cl: %lld images of %d x %d exceed the grid", cnt, g.hh, g.ww);
        const dim3 grid((unsigned)gx, (unsigned)gy);
        if (out_dtype == GG_F32)
            hipLaunchKernelGGL(views_direct_kernel<float>, grid, dim3(LP_THREADS), 0, stream, x, g, (long long)n0, shift, scale, (float *)out);
        else
            hipLaunchKernelGGL(views_direct_kernel<bf16_t>, grid, dim3(LP_THREADS), 0, stream, x, g, (long long)n0, shift, scale, (bf16_t *)out);
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_relu_cl(void *x, int32_t dtype, int64_t n, void *stream_)
{
    if (!x) GG_FAIL(GG_ERR_BAD_SHAPE, "relu_cl: null pointer");
    if (dtype != GG_BF16 && dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "relu_cl: dtype %d", dtype);
    if (n < 32 || n % 32) GG_FAIL(GG_ERR_BAD_SHAPE, "relu_cl: %lld elements are not whole 32-channel rows", (long long)n);
    const long long nvec = n / (dtype == GG_F32 ? 4 : 8);
    const long long blocks = (nvec + LP_THREADS - 1) / LP_THREADS;
    if (blocks > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "relu_cl: %lld elements exceed the grid", (long long)n);
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype == GG_F32)
        hipLaunchKernelGGL(relu_kernel<float>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, (float *)x, nvec);
    else
        hipLaunchKernelGGL(relu_kernel<bf16_t>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, (bf16_t *)x, nvec);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int64_t gg_lpips_tap_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t C, int32_t dtype)
{
    TapPlan p;
    const int rc = tap_check(n, h, w, C, dtype, &p);
    if (rc != GG_OK) return rc;
    return (int64_t)n * p.nb * (int64_t)sizeof(float);
}

extern "C" int gg_lpips_tap(const void *a, const void *b, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t C, const float *lin_w,
                            void *pool_a, void *pool_b, float *tap_out, float *total, int32_t accumulate, float *workspace,
                            int64_t workspace_bytes, void *stream_)
{
    if (!a || !b || !lin_w || !workspace || (!tap_out && !total)) GG_FAIL(GG_ERR_BAD_SHAPE, "lpips_tap: null pointer");
    if ((pool_a == nullptr) != (pool_b == nullptr)) GG_FAIL(GG_ERR_BAD_SHAPE, "lpips_tap: both pooled outputs or neither");
    TapPlan p;
    const int rc = tap_check(n, h, w, C, dtype, &p);
    if (rc != GG_OK) return rc;
    if (workspace_bytes < (int64_t)n * p.nb * (int64_t)sizeof(float))
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "lpips_tap: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)n * p.nb * 4);
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)p.nb, (unsigned)n);
    if (dtype == GG_F32)
        tap_launch<float>(p, grid, stream, a, b, lin_w, h, w, C, pool_a, pool_b, workspace);
    else
        tap_launch<bf16_t>(p, grid, stream, a, b, lin_w, h, w, C, pool_a, pool_b, workspace);
    GG_CHECK_LAUNCH();
    hipLaunchKernelGGL(lpips_tap_finish_kernel, dim3((unsigned)((n + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, stream, workspace, p.nb, n,
                       (float)((long long)h * w), tap_out, total, accumulate);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
