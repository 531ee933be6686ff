// Rendering of sampled volumes (latentdiffusion/sample_diffusion.py:23-58,241-261): gg_mask_overlay blends the organ mask over the CT and
// draws every organ's 3-D Sobel boundary in its colour; gg_make_grid_u8 tiles the slices into one uint8 HWC picture (torchvision's
// make_grid followed by .astype(uint8)).  Both are exact restatements: every fp32 operation of the reference is ONE correctly rounded
// fp32 operation here (contraction is switched off below: hipcc would turn a * b + c * d into an FMA, and a last-bit difference flips a
// byte after truncation), and the boundary rule is integer arithmetic.
//
// gg_mask_overlay.  A workgroup of 256 threads owns a tile of 8 (D) x 8 (H) x 64 (W) voxels; extents need not be multiples of it.
//   1. Class ids with a one-voxel halo go to LDS as bytes, [10][10][68]: id = i when m = x[1] * 11 (255 -> 11) is EXACTLY the integer i
//      in 1..11, else 0; a voxel outside the volume is 0 too (scipy's mode='constant').  This is the `mask == i` test of the reference's
//      eleven passes, done once.  While staging, the workgroup ORs (1 << id) of everything it stores: a halo tile that holds one value
//      has no boundary voxel (every derivative of a constant is 0) and skips step 2.
//   2. A lane owns one w and two h rows and walks the 8 slices of the tile (unrolled: the 27 byte reads of neighbouring slices are the
//      same LDS addresses, so the compiler keeps them in registers).  A voxel whose 27 neighbours are equal is done.  Otherwise the
//      classes PRESENT in the neighbourhood are the only ones whose response can be non-zero; for each, ascending, the three integer
//      responses ([-1, 0, 1] along one axis, [1, 2, 1] along the other two) are evaluated and the first class with a non-zero one wins.
//      (Not "some neighbour differs": opposite-signed differences cancel under the smoothing weights.)
//   3. The blend of the lane's own voxel and the three coalesced stores (out is [N, D, 3, H, W]: W contiguous in every channel plane).
// Traffic per voxel: 8 B read (+ the halo's share of x[1], from L2), 12 B written; no atomics on global memory, no workspace.
//
// gg_make_grid_u8.  One thread per output pixel: grid.x = picture row, grid.y * 256 + thread = column.  The pixel finds its cell by one
// division per axis, reads its 1 or 3 source values (coalesced along W) or the pad value, and stores 3 bytes.
#include "gg_common.h"

// hipcc contracts a * b + c into an FMA by default.  __fmul_rn / __fadd_rn do not help: in this toolchain they are plain operators in a
// header, compiled with the default, and are fused after inlining.  So contraction is off for every operator written in this file, and
// the arithmetic below is written with plain operators.  tests/test_render_gpu.py holds the result to the reference bit for bit.
#pragma clang fp contract(off)

namespace {

constexpr int RT_D = 8, RT_H = 8, RT_W = 64, RT_THREADS = 256;
constexpr int RH_D = RT_D + 2, RH_H = RT_H + 2, RH_W = RT_W + 2, RH_WP = 68;   // halo tile; rows padded to whole dwords
constexpr int RT_ROWS = RT_H / (RT_THREADS / RT_W);                             // h rows per lane: 2
constexpr int R_CLASSES = 12;

struct OverlayColors {
    float c[R_CLASSES * 3];
};

// id of the class a mask value belongs to for the boundary passes: i when m == i for an i in 1..11, else 0
__device__ __forceinline__ int overlay_class(float m)
{
    if (!(m >= 1.0f && m <= 11.0f)) return 0;
    const int c = (int)m;
    return (float)c == m ? c : 0;
}

__device__ __forceinline__ float overlay_mask_value(float raw)
{
    const float m = raw * 11.0f;
    return m == 255.0f ? 11.0f : m;
}

__global__ __launch_bounds__(RT_THREADS) void mask_overlay_kernel(const float *__restrict__ x, int D, int H, int W, int tilesW, float coef,
                                                                  float rest, OverlayColors colors, float *__restrict__ out)
{
    __shared__ unsigned char cls[RH_D][RH_H][RH_WP];
    __shared__ float col[R_CLASSES * 3];
    __shared__ unsigned present;
    const int tid = threadIdx.x;
    const int tw = (int)blockIdx.x % tilesW, th = (int)blockIdx.x / tilesW;
    const int w0 = tw * RT_W, h0 = th * RT_H, d0 = (int)blockIdx.y * RT_D;
    const long long HW = (long long)H * W, vol = HW * D;
    const float *ct = x + (long long)blockIdx.z * 2 * vol;
    const float *mk = ct + vol;
    float *o = out + (long long)blockIdx.z * 3 * vol;

    if (tid < R_CLASSES * 3) col[tid] = colors.c[tid];
    if (tid == 0) present = 0u;
    __syncthreads();

    unsigned mine = 0u;
    for (int idx = tid; idx < RH_D * RH_H * RH_W; idx += RT_THREADS) {
        const int hx = idx % RH_W, r = idx / RH_W;
        const int hy = r % RH_H, hz = r / RH_H;
        const int gz = d0 - 1 + hz, gy = h0 - 1 + hy, gx = w0 - 1 + hx;
        int c = 0;
        if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W)          // outside the volume: "no class", never read
            c = overlay_class(overlay_mask_value(mk[(long long)gz * HW + (long long)gy * W + gx]));
        cls[hz][hy][hx] = (unsigned char)c;
        mine |= 1u << c;
    }
    atomicOr(&present, mine);
    __syncthreads();
    const bool flat = __popc(present) == 1;                                      // workgroup-uniform

    const int lane = tid & (RT_W - 1), wave = tid / RT_W;
    const int gx = w0 + lane;
    if (gx >= W) return;                                                         // no barrier below
    for (int r = 0; r < RT_ROWS; ++r) {
        const int ly = wave * RT_ROWS + r, gy = h0 + ly;
        if (gy >= H) break;
#pragma unroll
        for (int lz = 0; lz < RT_D; ++lz) {
            const int gz = d0 + lz;
            if (gz >= D) break;
            int boundary = 0;
            if (!flat) {
                int v[3][3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b)
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[a][b][c] = cls[lz + a][ly + b][lane + c];
                bool same = true;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b)
#pragma unroll
                        for (int c = 0; c < 3; ++c) same = same && v[a][b][c] == v[1][1][1];
                if (!same) {
                    unsigned cand = 0u;
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int b = 0; b < 3; ++b)
#pragma unroll
                            for (int c = 0; c < 3; ++c) cand |= 1u << v[a][b][c];
                    cand &= ~1u;                                                 // class 0 is never painted
                    while (cand) {
                        const int i = __ffs((int)cand) - 1;
                        cand &= cand - 1u;
                        int sd = 0, sh = 0, sw = 0;
#pragma unroll
                        for (int a = 0; a < 3; ++a)
#pragma unroll
                            for (int b = 0; b < 3; ++b)
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    const int e = v[a][b][c] == i ? 1 : 0;
                                    const int da = a - 1, db = b - 1, dc = c - 1;                  // derivative weights -1, 0, 1
                                    const int sa = 2 - da * da, sb = 2 - db * db, sc = 2 - dc * dc; // smoothing weights 1, 2, 1
                                    sd += da * sb * sc * e;
                                    sh += sa * db * sc * e;
                                    sw += sa * sb * dc * e;
                                }
                        if ((sd | sh | sw) != 0) {
                            boundary = i;
                            break;
                        }
                    }
                }
            }
            const long long at = (long long)gz * HW + (long long)gy * W + gx;
            const float raw = ct[at];
            const float m = overlay_mask_value(mk[at]);
            const float clamped = raw < 0.0f ? 0.0f : (raw > 1.0f ? 1.0f : raw);   // NaN stays NaN, as torch.clamp leaves it
            const float image = 255.0f * clamped;
            // colors[trunc(m)] * (m > 0) + image * (m == 0): the index is clamped into the table whatever m is
            const int t = (m > 0.0f && m < (float)R_CLASSES) ? (int)m : (m >= (float)R_CLASSES ? R_CLASSES - 1 : 0);
            const float kept = m == 0.0f ? image : image * 0.0f;
            const float side = image * rest;
            float *po = o + (long long)gz * 3 * HW + (long long)gy * W + gx;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float colored = (m > 0.0f ? col[t * 3 + ch] : 0.0f) + kept;
                const float im = colored * coef + side;                  // two products and a sum, each rounded: never an FMA
                // color[b] * (b > 0) + im * (b == 0)
                po[ch * HW] = boundary ? col[boundary * 3 + ch] + im * 0.0f : im;
            }
        }
    }
}

__device__ __forceinline__ unsigned char grid_byte(float v)
{
    if (!(v > 0.0f)) return 0;                           // negatives, -0.x (truncates to 0) and NaN
    return v >= 255.0f ? (unsigned char)255 : (unsigned char)(int)v;
}

__global__ __launch_bounds__(256) void make_grid_u8_kernel(const float *__restrict__ imgs, int B, int C, int H, int W, int xmaps, int padding,
                                                          int single, float pad_value, int Wg, unsigned char *__restrict__ out)
{
    const int y = (int)blockIdx.x;
    const int xg = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (xg >= Wg) return;
    long long k = -1;
    int iy = 0, ix = 0;
    if (single) {
        k = 0, iy = y, ix = xg;
    } else {
        const int ch = H + padding, cw = W + padding;
        const int yy = y - padding, xx = xg - padding;
        if (yy >= 0 && xx >= 0) {
            const int row = yy / ch, colm = xx / cw;
            iy = yy - row * ch, ix = xx - colm * cw;
            const long long kk = (long long)row * xmaps + colm;
            if (iy < H && ix < W && colm < xmaps && kk < B) k = kk;
        }
    }
    unsigned char px[3];
    if (k < 0) {
        px[0] = px[1] = px[2] = grid_byte(pad_value);
    } else {
        const long long HW = (long long)H * W;
        const float *p = imgs + k * C * HW + (long long)iy * W + ix;
        px[0] = grid_byte(p[0]);
        px[1] = C == 3 ? grid_byte(p[HW]) : px[0];
        px[2] = C == 3 ? grid_byte(p[2 * HW]) : px[0];
    }
    unsigned char *q = out + ((long long)y * Wg + xg) * 3;
    q[0] = px[0], q[1] = px[1], q[2] = px[2];
}

}  // namespace

extern "C" int gg_mask_overlay(const float *x, int32_t N, int32_t D, int32_t H, int32_t W, double overlay_coef, const int32_t *colors,
                               float *out, void *stream_)
{
    if (!x || !out || !colors) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_overlay: null pointer");
    if (N < 1 || D < 1 || H < 1 || W < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_overlay: N=%d D=%d H=%d W=%d", N, D, H, W);
    const long long tilesW = gg_cdiv(W, RT_W), tilesH = gg_cdiv(H, RT_H), tilesD = gg_cdiv(D, RT_D);
    if (tilesW * tilesH > 0x7fffffffLL || tilesD > 65535 || N > 65535)
        GG_FAIL(GG_ERR_UNSUPPORTED, "mask_overlay: N=%d D=%d H=%d W=%d exceeds the grid", N, D, H, W);
    OverlayColors c;
    for (int i = 0; i < R_CLASSES * 3; ++i) c.c[i] = (float)colors[i];
    const dim3 grid((unsigned)(tilesW * tilesH), (unsigned)tilesD, (unsigned)N);
    // the reference multiplies by the Python floats overlay_coef and 1 - overlay_coef, each rounded to fp32 on its own
    hipLaunchKernelGGL(mask_overlay_kernel, grid, dim3(RT_THREADS), 0, (hipStream_t)stream_, x, D, H, W, (int)tilesW, (float)overlay_coef,
                       (float)(1.0 - overlay_coef), c, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_make_grid_u8(const float *imgs, int32_t B, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding, float pad_value,
                               uint8_t *out, void *stream_)
{
    if (!imgs || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "make_grid_u8: null pointer");
    if (B < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) GG_FAIL(GG_ERR_BAD_SHAPE, "make_grid_u8: B=%d C=%d H=%d W=%d (C is 1 or 3)", B, C, H, W);
    if (nrow < 1 || padding < 0) GG_FAIL(GG_ERR_BAD_SHAPE, "make_grid_u8: nrow=%d padding=%d", nrow, padding);
    const int single = B == 1;
    const long long xmaps = nrow < B ? nrow : B, ymaps = (B + xmaps - 1) / xmaps;
    const long long Hg = single ? H : ymaps * ((long long)H + padding) + padding;
    const long long Wg = single ? W : xmaps * ((long long)W + padding) + padding;
    if (Hg > 0x7fffffffLL || (Wg + 255) / 256 > 65535)
        GG_FAIL(GG_ERR_UNSUPPORTED, "make_grid_u8: a %lld x %lld picture exceeds the grid", Hg, Wg);
    const dim3 grid((unsigned)Hg, (unsigned)((Wg + 255) / 256));
    hipLaunchKernelGGL(make_grid_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream_, imgs, B, C, H, W, (int)xmaps, padding, single, pad_value,
                       (int)Wg, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
