// Surface distances of label volumes on the device: the class borders (gg_label_border), an exact Euclidean distance
// transform (gg_edt_squared) and the per-volume count / sum / maximum that HD, HD95 and the average surface distances are read from
// (gg_surface_reduce).  No atomics anywhere: every output is a fixed function of the inputs, bit for bit.
//
// EDT.  min_u (sd dd)^2 + (sh dh)^2 + (sw dw)^2 separates: g1 along W from the site flags, g2[h] = min_h' g1[h'] + (sh (h - h'))^2
// along H, the same along D.  One kernel does all three passes (edt_pass_kernel):
//   * a workgroup stages a tile of WHOLE lines in LDS (at most EDT_TILE = 8192 fp64 values, 64 KiB: two workgroups per CU), so that a
//     line is read from memory once;
//   * every thread owns one output at a time and scans its line outwards, k = 1, 2, ...: both candidates at distance k cost
//     d2 = (s k)^2, and the scan stops as soon as d2 >= best.  That is exact: every value in the line is >= 0, so a candidate at distance
//     >= k is >= (s k)^2, which only grows with k (a rounded product of rounded factors is monotone), and the candidate g + d2 that
//     would be formed is >= d2 as well, rounded or not;
//   * a tile without any finite value (most of a volume when the class is small) writes +inf and scans nothing.
//   Tile element o lives at LDS index o in every pass.  Along W (EDT_ALONG_W) a tile is `lines` consecutive rows, o = row * L + l,
//   memory offset = tile * lines * L + o: the step along the line is 1.  Along H and D a line is strided in memory, and a tile is tw
//   consecutive positions of the contiguous inner extent P (P = W for the H pass, P = H * W for the D pass; tw a power of two <= 32)
//   times the whole line: o = l * tw + i, memory offset = (outer * L + l) * P + p0 + i, the step along the line is tw.  In all three
//   passes consecutive lanes read and write consecutive addresses, in memory and in LDS.
//   Every term is (s * k) * (s * k), added with contraction off: with spacings whose products are exact the result is the integer answer.
// Ping-pong: labels -> sq (W), sq -> workspace (H), workspace -> sq (D).
#include <math.h>
#include "gg_common.h"

namespace {

constexpr int SF_THREADS = 256;
constexpr int EDT_MAX_LINE = 1024;                       // include/guidegen_hip.h states this limit
constexpr int EDT_TILE = 8192;                           // fp64 values of one LDS tile
constexpr int EDT_TW_MAX = 32;
constexpr int EDT_THREADS = 512;                        // 64 KiB of LDS per workgroup: two workgroups, 16 waves per CU
constexpr int RED_PER_THREAD = 16;
constexpr int RED_CHUNK = SF_THREADS * RED_PER_THREAD;   // 4096 voxels per first-stage workgroup

// ------------------------------------------------------------------------------------------------------------- border
__global__ __launch_bounds__(SF_THREADS) void label_border_kernel(const int *__restrict__ labels, int M, int D, int H, int W, int K,
                                                                  int connectivity, unsigned char *__restrict__ border)
{
    const int i = (int)(blockIdx.x * (unsigned)SF_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    const int *lab = labels + base;
    const int c = lab[i];
    bool edge = false;
    if ((unsigned)c < (unsigned)K) {
        const int w = i % W, dh = i / W, h = dh % H, d = dh / H;
        for (int dz = -1; dz <= 1 && !edge; ++dz)
            for (int dy = -1; dy <= 1 && !edge; ++dy)
                for (int dx = -1; dx <= 1 && !edge; ++dx) {
                    const int n = abs(dz) + abs(dy) + abs(dx);
                    if (n == 0 || n > connectivity) continue;
                    const int zz = d + dz, yy = h + dy, xx = w + dx;
                    // a neighbour outside the volume counts as another label (binary_erosion's border_value = 0); rows never wrap
                    edge = zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W || lab[(zz * H + yy) * W + xx] != c;
                }
    }
    border[base + i] = edge ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- EDT
// FIRST: the staged value is 0 at a site and +inf elsewhere (labels / border); otherwise it is in[].
// ALONG_W: see the head of the file.  n: elements of a full tile (<= EDT_TILE); total: elements of the whole buffer (ALONG_W only).
template <bool FIRST, bool ALONG_W>
__global__ __launch_bounds__(EDT_THREADS) void edt_pass_kernel(const int *__restrict__ labels, const unsigned char *__restrict__ border, int cls,
                                                              const double *__restrict__ in, double *__restrict__ out, int L, long long P,
                                                              int tw, int tw_shift, int tiles_p, int n, long long total, double s)
{
#pragma clang fp contract(off)
    __shared__ double edt_lds[EDT_TILE];                 // [n] used
    const int tid = threadIdx.x;
    long long base;                                      // memory offset of tile element 0 (ALONG_W) / of (l = 0, i = 0)
    int live_i;                                          // strided passes: positions of the inner extent this tile holds
    if (ALONG_W) {
        base = (long long)blockIdx.x * n;
        live_i = 0;
    } else {
        const long long outer = (long long)(blockIdx.x / (unsigned)tiles_p);
        const long long p0 = (long long)(blockIdx.x % (unsigned)tiles_p) * tw;
        base = outer * L * P + p0;
        live_i = (int)(P - p0 < tw ? P - p0 : tw);
    }
    const int step = ALONG_W ? 1 : tw;
    const double inf = __builtin_inf();

    int found = 0;
    for (int o = tid; o < n; o += EDT_THREADS) {
        long long g;
        bool live;
        if (ALONG_W) {
            g = base + o;
            live = g < total;
        } else {
            const int l = o >> tw_shift, i = o & (tw - 1);
            g = base + (long long)l * P + i;
            live = i < live_i;
        }
        double v = inf;
        if (live) {
            if (FIRST) v = (labels[g] == cls && (!border || border[g] != 0)) ? 0.0 : inf;
            else v = in[g];
        }
        found |= v < inf;
        edt_lds[o] = v;
    }
    found = __syncthreads_or(found);                     // also the barrier between staging and scanning

    for (int o = tid; o < n; o += EDT_THREADS) {
        long long g;
        bool live;
        int l;
        if (ALONG_W) {
            g = base + o;
            live = g < total;
            l = o % L;
        } else {
            l = o >> tw_shift;
            const int i = o & (tw - 1);
            g = base + (long long)l * P + i;
            live = i < live_i;
        }
        if (!live) continue;
        double best = inf;
        if (found) {
            best = edt_lds[o];
            for (int k = 1; k < L; ++k) {
                const double sk = s * (double)k;
                const double d2 = sk * sk;
                if (!(d2 < best)) break;
                const bool lo = l - k >= 0, hi = l + k < L;
                if (!lo && !hi) break;
                if (lo) best = fmin(best, edt_lds[o - k * step] + d2);
                if (hi) best = fmin(best, edt_lds[o + k * step] + d2);
            }
        }
        out[g] = best;
    }
}

// -------------------------------------------------------------------------------------------------------------- reduce
// the workgroup's (sum of a, sum of b, max of c) in thread 0; fixed shuffle tree, then the 4 waves in index order
__device__ __forceinline__ void sf_block_reduce(double &a, double &b, double &c, double *lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
        c = fmax(c, __shfl_down(c, o));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[w * 3 + 0] = a;
        lds[w * 3 + 1] = b;
        lds[w * 3 + 2] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
        b = lds[1];
        c = lds[2];
        for (int i = 1; i < SF_THREADS / GG_WAVE; ++i) {
            a += lds[i * 3 + 0];
            b += lds[i * 3 + 1];
            c = fmax(c, lds[i * 3 + 2]);
        }
    }
}

// grid (chunks, B): chunk blockIdx.x of volume blockIdx.y; thread t owns the 16 consecutive-by-256 voxels chunk * 4096 + j * 256 + t
__global__ __launch_bounds__(SF_THREADS) void surface_member_kernel(const int *__restrict__ labels, const unsigned char *__restrict__ border,
                                                                    const double *__restrict__ sq, int cls, long long M, int chunks,
                                                                    double *__restrict__ dist2, double *__restrict__ partials)
{
    __shared__ double lds[3 * SF_THREADS / GG_WAVE];
    const long long vol = (long long)blockIdx.y * M;
    const long long m0 = (long long)blockIdx.x * RED_CHUNK + threadIdx.x;
    double cnt = 0.0, sum = 0.0, mx = -1.0;
#pragma unroll 4
    for (int j = 0; j < RED_PER_THREAD; ++j) {
        const long long m = m0 + (long long)j * SF_THREADS;
        if (m < M) {
            const long long g = vol + m;
            const bool member = labels[g] == cls && (!border || border[g] != 0);
            const double v = member ? sq[g] : -1.0;
            dist2[g] = v;
            if (member) {
                cnt += 1.0;
                sum += sqrt(v);
                mx = fmax(mx, v);
            }
        }
    }
    sf_block_reduce(cnt, sum, mx, lds);
    if (threadIdx.x == 0) {
        double *p = partials + ((long long)blockIdx.y * chunks + blockIdx.x) * 3;
        p[0] = cnt;
        p[1] = sum;
        p[2] = mx;
    }
}

// grid (B): thread t adds the partials t, t + 256, ... of its volume in that order, then the same tree
__global__ __launch_bounds__(SF_THREADS) void surface_finish_kernel(const double *__restrict__ partials, int chunks, double *__restrict__ stats)
{
    __shared__ double lds[3 * SF_THREADS / GG_WAVE];
    const double *p = partials + (long long)blockIdx.x * chunks * 3;
    double cnt = 0.0, sum = 0.0, mx = -1.0;
    for (int i = threadIdx.x; i < chunks; i += SF_THREADS) {
        cnt += p[i * 3LL + 0];
        sum += p[i * 3LL + 1];
        mx = fmax(mx, p[i * 3LL + 2]);
    }
    sf_block_reduce(cnt, sum, mx, lds);
    if (threadIdx.x == 0) {
        stats[blockIdx.x * 3LL + 0] = cnt;
        stats[blockIdx.x * 3LL + 1] = sum;
        stats[blockIdx.x * 3LL + 2] = mx;
    }
}

int sf_volumes(const char *what, int64_t B, int64_t M)
{
    if (B < 1 || B > 65535) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: B=%lld outside [1, 65535]", what, (long long)B);
    if (M < 1 || M > 0x7fffffffLL) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: %lld voxels per volume outside [1, 2^31)", what, (long long)M);
    return GG_OK;
}

bool edt_extents_ok(int64_t B, int64_t D, int64_t H, int64_t W)
{
    return B >= 1 && B <= 65535 && D >= 1 && H >= 1 && W >= 1 && D <= EDT_MAX_LINE && H <= EDT_MAX_LINE && W <= EDT_MAX_LINE;
}

// one strided pass (H or D): `outers` blocks of L lines of the contiguous inner extent P
template <bool FIRST>
int edt_strided(const char *what, const double *in, double *out, long long outers, int L, long long P, double s, hipStream_t stream)
{
    int tw = 1, shift = 0;
    while (tw * 2 <= EDT_TW_MAX && tw * 2 * L <= EDT_TILE && tw < P) { tw *= 2; ++shift; }
    const long long tiles_p = (P + tw - 1) / tw;
    const long long tiles = outers * tiles_p;
    if (tiles > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "edt_squared: %lld tiles of the %s pass exceed the grid", tiles, what);
    const int n = tw * L;
    hipLaunchKernelGGL((edt_pass_kernel<FIRST, false>), dim3((unsigned)tiles), dim3(EDT_THREADS), 0, stream,
                       (const int *)nullptr, (const unsigned char *)nullptr, 0, in, out, L, P, tw, shift, (int)tiles_p, n, 0LL, s);
    return GG_OK;
}

}  // namespace

extern "C" int gg_label_border(const int32_t *labels, int32_t B, int32_t D, int32_t H, int32_t W, int32_t K, int32_t connectivity,
                               uint8_t *border, void *stream_)
{
    if (!labels || !border) GG_FAIL(GG_ERR_BAD_SHAPE, "label_border: null pointer");
    if (D < 1 || H < 1 || W < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "label_border: D=%d H=%d W=%d", D, H, W);
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "label_border: K=%d outside [1, 32]", K);
    if (connectivity < 1 || connectivity > 3) GG_FAIL(GG_ERR_BAD_SHAPE, "label_border: connectivity %d outside 1..3", connectivity);
    const int64_t M = (int64_t)D * H * W;
    if (int rc = sf_volumes("label_border", B, M)) return rc;
    const dim3 grid((unsigned)((M + SF_THREADS - 1) / SF_THREADS), (unsigned)B);
    hipLaunchKernelGGL(label_border_kernel, grid, dim3(SF_THREADS), 0, (hipStream_t)stream_, labels, (int)M, D, H, W, K, connectivity, border);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int64_t gg_edt_squared_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W)
{
    if (!edt_extents_ok(B, D, H, W) || (int64_t)D * H * W > 0x7fffffffLL) return 0;
    return (int64_t)B * D * H * W * (int64_t)sizeof(double);
}

extern "C" int gg_edt_squared(const int32_t *labels, const uint8_t *border, int32_t cls, int32_t B, int32_t D, int32_t H, int32_t W, double sd,
                              double sh, double sw, double *sq, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!labels || !sq || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "edt_squared: null pointer");
    if (D < 1 || H < 1 || W < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "edt_squared: D=%d H=%d W=%d", D, H, W);
    if (D > EDT_MAX_LINE || H > EDT_MAX_LINE || W > EDT_MAX_LINE)
        GG_FAIL(GG_ERR_UNSUPPORTED, "edt_squared: D=%d H=%d W=%d: an extent above %d, the line length the LDS tile is sized for", D, H, W,
                EDT_MAX_LINE);
    const int64_t M = (int64_t)D * H * W;
    if (int rc = sf_volumes("edt_squared", B, M)) return rc;
    if (!(sd > 0.0 && sh > 0.0 && sw > 0.0 && isfinite(sd) && isfinite(sh) && isfinite(sw)))
        GG_FAIL(GG_ERR_BAD_SHAPE, "edt_squared: spacing (%g, %g, %g) must be finite and > 0", sd, sh, sw);
    const int64_t need = gg_edt_squared_workspace_bytes(B, D, H, W);
    if (workspace_bytes < need)
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "edt_squared: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    hipStream_t stream = (hipStream_t)stream_;
    double *ws = (double *)workspace;

    // along W: whole rows, as many as the tile holds
    const long long rows = (long long)B * D * H;
    const int lines = EDT_TILE / W;                      // >= 8
    const long long tiles = (rows + lines - 1) / lines;
    if (tiles > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "edt_squared: %lld tiles of the W pass exceed the grid", tiles);
    const int n = lines * W;
    hipLaunchKernelGGL((edt_pass_kernel<true, true>), dim3((unsigned)tiles), dim3(EDT_THREADS), 0, stream, labels,
                       (const unsigned char *)border, cls, (const double *)nullptr, sq, W, 1LL, 1, 0, 1, n, rows * W, sw);
    if (int rc = edt_strided<false>("H", sq, ws, (long long)B * D, H, (long long)W, sh, stream)) return rc;
    if (int rc = edt_strided<false>("D", ws, sq, (long long)B, D, (long long)H * W, sd, stream)) return rc;
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int64_t gg_surface_reduce_workspace_bytes(int32_t B, int64_t M)
{
    if (B < 1 || M < 1) return 0;
    return (int64_t)B * ((M + RED_CHUNK - 1) / RED_CHUNK) * 3 * (int64_t)sizeof(double);
}

extern "C" int gg_surface_reduce(const int32_t *labels_a, const uint8_t *border_a, const double *sq_b, int32_t cls, int32_t B, int64_t M,
                                 double *dist2, double *stats, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!labels_a || !sq_b || !dist2 || !stats || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "surface_reduce: null pointer");
    if (int rc = sf_volumes("surface_reduce", B, M)) return rc;
    const int64_t need = gg_surface_reduce_workspace_bytes(B, M);
    if (workspace_bytes < need)
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "surface_reduce: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    hipStream_t stream = (hipStream_t)stream_;
    const int chunks = (int)((M + RED_CHUNK - 1) / RED_CHUNK);
    double *partials = (double *)workspace;
    hipLaunchKernelGGL(surface_member_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(SF_THREADS), 0, stream, labels_a,
                       (const unsigned char *)border_a, sq_b, cls, (long long)M, chunks, dist2, partials);
    hipLaunchKernelGGL(surface_finish_kernel, dim3((unsigned)B), dim3(SF_THREADS), 0, stream, (const double *)partials, chunks, stats);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
