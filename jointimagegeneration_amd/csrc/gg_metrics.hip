// Pairwise confusion matrices of label volumes (gg_label_confusion): the one pass over the voxels that Dice, the generalised energy
// distance and the Hungarian-matched IoU of an ensemble of sampled masks need (ccdm/ddpm/evaluator.py:188-190, ccdm/ddpm/utils.py:190-236).
//   cm[i, j, p, q] = #{ m : a[i, m] == p and b[j, m] == q },   skipped[i, j] = #{ m : a[i, m] or b[j, m] outside [0, K) }
// Integer counts: adds commute, so the result is exact and independent of the order the workgroups run in.
//
// Mapping.  grid = (voxel chunks, pair tiles).  A workgroup of 256 threads owns `chunk` consecutive voxels and a tile of na x nb pairs
// (na, nb <= T): per voxel it loads the na + nb labels ONCE and updates na * nb histograms, so that at 12 x 12 pairs and T = 6 every
// volume is read twice (48 volume reads in all), not 12 times (288).  A lane reads one voxel per row and load, a wave 64 consecutive
// voxels (256 B, coalesced; no alignment condition on M); CM_UNROLL such loads per row are in flight.
//
// Histograms: ONE uint32 copy per workgroup in LDS, [na * nb][K * K], updated with LDS atomicAdd and flushed once, at the end of the
// chunk, with 64-bit global atomicAdd (zero bins are not flushed: most bins of a label map are empty).  T comes from K on the host: the
// largest T in 1..6 with T * T * K * K * 4 <= 40 KiB, so that at least 4 workgroups (16 waves) fit the 160 KiB of a CU: K <= 16: T = 6
// (K = 14: 28 224 B, 5 workgroups); K = 32: T = 3 (36 864 B, 4 workgroups).
// Counter range: a voxel adds 1 to exactly one bin of a pair (or 64 voxels add 64 at once), so one LDS counter receives at most `chunk`
// counts before its flush, and chunk <= CM_CHUNK_MAX = 2^24 < 2^32: no counter can wrap.
//
// Same-bin contention.  Label maps are mostly background: without care the 64 lanes of a wave add to bin (0, 0) of every pair, one
// after the other.  Per row and load the wave finds out, with votes alone, whether its 64 labels are one valid value (every bit plane
// of the label is all ones or all zeros; the value is then lane 0's, read off the ballots).  A pair whose two rows are uniform takes ONE
// add of 64 from lane 0; any other pair takes the per-lane atomic.  GG_CONFUSION_UNIFORM=0 in the environment selects the kernel
// without this path (measurement switch, tools/bench_metrics.py; the numbers are in DESIGN.md 7f).
#include <stdlib.h>
#include <string.h>
#include "gg_common.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_UNROLL = 4;
constexpr int CM_TMAX = 6;
constexpr int CM_LDS_CAP = 40 * 1024;
constexpr long long CM_CHUNK_MIN = 4096;
constexpr long long CM_CHUNK_MAX = 1LL << 24;
constexpr int CM_TARGET_WGS = 1024;                      // 256 CUs x 4 resident workgroups

template <int T, bool UNI>
__global__ __launch_bounds__(CM_THREADS) void confusion_kernel(const int *__restrict__ a, const int *__restrict__ b, int Sa, int Sb, long long M,
                                                              int K, int nbits, long long chunk, int tilesB, unsigned long long *cm,
                                                              unsigned long long *skipped)
{
    extern __shared__ unsigned cm_hist[];                // [na * nb][K * K]
    __shared__ unsigned cm_skip[T * T];
    const int tid = threadIdx.x;
    const int lane = tid & (GG_WAVE - 1);
    const int i0 = ((int)blockIdx.y / tilesB) * T, j0 = ((int)blockIdx.y % tilesB) * T;
    const int na = min(T, Sa - i0), nb = min(T, Sb - j0);
    const int KK = K * K;
    const int nh = na * nb * KK;
    for (int x = tid; x < nh; x += CM_THREADS) cm_hist[x] = 0u;
    if (tid < T * T) cm_skip[tid] = 0u;
    __syncthreads();

    const long long m0 = (long long)blockIdx.x * chunk;
    const long long m1 = min(M, m0 + chunk);
    const int *pa = a + (long long)i0 * M;
    const int *pb = b + (long long)j0 * M;
    for (long long base = m0; base < m1; base += CM_THREADS * CM_UNROLL) {
        int la[CM_UNROLL][T], lb[CM_UNROLL][T];
#pragma unroll
        for (int u = 0; u < CM_UNROLL; ++u) {
            const long long m = base + u * CM_THREADS + tid;
            const bool live = m < m1;
#pragma unroll
            for (int i = 0; i < T; ++i) {                // a row past the tile, or a voxel past the chunk, is never read
                la[u][i] = (live && i < na) ? pa[(long long)i * M + m] : 0;
                lb[u][i] = (live && i < nb) ? pb[(long long)i * M + m] : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < CM_UNROLL; ++u) {
            const bool live = base + u * CM_THREADS + tid < m1;
            bool oka[T], okb[T], ua[T], ub[T];
            int fa[T], fb[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                oka[i] = live && (unsigned)la[u][i] < (unsigned)K;
                okb[i] = live && (unsigned)lb[u][i] < (unsigned)K;
                ua[i] = ub[i] = false;
                fa[i] = fb[i] = 0;
                if constexpr (UNI) {
                    // all 64 lanes live and valid, and every bit plane of the label all ones or all zeros: one value, lane 0's
                    bool a1 = __all(oka[i]), b1 = __all(okb[i]);
#pragma unroll
                    for (int bit = 0; bit < 5; ++bit) {
                        if (bit < nbits && a1) {         // wave-uniform: a row that is mixed in one bit plane skips the others
                            const unsigned long long ma = __ballot((la[u][i] >> bit) & 1);
                            a1 = ma == 0ull || ma == ~0ull;
                            fa[i] |= (int)(ma & 1ull) << bit;
                        }
                        if (bit < nbits && b1) {
                            const unsigned long long mb = __ballot((lb[u][i] >> bit) & 1);
                            b1 = mb == 0ull || mb == ~0ull;
                            fb[i] |= (int)(mb & 1ull) << bit;
                        }
                    }
                    ua[i] = a1;
                    ub[i] = b1;
                }
            }
#pragma unroll
            for (int i = 0; i < T; ++i) {
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    if (i >= na || j >= nb) continue;            // wave-uniform: a pair past the tile's edge
                    unsigned *h = cm_hist + (i * nb + j) * KK;
                    if (UNI && ua[i] && ub[j]) {         // wave-uniform branch
                        if (lane == 0) atomicAdd(&h[fa[i] * K + fb[j]], (unsigned)GG_WAVE);
                    } else if (oka[i] && okb[j]) {       // both labels inside [0, K): the only indexed access to the histogram
                        atomicAdd(&h[la[u][i] * K + lb[u][j]], 1u);
                    } else if (live) {
                        atomicAdd(&cm_skip[i * T + j], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();

    for (int x = tid; x < nh; x += CM_THREADS) {
        const unsigned v = cm_hist[x];
        if (v) {
            const int pair = x / KK, bin = x - pair * KK;
            const int i = pair / nb, j = pair - i * nb;
            atomicAdd(&cm[((long long)(i0 + i) * Sb + (j0 + j)) * KK + bin], (unsigned long long)v);
        }
    }
    if (skipped && tid < T * T) {
        const int i = tid / T, j = tid % T;
        const unsigned v = cm_skip[tid];
        if (v && i < na && j < nb) atomicAdd(&skipped[(long long)(i0 + i) * Sb + (j0 + j)], (unsigned long long)v);
    }
}

template <int T>
void confusion_launch(bool uni, dim3 grid, size_t lds, hipStream_t stream, const int *a, const int *b, int Sa, int Sb, long long M, int K,
                      int nbits, long long chunk, int tilesB, unsigned long long *cm, unsigned long long *skipped)
{
    if (uni)
        hipLaunchKernelGGL((confusion_kernel<T, true>), grid, dim3(CM_THREADS), lds, stream, a, b, Sa, Sb, M, K, nbits, chunk, tilesB, cm, skipped);
    else
        hipLaunchKernelGGL((confusion_kernel<T, false>), grid, dim3(CM_THREADS), lds, stream, a, b, Sa, Sb, M, K, nbits, chunk, tilesB, cm, skipped);
}

}  // namespace

extern "C" int gg_label_confusion(const int32_t *a, int32_t Sa, const int32_t *b, int32_t Sb, int64_t M, int32_t K, int64_t *cm_out,
                                  int64_t *skipped_out, void *stream_)
{
    if (!a || !b || !cm_out) GG_FAIL(GG_ERR_BAD_SHAPE, "label_confusion: null pointer");
    if (Sa < 1 || Sb < 1 || M < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "label_confusion: Sa=%d Sb=%d M=%lld", Sa, Sb, (long long)M);
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "label_confusion: K=%d outside [1, 32]", K);
    hipStream_t stream = (hipStream_t)stream_;
    const int KK = K * K;
    int T = CM_TMAX;
    while (T > 1 && T * T * KK * 4 > CM_LDS_CAP) --T;
    const long long tilesA = (Sa + T - 1) / T, tilesB = (Sb + T - 1) / T;
    if (tilesA * tilesB > 65535) GG_FAIL(GG_ERR_UNSUPPORTED, "label_confusion: %lld pair tiles exceed the grid", tilesA * tilesB);
    const int tiles = (int)(tilesA * tilesB);
    // about CM_TARGET_WGS workgroups in all; a chunk is a whole number of unrolled passes and at most CM_CHUNK_MAX voxels
    const long long want = CM_TARGET_WGS / tiles > 0 ? CM_TARGET_WGS / tiles : 1;
    const long long step = CM_THREADS * CM_UNROLL;
    long long chunk = ((M + want - 1) / want + step - 1) / step * step;
    if (chunk < CM_CHUNK_MIN) chunk = CM_CHUNK_MIN;
    if (chunk > CM_CHUNK_MAX) chunk = CM_CHUNK_MAX;
    const long long chunks = (M + chunk - 1) / chunk;
    if (chunks > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "label_confusion: M=%lld voxels exceed the grid", (long long)M);
    int nbits = 0;
    while ((1 << nbits) < K) ++nbits;
    const size_t lds = (size_t)(Sa < T ? Sa : T) * (size_t)(Sb < T ? Sb : T) * KK * sizeof(unsigned);
    const char *env = getenv("GG_CONFUSION_UNIFORM");
    const bool uni = !(env && strcmp(env, "0") == 0);

    if (hipMemsetAsync(cm_out, 0, (size_t)Sa * Sb * KK * sizeof(int64_t), stream) != hipSuccess ||
        (skipped_out && hipMemsetAsync(skipped_out, 0, (size_t)Sa * Sb * sizeof(int64_t), stream) != hipSuccess))
        GG_FAIL(GG_ERR_HIP, "label_confusion: hipMemsetAsync failed");
    const dim3 grid((unsigned)chunks, (unsigned)tiles);
    unsigned long long *cm = (unsigned long long *)cm_out, *sk = (unsigned long long *)skipped_out;
#define CM_CASE(TT)                                                                                             \
    case TT:                                                                                                    \
        confusion_launch<TT>(uni, grid, lds, stream, a, b, Sa, Sb, (long long)M, K, nbits, chunk, (int)tilesB, cm, sk); \
        break;
    switch (T) {
        CM_CASE(3) CM_CASE(4) CM_CASE(5) CM_CASE(6)          // K <= 32 never gives T < 3
    }
#undef CM_CASE
    GG_CHECK_LAUNCH();
    return GG_OK;
}
