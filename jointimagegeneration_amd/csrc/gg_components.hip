// Cleaning of sampled label volumes on the device: the per-voxel vote of S samples (gg_label_vote), connected components
// in canonical form (gg_label_components), their sizes and per-class summary (gg_component_stats) and the keep-largest / minimum-size
// filter (gg_component_filter).  Everything is integer work except the vote's entropy, whose fp32 recipe is fixed below, so every
// output is exact and independent of the order the workgroups run in.
//
// Components: a union-find over the voxels of one volume, parent[] in the caller's workspace, local indices (volumes never join).
//   Invariant: parent[i] <= i for every foreground voxel, always.  A tree's root is therefore the smallest index of the tree, a find
//   walks strictly downwards and ends within M steps, and the root of a finished component is its smallest linear index.
//   1. cc_init_kernel     parent[i] = first voxel of i's run of equal labels along x (-1: background or a label outside [0, K)).
//                         Plain stores; the kernel boundary publishes them.
//   2. cc_merge_kernel    one thread per voxel unions it with its equal-labelled neighbours in the rows BEFORE its own (the x
//                         neighbours are joined by step 1, the rows after it by their own threads).  A union whose two ends have left
//                         neighbours that are already joined the same way is skipped: the left pair performs it.
//                         Workgroups on different CUs and XCDs read and write the same parent entries here, a CU's L1 is never
//                         refreshed by another CU's stores and the per-XCD L2s are not coherent with each other: EVERY access to
//                         parent[] in this kernel is an agent-scope atomic (relaxed load, fetch_min), served where all CUs meet.
//                         No other ordering is needed: a reader may see any past value of an entry, and every past value is an
//                         ancestor-or-self under the invariant (fetch_min only lowers an entry, and only to a member of its set).
//   3. cc_flatten_kernel  after the boundary: root[i] = find(i) with plain loads of parent[], which no thread writes any more.
//   Union(a, b): a = find(a), b = find(b); equal: done; else fetch_min(parent[max], min).  If the old value was max itself it was a
//   root and now hangs under min: done.  Otherwise another thread re-parented it meanwhile: its old parent may have lost its only link
//   when min was lower, so the union goes on with (old, min).  Each retry strictly lowers the larger of the two ends.
//   Bounds: find <= M steps, union <= M retries; a thread that reaches a bound sets *status and returns (the host raises from it).
#include "gg_common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int VOTE_THREADS = 256;

__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Outputs that atomics add into are zeroed by a kernel of this file, not by a memset node: the whole sequence is then kernels in stream
// order, eager and inside a captured graph alike.
__global__ __launch_bounds__(256) void cc_zero_kernel(int *__restrict__ p, long long n)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) p[i] = 0;
}

void cc_zero(void *p, long long words, hipStream_t stream)
{
    hipLaunchKernelGGL(cc_zero_kernel, dim3(gg_blocks256(words, 4096)), dim3(256), 0, stream, (int *)p, words);
}

// ---------------------------------------------------------------------------------------------------------------- vote
// H = ln S - acc / S with the product and the difference rounded separately.  The contraction is switched off HERE: the compiler's
// default fuses the pair into one FMA even through __fmul_rn / __fsub_rn, and a unanimous vote then gets H = -2.4e-8 instead of 0.
__device__ __forceinline__ float vote_entropy(float lnS, float acc, float invS)
{
#pragma clang fp contract(off)
    const float prod = acc * invS;
    return lnS - prod;
}

// Counts of up to 32 classes, each <= 64, packed four to a register: no indexed register array, no scratch.
__global__ __launch_bounds__(VOTE_THREADS) void vote_kernel(const int *__restrict__ labels, int S, long long M, int K,
                                                            const float *__restrict__ table, float lnS, float invS,
                                                            int *__restrict__ winner, int *__restrict__ agreement,
                                                            float *__restrict__ entropy, unsigned long long *skipped)
{
    __shared__ float t_lds[65];
    __shared__ unsigned skip_lds;
    const int tid = threadIdx.x;
    if (tid <= S) t_lds[tid] = table[tid];
    if (tid == 0) skip_lds = 0u;
    __syncthreads();
    const long long m = (long long)blockIdx.x * VOTE_THREADS + tid;
    unsigned nskip = 0;
    if (m < M) {
        unsigned cnt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int s = 0; s < S; ++s) {
            const int l = labels[(long long)s * M + m];
            if ((unsigned)l < (unsigned)K) {
                const unsigned inc = 1u << ((l & 3) * 8);
                const int w = l >> 2;
#pragma unroll
                for (int j = 0; j < 8; ++j) cnt[j] += (w == j) ? inc : 0u;
            } else {
                ++nskip;
            }
        }
        int best = 0, bestc = 0;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k < K) {
                const int c = (int)((cnt[k >> 2] >> ((k & 3) * 8)) & 0xffu);
                if (c > bestc) { bestc = c; best = k; }                    // strict: the smallest label among the most voted
                acc = __fadd_rn(acc, t_lds[c]);
            }
        }
        winner[m] = best;
        agreement[m] = bestc;
        entropy[m] = bestc > 0 ? vote_entropy(lnS, acc, invS) : 0.0f;
    }
    if (nskip) atomicAdd(&skip_lds, nskip);
    __syncthreads();
    if (tid == 0 && skip_lds) atomicAdd(skipped, (unsigned long long)skip_lds);
}

// ---------------------------------------------------------------------------------------------------------- components
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const int *__restrict__ labels, int M, int W, int K, int background,
                                                             int *__restrict__ parent)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    const int *lab = labels + base;
    const int c = lab[i];
    int p = -1;
    if ((unsigned)c < (unsigned)K && c != background) {
        int x = i % W;
        p = i;
        while (x > 0 && lab[p - 1] == c) { --p; --x; }                     // at most W - 1 steps, never past the row's first voxel
    }
    parent[base + i] = p;
}

// the root of i; -1 when the bound is reached (status set)
__device__ __forceinline__ int cc_find(const int *parent, int i, int bound, int *status)
{
    for (int n = 0; n <= bound; ++n) {
        const int p = cc_load(parent + i);
        if (p >= i || p < 0) return i;                                     // p == i: a root (p > i or p < 0 cannot happen; they end the walk)
        i = p;
    }
    __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return -1;
}

__device__ __forceinline__ void cc_union(int *parent, int a, int b, int bound, int *status)
{
    for (int n = 0; n <= bound; ++n) {
        a = cc_find(parent, a, bound, status);
        b = cc_find(parent, b, bound, status);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                      // a the larger end
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;                                              // a was a root and now hangs under b
        a = old;                                                           // a had been re-parented: its old parent still has to meet b
    }
    __hip_atomic_store(status, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const int *__restrict__ labels, int M, int D, int H, int W, int K,
                                                              int background, int conn26, int *parent, int *status)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    const int *lab = labels + base;
    int *par = parent + base;
    const int c = lab[i];
    if ((unsigned)c >= (unsigned)K || c == background) return;
    const int x = i % W, yz = i / W, y = yz % H, z = yz / H;
    const bool left = x > 0 && lab[i - 1] == c;
    // the rows before this one: (dz, dy) = (0, -1), and with 26 neighbours (-1, -1), (-1, 0), (-1, 1); with 6: (0, -1) and (-1, 0)
    const int ndir = conn26 ? 4 : 2;
    for (int d = 0; d < ndir; ++d) {
        int dz, dy;
        if (conn26) { dz = d == 0 ? 0 : -1; dy = d == 0 ? -1 : d - 2; }
        else { dz = d == 0 ? 0 : -1; dy = d == 0 ? -1 : 0; }
        const int zz = z + dz, yy = y + dy;
        if (zz < 0 || yy < 0 || yy >= H) continue;                         // rows never wrap: a neighbour outside the volume is none
        const int q = (zz * H + yy) * W + x;                               // same x in the neighbour row
        if (lab[q] == c) {
            // q's run holds q - 1 and q + 1 where they carry c, so the diagonal unions add nothing; and where both left neighbours
            // carry c, thread i - 1 performs this very union of the two runs
            if (!(left && lab[q - 1] == c)) cc_union(par, i, q, M, status);
        } else if (conn26) {
            if (x > 0 && lab[q - 1] == c) cc_union(par, i, q - 1, M, status);
            if (x + 1 < W && lab[q + 1] == c) cc_union(par, i, q + 1, M, status);
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int *__restrict__ parent, int M, int *__restrict__ root, int *status)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    const int *par = parent + base;
    int r = par[i];
    if (r >= 0) {
        int n = 0;
        for (;;) {
            const int p = par[r];
            if (p >= r || p < 0) break;
            r = p;
            if (++n > M) {
                __hip_atomic_store(status, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                r = -1;
                break;
            }
        }
    }
    root[base + i] = r;
}

// --------------------------------------------------------------------------------------------------------------- stats
// size[root] += 1 per voxel.  The lanes of a wave that hold the same root as its first live lane add once, together.
__global__ __launch_bounds__(CC_THREADS) void cc_size_kernel(const int *__restrict__ root, int M, int *size)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    const long long base = (long long)blockIdx.y * M;
    int r = i < M ? root[base + i] : -1;
    if (r >= M) r = -1;                                                    // a root buffer that is not ours: nothing out of bounds
    const int lane = threadIdx.x & (GG_WAVE - 1);
    for (int n = 0; n < GG_WAVE; ++n) {                                    // every pass retires at least one live lane
        const unsigned long long live = __ballot(r >= 0);
        if (live == 0ull) break;
        const int first = __ffsll((long long)live) - 1;
        const int r0 = __shfl(r, first);
        const unsigned long long same = __ballot(r == r0);
        if (lane == first) atomicAdd(size + base + r0, (int)__popcll(same));
        if (r == r0) r = -1;
    }
}

// per class: components, voxels, and the largest as one 64-bit maximum of (size << 32 | 0x7fffffff - root): equal sizes tie to the
// smaller root.  stats[.., 2] holds that key until cc_stats_final_kernel splits it.
__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const int *__restrict__ labels, const int *__restrict__ root,
                                                              const int *__restrict__ size, int M, int K, unsigned long long *stats)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    if (root[base + i] != i) return;
    const int c = labels[base + i];
    if ((unsigned)c >= (unsigned)K) return;
    const int sz = size[base + i];
    unsigned long long *st = stats + ((long long)blockIdx.y * K + c) * 4;
    atomicAdd(st + 0, 1ull);
    atomicAdd(st + 1, (unsigned long long)sz);
    atomicMax(st + 2, ((unsigned long long)(unsigned)sz << 32) | (unsigned long long)(0x7fffffff - i));
}

__global__ void cc_stats_final_kernel(long long *stats, int rows)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= rows) return;
    const unsigned long long key = (unsigned long long)stats[r * 4LL + 2];
    stats[r * 4LL + 2] = (long long)(key >> 32);
    stats[r * 4LL + 3] = key ? (long long)(0x7fffffff - (int)(key & 0xffffffffull)) : -1LL;
}

// -------------------------------------------------------------------------------------------------------------- filter
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const int *__restrict__ labels, const int *__restrict__ root,
                                                               const int *__restrict__ size, const long long *__restrict__ stats,
                                                               int M, int K, const int *__restrict__ keep_largest,
                                                               const int *__restrict__ min_size, int background, int fill,
                                                               int *__restrict__ out, unsigned char *__restrict__ kept)
{
    const int i = (int)(blockIdx.x * (unsigned)CC_THREADS + threadIdx.x);
    if (i >= M) return;
    const long long base = (long long)blockIdx.y * M;
    const int c = labels[base + i];
    bool keep;
    if (c == background) {
        keep = true;
    } else if ((unsigned)c >= (unsigned)K) {
        keep = false;                                                      // no class, no policy: such a voxel is filled
    } else {
        const int r = root[base + i];
        keep = r >= 0 && r < M;
        if (keep) {
            const bool big = keep_largest[c] == 0 || (long long)r == stats[((long long)blockIdx.y * K + c) * 4 + 3];
            keep = big && size[base + r] >= min_size[c];
        }
    }
    out[base + i] = keep ? c : fill;
    kept[base + i] = keep ? 1 : 0;
}

int cc_grid(const char *what, int64_t B, int64_t M, dim3 *grid)
{
    if (B < 1 || B > 65535) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: B=%lld outside [1, 65535]", what, (long long)B);
    if (M < 1 || M > 0x7fffffffLL) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: %lld voxels per volume outside [1, 2^31)", what, (long long)M);
    *grid = dim3((unsigned)((M + CC_THREADS - 1) / CC_THREADS), (unsigned)B);
    return GG_OK;
}

}  // namespace

extern "C" int gg_label_vote(const int32_t *labels, int32_t S, int64_t M, int32_t K, const float *table_dev, float ln_s, float inv_s,
                             int32_t *winner, int32_t *agreement, float *entropy, int64_t *skipped, void *stream_)
{
    if (!labels || !table_dev || !winner || !agreement || !entropy || !skipped) GG_FAIL(GG_ERR_BAD_SHAPE, "label_vote: null pointer");
    if (S < 1 || S > 64) GG_FAIL(GG_ERR_BAD_SHAPE, "label_vote: S=%d outside [1, 64]", S);
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "label_vote: K=%d outside [1, 32]", K);
    if (M < 1 || M > 0x7fffffffLL) GG_FAIL(GG_ERR_BAD_SHAPE, "label_vote: M=%lld outside [1, 2^31)", (long long)M);
    hipStream_t stream = (hipStream_t)stream_;
    cc_zero(skipped, 2, stream);
    const unsigned blocks = (unsigned)((M + VOTE_THREADS - 1) / VOTE_THREADS);
    hipLaunchKernelGGL(vote_kernel, dim3(blocks), dim3(VOTE_THREADS), 0, stream, labels, S, (long long)M, K, table_dev, ln_s, inv_s, winner,
                       agreement, entropy, (unsigned long long *)skipped);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int64_t gg_label_components_workspace_bytes(int32_t B, int64_t M)
{
    return (B < 1 || M < 1) ? 0 : (int64_t)B * M * (int64_t)sizeof(int32_t);
}

extern "C" int gg_label_components(const int32_t *labels, int32_t B, int32_t D, int32_t H, int32_t W, int32_t K, int32_t connectivity,
                                   int32_t background, int32_t *root, void *workspace, int64_t workspace_bytes, int32_t *status,
                                   void *stream_)
{
    if (!labels || !root || !workspace || !status) GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: null pointer");
    if (D < 1 || H < 1 || W < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: D=%d H=%d W=%d", D, H, W);
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: K=%d outside [1, 32]", K);
    if (connectivity != 6 && connectivity != 26) GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: connectivity %d is neither 6 nor 26", connectivity);
    if (background < -1 || background >= K) GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: background %d outside [-1, %d)", background, K);
    const int64_t M = (int64_t)D * H * W;
    dim3 grid;
    if (int rc = cc_grid("label_components", B, M, &grid)) return rc;
    if (workspace_bytes < gg_label_components_workspace_bytes(B, M))
        GG_FAIL(GG_ERR_BAD_SHAPE, "label_components: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)gg_label_components_workspace_bytes(B, M));
    hipStream_t stream = (hipStream_t)stream_;
    int *parent = (int *)workspace;
    hipLaunchKernelGGL(cc_init_kernel, grid, dim3(CC_THREADS), 0, stream, labels, (int)M, W, K, background, parent);
    hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(CC_THREADS), 0, stream, labels, (int)M, D, H, W, K, background,
                       connectivity == 26 ? 1 : 0, parent, status);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(CC_THREADS), 0, stream, (const int *)parent, (int)M, root, status);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_component_stats(const int32_t *labels, const int32_t *root, int32_t B, int64_t M, int32_t K, int32_t *size, int64_t *stats,
                                  void *stream_)
{
    if (!labels || !root || !size || !stats) GG_FAIL(GG_ERR_BAD_SHAPE, "component_stats: null pointer");
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "component_stats: K=%d outside [1, 32]", K);
    dim3 grid;
    if (int rc = cc_grid("component_stats", B, M, &grid)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    cc_zero(size, (long long)B * M, stream);
    cc_zero(stats, (long long)B * K * 8, stream);
    hipLaunchKernelGGL(cc_size_kernel, grid, dim3(CC_THREADS), 0, stream, root, (int)M, size);
    hipLaunchKernelGGL(cc_stats_kernel, grid, dim3(CC_THREADS), 0, stream, labels, root, (const int *)size, (int)M, K,
                       (unsigned long long *)stats);
    const int rows = B * K;
    hipLaunchKernelGGL(cc_stats_final_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, (long long *)stats, rows);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_component_filter(const int32_t *labels, const int32_t *root, const int32_t *size, const int64_t *stats, int32_t B, int64_t M,
                                   int32_t K, const int32_t *keep_largest, const int32_t *min_size, int32_t background, int32_t fill,
                                   int32_t *out_labels, uint8_t *kept, void *stream_)
{
    if (!labels || !root || !size || !stats || !keep_largest || !min_size || !out_labels || !kept)
        GG_FAIL(GG_ERR_BAD_SHAPE, "component_filter: null pointer");
    if (K < 1 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "component_filter: K=%d outside [1, 32]", K);
    if (background < -1 || background >= K) GG_FAIL(GG_ERR_BAD_SHAPE, "component_filter: background %d outside [-1, %d)", background, K);
    if (fill < 0 || fill >= K) GG_FAIL(GG_ERR_BAD_SHAPE, "component_filter: fill %d outside [0, %d)", fill, K);
    dim3 grid;
    if (int rc = cc_grid("component_filter", B, M, &grid)) return rc;
    hipLaunchKernelGGL(cc_filter_kernel, grid, dim3(CC_THREADS), 0, (hipStream_t)stream_, labels, root, size, (const long long *)stats, (int)M, K,
                       keep_largest, min_size, background, fill, out_labels, kept);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
