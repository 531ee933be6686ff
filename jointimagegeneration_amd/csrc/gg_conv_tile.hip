// Streaming 1x1 convolution for big grids (the CCDM UNet's skip projections @64^3 and @128^3), byte-identical to conv_gather_kernel.
//
// A 1x1 stride-1 conv over channels-last rows is a GEMM whose activation operand is one contiguous run per source.  The gather kernel
// re-stages a 2 KiB weight tile and a 64-byte slice of every row per 32-channel k-step, behind one barrier each; on these shapes it is
// bound by neither bytes nor MFMAs.  Here
//   * the whole packed weight image (unchanged format, <= 64 KiB) is copied into LDS once per workgroup and stays there;
//   * every wave owns tiles of 32 consecutive positions: it loads a tile as full 16-byte-per-lane runs (all channels of a row, row after
//     row), one tile ahead of the one it computes on (register double buffer), writes it into its private LDS stage in the gather
//     kernel's [chunk][row][64 B swizzled] layout, runs the MFMAs, transposes the bf16 result through the same stage and stores it as
//     full lines;
//   * waves never wait for each other after the weight copy (the stage is wave-private; LDS instructions of one wave execute in
//     order), so the loads, MFMAs and stores of the four waves of a workgroup -- and of the workgroups sharing a CU -- overlap.
// Bit-identity: each output element is accumulated by the same instruction (v_mfma_f32_16x16x32_bf16, weights as A, activations as B),
// over the same 32-channel chunks in ascending order, from a zero accumulator, and passes through the same epilogue expression
// (gg_conv_epi_value / gg_conv_epi_bf16, gg_conv.h).  Like the gather kernel on these shapes it leaves no GroupNorm sums
// (gg_conv_emits_stats == 0).
#include "gg_conv.h"
#include <atomic>

#ifndef GG_TILE_CONV
#define GG_TILE_CONV 1        /* A/B switch: 0 = the tile kernels decline everything (the gather kernel runs, as before) */
#endif

// smallest grid the kernel takes: 64^3 positions.  Measured per launch in the CCDM forward (profiles/tile_conv/): @128^3 and @64^3 every
// shape beats the gather kernel; @32^3 (32 tiles per CU, one per wave: nothing to pipeline, and the weight copy is not amortised) 256 -> 128
// took 20.7 us against 16 us.
#define GG_TILE_MIN_M 262144

// LDS layout, stated once.  CT: 16-cout tiles (Cout_pad = 16 * CT), NCH: 32-channel chunks of cat[src1, src2].
template <int CT, int NCH>
struct TileGeom {
    static constexpr int NWAVE = 4, ROWS = 32;                         // positions per wave tile (two MFMA column tiles)
    static constexpr int COUT = CT * 16;
    static constexpr int WBYTES = (CT / 2) * NCH * 2048;               // packed weight image: [32-cout group][chunk][32 rows x 64 B], pre-swizzled
    static constexpr int XBYTES = NCH * ROWS * 64;                     // activation tile: [chunk][row][64 B], 16-byte slots swizzled by swz64
    static constexpr int ORS = COUT * 2 + 16;                          // output row stride: +16 B keeps the 8-byte accumulator-layout writes off one bank
    static constexpr int OBYTES = ROWS * ORS;
    static constexpr int STAGE = XBYTES > OBYTES ? XBYTES : OBYTES;    // one wave's stage: the activation tile, then (tile dead) the output tile
    static constexpr int S0 = WBYTES;                                  // stages follow the weights
    static constexpr int LDSB = S0 + NWAVE * STAGE;
    static constexpr int XLOADS = 2 * NCH;                             // 16-byte loads per lane and tile: ROWS * NCH * 4 pieces over 64 lanes
    static constexpr int OSTORES = CT;                                 // 16-byte stores per lane and tile: ROWS * COUT / 8 pieces over 64 lanes
    static_assert(CT % 2 == 0 && COUT <= 128, "whole 32-cout groups of the packed weight");
    static_assert(S0 % 16 == 0 && STAGE % 16 == 0 && ORS % 16 == 0, "16-byte LDS accesses stay aligned");
    // last byte written by the activation staging: chunk NCH-1, row ROWS-1, slot 3
    static_assert((NCH - 1) * ROWS * 64 + (ROWS - 1) * 64 + 3 * 16 + 16 <= STAGE, "activation tile inside the stage");
    // last byte written by the output staging: row ROWS-1, cout tile CT-1, quad 3 (8 bytes); last 16-byte piece read back
    static_assert((ROWS - 1) * ORS + ((CT - 1) * 16 + 3 * 4) * 2 + 8 <= STAGE, "output tile inside the stage");
    static_assert((ROWS - 1) * ORS + (COUT / 8 - 1) * 16 + 16 <= STAGE, "output pieces inside the stage");
    // last byte read as a weight fragment: group CT/2-1, chunk NCH-1, row 31, slot 3
    static_assert(((CT / 2 - 1) * NCH + NCH - 1) * 2048 + 31 * 64 + 3 * 16 + 16 <= WBYTES, "weight fragments inside the image");
    static_assert(ROWS * NCH * 4 == XLOADS * 64 && ROWS * (COUT / 8) == OSTORES * 64, "pieces divide evenly over the lanes");
    static_assert(LDSB <= 160 * 1024, "fits the CU's LDS");
    static constexpr int PER_CU = 2 * LDSB <= 160 * 1024 ? 2 : 1;      // resident workgroups per CU: the register budget follows the LDS
};

// LDS accesses of ONE wave to its private stage need no barrier (in-order LDS pipeline); the compiler must still not move them across
// each other (the staging writes and the fragment reads use different vector types)
__device__ __forceinline__ void tile_wave_lds_fence()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

template <int CT, int NCH>
__global__ __launch_bounds__(256, (TileGeom<CT, NCH>::PER_CU)) void conv_tile1x1_kernel(const ConvParams p)
{
    using G = TileGeom<CT, NCH>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    // ---- resident weights: the packed image as it is
    for (int i = tid; i < G::WBYTES / 16; i += 256)
        *reinterpret_cast<u32x4 *>(smem + i * 16) = *reinterpret_cast<const u32x4 *>(p.weight + (long long)i * 8);
    __syncthreads();

    char *st = smem + G::S0 + wave * G::STAGE;
    const long long ntiles = (p.M + G::ROWS - 1) / G::ROWS;
    const long long tstep = (long long)gridDim.x * G::NWAVE;
    const int n1 = 2 * p.nchunk1;                                       // loads per lane that belong to the first source
    const int sh1 = 31 - __builtin_clz((unsigned)p.C1 >> 3);            // log2 of the 16-byte pieces per row (host: power-of-two channel counts)
    const int sh2 = p.C2 ? 31 - __builtin_clz((unsigned)p.C2 >> 3) : 0;
    const unsigned osp = (unsigned)(p.Do * p.Ho * p.Wo);

    // piece j of a lane: (source, row, 16-byte piece of the row); rows >= valid are zero (never stored, but they feed MFMA columns)
    u32x4 xr[G::XLOADS];
    auto load_tile = [&](long long t) {
        const long long m0 = t * G::ROWS;
        const int valid = (int)(p.M - m0 < G::ROWS ? p.M - m0 : G::ROWS);
        const bf16_t *b1 = p.src1 + m0 * p.C1;
        const bf16_t *b2 = p.src2 ? p.src2 + m0 * p.C2 : nullptr;
#pragma unroll
        for (int j = 0; j < G::XLOADS; ++j) {
            const bool first = j < n1;
            const int i = lane + 64 * (first ? j : j - n1);
            const int row = i >> (first ? sh1 : sh2);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < valid) v = *reinterpret_cast<const u32x4 *>((first ? b1 : b2) + i * 8);
            xr[j] = v;
        }
    };
    auto stage_tile = [&]() {
#pragma unroll
        for (int j = 0; j < G::XLOADS; ++j) {
            const bool first = j < n1;
            const int i = lane + 64 * (first ? j : j - n1);
            const int sh = first ? sh1 : sh2;
            const int row = i >> sh, pc = i & ((1 << sh) - 1);
            const int chunk = (first ? 0 : p.nchunk1) + (pc >> 2);
            *reinterpret_cast<u32x4 *>(st + chunk * (G::ROWS * 64) + row * 64 + swz64(row, pc & 3) * 16) = xr[j];
        }
    };

    long long t = (long long)blockIdx.x * G::NWAVE + wave;
    if (t < ntiles) load_tile(t);
    for (; t < ntiles; t += tstep) {
        const long long m0 = t * G::ROWS;
        const int valid = (int)(p.M - m0 < G::ROWS ? p.M - m0 : G::ROWS);
        stage_tile();
        tile_wave_lds_fence();
        // bias rows of this tile, requested in front of the next tile's loads: the memory counter is in order, so the epilogue waits
        // for nothing younger than these
        f32x4 bv[2][CT];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const long long m = m0 + pt * 16 + fr;
            const long long mc = m < p.M ? m : p.M - 1;
            const float *brow = p.bias ? p.bias + (long long)((unsigned)mc / osp) * p.bias_stride : nullptr;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                bv[pt][ct] = brow ? *reinterpret_cast<const f32x4 *>(brow + ct * 16 + fq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (t + tstep < ntiles) load_tile(t + tstep);

        f32x4 acc[2][CT];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NCH; ++c) {                                  // chunks ascending: the gather kernel's k-step order (one tap)
            bf16x8 xf[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const int r = pt * 16 + fr;
                xf[pt] = *reinterpret_cast<const bf16x8 *>(st + c * (G::ROWS * 64) + r * 64 + swz64(r, fq) * 16);
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int r = (ct & 1) * 16 + fr;
                const bf16x8 wf = *reinterpret_cast<const bf16x8 *>(smem + ((ct >> 1) * NCH + c) * 2048 + r * 64 + swz64(r, fq) * 16);
#pragma unroll
                for (int pt = 0; pt < 2; ++pt)
                    acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[pt], acc[pt][ct], 0, 0, 0);
            }
        }
        tile_wave_lds_fence();                                           // the activation tile is dead: the stage becomes the output tile

        // ---- epilogue: the gather kernel's expression, then rows of COUT bf16 in LDS -> full-line stores
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int r = pt * 16 + fr;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int co = ct * 16 + fq * 4;
                const f32x4 v = gg_conv_epi_value(acc[pt][ct], p.bias != nullptr, bv[pt][ct], false, bf16x4{}, co, p.Cout);
                *reinterpret_cast<bf16x4 *>(st + r * G::ORS + co * 2) = gg_conv_epi_bf16(v);
            }
        }
        tile_wave_lds_fence();
        bf16_t *ob = (bf16_t *)p.out + m0 * G::COUT;
#pragma unroll
        for (int j = 0; j < G::OSTORES; ++j) {
            const int i = lane + 64 * j;
            const int row = i / (G::COUT / 8), pc = i % (G::COUT / 8);
            const u32x4 v = *reinterpret_cast<const u32x4 *>(st + row * G::ORS + pc * 16);
            if (row < valid) *reinterpret_cast<u32x4 *>(ob + i * 8) = v;          // every row < M is stored in full (the output is torch.empty)
        }
        tile_wave_lds_fence();                                           // the next tile's staging overwrites the output tile
    }
}

// ------------------------------------------------------------------------------------------ host
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// (CT, NCH) pairs that are instantiated: the CCDM skip projections 64+64 -> 64, 128+64 -> 64, 64 -> 128, 128+64 -> 128, 128+128 -> 128
static bool tile_instantiated(int CT, int NCH)
{
    return (CT == 4 && (NCH == 4 || NCH == 6)) || (CT == 8 && (NCH == 2 || NCH == 6 || NCH == 8));
}

int gg_conv_tile_family(const ConvParams &p)
{
    if (!GG_TILE_CONV || p.path_hint == GG_CONV_HINT_GATHER) return 0;
    if (p.kd != 1 || p.kh != 1 || p.kw != 1 || p.stride != 1 || p.upsample) return 0;
    if (p.Do != p.D || p.Ho != p.H || p.Wo != p.W) return 0;
    if (p.prologue_act || p.residual || p.out_dtype != GG_BF16 || p.epi_geglu || p.post_xt || p.ddim_x || p.skip_C1) return 0;
    if (p.Cout_pad != 64 && p.Cout_pad != 128) return 0;
    if (!pow2(p.C1) || p.C1 < 32 || (p.C2 && (!pow2(p.C2) || p.C2 < 32))) return 0;      // a row's 16-byte pieces decode with a shift
    if (!tile_instantiated(p.Cout_pad / 16, p.nchunk)) return 0;
    if (p.M < GG_TILE_MIN_M) return 0;
    return 1;
}

template <int CT, int NCH>
static int launch_tile1x1(const ConvParams &p, hipStream_t stream)
{
    using G = TileGeom<CT, NCH>;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return GG_ERR_HIP;
    static std::atomic<unsigned long long> attr_mask{0};
    const unsigned long long dev_bit = 1ull << (dev & 63);
    if (!(attr_mask.load(std::memory_order_acquire) & dev_bit)) {
        if (hipFuncSetAttribute((const void *)conv_tile1x1_kernel<CT, NCH>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDSB) != hipSuccess) return GG_ERR_UNSUPPORTED;
        attr_mask.fetch_or(dev_bit, std::memory_order_release);
    }
    // persistent waves: as many workgroups as stay resident (LDS; two by registers), each wave walking tiles with a grid stride
    const int per_cu = G::PER_CU;
    const long long ntiles = (p.M + G::ROWS - 1) / G::ROWS;
    long long blocks = (ntiles + G::NWAVE - 1) / G::NWAVE;
    if (blocks > (long long)cus * per_cu) blocks = (long long)cus * per_cu;
    hipLaunchKernelGGL((conv_tile1x1_kernel<CT, NCH>), dim3((unsigned)blocks), dim3(256), G::LDSB, stream, p);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

int gg_conv_tile_try(const ConvParams &p, hipStream_t stream)
{
    if (gg_conv_tile_family(p) != 1) return GG_ERR_UNSUPPORTED;
    if (stream == (hipStream_t)-1) return GG_OK;
    const int CT = p.Cout_pad / 16;
    if (CT == 4 && p.nchunk == 4) return launch_tile1x1<4, 4>(p, stream);
    if (CT == 4 && p.nchunk == 6) return launch_tile1x1<4, 6>(p, stream);
    if (CT == 8 && p.nchunk == 2) return launch_tile1x1<8, 2>(p, stream);
    if (CT == 8 && p.nchunk == 6) return launch_tile1x1<8, 6>(p, stream);
    if (CT == 8 && p.nchunk == 8) return launch_tile1x1<8, 8>(p, stream);
    return GG_ERR_UNSUPPORTED;
}
