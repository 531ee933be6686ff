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

int gg_conv_tile_try(const ConvParams &p, hipStream_t stream, bool launch)
{
    if (gg_conv_tile_family(p) != 1) return GG_ERR_UNSUPPORTED;
    if (!launch) return GG_OK;
    const int CT = p.Cout_pad / 16;
    if (CT == 4 && p.nchunk == 4) return launch_tile1x1<4, 4>(p, stream);
    if (CT == 4 && p.nchunk == 6) return launch_tile1x1<4, 6>(p, stream);
    if (CT == 8 && p.nchunk == 2) return launch_tile1x1<8, 2>(p, stream);
    if (CT == 8 && p.nchunk == 6) return launch_tile1x1<8, 6>(p, stream);
    if (CT == 8 && p.nchunk == 8) return launch_tile1x1<8, 8>(p, stream);
    return GG_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------ stride-2 3x3x3 tile conv
// The 128-cout Downsample conv of the CCDM UNet (128 -> 128 @64^3 -> 32^3), byte-identical to conv_gather_kernel without a K split.
// (64 couts -- 64 -> 64 @128^3 -> 64^3 -- were measured a tie, 172 us on both kernels: 64-byte slices of 128-byte rows, fetched twice;
// that width is not instantiated.)  One workgroup owns a 2x4x16 output tile and all couts.  Per 32-channel chunk the 5x9x33 input
// rows that the tile's 27 taps touch are staged ONCE (all of a thread's pieces in flight together); the columns of a W-line are stored
// de-interleaved by parity (17 even columns, then 16 odd ones), so that the 16 lanes of an operand read (outputs ow .. ow + 15 of tap kw:
// input columns 2 ow + kw) take 16 CONSECUTIVE rows and swz64 keeps them conflict-free as in the gather kernel.  The three kw taps of a
// (kd, kh) line share one weight round (global_load_lds into a double-buffered slot, as in conv_halo_kernel) and one barrier.
// Bit-identity: chunk-outer, (kd, kh, kw)-inner from a zero accumulator, v_mfma_f32_16x16x32_bf16 with A = weights, zero rows for the
// padding, then gg_conv_epi_value / gg_conv_epi_bf16: what conv_gather_kernel computes for splitk == 1.  No GroupNorm sums, as there.
#ifndef GG_TILE_S2
#define GG_TILE_S2 1          /* A/B switch: 0 = the stride-2 tile kernel declines everything (the gather kernel runs, as before) */
#endif

template <int NT>
struct TileS2Geom {
    static constexpr int TD = 2, TH = 4, TW = 16;                               // output tile
    static constexpr int ID = 2 * TD + 1, IH = 2 * TH + 1, IW = 2 * TW + 1;    // input box: 5 x 9 x 33 rows of 64 B
    static constexpr int WE = TW + 1;                                          // even columns of a W-line (17) come first, then the odd ones (16)
    static constexpr int NROWS = ID * IH * IW;
    static constexpr int XBYTES = ((NROWS * 64 + 1023) / 1024) * 1024;
    static constexpr int WBYTES = NT * 2048;                                   // one tap: 32 NT cout rows x 64 B
    static constexpr int LDSB = XBYTES + 2 * 3 * WBYTES;                       // the box image, then two slots of three taps
    // eight waves, one W-row of 16 outputs each: with four (two rows each) a lone wave per SIMD issued the staging and operand-address
    // instructions of a chunk at ~6 ticks each (128 -> 128 @64^3: 69 us; with eight 59 us; the gather kernel 89 us)
    static constexpr int NTHR = 512, NWAVE = 8, TPW = TD * TH / NWAVE;
    static constexpr int JMAX = (NROWS * 4 + NTHR - 1) / NTHR;                 // 16-byte pieces per thread and chunk
    static_assert(TD * TH == NWAVE * TPW, "every wave owns the same number of position tiles");
    static_assert(LDSB <= 160 * 1024, "box image + weight slots exceed the LDS of a CU");
    // last operand row: input line (2 (TD - 1) + 2, 2 (TH - 1) + 2), tap kw 1 (odd columns), lane 15
    static_assert(((ID - 1) * IH + IH - 1) * IW + WE + TW - 1 < NROWS && 1 + TW - 1 < WE, "operand rows inside the box image");
    static_assert((2 * 3 - 1) * WBYTES + (NT * 2 - 1) * 1024 + 1024 <= 2 * 3 * WBYTES, "weight pieces inside the slots");
};

template <int NT>
__global__ __launch_bounds__((TileS2Geom<NT>::NTHR), 1) void conv_tile_s2_kernel(const ConvParams p, const int tiles_d, const int tiles_h, const int tiles_w)
{
    using G = TileS2Geom<NT>;
    constexpr int IH = G::IH, IW = G::IW, WE = G::WE, NROWS = G::NROWS, WBYTES = G::WBYTES, TPW = G::TPW, JMAX = G::JMAX;
    extern __shared__ __attribute__((aligned(1024))) char smem[];      // G::LDSB bytes
    char *xs = smem, *wsm = smem + G::XBYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    int t = blockIdx.x;
    const int tw = t % tiles_w; t /= tiles_w;
    const int th = t % tiles_h; t /= tiles_h;
    const int td = t % tiles_d;
    const int n = t / tiles_d;
    const int od0 = td * G::TD, oh0 = th * G::TH, ow0 = tw * G::TW;          // output-tile origin
    const int id0 = 2 * od0 - 1, ih0 = 2 * oh0 - 1, iw0 = 2 * ow0 - 1;       // input coordinates of box row (0, 0, 0)
    const int xq = tid & 3;

    // weight round of line gl = chunk * 9 + (kd * 3 + kh): its three kw taps, NT contiguous 2 KiB groups each, strided by 27 * nchunk * 2 KiB
    auto issue_w = [&](int gl, int buf) {
        const int chunk = gl / 9, tap0 = (gl - chunk * 9) * 3;
        constexpr int NP = 3 * NT * 2;                  // 1 KiB pieces of the slot
#pragma unroll
        for (int i = 0; i < (NP + G::NWAVE - 1) / G::NWAVE; ++i) {
            const int piece = wave + G::NWAVE * i;
            if (piece < NP) {
                const int u = piece / (NT * 2), piece1k = piece - u * (NT * 2);
                const int g = piece1k >> 1, half = piece1k & 1;
                const bf16_t *src = p.weight + ((((long long)g * 27 + tap0 + u) * p.nchunk + chunk) << 10) + half * 512 + lane * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(wsm + (buf * 3 + u) * WBYTES + piece1k * 1024), 16, 0, 0);
            }
        }
    };

    f32x4 acc[TPW][2 * NT];
#pragma unroll
    for (int a = 0; a < TPW; ++a)
#pragma unroll
        for (int b = 0; b < 2 * NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int KL = p.nchunk * 9;
    issue_w(0, 0);
    for (int chunk = 0; chunk < p.nchunk; ++chunk) {
        // ================= stage the input box of this chunk: every piece of the thread requested before the first is written =================
        {
            const bool second = chunk >= p.nchunk1;
            const bf16_t *src = second ? p.src2 : p.src1;
            const int Cs = second ? p.C2 : p.C1;
            const int coff = (second ? chunk - p.nchunk1 : chunk) * 32 + xq * 8;
            const bf16_t *srcn = src + (long long)n * p.D * p.H * p.W * Cs + coff;
            u32x4 v[JMAX];
            int lrow[JMAX];                 // LDS row of the piece; -1: beyond the box (last round); bit 30: padding (stored as zeros)
#pragma unroll
            for (int j = 0; j < JMAX; ++j) {
                const int row = (tid >> 2) + (G::NTHR / 4) * j;          // box rows in input order (hd, hh, column): a W-line is one contiguous run
                const int hd = row / (IH * IW), rem = row - hd * (IH * IW), hh = rem / IW, iwl = rem - hh * IW;
                const int id = id0 + hd, ih = ih0 + hh, iw = iw0 + iwl;
                const bool in = row < NROWS;
                const bool ok = in && (unsigned)id < (unsigned)p.D && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                const unsigned pos = ok ? (unsigned)((id * p.H + ih) * p.W + iw) : 0u;      // (padding: a valid address, the value is dropped)
                v[j] = *reinterpret_cast<const u32x4 *>(srcn + pos * (unsigned)Cs);
                lrow[j] = in ? (((hd * IH + hh) * IW + (iwl & 1) * WE + (iwl >> 1)) | (ok ? 0 : (1 << 30))) : -1;
            }
#pragma unroll
            for (int j = 0; j < JMAX; ++j) {
                if (lrow[j] >= 0) {
                    const int lr = lrow[j] & ~(1 << 30);
                    const u32x4 val = (lrow[j] >> 30) ? u32x4{0u, 0u, 0u, 0u} : v[j];
                    *reinterpret_cast<u32x4 *>(xs + lr * 64 + swz64(lr, xq) * 16) = val;
                }
            }
        }
        __syncthreads();          // box visible; the first weight round of the chunk has landed too

#pragma unroll 1
        for (int kd = 0; kd < 3; ++kd) {
#pragma unroll 1
            for (int kh = 0; kh < 3; ++kh) {
                const int gl = chunk * 9 + kd * 3 + kh;
                if (gl + 1 < KL) issue_w(gl + 1, (gl + 1) & 1);
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const char *wb = wsm + ((gl & 1) * 3 + kw) * WBYTES;
                    bf16x8 xf[TPW];
#pragma unroll
                    for (int tt = 0; tt < TPW; ++tt) {
                        const int tile = wave * TPW + tt, od = tile / G::TH, oh = tile % G::TH;
                        const int row = ((2 * od + kd) * IH + 2 * oh + kh) * IW + (kw == 1 ? WE : 0) + (kw == 2 ? 1 : 0) + fr;
                        xf[tt] = *reinterpret_cast<const bf16x8 *>(xs + row * 64 + swz64(row, fq) * 16);
                    }
#pragma unroll
                    for (int ct = 0; ct < 2 * NT; ++ct) {
                        const int r = ct * 16 + fr;
                        const bf16x8 wf = *reinterpret_cast<const bf16x8 *>(wb + r * 64 + swz64(r, fq) * 16);   // image pre-swizzled at pack time
#pragma unroll
                        for (int tt = 0; tt < TPW; ++tt)
                            acc[tt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[tt], acc[tt][ct], 0, 0, 0);
                    }
                }
                __syncthreads();       // next line's weights landed; this line's slot / (after the last line) the box may be overwritten
            }
        }
    }

    // ================= epilogue: the gather kernel's; every bias / residual load in front of the first store =================
    const float *brow = p.bias ? p.bias + (long long)n * p.bias_stride : nullptr;
    f32x4 bv[2 * NT];
    bf16x4 resv[TPW][2 * NT];
    long long ob[TPW];
#pragma unroll
    for (int ct = 0; ct < 2 * NT; ++ct) bv[ct] = brow ? *reinterpret_cast<const f32x4 *>(brow + ct * 16 + fq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) {
        const int tile = wave * TPW + tt, od = tile / G::TH, oh = tile % G::TH;
        const long long m = (((long long)n * p.Do + (od0 + od)) * p.Ho + (oh0 + oh)) * p.Wo + (ow0 + fr);
        ob[tt] = m * p.Cout_pad + fq * 4;
#pragma unroll
        for (int ct = 0; ct < 2 * NT; ++ct)
            if (p.residual) resv[tt][ct] = *reinterpret_cast<const bf16x4 *>(p.residual + ob[tt] + ct * 16);
    }
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt)
#pragma unroll
        for (int ct = 0; ct < 2 * NT; ++ct) {
            const f32x4 val = gg_conv_epi_value(acc[tt][ct], p.bias != nullptr, bv[ct], p.residual != nullptr, resv[tt][ct], ct * 16 + fq * 4, p.Cout);
            const long long o = ob[tt] + ct * 16;
            if (p.out_dtype == GG_F32) *reinterpret_cast<f32x4 *>((float *)p.out + o) = val;
            else *reinterpret_cast<bf16x4 *>((bf16_t *)p.out + o) = gg_conv_epi_bf16(val);
        }
}

// shape envelope only; the caller (plan_tile_s2, gg_conv.hip) adds what the gather plan must say (no K split)
bool gg_conv_tile_s2_family(const ConvParams &p)
{
    using G = TileS2Geom<4>;
    if (!GG_TILE_S2 || p.path_hint == GG_CONV_HINT_GATHER || p.path_hint == GG_CONV_HINT_NO_TILE_S2 || !(gg_hint_is_production(p.path_hint) || p.path_hint == GG_CONV_HINT_TILE_S2)) return false;
    if (p.kd != 3 || p.kh != 3 || p.kw != 3 || p.stride != 2 || p.pad != 1 || p.upsample) return false;
    if (p.prologue_act || p.epi_geglu || p.post_xt || p.ddim_x || p.skip_C1) return false;
    if (p.D != 2 * p.Do || p.H != 2 * p.Ho || p.W != 2 * p.Wo) return false;
    if (p.Do % G::TD || p.Ho % G::TH || p.Wo % G::TW) return false;
    return p.Cout_pad == 128;
}

template <int NT>
static int launch_tile_s2(const ConvParams &p, hipStream_t stream)
{
    using G = TileS2Geom<NT>;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GG_ERR_HIP;
    static std::atomic<unsigned long long> attr_mask{0};
    const unsigned long long dev_bit = 1ull << (dev & 63);
    if (!(attr_mask.load(std::memory_order_acquire) & dev_bit)) {
        if (hipFuncSetAttribute((const void *)conv_tile_s2_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDSB) != hipSuccess) return GG_ERR_UNSUPPORTED;
        attr_mask.fetch_or(dev_bit, std::memory_order_release);
    }
    const int tiles_d = p.Do / G::TD, tiles_h = p.Ho / G::TH, tiles_w = p.Wo / G::TW;
    hipLaunchKernelGGL((conv_tile_s2_kernel<NT>), dim3((unsigned)(p.N * tiles_d * tiles_h * tiles_w)), dim3(G::NTHR), G::LDSB, stream, p, tiles_d, tiles_h, tiles_w);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

int gg_conv_tile_s2_launch(const ConvParams &p, hipStream_t stream)
{
    if (!gg_conv_tile_s2_family(p)) return GG_ERR_UNSUPPORTED;
    return launch_tile_s2<4>(p, stream);
}
