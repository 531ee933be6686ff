// CCDM reverse step of ONE voxel (shared by the stand-alone sampler kernel in gg_sampler.hip and by the fused epilogue of the UNet head
// conv in gg_conv_halo.hip): softmax of the head's logits, posterior q(x_{t-1} | x_t, x_0) summed over the predicted x_0, clamp,
// normalise, exponential race (or argmax).  The arithmetic is, expression for expression and in the same left-to-right fp32 order (no FMA
// contraction, IEEE division), the C restatement oracle/ccdm_posterior.c, so the labels agree bit-for-bit when probabilities (not
// logits) are fed -- and both callers produce the SAME label from the same fp32 logits.
#pragma once
#include "gg_common.h"

// ------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (counter-based): counter = (voxel lo, voxel hi, draw index, step offset), key = seed.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// One Philox word -> one Exp(1) draw: the top 24 bits + 1 scaled by 2^-24 is a uniform in (0, 1] that fp32 holds exactly, the hardware
// logarithm of it is <= 0 (0 at u == 1), and the 1e-30f keeps the divisor of the race positive.
__device__ __forceinline__ float ccdm_word_to_exp(const uint32_t w)
{
    const float uu = (float)((w >> 8) + 1u) * 5.9604644775390625e-8f;   // (0, 1]
    return -__logf(uu) + 1e-30f;
}

// The KMAX exponentials of one row: call q4 draws with counter (row lo, row hi, q4, low 32 bits of the step offset) and key (seed lo,
// seed hi), and its four words are the classes 4 * q4 .. 4 * q4 + 3.  This is THE draw of the CCDM kernels: the reverse step here, the fused
// head-conv epilogue (through ccdm_posterior_voxel), gg_ccdm_q_sample and gg_ccdm_draw_tape all call it.  words: the raw words out, or
// nullptr.
template <int KMAX>
__device__ __forceinline__ void ccdm_draw_row(float (&Ev)[KMAX], const uint64_t key, const long long row, const long long off,
                                              uint32_t *__restrict__ words = nullptr)
{
#pragma unroll
    for (int q4 = 0; q4 < KMAX / 4; ++q4) {
        uint32_t ctr[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)q4, (uint32_t)off};
        philox4x32_10(ctr, (uint32_t)key, (uint32_t)(key >> 32));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (words) words[q4 * 4 + j] = ctr[j];
            Ev[q4 * 4 + j] = ccdm_word_to_exp(ctr[j]);
        }
    }
}

// The key / counter rule of a draw.  PS == 0 (single key): key `seed`, counter the row m.  PS == 1 (per-sample keys): row m belongs to sample
// n = m / rows_per_sample and draws with key seeds[n] and counter m - n * rows_per_sample, so that a sample's labels do not depend on its
// slot in the batch.  (The fused head-conv epilogue in gg_conv_halo.hip keeps a uniform form of its own: a box lies in one sample, so it
// loads the key once per box.)
template <int PS>
__device__ __forceinline__ void ccdm_key_row(const uint64_t seed, const unsigned long long *__restrict__ seeds, const long long rows_per_sample,
                                             const long long m, uint64_t &key, long long &row)
{
    key = seed;
    row = m;
    if constexpr (PS) {
        const long long n = m / rows_per_sample;
        key = seeds[n];
        row = m - n * rows_per_sample;
    }
}

// KS > 0: the class count as a compile-time constant (K must equal it): no per-class bound checks (they are scalar branches, ~500 per voxel
// with a run-time K); KS == 0: run-time K <= KMAX.  Every helper below that loops over the classes takes the pair.

// The K exponentials of a row: E_row, K values of a tape (1.f beyond K), or nullptr: Philox draws them (ccdm_draw_row).
template <int KMAX, int KS = 0>
__device__ __forceinline__ void ccdm_exp_row(float (&Ev)[KMAX], const float *__restrict__ E_row, const int K_rt, const uint64_t key, const long long row,
                                             const long long off)
{
#pragma clang fp contract(off)
    const int K = KS > 0 ? KS : K_rt;
    if (E_row) {
#pragma unroll
        for (int c = 0; c < KMAX; ++c) Ev[c] = (c < K) ? E_row[c] : 1.f;
    } else {
        ccdm_draw_row<KMAX>(Ev, key, row, off);
    }
}

// nn.Softmax(dim=1) of the UNet head, fp32, in place
template <int KMAX, int KS = 0>
__device__ __forceinline__ void ccdm_softmax(float (&p)[KMAX], const int K_rt)
{
#pragma clang fp contract(off)
    const int K = KS > 0 ? KS : K_rt;
    float mx = p[0];
#pragma unroll
    for (int c = 1; c < KMAX; ++c) if (c < K) mx = fmaxf(mx, p[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) { p[c] = expf(p[c] - mx); s = s + p[c]; }
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) p[c] = p[c] / s;
}

// q(x_{t-1} = c | x_t = x, x_0 = d) = A[c] B[c][d] / den[d] with A[c] = a [c == x] + u and B[c][d] = abar [c == d] + v: A takes TWO
// values (c == x or not) and B two (c == d or not), so the numerators of the whole K x K table are four fp32 products.
struct ccdm_numer { float xd, xo, od, oo; };

__device__ __forceinline__ ccdm_numer ccdm_numerators(const float a, const float abar, const int K)
{
#pragma clang fp contract(off)
    const float Kf = (float)K;
    const float u = (1.0f - a) / Kf;
    const float v = (1.0f - abar) / Kf;
    const float bd = abar * 1.0f + v;
    const float bo = abar * 0.0f + v;
    const float Ax = a * 1.0f + u, Ao = a * 0.0f + u;
    return ccdm_numer{Ax * bd, Ax * bo, Ao * bd, Ao * bo};
}

// the numerator of (c, x, d)
__device__ __forceinline__ float ccdm_numer_of(const ccdm_numer &nm, const int c, const int x, const int d)
{
    return (c == x) ? (c == d ? nm.xd : nm.xo) : (c == d ? nm.od : nm.oo);
}

// The posterior summed over the predicted x_0: out[c] = sum_d q(c | x, d) p[d], c and d in [0, K).  The K numerators of a column d are three
// distinct fp32 products and the K IEEE divisions three -- the same operands, hence the same bits, as dividing every entry (42 divisions
// per voxel instead of 196: the kernel is VALU-bound, 4.7 k -> 2.9 k instructions per voxel).  The sums keep the restatement's
// left-to-right order.  A macro for a function body that has KMAX in scope and contraction off, because every function form tried
// changed the schedule of ccdm_posterior_voxel's callers with K = 14 compiled in (85 VGPRs as text in place, 111 to 258
// as a function over array references, over a callable or returning the row; the head-conv epilogue 120 against 167 to 238).
#define CCDM_POSTERIOR_SUM(out, p, nm, x, K)                                                                                  \
    _Pragma("unroll") for (int c_ = 0; c_ < KMAX; ++c_) (out)[c_] = 0.f;                                                        \
    _Pragma("unroll") for (int d_ = 0; d_ < KMAX; ++d_) {                                                                       \
        if (d_ < (K)) {                                                                                                       \
            float den_ = 0.f;                                                                                                 \
            _Pragma("unroll") for (int c_ = 0; c_ < KMAX; ++c_) if (c_ < (K)) den_ = den_ + ccdm_numer_of(nm, c_, x, d_);       \
            const float pd_ = (p)[d_];                                                                                        \
            const float q_dd_ = ((d_ == (x)) ? (nm).xd : (nm).od) / den_, q_xo_ = (nm).xo / den_, q_oo_ = (nm).oo / den_;     \
            _Pragma("unroll") for (int c_ = 0; c_ < KMAX; ++c_) if (c_ < (K)) {                                                 \
                const float post_ = (c_ == d_) ? q_dd_ : ((c_ == (x)) ? q_xo_ : q_oo_);                                       \
                (out)[c_] = (out)[c_] + post_ * pd_;                                                                          \
            }                                                                                                                 \
        }                                                                                                                     \
    }

// The exponential race over the weights w of sum s: pn = w[c] / s, and the first maximum of pn / Ev[c] wins (use_race == false: of pn, the
// argmax).  probs_row: the K values pn out, or nullptr.
template <int KMAX, int KS = 0>
__device__ __forceinline__ int ccdm_race(const float (&w)[KMAX], const float s, const bool use_race, const float (&Ev)[KMAX], const int K_rt,
                                         float *__restrict__ probs_row)
{
#pragma clang fp contract(off)
    const int K = KS > 0 ? KS : K_rt;
    int best = 0;
    float bestv = -1.0f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) {
        const float pn = w[c] / s;
        const float r = use_race ? pn / Ev[c] : pn;
        if (probs_row) probs_row[c] = pn;
        if (r > bestv) { bestv = r; best = c; }
    }
    return best;
}

// Reverse step.  p0: the head's K values of the voxel (logits or probabilities), overwritten; x: the voxel's current label; a / abar: the
// step's scalars (alpha_t, cumulative alpha of t - 1); E_row, seed (the key), m (the counter row), off: ccdm_exp_row's; probs_row:
// ccdm_race's.  Returns the new label.
template <int KMAX, int KS = 0>
__device__ __forceinline__ int ccdm_posterior_voxel(float (&p0)[KMAX], const int is_logits, const int x, const float a, const float abar, const int K_rt,
                                                    const long long m, const int draw, const float *__restrict__ E_row, const uint64_t seed,
                                                    const long long off, float *__restrict__ probs_row)
{
#pragma clang fp contract(off)
    const int K = KS > 0 ? KS : K_rt;
    if (is_logits) ccdm_softmax<KMAX, KS>(p0, K);
    const ccdm_numer nm = ccdm_numerators(a, abar, K);
    float out[KMAX];
    CCDM_POSTERIOR_SUM(out, p0, nm, x, K)
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) {
        if (out[c] < 1e-12f) out[c] = 1e-12f;
        s = s + out[c];
    }
    float Ev[KMAX];
    const bool use_race = draw != 0;
    if (use_race) ccdm_exp_row<KMAX, KS>(Ev, E_row, K, seed, m, off);
    return ccdm_race<KMAX, KS>(out, s, use_race, Ev, K, probs_row);
}

// q_xt_given_x0(x0 = lab, t).sample(): the weights ca [c == lab] + cb / K, their left-to-right sum, the race against Ev.
template <int KMAX>
__device__ __forceinline__ int ccdm_q_sample_voxel(const int lab, const float ca, const float cb, const int K, const float (&Ev)[KMAX])
{
#pragma clang fp contract(off)
    const float v = cb / (float)K;
    const float pd = ca * 1.0f + v, po = ca * 0.0f + v;
    float w[KMAX];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) { w[c] = (c == lab ? pd : po); s = s + w[c]; }
    return ccdm_race<KMAX>(w, s, true, Ev, K, nullptr);
}

// channels [0, K) of the voxel's one-hot row as 4-byte pairs (+ one 2-byte tail for odd K): 7 stores instead of 14 two-byte ones at K = 14
// (two-byte stores cost ~12x a 16-byte store per byte on this memory system, MI355X_MICROARCH.md); channel K and beyond (the
// condition image, the padding lanes) are NOT touched
template <int KMAX, int KS = 0>
__device__ __forceinline__ void ccdm_onehot_row(bf16_t *__restrict__ oh, const int best, const int K_rt)
{
    const int K = KS > 0 ? KS : K_rt;
#pragma unroll
    for (int c = 0; c + 1 < KMAX; c += 2) {
        if (c + 1 < K) {
            bf16x2 pr;
            pr[0] = (bf16_t)(c == best ? 1.0f : 0.0f);
            pr[1] = (bf16_t)(c + 1 == best ? 1.0f : 0.0f);
            *reinterpret_cast<bf16x2 *>(oh + c) = pr;
        } else if (c < K) {
            oh[c] = (bf16_t)(c == best ? 1.0f : 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// CCDM training objective of ONE voxel (ccdm/ddpm/trainer.py:305-320), forward only.  lg: the head's K fp32 logits, overwritten with
// p = softmax(lg) (the model's diffusion_out).  kl_out = class_weight * sum_c kl_div(log(max(theta_post_prob(xt, p), 1e-12)),
// theta_post(xt, x0)): the predicted posterior is clamped and NOT renormalised there, and a zero target contributes zero (xlogy; t == 1
// makes theta_post one-hot).  ce_out = cross_entropy(p, x0) on the PROBABILITIES, as the trainer feeds them (log_softmax in ATen's
// form: p - max - log(sum(exp(p - max)))).  The softmax and the unnormalised posterior are those of ccdm_posterior_voxel.
// ------------------------------------------------------------------------------------------------------------
template <int KMAX>
__device__ __forceinline__ void ccdm_loss_voxel(float (&lg)[KMAX], const int x, const int x0, const float a, const float abar, const int K,
                                                const float cw, float &kl_out, float &ce_out)
{
#pragma clang fp contract(off)
    ccdm_softmax<KMAX>(lg, K);
    const ccdm_numer nm = ccdm_numerators(a, abar, K);
    float qp[KMAX];
    CCDM_POSTERIOR_SUM(qp, lg, nm, x, K)
    // theta_post(xt, x0): the column d == x0 of the table, normalised
    float den0 = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) den0 = den0 + ccdm_numer_of(nm, c, x, x0);
    float kl = 0.f, pmx = lg[0], px0 = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) {
        const float qt = ccdm_numer_of(nm, c, x, x0) / den0;
        const float lq = logf(fmaxf(qp[c], 1e-12f));
        const float ent = qt > 0.f ? qt * logf(qt) : 0.f;
        kl = kl + (ent - qt * lq);
        pmx = fmaxf(pmx, lg[c]);
        if (c == x0) px0 = lg[c];
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) if (c < K) se = se + expf(lg[c] - pmx);
    kl_out = kl * cw;
    ce_out = -((px0 - pmx) - logf(se));
}

// ------------------------------------------------------------------------------------------------------------
// Host side: what the CCDM entries test before a launch of one row per thread, under the entry's own name: at least min_rows rows that
// split into samples of rows_per_sample (1: no split), one-hot rows of K channels or more that ccdm_onehot_row's 4-byte stores may
// write (onehot_out nullptr: none), a grid of 256-thread workgroups.
// ------------------------------------------------------------------------------------------------------------
static inline int ccdm_check_rows(const char *entry, long long M, long long min_rows, long long rows_per_sample, int K, const void *onehot_out,
                                  int onehot_stride)
{
    if (M < min_rows || rows_per_sample < 1 || M % rows_per_sample)
        GG_FAIL(GG_ERR_BAD_SHAPE, "%s: M=%lld is not a multiple of rows_per_sample=%lld", entry, M, rows_per_sample);
    if (onehot_out && onehot_stride < K) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: onehot_stride < K", entry);
    if (onehot_out && ((onehot_stride & 1) || ((uintptr_t)onehot_out & 3))) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: onehot rows must be 4-byte aligned (even stride)", entry);
    if ((M + 255) / 256 > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "%s: M=%lld voxels exceed the grid", entry, M);
    return GG_OK;
}

