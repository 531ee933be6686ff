"""TEST INFRASTRUCTURE ONLY -- plain integer restatement of the CCDM kernels' Philox draw (csrc/gg_posterior.h: philox4x32_10,
ccdm_draw_row, ccdm_word_to_exp) and the inputs the GPU word tests run it on.

The draw.  Row `row` of a sample with the 64-bit key `seed` draws kmax / 4 blocks of Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are in test_philox_cpu.py).  Block q4 has

    counter = (row & 0xffffffff, row >> 32, q4, offset & 0xffffffff)        key = (seed & 0xffffffff, seed >> 32)

and its four output words are the classes 4 * q4 .. 4 * q4 + 3.  Single-key mode: row = m.  Per-sample mode: sample n = m //
rows_per_sample draws with seeds[n] and row = m - n * rows_per_sample.  A word w becomes u = ((w >> 8) + 1) * 2^-24 in (0, 1], which fp32
holds exactly, and E = -log(u) + 1e-30.

`fault` re-creates one defect of that text at a time, so that test_philox_cpu.py can show that the compared inputs see each of them."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the two key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)

FAULTS = ("wrong_multiplier", "key_words_swapped", "counter_words_2_3_swapped", "q4_from_1", "row_not_reduced", "offset_ignored")


def philox4x32_10(ctr, key, m0=M0, m1=M1):
    """ctr: four integer arrays (or ints) of one shape, key: two -> four uint32 arrays, the ten rounds written out on uint64."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for _ in range(10):
        p0 = np.uint64(m0) * c[0]            # 32 x 32 -> 64 bits: never wraps
        p1 = np.uint64(m1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def draw_words(M, kmax, seed=0, seeds=None, rows_per_sample=None, offset=None, fault=None):
    """uint32 [M, kmax]: the words gg_ccdm_draw_tape writes to bits_out (seeds given: the per-sample mode)."""
    assert kmax in (16, 32) and fault in (None,) + FAULTS
    m = np.arange(M, dtype=np.uint64)
    if seeds is None:
        key, row = np.full(M, int(seed) & (2 ** 64 - 1), dtype=np.uint64), m
    else:
        assert M % rows_per_sample == 0 and len(seeds) == M // rows_per_sample
        n = m // np.uint64(rows_per_sample)
        key = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)[n.astype(np.int64)]
        row = m if fault == "row_not_reduced" else m - n * np.uint64(rows_per_sample)
    off = 0 if (offset is None or fault == "offset_ignored") else int(offset) & 0xFFFFFFFF
    klo, khi = key & MASK, key >> np.uint64(32)
    if fault == "key_words_swapped":
        klo, khi = khi, klo
    out = np.empty((M, kmax), dtype=np.uint32)
    for q4 in range(kmax // 4):
        q = q4 + 1 if fault == "q4_from_1" else q4
        ctr = [row & MASK, row >> np.uint64(32), np.full(M, q, dtype=np.uint64), np.full(M, off, dtype=np.uint64)]
        if fault == "counter_words_2_3_swapped":
            ctr[2], ctr[3] = ctr[3], ctr[2]
        w = philox4x32_10(ctr, (klo, khi), m0=M0 ^ 2 if fault == "wrong_multiplier" else M0)
        for j in range(4):
            out[:, q4 * 4 + j] = w[j]
    return out


def words_to_u(words):
    """fp32 u exactly as the kernel forms it: the integer (w >> 8) + 1 <= 2^24 converts exactly, and so does the product with 2^-24."""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def exp_ref(words):
    """fp64 -log(u) of that same fp32 u: what E_out approximates (before its + 1e-30)."""
    return -np.log(words_to_u(words).astype(np.float64))


def race_labels(words, K):
    """Labels of a race with equal probabilities over the first K classes: argmax_c 1 / E_c = the largest u, first maximum on a tie."""
    return np.argmax(np.asarray(words, dtype=np.uint32)[:, :K] >> np.uint32(8), axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU word tests
M_WORDS = 4099                                   # 16 full workgroups of 256 rows and a partial one of 3
SEED_HI = 0x8000000100C0FFEE                     # top bit set and a non-zero high word
SEEDS = (0, 1234, SEED_HI)
OFFSETS = (None, 7, 2 ** 32 + 7)                 # the kernel keeps the low 32 bits: the last equals 7
ROWS_PER_SAMPLE = 1367                           # 3 samples, not a multiple of 256: 4101 rows, the multiple of 3 next to M_WORDS
SEED_TRIPLES = ((0, 1234, SEED_HI), (1234, SEED_HI, 0), (SEED_HI, 0, 1234))


def word_cases():
    """(kmax, kwargs of draw_words) of every compared launch."""
    cases = []
    for kmax in (16, 32):
        for off in OFFSETS:
            for s in SEEDS:
                cases.append((kmax, dict(M=M_WORDS, seed=s, offset=off)))
            for tr in SEED_TRIPLES:
                cases.append((kmax, dict(M=3 * ROWS_PER_SAMPLE, seeds=tr, rows_per_sample=ROWS_PER_SAMPLE, offset=off)))
    return cases
