"""TEST INFRASTRUCTURE ONLY -- torch (CPU, fp32) restatement of gg_ccdm_inpaint_blend and gg_ccdm_q_sample, in the kernels' stated
operation order (include/guidegen_hip.h, csrc/gg_loss.hip), and the Philox offset word of the edited CCDM chain on plain integers.

One row m of sample n = m // rows_per_sample, with mix[n] = (keep, unif) and the K exponentials E[m]:

    v  = unif / float32(K)
    pd = keep * 1 + v        po = keep * 0 + v                (each product and sum rounded to fp32, nothing contracted)
    s  = ((p_0 + p_1) + p_2) + ...                            (p_c = pd at c == known, po elsewhere; left to right from 0)
    label = argmax_c (p_c / s) / E_c                          (two IEEE divisions; first maximum on a tie)

The blend writes that label where keep != 0 and leaves every other row as it is; the q-sample is the blend of every row."""
import numpy as np
import torch

KS = (2, 14, 16, 17, 32)
TS = (1, 2, 25, 50)
T_STEPS = 50
FX_SP = (4, 4, 4)                        # one fixture sample: 64 voxels; the four samples of a case carry the four t of TS
ROWS = 1367                              # rows per sample of the kernel tests (tests/philox_ref.ROWS_PER_SAMPLE): 3 samples, 17 workgroups
STRIDE = 40                              # one-hot row stride of the kernel tests
KEEP_PATTERNS = ("none", "all", "random", "last_row")


def race_labels(known, mix, rows_per_sample, K, E):
    """int32 [M]: the draw of every row.  known int [M]; mix fp32 [N, 2]; E fp32 [M, K]."""
    known = torch.as_tensor(known).long().view(-1)
    mix = torch.as_tensor(mix, dtype=torch.float32).view(-1, 2)
    E = torch.as_tensor(E, dtype=torch.float32).view(-1, K)
    M = known.numel()
    n = torch.arange(M) // rows_per_sample
    ca = mix[n, 0]
    v = mix[n, 1] / torch.tensor(float(K), dtype=torch.float32)
    pd = ca * 1.0 + v
    po = ca * 0.0 + v
    p = torch.where(torch.arange(K)[None, :] == known[:, None], pd[:, None], po[:, None])
    s = torch.zeros(M, dtype=torch.float32)
    for c in range(K):
        s = s + p[:, c]
    best = torch.zeros(M, dtype=torch.int32)
    bestv = torch.full((M,), -1.0, dtype=torch.float32)
    for c in range(K):
        r = (p[:, c] / s) / E[:, c]
        up = r > bestv
        bestv = torch.where(up, r, bestv)
        best = torch.where(up, torch.tensor(c, dtype=torch.int32), best)
    assert p.dtype == s.dtype == bestv.dtype == torch.float32
    return best


def q_sample(x0, mix, rows_per_sample, K, E):
    """gg_ccdm_q_sample: every row drawn."""
    return race_labels(x0, mix, rows_per_sample, K, E)


def blend(labels, known, keep, mix, rows_per_sample, K, E):
    """gg_ccdm_inpaint_blend on labels int [M]: a new int32 tensor."""
    labels = torch.as_tensor(labels).to(torch.int32).view(-1)
    keep = torch.as_tensor(keep).view(-1) != 0
    return torch.where(keep, race_labels(known, mix, rows_per_sample, K, E), labels)


def onehot_rows(labels, keep, K, stride, sentinel):
    """bf16 [M, stride]: what the blend leaves of a buffer filled with `sentinel`: channels [0, K) of the kept rows one-hot."""
    labels = torch.as_tensor(labels).long().view(-1)
    out = torch.full((labels.numel(), stride), sentinel, dtype=torch.bfloat16)
    oh = torch.nn.functional.one_hot(labels, K).to(torch.bfloat16)
    kept = torch.as_tensor(keep).view(-1) != 0
    out[kept, :K] = oh[kept]
    return out


def keep_pattern(name, n_samples, rows_per_sample, seed=0):
    """uint8 [n_samples * rows_per_sample]."""
    M = n_samples * rows_per_sample
    if name == "none":
        return torch.zeros(M, dtype=torch.uint8)
    if name == "all":
        return torch.ones(M, dtype=torch.uint8)
    if name == "random":
        return (torch.rand(M, generator=torch.Generator().manual_seed(77 + seed)) < 0.5).to(torch.uint8)
    assert name == "last_row"
    k = torch.zeros(M, dtype=torch.uint8)
    k[rows_per_sample - 1::rows_per_sample] = 1
    return k


def tile_tape(E, M, shift=0):
    """fp32 [M, K] from the fixture tape E [m, K]: its rows, cycled from row `shift` on."""
    E = torch.as_tensor(E, dtype=torch.float32)
    return E[(torch.arange(M) + shift) % E.shape[0]].contiguous()


# ------------------------------------------------------------------------------------------------ the Philox offset word, on integers
POSTERIOR, KNOWN, RENOISE = 0, 1, 2


def offset_word(t, j=0, purpose=POSTERIOR):
    """t | (j << 16) | (purpose << 28) for t < 2^16, j < 256, purpose < 3 (ints or integer arrays)."""
    return np.asarray(t, dtype=np.int64) | (np.asarray(j, dtype=np.int64) << 16) | (np.asarray(purpose, dtype=np.int64) << 28)
