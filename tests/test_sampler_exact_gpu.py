"""GPU suite: the CCDM sampler kernels pinned exactly.

* The Philox draw (csrc/gg_posterior.h: ccdm_draw_row), observed through gg_ccdm_draw_tape, word for word against the integer restatement
  philox_ref.py; the word -> exponential map on all 2^24 values it can see; and the draw inside every kernel that has one
  (gg_ccdm_posterior_sample, ..._seeds, gg_ccdm_q_sample, the fused head-conv epilogue) against tape mode fed with that tape.
* gg_ccdm_posterior_sample bit for bit against the plain-C oracle (oracle/ccdm_posterior.c) at the first, last and odd class counts of
  both instantiations, on rows built to hit the clamp, exact ties, a padded stride and the one-hot row's untouched lanes; the run-time-K
  softmax under the criteria of test_posterior_kernel_logits_and_philox.
* gg_minmax_normalise, gg_lincomb4 and gg_timestep_embedding against the plain torch expression.

M = 4099 rows per call: 16 full workgroups and one of 3 rows.  Per-sample calls take the multiple of the sample count next to it (4101 =
3 * 1367, 4100 = 2 * 2050), since the entry points require M to split evenly; 1367 and 2050 are no multiples of the workgroup size, so
that samples begin inside a workgroup."""
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from oracle import nets as O
from test_oracle_golden import c_posterior
from util import rel_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

M = P.M_WORDS
A, ABAR = 0.93, 0.41                  # the step scalars of every family but the clamp's
KS_EXACT = (2, 3, 5, 14, 15, 16, 17, 31, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()                       # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


def kmax_of(K):
    return 16 if K <= 16 else 32


def offset_tensor(off, dev):
    return None if off is None else torch.tensor([off], dtype=torch.int64, device=dev)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def scalars(a, abar, dev):
    return torch.tensor([a, abar], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ the words
@pytest.mark.parametrize("mode", ["single_key", "per_sample"])
@pytest.mark.parametrize("kmax", [16, 32])
def test_draw_tape_words_equal_the_integer_restatement(dev, kmax, mode):
    """bits_out == philox_ref.draw_words for seeds 0, 1234 and one with the top bit and a non-zero high word, offsets NULL, 7 and
    2^32 + 7 (the kernel keeps the low 32 bits of the offset: the last equals 7), one key for all rows or three samples of 1367 rows.
    test_philox_cpu.py shows that these launches see a wrong multiplier, swapped key or counter words, a shifted draw index, an unreduced
    per-sample row and an ignored offset.  NOT covered: the counter's second word (row >> 32) is zero below 2^32 rows."""
    from jointimagegeneration_amd import ops
    seen = {}
    for km, kw in P.word_cases():
        if km != kmax or ("seeds" in kw) != (mode == "per_sample"):
            continue
        if mode == "per_sample":
            bits, E = ops.ccdm_draw_tape(kw["M"], kmax, philox_seeds=ops.philox_seed_tensor(kw["seeds"], dev),
                                         philox_offset=offset_tensor(kw["offset"], dev))
        else:
            bits, E = ops.ccdm_draw_tape(kw["M"], kmax, philox_seed=kw["seed"], philox_offset=offset_tensor(kw["offset"], dev), device=dev)
        want = P.draw_words(kmax=kmax, **kw)
        assert np.array_equal(as_u32(bits), want), (kw, int((as_u32(bits) != want).sum()))
        # the exponentials of a drawn row are the map of its words: bits_in gives the same E
        _, E2 = ops.ccdm_draw_tape(kw["M"], kmax, bits_in=bits, want_bits=False)
        assert torch.equal(E, E2)
        seen[(kw.get("seed", kw.get("seeds")), kw["offset"])] = bits
    assert len(seen) == 9
    key0 = 0 if mode == "single_key" else P.SEED_TRIPLES[0]
    if mode == "single_key":                  # row 0 at seed 0, offset 0: the all-zero Random123 known answer itself
        assert [int(v) for v in as_u32(seen[(0, None)])[0, :4]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert torch.equal(seen[(key0, 7)], seen[(key0, 2 ** 32 + 7)]) and not torch.equal(seen[(key0, 7)], seen[(key0, None)])


# ------------------------------------------------------------------------------------------------ word -> exponential, all 2^24 values
# Measured on an MI355X (ROCm 7, the hardware logarithm): see DESIGN.md "The Philox draw".  The map is deterministic; the factor 2 only
# allows for another compiler lowering of __logf.
E_REL_MEASURED = 1.880720e-07      # largest |E - ref| / ref over u <= 1 - 2^-10
E_ABS_MEASURED = 1.054897e-10      # largest |E - ref| over u > 1 - 2^-10


def test_word_to_exponential_map_on_every_24_bit_value(dev):
    """bits_in = v << 8 for every v in [0, 2^24): u = (v + 1) * 2^-24.  E must be finite and > 0 (a divisor of the race), non-increasing
    in v, and exactly 1e-30f at u == 1; against fp64 -log(u) of the same fp32 u its relative error below u = 1 - 2^-10 and its absolute
    error above stay within twice the measured values."""
    from jointimagegeneration_amd import ops
    v = np.arange(2 ** 24, dtype=np.uint32)
    words = v << np.uint32(8)
    for kmax in (16, 32):
        bits_in = torch.from_numpy(words.view(np.int32).reshape(-1, kmax)).to(dev)
        _, E = ops.ccdm_draw_tape(bits_in.shape[0], kmax, bits_in=bits_in, want_bits=False)
        E = E.reshape(-1)
        if kmax == 32:
            assert torch.equal(E, E16)                                 # one map in both instantiations
            break
        E16 = E
    assert bool(torch.isfinite(E).all())
    assert bool((E > 0).all()), f"{int((E <= 0).sum())} draws with E <= 0, the first at v = {int((E <= 0).nonzero()[0])}"
    assert bool((E[1:] <= E[:-1]).all()), f"{int((E[1:] > E[:-1]).sum())} places where E grows with u"
    assert float(E[-1]) == float(np.float32(1e-30)) and float(E[-2]) > 1e-8
    got = E.cpu().numpy().astype(np.float64)
    ref = P.exp_ref(words)
    lo = P.words_to_u(words) <= np.float32(1.0 - 2.0 ** -10)
    rel = float((np.abs(got[lo] - ref[lo]) / ref[lo]).max())
    ab = float(np.abs(got[~lo] - ref[~lo]).max())
    print(f"word -> exponential: max rel err {rel:.6e} (u <= 1 - 2^-10), max abs err {ab:.6e} (above)")
    assert rel <= 2 * E_REL_MEASURED, rel
    assert ab <= 2 * E_ABS_MEASURED, ab


# ------------------------------------------------------------------------------------------------ the tape equals the draw
def random_rows(K, rows, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.softmax(3 * torch.randn(rows, K, generator=g), -1)
    lab = torch.randint(0, K, (rows,), generator=g).int()
    return p0, lab, g


@pytest.mark.parametrize("K", [2, 5, 14, 15, 16, 17, 32])
def test_posterior_philox_labels_equal_tape_labels(dev, K):
    from jointimagegeneration_amd import ops
    p0, lab, _ = random_rows(K, M, 100 + K, dev)
    sc, off = scalars(A, ABAR, dev), offset_tensor(7, dev)
    got = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, philox_seed=P.SEED_HI, philox_offset=off, draw=True)
    _, E = ops.ccdm_draw_tape(M, kmax_of(K), philox_seed=P.SEED_HI, philox_offset=off, want_bits=False, device=dev)
    tape = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, E=E[:, :K].contiguous(), draw=True)
    assert torch.equal(got, tape)
    greedy = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, draw=False)
    assert float((got != greedy).float().mean()) > 0.02               # the draw decides labels: the comparison is not vacuous
    other = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, philox_seed=P.SEED_HI, draw=True)
    assert not torch.equal(got, other)                                # ... and the offset reaches it


@pytest.mark.parametrize("K", [6, 14, 20])
def test_posterior_per_sample_philox_labels_equal_tape_labels(dev, K):
    from jointimagegeneration_amd import ops
    rows = 3 * P.ROWS_PER_SAMPLE
    p0, lab, _ = random_rows(K, rows, 200 + K, dev)
    sc, off = scalars(A, ABAR, dev), offset_tensor(2 ** 32 + 7, dev)
    seeds = ops.philox_seed_tensor(P.SEED_TRIPLES[1], dev)
    got = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, philox_seeds=seeds, philox_offset=off, draw=True)
    _, E = ops.ccdm_draw_tape(rows, kmax_of(K), philox_seeds=seeds, philox_offset=off, want_bits=False)
    tape = ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, E=E[:, :K].contiguous(), draw=True)
    assert torch.equal(got, tape)
    assert float((got != ops.ccdm_posterior_sample(p0.to(dev), False, lab.to(dev), sc, K, draw=False)).float().mean()) > 0.02


@pytest.mark.parametrize("K", [2, 14, 16])
def test_q_sample_philox_labels_equal_tape_labels(dev, K):
    """gg_ccdm_q_sample calls the same ccdm_draw_row (per-sample keys, the row within the sample)."""
    from jointimagegeneration_amd import ops
    rows = 2 * 2050
    g = torch.Generator().manual_seed(300 + K)
    x0 = torch.randint(0, K, (rows,), generator=g).int().to(dev)
    mix = torch.tensor([[0.7, 0.3], [0.2, 0.8]], dtype=torch.float32, device=dev)
    seeds, off = ops.philox_seed_tensor((P.SEED_HI, 1234), dev), offset_tensor(7, dev)
    got = ops.ccdm_q_sample(x0, mix, K, philox_seeds=seeds, philox_offset=off)
    _, E = ops.ccdm_draw_tape(rows, 16, philox_seeds=seeds, philox_offset=off, want_bits=False)
    tape = ops.ccdm_q_sample(x0, mix, K, E=E[:, :K].contiguous())
    assert torch.equal(got, tape)
    assert float((got != x0).float().mean()) > 0.1                    # labels really move
    assert not torch.equal(got, ops.ccdm_q_sample(x0, mix, K, philox_seeds=seeds))


def test_fused_head_conv_philox_labels_equal_tape_labels(dev, monkeypatch):
    """The reverse step as the head conv's epilogue (the harness of the `philox` case of
    test_head_conv_with_fused_ccdm_reverse_step_equals_conv_then_sampler_kernel): its draw is ccdm_posterior_voxel's."""
    from jointimagegeneration_amd import ops
    monkeypatch.setattr(ops, "PATH_HINT", 6)                 # the 1024-position box on a small grid
    K, Cin, sp = 14, 64, (16, 16, 32)
    rows = sp[0] * sp[1] * sp[2]
    g = torch.Generator().manual_seed(77)
    x = ops.CL(torch.randn((1,) + sp + (Cin,), generator=g).to(dev).bfloat16(), Cin)
    w = (torch.randn(K, Cin, 3, 3, 3, generator=g) * (3.0 / math.sqrt(Cin * 27))).to(dev)
    pw = ops.pack_conv_weight(w, Cin)
    bias = torch.zeros(1, 32, device=dev); bias[0, :K] = torch.randn(K, generator=g).to(dev) * 0.3
    gamma, beta = (1 + 0.1 * torch.randn(Cin, generator=g)).to(dev), (0.1 * torch.randn(Cin, generator=g)).to(dev)
    prol = ops.groupnorm_stats(x, gamma, beta, 1e-5)
    xt = torch.randint(0, K, (rows,), generator=g, dtype=torch.int32).to(dev)
    scal, off = scalars(0.97, 0.41, dev), offset_tensor(123, dev)
    _, E = ops.ccdm_draw_tape(rows, 16, philox_seed=991, philox_offset=off, want_bits=False, device=dev)
    labs = []
    for tape in (None, E[:, :K].contiguous()):
        lab = torch.empty(rows, dtype=torch.int32, device=dev)
        y = ops.conv(x, pw, bias, K, k=(3, 3, 3), out_f32=True, prologue=prol, bias_per_sample=True,
                     post=dict(xt=xt, scalars=scal, K=K, E=tape, philox_seed=991, philox_offset=off, draw=True, labels_out=lab))
        assert y.fused_post                                   # really the fused epilogue
        labs.append(lab)
    assert torch.equal(labs[0], labs[1])
    assert (labs[0] != xt).float().mean() > 0.02 and len(torch.unique(labs[0])) >= 4


# ------------------------------------------------------------------------------------------------ posterior, exact against the C oracle
def run_exact(ops, dev, head, p0, lab, E, a, abar, K, onehot=False):
    """The kernel on `head` (p0 in its first K lanes) against c_posterior on p0: labels and probs_out bit for bit -> the oracle's pair."""
    rows = p0.shape[0]
    probs = torch.empty(rows, K, device=dev)
    oh = torch.full((rows, 40), 7.0, dtype=torch.bfloat16, device=dev) if onehot else None
    got = ops.ccdm_posterior_sample(head.to(dev), False, lab.to(dev), scalars(a, abar, dev), K, E=None if E is None else E.to(dev),
                                    draw=E is not None, probs_out=probs, onehot_out=oh)
    labc, prc = c_posterior(p0, lab, E, a, abar, K)
    assert torch.equal(got.cpu(), labc), int((got.cpu() != labc).sum())
    assert torch.equal(probs.cpu(), prc), int((probs.cpu() != prc).sum())
    if onehot:                                   # lanes [0, K): the one-hot of the label; lanes >= K: NOT touched
        assert torch.equal(oh[:, :K].float().cpu(), torch.nn.functional.one_hot(labc.long(), K).float())
        assert torch.equal(oh[:, K:], torch.full((rows, 40 - K), 7.0, dtype=torch.bfloat16, device=dev))
    return labc, prc


@pytest.mark.parametrize("K", KS_EXACT)
def test_posterior_dense_and_padded_rows_bit_exact(dev, K):
    """Dense softmax rows in tape and argmax mode, and the same rows at head_stride = K + 3 with NaN in the extra lanes (a lane read past
    K would poison the sums); the one-hot row at a stride of 40 over a sentinel (every K: odd ones end in a 2-byte store)."""
    from jointimagegeneration_amd import ops
    p0, lab, g = random_rows(K, M, 400 + K, dev)
    E = torch.empty(M, K).exponential_(1, generator=g)
    run_exact(ops, dev, p0, p0, lab, E, A, ABAR, K, onehot=True)
    run_exact(ops, dev, p0, p0, lab, None, A, ABAR, K, onehot=True)
    head = torch.full((M, K + 3), float("nan"))
    head[:, :K] = p0
    run_exact(ops, dev, head, p0, lab, E, A, ABAR, K)
    run_exact(ops, dev, head, p0, lab, None, A, ABAR, K)


@pytest.mark.parametrize("K", KS_EXACT)
def test_posterior_clamp_rows_bit_exact(dev, K):
    """abar = 1 (the scalars of t == 1, with a < 1): the posterior reduces to p0, so a lane holding 0 or 1e-13 is below the clamp and one
    holding a softmax value is not.  Lane m % K of row m is kept alive; of the others a quarter are 0 and a quarter 1e-13."""
    from jointimagegeneration_amd import ops
    p0, lab, g = random_rows(K, M, 500 + K, dev)
    kind = torch.randint(0, 4, (M, K), generator=g)                    # 0: exact zero, 1: 1e-13, 2 / 3: left alone
    kind[torch.arange(M), torch.arange(M) % K] = 3
    alive = torch.where(kind >= 2, p0, torch.zeros(()))
    alive = alive / alive.sum(-1, keepdim=True)                        # the live lanes sum to 1 within rounding, the smallest is > 1e-9
    p0 = torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, torch.full((), 1e-13), alive))
    E = torch.empty(M, K).exponential_(1, generator=g)
    for tape in (E, None):
        _, prc = run_exact(ops, dev, p0, p0, lab, tape, 0.9, 1.0, K)
        # from the reference: exactly the lanes built to be below the clamp sit at 1e-12 / s, s the row sum = 1 within 1e-5
        clamped = (prc.double() - 1e-12).abs() < 1e-17
        assert torch.equal(clamped, kind < 2)
    share = float((kind < 2).float().mean())
    assert 0.5 * (K - 1) / K - 0.03 < share < 0.5 * (K - 1) / K + 0.03, share         # half of the K - 1 free lanes of a row


@pytest.mark.parametrize("K", KS_EXACT)
def test_posterior_tied_rows_bit_exact(dev, K):
    """Two equal largest probabilities at lanes i < j with equal exponentials there (every other lane has a small probability and a
    large exponential): wherever the two posteriors come out bit-equal, which the reference shows for at least a seventh of the rows
    (neither lane being the current label, the two sums differ only in the order of their terms), the race is an exact tie and the lower
    index wins."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(600 + K)
    p0 = 0.02 * torch.rand(M, K, generator=g) / K
    i = torch.randint(0, K - 1, (M,), generator=g)
    j = torch.minimum(i + 1 + (torch.rand(M, generator=g) * (K - 1 - i).float()).long(), torch.tensor(K - 1))
    big = 0.3 + 0.19 * torch.rand(M, generator=g)
    r = torch.arange(M)
    p0[r, i] = big
    p0[r, j] = big
    lab = torch.randint(0, K, (M,), generator=g).int()
    E = torch.full((M, K), 1e6)
    e = 0.5 + torch.rand(M, generator=g)
    E[r, i] = e
    E[r, j] = e
    a = 0.05                                                           # a weak pull towards the current label: the pair stays the largest
    labc, prc = run_exact(ops, dev, p0, p0, lab, E, a, ABAR, K)
    tie = prc[r, i] == prc[r, j]
    assert torch.equal(labc[tie].long(), i[tie])                       # the reference itself: first maximum wins
    lab0, _ = run_exact(ops, dev, p0, p0, lab, None, a, ABAR, K)      # argmax mode: the same tie without a tape
    top = tie & (prc.max(-1).values == prc[r, i])
    assert torch.equal(lab0[top].long(), i[top])
    print(f"K={K}: exact ties in {float(tie.float().mean()):.3f} of the rows, the largest posterior in {float(top.float().mean()):.3f}")
    if K > 2:                                                          # K == 2: one of the two lanes is the current label, no tie
        assert float(top.float().mean()) >= 1 / 7, float(top.float().mean())


@pytest.mark.parametrize("K", [6, 17, 32])
def test_posterior_logits_with_a_run_time_class_count(dev, K):
    """is_logits = 1 outside the compiled-in K = 14: the run-time-K softmax of both instantiations, stride padded, NaN beyond K.
    Criteria of test_posterior_kernel_logits_and_philox (expf differs in the last ulp between glibc and the GPU): probs rtol 1e-5, at
    most 1 label in 10 000 differing, 2 of these 20 000."""
    from jointimagegeneration_amd import ops
    rows = 20000
    g = torch.Generator().manual_seed(700 + K)
    logits = torch.full((rows, K + 3), float("nan"))
    logits[:, :K] = 2 * torch.randn(rows, K, generator=g)
    lab = torch.randint(0, K, (rows,), generator=g).int()
    E = torch.empty(rows, K).exponential_(1, generator=g)
    probs = torch.empty(rows, K, device=dev)
    got = ops.ccdm_posterior_sample(logits.to(dev), True, lab.to(dev), scalars(0.9, 0.5, dev), K, E=E.to(dev), draw=True, probs_out=probs)
    labc, prc = c_posterior(torch.softmax(logits[:, :K], -1), lab, E, 0.9, 0.5, K)
    differing = int((got.cpu() != labc).sum())
    print(f"K={K}: {differing} of {rows} labels differ, probs max rel {float(((probs.cpu() - prc).abs() / prc).max()):.3e}")
    assert differing <= 2
    assert torch.allclose(probs.cpu(), prc, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the three small kernels
def same_with_nan(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.mark.parametrize("n", [1, 63, 65, 4800, 2 ** 20 + 3])
def test_minmax_normalise_equals_the_torch_expression(dev, n):
    """(x - min) / (max - min) in fp32, one rounding per operation: torch.equal, NaN for NaN on a constant tensor (n == 1 is one)."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(800 + n % 997)
    base = 3 * torch.randn(n, generator=g)
    negative = -base.abs() - 0.25
    mixed = base.clone()
    mixed[::7] = -0.0
    mixed[3::7] = 0.0
    constant = torch.full((n,), -1.625)
    tail = base.clone()                                                # both extremes in the last, partial wave of the last workgroup
    tail[-1] = 40.0
    if n > 1:
        tail[-2] = -50.0
    for name, x in (("negative", negative), ("mixed", mixed), ("constant", constant), ("tail", tail)):
        want = (x - x.min()) / (x.max() - x.min())
        got = ops.minmax_normalise(x.to(dev)).cpu()
        if name == "constant" or n == 1:
            assert bool(want.isnan().all())
        else:
            assert not bool(want.isnan().any()) and float(want.min()) == 0.0 and float(want.max()) == 1.0
        assert same_with_nan(got, want), (name, n)


PLMS_SETS = (((55.0, -59.0, 37.0, -9.0), 24.0), ((23.0, -16.0, 5.0), 12.0), ((3.0, -1.0), 2.0), ((3.0,), 2.0))


@pytest.mark.parametrize("n", [1, 4099])
def test_lincomb4_equals_the_left_to_right_torch_expression(dev, n):
    """1, 2, 3 and 4 terms with the PLMS coefficient sets (plms.py:218-232): each product and each sum rounded once, in order."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(900 + n)
    es = [torch.randn(n, generator=g) * (1 + k) for k in range(4)]
    for coefs, denom in PLMS_SETS:
        want = coefs[0] * es[0]
        for c, e in zip(coefs[1:], es[1:]):
            want = want + c * e
        want = want / denom
        out = torch.full((n,), float("nan"), device=dev)
        ops.lincomb4([e.to(dev) for e in es[:len(coefs)]], coefs, denom, out)
        assert torch.equal(out.cpu(), want), (len(coefs), n)


@pytest.mark.parametrize("dim", [64, 65, 1])
def test_timestep_embedding_odd_widths(dev, dim):
    """cos || sin over dim // 2 frequencies, and for an odd dim one more column that is exactly 0 (at dim == 1 that is all there is).
    The other columns: the existing bounds, 2e-5 of the largest value for t <= 250 and 2e-4 for t <= 981."""
    from jointimagegeneration_amd import ops
    for t, tol in ((torch.tensor([0.0, 1.0, 17.0, 250.0]), 2e-5), (torch.tensor([1.0, 481.0, 981.0]), 2e-4)):
        got = ops.timestep_embedding(t.to(dev), dim).cpu()
        assert got.shape == (t.numel(), dim)
        half = dim // 2
        if dim % 2:
            assert torch.equal(got[:, 2 * half:], torch.zeros(t.numel(), 1))
        if half:
            assert rel_err(got[:, :2 * half], O.timestep_embedding(t, 2 * half)) < tol
