"""CCDM mask editing, the part that needs no GPU: the torch restatement of the blend (tests/ccdm_edit_ref.py) against the reference's
own draws (tests/golden/ccdm_edit.npz, from make_golden_ccdm_edit.py), its identities, the Philox offset word on integers, and the
refusals of the host layer, which are raised before anything touches a device."""
import numpy as np
import pytest
import torch

import ccdm_edit_ref as ER
import philox_ref as PR
from util import T, gold

torch.set_grad_enabled(False)
S_FX = int(np.prod(ER.FX_SP))


@pytest.fixture(scope="module")
def g():
    return gold("ccdm_edit")


@pytest.mark.parametrize("K", ER.KS)
@pytest.mark.parametrize("name", ["qx0", "qxtm1"])
def test_restatement_equals_the_reference_draws(g, K, name):
    """Every (K, t): sample n of the fixture is the draw at t = TS[n]."""
    known, E, mix = T(g[f"k{K}_known"]).view(-1), T(g[f"k{K}_{name}_E"]), T(g[f"k{K}_{name}_mix"])
    want = T(g[f"k{K}_{name}_labels"]).view(len(ER.TS), S_FX)
    got = ER.q_sample(known, mix, S_FX, K, E).view(len(ER.TS), S_FX)
    for n, t in enumerate(ER.TS):
        assert torch.equal(got[n], want[n]), f"K={K} {name} t={t}"
    # the stored mix rows are the schedule rows, formed as the reference forms them
    t = torch.tensor(ER.TS)
    ca, betas = T(g[f"k{K}_cumalphas"]), T(g[f"k{K}_betas"])
    rows = torch.stack([ca[t - 1], 1 - ca[t - 1]], 1) if name == "qx0" else torch.stack([1 - betas[t - 1], betas[t - 1]], 1)
    assert torch.equal(rows.float(), mix)


def test_product_schedule_rows_equal_the_fixture(g):
    """DiffusionModel.known_mix / renoise_mix hand the kernels the reference's own operands, bit for bit."""
    from jointimagegeneration_amd.ccdm import DiffusionModel
    for K in ER.KS:
        d = DiffusionModel("cosine", ER.T_STEPS, K, dims=3)
        assert torch.equal(d.known_mix(ER.TS), T(g[f"k{K}_qx0_mix"]))
        assert torch.equal(d.renoise_mix(ER.TS), T(g[f"k{K}_qxtm1_mix"]))


@pytest.mark.parametrize("K", ER.KS)
def test_blend_identities(g, K):
    known, E, mix = T(g[f"k{K}_known"]).view(-1), T(g[f"k{K}_qx0_E"]), T(g[f"k{K}_qx0_mix"])
    M = known.numel()
    labels = torch.randint(0, K, (M,), generator=torch.Generator().manual_seed(K), dtype=torch.int32)
    # keep all-zero: the input; keep all-one: the q-sample
    assert torch.equal(ER.blend(labels, known, torch.zeros(M, dtype=torch.uint8), mix, S_FX, K, E), labels)
    assert torch.equal(ER.blend(labels, known, torch.ones(M, dtype=torch.uint8), mix, S_FX, K, E), ER.q_sample(known, mix, S_FX, K, E))
    # a mixed mask: the q-sample where kept, the input elsewhere
    keep = ER.keep_pattern("random", len(ER.TS), S_FX, seed=K)
    got = ER.blend(labels, known, keep, mix, S_FX, K, E)
    assert torch.equal(got[keep != 0], ER.q_sample(known, mix, S_FX, K, E)[keep != 0]) and torch.equal(got[keep == 0], labels[keep == 0])
    # operands (1, 0): known, for any positive tape (the fixture's, a tiny one, a huge one, one that favours another class)
    one = torch.tensor([[1.0, 0.0]]).repeat(len(ER.TS), 1)
    skew = torch.ones(M, K)
    skew[torch.arange(M), known.long()] = 3.0e38
    for tape in (E, torch.full((M, K), 1e-30), torch.full((M, K), 3.0e38), skew):
        assert torch.equal(ER.blend(labels, known, torch.ones(M, dtype=torch.uint8), one, S_FX, K, tape), known.int())


# ------------------------------------------------------------------------------------------------ the offset word
def test_offset_word_is_t_for_the_posterior_draw():
    from jointimagegeneration_amd import ops
    t = np.arange(1 << 16)
    assert np.array_equal(ER.offset_word(t, 0, ER.POSTERIOR), t)
    for tt in (0, 1, 2, 250, 1000, 65535):
        assert ops.philox_offset_word(tt) == tt == ops.philox_offset_word(tt, 0, ops.PHILOX_POSTERIOR)
    assert (ops.PHILOX_POSTERIOR, ops.PHILOX_KNOWN, ops.PHILOX_RENOISE) == (ER.POSTERIOR, ER.KNOWN, ER.RENOISE) == (0, 1, 2)


def test_offset_word_is_distinct_over_its_whole_domain():
    """Every (t < 2^16, j < 256, purpose < 3) decodes back from its word, which fits 32 bits: no two share a word."""
    from jointimagegeneration_amd import ops
    t = np.arange(1 << 16, dtype=np.int64)
    for p in range(3):
        for j in range(256):
            w = ER.offset_word(t, j, p)
            assert w.max() < (1 << 32) and w.min() >= 0
            assert np.array_equal(w & 0xFFFF, t) and np.all((w >> 16) & 0xFF == j) and np.all(w >> 28 == p)
    rs = np.random.RandomState(0)
    for tt, j, p in zip(rs.randint(0, 1 << 16, 200), rs.randint(0, 256, 200), rs.randint(0, 3, 200)):
        assert ops.philox_offset_word(int(tt), int(j), int(p)) == int(ER.offset_word(tt, j, p))
    assert ops.philox_offset_word(65535, 255, 2) == 65535 | (255 << 16) | (2 << 28)


def test_offset_word_separates_the_philox_streams():
    """On the integer Philox of philox_ref: purpose 0 at j = 0 draws what offset t draws, and the three purposes and two repetitions of one
    step draw different words on every row."""
    kw = dict(M=8, kmax=16, seed=PR.SEED_HI)
    base = PR.draw_words(offset=7, **kw)
    assert np.array_equal(PR.draw_words(offset=int(ER.offset_word(7, 0, ER.POSTERIOR)), **kw), base)
    draws = [PR.draw_words(offset=int(ER.offset_word(7, j, p)), **kw) for j, p in ((0, 0), (0, 1), (0, 2), (3, 0), (3, 1), (3, 2))]
    for a in range(len(draws)):
        for b in range(a + 1, len(draws)):
            assert not np.any(np.all(draws[a] == draws[b], axis=1))


def test_offset_word_refusals():
    from jointimagegeneration_amd import ops
    with pytest.raises(ValueError, match="time_steps must be < 65536"):
        ops.philox_offset_word(65536)
    with pytest.raises(ValueError, match="resample must be <= 256"):
        ops.philox_offset_word(5, 256, 1)
    with pytest.raises(ValueError, match="purpose=3"):
        ops.philox_offset_word(5, 0, 3)


# ------------------------------------------------------------------------------------------------ refusals of the chain (CPU tensors)
def model(K=6, time_steps=5, schedule="cosine"):
    from jointimagegeneration_amd.ccdm import DenoisingModel, DiffusionModel
    return DenoisingModel(DiffusionModel(schedule, time_steps, K, dims=3), torch.nn.Identity(), "none", "majority", dims=3).eval()


def test_chain_refusals_by_name():
    m = model()
    sp = (1, 4, 4, 4)
    labels = torch.zeros(sp, dtype=torch.int32)
    known = torch.randint(0, 6, sp, generator=torch.Generator().manual_seed(0))
    keep = torch.ones(sp, dtype=torch.bool)
    cond = torch.zeros((1, 1) + sp[1:])
    with pytest.raises(ValueError, match="keep given without known"):
        m.sample_labels(labels, cond, keep=keep)
    with pytest.raises(ValueError, match="known given without keep"):
        m.sample_labels(labels, cond, known=known)
    with pytest.raises(ValueError, match=r"known has shape \(1, 4, 4, 5\), the labels \(1, 4, 4, 4\)"):
        m.sample_labels(labels, cond, known=torch.zeros((1, 4, 4, 5), dtype=torch.int64), keep=keep)
    with pytest.raises(ValueError, match=r"keep has shape \(4, 4, 4\), the labels \(1, 4, 4, 4\)"):
        m.sample_labels(labels, cond, known=known, keep=keep[0])
    hi = known.clone()
    hi[0, 1, 2, 3] = 6
    with pytest.raises(ValueError, match=r"known holds labels 0\.\.6 outside 0\.\.5"):
        m.sample_labels(labels, cond, known=hi, keep=keep)
    lo = known.clone()
    lo[0, 0, 0, 0] = -1
    with pytest.raises(ValueError, match=r"known holds labels -1\.\.5 outside 0\.\.5"):
        m.sample_labels(labels, cond, known=lo, keep=torch.zeros(sp, dtype=torch.uint8))      # ignored where keep == 0, still in range
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="must be an integer >= 1"):
            m.sample_labels(labels, cond, known=known, keep=keep, resample=bad)
    with pytest.raises(ValueError, match="keep must be bool or uint8"):
        m.sample_labels(labels, cond, known=known, keep=keep.float())
    with pytest.raises(ValueError, match="known must hold integer labels"):
        m.sample_labels(labels, cond, known=known.float(), keep=keep)
    # forward / forward_denoising take the same arguments (the engine has no CPU path: a CPU x is refused before anything else)
    import inspect
    for fn in (m.forward, m.forward_denoising, m.sample_labels):
        p = inspect.signature(fn).parameters
        assert (p["known"].default, p["keep"].default, p["resample"].default) == (None, None, 1)


def test_chain_refuses_what_the_offset_word_cannot_hold():
    sp = (1, 4, 4, 4)
    labels = torch.zeros(sp, dtype=torch.int32)
    known, keep = torch.zeros(sp, dtype=torch.int64), torch.ones(sp, dtype=torch.bool)
    cond = torch.zeros((1, 1) + sp[1:])
    with pytest.raises(ValueError, match="resample=257 exceeds 256"):
        model().sample_labels(labels, cond, known=known, keep=keep, resample=257)
    with pytest.raises(ValueError, match="time_steps=65536 >= 65536"):
        model(time_steps=65536, schedule="linear").sample_labels(labels, cond, known=known, keep=keep)
    with pytest.raises(ValueError, match="time_steps=65536 >= 65536"):
        model(time_steps=65536, schedule="linear").sample_labels(labels, cond, resample=2)
    with pytest.raises(NotImplementedError, match=r"gg_ccdm_q_sample, which takes K <= 16 \(K = 17\)"):
        model(K=17).sample_labels(labels, cond, known=known, keep=keep, resample=2)
    # 65535 steps and 256 repetitions are inside the word: the check passes
    assert model(time_steps=65535, schedule="linear").check_edit(sp, known, keep, 256)[0].dtype == torch.int32

