"""CCDM mask editing on the GPU (-m gpu): gg_ccdm_inpaint_blend bit for bit against the torch restatement (tests/ccdm_edit_ref.py, which
test_ccdm_edit_cpu.py holds to the reference's own draws), its Philox mode against gg_ccdm_draw_tape at the documented offset word, and the
edited chain of DenoisingModel.sample_labels: unchanged without a mask, composed exactly of the blend and the existing step with one,
kept voxels returned unchanged, resampling, graph against eager, and the ddpm_eval options.  Labels are integers: every comparison is
torch.equal."""
import json

import numpy as np
import pytest
import torch

import ccdm_edit_ref as ER
import philox_ref as PR
from util import CCDM_SMALL, T, gold, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
K_NET, SP = 6, (8, 8, 8)                 # the small CCDM UNet of the suite ("ccdm_small." weights) on 8^3 voxels
M_NET = 512


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return gold("ccdm_edit")


@pytest.fixture(scope="module")
def unet(dev):
    from jointimagegeneration_amd.unet import create_unet_openai
    return seeded(create_unet_openai(image_size=16, in_channels=K_NET + 1, out_channels=K_NET, num_res_blocks=2, cond_encoded_shape=None,
                                     dims=3, **CCDM_SMALL), "ccdm_small.").to(dev)


def chain(unet, dev, time_steps, vote="majority"):
    from jointimagegeneration_amd.ccdm import DenoisingModel, DiffusionModel
    return DenoisingModel(DiffusionModel("cosine", time_steps, K_NET, dims=3), unet, "none", vote, dims=3).eval().to(dev)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_labels(seed, n=1, K=K_NET, sp=SP):
    return torch.randint(0, K, (n,) + sp, generator=gen(seed), dtype=torch.int32)


def rand_keep(seed, n=1, sp=SP):
    return torch.rand((n,) + sp, generator=gen(seed)) < 0.5


def exp_tapes(count, seed, M=M_NET, K=K_NET):
    return [torch.empty(M, K).exponential_(1, generator=gen(seed + i)) for i in range(count)]


# ------------------------------------------------------------------------------------------------ 1. the kernel, bit for bit
@pytest.mark.parametrize("K", ER.KS)
def test_blend_kernel_equals_the_restatement_on_the_fixture_tapes(dev, g, K):
    from jointimagegeneration_amd import ops
    N, R, M = 3, ER.ROWS, 3 * ER.ROWS
    mix = T(g[f"k{K}_qx0_mix"])[1:4].contiguous()                    # three different rows: t = 2, 25, 50
    assert len({tuple(r) for r in mix.tolist()}) == 3
    E = ER.tile_tape(g[f"k{K}_qx0_E"], M, shift=K)
    known = torch.randint(0, K, (M,), generator=gen(10 + K), dtype=torch.int32)
    labels = torch.randint(0, K, (M,), generator=gen(20 + K), dtype=torch.int32)
    sentinel = 7.0
    for pat in ER.KEEP_PATTERNS:
        keep = ER.keep_pattern(pat, N, R, seed=K)
        lab = labels.to(dev)
        oh = torch.full((M, ER.STRIDE), sentinel, dtype=torch.bfloat16, device=dev)
        out = ops.ccdm_inpaint_blend(lab, known.to(dev), keep.to(dev), mix.to(dev), K, E=E.to(dev), onehot_out=oh)
        assert out.data_ptr() == lab.data_ptr()
        want = ER.blend(labels, known, keep, mix, R, K, E)
        assert torch.equal(lab.cpu(), want), f"K={K} keep={pat}"
        # channels >= K and every row with keep == 0 keep the sentinel; the kept rows hold the one-hot of their new label
        assert torch.equal(oh.cpu(), ER.onehot_rows(want, keep, K, ER.STRIDE, sentinel)), f"K={K} keep={pat}: one-hot rows"
        if pat == "none":
            assert torch.equal(lab.cpu(), labels)
        if pat == "all" and K <= 16:                                   # the unmasked launch, exactly
            assert torch.equal(lab, ops.ccdm_q_sample(known.to(dev), mix.to(dev), K, E=E.to(dev)))
        # without a one-hot output: the same labels
        lab2 = labels.to(dev)
        ops.ccdm_inpaint_blend(lab2, known.to(dev), keep.to(dev), mix.to(dev), K, E=E.to(dev))
        assert torch.equal(lab2, lab)
    # documented aliasing: known may be the labels buffer itself; the kept rows are then re-noised in place
    keep = ER.keep_pattern("random", N, R, seed=K)
    buf = labels.to(dev)
    ops.ccdm_inpaint_blend(buf, buf, keep.to(dev), mix.to(dev), K, E=E.to(dev))
    assert torch.equal(buf.cpu(), ER.blend(labels, labels, keep, mix, R, K, E))


def test_blend_kernel_final_operands_return_known(dev):
    from jointimagegeneration_amd import ops
    for K in (2, 17):
        M = 2 * ER.ROWS
        known = torch.randint(0, K, (M,), generator=gen(K), dtype=torch.int32).to(dev)
        keep = ER.keep_pattern("random", 2, ER.ROWS, seed=1).to(dev)
        labels = torch.randint(0, K, (M,), generator=gen(K + 1), dtype=torch.int32).to(dev)
        before = labels.clone()
        one = torch.tensor([[1.0, 0.0], [1.0, 0.0]], device=dev)
        ops.ccdm_inpaint_blend(labels, known, keep, one, K, philox_seed=5, philox_offset=torch.tensor([9], device=dev))
        assert torch.equal(labels, torch.where(keep != 0, known, before))


def test_blend_kernel_refusals(dev):
    """GG_ERR_BAD_SHAPE, each case of the header comment; all are decided on the host, before any launch."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    M, K = 64, 6
    lab = torch.zeros(M, dtype=torch.int32, device=dev)
    keep = torch.zeros(M, dtype=torch.uint8, device=dev)
    mix = torch.zeros((2, 2), device=dev)
    oh = torch.zeros((M, 8), dtype=torch.bfloat16, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(labels=lab, known=lab, keep_=keep, mix_=mix, rps=32, K_=K, M_=M, onehot=None, stride=0):
        return lib.gg_ccdm_inpaint_blend(labels if labels is None else labels.data_ptr(), known if known is None else known.data_ptr(),
                                         keep_ if keep_ is None else keep_.data_ptr(), mix_ if mix_ is None else mix_.data_ptr(), rps, K_, None, 0,
                                         None, None, M_, onehot, stride, s)
    BAD = -1
    assert call() == 0
    for kw in (dict(labels=None), dict(known=None), dict(keep_=None), dict(mix_=None), dict(K_=1), dict(K_=33), dict(rps=24), dict(rps=0),
               dict(M_=0), dict(onehot=oh.data_ptr(), stride=4), dict(onehot=oh.data_ptr(), stride=7), dict(onehot=oh.data_ptr() + 2, stride=8)):
        assert call(**kw) == BAD, kw
    assert b"ccdm_inpaint_blend" in lib.gg_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [2, 14, 16])
@pytest.mark.parametrize("mode", ["tape", "philox"])
def test_q_sample_equals_the_blend_with_every_row_kept(dev, K, mode):
    """The invariant the edited chain relies on: gg_ccdm_q_sample is gg_ccdm_inpaint_blend with keep all-one.  2 samples of 389 rows: four
    workgroups of 256 with a partial last one, and the sample boundary falls inside a workgroup and inside a wave."""
    from jointimagegeneration_amd import ops
    N, R, stride, sentinel = 2, 389, 32, 7.0
    M = N * R
    x0 = torch.randint(0, K, (M,), generator=gen(50 + K), dtype=torch.int32).to(dev)
    mix = torch.tensor([[0.75, 0.25], [0.25, 0.75]], device=dev)
    keep = torch.ones(M, dtype=torch.uint8, device=dev)
    if mode == "tape":
        draw = dict(E=torch.empty(M, K).exponential_(1, generator=gen(60 + K)).to(dev))
    else:
        draw = dict(philox_seeds=ops.philox_seed_tensor((1, 2 ** 63 + 5), dev),
                    philox_offset=torch.tensor([ops.philox_offset_word(7, 3, ops.PHILOX_RENOISE)], dtype=torch.int64, device=dev))
    oh_q = torch.full((M, stride), sentinel, dtype=torch.bfloat16, device=dev)
    oh_b = oh_q.clone()
    lab_q = ops.ccdm_q_sample(x0, mix, K, onehot_out=oh_q, **draw)
    lab_b = torch.randint(0, K, (M,), generator=gen(70 + K), dtype=torch.int32).to(dev)
    ops.ccdm_inpaint_blend(lab_b, x0, keep, mix, K, onehot_out=oh_b, **draw)
    assert torch.equal(lab_q, lab_b)
    assert torch.equal(oh_q[:, :K], oh_b[:, :K])
    assert torch.equal(oh_q[:, :K].float(), torch.nn.functional.one_hot(lab_q.long(), K).float())
    for oh in (oh_q, oh_b):                                           # channels >= K keep the sentinel they were filled with
        assert torch.equal(oh[:, K:], torch.full((M, stride - K), sentinel, dtype=torch.bfloat16, device=dev))
    assert not torch.equal(lab_q, x0) and int(lab_q.min()) >= 0 and int(lab_q.max()) < K
    # the re-noise step's call: labels_out is x0 itself
    buf = x0.clone()
    assert ops.ccdm_q_sample(buf, mix, K, labels_out=buf, **draw).data_ptr() == buf.data_ptr()
    assert torch.equal(buf, lab_q)


# ------------------------------------------------------------------------------------------------ 2. Philox mode equals tape mode
@pytest.mark.parametrize("K", [14, 17])
@pytest.mark.parametrize("tjp", [(7, 0, 1), (7, 3, 2)])
def test_blend_philox_mode_equals_the_drawn_tape(dev, g, K, tjp):
    from jointimagegeneration_amd import ops
    N, R, M = 3, ER.ROWS, 3 * ER.ROWS
    kmax = 16 if K <= 16 else 32
    word = ops.philox_offset_word(*tjp)
    assert word == int(ER.offset_word(*tjp))
    off = torch.tensor([word], dtype=torch.int64, device=dev)
    mix = T(g[f"k{K}_qx0_mix"])[1:4].contiguous().to(dev)
    known = torch.randint(0, K, (M,), generator=gen(30 + K), dtype=torch.int32).to(dev)
    start = torch.randint(0, K, (M,), generator=gen(40 + K), dtype=torch.int32).to(dev)
    keep = ER.keep_pattern("random", N, R, seed=3).to(dev)
    for seed, seeds in ((PR.SEED_HI, None), (0, PR.SEED_TRIPLES[1])):
        sd = None if seeds is None else ops.philox_seed_tensor(seeds, dev)
        bits, E = ops.ccdm_draw_tape(M, kmax, philox_seed=seed, philox_seeds=sd, philox_offset=off)
        # the tape is the documented stream: integer Philox at that offset word
        want_bits = PR.draw_words(M, kmax, seed=seed, seeds=seeds, rows_per_sample=R if seeds else None, offset=word)
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
        a, b = start.clone(), start.clone()
        ops.ccdm_inpaint_blend(a, known, keep, mix, K, philox_seed=seed, philox_seeds=sd, philox_offset=off)
        ops.ccdm_inpaint_blend(b, known, keep, mix, K, E=E[:, :K].contiguous())
        assert torch.equal(a, b), f"K={K} {tjp} seeds={seeds}"
        assert torch.equal(a.cpu(), ER.blend(start.cpu(), known.cpu(), keep.cpu(), mix.cpu(), R, K, E[:, :K].cpu()))
        assert not torch.equal(a, start)


# ------------------------------------------------------------------------------------------------ 3. no mask: today's chain
def interleave(blend_tapes, post_tapes, tv):
    """The tape list of a masked chain at resample = 1: per t the blend tape, then the posterior tape if t > 1."""
    out, pi = [], 0
    for i, t in enumerate(tv):
        out.append(blend_tapes[i])
        if t > 1:
            out.append(post_tapes[pi]); pi += 1
    return out


def test_no_mask_identity(dev, unet):
    m = chain(unet, dev, 6)
    xT, known = rand_labels(1).to(dev), rand_labels(2).to(dev)
    zero = torch.zeros((1,) + SP, dtype=torch.bool, device=dev)
    cond = torch.zeros((1, 1) + SP, device=dev)
    tv = m.t_values(None)
    post, blends = exp_tapes(5, 100), exp_tapes(6, 200)
    fused = {}
    for use_graph in (True, False):
        m.use_graph = use_graph
        for mode in ("philox", "tape"):
            tapes = None if mode == "philox" else post
            a, _ = m.sample_labels(xT, cond, rng_tapes=tapes)
            fa = m.last_step_fused
            b, _ = m.sample_labels(xT, cond, rng_tapes=tapes)
            c, _ = m.sample_labels(xT, cond, rng_tapes=None if mode == "philox" else interleave(blends, post, tv), known=known, keep=zero)
            fc = m.last_step_fused
            d, _ = m.sample_labels(xT, cond, rng_tapes=tapes, known=None, keep=None, resample=1)
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), (use_graph, mode)
            assert fa == fc
            fused[(use_graph, mode)] = a
    assert torch.equal(fused[(True, "philox")], fused[(False, "philox")]) and torch.equal(fused[(True, "tape")], fused[(False, "tape")])
    assert not torch.equal(fused[(True, "philox")], xT)


# ------------------------------------------------------------------------------------------------ 4. composition, exact
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_masked_step_is_the_blend_followed_by_the_existing_step(dev, unet, mode):
    import contextlib
    from jointimagegeneration_amd import ops
    m = chain(unet, dev, 5, "confidence")
    xT, known, keep = rand_labels(3), rand_labels(4), rand_keep(5)
    assert 0.4 < float(keep.float().mean()) < 0.6
    cond = torch.zeros((1, 1) + SP, device=dev)
    tv = m.t_values(None)
    post, blends = exp_tapes(4, 300), exp_tapes(5, 400)
    kmix = m.diffusion.known_mix(tv).cpu()
    with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
        trace = []
        lab, probs = m.sample_labels(xT.to(dev), cond, rng_tapes=interleave(blends, post, tv), trace=trace, known=known.to(dev), keep=keep.to(dev))
        assert [(e["t"], e["j"]) for e in trace] == [(t, 0) for t in tv]
        prev = xT
        for i, (t, e) in enumerate(zip(tv, trace)):
            want_in = ER.blend(prev.view(-1), known.view(-1), keep.view(-1), kmix[i:i + 1], M_NET, K_NET, blends[i])
            assert torch.equal(e["x_in"].cpu().view(-1), want_in), f"t={t}: the blend"
            sub = []
            m.sample_labels(e["x_in"], cond, init_t=t, rng_tapes=post[i:] + post[:i], trace=sub)     # its first step runs on this step's tape
            assert sub[0]["t"] == t and torch.equal(e["labels"], sub[0]["labels"]), f"t={t}: the existing step"
            assert torch.equal(e["probs"], sub[0]["probs"])
            prev = e["labels"].cpu()
    kept = keep.view(-1)
    assert torch.equal(lab.cpu().view(-1)[kept], known.view(-1)[kept])
    assert torch.equal(lab.cpu().view(-1)[~kept], trace[-1]["labels"].cpu().view(-1)[~kept])


def test_too_few_tapes_names_the_count(dev, unet):
    m = chain(unet, dev, 5)
    xT, known, keep = rand_labels(3).to(dev), rand_labels(4).to(dev), rand_keep(5).to(dev)
    cond = torch.zeros((1, 1) + SP, device=dev)
    with pytest.raises(ValueError, match="need 9 rng tapes, got 4"):                   # 5 blend + 4 posterior
        m.sample_labels(xT, cond, rng_tapes=exp_tapes(4, 0), known=known, keep=keep)
    with pytest.raises(ValueError, match="need 23 rng tapes, got 9"):                  # 2 * (5 + 4) + 5 re-noise
        m.sample_labels(xT, cond, rng_tapes=exp_tapes(9, 0), known=known, keep=keep, resample=2)
    with pytest.raises(ValueError, match="need 13 rng tapes, got 4"):                  # 2 * 4 posterior + 5 re-noise
        m.sample_labels(xT, cond, rng_tapes=exp_tapes(4, 0), resample=2)


# ------------------------------------------------------------------------------------------------ 5. ends
def test_kept_voxels_come_back_unchanged(dev, unet):
    xT, known = rand_labels(6).to(dev), rand_labels(7).to(dev)
    cond = torch.zeros((1, 1) + SP, device=dev)
    x_onehot = torch.nn.functional.one_hot(xT.long(), K_NET).permute(0, 4, 1, 2, 3).float()
    want_oh = torch.nn.functional.one_hot(known.long(), K_NET).permute(0, 4, 1, 2, 3)
    # keep all-one: known, and the "confidence" output is its one-hot
    ones = torch.ones((1,) + SP, dtype=torch.uint8, device=dev)
    lab, _ = chain(unet, dev, 6).sample_labels(xT, cond, known=known, keep=ones)
    assert torch.equal(lab, known)
    conf = chain(unet, dev, 6, "confidence")(x_onehot, cond, known=known, keep=ones)["diffusion_out"]
    assert conf.dtype == torch.float32 and torch.equal(conf, want_oh.float())
    # random keep: kept voxels equal known; "majority" and "confidence" agree on the argmax
    keep = rand_keep(8).to(dev)
    maj = chain(unet, dev, 6, "majority")(x_onehot, cond, known=known, keep=keep)["diffusion_out"]
    conf = chain(unet, dev, 6, "confidence")(x_onehot, cond, known=known, keep=keep)["diffusion_out"]
    assert torch.equal(maj.argmax(1)[keep], known.long()[keep])
    assert torch.equal(maj.argmax(1), conf.argmax(1))
    assert torch.equal(conf.permute(0, 2, 3, 4, 1)[keep], want_oh.permute(0, 2, 3, 4, 1)[keep].float())
    assert not torch.equal(maj.argmax(1), known.long())                               # the free voxels were generated, not copied


# ------------------------------------------------------------------------------------------------ 6. resampling
def test_resample_two_in_tape_mode(dev, unet):
    m = chain(unet, dev, 5)
    xT, known, keep = rand_labels(9).to(dev), rand_labels(10).to(dev), rand_keep(11).to(dev)
    cond = torch.zeros((1, 1) + SP, device=dev)
    tv, R = m.t_values(None), 2
    tapes = exp_tapes(23, 500)                                        # per (t, j): blend, posterior (t > 1), re-noise (j = 0)
    trace = []
    lab, _ = m.sample_labels(xT, cond, rng_tapes=tapes, trace=trace, known=known, keep=keep, resample=R)
    assert [(e["t"], e["j"]) for e in trace] == [(t, j) for t in tv for j in range(R)] and len(trace) == 2 * 5
    ti = 0
    for i, t in enumerate(tv):
        e0, e1 = trace[2 * i], trace[2 * i + 1]
        ti += 1 + int(t > 1)                                          # (t, 0): blend, posterior
        renoise_tape = tapes[ti]; ti += 1
        onehot = torch.nn.functional.one_hot(e0["labels"].long(), K_NET).permute(0, 4, 1, 2, 3).float()
        noised = m.diffusion.q_xt_given_xtm1(onehot, torch.tensor([t])).sample_labels(rng_tape=renoise_tape)
        blend_tape = tapes[ti]; ti += 1 + int(t > 1)                  # (t, 1): blend, posterior
        want_in = ER.blend(noised.cpu().view(-1), known.cpu().view(-1), keep.cpu().view(-1), m.diffusion.known_mix([t]).cpu(), M_NET, K_NET, blend_tape)
        assert torch.equal(e1["x_in"].cpu().view(-1), want_in), f"t={t}: re-noise, then blend"
    assert ti == 23
    assert torch.equal(lab[keep], known[keep])
    # resample = 1 is the default
    one = interleave(exp_tapes(5, 600), exp_tapes(4, 700), tv)
    a, _ = m.sample_labels(xT, cond, rng_tapes=one, known=known, keep=keep, resample=1)
    b, _ = m.sample_labels(xT, cond, rng_tapes=one, known=known, keep=keep)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. graph equals eager with a mask
@pytest.mark.parametrize("resample", [1, 2])
def test_masked_graph_equals_eager_and_samples_are_independent(dev, unet, resample):
    m = chain(unet, dev, 6)
    xT, known, keep = rand_labels(12, n=2).to(dev), rand_labels(13, n=2).to(dev), rand_keep(14, n=2).to(dev)
    cond = torch.zeros((2, 1) + SP, device=dev)
    seeds = [PR.SEED_HI, 1234]
    out = {}
    for use_graph in (True, False):
        m.use_graph = use_graph
        out[use_graph], _ = m.sample_labels(xT, cond, philox_seeds=seeds, known=known, keep=keep, resample=resample)
        single, _ = m.sample_labels(xT, cond, known=known, keep=keep, resample=resample)          # the single-key stream
        out[(use_graph, "single")] = single
    assert torch.equal(out[True], out[False]) and torch.equal(out[(True, "single")], out[(False, "single")])
    m.use_graph = True
    own, _ = m.sample_labels(xT[1:], cond[1:], philox_seeds=seeds[1:], known=known[1:], keep=keep[1:], resample=resample)
    assert torch.equal(out[True][1:], own)                            # sample 1 does not depend on its slot or its neighbour
    assert torch.equal(out[True][keep], known[keep])
    if resample == 2:                                                 # the repetitions changed the draw of the free voxels
        base, _ = m.sample_labels(xT, cond, philox_seeds=seeds, known=known, keep=keep)
        assert not torch.equal(base, out[True])


# ------------------------------------------------------------------------------------------------ 8. ddpm_eval
def test_ddpm_eval_edits_a_known_volume(dev, tmp_path):
    import yaml
    from jointimagegeneration_amd import ddpm_eval
    from jointimagegeneration_amd.io import read_nifti, write_nifti
    size, K, nvol = (8, 8, 8), 6, 2
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    kdir, mdir = tmp_path / "known", tmp_path / "keep"
    kdir.mkdir(); mdir.mkdir()
    rng = np.random.default_rng(5)
    knowns = [rng.integers(0, K, size=size).astype(np.uint8) for _ in range(nvol)]
    for vid, a in enumerate(knowns):
        write_nifti(str(kdir / f"known_{vid:04d}.nii.gz"), a)
        write_nifti(str(mdir / f"keep_{vid:04d}.nii.gz"), np.isin(a, (1, 3)).astype(np.uint8) * 5)
    common = [str(pf), "--size", *map(str, size), "--num-classes", str(K), "--num-volumes", str(nvol), "--steps", "4", "--known", str(kdir)]
    ddpm_eval.main(common[:1] + ["cls"] + common[1:] + ["--keep-classes", "1,3"])
    ddpm_eval.main(common[:1] + ["msk"] + common[1:] + ["--keep-mask", str(mdir)])
    ddpm_eval.main(common[:1] + ["s2"] + common[1:] + ["--keep-classes", "1,3", "--samples", "2", "--resample", "2"])
    doc = json.loads((tmp_path / "cls" / "metrics.json").read_text())["edit"]
    assert [v["id"] for v in doc["volumes"]] == [0, 1] and doc["resample"] == 1
    for vid, a in enumerate(knowns):
        kept = np.isin(a, (1, 3))
        pred = read_nifti(str(tmp_path / "cls" / f"pred_{vid:04d}.nii.gz"))
        assert np.array_equal(pred[kept], a[kept]) and not np.array_equal(pred, a)
        assert np.array_equal(pred, read_nifti(str(tmp_path / "msk" / f"pred_{vid:04d}.nii.gz")))      # the same mask, given as a volume
        assert doc["volumes"][vid]["kept_differing"] == 0 and doc["volumes"][vid]["kept_fraction"] == kept.sum() / kept.size
        for j in range(2):
            assert np.array_equal(read_nifti(str(tmp_path / "s2" / f"pred_{vid:04d}_s{j:02d}.nii.gz"))[kept], a[kept])
    doc2 = json.loads((tmp_path / "s2" / "metrics.json").read_text())["edit"]
    assert all(v["kept_differing"] == 0 for v in doc2["volumes"]) and doc2["resample"] == 2
    with pytest.raises(ValueError, match="exactly one of --keep-classes"):
        ddpm_eval.main(common[:1] + ["bad"] + common[1:])
    with pytest.raises(ValueError, match="exactly one of --keep-classes"):
        ddpm_eval.main(common[:1] + ["bad"] + common[1:] + ["--keep-classes", "1", "--keep-mask", str(mdir)])
    with pytest.raises(ValueError, match="give --known DIR"):
        ddpm_eval.main([str(pf), "bad", "--size", "8", "8", "8", "--num-classes", str(K), "--keep-classes", "1"])
    with pytest.raises(ValueError, match=r"classes are 0\.\.5"):
        ddpm_eval.main(common[:1] + ["bad"] + common[1:] + ["--keep-classes", "1,6"])
