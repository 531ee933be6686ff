"""GPU suite (-m gpu): CT editing -- GuideGenPipeline.sample_ct_volumes(known_ct=, keep=), ct_keep_from_labels, edit_volumes,
`sample_diffusion --known-ct` -- and the three kernels under it (gg_ct_edit_glue, gg_minmax_normalise_keep_scatter, gg_label_keep_volume).

What is exact and what is bounded:
  * kernels: torch.equal to the torch CPU formulas (max_pool2d window rule of test_ct_edit_cpu, ops.minmax_normalise, the oracle's glue);
  * kept voxels, fully kept volumes, an un-edited volume beside an edited one, graph vs eager, a volume vs other neighbours: torch.equal;
  * a mixed slice vs the sampler's inpainting called by hand at the same batch size with the same operands: torch.equal;
  * un-kept pixels vs the CPU reference loop (tests/ct_edit_ref.py) on tapes: max abs < 6e-2, the bound of the un-edited loop's oracle
    comparison in test_volumes_gpu.py (bf16 networks against fp32 ones).  Measured on an MI355X: 1.21e-2 and 1.26e-2; by hand: 0.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ct_edit_ref as R
from test_full_size_configs import _small_ccdm, _small_ldm
from util import sd_cpu, small_ldm, synth_labels

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEPTH, HW, STEPS, FACTOR = 7, 32, 5, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pipe(dev):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    return GuideGenPipeline(_small_ccdm(dev), _small_ldm(dev), ddim_steps=STEPS)


def window_rule(keep2d, f, r):
    """The latent keep mask as max_pool2d of the un-kept pixels (== ct_edit_ref.latent_keep_mask, test_ct_edit_cpu)."""
    return 1.0 - F.max_pool2d((~keep2d.bool()).float()[None, None], kernel_size=f * (2 * r + 1), stride=f, padding=r * f)[0, 0]


# ------------------------------------------------------------------------------------------------ kernels
# (f, hw, r): every r in {0, 1, 2} at f = 4 / hw 32; f = 8 on the 2 x 2 latent of hw 16 admits r = 0 only (a wider window is refused), so
# r = 1, 2 at f = 8 run on hw 48 / 40 (at 40 the window is the whole image)
@pytest.mark.parametrize("f,hw,r", [(4, 32, 0), (4, 32, 1), (4, 32, 2), (8, 16, 0), (8, 48, 1), (8, 40, 2)])
def test_ct_edit_glue_equals_the_window_rule(dev, f, hw, r):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(10 * f + r)
    N, lat = 3, hw // f
    pats = [torch.ones(hw, hw, dtype=torch.bool), torch.zeros(hw, hw, dtype=torch.bool), torch.rand(hw, hw, generator=g) > 0.02]
    for y, x in ((0, 0), (0, hw - 1), (hw - 1, 0), (hw - 1, hw - 1), (f - 1, f), (f, f - 1), (f, f), (f - 1, f - 1)):
        k = torch.ones(hw, hw, dtype=torch.bool)
        k[y, x] = False                                                    # each image corner, each side of a cell boundary
        pats.append(k)
    D = len(pats)
    keep = torch.stack([torch.stack([pats[(d + 4 * n) % D] for n in range(N)]) for d in range(D)]).to(torch.uint8)      # [D, N, hw, hw]
    keep[keep != 0] = torch.randint(1, 256, (int((keep != 0).sum()),), generator=g, dtype=torch.int32).to(torch.uint8)  # any non-zero keeps
    known = torch.rand((D, N, hw, hw), generator=g)
    sched = torch.zeros((D + 1, N, 3), dtype=torch.int32)
    for it in range(D):
        for n in range(N):
            sched[it, n] = torch.tensor([(it + 2 * n) % D, 0, 0 if (it + n) % 3 == 2 else 1])     # three different slices, one row inactive
    sched[D] = torch.tensor([[D + 3, 0, 1], [-2, 0, 1], [0, 0, 1]])        # slices out of range are clamped, never read out of bounds
    keep_d, known_d, sched_d = keep.to(dev), known.to(dev), sched.to(dev)
    it_d = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in range(D + 1):
        it_d.fill_(it)
        img = torch.full((N, 1, hw, hw, 32), 5.0, dtype=torch.bfloat16, device=dev)
        lm = torch.full((N * lat * lat, 1), 5.0, device=dev)
        ops.ct_edit_glue(known_d, keep_d, sched_d, it_d, r, img, lm)
        img, lm = img.cpu(), lm.cpu().view(N, lat, lat)
        assert bool((img[..., 1:] == 0).all()), "pad lanes"
        for n in range(N):
            s, active = min(max(int(sched[it, n, 0]), 0), D - 1), bool(sched[it, n, 2])
            want_img = known[s, n].bfloat16() if active else torch.zeros(hw, hw, dtype=torch.bfloat16)
            want_lm = window_rule(keep[s, n], f, r) if active else torch.zeros(lat, lat)
            assert torch.equal(img[n, 0, :, :, 0], want_img), (it, n)
            assert torch.equal(lm[n], want_lm), (it, n)
    for bad in (-1, D + 1):                                                 # a counter outside the schedule writes nothing
        it_d.fill_(bad)
        img = torch.full((N, 1, hw, hw, 32), 5.0, dtype=torch.bfloat16, device=dev)
        lm = torch.full((N * lat * lat, 1), 5.0, device=dev)
        ops.ct_edit_glue(known_d, keep_d, sched_d, it_d, r, img, lm)
        assert bool((img == 5.0).all()) and bool((lm == 5.0).all())
    with pytest.raises(ValueError, match="margin"):
        ops.ct_edit_glue(known_d, keep_d, sched_d, it_d, (hw // f) // 2 + 1, img, lm)


@pytest.mark.parametrize("shape", [(64, 64), (33, 35)], ids=["rows-of-4", "odd"])
def test_minmax_normalise_keep_scatter(dev, shape):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(4)
    N, depth = 3, 6
    src = (torch.randn((N,) + shape, generator=g) * torch.tensor([1.0, 40.0, 1e-3]).view(N, 1, 1) + torch.tensor([0.0, -7.0, 3.0]).view(N, 1, 1)).to(dev)
    known = torch.rand((depth, N) + shape, generator=g).to(dev)
    keep = (torch.rand((depth, N) + shape, generator=g) > 0.5).to(torch.uint8).to(dev) * 3
    keep[0, 2] = 0                                                          # sample 2's slice: nothing kept
    sched = torch.tensor([[[2, 1, 1], [5, 4, 0], [0, 0, 1]]], dtype=torch.int32, device=dev)   # sample 1 inactive
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    vol = torch.full((depth, N) + shape, -1.0, device=dev)
    ops.minmax_normalise_keep_scatter(src, sched, it, known, keep, vol, advance=True)
    assert int(it[0]) == 1
    for n, s in ((0, 2), (2, 0)):
        k = keep[s, n] != 0
        norm = ops.minmax_normalise(src[n].contiguous())
        assert torch.equal(vol[s, n][k], known[s, n][k]), "kept pixels"
        assert torch.equal(vol[s, n][~k], norm[~k]), "generated pixels"
        assert int(k.sum()) > 0 or n == 2
    assert torch.equal(vol[0, 2], ops.minmax_normalise(src[2].contiguous()))
    touched = torch.zeros(depth, N, dtype=torch.bool)
    touched[2, 0] = touched[0, 2] = True
    assert bool((vol[~touched.to(dev)] == -1.0).all())                      # the inactive sample and every other slice untouched
    before = vol.clone()
    ops.minmax_normalise_keep_scatter(src, sched, it, known, keep, vol, advance=True)      # counter 1 is outside this 1-row schedule
    assert int(it[0]) == 2 and torch.equal(vol, before)
    ops.minmax_normalise_keep_scatter(src, sched, it, known, keep, vol, advance=False)
    assert int(it[0]) == 2


def test_label_keep_volume_equals_the_oracle_glue_on_both_volumes(dev):
    from jointimagegeneration_amd import ops
    from oracle import samplers as S
    g = torch.Generator().manual_seed(6)
    N, Dm, HWm = 2, 5, 16
    old = torch.randint(0, 12, (N, Dm, HWm, HWm), generator=g, dtype=torch.int32)
    new = old.clone()
    new[0, 1:3, 4:9, 2:7] = 11
    new[1, 4, :, 10:] = (old[1, 4, :, 10:] + 1) % 12
    new[1, 0, 0, 0] = (old[1, 0, 0, 0] + 5) % 12
    keep = ops.label_keep_volume(old.to(dev), new.to(dev), DEPTH, HW, HW).cpu()
    assert keep.shape == (DEPTH, N, HW, HW) and keep.dtype == torch.uint8
    for n in range(N):
        want = S.mask_to_cond_volume(new[n].long(), (DEPTH, HW, HW)) == S.mask_to_cond_volume(old[n].long(), (DEPTH, HW, HW))
        assert torch.equal(keep[:, n], want.to(torch.uint8))
        assert 0 < int(want.sum()) < want.numel()
    assert bool((ops.label_keep_volume(old.to(dev), old.to(dev), DEPTH, HW, HW) == 1).all())


# ------------------------------------------------------------------------------------------------ the loop at B = 2 (small configs)
def _small_labels(lo, hi, seed, Dm=5, HWm=16):
    lab = torch.zeros((Dm, HWm, HWm), dtype=torch.int32)
    lab[lo:hi] = torch.from_numpy(synth_labels((hi - lo, HWm, HWm), 12, seed=seed)).int()
    lab[lo:hi, 2:5, 2:5] = 7
    return lab


def _case(dev):
    """Two volumes: volume 0's window is slices 6, 0, 1, 2, 3 (wrap-around m = -1), volume 1's is 0 .. 6.  keep of volume 1: slices 0, 1,
    2, 6 kept whole (skipped), 3 and 5 mixed, 4 free."""
    g = torch.Generator().manual_seed(21)
    labels = torch.stack([_small_labels(0, 3, seed=2), _small_labels(1, 5, seed=3)]).to(dev)
    known = torch.rand((2, DEPTH, HW, HW), generator=g).to(dev)
    keep = torch.ones((2, DEPTH, HW, HW), dtype=torch.bool)
    keep[0] = False
    keep[1, 3, :, HW // 2:] = False
    keep[1, 4] = False
    keep[1, 5, 9:14, 17:22] = False
    return labels, known, keep.to(dev)


def test_slice_windows_of_the_case():
    from jointimagegeneration_amd.pipeline import slice_window
    assert slice_window(_small_labels(0, 3, seed=2), DEPTH) == [-1, 0, 1, 2, 3]
    assert slice_window(_small_labels(1, 5, seed=3), DEPTH) == [0, 1, 2, 3, 4, 5, 6]


def test_kept_voxels_come_back_and_the_stats_count_every_kind_of_slice(dev, pipe):
    labels, known, keep = _case(dev)
    ct = pipe.sample_ct_volumes(labels, DEPTH, HW, [4242, 77], known_ct=known, keep=keep, edit_margin=1)
    st = pipe.stats
    assert (st["slices_visited"], st["slices_skipped_kept"], st["slices_mixed"]) == (5 + 3, 4, 2)
    assert st["unkept_outside_window"] == 2 * HW * HW                       # volume 0's slices 4 and 5: un-kept, outside its window, stay 0
    assert ct.shape == (2, DEPTH, HW, HW)
    assert torch.equal(ct[keep], known[keep])
    assert float(ct[0, 4:6].abs().max()) == 0.0
    gen = ~keep
    gen[0, 4:6] = False
    for i, d in ((0, 6), (0, 0), (0, 3), (1, 3), (1, 4), (1, 5)):
        v = ct[i, d][gen[i, d]]
        assert float(v.min()) >= 0.0 and float(v.max()) <= 1.0 and float(v.max() - v.min()) > 0.0, (i, d)
        assert not torch.equal(v, known[i, d][gen[i, d]])
    # keep given as uint8 (any non-zero keeps) is the same call
    ct8 = pipe.sample_ct_volumes(labels, DEPTH, HW, [4242, 77], known_ct=known, keep=keep.to(torch.uint8) * 200, edit_margin=1)
    assert torch.equal(ct8, ct)


def test_fully_kept_volumes_come_back_exactly_without_an_iteration(dev, pipe):
    labels, known, keep = _case(dev)
    allk = torch.ones_like(keep)
    engines = list(pipe._volume_graphs)
    ct = pipe.sample_ct_volumes(labels, DEPTH, HW, [1, 2], known_ct=known, keep=allk, edit_margin=2)
    assert torch.equal(ct, known)
    assert (pipe.stats["slices_visited"], pipe.stats["slices_skipped_kept"], pipe.stats["slices_mixed"]) == (0, 12, 0)
    assert list(pipe._volume_graphs) == engines, "a fully kept batch built a slice engine"      # no margin-2 engine: nothing was launched
    k2 = keep.clone()
    k2[0] = True                                                            # volume 0 kept whole beside the edited volume 1
    ct = pipe.sample_ct_volumes(labels, DEPTH, HW, [1, 2], known_ct=known, keep=k2)
    assert torch.equal(ct[0], known[0]) and torch.equal(ct[1][k2[1]], known[1][k2[1]])
    assert (pipe.stats["slices_visited"], pipe.stats["slices_skipped_kept"], pipe.stats["slices_mixed"]) == (3, 5 + 4, 2)


def test_unedited_volume_beside_an_edited_one_is_its_plain_run_and_graph_equals_eager(dev, pipe):
    labels, known, keep = _case(dev)
    seeds = [4242, 77]
    res = {}
    try:
        for use_graph in (True, False):
            pipe.use_graph = pipe.sampler.use_graph = use_graph
            plain = pipe.sample_ct_volumes(labels, DEPTH, HW, seeds)
            edit = pipe.sample_ct_volumes(labels, DEPTH, HW, seeds, known_ct=known, keep=keep)
            again = pipe.sample_ct_volumes(labels, DEPTH, HW, seeds, known_ct=known, keep=keep)       # with graphs: the replayed one
            assert pipe.stats["slices_mixed"] == 2 and pipe.stats["slices_skipped_kept"] == 4
            assert torch.equal(edit[0], plain[0]), "all-zero keep: volume 0 differs from its un-edited run"
            assert torch.equal(again, edit)
            assert not torch.equal(edit[1], plain[1])
            res[use_graph] = edit
    finally:
        pipe.use_graph = pipe.sampler.use_graph = True
    assert torch.equal(res[True], res[False]), "graph != eager"
    ve = [v for k, v in pipe._volume_graphs.items() if ("edit", 0) in k]
    assert ve and all(v["graph"] is not None for v in ve), "the edited iteration did not run as one captured graph"


def test_edited_volume_is_independent_of_its_neighbour(dev, pipe):
    labels, known, keep = _case(dev)
    labels = labels.flip(0).contiguous()                                    # the edited volume in slot 0
    known, keep = known.flip(0).contiguous(), keep.flip(0).contiguous()
    g = torch.Generator().manual_seed(3)
    base = pipe.sample_ct_volumes(labels, DEPTH, HW, [77, 11], known_ct=known, keep=keep, edit_margin=1)
    assert pipe.stats["slices_mixed"] == 2
    others = []
    l2 = labels.clone(); l2[1] = _small_labels(2, 4, seed=9).to(dev)         # other labels (another window)
    others.append(dict(labels=l2, known=known, keep=keep, seeds=[77, 11]))
    k2 = known.clone(); k2[1] = torch.rand((DEPTH, HW, HW), generator=g).to(dev)
    others.append(dict(labels=labels, known=k2, keep=keep, seeds=[77, 11]))
    m2 = keep.clone(); m2[1] = (torch.rand((DEPTH, HW, HW), generator=g) > 0.3).to(dev)             # every slice of the neighbour mixed
    others.append(dict(labels=labels, known=known, keep=m2, seeds=[77, 11]))
    others.append(dict(labels=labels, known=known, keep=keep, seeds=[77, 12]))
    outs = []
    for o in others:
        outs.append(pipe.sample_ct_volumes(o["labels"], DEPTH, HW, o["seeds"], known_ct=o["known"], keep=o["keep"], edit_margin=1))
        assert torch.equal(outs[-1][0], base[0]), "volume 0 depends on its neighbour"
    assert not torch.equal(outs[2][1], base[1]) and not torch.equal(outs[3][1], base[1])            # the neighbour's operands are used


def test_mixed_slice_equals_the_samplers_inpainting_by_hand(dev, pipe):
    """One mixed slice per volume, both in iteration 0, x_T and q-noise from tapes: the loop's slices == DDIMSampler.sample(mask=, x0=,
    x_T=, mask_noise_tape=) at B = 2 on the same operands, decode_first_stage, ops.minmax_normalise, composite."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler
    ldm = pipe.ldm
    labels, known, _ = _case(dev)
    r, lat, Cz = 1, HW // FACTOR, 4
    sl = [1, 3]                                                             # the one visited slice of each volume; previous slices 0 and 2 are kept
    keep = torch.ones((2, DEPTH, HW, HW), dtype=torch.bool, device=dev)
    keep[0, 1, 3:20, 8:11] = False
    keep[1, 3, :, HW // 2:] = False
    g = torch.Generator().manual_seed(31)
    x_T = torch.randn((2, Cz, lat, lat), generator=g)
    q = torch.randn((2, STEPS, 1, Cz, lat, lat), generator=g)
    ct = pipe.sample_ct_volumes(labels, DEPTH, HW, [0, 0], known_ct=known, keep=keep, edit_margin=r,
                                x_T_tapes=[[x_T[i:i + 1]] for i in range(2)], q_noise_tapes=[[q[i]] for i in range(2)])
    assert (pipe.stats["slices_visited"], pipe.stats["slices_mixed"]) == (2, 2)
    mask_slices = torch.empty((2, HW, HW), device=dev)
    scratch = torch.empty((1, 1, HW, HW, 32), dtype=torch.bfloat16, device=dev)
    for i in range(2):
        ops.mask_to_cond_slice(labels[i:i + 1].contiguous(), sl[i], DEPTH, HW, HW, None, scratch, mask_out=mask_slices[i])
    concat_cond = torch.stack([torch.stack([known[i, sl[i] - 1], mask_slices[i]]) for i in range(2)])
    c = ldm.get_learned_conditioning(concat_cond)
    known_sl = torch.stack([known[i, sl[i]] for i in range(2)])[:, None].contiguous()
    x0 = ldm.scale_factor * ldm.first_stage_model.encode(known_sl).mode()
    lm = torch.stack([window_rule(keep[i, sl[i]].cpu(), FACTOR, r) for i in range(2)])[:, None].to(dev)
    assert 0 < float(lm.sum()) < lm.numel()
    sampler = DDIMSampler(ldm)
    z, _ = sampler.sample(S=STEPS, batch_size=2, shape=(Cz, lat, lat), conditioning=c, eta=0.0, verbose=False, mask=lm, x0=x0, x_T=x_T.to(dev),
                          mask_noise_tape=[q[:, s, 0].to(dev) for s in range(STEPS)])
    ds = ldm.decode_first_stage(z)
    for i in range(2):
        norm = ops.minmax_normalise(ds[i, 0].contiguous())
        want = torch.where(keep[i, sl[i]], known[i, sl[i]], norm)
        err = float((ct[i, sl[i]] - want).abs().max())
        print(f"volume {i}, mixed slice {sl[i]}: loop vs the sampler's inpainting by hand: max abs {err:.3e}")
        assert torch.equal(ct[i, sl[i]], want)


def test_edited_loop_vs_the_cpu_reference_on_tapes(dev):
    """Un-kept pixels against tests/ct_edit_ref.py (fp32 oracle networks) within the bound of the un-edited loop's oracle comparison
    (test_ldm_volumes_vs_solo_sample_ct_and_oracle: 6e-2); kept pixels exact."""
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    ml = small_ldm().to(dev)
    p = GuideGenPipeline(None, ml, ddim_steps=STEPS)
    r, lat = 1, HW // FACTOR
    g = torch.Generator().manual_seed(41)
    labs, keeps = [], []
    for seed, (lo, hi) in ((5, (1, 6)), (6, (1, 5))):
        lab = torch.zeros((DEPTH, HW, HW), dtype=torch.int64)
        lab[lo:hi] = torch.from_numpy(synth_labels((hi - lo, HW, HW), 12, seed=seed))
        lab[lo:hi, 4:9, 4:9] = 7
        labs.append(lab)
    known = torch.rand((2, DEPTH, HW, HW), generator=g)
    keep = torch.ones((2, DEPTH, HW, HW), dtype=torch.bool)
    keep[0, 0] = False                                                      # volume 0: window 0 .. 5; 0 free, 1 kept, 2 mixed, 3 free, 4 mixed, 5 kept
    keep[0, 2, 8:24, 8:24] = False
    keep[0, 3] = False
    keep[0, 4, :, :13] = False
    keep[1, 1, 20:, :] = False                                              # volume 1: window 0 .. 4; 0 kept, 1 mixed, 2 kept, 3 free, 4 mixed
    keep[1, 3] = False
    keep[1, 4, 5, 5] = False
    n_vis, n_mix = [4, 3], [2, 2]
    xs = [[torch.randn(1, 4, lat, lat, generator=g) for _ in range(n)] for n in n_vis]
    qs = [[torch.randn(STEPS, 1, 4, lat, lat, generator=g) for _ in range(n)] for n in n_mix]
    labels = torch.stack([torch.rot90(v, k=1, dims=(1, 2)) for v in labs]).int().contiguous().to(dev)
    ct = p.sample_ct_volumes(labels, DEPTH, HW, [0, 0], known_ct=known.to(dev), keep=keep.to(dev), edit_margin=r, x_T_tapes=xs, q_noise_tapes=qs).cpu()
    assert (p.stats["slices_visited"], p.stats["slices_skipped_kept"], p.stats["slices_mixed"]) == (7, 4, 4)
    sd = sd_cpu(ml)
    for i in range(2):
        whole = (labs[i].float() / 255.0)[None, None]
        ref = R.edited_slices_on_state_dict(sd, whole, known[i], keep[i], xs[i], qs[i], STEPS, ml.alphas_cumprod.cpu(), 32, FACTOR, r,
                                            scale_factor=float(ml.scale_factor))[0, 0]
        assert torch.equal(ct[i][keep[i]], ref[keep[i]]) and torch.equal(ct[i][keep[i]], known[i][keep[i]])
        err = float((ct[i] - ref)[~keep[i]].abs().max())
        print(f"volume {i}: edited loop vs the CPU reference over {int((~keep[i]).sum())} un-kept pixels: max abs {err:.3e}")
        assert err < 6e-2


# ------------------------------------------------------------------------------------------------ refusals
def test_host_refusals_by_name_before_any_launch(dev, pipe, monkeypatch):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import PLMSSampler
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    labels, known, keep = _case(dev)

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched before the refusal")
    for name in ("ct_edit_glue", "mask_to_cond_slices", "minmax_normalise_keep_scatter"):
        monkeypatch.setattr(ops, name, no_launch)
    call = lambda **kw: pipe.sample_ct_volumes(labels, DEPTH, HW, [1, 2], **kw)
    with pytest.raises(ValueError, match="known_ct= and keep= go together"):
        call(known_ct=known)
    with pytest.raises(ValueError, match="known_ct= and keep= go together"):
        call(keep=keep)
    with pytest.raises(ValueError, match="give known_ct"):
        call(edit_margin=1)
    with pytest.raises(ValueError, match="known_ct must be an fp32"):
        call(known_ct=known[:, :-1], keep=keep)
    with pytest.raises(ValueError, match="known_ct must be an fp32"):
        call(known_ct=known.double(), keep=keep)
    with pytest.raises(ValueError, match="keep must be a bool or uint8"):
        call(known_ct=known, keep=keep.float())
    with pytest.raises(ValueError, match="keep must be a bool or uint8"):
        call(known_ct=known, keep=keep[:1])
    for bad in (known + 0.5, known - 0.5, torch.full_like(known, float("nan"))):
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            call(known_ct=bad, keep=keep)
    with pytest.raises(ValueError, match="edit_margin must be an int >= 0"):
        call(known_ct=known, keep=keep, edit_margin=-1)
    with pytest.raises(ValueError, match="wider than the 32 x 32 slice"):
        call(known_ct=known, keep=keep, edit_margin=4)                      # 4 * 9 = 36 > 32
    with pytest.raises(ValueError, match="q_noise_tapes holds 1 lists"):
        call(known_ct=known, keep=keep, q_noise_tapes=[[]])
    with pytest.raises(ValueError, match=r"q_noise_tapes\[1\] holds 1 tensors, volume 1 has 2 mixed slices"):
        call(known_ct=known, keep=keep, q_noise_tapes=[[], [torch.zeros(STEPS, 1, 4, 8, 8)]])
    with pytest.raises(ValueError, match=r"q_noise_tapes\[1\]\[0\] has shape"):
        call(known_ct=known, keep=keep, q_noise_tapes=[[], [torch.zeros(STEPS, 4, 8, 8)] * 2])
    with pytest.raises(ValueError, match=r"x_T_tapes\[0\] holds 1 tensors, volume 0 visits 5 slices"):
        call(known_ct=known, keep=keep, x_T_tapes=[[torch.zeros(1, 4, 8, 8)], []])
    ldm = pipe.ldm
    ldm.split_input_params = dict(ks=(4, 4), stride=(2, 2), vqf=4)
    try:
        with pytest.raises(NotImplementedError, match="split_input_params"):
            call(known_ct=known, keep=keep)
    finally:
        del ldm.split_input_params
    monkeypatch.setattr(ldm, "dims", 3)
    with pytest.raises(NotImplementedError, match="3-D latents"):
        call(known_ct=known, keep=keep)
    monkeypatch.setattr(ldm, "dims", 2)
    monkeypatch.setattr(ldm.model, "conditioning_key", "crossattn")
    with pytest.raises(NotImplementedError, match="conditioning_key 'concat'"):
        call(known_ct=known, keep=keep)
    monkeypatch.setattr(ldm.model, "conditioning_key", "concat")
    other = GuideGenPipeline(None, ldm, ddim_steps=STEPS)
    other.sampler = PLMSSampler(ldm)
    other.sampler.make_schedule(STEPS, ddim_eta=0.0, verbose=False)
    with pytest.raises(NotImplementedError, match="DDIM sampler at eta = 0, got PLMSSampler"):
        other.sample_ct_volumes(labels, DEPTH, HW, [1, 2], known_ct=known, keep=keep)
    other = GuideGenPipeline(None, ldm, ddim_steps=STEPS)
    other.sampler.make_schedule(STEPS, ddim_eta=0.5, verbose=False)
    with pytest.raises(NotImplementedError, match="DDIM sampler at eta = 0"):
        other.sample_ct_volumes(labels, DEPTH, HW, [1, 2], known_ct=known, keep=keep)


# ------------------------------------------------------------------------------------------------ entry points
def test_sample_diffusion_known_ct_writes_the_volumes_and_the_edit_block(dev, tmp_path, monkeypatch):
    from jointimagegeneration_amd import sample_diffusion as sd
    from jointimagegeneration_amd.io import read_nifti, write_nifti
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    model = _small_ldm(dev)
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (model, 3))
    monkeypatch.chdir(tmp_path)
    for d in ("new", "old", "ct", "keep"):
        (tmp_path / d).mkdir()
    g = torch.Generator().manual_seed(51)
    knowns = {}
    for stem, (lo, hi), seed in (("pred_0000", (1, 5), 3), ("pred_0001", (0, 3), 2)):
        old = _small_labels(lo, hi, seed=seed)
        new = old.clone()
        new[2, 6:12, 6:12] = 3                                              # the edit: one organ on mask slice 2
        knowns[stem] = torch.rand((DEPTH, HW, HW), generator=g)
        write_nifti(str(tmp_path / "old" / f"{stem}.nii.gz"), old.numpy().astype(np.uint8))
        write_nifti(str(tmp_path / "new" / f"{stem}.nii.gz"), new.numpy().astype(np.uint8))
        write_nifti(str(tmp_path / "ct" / f"{stem}.nii.gz"), knowns[stem].numpy())
        k = np.ones((DEPTH, HW, HW), dtype=np.uint8)
        k[3, 8:20, 8:20] = 0
        write_nifti(str(tmp_path / "keep" / f"{stem}.nii.gz"), k)
    common = ["--config", str(tmp_path / "m.yaml"), "--inputs", str(tmp_path / "new"), "--slices", str(DEPTH), "--size", str(HW), "-c", str(STEPS),
              "--known-ct", str(tmp_path / "ct")]
    sd.main(common + ["--known-mask", str(tmp_path / "old"), "--edit-margin", "1"])
    out = tmp_path / "samples" / "00000003"
    doc = json.loads((out / "metrics.json").read_text())["edit"]
    assert doc["edit_margin"] == 1 and [v["volume"] for v in doc["volumes"]] == ["pred_0000", "pred_0001"]
    from jointimagegeneration_amd import ops
    for v in doc["volumes"]:
        stem = v["volume"]
        assert v["kept_max_abs_diff"] == 0 and 0.5 < v["kept_fraction"] < 1.0
        assert v["slices_mixed"] >= 1 and v["slices_skipped_kept"] >= 1 and v["slices_visited"] == v["slices_mixed"]
        ct = torch.from_numpy(np.ascontiguousarray(read_nifti(str(out / f"{stem}_0000.nii.gz"))))
        old = torch.from_numpy(np.ascontiguousarray(read_nifti(str(tmp_path / "old" / f"{stem}.nii.gz")))).int()[None].to(dev)
        new = torch.from_numpy(np.ascontiguousarray(read_nifti(str(tmp_path / "new" / f"{stem}.nii.gz")))).int()[None].to(dev)
        k = ops.label_keep_volume(old, new, DEPTH, HW, HW)[:, 0].cpu() != 0
        assert ct.shape == (DEPTH, HW, HW) and torch.equal(ct[k], knowns[stem][k]) and not torch.equal(ct[~k], knowns[stem][~k])
    sd.main(common + ["--keep-mask", str(tmp_path / "keep"), "-l", str(tmp_path / "explicit")])
    doc = json.loads((tmp_path / "explicit" / "samples" / "00000003" / "metrics.json").read_text())["edit"]
    assert [(v["slices_visited"], v["slices_mixed"], v["kept_max_abs_diff"]) for v in doc["volumes"]] == [(1, 1, 0), (1, 1, 0)]
    for flags, msg in ((["--known-mask", "old", "--keep-mask", "keep"], "exactly one"), ([], "exactly one"), (["--known-mask", "old", "-v"], "vanilla_sample"),
                       (["--known-mask", "old", "--plms"], "--plms"), (["--known-mask", "old", "-e", "0.5"], "eta = 0.5"),
                       (["--known-mask", "old", "-n", "2"], "n_samples = 2"), (["--known-mask", "old", "--edit-margin", "-1"], "edit-margin")):
        with pytest.raises(SystemExit, match=msg):
            sd.main(common + flags)
    with pytest.raises(SystemExit, match="give --known-ct"):
        sd.main(common[:-2] + ["--edit-margin", "1"])
    model.no_first_stage = True
    try:
        with pytest.raises(SystemExit, match="without a first stage"):
            sd.main(common + ["--known-mask", "old"])
    finally:
        model.no_first_stage = False
    with pytest.raises(SystemExit, match="nothing is resampled"):
        sd.main(common[:4] + ["--slices", "6", "--size", str(HW), "-c", str(STEPS), "--known-ct", "ct", "--known-mask", "old"])


def test_edit_volumes_end_to_end_with_the_small_ccdm(dev, pipe):
    K, size = 6, (8, 8, 8)
    g = torch.Generator().manual_seed(61)
    known_labels = torch.randint(0, K, (2,) + size, generator=g, dtype=torch.int32).to(dev)
    known_ct = torch.rand((2, DEPTH, HW, HW), generator=g).to(dev)
    labels, ct, ct_keep = pipe.edit_volumes(known_labels, known_ct, [4242, 77], keep_classes=[0, 1, 2, 3], edit_margin=1)
    kept = torch.isin(known_labels, torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev))
    assert torch.equal(labels[kept], known_labels[kept]), "labels outside the edited classes changed"
    assert bool((labels[~kept] != known_labels[~kept]).any())
    assert torch.equal(ct_keep, pipe.ct_keep_from_labels(known_labels, labels, DEPTH, HW)) and ct_keep.shape == known_ct.shape
    k = ct_keep != 0
    assert 0 < int(k.sum()) < k.numel()
    assert torch.equal(ct[k], known_ct[k]), "CT voxels under unchanged labels changed"
    assert not torch.equal(ct[~k], known_ct[~k])
    assert pipe.stats["slices_visited"] >= 1 and pipe.stats["slices_mixed"] >= 1 and "ldm_s" in pipe.stats
    with pytest.raises(ValueError, match="exactly one of label_keep"):
        pipe.edit_volumes(known_labels, known_ct, [1, 2])
