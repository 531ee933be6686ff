"""GPU suite (-m gpu): batches of independent volumes (GuideGenPipeline.run_volumes / sample_masks / sample_ct_volumes) and the kernels
under them -- the per-sample Philox key of the CCDM reverse step (stand-alone kernel and fused head-conv epilogue), the batched stage
glue and the per-sample min-max normalise + scatter.

What is exact and what is bounded:
  * kernels: bit-equal to their per-sample / solo counterparts;
  * a volume of a batch vs the same batch with other neighbours (other masks, window lengths, seeds): bit-equal;
  * a volume of a batch vs its solo run: bf16 rounding only (kernel plans depend on the grid size), bounded and printed.  Measured on
    an MI355X: small LDM configs 0 (same plans at B = 1 and 2); C5 shapes, 3 slices: max abs 7.2e-3 (bound 2e-2, the solo-vs-reference
    tolerance); with x_T tapes vs the oracle's slice loop: 1.5e-2 (bound 6e-2, as the solo B8 tests); CCDM 128^3, 5 steps: 2.8 % of
    the labels (bound 4 %, as the existing batch-independence test), 8^3: 0.
"""
import math

import pytest
import torch

from test_full_size_configs import _full_ccdm, _small_ccdm, _small_ldm
from util import SEED, T, gold, sd_cpu, synth_labels

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


SEEDS = [4242, (1 << 40) + 17, (1 << 63) + 5]          # the last one has the top bit set (uint64 key through an int64 tensor)


# ------------------------------------------------------------------------------------------------ per-sample Philox key
@pytest.mark.parametrize("K", [14, 6])
def test_posterior_per_sample_key_equals_solo_calls(dev, K):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(3)
    N, R = 3, 4096 + 64
    M = N * R
    head = (2 * torch.randn(M, 32, generator=g)).to(dev)
    xt = torch.randint(0, K, (M,), generator=g, dtype=torch.int32).to(dev)
    scal = torch.tensor([0.93, 0.37], dtype=torch.float32, device=dev)
    off = torch.tensor([57], dtype=torch.int64, device=dev)
    seeds = ops.philox_seed_tensor(SEEDS, dev)
    lab = torch.empty(M, dtype=torch.int32, device=dev)
    oh = torch.zeros((M, 32), dtype=torch.bfloat16, device=dev)
    ops.ccdm_posterior_sample(head, True, xt, scal, K, philox_offset=off, labels_out=lab, onehot_out=oh, philox_seeds=seeds)
    for i in range(N):
        rows = slice(i * R, (i + 1) * R)
        li = torch.empty(R, dtype=torch.int32, device=dev)
        ohi = torch.zeros((R, 32), dtype=torch.bfloat16, device=dev)
        ops.ccdm_posterior_sample(head[rows].contiguous(), True, xt[rows].contiguous(), scal, K, philox_offset=off, labels_out=li,
                                  onehot_out=ohi, philox_seeds=seeds[i:i + 1].contiguous())
        assert torch.equal(lab[rows], li), f"sample {i}: per-sample key depends on the batch slot"
        assert torch.equal(oh[rows], ohi)
        assert (li != xt[rows]).float().mean() > 0.05
    # at N = 1 the per-sample mode IS the single-key mode
    for s in SEEDS:
        a = ops.ccdm_posterior_sample(head[:R].contiguous(), True, xt[:R].contiguous(), scal, K, philox_seed=s, philox_offset=off)
        b = ops.ccdm_posterior_sample(head[:R].contiguous(), True, xt[:R].contiguous(), scal, K, philox_offset=off,
                                      philox_seeds=ops.philox_seed_tensor([s], dev))
        assert torch.equal(a, b)
    # different keys draw differently (the key is really used)
    c = ops.ccdm_posterior_sample(head[:R].contiguous(), True, xt[:R].contiguous(), scal, K, philox_offset=off,
                                  philox_seeds=ops.philox_seed_tensor([SEEDS[0] + 1], dev))
    assert not torch.equal(c, lab[:R])


def test_fused_head_conv_per_sample_key_equals_standalone_kernel(dev, monkeypatch):
    """The fused epilogue (1024-position 3-D halo box) with per-sample keys == conv then the stand-alone kernel with per-sample keys, at
    the shape of test_head_conv_with_fused_ccdm_reverse_step_equals_conv_then_sampler_kernel with two samples; and at N = 1 the per-sample
    fused mode == the single-key fused mode."""
    from jointimagegeneration_amd import ops
    monkeypatch.setattr(ops, "PATH_HINT", 6)
    K, Cin, sp, N = 14, 64, (16, 16, 32), 2
    R = sp[0] * sp[1] * sp[2]
    M = N * R
    g = torch.Generator().manual_seed(77)
    x = ops.CL(torch.randn((N,) + sp + (Cin,), generator=g).to(dev).bfloat16(), Cin)
    w = (torch.randn(K, Cin, 3, 3, 3, generator=g) * (3.0 / math.sqrt(Cin * 27))).to(dev)
    pw = ops.pack_conv_weight(w, Cin)
    bias = torch.zeros(N, 32, device=dev); bias[:, :K] = torch.randn(N, K, generator=g).to(dev) * 0.3
    gamma, beta = (1 + 0.1 * torch.randn(Cin, generator=g)).to(dev), (0.1 * torch.randn(Cin, generator=g)).to(dev)
    prol = ops.groupnorm_stats(x, gamma, beta, 1e-5)
    xt = torch.randint(0, K, (M,), generator=g, dtype=torch.int32).to(dev)
    scal = torch.tensor([0.97, 0.41], dtype=torch.float32, device=dev)
    off = torch.tensor([123], dtype=torch.int64, device=dev)
    seeds = ops.philox_seed_tensor(SEEDS[:N], dev)
    kw = dict(k=(3, 3, 3), out_f32=True, prologue=prol, bias_per_sample=True)

    logits = ops.conv(x, pw, bias, K, **kw).t
    lab_a = torch.empty(M, dtype=torch.int32, device=dev)
    oh_a = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev)
    ops.ccdm_posterior_sample(logits.view(M, -1), True, xt, scal, K, philox_offset=off, labels_out=lab_a, onehot_out=oh_a, philox_seeds=seeds)
    lab_b = xt.clone()
    oh_b = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev)
    y = ops.conv(x, pw, bias, K, out=torch.empty_like(logits),
                 post=dict(xt=lab_b, scalars=scal, K=K, philox_offset=off, draw=True, labels_out=lab_b, onehot_out=oh_b, philox_seeds=seeds), **kw)
    assert y.fused_post
    assert torch.equal(lab_a, lab_b) and torch.equal(oh_a, oh_b)
    assert (lab_b != xt).float().mean() > 0.02
    # the sample in slot 1 draws as it would alone in slot 0 (stand-alone kernel, N = 1, its own rows)
    l1 = ops.ccdm_posterior_sample(logits.view(M, -1)[R:].contiguous(), True, xt[R:].contiguous(), scal, K, philox_offset=off,
                                   philox_seeds=seeds[1:].contiguous())
    assert torch.equal(l1, lab_b[R:])
    # N = 1: fused per-sample == fused single key
    x1 = ops.CL(x.t[:1].contiguous(), Cin)
    prol1 = ops.groupnorm_stats(x1, gamma, beta, 1e-5)
    kw1 = dict(kw, prologue=prol1)
    outs = []
    for extra in (dict(philox_seed=SEEDS[2]), dict(philox_seeds=ops.philox_seed_tensor([SEEDS[2]], dev))):
        lab = xt[:R].clone()
        y1 = ops.conv(x1, pw, bias[:1].contiguous(), K, out=torch.empty_like(logits[:1]),
                      post=dict(xt=lab, scalars=scal, K=K, philox_offset=off, draw=True, labels_out=lab, **extra), **kw1)
        assert y1.fused_post
        outs.append(lab)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ batched glue, normalise + scatter
def _glue_case(dev, N, Dm, HW, depth, hw, seed):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 14, (N, Dm, HW, HW), generator=g, dtype=torch.int32).to(dev)
    volume = torch.rand((depth, N, hw, hw), generator=g).to(dev)
    iters = 4
    sched = torch.stack([torch.randint(0, depth, (iters, N), generator=g), torch.randint(0, depth, (iters, N), generator=g),
                         torch.randint(0, 2, (iters, N), generator=g)], -1).int()
    sched[0, :, 0], sched[0, :, 1] = depth - 1, 0                        # the wrap-around row of a mask non-empty on slice 0
    sched_d = sched.to(dev)
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(iters):
        it.fill_(i)
        cond = torch.full((N, 1, hw, hw, 32), 5.0, dtype=torch.bfloat16, device=dev)
        ops.mask_to_cond_slices(labels, depth, hw, hw, sched_d, it, volume, cond)
        for n in range(N):
            want = torch.full((1, 1, hw, hw, 32), 5.0, dtype=torch.bfloat16, device=dev)
            s, p = int(sched[i, n, 0]), int(sched[i, n, 1])
            ops.mask_to_cond_slice(labels[n:n + 1].contiguous(), s, depth, hw, hw, volume[p, n].contiguous(), want)
            assert torch.equal(cond[n:n + 1], want), (i, n)
    it.fill_(iters)                                                       # beyond the schedule: nothing is written
    cond = torch.full((N, 1, hw, hw, 32), 5.0, dtype=torch.bfloat16, device=dev)
    ops.mask_to_cond_slices(labels, depth, hw, hw, sched_d, it, volume, cond)
    assert bool((cond == 5.0).all())


def test_batched_glue_equals_per_sample_glue_small(dev):
    _glue_case(dev, 3, 5, 16, 7, 32, seed=1)


def test_batched_glue_equals_per_sample_glue_full_size(dev):
    _glue_case(dev, 2, 128, 128, 256, 512, seed=2)


def test_segmented_minmax_normalise_scatter(dev):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(4)
    N, hw, depth = 3, 512, 6
    src = (torch.randn(N, hw, hw, generator=g) * torch.tensor([1.0, 40.0, 1e-3]).view(N, 1, 1)
           + torch.tensor([0.0, -7.0, 3.0]).view(N, 1, 1)).to(dev)
    sched = torch.tensor([[[2, 1, 1], [5, 4, 0], [0, 0, 1]]], dtype=torch.int32, device=dev)   # sample 1 inactive
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    vol = torch.full((depth, N, hw, hw), -1.0, device=dev)
    ops.minmax_normalise_scatter(src, sched, it, vol, advance=True)
    assert int(it[0]) == 1
    for n, s in ((0, 2), (2, 0)):
        assert torch.equal(vol[s, n], ops.minmax_normalise(src[n].contiguous()))
    touched = torch.zeros(depth, N, dtype=torch.bool)
    touched[2, 0] = touched[0, 2] = True
    assert bool((vol[~touched.to(dev)] == -1.0).all())                   # inactive sample and every other slice untouched
    ops.minmax_normalise_scatter(src, sched, it, vol, advance=True)      # counter 1 is outside this 1-row schedule: no write
    assert int(it[0]) == 2 and bool((vol[~touched.to(dev)] == -1.0).all())


# ------------------------------------------------------------------------------------------------ the warm / capture / replay ladder
def test_replay_captured_runs_eagerly_once_captures_once_then_replays(dev):
    """ops.replay_captured on its own: the body runs twice in Python (the eager call and the capture), every call computes on the buffers'
    current contents, and the graph of the second call is the one every later call replays."""
    from jointimagegeneration_amd import ops
    a = torch.empty(1024, dtype=torch.float32, device=dev)
    out = torch.zeros_like(a)
    calls = [0]

    def body():
        calls[0] += 1
        ops.lincomb4([a], [2.0], 1.0, out)

    holder = dict(warmed=False, graph=None)
    graphs = []
    for k in range(4):
        a.copy_(torch.randn(1024, generator=torch.Generator().manual_seed(100 + k)))
        ops.replay_captured(holder, "graph", body)
        assert torch.equal(out, 2 * a), f"call {k}"
        graphs.append(holder["graph"])
    assert calls[0] == 2 and holder["warmed"] is True
    assert graphs[0] is None and isinstance(graphs[1], torch.cuda.CUDAGraph) and graphs[3] is graphs[1]


# ------------------------------------------------------------------------------------------------ LDM stage at B = 2 (small configs)
def _small_labels(lo, hi, seed, Dm=5, HW=16):
    lab = torch.zeros((Dm, HW, HW), dtype=torch.int32)
    lab[lo:hi] = torch.from_numpy(synth_labels((hi - lo, HW, HW), 12, seed=seed)).int()
    lab[lo:hi, 2:5, 2:5] = 7
    return lab


def test_ldm_volume_independent_of_its_neighbour_graph_and_eager(dev):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    pipe = GuideGenPipeline(_small_ccdm(dev), _small_ldm(dev), ddim_steps=5)
    depth, hw = 7, 32
    v0 = _small_labels(0, 3, seed=2)                                      # non-empty on slice 0: wrap-around m = -1
    neighbours = [(_small_labels(1, 5, seed=3), 11), (_small_labels(2, 3, seed=4), 11), (_small_labels(0, 5, seed=5), 11),
                  (_small_labels(1, 5, seed=3), 12)]                      # reference, shorter window, longer window, other seed
    results = {}
    for use_graph in (True, False):
        pipe.use_graph = pipe.sampler.use_graph = use_graph
        cts = []
        for lab1, s1 in neighbours:
            labels = torch.stack([v0, lab1]).to(dev)
            cts.append(pipe.sample_ct_volumes(labels, depth, hw, [4242, s1]))
        for c in cts[1:]:
            assert torch.equal(c[0], cts[0][0]), "volume 0 depends on its neighbour"
        assert not torch.equal(cts[0][1], cts[3][1])                      # the neighbour's own seed is used
        results[use_graph] = cts
    for a, b in zip(results[True], results[False]):
        assert torch.equal(a, b), "graph != eager"
    print(f"LDM B = 2: volume 0 bit-equal under 3 other neighbours, graph == eager; wasted slots of the last batch "
          f"{pipe.stats['wasted_slot_fraction']:.3f}")


def test_ldm_volumes_vs_solo_sample_ct_and_oracle(dev):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    from util import oracle_slice_loop, small_ldm
    depth, hw = 7, 32
    m = _small_ldm(dev)
    pipe = GuideGenPipeline(_small_ccdm(dev), m, ddim_steps=5)
    vols = [_small_labels(0, 3, seed=2), _small_labels(1, 5, seed=3)]
    seeds = [4242, 77]
    ct = pipe.sample_ct_volumes(torch.stack(vols).to(dev), depth, hw, seeds)
    assert ct.shape == (2, depth, hw, hw)
    for i in range(2):
        solo = pipe.sample_ct(vols[i][None].to(dev), depth, hw, seeds[i])
        gen_b = (ct[i].flatten(1).abs().amax(1) > 0).cpu()
        gen_s = (solo[0].flatten(1).abs().amax(1) > 0).cpu()
        assert torch.equal(gen_b, gen_s) and int(gen_b.sum()) >= 3
        assert float(ct[i].abs().flatten(1).amax(1)[~gen_b.to(dev)].sum()) == 0.0     # untouched slices exactly zero
        err = float((ct[i] - solo[0]).abs().max())
        print(f"volume {i}: batched (B = 2) vs solo sample_ct: max abs {err:.3e} over {int(gen_b.sum())} slices")
        assert err < 2e-2
    # x_T tapes: each volume against the oracle's slice loop run on that volume alone (fixture-sized small LDM)
    g = gold("autoreg_small")
    lab = T(g["labels"]).long()                                           # [11, 32, 32], slice 0 empty
    S_steps = int(g["ddim_steps"])
    ml = small_ldm().to(dev)
    pipe = GuideGenPipeline(_small_ccdm(dev), ml, ddim_steps=S_steps)
    lab1 = lab.clone(); lab1[7:] = 0                                      # a shorter window
    gx = torch.Generator().manual_seed(8)
    xT0 = list(T(g["x_T"]).float())
    tapes = [xT0, [torch.randn(xT0[0].shape, generator=gx) for _ in range(7)]]
    labels = torch.stack([torch.rot90(v, k=1, dims=(1, 2)) for v in (lab, lab1)]).int().contiguous().to(dev)
    ct = pipe.sample_ct_volumes(labels, lab.shape[0], 32, [0, 0], x_T_tapes=tapes)
    for i, v in enumerate((lab, lab1)):
        whole = (v.float() / 255.0)[None, None]
        ref = oracle_slice_loop(sd_cpu(ml), whole, tapes[i], S_steps, ml.alphas_cumprod.cpu(), 32)[:, 0]
        err = float((ct[i].cpu() - ref[0]).abs().max())
        print(f"volume {i} with its x_T tape vs the oracle slice loop run alone: max abs {err:.3e}")
        assert err < 6e-2


# ------------------------------------------------------------------------------------------------ CCDM stage
def test_ccdm_masks_independent_of_the_neighbour_seed(dev):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    for full in (False, True):                                            # small: stand-alone kernel; 128^3: the fused head-conv epilogue
        if full:
            ccdm, _, _ = _full_ccdm(dev, 250)
            size, init_t = (128, 128, 128), 10005
        else:
            ccdm, size, init_t = _small_ccdm(dev, T_steps=8), (8, 8, 8), None
        pipe = GuideGenPipeline(ccdm, _small_ldm(dev), ddim_steps=5)
        a = pipe.sample_masks([SEEDS[0], 11], size, init_t)
        b = pipe.sample_masks([SEEDS[0], 12], size, init_t)
        assert torch.equal(a[0], b[0]), "mask 0 depends on its neighbour's seed"
        assert not torch.equal(a[1], b[1])
        solo = pipe.sample_mask(1, size, SEEDS[0], init_t)
        mism = float((solo[0] != a[0]).float().mean())
        print(f"CCDM {size}, B = 2 vs solo sample_mask: {mism:.5f} of the labels differ (kernel plans of the two grid sizes)")
        assert mism < 0.04
        if full:
            del ccdm, pipe
            torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ C5 shapes
def test_full_size_b2_first_slices_vs_solo(dev):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline, build_ldm
    pipe = GuideGenPipeline(_small_ccdm(dev), build_ldm(SEED, dev), ddim_steps=50)
    vols = []
    for lo, hi, s in ((10, 100, 1), (0, 40, 2)):
        lab = torch.zeros((128, 128, 128), dtype=torch.int32)
        lab[lo:hi] = torch.from_numpy(synth_labels((hi - lo, 128, 128), 12, seed=s)).int()
        vols.append(lab)
    seeds = [5, 6]
    ct = pipe.sample_ct_volumes(torch.stack(vols).to(dev), 256, 512, seeds, max_slices=3)
    for i in range(2):
        solo = pipe.sample_ct(vols[i][None].to(dev), 256, 512, seeds[i], max_slices=3)
        gen_b = (ct[i].flatten(1).abs().amax(1) > 0).cpu()
        assert torch.equal(gen_b, (solo[0].flatten(1).abs().amax(1) > 0).cpu()) and int(gen_b.sum()) == 3
        err = float((ct[i] - solo[0]).abs().max())
        print(f"C5 shapes, volume {i}: batched (B = 2) vs solo, 3 slices: max abs {err:.3e}")
        assert err < 2e-2
