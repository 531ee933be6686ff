"""GPU suite (-m gpu): every capped grid-stride kernel of tests/grid_caps.py at the smallest shape that sends some threads through a second
trip of their loop (the inventory, the shape rules and the arithmetic that proves "past the cap" live there; tests/test_grid_caps_cpu.py
checks both against the sources).

Elementwise kernels: no tolerance.  Outputs start as NaN (integers: a sentinel), 64 elements of slack behind every output the caller
owns must come back untouched, and every stored word is compared with the reference the kernel's own module already uses -- separate
fp32 torch operations, inputs on which the arithmetic is exact, or (GELU, GEGLU) the exhaustive bf16 sweep repeated over the whole
tensor: the first period is judged by tests/act_sweep.py, every later period must repeat it bit for bit.  Entries whose ops wrapper
allocates its output are launched through ops.call with the wrapper's own argument list, into a buffer with slack, and the wrapper's
result must equal it.

Reductions: a dropped or doubled row must be visible, not merely bounded.  gg_loss_rows l1 / l2 on integer inputs is compared with the
int64 sum exactly.  The others keep their module's fp64 restatement and tolerance; their input is a background whose term is zero or
tiny plus planted rows with large terms at the first row, the last row of trip one, the first row of trip two, the last row of its
workgroup, the first row of the ragged workgroup and the last row, and the test first asserts on the CPU that putting any single
planted row back to the background moves the reference by more than ten times the tolerance.  Two runs must give the same bits.
The cross-entropy sum of gg_ccdm_step_loss has no such input (a voxel's term lies in an interval of width 1 whatever the logits are, one
row out of 262 403 moves the sum by 4e-6): it is held to the tolerance, and the weighted KL sum of the same loop trip carries the
planted rows.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grid_caps as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def assert_bits(got, want, what):
    assert G.same_bits(got, want), f"{what}: {G.first_diff(got, want)}"


def assert_row_per_lane_operands(f32_rows, unet_in, out_stride):
    """The host conditions that select ddpm_step_c4_kernel / inpaint_blend_c4_kernel (gg_sampler.hip): 16-byte aligned fp32 operands, a
    row stride of `out` that is a multiple of 4, an 8-byte aligned unet_in whose stride is a multiple of 4.  Anything else falls back to the
    per-element kernel without a word, and the case would no longer run the kernel its row of grid_caps.py names."""
    assert all(t is None or t.data_ptr() % 16 == 0 for t in f32_rows) and out_stride % 4 == 0
    assert unet_in.data_ptr() % 8 == 0 and unet_in.shape[-1] % 4 == 0


def filled_like_with(buf, lanes, value):
    """what a sentinel-filled row buffer must hold after a kernel wrote `value` into its first `lanes` lanes: the fill everywhere else"""
    want = buf.clone()
    want[..., :lanes] = value
    return want


# ================================================================================================ cap 4096
@pytest.mark.parametrize("entry,C", [("ddim", 4), ("ddim", 3), ("ddpm", 4), ("ddpm", 3), ("x0", 4), ("x0", 3)])
def test_ldm_steps(dev, entry, C):
    """gg_ddim_step / gg_ddpm_step (step_kernel, per element) and gg_ddpm_step_x0 (ddpm_step_c4_kernel at C = 4, one row per lane; step_kernel at
    C = 3) against the separate torch operations of test_vq_gpu / progressive_ref."""
    from jointimagegeneration_amd import ops
    from progressive_ref import torch_step_x0
    from test_progressive_gpu import SC
    from test_vq_gpu import ddim_scalars, ddim_want
    M = G.STEP_C3_M if C == 3 else G.STEP_C4_M if entry == "x0" else G.STEP_E4_M
    gen = torch.Generator(device=dev).manual_seed(M + C)
    x0_ = torch.randn(M, C, device=dev, generator=gen) * 1.5
    out = torch.randn(M, 8, device=dev, generator=gen)
    noise = torch.randn(M, C, device=dev, generator=gen)
    sc = ddim_scalars(0.6, dev) if entry == "ddim" else torch.tensor(SC, device=dev)
    for flags in ((0, 3) if entry == "x0" else (0,)):
        for nz in (noise, None):
            if entry == "ddim":
                want_x, want_p = ddim_want(x0_, out[:, :C].contiguous(), sc, nz)
            else:
                want_x, want_p = torch_step_x0(x0_, out[:, :C], nz, sc, flags)
            x, chk_x = G.slack_buffer((M, C), torch.float32, dev)
            x.copy_(x0_)
            p0, chk_p = G.slack_buffer((M, C), torch.float32, dev)
            uin, chk_u = G.slack_buffer((M, 8), torch.bfloat16, dev)
            want_u = filled_like_with(uin, C, want_x.bfloat16())
            if entry == "x0" and C == 4:                   # what gg_ddpm_step_x0 asks of its operands before it launches the row-per-lane kernel
                assert_row_per_lane_operands((x, out, nz, p0), uin, out.shape[-1])
            if entry == "ddim":
                ops.ddim_step(x, out, sc, noise=nz, pred_x0_out=p0, unet_in=uin)
            elif entry == "ddpm":
                ops.ddpm_step(x, out, sc, noise=nz, unet_in=uin)
            else:
                ops.ddpm_step_x0(x, out, sc, noise=nz, predicts_x0=bool(flags & 1), clip=bool(flags & 2), pred_x0_out=p0, unet_in=uin)
            torch.cuda.synchronize()
            tag = f"{entry} C={C} flags={flags} noise={nz is not None}"
            assert_bits(x, want_x, tag + " x")
            if entry != "ddpm":
                assert_bits(p0, want_p, tag + " pred_x0")
            assert_bits(uin, want_u, tag + " unet_in")
            chk_x(), chk_p(), chk_u()


@pytest.mark.parametrize("C,mask_C", [(4, 1), (4, 4), (3, 1), (3, 3)])
def test_inpaint_blend(dev, C, mask_C):
    """inpaint_blend_c4_kernel<1>, <4> (one row per lane) and inpaint_blend_kernel (per element) against test_inpaint_gpu.torch_blend."""
    from jointimagegeneration_amd import ops
    from test_inpaint_gpu import torch_blend
    M = G.STEP_C4_M if C == 4 else G.STEP_C3_M
    gen = torch.Generator(device=dev).manual_seed(M * 31 + C * 7 + mask_C)
    x0_, x0, noise = (torch.randn(M, C, device=dev, generator=gen) for _ in range(3))
    mask = torch.rand(M, mask_C, device=dev, generator=gen)
    mask[::4] = (mask[::4] > 0.5).float()
    sc = torch.tensor([0.7834521, 0.6214398], device=dev)
    want = torch_blend(x0_, x0, mask, noise, sc)
    x, chk_x = G.slack_buffer((M, C), torch.float32, dev)
    x.copy_(x0_)
    uin, chk_u = G.slack_buffer((M, 8), torch.bfloat16, dev)
    want_u = filled_like_with(uin, C, want.bfloat16())
    if C == 4:                                             # what gg_inpaint_blend asks of its operands before it launches the row-per-lane kernel
        assert_row_per_lane_operands((x, x0, noise) + ((mask,) if mask_C == 4 else ()), uin, 4)
    ops.inpaint_blend(x, x0, mask, noise, sc, unet_in=uin)
    torch.cuda.synchronize()
    assert_bits(x, want, "x")
    assert_bits(uin, want_u, "unet_in")
    chk_x(), chk_u()


def test_lincomb4(dev):
    from jointimagegeneration_amd import ops
    from test_sampler_exact_gpu import PLMS_SETS
    n = G.past_cap(4096)
    gen = torch.Generator().manual_seed(900)
    es = [torch.randn(n, generator=gen) * (1 + k) for k in range(4)]
    for coefs, denom in PLMS_SETS:
        want = coefs[0] * es[0]                            # on the CPU, as in test_sampler_exact_gpu: torch divides by a scalar on the GPU
        for c, e in zip(coefs[1:], es[1:]):                # by multiplying with its reciprocal
            want = want + c * e
        want = want / denom
        out, chk = G.slack_buffer((n,), torch.float32, dev)
        ops.lincomb4([e.to(dev) for e in es[:len(coefs)]], coefs, denom, out)
        assert_bits(out.cpu(), want, f"{len(coefs)} terms")
        chk()


def test_mask_to_cond(dev):
    """gg_mask_to_cond_slice and gg_mask_to_cond_slices at N = 3, 725 x 725: the sample decode n = t / HW of the second trip crosses from
    sample 1 to sample 2.  Reference: the oracle's zoom0 index rule, rot90(k = 3), / 255 on the CPU."""
    from jointimagegeneration_amd import ops
    N, Dm, HWm, D, hw = 3, 5, 16, 7, G.GLUE_HW
    g = torch.Generator().manual_seed(12)
    labels = torch.randint(0, 14, (N, Dm, HWm, HWm), generator=g, dtype=torch.int32)
    prev = torch.rand((N, hw, hw), generator=g)
    labels_d = labels.to(dev)

    def expect(cond, c0, c1):
        want = filled_like_with(cond, 8, torch.zeros((), dtype=torch.bfloat16))
        want[:, 0, :, :, 0], want[:, 0, :, :, 1] = c0.to(dev), c1.to(dev)
        return want

    for s in (0, D - 1):
        cond, chk_c = G.slack_buffer((N, 1, hw, hw, 8), torch.bfloat16, dev)
        mask, chk_m = G.slack_buffer((N, hw, hw), torch.float32, dev)
        ops.mask_to_cond_slice(labels_d, s, D, hw, hw, prev.to(dev), cond, mask_out=mask)
        c0, c1, mk = G.glue_reference(labels.long(), [s] * N, prev, hw, hw, D)
        assert_bits(cond, expect(cond, c0, c1), f"slice {s} cond")
        assert_bits(mask, mk.to(dev), f"slice {s} mask")
        chk_c(), chk_m()
    volume = torch.rand((D, N, hw, hw), generator=g)
    sched = torch.tensor([[[6, 0, 1], [2, 1, 0], [4, 5, 1]]], dtype=torch.int32)          # (slice, previous slice, active); the glue ignores `active`
    cond, chk_c = G.slack_buffer((N, 1, hw, hw, 8), torch.bfloat16, dev)
    ops.mask_to_cond_slices(labels_d, D, hw, hw, sched.to(dev), torch.zeros(1, dtype=torch.int32, device=dev), volume.to(dev), cond)
    pv = torch.stack([volume[int(sched[0, n, 1]), n] for n in range(N)])
    c0, c1, _ = G.glue_reference(labels.long(), [int(sched[0, n, 0]) for n in range(N)], pv, hw, hw, D)
    assert_bits(cond, expect(cond, c0, c1), "batched glue")
    chk_c()


@pytest.mark.parametrize("hw,lat,r", G.CT_HW, ids=["words", "bytes"])
def test_ct_edit_glue(dev, hw, lat, r):
    """gg_ct_edit_glue at N = 3: the image rows of the second trip belong to samples 1 and 2.  Reference: the known slice and
    test_ct_edit_gpu.window_rule."""
    from jointimagegeneration_amd import ops
    from test_ct_edit_gpu import window_rule
    N, D, f = 3, 4, hw // lat
    g = torch.Generator().manual_seed(hw + r)
    known = torch.rand((D, N, hw, hw), generator=g)
    keep = (torch.rand((D, N, hw, hw), generator=g) > 0.001).to(torch.uint8) * torch.randint(1, 256, (D, N, hw, hw), generator=g, dtype=torch.int32).to(torch.uint8)
    sched = torch.tensor([[[1, 0, 1], [3, 0, 1], [2, 0, 1]], [[0, 0, 1], [1, 0, 0], [3, 0, 1]]], dtype=torch.int32)      # row 1: sample 1 inactive
    known_d, keep_d, sched_d = known.to(dev), keep.to(dev), sched.to(dev)
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(2):
        it.fill_(i)
        img, chk_i = G.slack_buffer((N, 1, hw, hw, 8), torch.bfloat16, dev)
        lm, chk_l = G.slack_buffer((N * lat * lat, 1), torch.float32, dev)
        ops.ct_edit_glue(known_d, keep_d, sched_d, it, r, img, lm)
        want_img = filled_like_with(img, 8, torch.zeros((), dtype=torch.bfloat16))
        want_lm = torch.zeros(N, lat, lat)
        for n in range(N):
            s, active = int(sched[i, n, 0]), bool(sched[i, n, 2])
            if active:
                want_img[n, 0, :, :, 0] = known[s, n].bfloat16().to(dev)
                want_lm[n] = window_rule(keep[s, n], f, r)
        assert 0 < int(want_lm.sum()) < want_lm.numel() - lat * lat          # kept and un-kept cells in the active samples
        assert_bits(img, want_img, f"iteration {i} image")
        assert_bits(lm, want_lm.view(-1, 1).to(dev), f"iteration {i} latent keep")
        chk_i(), chk_l()


@pytest.mark.parametrize("D,N,hw", [G.KEEP_VEC, G.KEEP_SCALAR], ids=["words", "bytes"])
def test_label_keep_volume(dev, D, N, hw):
    """gg_label_keep_volume: 4 pixels per thread (HW % 4 == 0) and one pixel per thread, the (d, n) decode of the second trip past
    several slice borders.  Reference: the oracle's glue on both volumes, as in test_ct_edit_gpu."""
    from jointimagegeneration_amd import ops
    from oracle import samplers as S
    g = torch.Generator().manual_seed(6 + hw)
    Dm, HWm = 5, 16
    old = torch.randint(0, 12, (N, Dm, HWm, HWm), generator=g, dtype=torch.int32)
    new = old.clone()
    new[0, 1:3, 4:9, 2:7] = 11
    new[1, 4, :, 10:] = (old[1, 4, :, 10:] + 1) % 12
    new[1, 0, 0, 0] = (old[1, 0, 0, 0] + 5) % 12
    assert (hw * hw % 4 == 0) == ((D, N, hw) == G.KEEP_VEC)
    out, chk = G.slack_buffer((D, N, hw, hw), torch.uint8, dev, fill=0x5a)
    ops.label_keep_volume(old.to(dev), new.to(dev), D, hw, hw, out=out)
    want = torch.stack([S.mask_to_cond_volume(new[n].long(), (D, hw, hw)) == S.mask_to_cond_volume(old[n].long(), (D, hw, hw)) for n in range(N)], 1)
    assert 0 < int(want.sum()) < want.numel()
    assert_bits(out, want.to(torch.uint8).to(dev), "keep")
    chk()


def test_gauss_sample_rows(dev):
    """logvar = 0 and multiples of 1 / 8: std is exactly 1 and mean + noise is exact, as in test_gauss_sample_rows_exact_points...; N = 3."""
    from jointimagegeneration_amd import ops
    N, C, S = G.ROWS_C2
    mom = torch.full((N, 1, 1, S, 5), float("nan"), device=dev)              # lane 4 is read by nobody
    mom[..., :C] = G.ints((N, 1, 1, S, C), -64, 64, 3, dev) / 8
    mom[..., C:2 * C] = 0.0
    noise = G.ints((N, C, 1, 1, S), -64, 64, 4, dev) / 8
    want = mom[..., :C].permute(0, 4, 1, 2, 3).contiguous() + noise
    out, chk_o = G.slack_buffer((N, C, 1, 1, S), torch.float32, dev)
    z_in, chk_z = G.slack_buffer((N, 1, 1, S, 8), torch.bfloat16, dev)
    want_z = filled_like_with(z_in, C, want.permute(0, 2, 3, 4, 1).bfloat16())
    ops.gauss_sample_rows(mom, C, noise, out=out, z_in=z_in)
    assert_bits(out, want, "z")
    assert_bits(z_in, want_z, "z_in")
    chk_o(), chk_z()


def test_q_sample_rows(dev):
    """per-sample scalars at N = 3: rows of the second trip belong to samples 1 and 2.  Reference: losses_ref.q_sample, fp32 torch."""
    from jointimagegeneration_amd import ops
    import losses_ref as R
    N, C, S = G.ROWS_C2
    gen = torch.Generator(device=dev).manual_seed(S)
    x, noise = (torch.randn((N, C, S), device=dev, generator=gen) for _ in range(2))
    scal = torch.tensor([[0.9987, 0.0509], [0.7071, 0.7072], [0.0063, 0.99998]], device=dev)
    want = R.q_sample(x, noise, scal[:, 0].contiguous(), scal[:, 1].contiguous())
    out, chk_o = G.slack_buffer((N, C, S), torch.float32, dev)
    uin, chk_u = G.slack_buffer((N * S, 8), torch.bfloat16, dev)
    want_u = filled_like_with(uin, C, want.permute(0, 2, 1).reshape(N * S, C).bfloat16())
    ops.q_sample_rows(x, noise, scal, out=out, unet_in=uin)
    assert_bits(out, want, "x_noisy")
    assert_bits(uin, want_u, "unet_in")
    chk_o(), chk_u()


def test_component_stats_zeroing(dev):
    """cc_zero_kernel through gg_component_stats: one volume of 1 048 835 voxels made of five slabs, `size` and `stats` full of garbage
    before the call: a word that the second trip leaves unzeroed shows in `size`.  Reference: components_ref.sizes_and_stats."""
    from jointimagegeneration_amd import ops
    import components_ref as R
    M, K = G.CC_M, 4
    edge = 4096 * G.THREADS
    cuts = [0, 1000, 262144, edge, edge + 255, M]
    cls = [1, 0, 2, 1, 3]                                                      # class 0: background, root -1
    labels, root = np.zeros((1, M), dtype=np.int32), np.full((1, M), -1, dtype=np.int32)
    for a, b, c in zip(cuts[:-1], cuts[1:], cls):
        labels[0, a:b] = c
        if c:
            root[0, a:b] = a
    want_size, want_stats = R.sizes_and_stats(labels, root, K)
    assert want_stats[0].tolist() == [[0, 0, 0, -1], [2, 1255, 1000, 0], [1, edge - 262144, edge - 262144, 262144], [1, 4, 4, edge + 255]]
    size, chk_s = G.slack_buffer((1, M), torch.int32, dev, fill=0x7f7f7f7f)
    stats, chk_t = G.slack_buffer((1, K, 4), torch.int64, dev, fill=0x7f7f7f7f7f7f7f7f)
    lab_d, root_d = torch.from_numpy(labels).to(dev), torch.from_numpy(root).to(dev)
    ops.call("gg_component_stats", lab_d.data_ptr(), root_d.data_ptr(), 1, M, K, size.data_ptr(), stats.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(size, torch.from_numpy(want_size.astype(np.int32)).to(dev), "size")
    assert_bits(stats, torch.from_numpy(want_stats.astype(np.int64)).to(dev), "stats")
    chk_s(), chk_t()
    size2, stats2 = ops.component_stats(lab_d, root_d, K)
    assert torch.equal(size2, size) and torch.equal(stats2, stats)


def test_groupnorm_apply_acc_general(dev):
    """gn_apply_acc_kernel past its two prefetched trips: 2 097 412 pieces per sample against 4096 * 256 per trip, so the plain stride
    loop behind the prefetch runs too (test_norm_exact_gpu's general case ends inside the second prefetched trip).  The statistics are
    whatever the accumulators say: per (sample, channel) sum = S m and sumsq = S (m^2 + s^2) in their fixed point, m in {-1, 0, 1},
    s in {1, 2}, so mean = m and rstd = 1 / s; x in [-4, 4], gamma = s * {+-1/2, +-1}, beta = +-1/4: the output (x - m) gamma / s + beta is
    an odd multiple of 1/4 below 6, exact in bf16 and never 0."""
    from jointimagegeneration_amd import ops
    import norm_exact as NX
    N, S, C = G.ACC_GENERAL
    assert NX.apply_acc_kernel(N, S, C, C) == "general" and S * (C // 8) > 2 * 4096 * G.THREADS
    k = torch.arange(N)[:, None] + torch.arange(C)[None, :]
    m = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)[k % 3]
    s = torch.tensor([1.0, 2.0], dtype=torch.float64)[(torch.arange(C) // 3) % 2][None, :].expand(N, C)          # per channel (= group)
    ratio = torch.tensor([0.5, -1.0, 1.0, -0.5], dtype=torch.float64)[torch.arange(C) % 4]          # gamma / s
    gamma = (ratio * s[0]).float()
    beta = torch.tensor([0.25, -0.25], dtype=torch.float64)[(torch.arange(C) // 2) % 2].float()
    acc = torch.stack([(S * m * NX.ACC_SUM_SCALE).long(), (S * (m * m + s * s) * NX.ACC_SQ_SCALE).long()], -1).view(N, 1, C, 2).contiguous()
    x = G.ints((N, 1, 1, S, C), -4, 4, 21, dev, torch.bfloat16)
    md, sd = m.to(dev)[:, None, None, None, :], s.to(dev)[:, None, None, None, :]
    want = (x.double() - md) / sd * gamma.double().to(dev) + beta.double().to(dev)
    assert bool((want.bfloat16().double() == want).all()) and float(want.abs().min()) >= 0.25
    out, chk = G.slack_buffer((N, 1, 1, S, C), torch.bfloat16, dev)
    acc_d, gamma_d, beta_d = acc.to(dev), gamma.to(dev), beta.to(dev)
    ops.call("gg_groupnorm_apply_acc", x.data_ptr(), C, acc_d.data_ptr(), None, 0, None, N, S, C, gamma_d.data_ptr(), beta_d.data_ptr(), 0.0, 0,
             out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, want.bfloat16(), "out")
    chk()
    assert torch.equal(ops.groupnorm_apply_acc(ops.CL(x, C, acc=acc_d), gamma_d, beta_d, 0.0, False).t, out)


# ================================================================================================ cap 8192
def test_groupnorm_apply(dev):
    """gn_apply_kernel at N = 3: integer x in [-8, 8], per-(n, c) scale from +-{1/2, 1, 2} and shift a multiple of 1/4: x * scale + shift is
    exact in fp32 and in bf16 (a multiple of 1/4 below 18), whether the kernel fuses the multiply-add or not."""
    from jointimagegeneration_amd import ops
    N, S, C = G.GN_APPLY
    k = torch.arange(N)[:, None] * 5 + torch.arange(C)[None, :]
    scale = torch.tensor([0.5, -1.0, 2.0, 1.0, -0.5, -2.0])[k % 6].contiguous().to(dev)
    shift = (((k * 3) % 9 - 4) * 0.25).float().contiguous().to(dev)
    x = G.ints((N, 1, 1, S, C), -8, 8, 22, dev, torch.bfloat16)
    want = x.double() * scale.double()[:, None, None, None, :] + shift.double()[:, None, None, None, :]
    assert bool((want.bfloat16().double() == want).all())
    out, chk = G.slack_buffer((N, 1, 1, S, C), torch.bfloat16, dev)
    ops.call("gg_groupnorm_apply", x.data_ptr(), C, None, 0, N, S, scale.data_ptr(), shift.data_ptr(), 0, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, want.bfloat16(), "out")
    chk()
    assert torch.equal(ops.groupnorm_apply(ops.CL(x, C), scale, shift, False).t, out)


def sweep_tiled(n, dev):
    """the 65280 finite bf16 values of act_sweep, repeated to n elements"""
    import act_sweep as A
    x = A.all_finite_bf16().to(dev)
    return x.repeat(G.ceil_div(n, x.numel()))[:n].contiguous()


def assert_periodic(flat, period, what):
    """every later period of `flat` repeats the first one bit for bit (the ragged last one its prefix)"""
    bits = flat.view(torch.int16)
    full = bits.numel() // period
    first = bits[:period]
    body = bits[:full * period].view(full, period)
    bad = (body != first[None]).any(1).nonzero().reshape(-1)
    assert not bad.numel(), f"{what}: period {int(bad[0])} (from element {int(bad[0]) * period}) differs from the first period"
    tail = bits[full * period:]
    assert torch.equal(tail, first[:tail.numel()]), f"{what}: the ragged last period differs from the first"


def test_geglu(dev):
    """value 1, the gate the exhaustive bf16 sweep repeated over 16.8 M outputs: the first period against act_sweep's checker and
    allowance (as test_geglu_gate_sweep), every later period equal to the first."""
    from jointimagegeneration_amd import ops
    import act_sweep as A
    rows, inner = G.GEGLU
    x, _, g64 = A.references()
    h = torch.ones((rows, 2 * inner), dtype=torch.bfloat16, device=dev)
    h[:, inner:] = sweep_tiled(rows * inner, dev).view(rows, inner)
    out, chk = G.slack_buffer((rows, inner), torch.bfloat16, dev)
    ops.call("gg_geglu", h.data_ptr(), rows, inner, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    A.check(out.reshape(-1)[:A.N_FINITE].cpu(), x, g64, allow=A.geglu_allow(x))
    assert_periodic(out.reshape(-1), A.N_FINITE, "geglu")
    chk()
    assert torch.equal(ops.geglu(h, inner).view(torch.int16), out.view(torch.int16))


def test_gelu(dev):
    """the sweep repeated over 16 779 285 elements (a 5-element scalar tail in the second trip): the first period within one bf16 ulp of
    fp64 (act_sweep.check, which holds the criterion of test_cond_gpu and more), every later period equal to the first."""
    from jointimagegeneration_amd import ops
    import act_sweep as A
    n = G.GELU_N
    x, _, g64 = A.references()
    xd = sweep_tiled(n, dev)
    out, chk = G.slack_buffer((n,), torch.bfloat16, dev)
    ops.call("gg_gelu", xd.data_ptr(), n, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    A.check(out[:A.N_FINITE].cpu(), x, g64)
    assert_periodic(out, A.N_FINITE, "gelu")
    chk()
    assert torch.equal(ops.gelu(xd).view(torch.int16), out.view(torch.int16))


def test_add(dev):
    from jointimagegeneration_amd import ops
    n = G.ADD_N
    a, b = G.ints((n,), -64, 64, 1, dev, torch.bfloat16), G.ints((n,), -64, 64, 2, dev, torch.bfloat16)
    want = a.double() + b.double()
    out, chk = G.slack_buffer((n,), torch.bfloat16, dev)
    ops.call("gg_add", a.data_ptr(), b.data_ptr(), n, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, want.bfloat16(), "a + b")
    assert bool((out.double() == want).all())
    chk()
    assert torch.equal(ops.add(a, b), out)


def test_labels_to_onehot(dev):
    from jointimagegeneration_amd import ops
    M, K, stride = G.ONEHOT
    lab = G.ints((M,), 0, K - 1, 5, dev, torch.int32)
    out, chk = G.slack_buffer((M, stride), torch.bfloat16, dev)
    ops.labels_to_onehot(lab, K, out)
    want = torch.zeros((M, stride), dtype=torch.bfloat16, device=dev)
    want[:, :K] = F.one_hot(lab.long(), K).to(torch.bfloat16)
    assert_bits(out, want, "one-hot rows")
    chk()


def test_layout_movers(dev):
    """gg_nchw_f32_to_cl_bf16 (two pieces per row: the second piece of every row is written in the second trip), gg_cl_to_nchw_f32 from bf16
    and from fp32 rows, gg_log_rows: integer values, pure data movement."""
    from jointimagegeneration_amd import ops
    N, C, S, cp = G.TO_CL
    x = G.ints((N, C, S), -64, 64, 7, dev)
    out, chk = G.slack_buffer((N, 1, 1, S, cp), torch.bfloat16, dev)
    ops.to_cl(x, out=out)
    want = torch.zeros((N, 1, 1, S, cp), dtype=torch.bfloat16, device=dev)
    want[..., :C] = x.permute(0, 2, 1).reshape(N, 1, 1, S, C).bfloat16()
    assert_bits(out, want, "to_cl")
    chk()
    N, C, S, cp = G.FROM_CL
    for dtype, code in ((torch.bfloat16, ops.GG_BF16), (torch.float32, ops.GG_F32)):
        src = torch.full((N, 1, 1, S, cp), float("nan"), dtype=dtype, device=dev)          # pad lanes: read by nobody
        src[..., :C] = G.ints((N, 1, 1, S, C), -64, 64, 8, dev, dtype)
        want = src[..., :C].reshape(N, S, C).permute(0, 2, 1).float().contiguous()
        dst, chk = G.slack_buffer((N, C, S), torch.float32, dev)
        ops.call("gg_cl_to_nchw_f32", src.data_ptr(), code, N, C, S, cp, dst.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert_bits(dst, want, f"from_cl {dtype}")
        chk()
        assert torch.equal(ops.from_cl(ops.CL(src, C), 1), dst)
    state = G.ints((N * S, C), -64, 64, 9, dev)
    slot, chk = G.slack_buffer((N, C, S), torch.float32, dev)
    ops.log_rows(state, N, slot)
    assert_bits(slot, state.view(N, S, C).permute(0, 2, 1).contiguous(), "log_rows")
    chk()


def test_embed_rows(dev):
    """bf16 rows of 64 lanes (pad lanes zero) with positions, and dense fp32 rows; test_cond_gpu.raw_embed launches at the C-ABI into a
    sentinel-filled buffer with 64 elements of slack."""
    from jointimagegeneration_amd import ops
    from test_cond_gpu import SENTINEL, raw_embed
    gen = torch.Generator().manual_seed(48)
    V = 97
    for (B, T_len, D, stride), bf16 in ((G.EMBED_BF16, True), (G.EMBED_F32, False)):
        tok, pos = torch.randn(V, D, generator=gen), torch.randn(40, D, generator=gen)
        ids = torch.randint(0, V, (B, T_len), generator=gen)
        want = tok[ids] + pos[:T_len][None]
        rc, rows, slack = raw_embed(ids, tok, pos, T_len, bf16, stride, dev)
        assert rc == 0 and bool((slack == SENTINEL).all())
        assert_bits(rows[:, :D].contiguous(), (want.bfloat16() if bf16 else want).view(-1, D), f"rows bf16={bf16}")
        assert bool((rows[:, D:] == 0).all())
        got = ops.embed_rows(ids.to(dev), tok.to(dev), pos.to(dev), bf16=bf16)
        assert torch.equal(got.cpu().reshape(-1, stride), rows)


# ================================================================================================ cap 16384
def _res_expect(src, C, up, rd):
    """nearest x2 / 2x average pool of integer values (every sum exact in fp32), pad lanes zero"""
    t = src.float()
    if up:
        want = t.repeat_interleave(2, 2).repeat_interleave(2, 3)
        want = want.repeat_interleave(2, 1) if rd else want
    else:
        N, D, H, W, cp = t.shape
        kd = 2 if rd else 1
        want = t.reshape(N, D // kd, kd, H // 2, 2, W // 2, 2, cp).sum((2, 4, 6)) / (4 * kd)
    want[..., C:] = 0
    return want


@pytest.mark.parametrize("shape,up,dtype", [(G.RES_UP2D, True, torch.bfloat16), (G.RES_UP3D, True, torch.bfloat16), (G.RES_POOL2D, False, torch.bfloat16),
                                            (G.RES_POOL3D, False, torch.bfloat16), (G.RES_UP2D, True, torch.float32), (G.RES_UP3D, True, torch.float32),
                                            (G.RES_POOL2D, False, torch.float32)],
                         ids=["up2d-bf16", "up3d-bf16", "pool2d-bf16", "pool3d-bf16", "up2d-f32", "up3d-f32", "pool2d-f32"])
def test_resample2x(dev, shape, up, dtype):
    """integer inputs in [-8, 8] as in test_resample2x_exact, 24 logical channels of 32 (source pad lanes hold 3, output pad lanes must be
    0), N = 3: the border of samples 1 and 2 lies in the second trip.  The output size is set by the cap (16384 * 256 pieces of 8
    channels); a pool reads 4 or 8 times as much.  The fp32 pool runs in 2-D only: resample_d is a run-time argument of the same
    instantiation, which the bf16 pool3d case and the fp32 up3d case both take, and its source would be 1.6 GB."""
    from jointimagegeneration_amd import ops
    N, D, H, W, rd = shape
    C, cp = 24, 32
    src = torch.full((N, D, H, W, cp), 3.0, dtype=dtype, device=dev)
    src[..., :C] = G.ints((N, D, H, W, C), -8, 8, H + int(up), dev, dtype)
    want = _res_expect(src, C, up, rd)
    wd = want.to(dtype)
    assert bool((wd.float() == want).all())
    out, chk = G.slack_buffer(tuple(want.shape), dtype, dev)
    ops.call("gg_resample2x", src.data_ptr(), ops.GG_F32 if dtype == torch.float32 else ops.GG_BF16, N, D, H, W, cp, C, 1 if rd else 0,
             0 if up else 1, None, None, 0, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, wd, "resample2x")
    chk()
    del want, wd
    assert torch.equal(ops.resample2x(ops.CL(src, C), up, rd).t, out)


def test_resample2x_with_prologue(dev):
    """the 2x average pool behind a per-(n, c) affine prologue: x in [-4, 4], scale from +-{1/2, 1} and 2, shift a multiple of 1/4 up to
    1: every x * scale + shift is a multiple of 1/4 below 10, every sum of four exact, the mean a multiple of 1/16 below 10: exact in
    bf16."""
    from jointimagegeneration_amd import ops
    N, D, H, W, rd = G.RES_POOL2D
    C, cp = 24, 32
    src = torch.zeros((N, D, H, W, cp), dtype=torch.bfloat16, device=dev)
    src[..., :C] = G.ints((N, D, H, W, C), -4, 4, 77, dev, torch.bfloat16)
    k = torch.arange(N)[:, None] * 7 + torch.arange(cp)[None, :]
    scale = torch.tensor([0.5, -1.0, 2.0, 1.0, -0.5])[k % 5].contiguous().to(dev)
    shift = (((k * 3) % 9 - 4) * 0.25).float().contiguous().to(dev)
    v = src.float() * scale[:, None, None, None, :] + shift[:, None, None, None, :]
    want = v.reshape(N, D, H // 2, 2, W // 2, 2, cp).sum((3, 5)) / 4
    want[..., C:] = 0
    del v
    assert bool((want.bfloat16().float() == want).all())
    out, chk = G.slack_buffer(tuple(want.shape), torch.bfloat16, dev)
    ops.call("gg_resample2x", src.data_ptr(), ops.GG_BF16, N, D, H, W, cp, C, 0, 1, scale.data_ptr(), shift.data_ptr(), 0, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, want.bfloat16(), "pool with prologue")
    chk()
    assert torch.equal(ops.resample2x(ops.CL(src, C), False, False, prologue=(scale, shift), act=False).t, out)


@pytest.mark.parametrize("path", ["f32", "film"])
def test_groupnorm_f32(dev, path):
    """gn_f32_apply_kernel / gn_f32_apply_film_kernel on the closed-form inputs of norm_exact.py (regime E, eps = 0, act off), N = 3 with
    the border of samples 1 and 2 in the second trip; outputs between 256 sentinel elements on either side."""
    import norm_exact as NX
    N, S, C = G.GN_F32
    case = NX.Case(f"{path}_past_cap", path, C, (S,))
    inp = NX.build(case, N, False)
    p = NX.pack(inp).to(dev)
    NX.check_reference(inp, 0.0, dev)
    bad = NX.check_result(inp, 0.0, NX.launch(path, p, 0.0, False))
    assert not bad, bad


@pytest.mark.parametrize("mode,s", [("nearest", 2), ("bilinear", 2), ("bicubic", 2), ("area", 2), ("area", 0.5), ("bilinear", 0.5)])
def test_interpolate2d(dev, mode, s):
    """cond_ref.exact_input planes with exact multipliers against F.interpolate on the CPU, three planes of 1450 x 1450 outputs: the plane
    decode of the second trip crosses from plane 1 to plane 2."""
    from jointimagegeneration_amd import ops
    import cond_ref
    assert s in cond_ref.exact_multipliers(mode)
    N, C, H, W = G.INTERP
    if s < 1:
        H, W = 4 * H, 4 * W
    x = cond_ref.exact_input((N, C, H, W), seed=int(10 * s))
    want = F.interpolate(x, scale_factor=s, mode=mode)
    assert want.numel() == N * C * 4 * G.INTERP[2] * G.INTERP[3]
    xd = x.to(dev)
    got = ops.interpolate2d(xd, s, mode)
    assert_bits(got.cpu(), want, f"{mode} x{s}")
    out, chk = G.slack_buffer(tuple(want.shape), torch.float32, dev)
    ops.call("gg_interpolate2d_f32", xd.data_ptr(), N * C, H, W, want.shape[2], want.shape[3], 1.0 / s, 1.0 / s, ops.INTERPOLATE_MODES[mode],
             out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert_bits(out, got, "into a buffer with slack")
    chk()


# ================================================================================================ cap 2048 and 2048 / N
def _with_late_extremes(x, first_late, k):
    """x with its minimum and maximum moved to indices that only a later trip reads"""
    x = x.clone()
    lo, hi = float(x.min()) - 1.0 - k, float(x.max()) + 2.0 + k
    x[first_late + 1 + k], x[x.numel() - 1 - k] = lo, hi
    return x


def test_minmax_normalise(dev):
    from jointimagegeneration_amd import ops
    n = G.MINMAX_N
    g = torch.Generator().manual_seed(800)
    x = _with_late_extremes(3 * torch.randn(n, generator=g), 2048 * G.THREADS, 0)
    assert int(x.argmin()) >= 2048 * G.THREADS and int(x.argmax()) >= 2048 * G.THREADS
    want = (x - x.min()) / (x.max() - x.min())
    out, chk = G.slack_buffer((n,), torch.float32, dev)
    ops.minmax_normalise(x.to(dev), out=out)
    assert_bits(out.cpu(), want, "normalised")
    chk()


@pytest.mark.parametrize("n_per,keep", [(G.MM_SCALAR, False), (G.MM_VEC, False), (G.MM_SCALAR, True), (G.MM_VEC, True)],
                         ids=["scatter", "scatter_4_trips", "keep_bytes", "keep_words"])
def test_minmax_scatter(dev, n_per, keep):
    """gg_minmax_normalise_scatter / _keep_scatter at N = 3 (682 workgroups per sample), each sample's minimum and maximum at indices that
    only a later trip reads.  Reference: the torch expression on each sample, the known value where keep != 0."""
    from jointimagegeneration_amd import ops
    N, depth = G.MM_N, 4
    g = torch.Generator().manual_seed(n_per)
    src = torch.randn((N, n_per), generator=g) * torch.tensor([1.0, 40.0, 1e-3]).view(N, 1) + torch.tensor([0.0, -7.0, 3.0]).view(N, 1)
    src = torch.stack([_with_late_extremes(src[n], G.MM_CAP * G.THREADS, n) for n in range(N)])
    assert all(int(src[n].argmin()) >= G.MM_CAP * G.THREADS and int(src[n].argmax()) >= G.MM_CAP * G.THREADS for n in range(N))
    sched = torch.tensor([[[2, 1, 1], [3, 2, 1], [0, 0, 1]]], dtype=torch.int32, device=dev)
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    vol, chk = G.slack_buffer((depth, N, n_per), torch.float32, dev)
    want = vol.cpu().clone()
    known = torch.rand((depth, N, n_per), generator=g)
    kp = (torch.rand((depth, N, n_per), generator=g) > 0.5).to(torch.uint8) * 3
    for n, s in ((0, 2), (1, 3), (2, 0)):
        norm = (src[n] - src[n].min()) / (src[n].max() - src[n].min())
        want[s, n] = torch.where(kp[s, n] != 0, known[s, n], norm) if keep else norm
    if keep:
        ops.minmax_normalise_keep_scatter(src.to(dev), sched, it, known.to(dev), kp.to(dev), vol)
    else:
        ops.minmax_normalise_scatter(src.to(dev), sched, it, vol)
    assert int(it[0]) == 1
    assert_bits(vol.cpu(), want, "volume")
    chk()


# ================================================================================================ split-K reduce (cap 2048)
@pytest.mark.parametrize("regime", ["D", "S"])
def test_splitk_reduce(dev, regime, monkeypatch):
    """conv_splitk_reduce_kernel behind the split gather kernel, on production dispatch: a 1x1 conv 512 -> 320 at N = 3, 59 x 61.  plan_gather
    starts at NT = 5 (85 * 2 blocks < 192), goes to NT = 2 (85 * 5 = 425 blocks, not below 192, so it stays) and splits K in two; the
    capped reduce then has M * Cout_pad / 4 = 863 760 units on 2048 blocks, with the border of samples 1 and 2 (per-sample bias
    n = m / osp) at unit 575 840, in the second trip.  Exact inputs of tests/conv_exact.py (regimes D and S), per-sample bias and a residual,
    against the fp64 reference bit for bit through test_conv_exact_gpu.run_exact, which also proves the gather path and the K split on the
    descriptor of the launch."""
    import conv_exact as X
    from test_conv_exact_gpu import run_exact
    N, cin, cout, H, W = G.SPLITK
    case = X.c2("sk_reduce_past_cap", "gather", N, cin, 0, cout, (H, W), k=(1, 1, 1), pad=0, bias="per_sample", residual=True, splitk=True)
    y = run_exact(case, regime, dev, monkeypatch)
    assert case.M * y.Cpad // 4 == G.BY_KERNEL["conv_splitk_reduce_kernel"].work[0] and y.Cpad == 320


# ================================================================================================ reductions
def _rel(got, want):
    return np.abs(np.asarray(got, dtype=np.float64) / np.asarray(want, dtype=np.float64) - 1)


@pytest.mark.parametrize("lt", ["l1", "l2"])
def test_loss_rows_exact_integers(dev, lt):
    """N = 2, C = 3, S = 262 403 on rows 5 lanes apart: integer pred and target with |v| <= 8.  Every term (at most 256) and every partial
    sum (at most 2.1e8) is an integer that fp64 holds exactly in any order, so got * C * S is the int64 sum but for the one rounding of
    the scale 1 / (C S) and of this product (relative 3e-16: 6e-8 absolute): a dropped or doubled row moves it by at least 1."""
    from jointimagegeneration_amd import ops
    N, C, S = G.N_RED, 3, G.S_RED
    rows = torch.full((N * S, 5), float("nan"), device=dev)
    pred = G.ints((N, S, C), -8, 8, 31, dev)
    target = G.ints((N, C, S), -8, 8, 32, dev)
    for n in range(N):
        for r in G.planted_rows(S, n):                    # the rows at the edges of the trips carry the largest term
            pred[n, r], target[n, :, r] = 8.0, -8.0
    rows[:, :C] = pred.view(N * S, C)
    d = (target.long() - pred.permute(0, 2, 1).long()).cpu()
    exact = (d.abs() if lt == "l1" else d * d).sum((1, 2))
    got = ops.loss_rows(lt, N, C, S, pred=rows, target=target)
    v = got.cpu().double() * C * S
    print(f"loss_rows {lt}: got * C * S = {v.tolist()}, int64 sums {exact.tolist()}")
    assert torch.equal(v.round().long(), exact) and float((v - exact.double()).abs().max()) < 0.25
    assert torch.equal(got, ops.loss_rows(lt, N, C, S, pred=rows, target=target))


def test_loss_rows_prior_kl(dev):
    """lv = 0 makes the background term 0.5 ((-1 - 0) + 1 + 0) exactly 0; planted rows hold x = 32 (k + 1)."""
    from jointimagegeneration_amd import ops
    import losses_ref as R
    from test_losses_gpu import TOL_LOSS_ROWS_PRIOR as TOL
    N, C, S = G.N_RED, 3, G.S_RED
    sc = torch.tensor([[1.0, 0.0], [0.5, 0.0]])
    x = torch.zeros((N, C, S))
    for n in range(N):
        for k, r in enumerate(G.planted_rows(S, n)):
            x[n, :, r] = 32.0 * (k + 1)
    ref = lambda t: np.array([R.prior_kl(t[n:n + 1], sc[n, 0], sc[n, 1])[0] for n in range(N)])
    want = ref(x)
    deleted = []
    for k in range(6):
        t = x.clone()
        for n in range(N):
            t[n, :, G.planted_rows(S, n)[k]] = 0.0
        deleted.append(ref(t))
    G.single_deletions_move(want, deleted, TOL, "prior_kl")
    got = ops.loss_rows("prior_kl", N, C, S, x_start=x.to(dev), scalars=sc.to(dev))
    err = float(_rel(got.cpu().numpy(), want).max())
    print(f"loss_rows prior_kl past the cap: rel {err:.3e} vs fp64 (bound {TOL:.3e})")
    assert err <= TOL
    assert torch.equal(got, ops.loss_rows("prior_kl", N, C, S, x_start=x.to(dev), scalars=sc.to(dev)))


def test_ccdm_step_loss(dev):
    """K = 4, t = (5, 27).  Background: x_t = x_0 = class 0 (weight 1) under logits that put all mass on class 0 (a gap of 120: exp
    underflows in fp32), so the predicted posterior equals the true one and the KL term is rounding noise.  Planted rows: x_0 in classes
    1 and 2 (weights 64 and 48), all mass on a wrong class.  The single-deletion condition is asserted on the weighted KL sum, through the
    restatement's additivity over voxels (the restatement of one voxel is that voxel's term); the CE sum is held to the tolerance."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ccdm import DiffusionModel
    import losses_ref as R
    from test_losses_gpu import TOL_CCDM_STEP_LOSS as TOL
    N, S, K = G.N_RED, G.S_RED, 4
    dm = DiffusionModel("cosine", R.CCDM_T, K, dims=3)
    t = torch.tensor([5, 27])
    cw = torch.tensor([1.0, 64.0, 48.0, 1.0])
    logits = torch.zeros((N, S, K))
    logits[..., 0] = 120.0
    x0, xt = torch.zeros((N, S), dtype=torch.int64), torch.zeros((N, S), dtype=torch.int64)
    for n in range(N):
        for k, r in enumerate(G.planted_rows(S, n)):
            x0[n, r], xt[n, r] = 1 + k % 2, (k + n) % K
            logits[n, r] = 0.0
            logits[n, r, (3 + k) % K if (3 + k) % K != 1 + k % 2 else 0] = 120.0
    scal = R.step_scalars(dm.alphas, dm.cumalphas, t.tolist())
    ref = lambda lg, a, b, sc: R.ccdm_step_loss(lg.numpy(), a.numpy(), b.numpy(), sc, cw, K)
    want = ref(logits, xt, x0, scal)
    deleted = []
    for k in range(6):
        d = want.copy()
        for n in range(N):
            r = G.planted_rows(S, n)[k]
            d[n] += ref(logits[n:n + 1, 2:3], xt[n:n + 1, 2:3], x0[n:n + 1, 2:3], scal[n:n + 1])[0]          # a background voxel in its place
            d[n] -= ref(logits[n:n + 1, r:r + 1], xt[n:n + 1, r:r + 1], x0[n:n + 1, r:r + 1], scal[n:n + 1])[0]
        deleted.append(d[:, 0])
    G.single_deletions_move(want[:, 0], deleted, TOL, "ccdm_step_loss weighted KL")
    rows = torch.full((N * S, 5), 7.0)
    rows[:, :K] = logits.view(N * S, K)
    args = (rows.to(dev), xt.int().view(-1).to(dev), x0.int().view(-1).to(dev), dm.step_scalar_rows(t).to(dev), cw.to(dev), K)
    got = ops.ccdm_step_loss(*args)
    err = _rel(got.cpu().numpy(), want)
    print(f"ccdm_step_loss past the cap: rel (kl, ce) per sample {err.tolist()} vs fp64 (bound {TOL:.3e}); sums {want.tolist()}")
    assert float(err.max()) <= TOL
    assert torch.equal(got, ops.ccdm_step_loss(*args))


def _aeloss_tol(name):
    from util import GOLD
    return 4 * float(np.load(os.path.join(GOLD, "aeloss.npz"))[name])


def test_gauss_kl_rows(dev):
    """mean = logvar = 0 makes the background term (0 + 1) - 1 - 0 exactly 0; planted rows hold mean = 16 (k + 1).  C = 2 on rows 5 lanes apart."""
    from jointimagegeneration_amd import ops
    import aeloss_ref as A
    tol = _aeloss_tol("tol_kl")
    N, C, S = G.N_RED, 2, G.S_RED
    mom = torch.zeros((N, 1, 1, S, 5))
    mom[..., 4] = float("nan")                            # read by nobody
    for n in range(N):
        for k, r in enumerate(G.planted_rows(S, n)):
            mom[n, 0, 0, r, :C] = 16.0 * (k + 1)
    ref = lambda m: A.gauss_kl(m[..., :2 * C].permute(0, 4, 1, 2, 3).double()).numpy()
    want = ref(mom)
    deleted = []
    for k in range(6):
        m = mom.clone()
        for n in range(N):
            m[n, 0, 0, G.planted_rows(S, n)[k], :C] = 0.0
        deleted.append(ref(m))
    G.single_deletions_move(want, deleted, tol, "gauss_kl")
    got = ops.gauss_kl_rows(mom.to(dev), C)
    err = float(_rel(got.cpu().numpy(), want).max())
    print(f"gauss_kl_rows past the cap: rel {err:.3e} vs fp64 (bound {tol:.3e})")
    assert err <= tol
    assert torch.equal(got, ops.gauss_kl_rows(mom.to(dev), C))


@pytest.mark.parametrize("bg,amp,stats", [(0.0, 1000.0, (0,)), (30.0, -50.0, (1, 3)), (-30.0, 50.0, (2, 4))], ids=["mean", "real_side", "fake_side"])
def test_logit_stats(dev, bg, amp, stats):
    """One grid of 1024 workgroups over 262 403 logits (not per sample).  No background makes all five terms tiny at once: l = 0 does for
    the mean, l = 30 for relu(1 - l) and softplus(-l), l = -30 for relu(1 + l) and softplus(l); each leg asserts the single-deletion
    condition on its own statistics and the tolerance on all five."""
    from jointimagegeneration_amd import ops
    import aeloss_ref as A
    tol = _aeloss_tol("tol_logit")
    M = G.S_RED
    l = torch.full((M, 3), 100.0)
    l[:, 0] = bg
    planted = G.planted_rows(M, 0)
    for k, r in enumerate(planted):
        l[r, 0] = amp * (k + 1)
    ref = lambda v: A.logit_stats(v[:, 0].double()).numpy()
    want = ref(l)
    deleted = []
    for r in planted:
        v = l.clone()
        v[r, 0] = bg
        deleted.append(ref(v)[list(stats)])
    G.single_deletions_move(want[list(stats)], deleted, tol, f"logit_stats {stats}")
    got = ops.logit_stats(l.to(dev))
    err = _rel(got.cpu().numpy(), want)
    print(f"logit_stats past the cap, background {bg}: rel {err.tolist()} vs fp64 (bound {tol:.3e})")
    assert float(err.max()) <= tol
    assert torch.equal(got, ops.logit_stats(l.to(dev)))


def _lpips_planted(h, w, G_quads, image):
    """pixels in the quads at the edges of the trips of a 128-workgroup grid: the first quad, the last quad of every full trip, the first
    quad of the next one, and the last quad; the second image takes their neighbours"""
    qw, Q = G.ceil_div(w, 2), G.lpips_quads(h, w)
    stride = G.LP_CAP * G_quads
    quads = {0, Q - 1}
    for t in range(1, G.ceil_div(Q, stride)):
        quads |= {t * stride - 1, t * stride}
    quads = sorted(q + image if q + image < Q else q - image for q in quads)
    return [(2 * (q // qw) + (i % 2), 2 * (q % qw) + (i // 2) % 2) for i, q in enumerate(quads)]


@pytest.mark.parametrize("C,h,w,dtype", [G.LPIPS_SHAPES[0] + (torch.bfloat16,), G.LPIPS_SHAPES[0] + (torch.float32,), G.LPIPS_SHAPES[1] + (torch.bfloat16,)],
                         ids=["c512_bf16", "c512_f32", "c64_bf16"])
def test_lpips_tap(dev, C, h, w, dtype):
    """More quads than 128 workgroups take in one trip.  a == b everywhere (every such pixel contributes exactly 0, as
    test_zero_rows_contribute_exactly_zero shows for zero rows and the subtraction of equal values does here) except at planted pixels;
    pooled outputs bit for bit against max_pool2d(relu(.), 2); the distance against the fp64 restatement under RTOL of test_lpips_gpu."""
    from jointimagegeneration_amd import ops
    from test_lpips_gpu import RTOL, rel, tap_f64
    L = G.lpips_lanes(C, 4 if dtype == torch.float32 else 8)          # tap_plan's rule, pinned to the source by test_grid_caps_cpu
    Gq = 256 // L
    assert (h + 1) // 2 * ((w + 1) // 2) > 128 * (256 // L)
    n = 2
    g = torch.Generator().manual_seed(C + h)
    a = (torch.randn(n, 1, h, w, C, generator=g) + 0.3).to(dtype)
    b = a.clone()
    planted = [_lpips_planted(h, w, Gq, i) for i in range(n)]
    for i in range(n):
        for y, x in planted[i]:
            b[i, 0, y, x] = (a[i, 0, y, x].float() + 0.5 * torch.randn(C, generator=g)).to(dtype)
    lw = torch.rand(C, generator=g) + 0.05
    ref = lambda bb: tap_f64(a, bb, lw).numpy()
    want = ref(b)
    zero = b.clone()
    for i in range(n):
        for y, x in planted[i]:
            zero[i, 0, y, x] = a[i, 0, y, x]
    assert (ref(zero) == 0).all()                          # the background contributes exactly 0 to the reference as well
    deleted = []
    for k in range(min(len(p) for p in planted)):
        bb = b.clone()
        for i in range(n):
            y, x = planted[i][k]
            bb[i, 0, y, x] = a[i, 0, y, x]
        deleted.append(ref(bb))
    G.single_deletions_move(want, deleted, RTOL, "lpips tap")
    ad, bd, lwd = a.to(dev), b.to(dev), lw.to(dev)
    got, pooled = ops.lpips_tap(ad, bd, lwd, pool=True)
    err = rel(got.cpu().numpy(), want)
    print(f"lpips tap C={C} {h}x{w} {dtype} past the cap: max rel err vs fp64 {err:.3e} (bound {RTOL:.1e})")
    assert err <= RTOL
    for src, dst in ((ad, pooled[:n]), (bd, pooled[n:])):
        want_p = F.max_pool2d(F.relu(src[:, 0].permute(0, 3, 1, 2).float()), 2).permute(0, 2, 3, 1).to(dtype)
        assert_bits(dst[:, 0].contiguous(), want_p.contiguous(), "pooled")
    again, pooled2 = ops.lpips_tap(ad, bd, lwd, pool=True)
    assert torch.equal(again, got) and torch.equal(pooled2, pooled)
