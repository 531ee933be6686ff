"""GPU suite (-m gpu): every cache and captured graph follows its inputs (tests/stale.py holds the harness and the inventory).

Each case runs one long-lived object (a sampler, a pipeline, a loss module) three times, so that its state holds a captured graph,
changes one thing the state was built from, runs it three more times, and requires the results to equal, bit for bit, those of freshly
built objects on the changed model (stale.check_follows).  The models are the small ones of the other suites: the 8 x 8, 4-channel
LatentDiffusion of test_split_gpu.py, the CCDM of test_losses_gpu.py on six steps, the pipeline of test_volumes_gpu.py; N = 2, S = 5.

What these cases found when they were written (each returned a result of the old input, silently): the chain state kept its step scalar
table, and the inpainting state its q_sample table, across a schedule change at eta = 0 (DDIM, PLMS, DPM-Solver on a fixed grid;
through register_schedule, given_betas and a load_state_dict of the buffers); the pipeline's sampler kept the schedule it was built
on; the chain graph kept the fuse_ddim it was captured under; the slice engines kept a float scale_factor, and a replaced
scale_by_std buffer; LPIPS kept a replaced shift / scale.  The fixes are in the tokens: DDIMSampler.state_token / refresh_schedule,
GuideGenPipeline._engine, LPIPS._pack_key."""
import json
import os

import numpy as np
import pytest
import torch

from stale import check_follows, launches
from util import GOLD, LDM_SMALL, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
START, END = 0.00085, 0.012                 # the other linear schedule (the models are built on 0.0015 .. 0.0195)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def x(dev):
    gen = torch.Generator().manual_seed(4096)
    r = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    hole = torch.ones(2, 1, 8, 8, device=dev)
    hole[:, :, 2:6, 2:6] = 0.0
    return dict(c=r(2, 4, 8, 8), c2=r(2, 4, 8, 8), uc=r(2, 4, 8, 8), x_T=r(2, 4, 8, 8), x_T2=r(2, 4, 8, 8), x0=r(2, 4, 8, 8),
                tape=[r(2, 4, 8, 8) for _ in range(5)], qtape=[r(2, 4, 8, 8) for _ in range(5)], hole=hole,
                c12=r(2, 4, 12, 12), x12=r(2, 4, 12, 12))


def ldm_model(dev, prefix="ldm_split_vq."):
    """The small LatentDiffusion with the VQ first stage (quantize_x0 needs its codebook; every other case ignores the first stage)."""
    from test_split_gpu import build_ldm
    return build_ldm(dev, "vq", prefix)


def scale(t, f=1.5):
    t.mul_(f)


def reschedule(dev, **kw):
    def mutate(model, obj):
        model.register_schedule(**kw)
        model.to(dev)                       # register_schedule leaves CPU buffers; the parameters are where they were
    return mutate


def schedule_buffers(dev, **kw):
    """The schedule buffers of a model registered on another schedule, as a state_dict of the buffers alone."""
    other = ldm_model(dev)
    other.register_schedule(**kw)
    return {k: v.to(dev) for k, v in other.state_dict().items() if "." not in k}


def sampler_case(dev, x, mutate, cls=None, kw=None, attrs=None, need_graph=True, shape=(4, 8, 8), prepare=None):
    """check_follows on a sampler of the small LDM.  `kw` (sample's keywords) and `attrs` (attributes of the sampler) are dicts the
    mutations may change: the fresh sampler is built and run with what they hold then."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    cls = cls or DDIMSampler
    kw = kw if kw is not None else {}
    attrs = attrs if attrs is not None else {}
    big = shape[-1] == 12

    def make_objects(model):
        if model is None:
            model = ldm_model(dev)
            if prepare is not None:
                prepare(model)
        s = cls(model)
        for k, v in attrs.items():
            setattr(s, k, v)
        return model, s

    def run(model, s):
        z, inter = s.sample(S=5, batch_size=2, shape=shape, conditioning=x["c12" if big else "c"], verbose=False,
                            x_T=x["x12" if big else "x_T"], **kw)
        flag = torch.tensor([bool(s.last_step_fused)])
        return (z, flag) + tuple(inter["x_inter"]) + tuple(inter["pred_x0"])

    held = (lambda s: [st["graph"] for st in s._graphs.values()]) if need_graph else None
    check_follows(make_objects, run, mutate, held)


def unet_of(model):
    return model.model.diffusion_model


WEIGHTS = {"head conv weight": lambda u: u.out[2].weight, "GroupNorm gamma": lambda u: u.out[0].weight,
           "time_embed[0].weight": lambda u: u.time_embed[0].weight}


# ------------------------------------------------------------------------------------------------ 0. the harness can fail
def test_harness_reports_a_planted_stale_token(dev, x, monkeypatch):
    """A host defect planted on purpose: ops.weights_token answers a constant, so the chain state and its graph survive a weight change.
    The head-conv case must now report the mismatch (the replay reads the old packed weight, which blocks.PACKED still holds)."""
    from jointimagegeneration_amd import ops
    monkeypatch.setattr(ops, "weights_token", lambda module: (0, 0, 0))
    with pytest.raises(AssertionError, match="does not return what fresh objects return"):
        sampler_case(dev, x, lambda model, s: scale(WEIGHTS["head conv weight"](unet_of(model))))


# ------------------------------------------------------------------------------------------------ 1. the LDM chain state
@pytest.mark.parametrize("sampler", ["ddim", "plms"])
@pytest.mark.parametrize("which", list(WEIGHTS))
def test_ldm_chain_follows_a_weight_written_in_place(dev, x, which, sampler):
    """Three weights, three caches: the head conv's weight is repacked (blocks.PACKED) and its pack's address is in the graph; a GroupNorm
    gamma is read in place by the graph; time_embed feeds the time-bias table of the state."""
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    sampler_case(dev, x, lambda model, s: scale(WEIGHTS[which](unet_of(model))), cls=DDIMSampler if sampler == "ddim" else PLMSSampler,
                 need_graph=sampler == "ddim")


def test_ldm_chain_follows_load_state_dict(dev, x):
    def mutate(model, s):
        other = ldm_model(dev, "ldm_other.")
        model.load_state_dict({k: v.clone() for k, v in other.state_dict().items()})
    sampler_case(dev, x, mutate)


def test_ldm_chain_follows_a_data_write_after_invalidate_caches(dev, x):
    from jointimagegeneration_amd import ops

    def mutate(model, s):
        for get in WEIGHTS.values():
            get(unet_of(model)).data.mul_(1.5)                  # invisible to the version counter ...
        ops.invalidate_caches(model)                            # ... so the writer says so
    sampler_case(dev, x, mutate)


SCHEDULES = ["register_schedule", "load_state_dict of the buffers", "given_betas"]


def schedule_mutation(dev, how):
    if how == "register_schedule":
        return reschedule(dev, linear_start=START, linear_end=END)
    if how == "given_betas":
        return reschedule(dev, given_betas=np.linspace(START ** 0.5, END ** 0.5, 1000, dtype=np.float64) ** 2 * 1.25)
    return lambda model, s: model.load_state_dict(schedule_buffers(dev, linear_start=START, linear_end=END), strict=False)


@pytest.mark.parametrize("sampler", ["ddim", "plms"])
@pytest.mark.parametrize("how", SCHEDULES)
def test_ldm_chain_follows_the_schedule(dev, x, how, sampler):
    """Another schedule under the same step count at eta = 0: the timesteps and the sigmas (all 0) are what they were, only the alphas
    of the step scalar table moved."""
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    sampler_case(dev, x, schedule_mutation(dev, how), cls=DDIMSampler if sampler == "ddim" else PLMSSampler, need_graph=sampler == "ddim")


@pytest.mark.parametrize("how", SCHEDULES[:2])
def test_inpainting_state_follows_the_schedule(dev, x, how):
    """The inpainting state's q_sample table (ip_scal) reads the model's sqrt_alphas_cumprod buffers."""
    sampler_case(dev, x, schedule_mutation(dev, how), kw=dict(mask=x["hole"], x0=x["x0"], mask_noise_tape=x["qtape"]))


def test_ldm_chain_follows_discretisation_and_eta(dev, x):
    kw = {}
    to = lambda **new: (lambda model, s: (kw.clear(), kw.update(new)))
    sampler_case(dev, x, [to(ddim_discretize="quad"), to(), to(eta=0.5, noise_tape=x["tape"]), to()], kw=kw)


@pytest.mark.parametrize("how", ["written in place", "replaced"])
def test_vq_state_follows_the_codebook(dev, x, how):
    def mutate(model, s):
        emb = model.first_stage_model.quantize.embedding
        if how == "replaced":
            emb.weight = torch.nn.Parameter(emb.weight.detach() * 0.75, requires_grad=False)
        else:
            emb.weight.mul_(0.75)
    sampler_case(dev, x, mutate, kw=dict(quantize_x0=True))


def test_split_state_follows_its_geometry(dev, x):
    from test_split_gpu import SPLIT

    def prepare(model):
        model.split_input_params = dict(SPLIT)

    def mutate(model, s):
        model.split_input_params["stride"] = (2, 2)             # the same dict, one value: 4 crops of 8 x 8 become 9
    sampler_case(dev, x, mutate, shape=(4, 12, 12), prepare=prepare)


def test_logged_state_follows_log_every_t(dev, x):
    kw = dict(log_every_t=2)
    sampler_case(dev, x, lambda model, s: kw.update(log_every_t=1), kw=kw)


def test_ldm_chain_follows_fuse_ddim_and_use_graph(dev, x):
    """fuse_ddim (the update as the head conv's epilogue, or as its own launch) is read while the chain is captured; the result carries
    the sampler's last_step_fused, which the toggled sampler must report as a fresh one does.  use_graph off and on again: the eager
    chain and the replayed one agree bit for bit by the project's own rule, so those two switches must not move the result; a weight
    changes while the graph is off, and the graph that comes back must be one of the new weight."""
    attrs = {}

    def setter(name, value, moves):
        def mutate(model, s):
            attrs[name] = value
            setattr(s, name, value)
        mutate.moves = moves
        return mutate
    sampler_case(dev, x, [setter("fuse_ddim", False, True), setter("fuse_ddim", True, True)], attrs=attrs)
    attrs.clear()
    sampler_case(dev, x, [setter("use_graph", False, False), lambda model, s: scale(WEIGHTS["head conv weight"](unet_of(model))),
                          setter("use_graph", True, False)], attrs=attrs)


def test_same_shape_inputs_reuse_state_and_graph(dev, x):
    """What must NOT rebuild anything: a new conditioning of the same shape, a new x_T, a new guidance scale, and a new temperature on a
    VQ state.  Same state object, same graph object, the launches of an unchanged call -- and still the result of a fresh sampler."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    model = ldm_model(dev)

    def run(s, **kw):
        kw.setdefault("x_T", x["x_T"])
        kw.setdefault("conditioning", x["c"])
        return s.sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, **kw)[0]
    s = DDIMSampler(model)
    base = [run(s) for _ in range(3)]
    (key, st), = s._graphs.items()
    graph = st["graph"]
    assert graph is not None
    _, n_same = launches(lambda: run(s))
    assert n_same["capture_graph"] == 0 and n_same["pack_conv_weight"] == 0 and n_same["conv"] == 0      # a replay
    for change in (dict(conditioning=x["c2"]), dict(x_T=x["x_T2"]), dict(conditioning=x["c2"], x_T=x["x_T2"])):
        got, n = launches(lambda: run(s, **change))
        assert s._graphs[key] is st and st["graph"] is graph and n == n_same, sorted(change)
        assert torch.equal(got, run(DDIMSampler(model), **change)) and not torch.equal(got, base[2]), sorted(change)
    guided = {}
    for g in (3.0, 5.0):
        kw = dict(unconditional_guidance_scale=g, unconditional_conditioning=x["uc"])
        got, guided[g] = launches(lambda: run(s, **kw))
        assert s._graphs[key] is st and st["graph"] is graph and list(s._graphs) == [key]
        assert torch.equal(got, run(DDIMSampler(model), **kw))
    assert guided[3.0] == guided[5.0] and guided[3.0]["capture_graph"] == 0 and guided[3.0]["pack_conv_weight"] == 0
    assert torch.equal(run(s), base[2]) and s._graphs[key] is st and st["graph"] is graph
    # temperature on a VQ state at eta = 0.6: the fifth scalar column is rewritten in place, nothing is rebuilt
    hot = dict(quantize_x0=True, eta=0.6, noise_tape=x["tape"])
    v = DDIMSampler(model)
    cold = [run(v, **hot) for _ in range(3)]
    vkey, = [k for k in v._graphs if k[-1] == ("vq", True)]
    vst = v._graphs[vkey]
    _, n_cold = launches(lambda: run(v, **hot))
    got, n_hot = launches(lambda: run(v, temperature=0.7, **hot))
    assert v._graphs[vkey] is vst and n_hot == n_cold and n_hot["pack_conv_weight"] == 0
    assert torch.equal(got, run(DDIMSampler(model), temperature=0.7, **hot)) and not torch.equal(got, cold[2])
    assert torch.equal(run(v, **hot), cold[2]) and v._graphs[vkey] is vst


# ------------------------------------------------------------------------------------------------ 2. DPM-Solver++
@pytest.mark.parametrize("what", ["weight", "schedule, logsnr grid", "schedule, uniform grid", "order", "clip_denoised"])
def test_dpm_solver_chain_follows(dev, x, what):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    kw, attrs = {}, {}
    if what == "weight":
        mutate = lambda model, s: scale(WEIGHTS["head conv weight"](unet_of(model)))
    elif what.startswith("schedule"):
        if "uniform" in what:
            kw["ddim_discretize"] = "uniform"                    # the timesteps stay: only the solver's rows move
        mutate = reschedule(dev, linear_start=START, linear_end=END)
    elif what == "order":
        def mutate(model, s):
            attrs["order"] = s.order = 1
    else:
        mutate = lambda model, s: kw.update(clip_denoised=True)
    sampler_case(dev, x, mutate, cls=DPMSolverSampler, kw=kw, attrs=attrs)


# ------------------------------------------------------------------------------------------------ 3. the pipeline's engines
def pipeline_case(dev, mutate, scale_by_std=False):
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    from test_full_size_configs import _small_ccdm, _small_ldm
    ccdm = _small_ccdm(dev)

    def make_objects(model):
        if model is None:
            model = _small_ldm(dev)
            if scale_by_std:                                     # scale_factor as the buffer that scale_by_std registers
                del model.scale_factor
                model.scale_by_std = True
                model.register_buffer("scale_factor", torch.tensor(1.0, device=dev))
        return model, GuideGenPipeline(ccdm, model, ddim_steps=5)

    def run(model, pipe):
        l1, ct1 = pipe.run_volume(N=2, mask_size=(16, 16, 16), depth=7, hw=32, seed=5, max_slices=2)
        l2, ct2 = pipe.run_volumes([3, 4], mask_size=(16, 16, 16), depth=7, hw=32, max_slices=2)
        return l1, ct1, l2, ct2

    def held(pipe):
        assert len(pipe._slice_graphs) == 1 and len(pipe._volume_graphs) == 1
        return [e["slice"] for e in pipe._slice_graphs.values()] + [e["graph"] for e in pipe._volume_graphs.values()]
    check_follows(make_objects, run, mutate, held)


def first_conv_weight(module):
    return next(p for p in module.parameters() if p.ndim >= 4)


@pytest.mark.parametrize("stage", ["cond_stage_model", "first_stage_model"])
def test_pipeline_follows_a_stage_weight(dev, stage):
    """The halves the slice loop runs: the cond stage's encoder, the first stage's decoder."""
    half = lambda model: model.cond_stage_model.encoder if stage == "cond_stage_model" else model.first_stage_model.decoder
    pipeline_case(dev, lambda model, pipe: scale(first_conv_weight(half(model))))


@pytest.mark.parametrize("how", ["float", "buffer written in place", "buffer replaced"])
def test_pipeline_follows_scale_factor(dev, how):
    """decode_head divides by ldm.scale_factor: a Python float is folded into the captured launch, the scale_by_std buffer is read by it."""
    def mutate(model, pipe):
        if how == "float":
            model.scale_factor = 0.5
        elif how == "buffer replaced":
            model.scale_factor = torch.tensor(0.5, device=dev)
        else:
            model.scale_factor.fill_(0.5)
    pipeline_case(dev, mutate, scale_by_std=how != "float")


def test_pipeline_follows_the_schedule(dev):
    """The pipeline builds its sampler, and the sampler its schedule tables, once; the model's schedule changes while both live on."""
    pipeline_case(dev, reschedule(dev, linear_start=START, linear_end=END))


# ------------------------------------------------------------------------------------------------ 4. CCDM
def ccdm_case(dev, mutate):
    import losses_ref as R

    def make_objects(model):
        model = model if model is not None else R.ccdm_loss_model().to(dev)
        return model, model

    def run(model, _):
        g = torch.Generator().manual_seed(7)
        x_T = torch.randint(0, R.CCDM_K, (2, 8, 8, 8), generator=g, dtype=torch.int32).to(dev)
        model.philox_seed = 11
        labels, probs = model.sample_labels(x_T, torch.zeros(2, 1, 8, 8, 8, device=dev), 6)
        return labels, probs
    check_follows(make_objects, run, mutate)


def test_ccdm_labels_follow_a_unet_weight(dev):
    ccdm_case(dev, lambda model, _: scale(first_conv_weight(model.unet), 2.0))


def test_ccdm_labels_follow_the_schedule(dev):
    def mutate(model, _):
        from jointimagegeneration_amd.ccdm import DiffusionModel
        d = model.diffusion
        other = DiffusionModel("linear", d.time_steps, d.num_classes, dims=3)
        d.load_state_dict({k: v.to(dev) for k, v in other.state_dict().items()})
    ccdm_case(dev, mutate)


# ------------------------------------------------------------------------------------------------ 5. LPIPS and the AE loss module
def loss_case(dev, mutate):
    """The 2-D loss module of test_aeloss_gpu.py (case d2_base: LPIPS term and a 3-layer frame discriminator with BatchNorm) on the
    fixture's inputs; both optimizer indices, every logged value."""
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    from test_aeloss_gpu import build_loss
    gold = dict(np.load(os.path.join(GOLD, "aeloss.npz")))
    with open(os.path.join(GOLD, "aeloss_surface.json")) as f:
        meta = json.load(f)
    case = next(c for c in meta["cases"] if c["name"] == "d2_base")
    xs, ys, mom = (torch.from_numpy(gold[f"{k}2"]).to(dev) for k in ("x", "y", "mom"))
    mode = dict(fp32=False)

    def make_objects(model):
        fresh = build_loss(gold, meta, case, dev)
        if model is not None:                                    # the mutated module's parameters AND buffers, into a new module
            fresh.load_state_dict(model.state_dict(), strict=False)
            mine = dict(fresh.named_buffers())
            for name, b in model.named_buffers():
                mine[name].copy_(b)
            return model, fresh
        return fresh, fresh

    def run(model, m):
        import contextlib
        from jointimagegeneration_amd import ops
        with (ops.fp32_validation() if mode["fp32"] else contextlib.nullcontext()):
            post = DiagonalGaussianDistribution(mom)
            l0, d0 = m(xs, ys, post, 0, case["step"], last_layer=None, split="val")
            l1, d1 = m(xs, ys, post, 1, case["step"], last_layer=None, split="val")
        return (l0, l1) + tuple(d0.values()) + tuple(d1.values())
    check_follows(make_objects, run, mutate(mode) if getattr(mutate, "takes_mode", False) else mutate)


@pytest.mark.parametrize("which", ["VGG conv", "LPIPS lin", "discriminator conv"])
def test_loss_modules_follow_a_conv_weight(dev, which):
    def mutate(model, m):
        if which == "VGG conv":
            scale(model.perceptual_loss.net.slice2.get_submodule("5").weight)
        elif which == "LPIPS lin":
            scale(model.perceptual_loss.lin2.model.get_submodule("1").weight)
        else:
            scale(model.frame_discriminator._layers()[1][0].weight)
    loss_case(dev, mutate)


@pytest.mark.parametrize("how", ["written in place", "replaced"])
def test_lpips_follows_shift_and_scale(dev, how):
    def mutate(model, m):
        sc = model.perceptual_loss.scaling_layer
        if how == "replaced":
            sc.shift, sc.scale = sc.shift + 0.25, sc.scale * 1.5
        else:
            sc.shift.add_(0.25)
            sc.scale.mul_(1.5)
    loss_case(dev, mutate)


def test_discriminator_follows_a_running_statistic(dev):
    def mutate(model, m):
        bn = next(b for _, b in model.frame_discriminator._layers() if b is not None)
        bn.running_var.mul_(2.0)
        bn.running_mean.add_(0.1)
    loss_case(dev, mutate)


def test_loss_modules_follow_fp32_validation_entered_and_left(dev):
    def mutate(mode):
        return [lambda model, m: mode.update(fp32=True), lambda model, m: mode.update(fp32=False)]
    mutate.takes_mode = True
    loss_case(dev, mutate)


# ------------------------------------------------------------------------------------------------ 6. the GroupNorm statistics arena
@pytest.fixture()
def unet_run(dev):
    """The small latent UNet of smoke() and one eager forward of it, N = 2 at 16 x 16: (the module, the forward)."""
    from jointimagegeneration_amd.unet import UNetModel
    u = seeded(UNetModel(**LDM_SMALL), "smoke.").to(dev)
    gen = torch.Generator().manual_seed(5)
    xin, t = torch.randn(2, 8, 16, 16, generator=gen).to(dev), torch.tensor([981, 400], device=dev)
    return u, lambda: u(xin, t)


def recorded_acc(fn):
    """fn() with ops.conv wrapped: (result, [acc is not None] per conv whose output could carry statistics (bf16))."""
    from jointimagegeneration_amd import ops
    seen = []
    real = ops.conv

    def conv(*a, **k):
        out = real(*a, **k)
        if out.t.dtype == torch.bfloat16:
            seen.append(out.acc is not None)
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "conv", conv)
        return fn(), seen


def test_arena_of_zero_entries_equals_gn_acc_off(dev, unet_run, monkeypatch):
    """An arena that refuses every allocation and GN_ACC = False both run the ladder without accumulators: the same bits."""
    from jointimagegeneration_amd import ops
    _, unet_run = unet_run
    monkeypatch.setattr(ops, "_ARENAS", {})
    monkeypatch.setattr(ops, "_ARENA_ENTRIES", 0)
    full, seen = recorded_acc(unet_run)
    assert seen and not any(seen)
    monkeypatch.setattr(ops, "GN_ACC", False)
    off, seen_off = recorded_acc(unet_run)
    assert len(seen_off) == len(seen) and not any(seen_off)
    assert torch.equal(full, off)


def test_arena_filling_mid_forward_stays_in_bounds_and_leaves_nothing(dev, unet_run, monkeypatch):
    """The arena runs out in the middle of a forward: the convs before that point leave their sums, the ones after it are refused and
    their norms take the statistics launches.  The kernel ladder changes at that point, so the forward is held against the bounds the
    shadow derives per call, not against the ample forward's bits.  The limit is lowered on an arena allocated at the ample size (the
    allocator never hands out more than the limit, the buffer is never smaller than it).  A forward with the ample limit afterwards, on
    that same arena, equals the forward of a new arena bit for bit: the half-filled forward left no sums behind."""
    from jointimagegeneration_amd import ops
    from shadow import shadow_ops
    unet, unet_run = unet_run
    ample = ops._ARENA_ENTRIES
    monkeypatch.setattr(ops, "_ARENAS", {})
    want, seen = recorded_acc(unet_run)
    used = ops._ARENAS[str(dev)]["off"]
    assert sum(seen) >= 2 and 0 < used <= ample, (sum(seen), used)
    arena = ops._ARENAS[str(dev)]
    monkeypatch.setattr(ops, "_ARENA_ENTRIES", used // 2)       # below the forward's need, above its first allocations
    with shadow_ops() as sh:
        ops.invalidate_caches(unet)                             # the shadow keeps the weights it sees packed: repack under it
        _, seen_half = recorded_acc(unet_run)
        torch.cuda.synchronize()
    print(sh.summary("small UNet, arena full mid-forward"))
    sh.assert_within_bounds(2)
    assert any(seen_half) and sum(seen_half) < sum(seen), (sum(seen_half), sum(seen))           # some received acc, some were refused
    assert ops._ARENAS[str(dev)] is arena and arena["off"] <= used // 2
    monkeypatch.setattr(ops, "_ARENA_ENTRIES", ample)
    again, seen_again = recorded_acc(unet_run)
    assert ops._ARENAS[str(dev)] is arena and seen_again == seen
    monkeypatch.setattr(ops, "_ARENAS", {})
    fresh, _ = recorded_acc(unet_run)
    assert torch.equal(again, fresh) and torch.equal(again, want)
