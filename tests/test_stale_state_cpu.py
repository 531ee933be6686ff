"""CPU side of the stale-state tests (tests/stale.py): the inventory of caches held against the package's source, the hit and miss
rules of blocks._Packed and of the weight tokens on CPU tensors, and the harness's own comparison."""
import gc

import pytest
import torch

import stale

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the inventory
def test_inventory_names_every_cache_site_of_the_package():
    """Every call site of weights_token / PACKED.get / capture_graph / replay_captured in the package belongs to a row of
    stale.INVENTORY, file by file and count by count: a cache added later fails here until it has a row (and a GPU case)."""
    found, listed = stale.scan_sites(), stale.table_sites()
    assert found, "the scan found no call site at all"
    assert found == listed, {k: (found.get(k, 0), listed.get(k, 0)) for k in sorted(set(found) | set(listed)) if found.get(k, 0) != listed.get(k, 0)}


def test_scan_counts_calls_and_not_definitions(tmp_path, monkeypatch):
    (tmp_path / "a.py").write_text("def weights_token(m):\n    return 0\nx = weights_token(1) + ops.weights_token(2)\n# PACKED.get( in a comment counts\n")
    (tmp_path / "b.txt").write_text("capture_graph(")
    monkeypatch.setattr(stale, "PACKAGE", str(tmp_path))
    assert stale.scan_sites() == {("a.py", "weights_token("): 2, ("a.py", "PACKED.get("): 1}


def test_every_row_names_existing_gpu_tests_and_every_baked_input_has_a_case():
    names = stale.gpu_test_names()
    assert names
    for r in stale.INVENTORY:
        assert r["cases"], r["cache"]
        for c in r["cases"]:
            assert c in names, f"{r['cache']}: {c} is not a test of tests/test_stale_state_gpu.py"
        for what, cases in r["bakes"].items():
            # the one input a GPU case cannot reach is covered below, on CPU tensors
            assert cases or what == "a freed module's id and storage reused", f"{r['cache']}: no case changes '{what}'"
    used = {c for r in stale.INVENTORY for c in r["cases"]}
    orphans = sorted(n for n in names - used if "follows" in n or "follow_" in n)
    assert not orphans, f"cases that no row of the inventory names: {orphans}"


# ------------------------------------------------------------------------------------------------ blocks._Packed
def counted(tag, log):
    return lambda: (log.append(tag), tag)[1]


def test_packed_hits_until_a_parameter_changes_version():
    from jointimagegeneration_amd.blocks import _Packed
    cache, log = _Packed(), []
    w, b = torch.nn.Parameter(torch.ones(4, 3)), torch.nn.Parameter(torch.zeros(4))
    assert cache.get(("k",), [w, b], counted("a", log)) == "a"
    assert cache.get(("k",), [w, b], counted("b", log)) == "a" and log == ["a"]
    b.add_(1.0)                                                 # in place: the version counter of ONE of the parameters
    assert cache.get(("k",), [w, b], counted("c", log)) == "c"
    assert cache.get(("k",), [w, b], counted("d", log)) == "c" and log == ["a", "c"]
    w.data.mul_(2.0)                                            # through .data: invisible, as ops.weights_token documents
    assert cache.get(("k",), [w, b], counted("e", log)) == "c"
    from jointimagegeneration_amd import ops
    holder = torch.nn.Module()
    holder.w, holder.b = w, b
    ops.invalidate_caches(holder)
    assert cache.get(("k",), [w, b], counted("f", log)) == "f"
    assert torch.equal(w, torch.full((4, 3), 2.0))              # the no-op write changed no value


def test_packed_misses_when_the_storage_moves_or_a_bias_appears():
    from jointimagegeneration_amd.blocks import _Packed
    cache, log = _Packed(), []
    w = torch.nn.Parameter(torch.ones(4, 3))
    cache.get(("k",), [w, None], counted("a", log))
    w.data = w.data.clone()                                     # what .to(device) does: same object, same version, other storage
    assert cache.get(("k",), [w, None], counted("b", log)) == "b"
    b = torch.nn.Parameter(torch.zeros(4))
    assert cache.get(("k",), [w, b], counted("c", log)) == "c"  # another parameter list under the same key
    assert cache.get(("k",), [w, None], counted("d", log)) == "d"
    assert cache.get(("k2",), [w, None], counted("e", log)) == "e" and cache.get(("k",), [w, None], counted("f", log)) == "d"


def test_packed_misses_for_a_new_module_on_a_freed_id_and_storage():
    """Python reuses id() once a module is freed, and the allocator hands its storage to the next tensor of that size: the key and the
    (data_ptr, _version) pair can both come back.  Here they are made to: the second parameter is a new tensor object on the first
    one's storage, under the key the first one had."""
    from jointimagegeneration_amd.blocks import _Packed
    cache, log = _Packed(), []
    def module(w, b):
        m = torch.nn.Module()
        m.weight, m.bias = torch.nn.Parameter(w), torch.nn.Parameter(b)
        return m
    m = module(torch.ones(4, 3), torch.zeros(4))
    key = (id(m), 32, "")
    store, bias_store = m.weight.detach(), m.bias.detach()
    assert cache.get(key, [m.weight, m.bias], counted("old", log)) == "old"
    ver = tuple((p.data_ptr(), p._version) for p in (m.weight, m.bias))
    del m
    gc.collect()
    n = module(store, bias_store)
    assert tuple((p.data_ptr(), p._version) for p in (n.weight, n.bias)) == ver
    assert cache.get(key, [n.weight, n.bias], counted("new", log)) == "new" and log == ["old", "new"]
    assert cache.get(key, [n.weight, n.bias], counted("again", log)) == "new"


def test_weights_token_sees_parameters_not_buffers():
    """What ops.weights_token answers for, stated once: in-place writes and moved storage of PARAMETERS.  Buffers (a schedule, LPIPS's
    shift / scale, BatchNorm's running statistics) are not in it, so a cache that bakes in a buffer needs the buffer in its own token."""
    from jointimagegeneration_amd import ops
    m = torch.nn.BatchNorm1d(4)
    t0 = ops.weights_token(m)
    m.running_mean.add_(1.0)
    assert ops.weights_token(m) == t0
    m.weight.mul_(2.0)
    t1 = ops.weights_token(m)
    assert t1 != t0
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    t2 = ops.weights_token(m)
    assert t2 != t1
    m.weight.data.mul_(2.0)
    assert ops.weights_token(m) == t2
    ops.invalidate_caches(m)
    assert ops.weights_token(m) != t2


def test_patchgan_token_sees_its_buffers():
    from jointimagegeneration_amd.aeloss import NLayerDiscriminator
    d = NLayerDiscriminator(input_nc=1, n_layers=2).eval()
    t0 = d._token()
    bn = next(b for _, b in d._layers() if b is not None)
    bn.running_var.mul_(1.5)
    assert d._token() != t0


def test_lpips_pack_key_sees_shift_and_scale():
    from jointimagegeneration_amd.lpips import LPIPS
    m = LPIPS().eval()
    k0 = m._pack_key()
    m.scaling_layer.shift.add_(0.25)
    k1 = m._pack_key()
    assert k1 != k0
    m.scaling_layer.scale = m.scaling_layer.scale.clone()       # replaced, not written
    assert m._pack_key() != k1
    assert m._pack_key() == m._pack_key()


# ------------------------------------------------------------------------------------------------ the chain token, on the host
def test_chain_token_holds_the_schedule_values():
    """The chain state's token on a CPU model: another schedule under the same timesteps and sigmas (eta = 0) is another token, through
    register_schedule and through a load_state_dict of the buffers alone; the same schedule again is the same token."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    from util import small_ldm
    m = small_ldm()
    s = DDIMSampler(m)
    s.make_schedule(5, ddim_eta=0.0, verbose=False)
    t0 = s.state_token()
    assert s.state_token() == t0
    m.register_schedule(linear_start=0.00085, linear_end=0.012)
    s.make_schedule(5, ddim_eta=0.0, verbose=False)
    t1 = s.state_token()
    assert t1[:3] == t0[:3] and t1 != t0                        # steps, timesteps and sigmas alone cannot tell the two apart
    other = small_ldm()
    m.load_state_dict({k: v for k, v in other.state_dict().items() if k in dict(other.named_buffers())}, strict=False)
    s.make_schedule(5, ddim_eta=0.0, verbose=False)
    assert s.state_token() == t0
    assert s.state_token(inpaint=True) != t0 and s.state_token(inpaint=True)[:len(t0)] == t0


# ------------------------------------------------------------------------------------------------ the harness
def test_same_compares_bits_shapes_and_lengths():
    a = torch.tensor([1.0, -0.0])
    assert stale.same(a, a.clone()) and stale.same((a, (a,)), (a.clone(), (a.clone(),)))
    assert not stale.same(a, torch.tensor([1.0, 1e-45]))
    assert not stale.same((a,), (a, a)) and not stale.same(a, a.view(1, 2)) and not stale.same(a, a.double())
    assert not stale.same(a, (a,))


def test_check_follows_passes_a_following_object_and_fails_a_stale_or_unmoved_one():
    """The harness on a host object with a cache: a version-keyed cache follows; a cache keyed by nothing is reported; a mutation that
    does not move the result is refused."""
    class Doubler:
        def __init__(self, model, keyed):
            self.model, self.keyed, self.hit = model, keyed, None

        def __call__(self):
            key = self.model.w._version if self.keyed else 0
            if self.hit is None or self.hit[0] != key:
                self.hit = (key, 2.0 * self.model.w.detach().clone())
            return self.hit[1]

    def make(keyed):
        def make_objects(model):
            if model is None:
                model = torch.nn.Module()
                model.w = torch.nn.Parameter(torch.arange(4.0))
            return model, Doubler(model, keyed)
        return make_objects
    run = lambda model, obj: obj()
    bump = lambda model, obj: model.w.mul_(1.5)
    stale.check_follows(make(True), run, bump)
    stale.check_follows(make(True), run, [bump, bump])
    with pytest.raises(AssertionError, match="does not return what fresh objects return"):
        stale.check_follows(make(False), run, bump)
    with pytest.raises(AssertionError, match="did not move the result"):
        stale.check_follows(make(True), run, lambda model, obj: model.w.add_(0.0))
    def switch(model, obj):
        model.w.add_(0.0)
    switch.moves = False
    stale.check_follows(make(True), run, [switch, bump])

    def loud_switch(model, obj):
        model.w.mul_(1.5)
    loud_switch.moves = False
    with pytest.raises(AssertionError, match="moved the result, and must not"):
        stale.check_follows(make(True), run, loud_switch)
    with pytest.raises(AssertionError, match="no captured graph is held"):
        stale.check_follows(make(True), run, bump, held=lambda obj: [None])
