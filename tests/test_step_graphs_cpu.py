"""parallel.StepGraphs, host side, without a GPU: the entry key, the live set and the fingerprint.

A captured graph replays the kernel arguments of its capture.  Whatever the launch-by-launch path reads on the host at
every call must therefore be in the entry's key (a change is another launch sequence) or in its fingerprint (a change makes
the captured addresses, or the set the captured backward differentiates, wrong).  These tests build a model on the host,
take the key / live list / fingerprint, change one such value, and look again; undoing the change must give the first key
back (the old entry is found again, not captured twice).  The device side of the same cases: test_step_graphs_gpu.py."""
import pytest
import torch
from torch import nn

ENV = [('ISTVT_STEM_MATERIALISE_A2', '1'), ('ISTVT_STEM_WGRAD_SIDE', '0'), ('ISTVT_STEM_PW_BWD_FUSED', '0'),
       ('ISTVT_BGRAD_SIDE', '1')]          # (variable, a value that is not its default)


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture()
def graphs(pkg, monkeypatch):
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    for name, _ in ENV:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(3)
    model = XceptionVidTr(num_frames=2, grid=6, depth=3, compute_dtype=torch.bfloat16).train()
    return model, parallel.StepGraphs(model, model._forward_eager)


X = torch.zeros(1, 2, 3, 91, 91)


def test_key_is_stable_and_host_only(graphs):
    model, g = graphs
    k = g.key(X, True)
    assert g.key(X, True) == k and hash(k) == hash(g.key(X, True))
    assert k[-1] is True and g.key(X, False)[-1] is False           # why_not() and the tests read grad / no_grad there
    assert g.key(X, False) != k
    assert g.key(torch.zeros(2, 2, 3, 91, 91), True) != k
    assert g.stats == {'captures': 0, 'replays': 0, 'eager': 0, 'recaptures': 0}


@pytest.mark.parametrize('path', ['xcep', 'xcep.model.block2', 'xcep.model.bn1', 'vit.transformer.layers.1.2.fn',
                                  'vit.transformer.layers.0.0', 'vit.transformer.layers.2.1.fn.to_out.1', 'vit.mlp_head'])
def test_key_follows_every_submodule_training_flag(graphs, path):
    """the kernels branch on xcep.training, each block's and each transformer module's own flag: the key holds them all"""
    model, g = graphs
    k = g.key(X, True)
    sub = model.get_submodule(path)
    sub.eval()
    assert model.training and g.key(X, True) != k
    sub.train()
    assert g.key(X, True) == k


def test_key_follows_dropout_p(graphs):
    model, g = graphs
    k = g.key(X, True)
    drops = [m for m in model.vit.transformer.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == 3 * 4                  # two attention output dropouts and two in the FeedForward, per layer
    for d in drops:
        d.p = 0.1
        k1 = g.key(X, True)
        assert k1 != k
        d.p = 0.3                               # the launch sequence depends on p > 0, not on the value (a kernel argument
        assert g.key(X, True) == k1             # of a forward that is never captured anyway)
        d.p = 0.0
        assert g.key(X, True) == k


@pytest.mark.parametrize('name,value', ENV)
def test_key_follows_each_environment_switch(graphs, monkeypatch, name, value):
    model, g = graphs
    k = g.key(X, True)
    monkeypatch.setenv(name, value)
    assert g.key(X, True) != k
    monkeypatch.delenv(name)
    assert g.key(X, True) == k
    default = {'1': '0', '0': '1'}[value]       # the default, spelled out, is the same launch sequence: the same key
    monkeypatch.setenv(name, default)
    assert g.key(X, True) == k


def test_env_switches_are_read_as_their_readers_read_them(pkg, monkeypatch):
    """env_switches() mirrors the four os.environ reads in stem.py / functional.py: the same names, the same defaults and
    the same comparisons (checked against the source text, so a reader that changes shows up here)"""
    import inspect
    from istvt_amd import functional, parallel, stem
    for name, _ in ENV:
        monkeypatch.delenv(name, raising=False)
    assert parallel.env_switches() == (False, True, True, False)
    reads = {"os.environ.get('ISTVT_STEM_MATERIALISE_A2', '0') != '1'": stem,
             "os.environ.get('ISTVT_STEM_WGRAD_SIDE', '1') != '0'": stem,
             "os.environ.get('ISTVT_STEM_PW_BWD_FUSED', '1') != '0'": stem,
             "os.environ.get('ISTVT_BGRAD_SIDE', '0') == '1'": functional}
    for text, mod in reads.items():
        assert inspect.getsource(mod).count(text) == 1, text


def test_key_follows_a_middle_layers_fp8_and_dead_row_flags(graphs):
    model, g = graphs
    k = g.key(X, True)
    mid = model.vit.transformer.layers[1][1].fn
    assert hasattr(mid, 'attn_fp8') and not mid.attn_fp8
    mid.attn_fp8 = True
    assert g.key(X, True) != k
    mid.attn_fp8 = False
    assert g.key(X, True) == k
    model.set_dead_row_elimination(True)
    assert g.key(X, True) != k
    model.set_dead_row_elimination(False)
    assert g.key(X, True) == k


def test_live_list_follows_requires_grad_and_swapped_submodules(graphs):
    from istvt_amd import parallel
    model, g = graphs

    def same(a, b):
        return len(a) == len(b) and all(p is q for p, q in zip(a, b))

    def named():
        return [p for _, p in parallel.live_named_parameters(model)]
    live0 = g.live_parameters()
    assert same(live0, named()) and len(live0) > 50
    fp0 = g._fingerprint(False)
    assert g._fingerprint(False) == fp0
    # freezing / unfreezing: a head weight and a stem convolution weight
    w_head, w_stem = model.vit.mlp_head[1].weight, model.xcep.model.conv2.weight
    for w in (w_head, w_stem):
        assert any(p is w for p in live0)
        w.requires_grad_(False)
        live = g.live_parameters()
        assert same(live, named()) and len(live) == len(live0) - 1 and not any(p is w for p in live)
        assert g._fingerprint(False) != fp0
        w.requires_grad_(True)
        assert same(g.live_parameters(), live0) and g._fingerprint(False) == fp0
    # the never-executed Xception tail stays out, whatever its flags
    tail = model.xcep.model.block5.rep[1].pointwise.weight
    assert tail.requires_grad and not any(p is tail for p in live0)
    # a parameter replaced inside its module: same tree, new tensor
    old = model.vit.mlp_head[1].bias
    model.vit.mlp_head[1].bias = nn.Parameter(old.detach().clone())
    live = g.live_parameters()
    assert same(live, named()) and not any(p is old for p in live)
    assert g._fingerprint(False) != fp0
    # a submodule swapped in: the cached module list is rebuilt (and with it the key's flags)
    k = g.key(X, True)
    idx = g.index()
    assert g.index() is idx
    head = nn.Linear(728, 1)
    model.vit.mlp_head[1] = head
    live = g.live_parameters()
    assert g.index() is not idx
    assert same(live, named()) and any(p is head.weight for p in live) and any(p is head.bias for p in live)
    assert g.key(X, True) == k                  # same flags: the fingerprint, not the key, tells the two heads apart
    head.eval()
    assert g.key(X, True) != k                  # the new module's flag is read, not the old one's
    head.train()
    # a module added to the tree
    idx = g.index()
    model.vit.extra = nn.Dropout(0.5)
    assert g.key(X, True) != k and g.index() is not idx
    del model.vit.extra
    assert g.key(X, True) == k


def test_fingerprint_needs_fused_gradient_views(graphs):
    """with gradients enabled every live parameter's gradient has to be a view of a fused bucket; the identities are part of
    the fingerprint, not only the addresses"""
    from istvt_amd import parallel
    model, g = graphs
    assert g._fingerprint(True) is None
    live = g.live_parameters()
    bucket = parallel.GradBucket(live, fuse_accumulate=True)
    fp = g._fingerprint(True)
    assert fp is not None and len(fp) == 3 * len(live)
    assert all(id(p) in fp and p.data_ptr() in fp and p.grad.data_ptr() in fp for p in live)
    w = model.vit.mlp_head[1].weight
    saved, w.grad = w.grad, None
    assert g._fingerprint(True) is None
    w.grad = saved
    assert g._fingerprint(True) == fp
    # another tensor at the same address is another parameter
    twin = nn.Parameter(w.detach())
    assert twin.data_ptr() == w.data_ptr()
    twin.grad, twin._istvt_fused_grad = w.grad, True
    model.vit.mlp_head[1].weight = twin
    assert g._fingerprint(True, g.live_parameters()) != fp
    del bucket


def test_a_changed_module_tree_drops_what_was_captured(graphs):
    """graphs, warm-up counts and the not-capturable marks belong to the module tree they were made with"""
    model, g = graphs
    k = g.key(X, True)
    g.entries[k] = object()
    g.seen[k] = 5
    g.nocapture[k] = 'x'
    model.vit.mlp_head[1] = nn.Linear(728, 1)
    g.key(X, True)
    assert not g.entries and not g.seen and not g.nocapture and g.stats['recaptures'] == 1


def test_the_cached_module_list_is_no_cycle_through_the_model(pkg):
    """model -> StepGraphs -> module list must not lead back to the model: a model with captured graphs has to die by
    reference count (its graphs' memory pools and static-address mode go with it), not whenever the collector runs"""
    import gc
    import weakref
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=2, grid=6, depth=1).train()
    model.enable_step_graphs(True)
    g = model._step_graphs
    g.key(X, True)
    g.live_parameters()
    assert g.index().modules and g.live
    gone = weakref.ref(model)
    head = weakref.ref(model.vit.mlp_head[1].weight)
    gc.collect()
    gc.disable()
    try:
        del model, g
        assert gone() is None and head() is None
    finally:
        gc.enable()


def test_dropout_detection_leaves_the_generator_alone(graphs, monkeypatch):
    """the key and the live set read flags only; the seed-draw counter counts functional._new_seed() calls and is what
    StepGraphs compares across a warm-up forward -- neither consumes nor perturbs torch's CPU generator"""
    from istvt_amd import functional as Fn
    model, g = graphs
    for m in model.vit.transformer.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.1
    torch.manual_seed(17)
    state = torch.get_rng_state()
    g.key(X, True)
    g.live_parameters()
    g._fingerprint(False)
    _ = Fn.seed_draws[0]
    assert torch.equal(torch.get_rng_state(), state)
    # a warm-up forward that draws is marked not capturable, with the draws of the launch-by-launch forward and no more:
    # the device work is replaced by a forward that only draws, the preconditions by "fine"
    drawn = []

    def forward(x):
        drawn.append((Fn._new_seed(), Fn._new_seed()))
        return x
    g._fwd = lambda: forward
    monkeypatch.setattr(g, 'why_not', lambda x, key: None)
    monkeypatch.setattr(g, '_fingerprint', lambda grads, live=None: ())
    n0 = Fn.seed_draws[0]
    for _ in range(4):                          # two warm-up calls would do; the later ones must not capture either
        g(X)
    assert Fn.seed_draws[0] == n0 + 8
    assert g.stats == {'captures': 0, 'replays': 0, 'eager': 4, 'recaptures': 0} and not g.entries
    assert 'dropout' in g.last_reason and list(g.nocapture) == [g.key(X, True)]
    torch.manual_seed(17)
    expect = [(Fn._new_seed(), Fn._new_seed()) for _ in range(4)]
    assert drawn == expect                      # the generator saw exactly the loop's own draws, in order
    # eval mode is another key and is not marked
    model.eval()
    assert g.key(X, False) not in g.nocapture
