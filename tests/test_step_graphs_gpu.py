"""parallel.StepGraphs on a real MI355X: every host value a capture would freeze.

A captured HIP graph replays the kernel arguments of its capture.  What the launch-by-launch path reads on the host at every
call -- dropout seeds, each submodule's train / eval flag, which parameters require a gradient, which modules hang in the
tree, four environment switches, each attention module's fp8 flag -- must therefore either be part of an entry's key or
fingerprint, or keep the step out of the graphs.  Each test brings a graphed model to a captured, replaying state, changes
one of these values, and goes on training.

The definition is a launch-by-launch twin built from the same seed (itself held to fp64 elsewhere in the suite); every
sequence runs on both.  "The same bits" is torch.equal on the logits of every step, on the flat gradient bucket after
every backward, on the flat parameter buffer after every optimizer step and on every BatchNorm running statistic and batch
counter.  Shapes: the twin scheme of test_model_gpu._graph_pair (restated here), the smallest the stem's 139 -> 9 grid
allows.  The host side of the same cases, without a GPU: test_step_graphs_cpu.py."""
import gc

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

ENV = [('ISTVT_STEM_MATERIALISE_A2', '1'), ('ISTVT_STEM_WGRAD_SIDE', '0'), ('ISTVT_STEM_PW_BWD_FUSED', '0'),
       ('ISTVT_BGRAD_SIDE', '1')]          # (variable, a value that is not its default)


def _bn_state(module):
    """every BatchNorm running statistic and batch counter under `module`, as one tensor"""
    return torch.cat([v.detach().reshape(-1).double() for k, v in module.named_buffers()
                      if 'running' in k or 'num_batches' in k])


class Twins:
    """two XceptionVidTr from one seed with GradBucket(fuse_accumulate, flatten_params) + FusedSGD; the second one with
    enable_step_graphs(True)"""

    def __init__(self, depth=2, T=4, side=139, B=3, grid=9):
        import istvt_pkg
        istvt_pkg.load()
        from istvt_amd import parallel
        from istvt_amd.network.vivit.vivit import XceptionVidTr
        self.parallel = parallel
        self.made = []
        for graphs in (False, True):
            torch.manual_seed(5)
            model = XceptionVidTr(num_frames=T, grid=grid, depth=depth, compute_dtype=torch.bfloat16).cuda().train()
            if graphs:
                model.enable_step_graphs(True)
            self.made.append((model,) + self.bucket_for(model))
        g = torch.Generator().manual_seed(6)
        self.xs = [torch.randn((B, T, 3, side, side), generator=g).cuda() for _ in range(2)]
        self.ys = [(torch.rand((B,), generator=g) > 0.5).float().cuda() for _ in range(2)]
        self.crit = nn.BCEWithLogitsLoss()
        self.g = self.made[1][0]._step_graphs
        self.steps = 0

    def bucket_for(self, model):
        live = [p for _, p in self.parallel.live_named_parameters(model)]
        bucket = self.parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
        return bucket, self.parallel.FusedSGD(bucket, lr=1e-2, momentum=0.9, zero_grad=True)

    @property
    def models(self):
        return [m for m, _, _ in self.made]

    def each(self, fn, seed=None):
        """fn(model, bucket, optimizer) on the launch-by-launch twin, then on the graphed one (torch's CPU generator seeded
        before each when `seed` is given); the two results must be the same bits.  Returns the twin's."""
        res = []
        for model, bucket, opt in self.made:
            if seed is not None:
                torch.manual_seed(seed)
            res.append(fn(model, bucket, opt))
        torch.cuda.synchronize()
        same(res[0], res[1])
        return res[0]

    def train_step(self, model, bucket, opt, i):
        opt.zero_grad()
        logits = model(self.xs[i % 2])
        self.crit(logits.view(-1), self.ys[i % 2]).backward()
        grads = bucket.flat.clone()
        opt.step()
        return {'logits': logits.detach().clone(), 'bucket.flat after backward': grads,
                'bucket.flat_params after step': bucket.flat_params.clone(), 'BatchNorm buffers': _bn_state(model)}

    def loop(self, n, seed=None):
        """n training steps on each twin (a twin's whole loop, then the other's); -> the twin's per-step results"""
        first = self.steps
        self.steps += n
        return self.each(lambda m, b, o: [self.train_step(m, b, o, i) for i in range(first, first + n)], seed)

    def capture(self):
        """the captured, replaying state every test starts from: 4 plain steps, one capture"""
        self.loop(4)
        st = self.g.stats
        assert st['captures'] == 1 and st['replays'] == 2 and st['eager'] == 2 and len(self.g.entries) == 1, st
        return self

    def resync(self):
        """the launch-by-launch twin takes over the graphed model's parameters, optimizer state and buffers"""
        from istvt_amd import ops
        (tm, tb, to), (gm, gb, go) = self.made
        tb.flat_params.copy_(gb.flat_params)
        for name in to._state_names:
            getattr(to, name).copy_(getattr(go, name))
        for (_, v), (_, w) in zip(tm.named_buffers(), gm.named_buffers()):
            v.copy_(w)
        ops.invalidate_weight_cache()


def same(a, b, where=''):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            same(a[k], b[k], '%s %s' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, '%s [%d]' % (where, i))
    else:
        assert torch.equal(a, b), 'the graphed model left the launch-by-launch bits at' + where


@pytest.fixture()
def twins():
    made = []

    def make(**kw):
        made.append(Twins(**kw).capture())
        return made[-1]
    yield make
    for t in made:                              # static-address mode must not outlive the test
        t.g.drop()
        t.made[1][0].enable_step_graphs(False)
    del made[:]
    gc.collect()


def _set_dropout(t, p):
    count = 0
    for m in t.models:
        for d in m.vit.transformer.modules():
            if isinstance(d, nn.Dropout):
                d.p = p
                count += 1
    assert count == 2 * 2 * 4                   # per layer: two attention output dropouts, two in the FeedForward


def test_dropout_seeds_are_not_frozen(twins):
    """An applied nn.Dropout(p > 0) in train mode draws a Philox key on the host at every forward; a replay would use the
    capture's masks for the rest of training.  Such a step is not captured at all: it runs launch by launch, says why, and
    draws from torch's CPU generator exactly what the twin draws (the bit equality under one seed is what checks that)."""
    t = twins()
    g = t.g
    _set_dropout(t, 0.1)
    st0, n_ent = dict(g.stats), len(g.entries)
    t.loop(6, seed=21)
    assert g.stats['captures'] == st0['captures'] and len(g.entries) == n_ent
    assert g.stats['replays'] == st0['replays'] and g.stats['eager'] == st0['eager'] + 6
    assert 'dropout' in g.last_reason

    # the test has power: on one input, with no optimizer step in between, only the masks differ -- and they do
    def two_passes(model, bucket, opt):
        opt.zero_grad()
        logits = []
        for _ in range(2):
            out = model(t.xs[0])
            t.crit(out.view(-1), t.ys[0]).backward()
            logits.append(out.detach().clone())
        grads = bucket.flat.clone()
        opt.step()                              # (consumes and re-zeroes the summed gradient)
        return logits, grads, bucket.flat_params.clone(), _bn_state(model)
    logits = t.each(two_passes, seed=22)[0]
    assert not torch.equal(logits[0], logits[1])
    assert g.stats['eager'] == st0['eager'] + 8 and 'dropout' in g.last_reason and len(g.entries) == n_ent

    # dropout is the identity in eval mode: that forward is still captured and replayed after its warm-up
    def evaluate(model, bucket, opt):
        model.eval()
        with torch.no_grad():
            outs = [model(t.xs[1]).clone() for _ in range(4)]
        model.train()
        return outs
    t.each(evaluate)
    assert len(g.entries) == n_ent + 1 and sum(1 for k in g.entries if not k[-1]) == 1
    assert g.stats['captures'] == st0['captures'] + 1 and g.stats['replays'] == st0['replays'] + 2
    assert g.stats['eager'] == st0['eager'] + 10

    # every p back at 0: the training step is graphed again (its first entry is found again), with the twin's bits
    _set_dropout(t, 0.0)
    st1 = dict(g.stats)
    t.loop(3, seed=23)
    assert g.stats['replays'] == st1['replays'] + 3 and g.stats['eager'] == st1['eager']
    assert g.stats['captures'] == st1['captures'] and len(g.entries) == n_ent + 1


def test_submodule_eval_is_another_launch_sequence(twins):
    """model.xcep.eval() after a capture (fine-tuning from pretrained Xception weights with frozen BatchNorm statistics):
    the stem goes by xcep.training, not model.training.  A replay of the old entry would run the batch-statistics kernels
    and keep moving the running statistics."""
    t = twins()
    g = t.g
    before = [_bn_state(m.xcep) for m in t.models]
    for m in t.models:
        m.xcep.eval()
    st0 = dict(g.stats)
    t.loop(3)
    for m, b in zip(t.models, before):
        assert m.training and torch.equal(_bn_state(m.xcep), b)         # frozen on both twins
    assert g.stats['captures'] == st0['captures'] + 1 and g.stats['eager'] == st0['eager'] + 2 and len(g.entries) == 2
    for m in t.models:
        m.xcep.train()
    st1 = dict(g.stats)
    t.loop(3)
    for m, b in zip(t.models, before):
        assert not torch.equal(_bn_state(m.xcep), b)                    # ... and moving again
    # the first configuration's entry is found again, not captured a second time
    assert g.stats['captures'] == st1['captures'] and g.stats['replays'] == st1['replays'] + 3 and len(g.entries) == 2
    assert g.stats['eager'] == st1['eager']
    # the key covers every module's flag, not only xcep's: one transformer layer's FeedForward (dropout at 0)
    for m in t.models:
        m.vit.transformer.layers[1][2].fn.eval()
    t.loop(3)
    assert g.stats['captures'] == st1['captures'] + 1 and g.stats['eager'] == st1['eager'] + 2 and len(g.entries) == 3
    for m in t.models:
        m.vit.transformer.layers[1][2].fn.train()
    st2 = dict(g.stats)
    t.loop(2)
    assert g.stats['captures'] == st2['captures'] and g.stats['replays'] == st2['replays'] + 2 and len(g.entries) == 3


def test_freezing_and_unfreezing_parameters(twins):
    """requires_grad_(False) after a capture (staged unfreezing): the launch-by-launch path stops adding that gradient into
    the bucket; a replay of the old backward graph would keep writing it and the fused optimizer keep stepping it."""
    t = twins()
    g = t.g

    def frozen(m):
        x = m.xcep.model
        return [m.vit.mlp_head[1].weight, x.conv2.weight,               # a Linear; a dense convolution (slab reduce + add),
                x.block1.rep[0].pointwise.weight,                       # a 1x1 convolution of the fused BN-backward kernel,
                x.block3.rep[1].conv1.weight]                           # a depthwise convolution (side-stream weight gradient)

    def slices(m, bucket):
        out, off = [], 0
        for p in bucket.params:
            if any(p is q for q in frozen(m)):
                out.append((off, off + p.numel()))
            off += p.numel()
        assert len(out) == 4
        return out
    cuts = [slices(m, b) for m, b, _ in t.made]
    assert cuts[0] == cuts[1]
    res = t.loop(1)
    for a, b in cuts[0]:                        # power: these gradients are not zero while the parameters are live
        assert res[0]['bucket.flat after backward'][a:b].any()
    for m in t.models:
        for p in frozen(m):
            p.requires_grad_(False)
    res = t.loop(3)                             # (each() holds the graphed model's gradients to the twin's: zero there too)
    for r in res:
        for a, b in cuts[0]:
            assert not r['bucket.flat after backward'][a:b].any()
    assert g.stats['recaptures'] == 1 and g.stats['captures'] == 2
    for m in t.models:
        for p in frozen(m):
            p.requires_grad_(True)
    res = t.loop(3)
    for r in res:
        for a, b in cuts[0]:
            assert r['bucket.flat after backward'][a:b].any()
    assert g.stats['recaptures'] == 2 and g.stats['captures'] == 3


def test_a_swapped_head_is_seen(twins):
    """a fresh nn.Linear in place of the classifier after a capture: it is not in the bucket, so the step runs launch by
    launch (and says why) instead of replaying the old head's weights; with a new bucket it is captured again, once"""
    t = twins()
    g = t.g
    for m in t.models:
        torch.manual_seed(11)
        m.vit.mlp_head[1] = nn.Linear(728, 1).cuda()
    n_eager, n_cap = g.stats['eager'], g.stats['captures']

    def forward(model, bucket, opt):
        return model(t.xs[0]).detach().clone()
    t.each(forward)
    assert g.stats['eager'] == n_eager + 1 and g.last_reason == 'a live gradient is not a fused-bucket view'
    assert g.stats['captures'] == n_cap and not g.entries
    t.made[:] = [(m,) + t.bucket_for(m) for m in t.models]
    t.resync()
    t.loop(4)
    assert g.stats['recaptures'] == 1 and g.stats['captures'] == n_cap + 1 and len(g.entries) == 1
    assert g.stats['replays'] >= 4                                      # 2 before the swap, 2 of these 4 steps


def test_environment_switches_are_part_of_the_key(twins, monkeypatch):
    """the four switches stem.py and functional.py read from the environment at every call select launch sequences: after a
    change the next steps warm up and capture an entry of their own (never a replay of the old one); back at the old value
    the first entry is found again"""
    t = twins()
    g = t.g
    g.max_entries = 8                           # the first entry and one per switch
    first = next(iter(g.entries))
    for name, value in ENV:
        st0, n_ent = dict(g.stats), len(g.entries)
        monkeypatch.setenv(name, value)
        t.loop(3)
        assert len(g.entries) == n_ent + 1 and g.stats['captures'] == st0['captures'] + 1, name
        assert g.stats['eager'] == st0['eager'] + 2 and g.stats['replays'] == st0['replays'] + 1, name
        calls = g.entries[first].calls
        monkeypatch.delenv(name)
        t.loop(1)
        assert g.entries[first].calls == calls + 1 and g.stats['replays'] == st0['replays'] + 2, name
        assert g.stats['captures'] == st0['captures'] + 1 and g.stats['eager'] == st0['eager'] + 2, name
    assert g.stats['recaptures'] == 0


def test_fp8_flag_of_a_middle_layer(twins):
    """attn_fp8 on the middle layer's SpatialOnlyAttention only (depth 3): neither the first nor the last module that has
    the flag.  The next steps are the twin's bits, from an entry of their own, not a replay of the all-bf16 graph."""
    t = twins(depth=3)
    g = t.g
    for m in t.models:
        mid = m.vit.transformer.layers[1][1].fn
        assert type(mid).__name__ == 'SpatialOnlyAttention' and not mid.attn_fp8
        mid.attn_fp8 = True
    st0 = dict(g.stats)
    t.loop(3)
    assert len(g.entries) == 2 and g.stats['captures'] == st0['captures'] + 1
    assert g.stats['eager'] == st0['eager'] + 2 and g.stats['replays'] == st0['replays'] + 1
    for m in t.models:
        m.vit.transformer.layers[1][1].fn.attn_fp8 = False
    t.loop(1)
    assert g.stats['captures'] == st0['captures'] + 1 and g.stats['replays'] == st0['replays'] + 2
