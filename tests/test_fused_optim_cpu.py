"""Fused optimizers, host side: the segment table of the grouped step kernels and the argument
checks of parameter groups.  No GPU: the table is plain Python and every check fires before the optimizers ask for one."""

import pytest
import torch

SHAPES = [(37, 5), (1001,), (8, 3, 3, 3), (3,), (1,), (4097,)]          # 185, 1001, 216, 3, 1, 4097 elements


@pytest.fixture(scope='module')
def parallel():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import parallel
    return parallel


def _params(shapes=SHAPES):
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def test_new_entry_points_declared_and_exported(parallel):
    from istvt_amd import _lib
    lib = _lib.lib()                                        # (header, table and library: test_abi_cpu.py)
    # the workspace helper: one double per chunk of n, and the chunk is the constant the tests size their cases by
    c = parallel.GRAD_NORM_CHUNK
    assert [lib.istvt_grad_norm_ws_elems(n) for n in (1, c, c + 1, 3 * c + 5)] == [1, 1, 2, 4]


def test_segment_table_merges_runs_of_one_group(parallel):
    ps = _params()
    # interleaved groups: nothing to merge, every parameter is its own segment; the 1-element parameter too
    ends, gids, group_of = parallel.segment_table(ps, [[ps[0], ps[2], ps[4]], [ps[1], ps[3]]])
    assert ends == [185, 1186, 1402, 1405, 1406, 5503]
    assert gids == [0, 1, 0, 1, 0, 2]                       # parameter 5 is named nowhere: the default (last) group
    assert group_of == [0, 1, 0, 1, 0, 2]
    # the order inside a group's list does not matter, neighbours of one group merge into one run
    ends, gids, group_of = parallel.segment_table(ps, [[ps[3], ps[0], ps[1]], [ps[4]]])
    assert (ends, gids) == ([1186, 1402, 1405, 1406, 5503], [0, 2, 0, 1, 2])
    assert group_of == [0, 0, 2, 0, 1, 2]
    # a lone 1-element parameter between two runs of another group keeps a segment of its own
    ends, gids, _ = parallel.segment_table(ps, [[ps[4]], [ps[0], ps[1], ps[2], ps[3], ps[5]]])
    assert (ends, gids) == ([1405, 1406, 5503], [1, 0, 1])
    # no groups: one default group, one segment
    assert parallel.segment_table(ps, []) == ([5503], [0], [0] * 6)
    # every parameter named: no default group appears
    ends, gids, group_of = parallel.segment_table(ps, [ps[:3], ps[3:]])
    assert (ends, gids, group_of) == ([1402, 5503], [0, 1], [0, 0, 0, 1, 1, 1])
    # the table always ends at the bucket's size and is strictly increasing
    assert ends[-1] == sum(p.numel() for p in ps) and all(a < b for a, b in zip(ends, ends[1:]))


def test_segment_table_refuses_bad_groups(parallel):
    ps = _params()
    with pytest.raises(ValueError, match='more than one'):
        parallel.segment_table(ps, [[ps[0], ps[1]], [ps[1]]])                   # a parameter in two groups
    with pytest.raises(ValueError, match='more than one'):
        parallel.segment_table(ps, [[ps[0], ps[0]]])                            # ... or twice in one
    with pytest.raises(ValueError, match='not in the bucket'):
        parallel.segment_table(ps, [[ps[0], torch.nn.Parameter(torch.zeros(3))]])
    many = _params([(2,)] * 10)
    assert len(parallel.segment_table(many[:8], [[q] for q in many[:8]])[0]) == 8   # eight named groups and no rest: fine
    with pytest.raises(ValueError, match='at most 8'):
        parallel.segment_table(many, [[q] for q in many[:9]])                   # nine groups
    with pytest.raises(ValueError, match='at most 8'):
        parallel.segment_table(many, [[q] for q in many[:8]])                   # eight named groups + the default one


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_constructor_refuses_bad_groups_before_it_needs_a_gpu(parallel, kind):
    ps = _params()
    bucket = parallel.GradBucket(ps, flatten_params=True)

    def make(groups, **kw):
        if kind == 'sgd':
            return parallel.FusedSGD(bucket, lr=0.1, momentum=0.9, param_groups=groups, **kw)
        return parallel.FusedAdamW(bucket, lr=0.1, param_groups=groups, **kw)

    differing = {'momentum': 0.5} if kind == 'sgd' else {'betas': (0.8, 0.999)}
    with pytest.raises(ValueError, match='same in every param group'):
        make([dict({'params': [ps[0]]}, **differing)])
    with pytest.raises(ValueError, match='more than one'):
        make([{'params': [ps[0]]}, {'params': [ps[0], ps[1]], 'lr': 0.01}])
    with pytest.raises(ValueError, match='not in the bucket'):
        make([{'params': [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(ValueError, match='at most 8'):
        make([{'params': [q]} for q in ps] + [{'params': []}] * 3)
    with pytest.raises(ValueError, match='max_grad_norm'):
        make(None, max_grad_norm=0.0)
    # valid groups get as far as the missing GPU (a bucket on the host): there is no CPU path
    with pytest.raises(RuntimeError, match='GPU only'):
        make([{'params': [ps[0], ps[2], ps[4]], 'lr': 0.05, 'weight_decay': 0.0}, {'params': [ps[1], ps[3]], 'lr': 0.01}])
