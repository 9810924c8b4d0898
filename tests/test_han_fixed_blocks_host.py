"""CPU: the fixed-capacity block path of mini-batch HAN without a device (allset_amd/han_sampling.py ``FixedBlock``,
``HANSampler.sample_blocks_fixed``, ``GraphedSampledStep``; csrc/han_sample.hip's ``_dc`` walks and fixed-block entries): the driver's
flags, the capacity arithmetic, the refusals that must come before any device work, and that the eager API is unchanged."""
from __future__ import annotations

import inspect
from types import SimpleNamespace

import pytest
import torch


def _host_sampler(k=2):
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HANSampler
    return HANSampler(SimpleNamespace(n=100000, device=torch.device("cpu")), DEFAULT_METAPATHS, k, seed=3)


def test_parser_has_both_flags_and_graph_step_implies_fixed_blocks():
    from allset_amd import han_sampling as hs
    p = hs.build_parser()
    d = p.parse_args([]).__dict__
    assert d["fixed_blocks"] is False and d["graph_step"] is False
    assert hs.setup(dict(d))["fixed_blocks"] is False
    a = hs.setup(p.parse_args(["--fixed_blocks"]).__dict__)
    assert a["fixed_blocks"] is True and a["graph_step"] is False
    b = hs.setup(p.parse_args(["--graph_step"]).__dict__)
    assert b["fixed_blocks"] is True and b["graph_step"] is True


def test_capacity_arithmetic():
    from allset_amd import ops
    from allset_amd.han_sampling import Block, FixedBlock
    assert issubclass(FixedBlock, Block)
    for B, k in ((1, 1), (3, 2), (32, 20), (1024, 20), (1024, 64), (1025, 1)):
        assert FixedBlock.capacity(B, k) == B * (k + 1) == ops.han_fixed_check(B, k)
    assert ops.han_fixed_check(1024, 64) == 66560 <= ops.han_fixed_max_slab()          # the size the path must at least be built for
    z = torch.zeros(1)
    fb = FixedBlock(5, 3, z, z, z, z, z, z, z, z)
    assert (fb.n_dst, fb.n_src, fb.nnz, fb.k) == (5, 20, 20, 3)


def test_refusals_come_before_any_device_work():
    from allset_amd import _lib, ops
    s = _host_sampler(k=64)
    with pytest.raises(ValueError, match="B == 0"):
        s.sample_blocks_fixed([])
    with pytest.raises(ValueError, match="B == 0"):
        s.sample_blocks_fixed(torch.zeros(0, dtype=torch.int64))
    limit = ops.han_fixed_max_slab()
    B = limit // 65 + 1
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        s.sample_blocks_fixed(list(range(B)))
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        ops.han_fixed_check(B, 64)
    with pytest.raises(_lib.AllSetHipError, match="at least one seed"):
        ops.han_fixed_check(0, 4)
    assert s.counter == 0 and s.status is None                                       # nothing was consumed or allocated
    lib = _lib.load()
    err = lambda: lib.allset_last_error().decode()
    assert lib.allset_han_block_relabel(0, 0, 0, 0, 4, 0, 0, 0, 0, 0) == -1 and "at least one seed" in err()
    assert lib.allset_han_block_relabel(0, 0, 0, B, 64, 0, 0, 0, 0, 0) not in (0, -1) and "exceeds the built maximum" in err()
    assert lib.allset_han_block_relabel(0, 0, 0, 3, 4, 0, 0, 0, 0, 0) == -1 and "null" in err()
    assert lib.allset_han_block_compact_fixed(0, 0, 0, 0, 0, 0, 0, 0, 3, 4, 0, 0, 0, 0, 0) == -1 and "null" in err()
    assert lib.allset_han_block_transpose(0, 0, 0, 3, 65, 0, 0, 0, 0) not in (0, -1) and "exceeds the built maximum" in err()
    assert lib.allset_han_block_transpose(0, 0, 0, 3, 4, 0, 0, 0, 0) == -1 and "null" in err()
    assert lib.allset_han_walk_dc(0, 0, 0, 0, 0, 4, 4, 0, 0, 3, 65, 1, 0, 0, 0, 0) != 0 and "exceeds the built maximum" in err()
    assert lib.allset_han_walk_dc(0, 1, 1, 1, 1, 4, 4, 0, 1, 3, 5, 1, 0, 0, 1, 0) == -1 and "null counter" in err()
    assert _lib.ABI_VERSION == 15


@pytest.mark.parametrize("fn", ["han_walk", "han_walk_typed"])
def test_counter_tensors_are_checked_by_name(fn):
    from allset_amd import _lib, ops
    seeds = torch.zeros(2, dtype=torch.int32)
    call = (lambda c, **kw: ops.han_walk(0, None, None, 0, seeds, 2, 0, c, **kw)) if fn == "han_walk" else \
        (lambda c, **kw: ops.han_walk_typed(0, [], seeds, 2, 0, c, **kw))
    with pytest.raises(_lib.AllSetHipError, match=f"{fn}: a counter tensor must live on the device"):
        call(torch.zeros(1, dtype=torch.int64))
    with pytest.raises(_lib.AllSetHipError, match=f"{fn}: a counter tensor is ONE uint64 / int64 element"):
        call(torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.AllSetHipError, match=f"{fn}: a counter tensor is ONE uint64 / int64 element"):
        call(torch.zeros(2, dtype=torch.int64), counter_add=1)
    with pytest.raises(ValueError, match="counter tensor must live on the device"):
        _host_sampler().sample_blocks_fixed([1, 2], counter=torch.zeros(1, dtype=torch.int64))


def test_graphed_step_needs_a_capturable_optimizer():
    from allset_amd import _lib
    from allset_amd.han_sampling import GraphedSampledStep
    lin = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(lin.parameters(), lr=0.01)
    with pytest.raises(_lib.AllSetHipError, match="capturable optimizer"):
        GraphedSampledStep(lin, _host_sampler(), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), torch.nn.CrossEntropyLoss(), opt, 2)


def test_the_eager_api_is_unchanged():
    from allset_amd.han_sampling import Block, HANSampler
    assert list(inspect.signature(HANSampler.sample_blocks).parameters) == ["self", "seeds", "counter"]
    assert inspect.signature(HANSampler.sample_blocks).parameters["counter"].default is None
    assert list(inspect.signature(Block.__init__).parameters) == ["self", "n_dst", "n_src", "src_ids", "src", "dst", "rowptr", "col", "perm",
                                                                 "rowptrT", "colT", "slotT"]
    assert list(inspect.signature(Block.from_edges).parameters) == ["src", "dst", "n_src", "n_dst", "src_ids"]
    assert callable(Block.srcdata_nid) and not hasattr(Block, "sizes") and not hasattr(Block, "exact")
    t = torch.arange(3)
    b = Block(2, 3, t, t, t, t, t, t, t, t, t)
    assert (b.n_dst, b.n_src, b.nnz) == (2, 3, 3) and b.src is t and b.perm is t
    assert sorted(vars(b)) == sorted(["n_dst", "n_src", "nnz", "src_ids", "src", "dst", "rowptr", "col", "perm", "rowptrT", "colT", "slotT"])
