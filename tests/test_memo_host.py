"""CPU: ``allset_amd._memo`` -- derived data kept on the tensor it derives from -- and the structure caches that sit on it
(``cached_incidence``, ``Incidence.weights``, ``SetGNN``'s incidence pair, ``dense.sparse_rows``).  Their kernels:
tests/test_gpu_parity.py, tests/test_gpu_ops.py, tests/test_gpu_input_linear.py."""
import copy
import gc
import pickle
import weakref

import pytest
import torch

from allset_amd import _memo
from allset_amd.incidence import Incidence
from allset_amd.ops import CSR


class _Value:
    """(weakref-able, unlike a tuple)"""


def _counted():
    calls = []

    def build():
        calls.append(1)
        return _Value()
    return calls, build


def test_the_same_object_hits_and_the_builder_runs_once():
    t = torch.arange(6.0)
    calls, build = _counted()
    a = _memo.get(t, "slot", (3,), build)
    assert _memo.get(t, "slot", (3,), build) is a and len(calls) == 1
    assert _memo.get(t, "slot", (4,), build) is not a and len(calls) == 2          # another key: its own entry ...
    assert _memo.get(t, "other", (3,), build) is not a and len(calls) == 3         # ... another slot too
    assert _memo.get(t, "slot", (3,), build) is a and len(calls) == 3
    assert _memo.get(t, "none", (), lambda: None) is None                          # None is a value, not a miss
    assert _memo.lookup(t, "none") is None and _memo.lookup(t, "never") is _memo.MISS


def test_an_in_place_update_rebuilds():
    t = torch.arange(6.0)
    calls, build = _counted()
    a = _memo.get(t, "slot", (), build)
    b = _memo.get(t, "slot", (1,), build)
    t.add_(1)
    assert _memo.lookup(t, "slot") is _memo.MISS
    c = _memo.get(t, "slot", (), build)
    assert c is not a and len(calls) == 3 and _memo.get(t, "slot", (), build) is c
    assert b not in [e[1] for e in t.__dict__["_allset_memo"].values()]             # what the update invalidated went with the rebuild


def test_the_address_is_a_guard():
    """``t.data = other`` moves the tensor to another storage without touching its version counter."""
    t, other = torch.arange(6.0), torch.arange(6.0) + 1
    calls, build = _counted()
    a = _memo.get(t, "slot", (), build)
    v = t._version
    t.data = other
    assert t._version == v and t.data_ptr() == other.data_ptr()
    assert _memo.get(t, "slot", (), build) is not a and len(calls) == 2
    t.data = torch.arange(8.0)                                                      # ... and so are shape and dtype
    assert _memo.lookup(t, "slot") is _memo.MISS
    t2 = torch.arange(6.0)
    _memo.get(t2, "slot", (), build)
    t2.data = t2.data.to(torch.float64)
    assert _memo.lookup(t2, "slot") is _memo.MISS


def test_a_write_through_data_into_the_same_storage_is_not_seen():
    """DOCUMENTED LIMIT: ``t.data.uniform_()`` (the reference's ``glorot``; a raw-pointer optimizer kernel does the same) changes the
    values with the version counter, the address, the shape and the dtype all as they were -- no stamp can detect it, and the stale
    value is served.  This is why data derived from WEIGHTS (the plane images of ``dense.prefetch_wide_planes``) may not use this
    helper and belongs to the step that built it."""
    t = torch.arange(6.0)
    calls, build = _counted()
    a = _memo.get(t, "slot", (), build)
    t.data.uniform_()
    assert _memo.get(t, "slot", (), build) is a and len(calls) == 1


def test_only_the_very_same_object_is_served():
    t = torch.arange(6.0)
    calls, build = _counted()
    _memo.get(t, "slot", (), build)
    assert _memo.lookup(copy.deepcopy(t), "slot") is _memo.MISS
    assert _memo.lookup(copy.copy(t), "slot") is _memo.MISS
    assert _memo.lookup(pickle.loads(pickle.dumps(t)), "slot") is _memo.MISS        # (and a memo does not keep a tensor from pickling)
    assert _memo.lookup(t.detach(), "slot") is _memo.MISS and _memo.lookup(t.view(6), "slot") is _memo.MISS
    lin = torch.nn.Linear(4, 3)
    w = lin.weight
    _memo.get(w, "slot", (), build)
    assert _memo.lookup(w, "slot") is not _memo.MISS
    assert _memo.lookup(lin.to(torch.float64).weight, "slot") is _memo.MISS         # the same attributes, another dtype and storage
    assert _memo.lookup(copy.deepcopy(lin).weight, "slot") is _memo.MISS
    p = torch.nn.Parameter(torch.arange(6.0))
    _memo.get(p, "slot", (), build)
    rewrapped = torch.nn.Parameter(p.data)                                          # same storage, same version, another object
    rewrapped.__dict__.update(p.__dict__)                                           # (even when the attributes travel along)
    assert rewrapped.data_ptr() == p.data_ptr() and _memo.lookup(rewrapped, "slot") is _memo.MISS
    assert _memo.lookup(p, "slot") is not _memo.MISS


def test_the_stamp_is_taken_after_the_builder_ran():
    """``SetGNN`` re-bases ``edge_index[1]`` in place while it builds the incidences."""
    t = torch.arange(6.0)
    calls = []

    def build():
        calls.append(1)
        t.sub_(1)
        return _Value()
    a = _memo.get(t, "slot", (), build)
    assert _memo.get(t, "slot", (), build) is a and len(calls) == 1 and float(t[0]) == -1.0


def test_lookup_never_builds():
    t = torch.arange(6.0)
    assert _memo.lookup(t, "slot") is _memo.MISS and _memo.lookup(t, "slot", (), None) is None
    assert "_allset_memo" not in t.__dict__
    calls, build = _counted()
    a = _memo.get(t, "slot", (), build)
    assert _memo.lookup(t, "slot") is a and len(calls) == 1


def test_a_value_dies_with_its_owner():
    """No module-level table holds it (the package used to keep up to 16 incidences alive after their edge lists had died)."""
    t = torch.arange(6.0)
    w = weakref.ref(_memo.get(t, "slot", (), _counted()[1]))
    assert w() is not None
    del t
    gc.collect()
    assert w() is None


# ---- the structure caches on it ------------------------------------------------------------------------------------------------------

def _cpu_incidence(edge_index, n_src=None, n_dst=None):
    """``Incidence.from_edge_index`` in torch (the library's needs a device)."""
    src, dst = edge_index[0], edge_index[1]
    n_src, n_dst = int(src.max()) + 1 if n_src is None else n_src, int(dst.max()) + 1 if n_dst is None else n_dst

    def csr(rows, cols, n_rows, n_cols):
        perm = torch.argsort(rows, stable=True)
        rowptr = torch.zeros(n_rows + 1, dtype=torch.int32)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
        return CSR(rowptr, cols[perm].to(torch.int32), perm.to(torch.int32), n_rows, n_cols)
    return Incidence(csr(dst, src, n_dst, n_src), csr(src, dst, n_src, n_dst), n_src, n_dst, int(src.max()) + 1, int(dst.max()) + 1)


def _edge_list():
    g = torch.Generator().manual_seed(2)
    return torch.stack([torch.randint(0, 30, (200,), generator=g), torch.randint(0, 12, (200,), generator=g)])


def test_cached_incidence_lives_on_the_edge_list(monkeypatch):
    from allset_amd import incidence
    built = []
    monkeypatch.setattr(Incidence, "from_edge_index", staticmethod(lambda ei, n_src=None, n_dst=None: built.append(1) or _cpu_incidence(ei, n_src, n_dst)))
    ei = _edge_list()
    a = incidence.cached_incidence(ei, 30)
    assert incidence.cached_incidence(ei, 30) is a and len(built) == 1
    assert incidence.cached_incidence(ei, 30, 16) is not a and incidence.cached_incidence(ei, 30) is a and len(built) == 2
    assert incidence.cached_incidence(ei.clone(), 30) is not a                      # equal contents, another tensor
    ei[1, 0] = 11
    assert incidence.cached_incidence(ei, 30) is not a and len(built) == 4
    w = weakref.ref(a)
    del a, ei
    gc.collect()
    assert w() is None


def test_a_fixed_float_norm_is_routed_once(monkeypatch):
    """Non-differentiable float norm (deg_half_sym, preprocessing.py:456-463) over three aggregations: one routing gather; a float norm
    is probed for all ones on its second sight, an integer norm on its first; a norm that requires grad is refused."""
    ei = _edge_list()
    inc = _cpu_incidence(ei)
    routed = []
    real = Incidence._route
    monkeypatch.setattr(Incidence, "_route", lambda self, f: routed.append(1) or real(self, f))
    norm = torch.rand(200) + 0.1
    first = inc.weights(norm)
    for _ in range(2):
        again = inc.weights(norm)
        assert again[0] is first[0] and again[1] is first[1]
    assert len(routed) == 1 and not inc.known_unweighted(norm)
    assert torch.equal(first[0], norm[inc.by_dst.perm.long()]) and torch.equal(first[1], norm[inc.by_src.perm.long()])
    norm.mul_(2.0)                                                                  # in place: routed again
    assert torch.equal(inc.weights(norm)[0], norm[inc.by_dst.perm.long()]) and len(routed) == 2
    other = norm.clone()                                                            # equal contents, another tensor: its own routing
    assert inc.weights(other)[0] is not inc.weights(norm)[0] and len(routed) == 4   # (one entry: each call replaced the other's)
    ones = torch.ones(200)
    assert not inc.known_unweighted(ones)                                           # a read alone: no sighting, no probe
    assert inc.weights(ones)[0] is not None and not inc.known_unweighted(ones)      # first sight: routed unprobed
    assert inc.weights(ones) == (None, None) and inc.known_unweighted(ones)         # second sight: probed
    assert inc.known_unweighted(torch.ones(200, dtype=torch.int64))                 # integer ones: probed on first sight
    assert not inc.known_unweighted(ones)                                           # (which replaced the float norm's entry)
    with pytest.raises(RuntimeError):
        inc.weights(torch.ones(200, requires_grad=True))


def test_setgnn_rebases_once_and_keeps_the_pair_on_the_edge_list():
    import cases
    from allset_amd import SetGNN
    g = torch.Generator().manual_seed(1)
    n_v = 20
    pairs = sorted({(int(torch.randint(0, n_v, (1,), generator=g)), int(torch.randint(0, 8, (1,), generator=g)) + n_v) for _ in range(60)})
    ei = torch.tensor(pairs, dtype=torch.int64).t().contiguous()
    model, twin = SetGNN(cases.make_args("pma_h1", 24, 64, 5)), SetGNN(cases.make_args("pma_h1", 24, 64, 5))
    assert int(ei[1].min()) == n_v
    pair = model._loo_incidences(ei, n_v, "all_one")
    v = ei._version
    assert int(ei[1].min()) == 0 and v > 0                                          # re-based in place, once ...
    assert model._loo_incidences(ei, n_v, "all_one") is pair and ei._version == v    # ... and the entry made then is valid now
    assert twin._loo_incidences(ei, n_v, "all_one") is pair                         # a pure function of the tensor: shared
    sym = model._loo_incidences(ei, n_v, "deg_half_sym")
    assert sym is not pair and sym[0].normtype == "deg_half_sym" and model._loo_incidences(ei, n_v, "all_one") is pair
    assert pair[0].loo is pair[1].loo
    w = weakref.ref(pair[0].loo)
    del pair, sym, ei
    gc.collect()
    assert w() is None                                                              # no model holds it once the data is gone


def test_sparse_rows_lives_on_the_features():
    from allset_amd import dense
    x = (torch.rand(40, 300, generator=torch.Generator().manual_seed(0)) < 0.02).float()
    assert dense.sparse_rows(x, build=False) is None and "_allset_memo" not in x.__dict__
    a = dense.sparse_rows(x)
    assert a is not None and dense.sparse_rows(x) is a and dense.sparse_rows(x, build=False) is a
    assert a.nnz == int((x != 0).sum())
    assert dense.sparse_rows(x.clone()) is not a
    x[0, 0] = 5.0
    assert dense.sparse_rows(x, build=False) is None and dense.sparse_rows(x) is not a
    assert dense.sparse_rows(torch.rand(10, 300)) is None                           # dense features
    w = weakref.ref(a)
    del a, x
    gc.collect()
    assert w() is None
