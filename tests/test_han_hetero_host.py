"""CPU: the host side of the heterogeneous HAN (allset_amd/han_hetero.py) -- HeteroGraph's and the metapath's validation errors (they
are raised before anything touches a device), the driver's ``--hetero`` flag, the ABI declarations of the boolean sparse product and the
seeded ACM-shaped generator of allset_amd/synthetic.py."""
import numpy as np
import pytest
import torch

PA = ("paper", "pa", "author")
AP = ("author", "ap", "paper")
PF = ("paper", "pf", "field")
FP = ("field", "fp", "paper")
t = lambda *v: torch.tensor(v, dtype=torch.int64)


def small_graph():
    from allset_amd.han_hetero import HeteroGraph
    return HeteroGraph({PA: (t(0, 1, 2), t(0, 0, 3)), AP: (t(0, 0, 3), t(0, 1, 2)), PF: (t(0, 1, 2), t(1, 1, 0)), FP: (t(1, 1, 0), t(0, 1, 2))})


def test_hetero_graph_sizes_and_names():
    from allset_amd.han_hetero import HeteroGraph
    g = small_graph()
    assert (g.number_of_nodes("paper"), g.number_of_nodes("author"), g.number_of_nodes("field")) == (3, 4, 2)      # max id + 1, as DGL
    assert g.to_canonical_etype("pa") == PA and g.to_canonical_etype(FP) == FP
    assert g.ntypes == ["author", "field", "paper"] and g.canonical_etypes == [PA, AP, PF, FP]
    g = HeteroGraph({PA: (t(0), t(0))}, num_nodes={"paper": 5, "author": 7, "venue": 2})
    assert (g.number_of_nodes("paper"), g.number_of_nodes("author"), g.number_of_nodes("venue")) == (5, 7, 2)
    with pytest.raises(ValueError, match="unknown node type"):
        g.number_of_nodes("field")


@pytest.mark.parametrize("edges,num_nodes,match", [
    ({}, None, "non-empty dict"),
    ({("paper", "pa"): (t(0), t(0))}, None, "triple"),
    ({PA: (t(0, 1), t(0))}, None, "2 source ids but 1 target"),
    ({PA: (torch.tensor([0], dtype=torch.int32), t(0))}, None, "int64"),
    ({PA: (t(0, -1), t(0, 0))}, None, "negative 'paper' id -1"),
    ({PA: (t(0, 4), t(0, 0))}, {"paper": 4, "author": 1}, r"num_nodes\['paper'\] = 4 but ids of that type reach 4"),
    ({PA: (t(0), t(0)), ("author", "pa", "paper"): (t(0), t(0))}, None, "names two relations"),
    ({PA: t(0)}, None, "pair"),
])
def test_hetero_graph_validation_errors(edges, num_nodes, match):
    from allset_amd.han_hetero import HeteroGraph
    with pytest.raises(ValueError, match=match):
        HeteroGraph(edges, num_nodes)


def test_metapath_validation_errors_come_before_any_device_work():
    from allset_amd.han_hetero import HANLayer, metapath_reachable_graph
    g = small_graph()                                                                     # CPU tensors: nothing may reach a kernel
    with pytest.raises(ValueError, match="unknown edge type 'pp'"):
        metapath_reachable_graph(g, ["pa", "pp"])
    with pytest.raises(ValueError, match=r"step 0 \('pa'\) ends on 'author' but step 1 \('pf'\) starts from 'paper'"):
        metapath_reachable_graph(g, ["pa", "pf"])
    with pytest.raises(ValueError, match="non-empty list"):
        metapath_reachable_graph(g, [])
    with pytest.raises(ValueError, match="unknown relation"):
        metapath_reachable_graph(g, [("paper", "pa", "field")])
    layer = HANLayer([["pa", "zz"]], 4, 2, 1, 0.0)
    with pytest.raises(ValueError, match="unknown edge type 'zz'"):
        layer(g, torch.zeros(3, 4))


def test_cpu_tensors_are_refused_without_fallback():
    from allset_amd import _lib
    from allset_amd.han_hetero import metapath_reachable_graph
    with pytest.raises(_lib.AllSetHipError, match="no CPU fallback"):
        metapath_reachable_graph(small_graph(), ["pa", "ap"])


def test_gatconv_flags():
    import torch.nn.functional as F
    from allset_amd import han, han_hetero
    conv = han_hetero.GATConv(4, 2, 3, 0.1, 0.2, activation=F.elu, allow_zero_in_degree=True)
    assert conv._allow_zero_in_degree and list(conv.state_dict()) == ["attn_l", "attn_r", "bias", "fc.weight"]
    with pytest.raises(ValueError, match="allow_zero_in_degree"):
        han.GATConv(4, 2, 3, activation=F.elu, allow_zero_in_degree=True)                 # (the hypergraph-mode conv keeps refusing it)
    with pytest.raises(ValueError, match="F.elu"):
        han_hetero.GATConv(4, 2, 3, allow_zero_in_degree=True)


def test_parser_accepts_hetero_and_absent_dataset_is_a_clear_error():
    from allset_amd import han, han_hetero
    a = han.build_parser().parse_args(["--hetero", "--dataset", "synthetic", "--runs", "1"]).__dict__
    assert a["hetero"] is True and han.build_parser().parse_args([]).hetero is False
    assert han_hetero.META_PATHS == [["pa", "ap"], ["pf", "fp"]]
    with pytest.raises(FileNotFoundError, match="not available"):
        han.load_data(dict(hetero=True, dataset="ACMRaw", seed=1, device="cpu"))


def test_abi_declares_the_entry_points():
    from allset_amd import _lib
    from allset_amd.build import SOURCES
    assert "metapath.hip" in SOURCES and _lib.ABI_VERSION == 15
    for sym, n_args in (("allset_spgemm_bool_bins", 1), ("allset_spgemm_bool_workspace_bytes", 2), ("allset_spgemm_bool_count", 11),
                        ("allset_spgemm_bool_fill", 13)):
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym]) == n_args, sym
    lib = _lib.load()
    from ctypes import byref, c_size_t
    need = c_size_t(0)
    assert lib.allset_spgemm_bool_workspace_bytes(1000, byref(need)) == 0 and need.value == 16 + 12 * 1000      # O(n_a)


def test_int32_limits_are_errors_with_a_message_before_any_launch():
    from allset_amd import _lib
    lib = _lib.load()
    # n_c beyond int32 (count) and nnz_c beyond int32 (fill): refused on the arguments alone, no pointer is read
    assert lib.allset_spgemm_bool_count(0, 0, 0, 0, 4, 4, 2 ** 31, 0, 0, 0, 0) != 0
    assert "n_c = 2147483648 columns exceed int32" in lib.allset_last_error().decode()
    assert lib.allset_spgemm_bool_fill(0, 0, 0, 0, 4, 4, 4, 0, 2 ** 31, 0, 0, 0, 0) != 0
    assert "2147483648 entries" in lib.allset_last_error().decode()


def test_generator_is_deterministic_and_has_authorless_papers_and_hub_fields():
    from allset_amd.han_hetero import HeteroGraph
    from allset_amd.synthetic import acm_like_hetero
    a = acm_like_hetero(n_papers=600, n_authors=500, n_fields=12, seed=3, device="cpu")
    b = acm_like_hetero(n_papers=600, n_authors=500, n_fields=12, seed=3, device="cpu")
    c = acm_like_hetero(n_papers=600, n_authors=500, n_fields=12, seed=4, device="cpu")
    assert sorted(a.edges) == sorted([PA, AP, PF, FP])
    for rel in a.edges:
        assert torch.equal(a.edges[rel][0], b.edges[rel][0]) and torch.equal(a.edges[rel][1], b.edges[rel][1])
    assert torch.equal(a.features, b.features) and torch.equal(a.labels, b.labels)
    assert not torch.equal(a.labels, c.labels)
    g = HeteroGraph(a.edges, a.num_nodes)
    assert g.number_of_nodes("paper") == 600 and g.number_of_nodes("author") == 500 and g.number_of_nodes("field") == 12
    p, au = a.edges[PA]
    n_auth = torch.bincount(p, minlength=600)
    assert a.orphans == int((n_auth == 0).sum()) and 10 <= a.orphans <= 60                # ~5 % of the papers have no author
    assert int(n_auth.max()) <= 5 and torch.unique(p * 500 + au).numel() == p.numel()
    assert torch.equal(a.edges[AP][0], au) and torch.equal(a.edges[AP][1], p)             # ap is pa reversed
    pf_p, pf_f = a.edges[PF]
    assert torch.equal(pf_p, torch.arange(600)) and torch.equal(a.edges[FP][0], pf_f)     # one field per paper
    sizes = torch.bincount(pf_f, minlength=12).double()
    assert float(sizes.max()) > 4 * float(sizes.median())                                 # strongly skewed: hub rows in PFP
    x = a.features
    assert x.dtype == torch.float32 and set(x.unique().tolist()) == {0.0, 1.0}            # binary bag of words
    words = x.shape[1] // a.num_classes
    for cls in range(a.num_classes):                                                      # correlated with the class
        own = x[a.labels == cls][:, cls * words:(cls + 1) * words].mean()
        other = x[a.labels != cls][:, cls * words:(cls + 1) * words].mean()
        assert float(own) > float(other) + 0.15
    assert a.labels.shape == (600,) and int(a.labels.max()) == a.num_classes - 1
