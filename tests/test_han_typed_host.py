"""CPU: typed mini-batch HAN without a device (``han_sampling.TypedMetapathWalker``, ``allset_han_walk_typed``): the parser's
``--hetero``, every metapath the walker refuses (on a CPU ``HeteroGraph``, before any device work), the untouched hypergraph
metapaths, the new entry point's header / binding / export and its argument checks (which return before any launch), and the exact
law of tests/han_typed_cases.py against a sampled walk in numpy."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_typed_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_parser_accepts_hetero_and_its_default_is_off():
    from allset_amd import han_sampling as hs
    assert hs.build_parser().parse_args([]).hetero is False
    a = hs.build_parser().parse_args(["--hetero", "--dataset", "synthetic"])
    assert a.hetero is True and a.dataset == "synthetic"
    with pytest.raises(FileNotFoundError, match="not available to --hetero"):          # han_hetero.load_data's, before any device work
        hs.load_data(hs.setup(hs.build_parser().parse_args(["--hetero", "--dataset", "cora"]).__dict__))


def test_hypergraph_metapaths_are_unchanged():
    from allset_amd import han_sampling as hs
    assert hs.DEFAULT_METAPATHS == [['Vs_E', 'E_Vs'], ['Es_V', 'V_Es']]
    assert hs.METAPATHS == {('Vs_E', 'E_Vs'): 0, ('Es_V', 'V_Es'): 1}
    assert [hs.metapath_index(m) for m in (['Vs_E', 'E_Vs'], ('Es_V', 'V_Es'), 'VEV', 'EVE', 0, 1)] == [0, 1, 0, 1, 0, 1]
    with pytest.raises(ValueError, match="unknown metapath"):
        hs.metapath_index(['pa', 'ap'])


def test_walker_resolves_metapaths_and_refuses_the_rest_on_the_host():
    from allset_amd import han_sampling as hs, ops
    g = tc.hetero_graph(CPU)
    w = hs.TypedMetapathWalker(g)
    assert w.device == CPU and w.ntype is None and w.n is None
    assert w.resolve(["pa", "ap"]) == [("p", "pa", "a"), ("a", "ap", "p")]
    assert w.resolve([("p", "pf", "f"), "fp"]) == [("p", "pf", "f"), ("f", "fp", "p")]       # names or canonical triples
    assert len(w.resolve(tc.METAPATHS["hop8"])) == ops.HAN_MAX_HOPS == 8 and w.resolve(["cites"]) == [("p", "cites", "p")]
    with pytest.raises(ValueError, match="unknown edge type"):
        w.resolve(["pa", "xx"])
    with pytest.raises(ValueError, match="unknown relation"):
        w.resolve([("p", "pa", "f"), "fp"])
    with pytest.raises(ValueError, match="starts from"):
        w.resolve(["pa", "fp"])                                                              # 'a' does not meet 'f'
    with pytest.raises(ValueError, match="non-empty"):
        w.resolve([])
    with pytest.raises(ValueError, match="non-empty"):
        w.resolve("pa")
    with pytest.raises(ValueError, match="HAN_MAX_HOPS = 8"):
        w.resolve(tc.METAPATHS["hop8"] + ["cites"])
    with pytest.raises(ValueError, match="must end on the type it starts from"):
        w.resolve(["pa"])
    with pytest.raises(ValueError, match="must end on the type it starts from"):
        w.resolve(["pa", "ap", "pf"])
    assert w.ntype is None                                                                   # resolving binds nothing
    with pytest.raises(TypeError):
        hs.TypedMetapathWalker(object())


def test_sampler_over_a_typed_walker_is_validated_on_the_host():
    from allset_amd import han_sampling as hs
    g = tc.hetero_graph(CPU)
    w = hs.TypedMetapathWalker(g)
    with pytest.raises(ValueError, match="start from 2 node types"):
        hs.HANSampler(w, [["pa", "ap"], ["ap", "pa"]], 4)
    assert w.ntype is None
    with pytest.raises(ValueError, match="num_neighbors"):
        hs.HANSampler(w, [["pa", "ap"]], 65)
    s = hs.HANSampler(w, [["pa", "ap"], ["pf", "fp"], ["cites"]], 5, seed=3)
    assert s.metapaths == [0, 1, 2] and (w.ntype, w.n) == ("p", tc.N["p"])                   # the index is the position in the list
    assert s.chains[1] == [("p", "pf", "f"), ("f", "fp", "p")]
    with pytest.raises(ValueError, match="of their own"):
        hs.HANSampler(w, [["ap", "pa"]], 4)                                                  # this walker samples papers
    with pytest.raises(ValueError, match="of their own"):
        hs.random_walk_endpoints(w, ["r1", "r2"], [0], 4, 0, 0)
    with pytest.raises(ValueError, match="duplicate seeds"):
        s.sample_blocks([1, 2, 1])
    with pytest.raises(ValueError, match="outside"):
        s.sample_blocks([1, tc.N["p"]])                                                      # seeds are ids of the head type
    with pytest.raises(ValueError, match="integer"):
        s.sample_blocks([0.5, 1.0])
    with pytest.raises(ValueError, match="num_walks"):
        hs.random_walk_endpoints(w, ["pa", "ap"], [0], 65, 0, 0)
    with pytest.raises(ValueError, match="index"):
        hs.random_walk_endpoints(w, ["pa", "ap"], [0], 4, 0, 0, index=256)
    assert s.counter == 0                                                                    # a refused call takes no step counter
    wa = hs.TypedMetapathWalker(g)
    hs.HANSampler(wa, [["ap", "pa"], ["r1", "r2"]], 4)
    assert (wa.ntype, wa.n) == ("a", tc.N["a"])


def test_header_binding_and_export_agree_for_the_typed_walk():
    from allset_amd import _lib, ops
    sym = "allset_han_walk_typed"
    header = open(os.path.join(ROOT, "include", "allset_hip_ext.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", code)
    assert m, f"{sym} not declared"
    assert sym in _lib.EXPORTED_SYMBOLS and len(_lib.SIGNATURES[sym]) == m.group(1).count(",") + 1
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + sym + r"\b", out), f"{sym} not exported"
    assert _lib.ABI_VERSION == 15 and _lib.load().allset_version() == 15                     # an addition: no bump
    assert ops.HAN_MAX_HOPS == 8 and callable(ops.han_walk_typed)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every call here fails its argument checks or has nothing to do: nothing is launched, no device is needed."""
    import ctypes
    from allset_amd import _lib
    lib = _lib.load()
    err = lambda: lib.allset_last_error().decode()
    tab = (ctypes.c_void_p * 9)()                                                            # nine null pointers
    rows = (ctypes.c_int64 * 9)(*([4] * 9))
    call = lambda mp, L, rp, col, n, seeds, B, k, out: lib.allset_han_walk_typed(mp, L, rp, col, n, seeds, B, k, 1, 0, out, 0)
    assert call(0, 9, tab, tab, rows, 0, 3, 5, 0) == -1 and "HAN_MAX_HOPS" in err() and "got 9" in err()
    assert call(0, 0, tab, tab, rows, 0, 3, 5, 0) == -1 and "HAN_MAX_HOPS" in err()
    assert call(0, 2, tab, tab, rows, 0, 3, 65, 0) not in (0, -1) and "exceeds the built maximum" in err()
    assert call(0, 2, tab, tab, rows, 0, 3, 0, 0) == -1 and "k >= 1" in err()
    assert call(-1, 2, tab, tab, rows, 0, 3, 5, 0) == -1 and "metapath" in err()
    assert call(0, 2, 0, tab, rows, 0, 3, 5, 0) == -1 and "null relation table" in err()
    assert call(0, 2, tab, tab, rows, 0, 3, 5, 0) == -1 and "null seeds" in err()
    big = (ctypes.c_int64 * 2)(4, 2 ** 31 - 1)
    assert call(0, 2, tab, tab, big, 0, 3, 5, 0) == -1 and "fit int32" in err()
    neg = (ctypes.c_int64 * 2)(4, -1)
    assert call(0, 2, tab, tab, neg, 0, 3, 5, 0) == -1 and "fit int32" in err()
    assert call(0, 2, tab, tab, rows, 0, 2 ** 31, 5, 0) == -1 and "exceeds int32" in err()
    one = (ctypes.c_int32 * 1)()
    assert call(0, 2, tab, tab, rows, one, 3, 5, one) == -1 and "null rowptr" in err()       # (host arrays: checked, never read)
    assert call(0, 2, tab, tab, rows, 0, 0, 5, 0) == 0 and err() == ""                       # B == 0: nothing to do


def test_exact_law_agrees_with_a_sampled_multigraph_walk():
    """The law the GPU tests compare against, against a plain numpy walk over the edge LISTS (a fixed numpy seed: deterministic)."""
    edges = tc.edge_lists()
    rng = np.random.default_rng(1)
    out = {e: [dst[src == u] for u in range(tc.N[tc.RELS[e][0]])] for e, (src, dst) in edges.items()}
    for name, s in (("pap", 0), ("papap", 5), ("hop8", 1), ("r1r2", 4), ("cites", 31), ("pap", 38)):
        law = tc.endpoint_law(tc.METAPATHS[name], s)
        n = 20000
        ends = np.empty(n, dtype=np.int64)
        for i in range(n):
            cur = s
            for e in tc.METAPATHS[name]:
                nb = out[e][cur]
                cur = int(nb[rng.integers(nb.size)]) if nb.size else -1
                if cur < 0:
                    break
            ends[i] = cur
        assert set(ends.tolist()) <= set(law)
        for u, pu in law.items():
            assert abs((ends == u).mean() - pu) <= 5 * np.sqrt(pu * (1 - pu) / n), (name, s, u)
    assert tc.endpoint_law(tc.METAPATHS["pap"], 38) == {-1: 1.0} and tc.endpoint_law(tc.METAPATHS["pap"], 40) == {-1: 1.0}
    assert tc.endpoint_law(["e0"], 3) == {-1: 1.0}
    # duplicated edges count: paper 0's first incidence is listed twice
    pa = tc.counts("pa")
    assert pa.max() == 2.0 and pa[list(tc.ORPHANS)].sum() == 0 and tc.counts("r2")[tc.DEAD_B].sum() == 0
