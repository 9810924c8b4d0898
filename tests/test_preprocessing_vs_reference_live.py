"""CPU: allset_amd.preprocessing against the reference functions (reference preprocessing.py:394-469, 22-144) on randomised
block edge lists -- sizes, duplicate-free incidences, size-1 hyperedges, vertices without hyperedges.  Index work: bit-exact,
compared as lexicographically sorted edge lists (the reference's own sorts are unstable).  The reference's results are the ones
oracle/gen_live_fixtures.py recorded in tests/golden/live_preprocessing.npz (the edge lists are rebuilt from their seeds); where the
reference itself is importable (oracle/ref_shim.py) every configuration is run through it LIVE as well."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import util
from oracle import gen_live_fixtures as live
from oracle import ref_shim

canon = live.canon


def test_preprocessing_equals_live_reference():
    from allset_amd import preprocessing as P
    configs = live.preproc_configs()
    with np.load(os.path.join(util.GOLDEN, "live_preprocessing.npz"), allow_pickle=False) as z:
        rec = {k: z[k] for k in z.files}
    assert len(configs) == live.N_PREPROC and f"c{len(configs) - 1}/sl" in rec
    for i, c in enumerate(configs):
        refs = [("recorded", {k.split("/", 1)[1]: v for k, v in rec.items() if k.startswith(f"c{i}/")})]
        if ref_shim.available():
            refs.append(("live", live.reference_preprocessing(c)))
        block, n_v, n_e = live.preproc_block(c), c["n_v"], c["n_e"]

        def fresh():
            return SimpleNamespace(edge_index=torch.from_numpy(block).clone(), n_x=[n_v], num_hyperedges=[n_e])
        p = P.ExtractV2E(fresh())
        got = {"v2e": canon(p.edge_index)}
        p = P.Add_Self_Loops(p)
        got.update(sl=canon(p.edge_index), totedges=int(p.totedges))
        for label, r in refs:
            what = f"{label} c{i} {c}"
            np.testing.assert_array_equal(got["v2e"], r["v2e"], err_msg=what)
            np.testing.assert_array_equal(got["sl"], r["sl"], err_msg=what)
            assert got["totedges"] == int(r["totedges"]), what
            sl = r["sl"]
            for opt in ("all_one", "deg_half_sym"):
                pn = P.norm_contruction(SimpleNamespace(edge_index=torch.from_numpy(sl).clone()), option=opt)
                rn = r["norm_" + opt]
                assert pn.norm.numpy().dtype == rn.dtype, (what, opt)
                np.testing.assert_allclose(pn.norm.numpy(), rn, rtol=1e-6, atol=1e-7, err_msg=what)
            for th in (0, 3):
                de = SimpleNamespace(edge_index=torch.from_numpy(sl).clone(), n_x=torch.tensor([n_v]), num_hyperedges=[n_e],
                                     totedges=int(r["totedges"]))
                np.testing.assert_array_equal(canon(P.expand_edge_index(de, edge_th=th).edge_index), r[f"expand_{th}"], err_msg=what)
