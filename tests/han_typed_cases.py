"""The tiny typed graph of the typed mini-batch HAN tests (tests/test_gpu_han_typed.py, tests/test_han_typed_host.py) and the exact
law of a metapath walk over it, test-only; it shares no code with the package.

Node types: 40 ``p``, 15 ``a``, 6 ``f``, 5 ``b``.  Relations:
  ``pa`` / ``ap``   paper - author in both directions: papers 0..37 have 1..4 authors, papers 38 and 39 have NONE, and the first six
                    incidences are listed twice (a duplicated edge is twice as likely in a multigraph walk);
  ``pf`` / ``fp``   paper - field, one field per paper, four incidences listed twice;
  ``r1`` (a -> b), ``r2`` (b -> a)   NOT each other's reverse; ``b`` node 4 has no out-edge, so a walk that reaches it terminates;
  ``cites`` (p -> p)   source and destination type coincide; papers 30..39 cite nothing;
  ``e0`` (p -> p)   no edges at all.

A walk takes, at every hop, one uniformly random entry of the current node's edge LIST of that relation, and terminates (endpoint
-1) at a node without one.  Its law is therefore the product of the row-normalised edge-COUNT matrices, in float64, with the mass
that meets an empty row moved to -1."""
import numpy as np

N = {"p": 40, "a": 15, "f": 6, "b": 5}
RELS = {"pa": ("p", "a"), "ap": ("a", "p"), "pf": ("p", "f"), "fp": ("f", "p"), "r1": ("a", "b"), "r2": ("b", "a"),
        "cites": ("p", "p"), "e0": ("p", "p")}
ORPHANS = (38, 39)
DEAD_B = 4
METAPATHS = {
    "pap": ["pa", "ap"],
    "papfp": ["pa", "ap", "pf", "fp"],
    "papap": ["pa", "ap", "pa", "ap"],                       # a repeated relation: fails if two hops share a random number
    "cites": ["cites"],
    "hop8": ["pa", "ap", "pf", "fp", "pa", "ap", "pf", "fp"],
    "r1r2": ["r1", "r2"],
}


def edge_lists():
    """``{etype: (src int64[E], dst int64[E])}``, drawn once from a fixed generator."""
    rng = np.random.default_rng(2024)
    ps, as_ = [], []
    for p in range(N["p"] - len(ORPHANS)):
        for a in rng.choice(N["a"], size=int(rng.integers(1, 5)), replace=False):
            ps.append(p), as_.append(int(a))
    ps, as_ = np.array(ps + ps[:6], dtype=np.int64), np.array(as_ + as_[:6], dtype=np.int64)
    pf_p = np.arange(N["p"], dtype=np.int64)
    pf_f = rng.integers(0, N["f"], size=N["p"]).astype(np.int64)
    pf_p, pf_f = np.concatenate([pf_p, pf_p[5:9]]), np.concatenate([pf_f, pf_f[5:9]])
    r1_a = np.repeat(np.arange(N["a"], dtype=np.int64), 2)
    r1_b = np.stack([np.arange(N["a"]) % N["b"], (3 * np.arange(N["a"]) + 1) % N["b"]], 1).reshape(-1).astype(np.int64)
    r2_b = np.array([0, 0, 0, 1, 1, 2, 3, 3, 3, 3], dtype=np.int64)                  # b = 4: no out-edge
    r2_a = np.array([1, 5, 5, 0, 14, 7, 2, 3, 9, 11], dtype=np.int64)
    c_src = np.repeat(np.arange(30, dtype=np.int64), 3)
    c_dst = rng.integers(0, N["p"], size=c_src.size).astype(np.int64)
    none = np.zeros(0, dtype=np.int64)
    return {"pa": (ps, as_), "ap": (as_, ps), "pf": (pf_p, pf_f), "fp": (pf_f, pf_p), "r1": (r1_a, r1_b), "r2": (r2_b, r2_a),
            "cites": (c_src, c_dst), "e0": (none, none)}


def hetero_graph(device):
    """The graph as the package's ``HeteroGraph`` with its id tensors on ``device``."""
    import torch
    from allset_amd.han_hetero import HeteroGraph
    t = lambda a: torch.from_numpy(a).to(device)
    return HeteroGraph({(RELS[e][0], e, RELS[e][1]): (t(s), t(d)) for e, (s, d) in edge_lists().items()}, dict(N))


def counts(etype):
    """float64[n_src, n_dst]: how often each edge is listed."""
    src, dst = edge_lists()[etype]
    m = np.zeros((N[RELS[etype][0]], N[RELS[etype][1]]))
    np.add.at(m, (src, dst), 1.0)
    return m


def endpoint_law(metapath, seed_node):
    """Exact ``{endpoint: probability}`` of one walk from ``seed_node``, -1 (termination) included where its probability is not 0.  A
    seed outside the head type's id range has no out-edge: ``{-1: 1.0}``."""
    n_head = N[RELS[metapath[0]][0]]
    if not 0 <= seed_node < n_head:
        return {-1: 1.0}
    v = np.zeros(n_head)
    v[seed_node] = 1.0
    dead = 0.0
    for etype in metapath:
        m = counts(etype)
        deg = m.sum(1)
        dead += float(v[deg == 0].sum())
        v = (v[deg > 0] / deg[deg > 0]) @ m[deg > 0]
    law = {int(u): float(v[u]) for u in np.nonzero(v)[0]}
    if dead > 0:
        law[-1] = dead
    assert abs(sum(law.values()) - 1.0) < 1e-12
    return law


def check_walks(ends, law, what):
    """``ends`` int[counters, k]: the endpoints of one seed's walks over consecutive step counters, against the exact ``law`` -- every
    endpoint's frequency, the collision rate of two walk lanes and of one lane at two consecutive counters (``sum p^2`` if they are
    independent), each under the binomial 5-sigma bound; the support inside the exact support."""
    n = ends.size
    assert set(np.unique(ends).tolist()) <= set(law), (what, sorted(set(np.unique(ends).tolist()) - set(law)))
    worst = 0.0
    for u, pu in law.items():
        f = float((ends == u).mean())
        bound = 5 * np.sqrt(pu * (1 - pu) / n)
        worst = max(worst, abs(f - pu) / bound) if bound else worst
        assert abs(f - pu) <= bound, (what, u, f, pu, bound)
    q = sum(p * p for p in law.values())
    lanes = ends[:, 0::2] == ends[:, 1::2]
    qb = 5 * np.sqrt(q * (1 - q) / lanes.size) if q < 1 else 0.0
    fq = float(lanes.mean())
    print(f"{what}: {len(law)} endpoints, worst |f - p| / bound {worst:.2f}; lane collisions {fq:.4f} vs {q:.4f} +- {qb:.4f}")
    assert abs(fq - q) <= qb, (what, "lanes", fq, q, qb)
    steps = ends[0::2, :] == ends[1::2, :]
    sb = 5 * np.sqrt(q * (1 - q) / steps.size) if q < 1 else 0.0
    assert abs(float(steps.mean()) - q) <= sb, (what, "counters", float(steps.mean()), q, sb)
