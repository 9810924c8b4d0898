"""Seeded synthetic hypergraphs of stated |V| / |E| / degree, generated on the device
(BASELINE.json configs[2..4]).

Conventions follow what the reference's loaders + preprocessing hand to ``SetGNN``: members of a
hyperedge are distinct (the loaders ``coalesce`` duplicates away, load_other_datasets.py:178-181),
incidences are emitted sorted by vertex id (preprocessing.py:398,446-447), ``norm`` is all-ones int64
(preprocessing.py:454).  Hyperedge ids start at ``e_base`` (0 by default; ``n_v`` reproduces the layout
train.py passes, which ``SetGNN.forward`` re-bases).
"""
from __future__ import annotations

from types import SimpleNamespace


import torch


def _distinct_members(n_rows: int, k: int, n_v: int, gen: torch.Generator, device) -> torch.Tensor:
    """[n_rows, k] vertex ids, uniform, distinct within each row (rejection on the rare duplicate rows)."""
    members = torch.randint(n_v, (n_rows, k), generator=gen, device=device, dtype=torch.int64)
    if k > n_v:
        raise ValueError("hyperedge size exceeds the number of vertices")
    for _ in range(64):
        s, _ = members.sort(dim=1)
        dup = (s[:, 1:] == s[:, :-1]).any(dim=1)
        n_dup = int(dup.sum())
        if n_dup == 0:
            break
        members[dup] = torch.randint(n_v, (n_dup, k), generator=gen, device=device, dtype=torch.int64)
    return members


def hyperedge_sizes(n_e: int, degree: float, dist: str, gen: torch.Generator, device, max_degree: int = 4096,
                    zipf_a: float = 2.0) -> torch.Tensor:
    """int64[n_e] hyperedge sizes.  'fixed': all == degree.  'poisson': Poisson(degree) clipped to >= 1.
    'zipf': truncated power law P(s) ~ s^-a on [1, max_degree], rescaled so the mean is ~degree."""
    if dist == "fixed":
        return torch.full((n_e,), int(degree), dtype=torch.int64, device=device)
    if dist == "poisson":
        lam = torch.full((n_e,), float(degree), device=device)
        return torch.poisson(lam, generator=gen).clamp_(min=1).to(torch.int64)
    if dist == "zipf":
        s = torch.arange(1, max_degree + 1, device=device, dtype=torch.float64)
        pmf = s.pow(-zipf_a)
        pmf /= pmf.sum()
        draw = torch.multinomial(pmf.float(), n_e, replacement=True, generator=gen) + 1      # in [1, max_degree]
        mean = float(draw.double().mean())
        scaled = (draw.double() * (degree / mean)).round().clamp_(1, max_degree)
        return scaled.to(torch.int64)
    raise ValueError(f"unknown degree distribution {dist!r}")


def random_hypergraph(n_v: int, n_e: int, degree: float = 16, seed: int = 0, device="cuda", dist: str = "fixed",
                      max_degree: int = 4096, e_base: int = 0, e_offset: int = 0, sort_by_vertex: bool = True,
                      zipf_a: float = 2.0, locality: float = 0.0, home=None) -> SimpleNamespace:
    """``n_e`` hyperedges over ``n_v`` vertices.  Returns ``SimpleNamespace(edge_index, norm, n_v, n_e,
    nnz, seed, dist)`` with ``edge_index`` int64 [2, nnz] (row 0 vertex ids, row 1 hyperedge ids
    ``e_base + e_offset + [0, n_e)``) on ``device``.

    ``e_offset`` lets one rank of a sharded run generate only its own block of hyperedges (their members
    still range over the global vertex set).

    ``locality`` in [0, 1) with ``home = (block, n_blocks)``: each membership is re-drawn, with that probability, from the
    home block of vertices ``[block * n_v / n_blocks, (block + 1) * n_v / n_blocks)`` -- a hypergraph whose partitions have few
    boundary vertices (what the row partition's boundary-vertex exchange, ``allset_amd.dist.Halo``, is for).  0 = the uniform
    hypergraph of the benchmark.  (Re-drawn members may repeat inside a hyperedge; duplicates are coalesced.)
    """
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    if dist == "fixed":
        k = int(degree)
        members = _distinct_members(n_e, k, n_v, gen, device)
        v = members.reshape(-1)
        e = torch.arange(n_e, device=device, dtype=torch.int64).repeat_interleave(k)
    else:
        sizes = hyperedge_sizes(n_e, degree, dist, gen, device, max_degree, zipf_a).clamp_(max=n_v)
        e = torch.arange(n_e, device=device, dtype=torch.int64).repeat_interleave(sizes)
        v = torch.randint(n_v, (int(e.numel()),), generator=gen, device=device, dtype=torch.int64)
        key = torch.unique(e * n_v + v)            # coalesce duplicate memberships (as the reference loaders do)
        e, v = key // n_v, key % n_v
    if locality > 0.0:
        if home is None:
            raise ValueError("locality needs home = (block, n_blocks)")
        blk, nb = int(home[0]), int(home[1])
        per = n_v // nb
        local = torch.rand(v.shape, generator=gen, device=device) < float(locality)
        redraw = blk * per + torch.randint(per, v.shape, generator=gen, device=device, dtype=torch.int64)
        v = torch.where(local, redraw, v)
        key = torch.unique(e * n_v + v)
        e, v = key // n_v, key % n_v
    if sort_by_vertex:
        order = torch.argsort(v, stable=True)
        v, e = v[order], e[order]
    edge_index = torch.stack([v, e + (e_base + e_offset)], dim=0).contiguous()
    norm = torch.ones(edge_index.shape[1], dtype=torch.int64, device=device)
    return SimpleNamespace(edge_index=edge_index, norm=norm, n_v=n_v, n_e=n_e, nnz=int(edge_index.shape[1]),
                           seed=int(seed), dist=dist)


def acm_like_hetero(n_papers: int = 3000, n_authors: int = 4000, n_fields: int = 30, num_classes: int = 3, num_features: int = 128,
                    authors_per_paper: int = 3, orphan_fraction: float = 0.05, field_skew: float = 1.5, signal: float = 0.25,
                    seed: int = 0, device="cuda") -> SimpleNamespace:
    """A seeded ACM-shaped typed graph for the heterogeneous HAN (``han_hetero``): papers, authors and fields with the relations
    ``pa`` / ``ap`` (paper - author, both directions) and ``pf`` / ``fp`` (paper - field).

    Every paper has ONE field, drawn from ``P(f) ~ (f + 1) ** -field_skew`` within its class's share of the fields (so field sizes are
    strongly skewed and PFP has hub rows: field 0 holds a large part of its class), and 1 .. ``2 * authors_per_paper - 1`` distinct
    authors, mostly from its class's share of the authors -- except the ``orphan_fraction`` of the papers that have NO author: PAP has
    zero-in-degree nodes.  Features are binary bag-of-words rows, a word being likelier (by ``signal``) inside its class's share of the
    vocabulary; labels are on the papers.  Drawn on the host from ``numpy.random.default_rng(seed)``: the same graph on every device.

    Returns ``SimpleNamespace(edges, num_nodes, features, labels, num_classes, orphans)``: ``edges`` maps ``(srctype, etype, dsttype)``
    to ``(src, dst)`` int64 id tensors on ``device`` (the first argument of ``dgl.heterograph``), ``num_nodes`` maps a type to its
    count, ``features`` f32 [n_papers, num_features], ``labels`` int64 [n_papers], ``orphans`` the number of author-less papers."""
    import numpy as np
    if min(n_papers, n_authors, n_fields, num_classes, num_features) < 1 or n_fields < num_classes or n_authors < num_classes:
        raise ValueError("acm_like_hetero: every count must be >= 1, with at least one field and one author per class")
    if not 0.0 <= orphan_fraction < 1.0:
        raise ValueError("acm_like_hetero: orphan_fraction must be in [0, 1)")
    rng = np.random.default_rng(int(seed))
    labels = rng.integers(0, num_classes, size=n_papers)
    # fields: class c owns fields c, c + num_classes, c + 2 num_classes, ...; a power law over the owned ones
    field = np.empty(n_papers, dtype=np.int64)
    for c in range(num_classes):
        own = np.arange(c, n_fields, num_classes)
        w = (np.arange(own.size) + 1.0) ** -float(field_skew)
        idx = np.nonzero(labels == c)[0]
        field[idx] = own[rng.choice(own.size, size=idx.size, p=w / w.sum())]
    # authors: 1 .. 2 k - 1 per paper, 80 % from the class's share; orphans have none
    orphan = rng.random(n_papers) < orphan_fraction
    n_auth = np.where(orphan, 0, rng.integers(1, 2 * authors_per_paper, size=n_papers))
    p_ids = np.repeat(np.arange(n_papers, dtype=np.int64), n_auth)
    own_class = rng.random(p_ids.size) < 0.8
    per = n_authors // num_classes
    home = labels[p_ids] * per + rng.integers(0, per, size=p_ids.size)
    a_ids = np.where(own_class, home, rng.integers(0, n_authors, size=p_ids.size)).astype(np.int64)
    key = np.unique(p_ids * n_authors + a_ids)                                   # distinct authors within a paper
    p_ids, a_ids = key // n_authors, key % n_authors
    # bag of words
    words = num_features // num_classes
    prob = np.full((n_papers, num_features), 0.05)
    for c in range(num_classes):
        rows = np.nonzero(labels == c)[0]
        prob[np.ix_(rows, np.arange(c * words, (c + 1) * words))] += float(signal)
    feats = (rng.random((n_papers, num_features)) < prob).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)
    papers = np.arange(n_papers, dtype=np.int64)
    edges = {("paper", "pa", "author"): (t(p_ids), t(a_ids)), ("author", "ap", "paper"): (t(a_ids), t(p_ids)),
             ("paper", "pf", "field"): (t(papers), t(field)), ("field", "fp", "paper"): (t(field), t(papers))}
    return SimpleNamespace(edges=edges, num_nodes={"paper": n_papers, "author": n_authors, "field": n_fields},
                           features=torch.from_numpy(feats).to(device), labels=torch.from_numpy(labels.astype(np.int64)).to(device),
                           num_classes=int(num_classes), orphans=int(orphan.sum()))
