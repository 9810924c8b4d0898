"""The HAN baseline of the reference's results table (``src/DGL_HAN/``: ``model.py``, ``main.py``, ``utils.py``) on the HIP path.

In the reference HAN is a separate program on DGL; here it is this module: the model classes with the reference's names, constructor
signatures and ``state_dict`` layout (``GATConv`` restates DGL 0.7.1's), the metapath graphs built on the device from the project's
(vertex, hyperedge) incidence, and the driver ``python -m allset_amd.han`` with ``main.py``'s flags and ``utils.default_configure``'s
settings.  The per-metapath attention hops and the semantic attention are HIP kernels (``csrc/han.hip``,
``functional.han_gat_propagate`` / ``functional.semantic_attention``); each hop writes its column block of the stacked
``[N, M * H * C]`` buffer directly.

Two choices are this project's, because the generator of the reference's ``*_raw.pickle`` files is not in its tree: hyperedge nodes
get ZERO feature rows and label ``-1`` (so they are never in a split).  Reading those external pickles is out of scope.

``--hetero`` is the reference's other mode (one typed graph, metapaths of edge types): ``allset_amd/han_hetero.py``; the loop below serves both.
"""
from __future__ import annotations

import argparse
import copy
import time
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, dense
from .functional import han_gat_propagate, semantic_attention
from .incidence import Incidence

Tensor = torch.Tensor
INT32_MAX = 2 ** 31 - 1


# --------------------------------------------------------------------------------------------------
# metapath graphs
# --------------------------------------------------------------------------------------------------

class MetapathGraph:
    """A directed multigraph over ``n`` nodes in both CSR orientations, built once on the device.

    ``src`` / ``dst`` int64[nnz]: the edge list (source -> target), duplicates kept.  ``rowptr`` / ``col``: target-major CSR (an
    edge's slot there is its identity for the attention dropout), ``perm``: slot -> edge-list position.  ``rowptrT`` / ``colT``:
    source-major CSR, ``slotT``: the target-major slot of each of its entries.  A node without an incoming edge raises, as DGL's
    ``GATConv`` does (its softmax would be over nothing)."""

    def __init__(self, src: Tensor, dst: Tensor, n: int):
        if src.numel() > INT32_MAX:
            raise ValueError(f"metapath graph with {src.numel()} edges: edge slots are int32 (at most {INT32_MAX})")
        self.n, self.nnz = int(n), int(src.numel())
        if self.n > 0 and bool((torch.bincount(dst, minlength=self.n) == 0).any()):
            raise ValueError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. Adding a self-loop on "
                             "every node (as metapath_graphs does) resolves the issue.")
        _lib.require_device(src, dst)
        self.src, self.dst = src.contiguous(), dst.contiguous()
        inc = Incidence.from_edge_index(torch.stack([self.src, self.dst]), n_src=self.n, n_dst=self.n)
        self.rowptr, self.col, self.perm = inc.by_dst.rowptr, inc.by_dst.col, inc.by_dst.perm
        self.rowptrT, self.colT = inc.by_src.rowptr, inc.by_src.col
        self.slotT = inc.pos_dst_of_src()


def metapath_edges(edge_index: Tensor, n_v: int, n_e: int):
    """The VEV and EVE edge lists (each ``(row, col)`` int64, edges row -> col) over ``n_v + n_e`` nodes from (vertex, hyperedge)
    incidences ``edge_index`` int64[2, nnz] with zero-based hyperedge ids: nodes ``0..n_v-1`` are the vertices, ``n_v..n_v+n_e-1`` the
    hyperedges; VEV = the non-zeros of binarised ``H H^T`` on the vertex block, EVE those of ``H^T H`` on the hyperedge block, in
    row-major order; then ONE self-loop appended for every node (``dgl.add_self_loop``: existing loops are not removed, so a node
    with a diagonal entry has two).  Torch programs on ``edge_index``'s device; off the per-step path."""
    v, e = edge_index[0], edge_index[1]
    n = n_v + n_e
    key = torch.unique(v * n_e + e)                       # binarise H (duplicate incidences count once)
    v, e = key // max(n_e, 1), key % max(n_e, 1)
    loops = torch.arange(n, dtype=torch.int64, device=edge_index.device)

    def two_hop(a, b, n_a, base):
        """Pairs (a_i, a_j) sharing a b: the non-zeros of the binarised product, row-major."""
        order = torch.argsort(b, stable=True)
        a_s, b_s = a[order], b[order]
        cnt = torch.bincount(b_s, minlength=1)
        total = int((cnt * cnt).sum())
        if total > INT32_MAX:
            raise ValueError(f"metapath expansion has {total} candidate pairs: edge counts must fit int32")
        start = torch.cumsum(cnt, 0) - cnt
        rep = cnt[b_s]                                     # each member pairs with every member of its group
        left = torch.repeat_interleave(torch.arange(a_s.numel(), device=a.device), rep)
        off = torch.arange(left.numel(), device=a.device) - torch.repeat_interleave(torch.cumsum(rep, 0) - rep, rep)
        right = start[b_s[left]] + off
        k = torch.unique(a_s[left] * n_a + a_s[right])
        return k // max(n_a, 1) + base, k % max(n_a, 1) + base

    out = []
    for a, b, n_a, base in ((v, e, n_v, 0), (e, v, n_e, n_v)):
        r, c = two_hop(a, b, n_a, base) if a.numel() else (loops[:0], loops[:0])
        if r.numel() + n > INT32_MAX:
            raise ValueError(f"metapath graph with {r.numel() + n} edges: edge counts must fit int32")
        out.append((torch.cat([r, loops]), torch.cat([c, loops])))
    return out


def metapath_graphs(data, e_base: int = 0) -> List[MetapathGraph]:
    """``[VEV, EVE]`` for a hypergraph ``data`` whose ``edge_index`` holds the (vertex, hyperedge) incidences with hyperedge ids
    starting at ``e_base`` (0, or ``n_x`` for the V->E half as ``preprocessing.ExtractV2E`` leaves it), ``n_x`` vertices and
    ``num_hyperedges`` hyperedges -- see :func:`metapath_edges`.  The node set is vertices then hyperedges; :func:`node_features` gives hyperedge nodes
    zero feature rows and label -1 (this project's choice: the reference's generator of these inputs is not in its tree)."""
    n_v, n_e = _first(data.n_x), _first(data.num_hyperedges)
    ei = data.edge_index
    _lib.require_device(ei)
    if e_base:
        ei = torch.stack([ei[0], ei[1] - int(e_base)])
    if ei.numel() and (int(ei[0].min()) < 0 or int(ei[0].max()) >= n_v or int(ei[1].min()) < 0 or int(ei[1].max()) >= n_e):
        raise ValueError(f"metapath_graphs: incidences outside {n_v} vertices x {n_e} hyperedges (hyperedge ids start at e_base = {e_base})")
    return [MetapathGraph(r, c, n_v + n_e) for r, c in metapath_edges(ei, n_v, n_e)]


def node_features(data):
    """``(features [n_v + n_e, F], labels [n_v + n_e])``: hyperedge nodes get zero rows and label -1."""
    n_v, n_e = _first(data.n_x), _first(data.num_hyperedges)
    x = torch.cat([data.x.float(), torch.zeros((n_e, data.x.shape[1]), dtype=torch.float32, device=data.x.device)])
    y = torch.cat([data.y.long(), torch.full((n_e,), -1, dtype=torch.int64, device=data.y.device)])
    return x, y


def _first(v) -> int:
    return int(v[0]) if isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() > 0) else int(v)


# --------------------------------------------------------------------------------------------------
# model (reference DGL_HAN/model.py; GATConv: dgl 0.7.1 nn/pytorch/conv/gatconv.py)
# --------------------------------------------------------------------------------------------------

class GATConv(nn.Module):
    """DGL 0.7.1 ``GATConv`` as HAN uses it: no residual, a bias, one shared ``fc``; ``state_dict`` keys ``fc.weight``, ``attn_l``
    [1, H, C], ``attn_r`` [1, H, C], ``bias`` [H * C].  Only ``activation=F.elu`` (HAN's) is built into the kernel."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0., negative_slope=0.2, residual=False,
                 activation=None, allow_zero_in_degree=False, bias=True):
        super().__init__()
        if residual or not bias or allow_zero_in_degree:
            raise ValueError("GATConv: residual / bias=False / allow_zero_in_degree are not built (HAN uses none of them)")
        if activation is not F.elu:
            raise ValueError("GATConv: the HIP hop is built with HAN's activation, F.elu")
        self._num_heads, self._in_feats, self._out_feats = num_heads, in_feats, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop, self.attn_drop, self.negative_slope = float(feat_drop), float(attn_drop), float(negative_slope)
        self.bias = nn.Parameter(torch.empty(num_heads * out_feats))
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        nn.init.constant_(self.bias, 0)

    def forward(self, graph: MetapathGraph, feat: Tensor, out: Optional[Tensor] = None, block: int = 0) -> Tensor:
        """[N, H, C] -- or, with ``out``, the stacked buffer itself with column block ``block`` filled."""
        H, C = self._num_heads, self._out_feats
        h = dense.hash_dropout(feat, self.feat_drop, self.training)
        fs = dense.linear(h, self.fc.weight, None)
        f3 = fs.view(-1, H, C)
        el = (f3 * self.attn_l).sum(-1)
        er = (f3 * self.attn_r).sum(-1)
        y = han_gat_propagate(fs, el, er, graph, H, self.negative_slope, self.bias, self.attn_drop if self.training else 0.0, out, block)
        return y if out is not None else y.view(-1, H, C)


class SemanticAttention(nn.Module):
    def __init__(self, in_size, hidden_size=128):
        super().__init__()
        self.project = nn.Sequential(nn.Linear(in_size, hidden_size), nn.Tanh(), nn.Linear(hidden_size, 1, bias=False))

    def forward(self, z: Tensor) -> Tensor:
        """``z`` [N, M, D] -> [N, D]."""
        return semantic_attention(z, self.project[0].weight, self.project[0].bias, self.project[2].weight.view(-1))


class HANLayer(nn.Module):
    def __init__(self, num_meta_paths, in_size, out_size, layer_num_heads, dropout):
        super().__init__()
        self.gat_layers = nn.ModuleList()
        for _ in range(num_meta_paths):
            self.gat_layers.append(GATConv(in_size, out_size, layer_num_heads, dropout, dropout, activation=F.elu))
        self.semantic_attention = SemanticAttention(in_size=out_size * layer_num_heads)
        self.num_meta_paths = num_meta_paths

    def forward(self, gs, h: Tensor) -> Tensor:
        M = len(gs)
        d = self.gat_layers[0]._num_heads * self.gat_layers[0]._out_feats
        z = torch.empty((h.shape[0], M * d), dtype=torch.float32, device=h.device)      # the reference's torch.stack(..., dim=1)
        for i, g in enumerate(gs):
            z = self.gat_layers[i](g, h, out=z, block=i)
        return self.semantic_attention(z.view(h.shape[0], M, d))


class HAN(nn.Module):
    def __init__(self, num_meta_paths, in_size, hidden_size, out_size, num_heads, dropout):
        super().__init__()
        self.layers = nn.ModuleList()
        self.layers.append(HANLayer(num_meta_paths, in_size, hidden_size, num_heads[0], dropout))
        for l in range(1, len(num_heads)):
            self.layers.append(HANLayer(num_meta_paths, hidden_size * num_heads[l - 1], hidden_size, num_heads[l], dropout))
        self.predict = nn.Linear(hidden_size * num_heads[-1], out_size)

    def forward(self, g, h: Tensor) -> Tensor:
        for gnn in self.layers:
            h = gnn(g, h)
        return dense.linear(h, self.predict.weight, self.predict.bias)


# --------------------------------------------------------------------------------------------------
# driver (reference DGL_HAN/main.py, utils.py)
# --------------------------------------------------------------------------------------------------

default_configure = {'lr': 0.005, 'num_heads': [8], 'hidden_units': 8, 'dropout': 0.6, 'weight_decay': 0.001, 'num_epochs': 200,
                     'patience': 100}


class EarlyStopping:
    """The reference's rule (utils.py:369-404) with the best state kept in memory: the first step saves; a step whose loss is higher
    AND whose accuracy is lower than the best of each counts towards ``patience``; any other step resets the count, updates the two
    bests separately, and saves only if it is at least as good in BOTH."""

    def __init__(self, patience=10):
        self.patience = patience
        self.counter = 0
        self.best_acc = None
        self.best_loss = None
        self.early_stop = False
        self.best_state = None
        self.saves = 0

    def step(self, loss, acc, model):
        if self.best_loss is None:
            self.best_acc = acc
            self.best_loss = loss
            self.save_checkpoint(model)
        elif (loss > self.best_loss) and (acc < self.best_acc):
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True
        else:
            if (loss <= self.best_loss) and (acc >= self.best_acc):
                self.save_checkpoint(model)
            self.best_loss = min(loss, self.best_loss)
            self.best_acc = max(acc, self.best_acc)
            self.counter = 0
        return self.early_stop

    def save_checkpoint(self, model):
        self.best_state = copy.deepcopy(model.state_dict())
        self.saves += 1

    def load_checkpoint(self, model):
        model.load_state_dict(self.best_state)


def rand_train_test_idx(label, train_prop=.5, valid_prop=.25):
    """The reference's non-balanced split over the labelled nodes (main.py:31-60): one ``np.random.permutation`` per call."""
    labeled = torch.where(label != -1)[0]
    n = labeled.shape[0]
    train_num, valid_num = int(n * train_prop), int(n * valid_prop)
    perm = torch.as_tensor(np.random.permutation(n)).to(labeled.device)
    return {'train': labeled[perm[:train_num]], 'valid': labeled[perm[train_num:train_num + valid_num]],
            'test': labeled[perm[train_num + valid_num:]]}


def score(logits: Tensor, labels: Tensor):
    """``(accuracy, micro F1, macro F1)`` in torch, as sklearn's ``f1_score`` counts them: classes = those present in the labels or
    the predictions, a class's F1 = 2 tp / (2 tp + fp + fn), macro = their plain mean, micro from the pooled counts."""
    pred = logits.argmax(dim=1)
    k = int(max(int(labels.max()), int(pred.max()))) + 1 if labels.numel() else 1
    conf = torch.bincount(labels * k + pred, minlength=k * k).view(k, k).double()
    tp = conf.diag()
    fp, fn = conf.sum(0) - tp, conf.sum(1) - tp
    present = (conf.sum(0) + conf.sum(1)) > 0
    f1 = torch.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp(min=1), torch.zeros_like(tp))
    micro = float(2 * tp.sum() / (2 * tp.sum() + fp.sum() + fn.sum()).clamp(min=1))
    macro = float(f1[present].mean()) if bool(present.any()) else 0.0
    acc = float((pred == labels).double().mean()) if labels.numel() else 0.0
    return acc, micro, macro


def evaluate(model, gs, features, labels, mask, loss_func):
    model.eval()
    with torch.no_grad():
        logits = model(gs, features)
    loss = loss_func(logits[mask], labels[mask])
    return (loss,) + score(logits[mask], labels[mask])


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser('HAN')
    p.add_argument('-s', '--seed', type=int, default=1, help='Random seed')
    p.add_argument('--hetero', action='store_true', help="one typed graph and metapaths of edge types (allset_amd.han_hetero) instead "
                   "of the hypergraph's VEV / EVE graphs")
    p.add_argument('--dataset', default='synthetic', help="'synthetic' or a dataset name train.py loads (with --raw_data_dir / "
                   "--processed_data)")
    p.add_argument('--runs', type=int, default=20)
    p.add_argument('--cuda', type=int, default=0)
    p.add_argument('--feature_noise', type=float, default=1)
    p.add_argument('--train_prop', type=float, default=0.5)
    p.add_argument('--valid_prop', type=float, default=0.25)
    # additions of this driver: where train.py's loaders find a named dataset, and a shorter run for tests
    p.add_argument('--raw_data_dir', default=None)
    p.add_argument('--processed_data', default=None)
    p.add_argument('--num_epochs', type=int, default=None, help=f"default {default_configure['num_epochs']}")
    return p


def setup(args: dict) -> dict:
    epochs = args.pop('num_epochs', None)
    args.update(default_configure)
    if epochs is not None:
        args['num_epochs'] = epochs
    np.random.seed(args['seed'])
    torch.manual_seed(args['seed'])
    args['device'] = f"cuda:{args['cuda']}"
    return args


def load_data(args: dict):
    """``(gs, features, labels, num_classes)`` on ``args['device']``; with ``--hetero``, ``gs`` is the typed graph itself."""
    if args.get('hetero'):
        from . import han_hetero
        return han_hetero.load_data(args)
    from . import train
    from .preprocessing import ExtractV2E
    targs = SimpleNamespace(dname=args['dataset'], raw_data_dir=args.get('raw_data_dir'), processed_data=args.get('processed_data'),
                            feature_noise=str(args['feature_noise']), seed=args['seed'])
    data = ExtractV2E(train.load_data(targs))
    data = data.to(args['device'])
    features, labels = node_features(data)
    return metapath_graphs(data, e_base=_first(data.n_x)), features, labels, int(targs.num_classes)


def main(args: dict) -> dict:
    gs, features, labels, num_classes = load_data(args)
    num_nodes = features.shape[0]
    history = {'acc': [], 'micro_f1': [], 'macro_f1': [], 'time': [], 'train_loss': []}
    for run in range(args['runs']):
        start = time.time()
        split = rand_train_test_idx(labels, args['train_prop'], args['valid_prop'])
        masks = {}
        for k, idx in split.items():
            masks[k] = torch.zeros(num_nodes, dtype=torch.bool, device=features.device)
            masks[k][idx] = True
        if args.get('hetero'):
            from . import han_hetero
            model = han_hetero.make_model(args, features.shape[1], num_classes).to(args['device'])
        else:
            model = HAN(num_meta_paths=len(gs), in_size=features.shape[1], hidden_size=args['hidden_units'], out_size=num_classes,
                        num_heads=args['num_heads'], dropout=args['dropout']).to(args['device'])
        stopper = EarlyStopping(patience=args['patience'])
        loss_fcn = torch.nn.CrossEntropyLoss()
        optimizer = torch.optim.Adam(model.parameters(), lr=args['lr'], weight_decay=args['weight_decay'])
        losses = []
        for epoch in range(args['num_epochs']):
            model.train()
            logits = model(gs, features)
            loss = loss_fcn(logits[masks['train']], labels[masks['train']])
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            val_loss, val_acc, _, _ = evaluate(model, gs, features, labels, masks['valid'], loss_fcn)
            if stopper.step(float(val_loss), val_acc, model):
                break
        stopper.load_checkpoint(model)
        _, test_acc, test_micro, test_macro = evaluate(model, gs, features, labels, masks['test'], loss_fcn)
        history['acc'].append(100 * test_acc)
        history['micro_f1'].append(100 * test_micro)
        history['macro_f1'].append(100 * test_macro)
        history['train_loss'].append(losses)
        history['time'].append(time.time() - start)
    print(f">> Final test acc: {np.mean(history['acc']):.2f}, std: {np.std(history['acc']):.2f}; "
          f"test marco f1: {np.mean(history['macro_f1']):.2f}, std: {np.std(history['macro_f1']):.2f}")
    print(f">> Train time per run: {np.mean(history['time']):.2f}, std: {np.std(history['time']):.2f}")
    return history


if __name__ == '__main__':
    main(setup(build_parser().parse_args().__dict__))
