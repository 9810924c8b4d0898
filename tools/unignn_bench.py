"""Timing of the UniGNN baselines' hops (csrc/unignn.hip) at |V| = |E| = 2^20, hyperedges of size 16, d = 128 and
256, every group's arms alternating in the same run (median of ``--reps`` repetitions of 10 calls, with the min..max spread):

K1  the fused E->V hop (``ops.unignn_hop_fwd``: degV scale, self term, row norm, relu, dropout 0.5) against the existing degree-scaled
    launch it extends (``ops.hconv_propagate`` over the same vertex-major CSR with ``s = degV``: csrc/hconv.hip, which this work leaves
    byte-identical) and against the unfused composition (that launch plus torch ops and the one-pass relu + dropout): milliseconds,
    algorithmic bytes and their fraction of 8 TB/s, the time ratio against the ratio of algorithmic bytes.
K2  UniGAT's V->E hop with the logit (``ops.unignn_v2e_att_fwd``, 8 heads) against ``hconv_propagate`` v2e plus the separate logit pass.
E2V UniGAT's attention pooling (``ops.pma_fwd``) alone and followed by the separate row tail (norm + skip + relu + dropout).
Steps: a graphed training step per conv (ms per replay) on a Cora-shaped synthetic hypergraph.

    python tools/unignn_bench.py [--skip-large] [--skip-steps] [--reps N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, dense, ops  # noqa: E402
from allset_amd.functional import unignn_row_tail  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _time_alternating(fns, reps=7, iters=10, warm=3):
    """Median / min / max ms per call of every function, their windows interleaved (A B C A B C ...) so that what else runs on the
    machine meets all of them alike."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(_window(fn, iters))
    return {k: dict(ms=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}


def large(reps):
    n, k, H = 1 << 20, 16, 8
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    inc = Incidence.from_edge_index(torch.stack([v, e]), n_src=n, n_dst=n)
    del v, e
    inc_ev = inc.reversed(n_dst=n)
    nnz = inc.nnz
    degV = torch.rand(n, device=DEV) + 0.5
    inv_size = torch.full((n,), 1.0 / k, device=DEV)
    out = {"n_vertices": n, "n_hyperedges": n, "incidences": nnz}
    with torch.no_grad():
        for d in (128, 256):
            xe, xs = torch.randn(n, d, device=DEV), torch.randn(n, d, device=DEV)
            att = torch.randn(d, device=DEV)
            hconv_bytes = nnz * (4 * d + 4) + (n + 1) * 4 + n * 4 * d + n * 4
            r = {}
            # ---- K1
            def unfused_gcn():
                a = ops.hconv_propagate(inc.by_src, xe, n, s=degV)
                nrm = a.norm(dim=1)
                t = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
                return dense.relu_dropout(a * t.unsqueeze(1), 0.5)

            def unfused_gin():
                a = ops.hconv_propagate(inc.by_src, xe, n) + xs * 1.25
                nrm = a.norm(dim=1)
                t = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
                return dense.relu_dropout(a * t.unsqueeze(1), 0.5)
            arms = {"hconv_fwd_e2v": (lambda: ops.hconv_propagate(inc.by_src, xe, n, s=degV), hconv_bytes),
                    "k1_gcn_norm_relu_drop": (lambda: ops.unignn_hop_fwd(inc.by_src, xe, n, degV, None, 1.0, True, "relu", 0.5, 7),
                                              hconv_bytes + n * 4),
                    "k1_gin_self_norm_relu_drop": (lambda: ops.unignn_hop_fwd(inc.by_src, xe, n, None, xs, 1.25, True, "relu", 0.5, 7),
                                                   hconv_bytes + n * 4 * d),
                    "k1_sage_self_plain": (lambda: ops.unignn_hop_fwd(inc.by_src, xe, n, None, xs, 1.0, False, None, 0.0),
                                           hconv_bytes - n * 4 + n * 4 * d),
                    "unfused_gcn_hconv_plus_torch": (unfused_gcn, None), "unfused_gin_hconv_plus_torch": (unfused_gin, None)}
            t = _time_alternating({kk: f for kk, (f, _) in arms.items()}, reps)
            base = t["hconv_fwd_e2v"]
            for kk, (_, b) in arms.items():
                r[kk] = dict(t[kk])
                if b is not None:
                    r[kk].update(algo_bytes=int(b), frac_8TBs=b / (t[kk]["ms"] * 1e-3) / PEAK, bytes_ratio_over_hconv=b / hconv_bytes,
                                 time_ratio_over_hconv=t[kk]["ms"] / base["ms"])
            r["hconv_spread_max_over_min"] = base["ms_max"] / base["ms_min"]
            # ---- K2
            def v2e_unfused():
                z = ops.hconv_propagate(inc.by_dst, xs, n, s=inv_size)
                return z, (z.view(n, H, -1) * att.view(1, H, -1)).sum(-1)
            t2 = _time_alternating({"hconv_fwd_v2e": lambda: ops.hconv_propagate(inc.by_dst, xs, n, s=inv_size),
                                    "k2_v2e_att": lambda: ops.unignn_v2e_att_fwd(inc.by_dst, xs, n, inv_size, att, H),
                                    "unfused_v2e_plus_logit_pass": v2e_unfused}, reps)
            t2["k2_time_ratio_over_unfused"] = t2["k2_v2e_att"]["ms"] / t2["unfused_v2e_plus_logit_pass"]["ms"]
            t2["k2_time_ratio_over_hconv_v2e"] = t2["k2_v2e_att"]["ms"] / t2["hconv_fwd_v2e"]["ms"]
            r["v2e"] = t2
            # ---- UniGAT's E->V: the pooling launch and the separate tail behind it
            ae = torch.randn(n, H, device=DEV)
            csr = inc_ev.by_dst

            def pool():
                return ops.pma_fwd(csr.rowptr, csr.col, ae, xe, H, 0.2, n, variant=1, row_order=csr.row_order)[0]
            t3 = _time_alternating({"pma_fwd_e2v": pool,
                                    "pma_fwd_plus_relu_dropout": lambda: dense.relu_dropout(pool(), 0.5),
                                    "pma_fwd_plus_norm_skip_tail": lambda: unignn_row_tail(pool(), skip=xs, use_norm=True, act="relu", p=0.5)},
                                   reps)
            t3["tail_cost_ms_relu_dropout"] = t3["pma_fwd_plus_relu_dropout"]["ms"] - t3["pma_fwd_e2v"]["ms"]
            t3["tail_cost_ms_norm_skip"] = t3["pma_fwd_plus_norm_skip_tail"]["ms"] - t3["pma_fwd_e2v"]["ms"]
            r["unigat_e2v"] = t3
            out[f"d{d}"] = r
            del xe, xs, ae
    return out


def graphed_steps(reps):
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.train import UNIGNN_CONV_METHODS, build_model, build_parser, make_optimizer, preprocess, synthetic_dataset
    out = {}
    for method in UNIGNN_CONV_METHODS:
        n_v, n_e, f, c = 2708, 1579, 1433, 7
        args = build_parser().parse_args(["--method", method, "--heads", "2", "--MLP_hidden", "32", "--UniGNN_use-norm"])
        data = preprocess(args, synthetic_dataset(n_v=n_v, n_e=n_e, num_classes=c, num_features=f, seed=0))
        args.num_features, args.num_classes = f, c
        model = build_model(args, data).to(DEV)
        data = data.to(DEV)
        args.degV = args.UniGNN_degV = args.UniGNN_degV.to(DEV)
        args.degE = args.UniGNN_degE = args.UniGNN_degE.to(DEV)
        y = data.y.long()
        step = GraphedTrainStep(model, data, lambda o: torch.nn.functional.nll_loss(o, y), make_optimizer(args, model))
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        ms = [_window(step, 200) for _ in range(reps)]
        out[f"cora_{method}_use_norm_graphed_step"] = dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_large:
        res.update(large(a.reps))
    if not a.skip_steps:
        res.update(graphed_steps(a.reps))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
