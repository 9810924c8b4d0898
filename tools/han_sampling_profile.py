"""Time one training step of mini-batch HAN (allset_amd/han_sampling.py), split into sampler walk, block build, forward, and backward
+ Adam, and count the launches per step; on the synthetic dataset and on a Cora-shaped one, at batch sizes 32 (the reference's
default) and 1024.

The yardsticks of the sampler are written HERE and share nothing with the code under test: ``torch_sample`` restates the same
sampling (k two-hop walks per seed over the two CSRs, distinct endpoints, self-loop, seeds-first relabelling) in torch ops on the
same device with torch's own generator, and ``tests/han_sampling_oracle.py`` is the numpy restatement on the CPU.  Every figure is the
median of ``--repeats`` repetitions of ``--steps`` steps with the spread (min .. max) beside it.

    python tools/han_sampling_profile.py [--out profiles/han_sampling.json]

``--fixed`` measures the sync-free path instead, for the same four rows: the eager step as it was (the
yardstick, re-measured in the same session), the sampler over ``sample_blocks_fixed`` (launches and time), the eager step on fixed
blocks and the step replayed as one graph (``GraphedSampledStep``):

    python tools/han_sampling_profile.py --fixed --out profiles/han_sampling_fixed.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = torch.device("cuda:0")


def datasets():
    from allset_amd import train
    from allset_amd.preprocessing import ExtractV2E
    import han_cases as hc
    out = {}
    targs = SimpleNamespace(dname="synthetic", raw_data_dir=None, processed_data=None, feature_noise="1", seed=1)
    data = ExtractV2E(train.load_data(targs))
    n_v = int(data.n_x[0]) if isinstance(data.n_x, (list, tuple)) else int(data.n_x)
    n_e = int(data.num_hyperedges[0]) if isinstance(data.num_hyperedges, (list, tuple)) else int(data.num_hyperedges)
    ei = data.edge_index.clone()
    v, e = ei[0], ei[1] - n_v
    keep = (v < n_v) & (e >= 0)
    out["synthetic"] = (torch.stack([v[keep], e[keep]]), n_v, n_e, data.x.float(), data.y.long(), int(targs.num_classes))
    c = hc.spec("cora_han")
    x, pairs, n_v, n_e = hc.raw_data(c)
    y = torch.from_numpy(np.random.default_rng(0).integers(0, 7, size=n_v))
    out["cora-shaped"] = (torch.from_numpy(pairs), n_v, n_e, torch.from_numpy(x[:n_v]).float(), y, 7)
    return out


def torch_sample(v2e, e2v, n_v, mp, seeds, k, gen):
    """The yardstick: the same sampling in torch ops.  ``v2e`` / ``e2v`` = (rowptr int64, col int64)."""
    (rpa, ca), (rpb, cb), base = ((v2e, e2v, 0) if mp == 0 else (e2v, v2e, n_v))
    B = seeds.numel()
    loc = seeds - base
    ok = (loc >= 0) & (loc < rpa.numel() - 1)
    locc = loc.clamp(0, rpa.numel() - 2)
    deg = (rpa[locc + 1] - rpa[locc]) * ok
    u = torch.rand((B, k), device=seeds.device, generator=gen)
    alive = deg > 0
    mid = ca[(rpa[locc].unsqueeze(1) + (u * deg.unsqueeze(1)).long().clamp(max=(deg - 1).clamp(min=0).unsqueeze(1))).clamp(max=ca.numel() - 1)]
    d2 = rpb[mid + 1] - rpb[mid]
    u2 = torch.rand((B, k), device=seeds.device, generator=gen)
    end = cb[(rpb[mid] + (u2 * d2).long().clamp(max=(d2 - 1).clamp(min=0))).clamp(max=cb.numel() - 1)] + base
    end = torch.where(alive.unsqueeze(1) & (end != seeds.unsqueeze(1)), end, torch.full_like(end, -1))
    tgt = torch.arange(B, device=seeds.device).unsqueeze(1).expand(B, k)
    key = torch.unique(tgt[end >= 0] * (2 ** 31) + end[end >= 0])                    # distinct (target, endpoint), ascending
    t, g = key // (2 ** 31), key % (2 ** 31)
    t, g = torch.cat([t, torch.arange(B, device=seeds.device)]), torch.cat([g, seeds])
    order = torch.argsort(t, stable=True)
    t, g = t[order], g[order]
    is_seed = torch.isin(g, seeds)
    others = torch.unique(g[~is_seed])
    src_ids = torch.cat([seeds, others])
    sorted_ids, perm = torch.sort(src_ids)
    local = perm[torch.searchsorted(sorted_ids, g)]
    return src_ids, local, t


def timed(fn, steps, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return dict(median_us=float(np.median(out)), min_us=float(min(out)), max_us=float(max(out)))


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(1 for e in prof.events() if e.device_type.name != "CPU" and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--num_neighbors", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fixed", action="store_true", help="the fixed-capacity / graphed columns instead of the eager breakdown")
    a = ap.parse_args()
    from allset_amd import han_sampling as hs, ops
    import han_sampling_oracle as orc
    k = a.num_neighbors
    results = []
    for dname, (pairs, n_v, n_e, x, y, n_cls) in datasets().items():
        data = SimpleNamespace(edge_index=pairs.to(DEV), n_x=[n_v], num_hyperedges=[n_e])
        walker = hs.MetapathWalker(data)
        feats = torch.cat([x, torch.zeros(n_e, x.shape[1])]).to(DEV)
        labels = y.to(DEV)
        as64 = lambda csr: (csr.rowptr.long(), csr.col.long())
        v2e64, e2v64 = as64(walker.v2e), as64(walker.e2v)
        v2e_l, e2v_l = orc.adjacency(pairs.numpy(), n_v, n_e)
        for B in (32, 1024):
            torch.manual_seed(0)
            model = hs.HAN(2, feats.shape[1], 8, n_cls, [8], 0.6).to(DEV).train()
            opt = torch.optim.Adam(model.parameters(), lr=0.001, weight_decay=0.001)
            loss_fn = torch.nn.CrossEntropyLoss()
            sampler = hs.HANSampler(walker, hs.DEFAULT_METAPATHS, k, seed=1)
            ids = torch.randperm(n_v)[:B].to(DEV)
            s32 = ids.to(torch.int32)
            gen = torch.Generator(device=DEV).manual_seed(0)
            rng = np.random.default_rng(0)
            state = {}

            def walk_only():
                for mp in (0, 1):
                    A, Bc, base = walker.orientation(mp)
                    ops.han_walk(mp, A, Bc, base, s32, k, 1, 0)

            def sample():
                state["blocks"] = sampler.sample_blocks(ids)[1]

            def torch_sampler():
                for mp in (0, 1):
                    torch_sample(v2e64, e2v64, n_v, mp, ids, k, gen)

            def numpy_sampler():
                seeds = ids.cpu().numpy()
                for mp in (0, 1):
                    orc.to_block(orc.neighbour_rows(v2e_l, e2v_l, n_v, mp, seeds, k, rng), seeds)

            def forward():
                blocks = state["blocks"]
                state["loss"] = loss_fn(model(blocks, hs.load_subtensors(blocks, feats)), labels[ids])

            def fwd_bwd():
                forward()
                opt.zero_grad()
                state["loss"].backward()
                opt.step()

            def step():
                sample()
                fwd_bwd()

            if a.fixed:
                from allset_amd.optim import FusedAdam

                def sample_fixed():
                    state["fixed"] = sampler.sample_blocks_fixed(ids)[1]

                torch.manual_seed(0)
                model_f = hs.HAN(2, feats.shape[1], 8, n_cls, [8], 0.6).to(DEV).train()
                opt_f = FusedAdam(model_f.parameters(), lr=0.001, weight_decay=0.001)

                def step_fixed():
                    sample_fixed()
                    blocks = state["fixed"]
                    loss = loss_fn(model_f(blocks, hs.load_subtensors(blocks, feats)), labels[ids])
                    opt_f.zero_grad()
                    loss.backward()
                    opt_f.step()

                torch.manual_seed(0)
                model_g = hs.HAN(2, feats.shape[1], 8, n_cls, [8], 0.6).to(DEV).train()
                opt_g = FusedAdam(model_g.parameters(), lr=0.001, weight_decay=0.001)
                graphed = hs.GraphedSampledStep(model_g, hs.HANSampler(walker, hs.DEFAULT_METAPATHS, k, seed=1), feats, labels, loss_fn,
                                                opt_g, B)
                step(), step_fixed(), graphed.step(ids)
                r = dict(dataset=dname, batch_size=B, num_neighbors=k, capacity=hs.FixedBlock.capacity(B, k),
                         n_src=[b.n_src for b in state["blocks"]], nnz=[b.nnz for b in state["blocks"]])
                r["step_eager"] = timed(step, a.steps, a.repeats)                     # the yardstick: the step as it was
                r["sampler_hip"] = timed(sample, a.steps, a.repeats)
                r["sampler_fixed"] = timed(sample_fixed, a.steps, a.repeats)
                r["step_fixed_eager"] = timed(step_fixed, a.steps, a.repeats)
                r["step_graphed"] = timed(lambda: graphed.step(ids), a.steps, a.repeats)
                r["launches"] = dict(sampler=count_launches(sample), sampler_fixed=count_launches(sample_fixed),
                                     step=count_launches(step), step_fixed_eager=count_launches(step_fixed))
                results.append(r)
                print(json.dumps(r), flush=True)
                continue
            sample()
            r = dict(dataset=dname, batch_size=B, num_neighbors=k, n_src=[b.n_src for b in state["blocks"]],
                     nnz=[b.nnz for b in state["blocks"]])
            r["walk_kernels"] = timed(walk_only, a.steps, a.repeats)
            r["sampler_hip"] = timed(sample, a.steps, a.repeats)
            r["sampler_torch_ops"] = timed(torch_sampler, a.steps, a.repeats)
            t0 = time.perf_counter()
            numpy_sampler()
            r["sampler_numpy_cpu_us"] = (time.perf_counter() - t0) * 1e6
            r["forward"] = timed(forward, a.steps, a.repeats)
            r["forward_backward_adam"] = timed(fwd_bwd, a.steps, a.repeats)
            r["step"] = timed(step, a.steps, a.repeats)
            r["launches"] = dict(sampler=count_launches(sample), sampler_torch_ops=count_launches(torch_sampler), forward=count_launches(forward),
                                 forward_backward_adam=count_launches(fwd_bwd), step=count_launches(step))
            results.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
