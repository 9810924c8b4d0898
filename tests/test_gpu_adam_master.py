"""GPU: mixed-precision training -- ``FusedAdam(master_weights=True)`` through ``adam_master_kernel`` (csrc/optim.hip) and the driver's
``--dtype bf16``.  One step from a prepared state is held to the project's fp32 Adam bound (``bf16_dense_cases.adam_within``, float64
reference) on the master and both moments, and the bf16 model copy must be the master's rounding bit for bit; updates below half a
bf16 spacing accumulate; a captured step replays bit-identically to eager steps; the driver trains, measured against its own fp32
run in the same test.  tests/test_adam_master_host.py covers the torch slow path and the state-dict round trip."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_dense_cases as dc  # noqa: E402
import cases  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _bits16(t):
    return t.detach().view(torch.int16)


def _is_rounded_master(p, master):
    return torch.equal(_bits16(p), _bits16(master.to(BF16)))


# ---- one step from a prepared state -------------------------------------------------------------------------------------------------------
def _prepared(n, what):
    """``adam_state``'s fp32 tables with the gradient rounded to bf16 (what a bf16 model hands over) and its cancellation guard
    re-applied to the rounded value."""
    p, g, m, v = dc.adam_state(n, False, what)
    g = dc.bf16_round(g)
    wd_max = max(dc.ADAM_WD)
    g = torch.where((g + wd_max * p).abs() < 0.5 * (wd_max * p).abs(), -g, g)
    return p, g, m, v


@pytest.mark.parametrize("wd", dc.ADAM_WD)
@pytest.mark.parametrize("pre", dc.ADAM_PRE_STEPS)
def test_master_step_from_a_prepared_state(pre, wd, device):
    """Sizes on both sides of the 2048-element chunk, a zero-element parameter between two others, one live parameter more than a
    pointer table holds, one parameter without a gradient; the float64 restatement of csrc/optim.hip's header and the fp32 bounds
    of ``adam_within`` (the kernel keeps ``adam_kernel``'s operation order, the gradient is exact in fp32)."""
    from allset_amd import _lib
    from allset_amd.optim import FusedAdam
    cap = int(_lib.load().allset_adam_max_tensors())
    sizes = dc.adam_sizes(cap)
    assert len(sizes) == cap + 1 and 0 in sizes
    host, params = [], []
    for k, n in enumerate(sizes):
        p, g, m, v = _prepared(n, f"master-{k}")
        host.append((p, g, m, v))
        P = torch.nn.Parameter(p.float().to(BF16).to(device))
        assert torch.equal(g.to(BF16).double(), g)
        P.grad = g.to(BF16).to(device)
        params.append(P)
    idle = torch.nn.Parameter(dc.adam_state(5, True, "idle")[0].to(BF16).to(device))
    idle_before = idle.detach().clone()
    opt = FusedAdam(params + [idle], weight_decay=wd, master_weights=True, **dc.ADAM_HYPER)
    for P, (p, g, m, v) in zip(params, host):
        opt.state[P] = dict(step=torch.tensor(float(pre), dtype=torch.float32, device=device), master=p.float().to(device),
                            exp_avg=m.float().to(device), exp_avg_sq=v.float().to(device))
    assert len(opt.step_counters()) == len(params)
    opt.step()
    for k, (P, (p, g, m, v)) in enumerate(zip(params, host)):
        st = opt.state[P]
        what = f"adam master t{pre + 1} wd{wd} tensor {k} ({sizes[k]})"
        assert float(st["step"]) == pre + 1
        assert all(st[key].dtype == torch.float32 for key in ("master", "exp_avg", "exp_avg_sq")) and P.dtype == BF16
        ref = dc.adam_reference(p, g, m, v, pre + 1, wd=wd, **dc.ADAM_HYPER)
        dc.assert_adam(st["exp_avg"], ref, "m", False, what)
        dc.assert_adam(st["exp_avg_sq"], ref, "v", False, what)
        dc.assert_adam(st["master"], ref, "p", False, what)
        assert _is_rounded_master(P, st["master"]), what
    assert torch.equal(idle.detach(), idle_before) and len(opt.state[idle]) == 0


# ---- updates below half a bf16 spacing ----------------------------------------------------------------------------------------------------
def test_updates_below_half_a_bf16_spacing_accumulate_through_the_kernel(device):
    """tests/test_adam_master_host.py's first test on the device: constant gradient 1, lr = 2^-12, 64 steps from 1.0.  The master
    arrives at 1 - 64 * 2^-12 = 0.984375; the default bf16 form (``adam_kernel<uint16_t>``) rounds every update away."""
    from allset_amd.optim import FusedAdam

    def run(master_weights):
        p = torch.nn.Parameter(torch.ones(8, dtype=BF16, device=device))
        opt = FusedAdam([p], lr=2.0 ** -12, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, master_weights=master_weights)
        for _ in range(64):
            p.grad = torch.ones(8, dtype=BF16, device=device)
            opt.step()
        return p, opt
    p, opt = run(True)
    master = opt.state[p]["master"]
    print(f"master after 64 steps: {master.tolist()}")
    assert master.dtype == torch.float32 and float(opt.state[p]["step"]) == 64.0
    assert float((master - 0.984375).abs().max()) <= 1e-5
    assert float((p.detach().float() - 0.984375).abs().max()) <= 2.0 ** -8
    assert _is_rounded_master(p, master)
    q, opt_q = run(False)
    assert "master" not in opt_q.state[q]
    assert torch.equal(q.detach(), torch.ones(8, dtype=BF16, device=device))


# ---- a captured step ------------------------------------------------------------------------------------------------------------------------
def _setup(name, device):
    from allset_amd import SetGNN
    case = cases.build_case(name)
    args = case["args"]
    args.dropout = 0.0
    torch.manual_seed(0)
    model = SetGNN(args).to(device)
    model.reset_parameters()
    model = model.to(BF16)
    data = SimpleNamespace(x=torch.from_numpy(case["x"]).to(device).to(BF16),
                           edge_index=torch.from_numpy(case["edge_index"]).to(device),
                           norm=torch.from_numpy(case["norm"]).to(device))
    y = torch.randint(0, args.num_classes, (data.x.shape[0],), generator=torch.Generator().manual_seed(1)).to(device)
    return model, data, y


@pytest.mark.parametrize("name", ["citeseer_pma_h4", "wide256_ds_add"])
def test_graphed_train_step_with_masters_matches_eager(name, device):
    """tests/test_gpu_graphs.py ``test_graphed_train_step_matches_eager_without_dropout`` for a bf16 model trained through masters:
    warm-up and restore leave masters, parameters and counters at the start; 4 replays equal 4 eager steps bit for bit."""
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model_a, data_a, y = _setup(name, device)
    model_b, data_b, _ = _setup(name, device)
    model_b.load_state_dict(model_a.state_dict())
    opt_a = FusedAdam(model_a.parameters(), lr=1e-2, master_weights=True)
    opt_b = FusedAdam(model_b.parameters(), lr=1e-2, master_weights=True)
    loss_fn = lambda out: F.nll_loss(F.log_softmax(out.float(), dim=1), y)
    start = [p.detach().clone() for p in model_a.parameters()]

    def eager():
        model_b.eval()
        opt_b.zero_grad(set_to_none=True)
        loss = loss_fn(model_b(data_b))
        loss.backward()
        opt_b.step()
        return loss

    step = GraphedTrainStep(model_a, data_a, loss_fn, opt_a, warmup=3, train_mode=False)
    stepped = [p for p in model_a.parameters() if "master" in opt_a.state.get(p, {})]
    assert stepped
    for pa, p0 in zip(model_a.parameters(), start):
        assert pa.dtype == BF16 and torch.equal(_bits16(pa), _bits16(p0))
        st = opt_a.state.get(pa, {})
        if st:
            # the pre-capture master of a parameter is the parameter as fp32: the state is created at its first step
            assert st["master"].dtype == torch.float32 and torch.equal(st["master"], p0.float())
            assert _is_rounded_master(pa, st["master"])
            assert float(st["step"]) == 0.0
            assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
    model_b.load_state_dict(model_a.state_dict())
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    for i in range(4):
        la = step().clone()
        lb = eager()
        assert torch.equal(la.detach(), lb.detach()), (i, float(la.detach()), float(lb.detach()))
    for (k, pa), pb in zip(model_a.named_parameters(), model_b.parameters()):
        assert torch.equal(_bits16(pa), _bits16(pb)), k
        sa, sb = opt_a.state.get(pa, {}), opt_b.state.get(pb, {})
        assert bool(sa) == bool(sb), k
        if sa:
            assert torch.equal(sa["master"].view(torch.int32), sb["master"].view(torch.int32)), k
            assert _is_rounded_master(pa, sa["master"]), k
            assert float(sa["step"]) == 4.0 and float(sb["step"]) == 4.0
    assert any(not torch.equal(pa, p0) for pa, p0 in zip(model_a.parameters(), start))


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------
DRIVER = ["--method", "AllSetTransformer", "--heads", "4", "--MLP_hidden", "128", "--All_num_layers", "1", "--dname", "synthetic",
          "--seed", "7", "--dropout", "0.2"]


def _drive(monkeypatch, tmp_path, extra):
    """``train.run`` in this process, with the optimizers it made (the last run's is looked at)."""
    from allset_amd import train
    made = []
    make = train.make_optimizer

    def recording(args, model):
        opt = make(args, model)
        made.append((model, opt))
        return opt
    monkeypatch.setattr(train, "make_optimizer", recording)
    res = train.run(train.parse_args(DRIVER + ["--res_root", str(tmp_path)] + extra))
    return res, made[-1]


def test_train_driver_bf16_against_its_fp32_run(monkeypatch, tmp_path, device):
    """``--dtype bf16`` against ``--dtype fp32`` (the yardstick: the driver as it was), same seed, same splits, 3 runs of 60 epochs,
    captured steps.  bf16 must train (the project's criterion of tests/test_gpu_graphs.py: the mean loss of the last 3 epochs below
    0.7 x the first 3) and reach, per run, the fp32 run's best validation accuracy minus ``margin`` = the spread of the three fp32
    values + one validation vertex.  Then 10 eager epochs (``--hip_graph 0``: ``deferred_param_grads`` outside a graph)."""
    common = ["--epochs", "60", "--runs", "3", "--hip_graph", "1"]
    res32, (model32, _) = _drive(monkeypatch, tmp_path, common + ["--dtype", "fp32"])
    res16, (model16, opt16) = _drive(monkeypatch, tmp_path, common + ["--dtype", "bf16"])
    assert all(p.dtype == torch.float32 for p in model32.parameters())
    assert all(p.dtype == BF16 for p in model16.parameters())
    masters = [opt16.state[p] for p in model16.parameters() if p in opt16.state and opt16.state[p]]
    assert masters and all(st["master"].dtype == torch.float32 and st["exp_avg"].dtype == torch.float32
                           and st["exp_avg_sq"].dtype == torch.float32 for st in masters)
    for p in model16.parameters():
        if opt16.state.get(p):
            assert _is_rounded_master(p, opt16.state[p]["master"])
    v32, v16 = [float(v) for v in res32["best_val"]], [float(v) for v in res16["best_val"]]
    t32, t16 = [float(v) for v in res32["best_test"]], [float(v) for v in res16["best_test"]]
    n_valid = int(4000 * 0.25)                              # synthetic_dataset's 4000 vertices, --valid_prop 0.25
    margin = (max(v32) - min(v32)) + 100.0 / n_valid
    print(f"best_val fp32 {v32} bf16 {v16}; best_test fp32 {t32} bf16 {t16}; margin {margin:.3f}")
    loss = np.asarray(res16["train_loss"], dtype=np.float64)
    assert loss.shape == (3, 60) and np.asarray(res32["train_loss"]).shape == (3, 60)
    assert np.isfinite(loss).all() and np.isfinite(v16).all() and np.isfinite(t16).all()
    for r in range(3):
        first, last = loss[r, :3].mean(), loss[r, -3:].mean()
        print(f"run {r}: bf16 train loss first 3 {first:.4f} last 3 {last:.4f}; fp32 "
              f"{np.mean(res32['train_loss'][r][:3]):.4f} -> {np.mean(res32['train_loss'][r][-3:]):.4f}")
        assert last < 0.7 * first, (r, first, last)
        assert v16[r] >= v32[r] - margin, (r, v16[r], v32[r], margin)
    res_e, _ = _drive(monkeypatch, tmp_path, ["--epochs", "10", "--runs", "1", "--hip_graph", "0", "--dtype", "bf16"])
    le = np.asarray(res_e["train_loss"], dtype=np.float64)
    print(f"eager bf16 train loss {le.tolist()}")
    assert le.shape == (1, 10) and np.isfinite(le).all()
    assert np.isfinite([float(v) for v in res_e["best_val"]] + [float(v) for v in res_e["best_test"]]).all()
    assert le[0, -1] <= le[0, 0]
