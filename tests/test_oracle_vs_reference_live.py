"""CPU: the oracle against the reference on randomised SetGNN configurations -- the same generator the GPU-side
random-configuration parity test uses, so that chain reads  reference == oracle (here)  and  oracle == product
(tests/test_gpu_random_shapes.py).  Logits, d(loss)/dx and every parameter gradient.

The reference's results are the ones oracle/gen_live_fixtures.py recorded in tests/golden/live_*.npz (the configurations are drawn
there from fixed seeds; the tests rebuild every input).  Where the reference itself is importable (oracle/ref_shim.py) every
configuration is compared with it LIVE as well, on the whole tensors."""
import os
import sys

import numpy as np
import pytest
import torch

import util
from oracle import allset_oracle as oracle
from oracle import gen_live_fixtures as live
from oracle import ref_shim


def _initial_state_dict(args, seed, norm=None):
    """The reference's initial parameters of a configuration: ``torch.manual_seed(seed)`` + ``reset_parameters()``, which
    allset_amd.SetGNN reproduces bit for bit (checked against the recorded checksum of the reference's state_dict)."""
    from allset_amd import SetGNN
    torch.manual_seed(seed)
    model = SetGNN(args, norm=norm)
    model.reset_parameters()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, [k for k, _ in model.named_parameters()]


def _param_grads_match(sdict, names, ref, prefix, rtol, atol_rel):
    for kk in names:
        e = ref[prefix + "grad:" + kk]
        g = sdict[kk].grad
        if e["kind"] == "none" or g is None:
            assert (e["kind"] == "none" or e["max"] == 0.0) and (g is None or float(g.abs().max()) == 0.0), kk
            continue
        util.assert_matches_entry(g, e, kk, rtol=rtol, atol=atol_rel * max(1.0, e["max"]))


def _sources(record_name, run_live):
    """(label, {key: entry}) per source: the recorded reference, and the live one where it can be imported."""
    yield "recorded", live.load_table(record_name)
    if ref_shim.available():
        yield "live", run_live()


def test_oracle_equals_live_reference_on_random_configurations():
    configs = live.random_configs()
    chk = np.load(os.path.join(util.GOLDEN, "live_random_configs.npz"))["chk"]
    assert len(chk) == len(configs) == live.N_RANDOM

    def run_live():
        out = {}
        for i, c in enumerate(configs):
            res = live.reference_random_config(c)
            assert res["chk"] == chk[i], (i, "the live reference's initial parameters differ from the recorded ones")
            out[f"c{i}/logits"], out[f"c{i}/grad_x"] = live.entry(res["logits"]), live.entry(res["grad_x"])
            out.update({f"c{i}/grad:{k}": live.entry(g) for k, g in res["grads"].items()})
        return out

    for label, ref in _sources("live_random_configs", run_live):
        for i, c in enumerate(configs):
            args, ei, x, nrm, rng = live.random_config_inputs(c)
            norm_t = torch.from_numpy(nrm)
            sdict, names = _initial_state_dict(args, c["sd"], norm_t.to(torch.float32) if c["mask"] else None)
            assert live.state_dict_checksum(sdict) == chk[i], (i, c)
            for kk, v in sdict.items():
                if v.is_floating_point() and "running" not in kk:
                    v.requires_grad_(True)
            xo = torch.from_numpy(x).clone().requires_grad_(True)
            out = oracle.setgnn_forward(sdict, args, xo, torch.from_numpy(ei), norm_t)
            G = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32))
            (out * G).sum().backward()
            p = f"c{i}/"
            # fp32 on both sides: against a recording made on another host (another BLAS / thread count / vector ISA) the logits get
            # tests/test_oracle_golden.py's cross-host tolerance, 2e-5 of their scale; the live comparison keeps 1e-5
            tol = (1e-5, 1e-5) if label == "live" else (2e-5, 2e-5 * max(1.0, ref[p + "logits"]["max"]))
            util.assert_matches_entry(out.detach(), ref[p + "logits"], f"{label} c{i} logits", rtol=tol[0], atol=tol[1])
            util.assert_matches_entry(xo.grad, ref[p + "grad_x"], f"{label} c{i} grad_x", rtol=1e-4,
                                      atol=1e-5 * max(1.0, ref[p + "grad_x"]["max"]))
            _param_grads_match(sdict, names, ref, p, rtol=1e-4, atol_rel=1e-5)


def test_oracle_training_mode_with_explicit_masks_equals_live_reference():
    """The explicit-mask training mode of the oracle (``setgnn_forward(..., drop=ExplicitDropout(masks))``) against the
    reference in ``.train()`` mode with the dropout masks torch drew there: same dropout sites in the same order (every recorded
    mask is consumed, shapes agree), same logits and gradients.  Both sides run in float64 (dropout in front of stacked LayerNorms
    over 16 columns amplifies fp32 rounding differences between the two implementations to ~3e-5; in float64 the comparison is
    about semantics).  This pins the oracle that tests/test_gpu_train_parity.py checks the product's training step against."""
    configs = live.training_configs()
    chk = np.load(os.path.join(util.GOLDEN, "live_training_masks.npz"))["chk"]
    assert len(chk) == len(configs) == live.N_TRAINING

    def run_live():
        out = {}
        for i, c in enumerate(configs):
            res = live.reference_training_config(c)
            assert res["chk"] == chk[i], (i, "the live reference's initial parameters differ from the recorded ones")
            out[f"c{i}/logits"], out[f"c{i}/grad_x"] = live.entry(res["logits"]), live.entry(res["grad_x"])
            out.update({f"c{i}/grad:{k}": live.entry(g) for k, g in res["grads"].items()})
            out.update({f"c{i}/mask{j}": live.entry(m) for j, m in enumerate(res["masks"])})
        return out

    for label, ref in _sources("live_training_masks", run_live):
        for i, c in enumerate(configs):
            args, ei, x, norm_np, rng = live.training_config_inputs(c)
            sd0, names = _initial_state_dict(args, c["sd"])
            assert live.state_dict_checksum(sd0) == chk[i], (i, c)
            sdict = {kk: (v.double() if v.is_floating_point() else v) for kk, v in sd0.items()}
            for kk, v in sdict.items():
                if v.is_floating_point() and "running" not in kk:
                    v.requires_grad_(True)
            p = f"c{i}/"
            masks = []
            while f"{p}mask{len(masks)}" in ref:
                masks.append(torch.from_numpy(np.asarray(ref[f"{p}mask{len(masks)}"]["value"])))
            xo = torch.from_numpy(x).double().requires_grad_(True)
            drop = oracle.ExplicitDropout(masks)
            out = oracle.setgnn_forward(sdict, args, xo, torch.from_numpy(ei), torch.from_numpy(norm_np), drop=drop)
            assert drop.used == len(masks) and len(masks) >= 2, (label, i, drop.used, len(masks))
            G = torch.from_numpy(rng.standard_normal(tuple(out.shape)))
            (out * G).sum().backward()
            util.assert_matches_entry(out.detach(), ref[p + "logits"], f"{label} c{i} logits", rtol=1e-9, atol=1e-9)
            util.assert_matches_entry(xo.grad, ref[p + "grad_x"], f"{label} c{i} grad_x", rtol=1e-8,
                                      atol=1e-9 * max(1.0, ref[p + "grad_x"]["max"]))
            _param_grads_match(sdict, names, ref, p, rtol=1e-8, atol_rel=1e-9)


@pytest.mark.parametrize("name", ["rand50_ds_add", "rand50_pma_h4", "rand50_ds_mean_wnorm", "rand50_ds_add_L2_gpr"])
def test_oracle_training_trajectory_equals_live_reference(name):
    """Ten Adam steps of the reference's training loop body (train.py:470-476: forward, nll_loss(log_softmax) on the train split,
    backward, step) on the reference model and on the oracle, both float64, dropouts off (eval-mode forward): the loss
    sequence and the final parameters agree to rounding.  The GPU side of the chain is tests/test_gpu_train_trajectory.py."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_train_trajectory import trajectory_oracle
    assert name in live.TRAJECTORY_CASES
    case, y, train_idx = live.trajectory_inputs(name)
    args = case["args"]
    norm_t = torch.from_numpy(case["norm"])
    sd, names = _initial_state_dict(args, case["seed"], norm_t.to(torch.float32) if args.LearnMask else None)
    chk = np.load(os.path.join(util.GOLDEN, "live_trajectories.npz"))["chk"][live.TRAJECTORY_CASES.index(name)]
    assert live.state_dict_checksum(sd) == chk
    ref_losses, ref_params = trajectory_oracle(case, sd, y, train_idx, 10, 0.01)

    sources = [("recorded", live.load_table("live_trajectories"))]
    if ref_shim.available():
        res = live.reference_trajectory(name)
        assert res["chk"] == chk, "the live reference's initial parameters differ from the recorded ones"
        sources.append(("live", {f"{name}/losses": live.entry(torch.from_numpy(res["losses"])),
                                 **{f"{name}/param:{k}": live.entry(p) for k, p in res["params"].items()}}))
    for label, ref in sources:
        np.testing.assert_allclose(ref_losses, ref[f"{name}/losses"]["value"], rtol=1e-9, atol=1e-11, err_msg=label)
        for k in names:
            util.assert_matches_entry(ref_params[k].detach(), ref[f"{name}/param:{k}"], f"{label} {k}", rtol=1e-7, atol=1e-9)
