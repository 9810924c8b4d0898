#!/usr/bin/env python
"""Record what the REAL reference computes on the configurations of the live-comparison tests, so that those tests run
where the reference cannot be imported.  TEST INFRASTRUCTURE.

Container-only (needs the reference through ``oracle/ref_shim.py``).  Usage:  ``python oracle/gen_live_fixtures.py``
-> rewrites ``tests/golden/live_*.npz``:

* ``live_random_configs.npz``    random SetGNN configurations, eval mode: logits, d(loss)/dx, every parameter gradient
                                 (tests/test_oracle_vs_reference_live.py::test_oracle_equals_live_reference_on_random_configurations)
* ``live_training_masks.npz``    random configurations in ``.train()`` mode, float64: the dropout masks torch drew, logits,
                                 d(loss)/dx, every parameter gradient (...::test_oracle_training_mode_with_explicit_masks_equals_live_reference)
* ``live_trajectories.npz``      ten Adam steps of the reference's training-loop body: losses and final parameters
                                 (...::test_oracle_training_trajectory_equals_live_reference)
* ``live_golden_logits.npz``     eval logits of three golden cases (tests/test_oracle_golden.py::test_oracle_matches_live_reference_when_present)
* ``live_preprocessing.npz``     the reference's preprocessing chain on random block edge lists
                                 (tests/test_preprocessing_vs_reference_live.py)

The configurations are drawn here from fixed seeds (``random_configs`` & co.); the tests rebuild every input from them.  The
initial parameters are not stored: the reference draws them with ``torch.manual_seed(sd)`` + ``reset_parameters()``, which
``allset_amd.SetGNN`` reproduces bit for bit -- each entry stores a checksum of the reference's state_dict that the tests check.
Logits, input gradients, losses, masks and every tensor of up to ``FULL_NUMEL`` entries are stored whole; larger ones (the
weight matrices) as a fixed seeded sample of ``SAMPLE`` entries plus their sum, absolute sum, max-abs and size.  Where the reference IS importable the tests
also compare against it live, on the whole tensors.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cases  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL_NUMEL = 256
SAMPLE = 64
N_RANDOM, N_TRAINING, N_PREPROC = 25, 25, 40
TRAJECTORY_CASES = ("rand50_ds_add", "rand50_pma_h4", "rand50_ds_mean_wnorm", "rand50_ds_add_L2_gpr")
GOLDEN_LOGIT_CASES = ("rand50_pma_h4", "edge_ds_max", "rand50_ds_mean_wnorm")


# ---------------------------------------------------------------------------------------------------------------------
# the configurations (stratified over the categorical choices, the rest drawn)
# ---------------------------------------------------------------------------------------------------------------------

def random_configs():
    rng = np.random.default_rng(20261016)
    out = []
    for i in range(N_RANDOM):
        out.append(dict(pma=bool(i % 2), layers=int(rng.integers(1, 4)), mlp_layers=int(rng.integers(1, 4)),
                        hidden=(16, 64, 256)[i % 3], heads=int(rng.choice([1, 2, 4])), aggr=("add", "mean", "max")[(i // 2) % 3],
                        norm=("ln", "bn", "None")[(i // 3) % 3], input_norm=bool(rng.integers(2)), mask=bool(rng.integers(2)),
                        gpr=bool(rng.integers(2)), wnorm=bool(rng.integers(2)), sd=int(rng.integers(0, 10 ** 6))))
    return out


def training_configs():
    rng = np.random.default_rng(20261017)
    out = []
    for i in range(N_TRAINING):
        out.append(dict(pma=bool(i % 2), layers=int(rng.integers(1, 3)), mlp_layers=int(rng.integers(1, 4)),
                        hidden=(16, 64)[(i // 2) % 2], heads=int(rng.choice([1, 4])), aggr=("add", "mean", "max")[i % 3],
                        norm=("ln", "None")[(i // 3) % 2], gpr=bool(rng.integers(2)), p=(0.5, 0.2)[(i // 4) % 2],
                        sd=int(rng.integers(0, 10 ** 6))))
    return out


def preproc_configs():
    rng = np.random.default_rng(20261018)
    return [dict(n_v=int(rng.integers(3, 61)), n_e=int(rng.integers(1, 31)), extra=int(rng.integers(0, 151)),
                 singles=int(rng.integers(0, 9)), sd=int(rng.integers(0, 10 ** 6))) for _ in range(N_PREPROC)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs of one configuration (the tests call these too)
# ---------------------------------------------------------------------------------------------------------------------

def random_config_inputs(c):
    """(args, edge_index, x, norm, rng) of a random configuration; ``rng`` is left where the cotangent is drawn."""
    rng = np.random.default_rng(c["sd"])
    n_v, n_e, f, k = 40, 17, 12, 5
    ei = cases.random_hypergraph(rng, n_v, n_e, 150, True)
    x = rng.standard_normal((n_v, f)).astype(np.float32)
    args = cases.make_args("pma_h1" if c["pma"] else "ds_add", f, c["hidden"], k, All_num_layers=c["layers"],
                           MLP_num_layers=c["mlp_layers"], heads=c["heads"] if c["pma"] else 1,
                           aggregate=c["aggr"] if not c["pma"] else "add", normalization=c["norm"],
                           deepset_input_norm=c["input_norm"], LearnMask=c["mask"], GPR=c["gpr"], Classifier_num_layers=2)
    nrm = cases._norm_deg_half_sym(ei) if (c["wnorm"] or c["mask"]) else np.ones(ei.shape[1], dtype=np.int64)
    return args, ei, x, nrm, rng


def training_config_inputs(c):
    rng = np.random.default_rng(c["sd"])
    n_v, n_e, f, k = 40, 17, 12, 5
    ei = cases.random_hypergraph(rng, n_v, n_e, 150, True)
    x = rng.standard_normal((n_v, f)).astype(np.float32)
    args = cases.make_args("pma_h1" if c["pma"] else "ds_add", f, c["hidden"], k, All_num_layers=c["layers"],
                           MLP_num_layers=c["mlp_layers"], heads=c["heads"] if c["pma"] else 1,
                           aggregate=c["aggr"] if not c["pma"] else "add", normalization=c["norm"], GPR=c["gpr"],
                           Classifier_num_layers=2, dropout=c["p"])
    return args, ei, x, np.ones(ei.shape[1], dtype=np.int64), rng


def trajectory_inputs(name):
    """(case, y, train_idx) of a trajectory case: labels and the train split as the test draws them."""
    case = cases.build_case(name)
    n = case["x"].shape[0]
    rng = np.random.default_rng(case["seed"])
    y = torch.from_numpy(rng.integers(0, case["args"].num_classes, size=n))
    train_idx = torch.from_numpy(np.sort(rng.choice(n, size=max(n // 2, 4), replace=False)))
    return case, y, train_idx


def preproc_block(c):
    """The bidirectional block edge list of a preprocessing configuration (every hyperedge gets a member; ``singles`` of them stay
    size-1, each owned by a distinct vertex -- the reference's Add_Self_Loops indexes out of bounds otherwise,
    preprocessing.py:428-440; the last vertex id is present)."""
    n_v, n_e = c["n_v"], c["n_e"]
    rng = np.random.default_rng(c["sd"])
    singles = min(c["singles"], n_e, n_v - 1)
    owners = rng.permutation(n_v - 1)[:singles]
    pairs = {(int(owners[e]), e) for e in range(singles)}
    for e in range(singles, n_e):                      # every other hyperedge has at least two distinct members
        a = int(rng.integers(n_v))
        pairs.add((a, e))
        pairs.add(((a + 1 + int(rng.integers(n_v - 1))) % n_v, e))
    if singles < n_e:
        pairs.add((n_v - 1, n_e - 1))
    for _ in range(c["extra"]):
        if singles < n_e:
            pairs.add((int(rng.integers(n_v)), int(rng.integers(singles, n_e))))
    pairs = sorted(pairs)
    v = np.array([p[0] for p in pairs], dtype=np.int64)
    e = np.array([p[1] for p in pairs], dtype=np.int64) + n_v
    block = np.concatenate([np.stack([v, e]), np.stack([e, v])], axis=1)
    return block[:, rng.permutation(block.shape[1])]


def canon(ei) -> np.ndarray:
    a = ei.cpu().numpy() if torch.is_tensor(ei) else np.asarray(ei)
    return a[:, np.lexsort((a[1], a[0]))]


def state_dict_checksum(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------------
# the reference's side
# ---------------------------------------------------------------------------------------------------------------------

def reference_random_config(c):
    """Eval-mode forward + backward of the reference on a random configuration: logits, d/dx, {name: grad or None}, checksum."""
    _, ref_models = ref_shim.import_reference()
    args, ei, x, nrm, rng = random_config_inputs(c)
    norm_t = torch.from_numpy(nrm)
    torch.manual_seed(c["sd"])
    model = ref_models.SetGNN(args, norm=norm_t.to(torch.float32) if c["mask"] else None)
    model.reset_parameters()
    model.eval()
    chk = state_dict_checksum(model.state_dict())
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    ref = model(SimpleNamespace(x=xr, edge_index=torch.from_numpy(ei).clone(), norm=norm_t))
    G = torch.from_numpy(rng.standard_normal(tuple(ref.shape)).astype(np.float32))
    (ref * G).sum().backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return dict(logits=ref.detach(), grad_x=xr.grad.detach(), grads=grads, chk=chk)


class RecordDropout:
    """Wraps torch's own ``F.dropout`` while the reference runs in training mode: calls the real function and reads the keep mask
    off its output (``out != 0``; where the input itself is 0 -- behind a relu -- the mask is immaterial for the value and the
    gradient is cut by the relu, so those positions count as kept)."""

    def __init__(self):
        import torch.nn.functional as F
        self.F, self.orig, self.masks = F, F.dropout, []

    def __enter__(self):
        def dropout(x, p=0.5, training=True, inplace=False):
            out = self.orig(x, p=p, training=training, inplace=False)
            if training and p > 0.0:
                self.masks.append(((out != 0) | (x == 0)).detach().clone())
            return out
        self.F.dropout = dropout
        return self

    def __exit__(self, *exc):
        self.F.dropout = self.orig
        return False


def reference_training_config(c):
    """``.train()``-mode forward + backward of the reference in float64 with torch's dropout masks recorded."""
    _, ref_models = ref_shim.import_reference()
    args, ei, x, norm_np, rng = training_config_inputs(c)
    torch.manual_seed(c["sd"])
    model = ref_models.SetGNN(args)
    model.reset_parameters()
    chk = state_dict_checksum(model.state_dict())
    model.double().train()
    xr = torch.from_numpy(x).double().requires_grad_(True)
    with RecordDropout() as rec:
        ref = model(SimpleNamespace(x=xr, edge_index=torch.from_numpy(ei).clone(), norm=torch.from_numpy(norm_np)))
    G = torch.from_numpy(rng.standard_normal(tuple(ref.shape)))
    (ref * G).sum().backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return dict(logits=ref.detach(), grad_x=xr.grad.detach(), grads=grads, chk=chk, masks=rec.masks)


def reference_trajectory(name, steps=10, lr=0.01):
    """Ten Adam steps of the reference's training-loop body (train.py:470-476), float64, dropouts off: losses, final parameters."""
    import torch.nn.functional as F
    _, ref_models = ref_shim.import_reference()
    case, y, train_idx = trajectory_inputs(name)
    args = case["args"]
    torch.manual_seed(case["seed"])
    norm_t = torch.from_numpy(case["norm"])
    model = ref_models.SetGNN(args, norm=norm_t.to(torch.float32) if args.LearnMask else None)
    model.reset_parameters()
    chk = state_dict_checksum(model.state_dict())
    model.double().eval()
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    data = SimpleNamespace(x=torch.from_numpy(case["x"]).double(), edge_index=torch.from_numpy(case["edge_index"]).clone(),
                           norm=norm_t.double() if norm_t.is_floating_point() else norm_t)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        out = model(data)
        loss = F.nll_loss(F.log_softmax(out, dim=1)[train_idx], y[train_idx])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return dict(losses=np.array(losses), params={k: p.detach().clone() for k, p in model.named_parameters()}, chk=chk)


def reference_golden_logits(name):
    import util
    _, ref_models = ref_shim.import_reference()
    case, g = cases.build_case(name), util.load_golden(name)
    model = ref_models.SetGNN(case["args"])
    model.load_state_dict(util.state_dict_for(case, g))
    model.eval()
    with torch.no_grad():
        return model(SimpleNamespace(x=torch.from_numpy(case["x"]), edge_index=torch.from_numpy(case["edge_index"]).clone(),
                                     norm=torch.from_numpy(case["norm"])))


def reference_preprocessing(c):
    """The reference's chain on one block edge list: canonical edge lists after ExtractV2E, Add_Self_Loops (+ totedges), both norm
    constructions over the self-looped list, expand_edge_index at thresholds 0 and 3."""
    ref_pre = ref_shim.import_reference_preprocessing()
    block, n_v, n_e = preproc_block(c), c["n_v"], c["n_e"]
    r = ref_pre.ExtractV2E(SimpleNamespace(edge_index=torch.from_numpy(block).clone(), n_x=[n_v], num_hyperedges=[n_e]))
    out = {"v2e": canon(r.edge_index)}
    r = ref_pre.Add_Self_Loops(r)
    sl = canon(r.edge_index)
    out.update(sl=sl, totedges=np.int64(int(r.totedges)))
    for opt in ("all_one", "deg_half_sym"):
        rn = ref_pre.norm_contruction(SimpleNamespace(edge_index=torch.from_numpy(sl).clone()), option=opt)
        out["norm_" + opt] = rn.norm.numpy()
    for th in (0, 3):
        de = SimpleNamespace(edge_index=torch.from_numpy(sl).clone(), n_x=torch.tensor([n_v]), num_hyperedges=[n_e],
                             totedges=int(r.totedges))
        out[f"expand_{th}"] = canon(ref_pre.expand_edge_index(de, edge_th=th).edge_index)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# storage: whole small tensors, a seeded sample of large ones -- one table per file (a few arrays, not one array per tensor)
# ---------------------------------------------------------------------------------------------------------------------

class Table:
    """Named tensors packed into a few flat arrays.  A tensor of at most FULL_NUMEL entries (or added ``whole``) is kept whole; a larger one as a seeded
    sample of SAMPLE entries (flat indices + values); every entry also stores the whole tensor's sum, absolute sum, max-abs and size;
    ``None`` (a parameter without a gradient) is an entry of its own; bool masks are bit-packed."""

    def __init__(self, dtype=np.float32):
        self.dtype, self.keys, self.kinds, self.shapes, self.stats = dtype, [], [], [], []
        self.vals, self.idx, self.bits = [], [], []

    def add(self, key: str, t, whole: bool = False) -> None:
        self.keys.append(key)
        if t is None:
            self.kinds.append(2); self.shapes.append("[]"); self.stats.append([0.0, 0.0, 0.0, 0.0])
            self.vals.append(np.zeros(0)); self.idx.append(np.zeros(0, np.int32)); self.bits.append(np.zeros(0, np.uint8))
            return
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        self.shapes.append(json.dumps(list(a.shape)))
        if a.dtype == np.bool_:
            self.kinds.append(3); self.stats.append([float(a.sum()), float(a.sum()), 1.0, float(a.size)])
            self.vals.append(np.zeros(0)); self.idx.append(np.zeros(0, np.int32)); self.bits.append(np.packbits(a.reshape(-1)))
            return
        flat = a.astype(np.float64).reshape(-1)
        self.stats.append([flat.sum(), np.abs(flat).sum(), np.abs(flat).max() if flat.size else 0.0, float(flat.size)])
        self.bits.append(np.zeros(0, np.uint8))
        if whole or flat.size <= FULL_NUMEL:
            self.kinds.append(0); self.vals.append(flat); self.idx.append(np.zeros(0, np.int32))
        else:
            rng = np.random.default_rng([zlib.crc32(key.encode()) & 0x7FFFFFFF, 780])
            sel = np.sort(rng.choice(flat.size, size=SAMPLE, replace=False))
            self.kinds.append(1); self.vals.append(flat[sel]); self.idx.append(sel.astype(np.int32))

    def arrays(self) -> dict:
        off = lambda parts: np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)       # noqa: E731
        return {"keys": np.array(self.keys), "kinds": np.array(self.kinds, np.int8), "shapes": np.array(self.shapes),
                "stats": np.array(self.stats, np.float64).reshape(-1, 4),
                "vals": np.concatenate(self.vals).astype(self.dtype), "val_off": off(self.vals),
                "idx": np.concatenate(self.idx).astype(np.int32), "idx_off": off(self.idx),
                "bits": np.concatenate(self.bits).astype(np.uint8), "bit_off": off(self.bits)}


def load_table(name: str) -> dict:
    """tests/golden/<name>.npz written by ``Table`` -> {key: entry}; an entry is a dict with ``kind`` ("full", "sample", "none",
    "mask"), ``shape``, ``sum`` / ``abs`` / ``max`` / ``size`` of the whole tensor, and ``value`` (full: the tensor; mask: the bool
    tensor) or ``idx`` / ``value`` (sample: flat indices and their values)."""
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        t = {k: z[k] for k in z.files}
    out = {}
    for i, key in enumerate(t["keys"]):
        kind = ("full", "sample", "none", "mask")[int(t["kinds"][i])]
        shape = tuple(json.loads(str(t["shapes"][i])))
        s = t["stats"][i]
        e = {"kind": kind, "shape": shape, "sum": float(s[0]), "abs": float(s[1]), "max": float(s[2]), "size": int(s[3])}
        v = t["vals"][t["val_off"][i]:t["val_off"][i + 1]]
        if kind == "full":
            e["value"] = v.reshape(shape)
        elif kind == "sample":
            e["idx"], e["value"] = t["idx"][t["idx_off"][i]:t["idx_off"][i + 1]].astype(np.int64), v
        elif kind == "mask":
            bits = t["bits"][t["bit_off"][i]:t["bit_off"][i + 1]]
            e["value"] = np.unpackbits(bits, count=int(np.prod(shape, dtype=np.int64))).astype(bool).reshape(shape)
        out[str(key)] = e
    return out


def entry(t) -> dict:
    """A whole tensor (or None) in ``load_table``'s entry form: how the tests hold a LIVE reference result beside a recorded one."""
    if t is None:
        return {"kind": "none", "shape": (), "sum": 0.0, "abs": 0.0, "max": 0.0, "size": 0}
    a = t.detach().cpu().numpy()
    f = np.abs(a.astype(np.float64))
    return {"kind": "mask" if a.dtype == np.bool_ else "full", "shape": tuple(a.shape), "value": a, "sum": float(a.astype(np.float64).sum()),
            "abs": float(f.sum()), "max": float(f.max()) if f.size else 0.0, "size": int(a.size)}


def add_result(tab: Table, prefix: str, res: dict) -> None:
    tab.add(prefix + "logits", res["logits"], whole=True)
    tab.add(prefix + "grad_x", res["grad_x"], whole=True)
    for k, g in res["grads"].items():
        tab.add(prefix + "grad:" + k, g)


def main() -> None:
    assert ref_shim.available(), "needs the reference (oracle/ref_shim.py)"
    os.makedirs(GOLDEN, exist_ok=True)
    tab, chk = Table(np.float32), []
    for i, c in enumerate(random_configs()):
        res = reference_random_config(c)
        add_result(tab, f"c{i}/", res)
        chk.append(res["chk"])
    np.savez_compressed(os.path.join(GOLDEN, "live_random_configs.npz"), chk=np.array(chk), **tab.arrays())

    tab, chk = Table(np.float64), []
    for i, c in enumerate(training_configs()):
        res = reference_training_config(c)
        add_result(tab, f"c{i}/", res)
        for j, m in enumerate(res["masks"]):
            tab.add(f"c{i}/mask{j}", m)
        chk.append(res["chk"])
    np.savez_compressed(os.path.join(GOLDEN, "live_training_masks.npz"), chk=np.array(chk), **tab.arrays())

    tab, chk = Table(np.float64), []
    for name in TRAJECTORY_CASES:
        res = reference_trajectory(name)
        tab.add(f"{name}/losses", res["losses"], whole=True)
        for k, p in res["params"].items():
            tab.add(f"{name}/param:{k}", p)
        chk.append(res["chk"])
    np.savez_compressed(os.path.join(GOLDEN, "live_trajectories.npz"), chk=np.array(chk), **tab.arrays())

    np.savez_compressed(os.path.join(GOLDEN, "live_golden_logits.npz"),
                        **{name: reference_golden_logits(name).numpy() for name in GOLDEN_LOGIT_CASES})

    rec = {}
    for i, c in enumerate(preproc_configs()):
        for k, v in reference_preprocessing(c).items():
            rec[f"c{i}/{k}"] = v
    np.savez_compressed(os.path.join(GOLDEN, "live_preprocessing.npz"), **rec)
    for f in sorted(os.listdir(GOLDEN)):
        if f.startswith("live_"):
            print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
