"""GPU: the fused Linear forward that writes packed nonzero rows from its own epilogue (csrc/fused_fwd2.hip mode 3, DESIGN.md section
4.5) against the pair it replaces -- the dense kernel's output and ``ops.pack_rows`` of it -- and the layers that route through it.
Every comparison is an equality of bit patterns."""
import numpy as np
import pytest
import torch

import test_packed_rows_format as fmt
from test_gpu_packed_gather import _assert_same, _bits, _conv, _csr, _hypergraph, _sharded_step, _timed

pytestmark = pytest.mark.gpu

SUM = 0
# 1; a partial four-row group; the 32-row stage boundary; some workgroups take a second stage; every one of the four prefetch register
# sets and the peeled tail ticks
ROWS = (1, 3, 31, 32, 33, 32 * 256 + 1, 32 * 256 * 5 + 7)
TABLES = ("random", "mixed", "empty", "overflow")
P_NEARLY_NONE = {0.5: 1.0 / 256.0, 0.3: 0.01}      # "a dropout so small that nearly every column stays", in the same resolution


def _params(table, p, device):
    """(W, bias, gamma, beta, p_out).  Biases as tests/cases.py kinkfree_biases places them: +-6 against O(1) Linear terms."""
    g = torch.Generator().manual_seed(17)
    W = torch.randn(128, 128, generator=g) / 128 ** 0.5
    gamma = 1.0 + 0.1 * torch.randn(128, generator=g)
    beta = 0.1 * torch.randn(128, generator=g)
    if table == "random":
        bias, p_out = 0.1 * torch.randn(128, generator=g), p
        return [t.to(device) for t in (W, bias, gamma, beta)] + [p_out]
    # the Linear term of a LayerNorm row under dropout p has standard deviation sqrt(1 / (1 - p)) <= 1.5 with W as drawn; a quarter of
    # that leaves the +-6 seventeen standard deviations away: no relu flips among the 5e6 outputs of the largest table
    W = 0.25 * W
    if table == "mixed":                        # every column survives the relu; dropout 0.5 leaves k ~ Bin(128, 1/2) around the cap
        bias, p_out = torch.full((128,), 6.0), 0.5
    elif table == "empty":
        bias, p_out = torch.full((128,), -6.0), p
    else:
        bias, p_out = torch.full((128,), 6.0), P_NEARLY_NONE[p]
    return [t.to(device) for t in (W, bias, gamma, beta)] + [p_out]


_REF = {}


def _pair(table, arith, p, n, device):
    """The parent path (dense kernel + pack_rows) and the packed-mode kernel on the same input under the same seeds; computed once."""
    key = (table, arith, p, n)
    if key not in _REF:
        from allset_amd import dense, ops
        W, bias, gamma, beta, p_out = _params(table, p, device)
        x = torch.randn(n, 128, generator=torch.Generator().manual_seed(n)).to(device)
        words = dense.activation_mask_words(n, 128)
        m_ref = torch.zeros(words, dtype=torch.int32, device=device)
        m_new = torch.zeros(words, dtype=torch.int32, device=device)
        with dense.arithmetic(arith):
            y, stats = dense.fused_linear_fwd(x, W, bias, gamma, beta, 1e-5, True, p, 101, True, p_out, 202, None, m_ref)
            packed_ref = ops.pack_rows(y, fmt="mask")
            packed, side, stats_new = ops.fused_linear_fwd_packed(x, W, bias, gamma, beta, 1e-5, True, p, 101, True, p_out, 202, None, m_new,
                                                                  dense._arith_for(0, 128, 128, True, 0), fmt="mask")
        r = dict(y=y, stats=stats, packed_ref=packed_ref, m_ref=m_ref, packed=packed, side=side, stats_new=stats_new, m_new=m_new)
        if key[1:] != ("fp16x3", 0.5, 32 * 256 + 1):                 # (only what the gather test below reads again is kept)
            return r
        _REF[key] = r
    return _REF[key]


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("p", [0.5, 0.3])
@pytest.mark.parametrize("arith", ["fp16x3", "bf16x6"])
def test_packed_epilogue_equals_linear_then_pack_rows(arith, p, table, device):
    for n in ROWS:
        r = _pair(table, arith, p, n, device)
        k = fmt.mask_bits(r["packed_ref"].cpu()).sum(1).to(device)
        fits = k <= fmt.CAP
        assert torch.equal(r["packed"][:, :4], r["packed_ref"][:, :4]), (n, "mask dwords")
        defined = (torch.arange(fmt.PITCH_DW, device=device)[None, :] < (4 + k)[:, None]) & fits[:, None]
        assert torch.equal(r["packed"][defined], r["packed_ref"][defined]), (n, "value dwords of the rows that fit")
        assert torch.equal(_bits(r["side"])[~fits], _bits(r["y"])[~fits]), (n, "side table on the overflow rows")
        assert torch.equal(r["m_new"], r["m_ref"]), (n, "1-bit activation mask")
        assert torch.equal(_bits(r["stats_new"]), _bits(r["stats"])), (n, "row statistics")
        # the CPU encoder vouches for the reference's own packed rows, and for what the table is meant to hold
        enc = fmt.encode_rows(r["y"].cpu())
        assert torch.equal(enc[:, :4], r["packed_ref"][:, :4].cpu())
        share = float(fits.float().mean())
        print(f"{table} {arith} p={p} n={n}: rows that fit {share:.3f}, k mean {float(k.float().mean()):.1f} max {int(k.max())}")
        if table == "empty":
            assert int(k.max()) == 0
        if table == "overflow":
            assert not bool(fits.any())
        if table == "mixed" and n >= 32 * 256:
            assert 0.15 <= share <= 0.85, share                      # expected: P(Bin(128, 1/2) <= 60) = 0.27 fit, 0.73 overflow


@pytest.mark.parametrize("table", ["random", "mixed", "overflow"])
def test_gather_over_the_fused_output_is_the_dense_gather(table, device):
    from allset_amd import ops
    n_s = 32 * 256 + 1
    r = _pair(table, "fp16x3", 0.5, n_s, device)
    rowptr, col = _csr(300, n_s, seed=7)
    rowptr, col = rowptr.to(device), col.to(device)
    want, _ = ops.segreduce(SUM, rowptr, col, None, r["y"], 300, variant=1)
    got = ops.segreduce_packed(SUM, rowptr, col, r["packed"], r["side"], 300, fmt="mask")
    assert torch.equal(_bits(got), _bits(want))


# ---- layer level ---------------------------------------------------------------------------------------------------------------
def _run(step, params, x, mode):
    """One forward + backward of ``step`` under ``set_packed_epilogue(mode)`` with the dropout seed state brought to the same value."""
    from allset_amd import functional as AF
    was = AF.packed_epilogue()
    AF.set_packed_epilogue(mode)
    try:
        for p in params:
            p.grad = None
        xs = x.clone().requires_grad_(True)
        torch.manual_seed(11)
        (out, names) = _timed(lambda: step(xs))
        out.backward(torch.ones_like(out) * 0.5 + out.detach() * 0.25)
        return [out.detach(), xs.grad] + [p.grad.clone() for p in params], names
    finally:
        AF.set_packed_epilogue(was)


def test_halfnlhconv_fused_route_is_bitwise_unchanged(device):
    from allset_amd import Incidence
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).train()
    x = torch.randn(n_v, 128, device=device)
    params = list(conv.parameters())
    step = lambda t: conv(t, inc, None, "add")
    on, names_on = _run(step, params, x, "on")
    off, names_off = _run(step, params, x, "off")
    auto, names_auto = _run(step, params, x, "auto")
    assert "pack_rows" not in names_on and "segreduce_fwd" in names_on and "fused_linear_fwd" in names_on
    assert "pack_rows" in names_off
    assert "pack_rows" in names_auto                                 # 500 rows: below the threshold
    _assert_same(on, off)
    _assert_same(auto, off)


def test_sharded_layer_world1_fused_route_is_bitwise_unchanged(device):
    step, params, n_v = _sharded_step(device)
    x = torch.randn(n_v, 128, device=device)
    on, names_on = _run(step, params, x, "on")
    off, names_off = _run(step, params, x, "off")
    assert "pack_rows" not in names_on and "pack_rows" in names_off
    _assert_same(on, off)


def test_packed_gather_switch_turns_the_fused_route_off_too(device):
    from allset_amd import Incidence
    from allset_amd import functional as AF
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).train()
    x = torch.randn(n_v, 128, device=device)
    AF.set_packed_gather(False)
    try:
        assert not conv.packs_enc(x, inc, None, "add")
    finally:
        AF.set_packed_gather(True)


@pytest.mark.parametrize("case", ["eval", "dropout03", "hook", "single_linear", "bf16", "d64"])
def test_fallbacks_keep_todays_launches_and_results(case, device):
    from allset_amd import HalfNLHconv, Incidence
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    d = 64 if case == "d64" else 128
    torch.manual_seed(0)
    conv = HalfNLHconv(d, d, d, 1 if case == "single_linear" else 2, 0.3 if case == "dropout03" else 0.5, "ln", True, attention=False).to(device)
    conv = conv.eval() if case == "eval" else conv.train()
    seen = []
    if case == "hook":
        conv.f_enc.register_forward_hook(lambda mod, args, out: seen.append(out))
    x = torch.randn(n_v, d, device=device)
    if case == "bf16":
        conv, x = conv.to(torch.bfloat16), x.to(torch.bfloat16)
    params = list(conv.parameters())
    step = lambda t: conv(t, inc, None, "add")
    on, names_on = _run(step, params, x, "on")
    off, names_off = _run(step, params, x, "off")
    assert names_on == names_off                                     # the same launches, fused route forced or not
    _assert_same(on, off)
    if case == "hook":                                               # the hook saw the dense activation both times
        assert len(seen) == 2 and all(isinstance(t, torch.Tensor) and t.shape == (n_v, d) for t in seen)
        assert torch.equal(_bits(seen[0]), _bits(seen[1]))


def test_fused_route_replays_from_a_graph(device):
    """The fused route is decided from arguments alone: the layer step captures into one graph under "on", and the replay equals the
    eager step under the same seed counter (the pattern of test_gpu_packed_gather.test_layer_step_replays_from_a_graph)."""
    from allset_amd import dense
    from allset_amd import functional as AF
    from allset_amd.graphs import _side_stream_warmup
    step, params, n_v = _sharded_step(device)
    x = torch.randn(n_v, 128, device=device, requires_grad=True)
    counter = torch.full((1,), 5, dtype=torch.int64, device=device)
    G = torch.ones(n_v, 128, device=device)

    def fwd_bwd():
        for p in params:
            p.grad = None
        x.grad = None
        out = step(x)
        with dense.deferred_param_grads():
            out.backward(G)
        return out

    AF.set_packed_epilogue("on")
    try:
        _, names = _timed(lambda: step(x.detach()))
        assert "pack_rows" not in names
        with torch.cuda.device(device):
            with dense.device_seed_counter(counter):
                st = _side_stream_warmup(fwd_bwd, 2)
            graph = torch.cuda.CUDAGraph()
            with dense.device_seed_counter(counter), torch.cuda.graph(graph, stream=st):
                out = fwd_bwd()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params]
        del out
        with dense.device_seed_counter(counter):
            out = fwd_bwd()
        _assert_same([out.detach(), x.grad] + [p.grad for p in params], replayed)
    finally:
        AF.set_packed_epilogue("auto")
