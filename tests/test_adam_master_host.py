"""CPU: ``FusedAdam(master_weights=True)`` on its torch slow path (the fused kernel is tests/test_gpu_adam_master.py) and the
``--dtype`` flag of the driver.  A bf16 parameter trained through an fp32 master accumulates updates below half a bf16 spacing that
the bf16-moment form rounds away; the fp32 state survives ``state_dict`` / ``load_state_dict`` bit for bit (the stock
``load_state_dict`` would cast it to the parameter's bfloat16); ``master_state_dict`` is the full-precision checkpoint."""
import copy

import pytest
import torch

BF16 = torch.bfloat16


def _constant_gradient_run(master_weights, device="cpu", steps=64):
    from allset_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.ones(8, dtype=BF16, device=device))
    opt = FusedAdam([p], lr=2.0 ** -12, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, master_weights=master_weights)
    for _ in range(steps):
        p.grad = torch.ones(8, dtype=BF16, device=device)
        opt.step()
    return p, opt


def test_updates_below_half_a_bf16_spacing_accumulate_in_the_master():
    """Constant gradient 1: Adam's update is lr = 2^-12 per step (m_hat / sqrt(v_hat) = 1 up to eps), a sixteenth of the bf16
    spacing 2^-8 below 1.0.  64 steps move an fp32 weight to 1 - 64 * 2^-12 = 0.984375 (fp32 roundings of the 64 sums and eps = 1e-8:
    well inside 1e-5); the bf16 parameter is the master's rounding, within one spacing of that value; without masters every update is
    rounded away and the parameter is still exactly 1.0."""
    p, opt = _constant_gradient_run(True)
    master = opt.state[p]["master"]
    assert master.dtype == torch.float32 and p.dtype == BF16
    assert float((master - 0.984375).abs().max()) <= 1e-5
    assert float((p.detach().float() - 0.984375).abs().max()) <= 2.0 ** -8
    assert torch.equal(p.detach().view(torch.int16), master.to(BF16).view(torch.int16))
    q, opt_q = _constant_gradient_run(False)
    assert "master" not in opt_q.state[q]
    assert torch.equal(q.detach(), torch.ones(8, dtype=BF16))


def _stepped(sizes, seed, steps, params=None):
    from allset_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    if params is None:
        params = [torch.nn.Parameter(torch.randn(n, generator=g).to(BF16)) for n in sizes]
    opt = FusedAdam(params, lr=1e-2, weight_decay=0.01, master_weights=True)
    grads = [[torch.randn(n, generator=g).to(BF16) for n in sizes] for _ in range(steps)]
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        opt.step()
    return params, opt


def test_state_dict_round_trip_keeps_the_fp32_state_bit_for_bit():
    from allset_amd.optim import FusedAdam
    sizes = (2049, 1, 300)
    params, opt = _stepped(sizes, 11, 2)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["param_groups"][0]["master_weights"] is True
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = FusedAdam(twins, lr=1e-2, weight_decay=0.01, master_weights=True)
    opt2.load_state_dict(sd)
    for p, q in zip(params, twins):
        for k in ("master", "exp_avg", "exp_avg_sq"):
            a, b = opt.state[p][k], opt2.state[q][k]
            assert a.dtype == torch.float32 and b.dtype == torch.float32, k
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        assert float(opt2.state[q]["step"]) == 2.0
    # the masters hold more than the bf16 parameters do (else the round trip through bfloat16 would go unnoticed)
    assert any(not torch.equal(opt.state[p]["master"], p.detach().float()) for p in params)
    g = torch.Generator().manual_seed(12)
    for p, q in zip(params, twins):
        gr = torch.randn(p.shape, generator=g).to(BF16)
        p.grad, q.grad = gr.clone(), gr.clone()
    opt.step()
    opt2.step()
    for p, q in zip(params, twins):
        assert torch.equal(opt.state[p]["master"].view(torch.int32), opt2.state[q]["master"].view(torch.int32))
        assert torch.equal(p.detach().view(torch.int16), q.detach().view(torch.int16))
        assert torch.equal(q.detach().view(torch.int16), opt2.state[q]["master"].to(BF16).view(torch.int16))


def test_parse_args_dtype_and_what_bf16_refuses():
    from allset_amd.train import parse_args
    assert parse_args([]).dtype == 'fp32'
    assert parse_args(['--dtype', 'bf16', '--method', 'AllDeepSets']).dtype == 'bf16'
    assert parse_args(['--dtype', 'bf16', '--method', 'AllSetTransformer', '--exclude_self']).dtype == 'bf16'
    for argv in (['--dtype', 'bf16', '--method', 'HGNN'],
                 ['--dtype', 'bf16', '--normalization', 'bn'],
                 ['--dtype', 'bf16', '--method', 'AllSetTransformer', '--exclude_self', '--exclude_self_loo_attention']):
        with pytest.raises(SystemExit):
            parse_args(argv)


def test_bf16_exclude_self_takes_the_expansion():
    from allset_amd.train import exclude_self_path, parse_args
    assert exclude_self_path(parse_args(['--dtype', 'bf16', '--method', 'AllDeepSets', '--exclude_self', '--MLP_hidden', '128'])) == 'expand'


def test_master_state_dict_is_fp32_and_the_default_form_has_no_master():
    from allset_amd.optim import FusedAdam
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 2)).to(BF16)
    opt = FusedAdam(model.parameters(), lr=1e-3, master_weights=True)
    x = torch.randn(9, 5).to(BF16)
    fresh = opt.master_state_dict(model)                      # before any step: the parameters themselves, as fp32
    for k, p in model.named_parameters():
        assert fresh[k].dtype == torch.float32 and torch.equal(fresh[k], p.detach().float())
    for _ in range(3):
        opt.zero_grad()
        model(x).float().square().sum().backward()
        opt.step()
    sd = opt.master_state_dict(model)
    assert list(sd) == list(model.state_dict())
    moved = 0
    for k, p in model.named_parameters():
        assert sd[k].dtype == torch.float32, k
        assert torch.equal(sd[k].to(BF16).view(torch.int16), p.detach().view(torch.int16)), k
        assert sd[k].data_ptr() != opt.state[p]["master"].data_ptr()
        moved += int(not torch.equal(sd[k], p.detach().float()))
    assert moved > 0
    # sync_masters: parameters overwritten from outside are what the next step starts from
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(0.5)
    opt.sync_masters()
    for p in model.parameters():
        assert torch.equal(opt.state[p]["master"], torch.full(p.shape, 0.5))
    # the default form is unchanged: no master, state in the parameter's dtype
    plain = torch.nn.Parameter(torch.randn(6).to(BF16))
    opt_plain = FusedAdam([plain], lr=1e-3)
    plain.grad = torch.randn(6).to(BF16)
    opt_plain.step()
    assert sorted(opt_plain.state[plain]) == ["exp_avg", "exp_avg_sq", "step"]
    assert opt_plain.state[plain]["exp_avg"].dtype == BF16 and opt_plain.param_groups[0]["master_weights"] is False
    # fp32 parameters of a master_weights group behave as before
    w = torch.nn.Parameter(torch.randn(6))
    opt_w = FusedAdam([w], lr=1e-3, master_weights=True)
    w.grad = torch.randn(6)
    opt_w.step()
    assert sorted(opt_w.state[w]) == ["exp_avg", "exp_avg_sq", "step"]
