"""CPU checks of the fused optimizer: the NumPy oracle of pwc_optim.hip's arithmetic (tests/optim_oracle.py) against torch.optim.Adam /
AdamW, and the host logic of opticalflow_amd.optim (chunk table, checkpoints, rejected inputs, hyper-parameters re-read).  The kernels
themselves are checked against the same oracle in tests/test_gpu_optim.py."""
import copy

import numpy as np
import pytest
import torch

from optim_oracle import AdamOracle, clip_coef
from opticalflow_amd import FusedAdam, FusedAdamW, _lib
from opticalflow_amd.optim import chunk_table

SHAPES = [(1,), (3,), (7, 5), (16, 3, 3, 3), (257,), (2, 1031)]
MODES = {"plain": (torch.optim.Adam, 0.0, False), "l2": (torch.optim.Adam, 1e-4, False), "decoupled": (torch.optim.AdamW, 1e-2, True)}
STEPS, LR = 5, 1e-3


def _inputs(seed=0):
    """|p| ~ 0.5; gradients of either sign whose magnitudes span 1e-4 .. 10 (log-uniform), new ones for every step."""
    rng = np.random.default_rng(seed)
    params = [(rng.uniform(0.25, 0.75, s) * rng.choice([-1.0, 1.0], s)) for s in SHAPES]
    grads = [[10.0 ** rng.uniform(-4, 1, s) * rng.choice([-1.0, 1.0], s) for s in SHAPES] for _ in range(STEPS)]
    return params, grads


def _run_torch(cls, wd, params, grads, dtype):
    """clip_grad_norm_(1.0) + the single-tensor torch optimizer in `dtype`; returns the parameters and the norm of every step."""
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in params]
    opt = cls(ps, lr=LR, weight_decay=wd, foreach=False)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=dtype)
        norms.append(torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=False))
        opt.step()
    return [p.detach().numpy() for p in ps], norms


def _run_oracle(wd, decoupled, params, grads, coefs, dtype):
    o = AdamOracle(params, dtype)
    for gs, c in zip(grads, coefs):
        o.step(gs, LR, weight_decay=wd, decoupled=decoupled, coef=c)
    return o.p


@pytest.fixture(scope="module")
def torch64():
    params, grads = _inputs()
    return params, grads, {k: _run_torch(cls, wd, params, grads, torch.float64) for k, (cls, wd, _) in MODES.items()}


@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_float64_matches_torch(torch64, mode):
    params, grads, ref = torch64
    _, wd, decoupled = MODES[mode]
    ref_p, norms = ref[mode]
    coefs = [min(1.0, 1.0 / (float(n) + 1e-6)) for n in norms]
    assert min(coefs) < 1.0                                      # the clip is active
    got = _run_oracle(wd, decoupled, params, grads, coefs, np.float64)
    err = max(np.abs(a - b).max() for a, b in zip(got, ref_p))
    print("float64 oracle vs torch (%s): max abs diff %.3e" % (mode, err))
    assert err <= 1e-15


@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_float32_no_worse_than_torch_float32(torch64, mode):
    params, grads, ref = torch64
    cls, wd, decoupled = MODES[mode]
    ref_p = ref[mode][0]
    p32 = [p.astype(np.float32) for p in params]
    g32 = [[g.astype(np.float32) for g in gs] for gs in grads]
    t32, norms32 = _run_torch(cls, wd, p32, g32, torch.float32)
    coefs = [clip_coef(float(n), 1.0) for n in norms32]
    o32 = _run_oracle(wd, decoupled, p32, g32, coefs, np.float32)
    assert all(p.dtype == np.float32 for p in o32)
    err_oracle = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(o32, ref_p))
    err_torch = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(t32, ref_p))
    print("float32 vs float64 torch (%s): oracle %.3e, torch float32 %.3e" % (mode, err_oracle, err_torch))
    assert err_oracle <= 2.0 * err_torch


def test_oracle_skip_and_grad_scale():
    params, grads = _inputs(1)
    a, b = AdamOracle(params, np.float32), AdamOracle(params, np.float32)
    a.step(grads[0], LR, found_inf=True)
    assert a.step_count == 0 and all(np.array_equal(x, np.float32(y)) for x, y in zip(a.p, params))
    a.step([g * 1024.0 for g in grads[0]], LR, grad_scale=1024.0)          # a power of two: g * s / s is exact
    b.step(grads[0], LR)
    assert all(np.array_equal(x, y) for x, y in zip(a.p, b.p))
    b.step([None] + grads[1][1:], LR)
    assert np.array_equal(b.p[0], a.p[0]) and not np.array_equal(b.p[1], a.p[1])


# ------------------------------------------------------------------ host logic
def test_chunk_table():
    K = _lib.load().pwc_optim_chunk_elems()
    assert K > 0 and K % 4 == 0
    numels = [1, K - 1, K, K + 1, 0, 3 * K + 5]
    t = chunk_table(numels, K)
    assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"]
    assert t.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [5, 0], [5, 1], [5, 2], [5, 3]]
    covered = {}
    for ti, c in t.tolist():                                     # every element of every tensor exactly once
        n = min(K, numels[ti] - c * K)
        assert n > 0
        covered[ti] = covered.get(ti, 0) + n
    assert covered == {i: n for i, n in enumerate(numels) if n}
    assert chunk_table([], K).shape == (0, 2) and chunk_table([0, 0], K).shape == (0, 2)
    with pytest.raises(ValueError):
        chunk_table([4], 0)
    assert _lib.load().pwc_optim_workspace_bytes(len(t), 2) == 8 * len(t) + 2 * 32
    assert _lib.load().pwc_optim_workspace_bytes(0, 1) == -1


def test_gradient_pointers_skip_missing_gradients():
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (4, 9, 2)]
    opt = FusedAdam(ps, lr=1e-3)
    ps[0].grad, ps[2].grad = torch.ones(4), torch.ones(2)
    gptrs, keep, dirty = opt._collect(ps)
    assert gptrs == [ps[0].grad.data_ptr(), 0, ps[2].grad.data_ptr()] and dirty and not keep
    assert set(opt.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq"} and not opt.state.get(ps[1])
    ps[2].grad = torch.ones(2, 2)[:, 0]                          # not dense: a copy is read, p.grad stays as it is
    gptrs, keep, _ = opt._collect(ps)
    assert len(keep) == 1 and gptrs[2] == keep[0].data_ptr() != ps[2].grad.data_ptr()


def test_step_refuses_cpu_parameters():
    from opticalflow_amd import PwcHipError
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([p], lr=1e-3, max_grad_norm=1.0)
    opt.step()                                                   # no gradient anywhere: nothing to do, as in torch
    p.grad = torch.ones(4)
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        opt.step()
    assert not bool(p.detach().any())


def test_rejected_inputs():
    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls([p], lr=1e-3, amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls([p], lr=1e-3, maximize=True)
        for bad in (torch.float64, torch.float16, torch.bfloat16, torch.complex64):
            with pytest.raises(TypeError):
                cls([torch.nn.Parameter(torch.zeros(4, dtype=bad))], lr=1e-3)
        with pytest.raises(ValueError):
            cls([p], lr=1e-3, max_grad_norm=0.0)
        with pytest.raises(ValueError):
            cls([p], lr=-1.0)
        with pytest.raises(TypeError):
            cls([p], lr=torch.tensor(1e-3))
    opt = FusedAdam([p], lr=1e-3)
    opt.param_groups[0]["amsgrad"] = True                        # e.g. from a loaded checkpoint
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    with pytest.raises(TypeError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]})
    assert FusedAdam._step_supports_amp_scaling and FusedAdamW([p]).defaults["weight_decay"] == 1e-2


def test_hyper_parameters_are_read_at_every_step():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([p], lr=1e-2, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    assert opt._hyper(opt.param_groups[0]) == (1e-2, 0.9, 0.999, 1e-8, 1e-4, False)
    opt.step()
    sched.step()
    assert opt._hyper(opt.param_groups[0])[0] == 5e-3
    opt.param_groups[0]["lr"] = 1e-4                              # train.py's manual schedule
    opt.param_groups[0]["betas"] = (0.8, 0.99)
    assert opt._hyper(opt.param_groups[0])[:3] == (1e-4, 0.8, 0.99)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(FusedAdamW([p], lr=1e-3), patience=0, factor=0.1)
    plateau.step(1.0)
    plateau.step(2.0)
    assert plateau.optimizer._hyper(plateau.optimizer.param_groups[0])[0] == pytest.approx(1e-4)
    assert plateau.optimizer._hyper(plateau.optimizer.param_groups[0])[5] is True


@pytest.mark.parametrize("fused_cls,torch_cls", [(FusedAdam, torch.optim.Adam), (FusedAdamW, torch.optim.AdamW)])
def test_state_dict_round_trips_with_torch(fused_cls, torch_cls):
    def make():
        g = torch.Generator().manual_seed(3)
        return [torch.nn.Parameter(torch.rand(s, generator=g)) for s in [(5,), (3, 4)]]
    # torch -> fused: three torch steps, then the state loads and the device record is rebuilt from `step`
    ps = make()
    topt = torch_cls(ps, lr=2e-3, betas=(0.8, 0.95), weight_decay=1e-2, foreach=False)
    for i in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (i + 1))
        topt.step()
    qs = make()
    fopt = fused_cls(qs, lr=1e-3, max_grad_norm=1.0)
    fopt.load_state_dict(copy.deepcopy(topt.state_dict()))       # a checkpoint: load_state_dict itself keeps the tensors it is given
    assert fopt._steprec_host == [[3.0, 0.8 ** 3, 0.95 ** 3]] and fopt.max_grad_norm == 1.0
    g = fopt.param_groups[0]
    assert g["lr"] == 2e-3 and g["betas"] == (0.8, 0.95) and g["decoupled_weight_decay"] == fopt._decoupled
    for p, q in zip(ps, qs):
        assert torch.equal(fopt.state[q]["exp_avg"], topt.state[p]["exp_avg"])
        assert torch.equal(fopt.state[q]["exp_avg_sq"], topt.state[p]["exp_avg_sq"])
    # fused -> torch: the state dict has torch's keys, loads, and torch steps from it exactly as from its own
    sd = fopt.state_dict()
    assert set(sd["param_groups"][0]) >= set(topt.state_dict()["param_groups"][0])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 3.0 for s in sd["state"].values())
    rs = make()
    with torch.no_grad():
        for r, p in zip(rs, ps):
            r.copy_(p)
    topt2 = torch_cls(rs, lr=1.0, foreach=False)
    topt2.load_state_dict(copy.deepcopy(sd))
    for p, r in zip(ps, rs):
        p.grad = torch.full_like(p, -0.3)
        r.grad = torch.full_like(r, -0.3)
    topt.step()
    topt2.step()
    assert all(torch.equal(p, r) for p, r in zip(ps, rs))
    # unequal per-parameter steps cannot be represented
    bad = topt.state_dict()
    bad["state"][0]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="unequal step"):
        fused_cls(make(), lr=1e-3).load_state_dict(bad)
    ams = torch_cls(make(), lr=1e-3, amsgrad=True, foreach=False)
    for p in ams.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    ams.step()
    with pytest.raises(ValueError, match="amsgrad"):
        fused_cls(make(), lr=1e-3).load_state_dict(ams.state_dict())
