"""FusedAdam / FusedAdamW on the device (csrc/pwc_optim.hip) against tests/optim_oracle.py, bit for bit: the float32 oracle restates the
kernel's arithmetic, and tests/test_optim_cpu.py ties that oracle to torch.optim.Adam / AdamW.  The oracle is fed the device's own
total norm (the clip coefficient is float32 arithmetic on it); the norm has its own check against a float64 sum."""
import copy

import numpy as np
import pytest
import torch

from optim_oracle import AdamOracle, clip_coef

pytestmark = pytest.mark.gpu

STEPS, LR = 5, 1e-3
MODES = {"plain": ("adam", 0.0), "l2": ("adam", 1e-4), "decoupled": ("adamw", 1e-2)}


@pytest.fixture(scope="module")
def dev(gpu_device):
    from opticalflow_amd import _lib
    _lib.load()
    return gpu_device


@pytest.fixture(scope="module")
def K(dev):
    from opticalflow_amd import ops
    return ops.optim_chunk_elems()


def _cls(kind):
    from opticalflow_amd import FusedAdam, FusedAdamW
    return FusedAdam if kind == "adam" else FusedAdamW


class Case:
    """The parameter set of the kernel tests: every tail length of the 16-byte path, the chunk boundaries, PWCDCNet's largest
    tensor, more tensors than any one argument block could hold, a parameter and a gradient that are not 16-byte aligned, and two
    parameters that never get a gradient.  Gradient magnitudes span 1e-4 .. 10 on the small tensors and 1e-4 .. 1 on the large ones,
    which keeps the total norm between 1 and 1e3: max_norm = 1 clips, max_norm = 1e3 gives a coefficient of exactly 1."""

    def __init__(self, K, seed=0):
        self.numels = [1, 2, 3, 5, 7, 64, 255, 256, 257, K - 1, K, K + 1, 3 * K + 5, 650880] + [2] * 300 + [1027, 9, K + 3, 4100]
        self.unaligned_p = len(self.numels) - 4          # numel 1027: a view one element into its buffer
        self.no_grad = (len(self.numels) - 3, len(self.numels) - 2)
        self.unaligned_g = len(self.numels) - 1          # numel 4100: its gradient is such a view
        rng = np.random.default_rng(seed)
        self.values = [(rng.uniform(0.25, 0.75, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in self.numels]
        self.grads = []
        for _ in range(STEPS):
            gs = []
            for i, n in enumerate(self.numels):
                if i in self.no_grad:
                    gs.append(None)
                    continue
                g = (10.0 ** rng.uniform(-4, 1 if n < 1000 else 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
                if n > 16:
                    g[rng.integers(0, n, n // 16)] = 0.0  # exact zeros: v stays 0 there while nothing else arrives
                gs.append(g)
            self.grads.append(gs)

    def params(self, dev):
        ps = []
        for i, v in enumerate(self.values):
            if i == self.unaligned_p:
                buf = torch.zeros(v.size + 1, dtype=torch.float32, device=dev)
                buf[1:] = torch.from_numpy(v).to(dev)
                p = torch.nn.Parameter(buf[1:])
                assert p.data_ptr() % 16 == 4
            else:
                p = torch.nn.Parameter(torch.from_numpy(v).to(dev))
            ps.append(p)
        return ps

    def set_grads(self, ps, step, dev, scale=1.0, hold=None):
        """New gradient tensors for this step (hold keeps the old ones alive, so the new ones cannot get their addresses)."""
        for i, (p, g) in enumerate(zip(ps, self.grads[step])):
            if g is None:
                p.grad = None
                continue
            if hold is not None and p.grad is not None:
                hold.append(p.grad)
            t = torch.from_numpy(g).to(dev)
            if scale != 1.0:
                t = t * scale
            if i == self.unaligned_g:
                buf = torch.zeros(g.size + 1, dtype=torch.float32, device=dev)
                buf[1:] = t
                t = buf[1:]
                assert t.data_ptr() % 16 == 4
            p.grad = t.view_as(p)


@pytest.fixture(scope="module")
def case(K):
    return Case(K)


def _state(opt, ps):
    out = []
    for p in ps:
        st = opt.state.get(p)
        out.append((p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy() if st else None, st["exp_avg_sq"].cpu().numpy() if st else None))
    return out


def _run_fused(case, dev, mode, max_norm, steps=STEPS):
    kind, wd = MODES[mode]
    ps = case.params(dev)
    opt = _cls(kind)(ps, lr=LR, weight_decay=wd, max_grad_norm=max_norm)
    norms, hold = [], []
    for s in range(steps):
        case.set_grads(ps, s, dev, hold=hold)
        before = [p.grad.clone() if p.grad is not None else None for p in ps] if s == 0 else None
        opt.step()
        norms.append(opt.last_grad_norm.clone() if max_norm is not None else None)
        if before is not None:                                   # p.grad is left as it was, clipped or not
            assert all(b is None or torch.equal(b, p.grad) for b, p in zip(before, ps))
    torch.cuda.synchronize()
    return _state(opt, ps), [None if n is None else np.float32(n.item()) for n in norms], opt, ps


def _run_oracle(case, mode, max_norm, norms, steps=STEPS):
    kind, wd = MODES[mode]
    o = AdamOracle(case.values, np.float32)
    coefs = []
    for s in range(steps):
        c = np.float32(1.0) if max_norm is None else clip_coef(norms[s], max_norm)
        coefs.append(float(c))
        o.step(case.grads[s], LR, weight_decay=wd, decoupled=(kind == "adamw"), coef=c)
    return o, coefs


def _assert_bit_equal(case, got, o):
    for i, (p, m, v) in enumerate(got):
        if i in case.no_grad:
            assert m is None and v is None and p.tobytes() == case.values[i].tobytes(), "untouched parameter %d changed" % i
            continue
        for name, a, b in (("p", p, o.p[i]), ("exp_avg", m, o.m[i]), ("exp_avg_sq", v, o.v[i])):
            assert a.dtype == np.float32 and a.tobytes() == b.reshape(a.shape).tobytes(), \
                "%s of tensor %d (numel %d): %d of %d elements differ, max abs diff %.3e" % (
                    name, i, a.size, int((a != b.reshape(a.shape)).sum()), a.size, float(np.abs(a - b.reshape(a.shape)).max()))


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e3])
@pytest.mark.parametrize("mode", list(MODES))
def test_update_bit_equal_to_oracle(dev, case, mode, max_norm):
    got, norms, opt, _ = _run_fused(case, dev, mode, max_norm)
    o, coefs = _run_oracle(case, mode, max_norm, norms)
    if max_norm == 1.0:
        assert max(coefs) < 1.0
    elif max_norm == 1e3:
        assert all(c == 1.0 for c in coefs) and min(norms) > 1.0
    else:
        assert opt.last_grad_norm is None
    _assert_bit_equal(case, got, o)
    assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {float(STEPS)}


def test_total_norm_within_two_ulp(dev, case):
    _, norms, _, _ = _run_fused(case, dev, "plain", 1.0, steps=2)
    for s in range(2):
        total = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in case.grads[s] if g is not None)
        ref = np.float32(np.sqrt(total))
        ulps = abs(float(norms[s]) - float(ref)) / float(np.spacing(ref))
        print("step %d: device norm %.9g, float64 reference %.9g, %.2f ulp" % (s, norms[s], ref, ulps))
        assert ulps <= 2.0


def test_two_runs_are_byte_identical(dev, case):
    a, na, _, _ = _run_fused(case, dev, "decoupled", 1.0, steps=3)
    b, nb, _, _ = _run_fused(case, dev, "decoupled", 1.0, steps=3)
    assert [x.tobytes() for x in na] == [x.tobytes() for x in nb]
    for (p, m, v), (q, n, w) in zip(a, b):
        assert p.tobytes() == q.tobytes()
        assert (m is None and n is None) or (m.tobytes() == n.tobytes() and v.tobytes() == w.tobytes())


def test_found_inf_skips_and_grad_scale_unscales(dev, case):
    scale = 65536.0                                              # GradScaler's scales are powers of two: g * s / s is exact
    ps = case.params(dev)
    opt = _cls("adamw")(ps, lr=LR, weight_decay=1e-2, max_grad_norm=1.0)
    case.set_grads(ps, 0, dev, scale=scale)
    opt.grad_scale = torch.full((), scale, dtype=torch.float32, device=dev)
    opt.found_inf = torch.ones((), dtype=torch.float32, device=dev)
    opt.step()
    torch.cuda.synchronize()
    for i, p in enumerate(ps):                                   # skipped: nothing written, the count stays
        assert p.detach().cpu().numpy().tobytes() == case.values[i].tobytes()
        st = opt.state.get(p)
        assert not st or (not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()))
    assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {0.0}
    opt.found_inf = torch.zeros((), dtype=torch.float32, device=dev)
    opt.step()                                                   # the good step that follows is the oracle's step 1 on g / s
    norm = np.float32(opt.last_grad_norm.item())
    o = AdamOracle(case.values, np.float32)
    o.step(case.grads[0], LR, weight_decay=1e-2, decoupled=True, coef=clip_coef(norm, 1.0))
    _assert_bit_equal(case, _state(opt, ps), o)
    total = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in case.grads[0] if g is not None)
    assert abs(float(norm) - np.sqrt(total)) <= 2.0 * float(np.spacing(np.float32(np.sqrt(total))))   # the norm of the UNSCALED gradients
    assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {1.0}


def test_grad_scaler_drives_the_optimizer(dev):
    """torch.amp.GradScaler.step() takes the _step_supports_amp_scaling route: an inf gradient skips the step and backs the scale
    off, a finite one steps with the gradients unscaled inside the update."""
    vals = np.linspace(-1.0, 1.0, 37, dtype=np.float32)
    g = np.linspace(0.5, -0.25, 37, dtype=np.float32)
    p = torch.nn.Parameter(torch.from_numpy(vals).to(dev))
    opt = _cls("adam")([p], lr=LR)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=1000)
    scaler.scale(torch.zeros((), device=dev))                    # creates the scale tensor
    p.grad = torch.from_numpy(g).to(dev) * 1024.0
    p.grad[3] = float("inf")
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 512.0 and p.detach().cpu().numpy().tobytes() == vals.tobytes()
    p.grad = torch.from_numpy(g).to(dev) * 512.0
    scaler.step(opt)
    scaler.update()
    o = AdamOracle([vals], np.float32)
    o.step([g], LR)
    assert p.detach().cpu().numpy().tobytes() == o.p[0].tobytes()
    assert not hasattr(opt, "found_inf") and float(opt.state_dict()["state"][0]["step"]) == 1.0


def test_gradient_pointers_may_change_or_stay(dev, case):
    """Step 0 and 2 with newly allocated gradients (zero_grad(set_to_none=True) in between), step 1 written into step 0's tensors."""
    ps = case.params(dev)
    opt = _cls("adam")(ps, lr=LR, weight_decay=1e-4, max_grad_norm=1.0)
    norms = []
    case.set_grads(ps, 0, dev)
    ptrs0 = [p.grad.data_ptr() for p in ps if p.grad is not None]
    opt.step()
    norms.append(np.float32(opt.last_grad_norm.item()))
    with torch.no_grad():
        for p, g in zip(ps, case.grads[1]):
            if g is not None:
                p.grad.copy_(torch.from_numpy(g).to(dev).view_as(p))
    assert ptrs0 == [p.grad.data_ptr() for p in ps if p.grad is not None]
    opt.step()
    norms.append(np.float32(opt.last_grad_norm.item()))
    hold = [p.grad for p in ps]
    opt.zero_grad(set_to_none=True)
    case.set_grads(ps, 2, dev)
    assert ptrs0 != [p.grad.data_ptr() for p in ps if p.grad is not None]
    opt.step()
    norms.append(np.float32(opt.last_grad_norm.item()))
    del hold
    o, _ = _run_oracle(case, "l2", 1.0, norms, steps=3)
    _assert_bit_equal(case, _state(opt, ps), o)


def test_step_bumps_the_version_of_updated_parameters(dev):
    """The kernels write through raw pointers; PWCDCNet's cached inference plans and autograd's saved-tensor checks go by
    Tensor._version, so a step must bump it for the parameters it updated, and only for those."""
    ps = [torch.nn.Parameter(torch.ones(5, device=dev)) for _ in range(3)]
    opt = _cls("adam")(ps, lr=LR)
    ps[0].grad, ps[2].grad = torch.ones(5, device=dev), torch.ones(5, device=dev)
    before = [p._version for p in ps]
    opt.step()
    assert [p._version - b for p, b in zip(ps, before)] == [1, 0, 1]
    saved = (ps[0] * ps[0]).sum()                                # its backward needs ps[0] as it was
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        saved.backward()


def test_schedulers_are_followed(dev, case):
    ps = case.params(dev)
    opt = _cls("adam")(ps, lr=4e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    o = AdamOracle(case.values, np.float32)
    lrs = []
    for s in range(STEPS):
        if s == 4:
            for g in opt.param_groups:                           # train.py's manual schedule
                g["lr"] = 7e-4
        lr = opt.param_groups[0]["lr"]
        lrs.append(lr)
        case.set_grads(ps, s, dev)
        opt.step()
        sched.step()
        o.step(case.grads[s], lr, weight_decay=1e-4)
    assert lrs == [4e-3, 4e-3, 2e-3, 2e-3, 7e-4]
    _assert_bit_equal(case, _state(opt, ps), o)


def test_two_parameter_groups_share_the_norm(dev, case):
    ps = case.params(dev)
    cut = 13                                                     # group 0 ends inside the run of chunk-boundary sizes
    opt = _cls("adamw")([{"params": ps[:cut], "lr": 2e-3, "weight_decay": 0.0},
                         {"params": ps[cut:], "lr": 5e-4, "weight_decay": 5e-2, "betas": (0.8, 0.99)}], lr=LR, max_grad_norm=1.0)
    oa, ob = AdamOracle(case.values[:cut], np.float32), AdamOracle(case.values[cut:], np.float32)
    for s in range(3):
        case.set_grads(ps, s, dev)
        opt.step()
        norm = np.float32(opt.last_grad_norm.item())
        total = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in case.grads[s] if g is not None)
        assert abs(float(norm) - np.sqrt(total)) <= 2.0 * float(np.spacing(np.float32(np.sqrt(total))))      # over BOTH groups
        c = clip_coef(norm, 1.0)
        oa.step(case.grads[s][:cut], 2e-3, weight_decay=0.0, decoupled=True, coef=c)
        ob.step(case.grads[s][cut:], 5e-4, betas=(0.8, 0.99), weight_decay=5e-2, decoupled=True, coef=c)
    merged = AdamOracle([], np.float32)
    merged.p, merged.m, merged.v = oa.p + ob.p, oa.m + ob.m, oa.v + ob.v
    _assert_bit_equal(case, _state(opt, ps), merged)
    sd = opt.state_dict()
    assert {float(s["step"]) for s in sd["state"].values()} == {3.0} and len(sd["param_groups"]) == 2


# ------------------------------------------------------------------ end to end
LEVEL_W = (1.0, 0.5, 0.25, 0.125, 0.0625)


def _close(got, ref, rel, what):
    """tests/test_gpu_train.py's training-step parity bound: max abs error <= rel * max |ref|."""
    err = (got.double() - ref.double()).abs().max().item()
    bound = rel * ref.abs().max().item()
    print("%s: max err %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, "%s: max err %.3e > %.3e" % (what, err, bound)


def _train(dev, make_opt, steps, clip_outside, resume=None, keep=None):
    """`steps` training steps of PWCDCNet(trainable=True) at 1 x 6 x 64 x 64 from the synthetic weights, from a (model state,
    optimizer state) checkpoint, or continuing a (net, optimizer) pair; returns them and the five flows after the steps."""
    from conftest import seeded_rand
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    if keep is not None:
        net, opt = keep
    else:
        net = PWCDCNet(trainable=True)
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        net = net.to(dev).train()
        if resume is not None:
            net.load_state_dict(resume[0])
        opt = make_opt(net.parameters())
        if resume is not None:
            opt.load_state_dict(copy.deepcopy(resume[1]))
    x = seeded_rand((1, 6, 64, 64), 700).to(dev)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        sum(w * f.abs().mean() for w, f in zip(LEVEL_W, net(x))).backward()
        if clip_outside:
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
    with torch.no_grad():
        flows = [f.clone() for f in net(x)]
    return net, opt, flows


def test_training_steps_match_torch_adamw(dev):
    from opticalflow_amd import FusedAdamW
    hp = dict(lr=1e-4, weight_decay=1e-2)
    net_f, opt_f, flows_f = _train(dev, lambda ps: FusedAdamW(ps, max_grad_norm=1.0, **hp), 3, clip_outside=False)
    net_t, opt_t, flows_t = _train(dev, lambda ps: torch.optim.AdamW(ps, **hp), 3, clip_outside=True)
    assert float(opt_f.last_grad_norm) > 0.0
    for lvl, (a, b) in enumerate(zip(flows_f, flows_t)):
        _close(a, b, 1e-3, "flow level %d after 3 steps" % lvl)
    # the fused run's checkpoint resumes in torch.optim.AdamW: one more step there against one more fused step
    ckpt = (copy.deepcopy(net_f.state_dict()), opt_f.state_dict())
    assert {float(s["step"]) for s in ckpt[1]["state"].values()} == {3.0}
    _, _, more_t = _train(dev, lambda ps: torch.optim.AdamW(ps, **hp), 1, clip_outside=True, resume=ckpt)
    # the fused run goes on with its own network, whose inference plan of the weights after step 3 is cached: the flows after
    # step 4 are right only if the step told the network that its parameters changed
    _, _, more_f = _train(dev, None, 1, clip_outside=False, keep=(net_f, opt_f))
    for lvl, (a, b) in enumerate(zip(more_f, more_t)):
        _close(a, b, 1e-3, "flow level %d, step 4 from the fused checkpoint" % lvl)
    assert not torch.equal(more_f[0], flows_f[0])
