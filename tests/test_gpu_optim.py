"""The device optimisers (csrc/optim.hip: fst_adam_multi behind SharedStepAdam, fst_rmsprop_multi behind FusedRMSprop /
rmsprop_step_many) against torch.optim.Adam / RMSprop in float64 over several steps.  Needs an MI355X.

One step cannot tell a formula apart: at t = 1 RMSprop moves every element by ~10·lr·sign(g) and Adam by ~lr·sign(g), whatever
the bias correction or the decay.  So every test runs STEPS steps with gradient scales from 1e-3 to 1e3 per tensor and exact
zeros, and covers the launch geometry: up to 64 tensors per launch (OPT_MAX_T) and chunks beyond, 1-element tensors, a tensor
larger than the 64 workgroups x 1024 elements a tensor gets per pass (grid-stride loop), several learning rates in one launch, a
parameter without a gradient for one step.

The hyper-parameters are fp32 values (what the kernels receive) in both computations, so the comparison sees the update's own
arithmetic.  Per element the fp32 state carries at most a few ulp of |p| per step plus the update's relative rounding:
tol = 4·eps32·|p|·steps + 1e-5·lr·steps — with |p| of order 1 and lr >= 1e-2 about 0.1 % of lr after ten steps, well below what
a one-step shift of the bias correction (>= 1 % of lr) or a wrong decay weight moves.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd.optim import FusedRMSprop, SharedStepAdam, rmsprop_step_many

DEV = "cuda"
STEPS = 10
EPS32 = float(np.finfo(np.float32).eps)
f32 = lambda v: float(np.float32(v))


def _sizes(layout):
    """Tensor element counts of a test layout (the 300 000-element tensor grid-strides: 64 workgroups x 1024 per pass)."""
    rng = np.random.default_rng(len(layout))
    if layout == "one":
        return [1]
    if layout == "64":                                           # exactly one full launch
        return [1] + [int(v) for v in rng.integers(2, 3000, 63)]
    if layout == "65":                                           # a full launch and a one-tensor launch holding the big one
        return [int(v) for v in rng.integers(1, 3000, 64)] + [300_000]
    if layout == "130":                                          # three launches: 64 + 64 + 2, the big tensor in the middle one
        s = [int(v) for v in rng.integers(1, 3000, 130)]
        s[0], s[64], s[100], s[129] = 1, 1, 300_000, 5
        return s
    raise ValueError(layout)


def _start(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) * 2 - 1) for n in sizes]          # |p| <= 1


def _grads(sizes, step, seed):
    """fp32 gradients of one step: a per-tensor scale in 1e-3..1e3, a per-step factor, ~10 % exact zeros."""
    g = torch.Generator().manual_seed(seed * 1000 + step)
    scales = 10.0 ** (torch.rand(len(sizes), generator=torch.Generator().manual_seed(seed)) * 6 - 3)
    out = []
    for n, s in zip(sizes, scales):
        v = torch.randn(n, generator=g) * float(s) * (0.5 + torch.rand(1, generator=g).item())
        v[torch.rand(n, generator=g) < 0.1] = 0.0
        out.append(v)
    return out


def _assert_steps_close(got, want, lr, steps, what):
    for i, (a, w) in enumerate(zip(got, want)):
        a, w = a.detach().double().cpu(), w.detach().double()
        err = (a - w).abs()
        tol = 4 * EPS32 * w.abs() * steps + 1e-5 * lr * steps
        bad = err > tol
        assert not bool(bad.any()), (f"{what}: tensor {i} ({w.numel()} elements): {int(bad.sum())} elements off, max err "
                                     f"{float(err.max()):.3e} (tol {float(tol[bad].min()):.3e} at the worst)")


@pytest.mark.parametrize("layout", ["one", "64", "65", "130"])
def test_shared_step_adam_vs_torch_adam(layout):
    sizes = _sizes(layout)
    p0 = _start(sizes, 7)
    lr, betas, eps = f32(1e-2), (f32(0.9), f32(0.999)), f32(1e-8)
    dev = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ref = [torch.nn.Parameter(p.double()) for p in p0]
    opt = SharedStepAdam(dev, lr=lr, betas=betas, eps=eps)
    ref_opt = torch.optim.Adam(ref, lr=lr, betas=betas, eps=eps, foreach=False)
    skip = len(sizes) // 2 if len(sizes) > 1 else None            # this parameter has no gradient at step 3
    for t in range(1, STEPS + 1):
        gs = _grads(sizes, t, 7)
        for i, (pd, pr, g) in enumerate(zip(dev, ref, gs)):
            none = i == skip and t == 3
            pd.grad = None if none else g.to(DEV)
            pr.grad = None if none else g.double()
        # one shared device counter: a parameter that sat a step out is corrected with the group's t, not its own count
        for pr in ref:
            if "step" in ref_opt.state[pr]:
                ref_opt.state[pr]["step"].fill_(t - 1)
        opt.step()
        ref_opt.step()
    assert float(opt.param_groups[0]["step"]) == STEPS, "the shared device step counter"
    _assert_steps_close(dev, ref, lr, STEPS, f"Adam {layout}")
    for name in ("exp_avg", "exp_avg_sq"):
        for i, (pd, pr) in enumerate(zip(dev, ref)):
            a, w = opt.state[pd][name].double().cpu(), ref_opt.state[pr][name]
            assert float((a - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-30, f"Adam {layout}: {name} of tensor {i}"


def test_shared_step_adam_skipped_parameter_stays_put():
    """A parameter whose .grad is None is not touched by the step (nor are its moments), while the others move."""
    sizes = [3, 70_000, 5]
    p0 = _start(sizes, 3)
    dev = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    opt = SharedStepAdam(dev, lr=1e-2)
    gs = _grads(sizes, 1, 3)
    dev[0].grad, dev[1].grad, dev[2].grad = gs[0].to(DEV), None, gs[2].to(DEV)
    opt.step()
    assert torch.equal(dev[1].detach().cpu(), p0[1])
    assert float(opt.state[dev[1]]["exp_avg"].abs().max()) == 0.0 and float(opt.state[dev[1]]["exp_avg_sq"].abs().max()) == 0.0
    assert not torch.equal(dev[0].detach().cpu(), p0[0]) and not torch.equal(dev[2].detach().cpu(), p0[2])


@pytest.mark.parametrize("layout", ["one", "64", "65", "130"])
def test_rmsprop_step_many_vs_torch_rmsprop(layout):
    """Three FusedRMSprops with different learning rates stepped by ONE rmsprop_step_many call per step: the tensors of one launch
    carry different lr (the joint step's ten optimisers share launches the same way)."""
    sizes = _sizes(layout)
    p0 = _start(sizes, 11)
    alpha, eps = f32(0.99), f32(1e-8)
    lrs = [f32(1e-2), f32(3e-2), f32(2e-2)]
    parts = [list(range(i, len(sizes), 3)) for i in range(3)] if len(sizes) >= 3 else [[0], [], []]
    dev = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ref = [torch.nn.Parameter(p.double()) for p in p0]
    opts = [FusedRMSprop([dev[i] for i in idx], lr=lr, alpha=alpha, eps=eps) for idx, lr in zip(parts, lrs) if idx]
    ref_opts = [torch.optim.RMSprop([ref[i] for i in idx], lr=lr, alpha=alpha, eps=eps, foreach=False)
                for idx, lr in zip(parts, lrs) if idx]
    lr_of = {i: lr for idx, lr in zip(parts, lrs) for i in idx}
    skip = len(sizes) // 2 if len(sizes) > 1 else None
    for t in range(1, STEPS + 1):
        gs = _grads(sizes, t, 11)
        for i, (pd, pr, g) in enumerate(zip(dev, ref, gs)):
            none = i == skip and t == 4
            pd.grad = None if none else g.to(DEV)
            pr.grad = None if none else g.double()
        rmsprop_step_many(opts)
        for o in ref_opts:
            o.step()
    for i, (pd, pr) in enumerate(zip(dev, ref)):
        _assert_steps_close([pd], [pr], lr_of[i], STEPS, f"RMSprop {layout} tensor {i} (lr {lr_of[i]:g})")
        st = [o for o in opts if pd in o.state][0].state[pd]["square_avg"]
        w = [o for o in ref_opts if pr in o.state][0].state[pr]["square_avg"]
        assert float((st.double().cpu() - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-30, f"RMSprop {layout}: square_avg {i}"


def test_fused_rmsprop_step_alone_matches_torch():
    """FusedRMSprop.step() on its own (the single-optimiser entry point), a 1-element tensor next to a grid-striding one."""
    sizes = [1, 200_000]
    p0 = _start(sizes, 5)
    dev = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ref = [torch.nn.Parameter(p.double()) for p in p0]
    opt, ref_opt = FusedRMSprop(dev, lr=f32(1e-2)), torch.optim.RMSprop(ref, lr=f32(1e-2), alpha=f32(0.99), eps=f32(1e-8))
    for t in range(1, STEPS + 1):
        for pd, pr, g in zip(dev, ref, _grads(sizes, t, 5)):
            pd.grad, pr.grad = g.to(DEV), g.double()
        opt.step()
        ref_opt.step()
    _assert_steps_close(dev, ref, f32(1e-2), STEPS, "FusedRMSprop.step")
