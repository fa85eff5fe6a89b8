"""The six pre-training phases as captured hipGraphs: ``JointTrainer.capture_phase`` / ``replay_phase`` / ``release_phase`` /
``captured_phases`` against (1) the reference's own phase fixture, (2) the eager ``phase_step`` from the same snapshot.

Gates.  Against the fixture: 1e-4 · max(1, |want|), the eager phase test's.  Replay against eager, losses: 1e-6 · max(1, |eager|),
the joint replay test's (same launches on the same numbers; fp32 rounding room only).  State after the update: the two phases
without CPC issue identical launches and read nothing from a device scalar, so every tensor is bit-equal; the four with CPC read
the start index from a device scalar (the GRU runs all T/2 steps and gathers one, where the eager step stops at it), which moves
gradients in their last bits, and RMSprop's first step is lr·g/(0.1·|g| + eps) = ±10·lr whatever |g| — so a weight whose gradient
is rounding noise may step the other way.  There the full-batch joint test's gate applies to the parameters whose gradient is
real: at most 1 % of a tensor's elements off by more than 2e-3 of its scale.  (Measured in the default arithmetic: every
difference is zero, with CPC too; under FST_MATH=f32 the metric network's "ssl" is 6e-5 off on a weight of scale 0.2.)"""
import os
import types

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import ops
from test_gpu_dist import _build_small_trainer, _collect, _guarded
from test_gpu_modules import _joint_trainer, close, load

DEV = "cuda"
PHASES = ["target_pretrain", "source_pretrain", "ssl_with_ce", "ssl", "nf_with_ce", "nf"]
NO_CPC = ("source_pretrain", "nf")
LOSS_KEYS = ("nf_t", "nf_s", "ce_t", "sl_t", "ce_s", "sl_s")
JOINT_LOSSES = LOSS_KEYS + ("cdan", "ce_s2t2s", "fd_s")
# modules a phase runs (all in train mode): the BatchNorm buffers of those it runs WITHOUT stepping still move ("ssl": both classifiers)
RUNS = {"target_pretrain": ("fe_t", "cpc", "clf_t"), "source_pretrain": ("fe_s", "dimunif", "clf_s"),
        "ssl_with_ce": ("fe_t", "fe_s", "dimunif", "cpc", "clf_t", "clf_s"), "ssl": ("fe_t", "fe_s", "dimunif", "cpc", "clf_t", "clf_s"),
        "nf_with_ce": ("fe_t", "fe_s", "dimunif", "cpc", "clf_t", "clf_s", "nf"), "nf": ("fe_t", "fe_s", "dimunif", "nf")}
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")

_FIX = {}


def fixture(name):
    if name not in _FIX:
        _FIX[name] = load(name)
    return _FIX[name]


def toy():
    """(trainer, batch A, CPC indices A): the joint fixture's state, batch and indices — what the eager phase test runs."""
    g = fixture("joint_small")
    tr = _joint_trainer(g)
    args = [torch.tensor(g[f"s0.{k}"], device=DEV) for k in ("x_t", "y_t", "x_s", "y_s")]
    return tr, args, tuple(int(v) for v in g["s0.t_samples"])


def batch_b(args):
    """Another batch of the same shapes: other data, other labels (every class index stays valid: a permutation of A's)."""
    gen = torch.Generator().manual_seed(77)
    x_t, y_t, x_s, y_s = args
    return [torch.randn(x_t.shape, generator=gen).to(DEV), y_t.flip(0).contiguous(),
            torch.randn(x_s.shape, generator=gen).to(DEV), y_s.roll(1).contiguous()]


def clone(rep):
    return {k: v.clone() for k, v in rep.items()}


def same_losses(got, want, what, tol=1e-6):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        a, b = float(got[k]), float(want[k])
        print(f"{what} {k}: {a!r} vs {b!r} (diff {abs(a - b):.3e})")
        assert abs(a - b) <= tol * max(1.0, abs(b)), (what, k, a, b)


def real_gradient_gate(a, b, key, what):
    d = (a[key] - b[key]).abs()
    scale = float(b[key].abs().max())
    frac = float((d > 2e-3 * scale).double().mean())
    print(f"{what} {key}: max diff {float(d.max()):.3e}, scale {scale:.3e}, fraction beyond 2e-3 of it {frac:.4f}")
    assert frac < 0.01, (what, key, float(d.max()), scale)


def same_state(phase, after_graph, after_eager, what):
    """test 2's state gate: bit-equality without CPC; with it, the gradient-real parameters at the full-batch joint test's gate."""
    if phase in NO_CPC:
        differing = [k for k, v in after_eager.items() if not torch.equal(after_graph[k], v)]
        assert not differing, f"{what}: {len(differing)} state tensors differ, e.g. {differing[:5]}"
        return
    keys = ["m.fe_t.net_1.net.net.1.conv1d.weight", "m.cpc.Wk.0.weight"]
    if "clf_t" in fst.JointTrainer.PHASES[phase]:
        keys.append("m.clf_t.hidden.weight")
    for k in keys:
        real_gradient_gate(after_graph, after_eager, k, what)


def unstepped_untouched(phase, before, after, what):
    """Modules (and their optimiser moments) the phase does not step: bit-for-bit where they were, except the BatchNorm buffers
    of modules the phase runs."""
    stepped = fst.JointTrainer.PHASES[phase]
    checked = 0
    for k, v in before.items():
        part = k.split(".")
        if part[0] in ("m", "o") and part[1] in stepped:
            continue
        if part[0] == "m" and part[1] in RUNS[phase] and k.endswith(BN_BUFFERS):
            continue
        assert torch.equal(after[k], v), f"{what}: {k} moved although the phase does not step it"
        checked += 1
    assert checked > 0
    new = [k for k in after if k not in before]
    assert not new, f"{what}: the replay created state: {new[:5]}"


def replay_vs_eager(tr, phase, args, ts, what):
    """One replay, then — from the same snapshot — one eager step: the gates of test 2."""
    snap = tr.snapshot()
    rep = clone(tr.replay_phase(phase, *args, t_samples=ts))
    after_graph = tr.snapshot()["t"]
    tr.restore(snap)
    eager = tr.phase_step(phase, *args, t_samples=ts)
    same_losses(rep, eager, what)
    after_eager = tr.snapshot()["t"]
    same_state(phase, after_graph, after_eager, what)
    unstepped_untouched(phase, snap["t"], after_graph, what)
    return rep


# ------------------------------------------------------------------ 1. the reference's fixture
@pytest.mark.parametrize("phase", PHASES)
def test_captured_phase_golden(phase):
    """capture_phase leaves the trainer as it found it (parameters, BatchNorm buffers, optimiser moments; the RMSprop moments the
    warm-up created are zero, their initial value); one replay then gives the reference's losses and BatchNorm running mean."""
    ph = fixture("phases_small")
    tr, args, ts = toy()
    before = tr.snapshot()
    assert tr.capture_phase(phase, *args) is tr
    after = tr.snapshot()
    assert after["host"] == before["host"]
    for k, v in before["t"].items():
        assert torch.equal(after["t"][k], v), f"capture_phase moved {k}"
    created = [k for k in after["t"] if k not in before["t"]]
    assert created and all(k.endswith(".square_avg") for k in created), created[:5]
    assert all(not bool(after["t"][k].any()) for k in created), "a moment created by the warm-up is not back at zero"
    rep = tr.replay_phase(phase, *args, t_samples=ts)
    want_total = float(ph[f"{phase}.total"])
    assert abs(rep["total"].item() - want_total) <= 1e-4 * max(1.0, abs(want_total)), (rep["total"].item(), want_total)
    for k in LOSS_KEYS:
        if f"{phase}.loss.{k}" in ph:
            want = float(ph[f"{phase}.loss.{k}"])
            assert abs(rep[k].item() - want) <= 1e-4 * max(1.0, abs(want)), (k, rep[k].item(), want)
        else:
            assert k not in rep
    close(tr.m["clf_t"].state_dict()["net.0.bn.running_mean"], ph[f"{phase}.after.clf_t.bn_mean0"], 1e-4, "clf_t BN running mean")


# ------------------------------------------------------------------ 2. replay == eager
@pytest.mark.parametrize("phase", PHASES)
def test_phase_replay_equals_eager_step(phase):
    tr, args, ts = toy()
    tr.capture_phase(phase, *args)
    replay_vs_eager(tr, phase, args, ts, phase)


# ------------------------------------------------------------------ 3. run to run
# The joint step's FST_MATH=f32 relaxation (1e-5 on reports, state not compared) exists for ONE reason: RandomLayer's products fall
# back to a K-split GEMM whose slabs are added with float atomics.  No phase runs the CDAN branch: the weight gradients reduce slabs
# in a fixed order in both arithmetic modes, and two replays measured bit-identical under FST_MATH=f32 as well (all six phases, every
# report and state tensor).  So equality is asserted whatever the mode.
@pytest.mark.parametrize("phase", PHASES)
def test_phase_replay_is_repeatable(phase):
    tr, args, ts = toy()
    tr.capture_phase(phase, *args)
    snap = tr.snapshot()
    rep1 = clone(tr.replay_phase(phase, *args, t_samples=ts))
    state1 = tr.snapshot()["t"]
    tr.restore(snap)
    rep2 = tr.replay_phase(phase, *args, t_samples=ts)
    state2 = tr.snapshot()["t"]
    for k, v in rep1.items():
        print(f"{phase} two replays {k}: diff {float((rep2[k].double() - v.double()).abs().max()):.3e}")
        assert torch.equal(rep2[k], v), f"two replays differ in {k}"
    differing = [k for k, v in state1.items() if not torch.equal(state2[k], v)]
    assert not differing, f"two replays leave different state in {len(differing)} tensors, e.g. {differing[:5]}"


# ------------------------------------------------------------------ 4. the static inputs are refreshed
@pytest.mark.parametrize("phase", PHASES)
def test_phase_replay_reads_fresh_inputs(phase):
    """Captured on batch A, replayed on batch B (other data, labels and CPC indices): equals the eager step on B."""
    tr, args, ts = toy()
    tr.capture_phase(phase, *args)
    other, ts_b = batch_b(args), (5, 1)
    assert ts_b != ts and not torch.equal(other[1], args[1]) and not torch.equal(other[3], args[3])
    snap = tr.snapshot()
    on_a = clone(tr.replay_phase(phase, *args, t_samples=ts))
    tr.restore(snap)
    on_b = replay_vs_eager(tr, phase, other, ts_b, f"{phase} on batch B")
    assert abs(float(on_a["total"]) - float(on_b["total"])) > 1e-4, "batch B gives batch A's loss"


# ------------------------------------------------------------------ 5. several captures resident
def test_several_resident_captures():
    tr, args, ts = toy()
    tr.capture_phase("ssl", *args)
    tr.capture_phase("ssl_with_ce", *args)
    torch.manual_seed(5)
    tr.capture(*args, epoch=0)
    assert tr.captured_phases() == ("ssl", "ssl_with_ce")
    snap = tr.snapshot()
    seq = ("ssl", "ssl_with_ce", "ssl", "joint", "ssl")
    graph, held = [], None
    for i, what in enumerate(seq):
        if what == "joint":
            graph.append({k: v.clone() for k, v in tr.replay(*args, ts).items() if k in JOINT_LOSSES})
            continue
        rep = tr.replay_phase(what, *args, t_samples=ts)
        graph.append(clone(rep))
        if held is not None and held[0] != what:                           # the other phase's report survived this replay
            for k, v in held[2].items():
                assert torch.equal(held[1][k], v), f"position {i}: the report of {held[0]} changed under a replay of {what}"
        held = (what, rep, graph[-1])
    tr.restore(snap)
    for i, what in enumerate(seq):
        if what == "joint":
            eager = {k: v for k, v in tr.step(*args, epoch=0, t_samples=ts).items() if k in JOINT_LOSSES}
        else:
            eager = tr.phase_step(what, *args, t_samples=ts)
        same_losses(graph[i], eager, f"position {i} ({what})")
    tr.release_phase("ssl")
    assert tr.captured_phases() == ("ssl_with_ce",)
    with pytest.raises(RuntimeError):
        tr.replay_phase("ssl", *args, t_samples=ts)
    tr.replay_phase("ssl_with_ce", *args, t_samples=ts)                    # the other capture is still good
    tr.release_phase()
    assert tr.captured_phases() == ()


# ------------------------------------------------------------------ 6. errors, invalidation
def test_phase_capture_errors_and_invalidation():
    tr, args, ts = toy()
    with pytest.raises(ValueError, match="unknown phase"):
        tr.capture_phase("pretrain", *args)
    with pytest.raises(ValueError, match="unknown phase"):
        tr.replay_phase("pretrain", *args)
    with pytest.raises(RuntimeError):
        tr.replay_phase("nf", *args)
    tr.capture_phase("nf", *args)
    with pytest.raises(ValueError):
        tr.replay_phase("nf", args[0][:2], args[1][:2], args[2], args[3])
    with pytest.raises(ValueError):
        tr.replay_phase("nf", args[0], args[1].int(), args[2], args[3])
    assert tr.captured_phases() == ("nf",)
    tr.load_state_dict(tr.state_dict())
    assert tr.captured_phases() == ()
    with pytest.raises(RuntimeError):
        tr.replay_phase("nf", *args)
    tr.capture_phase("nf", *args)
    replay_vs_eager(tr, "nf", args, ts, "nf after load_state_dict")
    tr.capture_phase("nf", *args)                                          # capturing again replaces the graph
    assert tr.captured_phases() == ("nf",)
    replay_vs_eager(tr, "nf", args, ts, "nf captured again")


def test_global_sync_over_several_ranks_is_not_captured():
    """Mode B puts collectives inside autograd: with more than one rank capture_phase raises, as capture() does (a stubbed
    world size: the branch needs no second process)."""
    tr, args, _ = toy()
    tr.bucket, tr.sync = types.SimpleNamespace(world=2), "global"
    with pytest.raises(RuntimeError, match="global"):
        tr.capture_phase("ssl", *args)
    assert tr.captured_phases() == ()


# ------------------------------------------------------------------ 7. data parallel, one rank over RCCL
DP_PHASES = ("ssl_with_ce", "nf")


def _worker_phase_rccl(rank, world, port, q):
    """One rank, backend "nccl" (= RCCL), the bucket forced to issue its collective: a phase captured with a bucket is two graphs
    with the eager all-reduce between them, and computes what the bucket-less capture computes from the same state."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    g = fixture("joint_small")
    args = [torch.tensor(g[f"s0.{k}"], device=dev) for k in ("x_t", "y_t", "x_s", "y_s")]
    ts = tuple(int(v) for v in g["s0.t_samples"])
    ref, _ = _build_small_trainer(fst, dev, None, "ddp")
    out = {}
    for sync in ("ddp", "global"):
        tr, _ = _build_small_trainer(fst, dev, fst.GradBucket(always_reduce=True), sync)
        for phase in DP_PHASES:
            start = {id(t): t.snapshot() for t in (tr, ref)}              # both trainers hold the fixture's state here
            tr.capture_phase(phase, *args)
            ref.capture_phase(phase, *args)
            n_graphs = (len(tr._phase[phase]["graphs"]), len(ref._phase[phase]["graphs"]))
            a = {k: float(v) for k, v in tr.replay_phase(phase, *args, t_samples=ts).items()}
            b = {k: float(v) for k, v in ref.replay_phase(phase, *args, t_samples=ts).items()}
            sa, sb = tr.snapshot()["t"], ref.snapshot()["t"]
            keys = [k for k in sb if k.startswith("m.nf.")] if phase == "nf" else \
                ["m.fe_t.net_1.net.net.1.conv1d.weight", "m.cpc.Wk.0.weight", "m.clf_t.hidden.weight"]
            worst = max(float(((sa[k] - sb[k]).abs() > 2e-3 * float(sb[k].abs().max())).double().mean()) for k in keys)
            moved = any(not torch.equal(sb[k], start[id(ref)]["t"][k]) for k in keys)
            out[(sync, phase)] = (n_graphs, a, b, worst, moved)
            for t in (tr, ref):
                t.release_phase()
                t.restore(start[id(t)], new_to_zero=True)              # the moments the captures created: back to zero
    q.put((0, out))
    dist.destroy_process_group()


def _run_worker(name, rank, world, port, q):
    _guarded(globals()[name])(rank, world, port, q)


def test_data_parallel_phase_capture_on_one_rccl_rank():
    world, port = 1, 29683
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_worker, args=("_worker_phase_rccl", 0, world, port, q))]
    procs[0].start()
    (_, out), = _collect(q, world, procs)
    assert set(out) == {(s, p) for s in ("ddp", "global") for p in DP_PHASES}
    for (sync, phase), (n_graphs, a, b, worst, moved) in out.items():
        assert n_graphs == (2, 1), (sync, phase, n_graphs)
        same_losses(a, b, f"{sync} {phase} bucket vs none")
        print(f"{sync} {phase}: largest fraction of a parameter beyond 2e-3 of its scale {worst:.4f}")
        assert worst < 0.01 and moved, (sync, phase, worst, moved)


# ------------------------------------------------------------------ 8. the metric network
def test_metric_network_phases_replay_equals_eager():
    """JointConfig(L=512) at B=4: the smallest shape with the persistent WN stack kernels, the window conv kernels and the
    persistent GRU inside a phase capture."""
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=512, L_s=512, dropout_p=0.0), DEV)
    gen = torch.Generator().manual_seed(7)

    def pair():
        x = torch.randn(4, 1, 512, generator=gen)
        return ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)).to(DEV), torch.randint(4, (4,), generator=gen).to(DEV)
    (x_t, y_t), (x_s, y_s) = pair(), pair()
    args = (x_t, y_t, x_s, y_s)
    for phase in ("nf", "ssl"):
        tr.capture_phase(phase, *args)
    assert tr.captured_phases() == ("nf", "ssl")
    for phase in ("nf", "ssl"):
        replay_vs_eager(tr, phase, args, (31, 77), f"metric network {phase}")
