"""SharedStepAdam == torch.optim.Adam (same update formula, one shared step counter) on a bag of small tensors that all
receive a gradient every step — the only way the hot path uses it (a tensor that skipped a step would keep its own
counter in torch's Adam, which is exactly the per-tensor state this optimiser does away with)."""
import torch

from feature_level_style_transfer_for_tsc_amd.optim import SharedStepAdam


def test_matches_torch_adam_over_several_steps():
    g = torch.Generator().manual_seed(0)
    shapes = [(5, 3), (7,), (2, 4, 3), (1,)] * 5
    a = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ref, mine = torch.optim.Adam(a, lr=0.002), SharedStepAdam(b, lr=0.002)
    for step in range(7):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g) * (10.0 ** (step % 3 - 1))
            pa.grad, pb.grad = gr.clone(), gr.clone()
        ref.step(); mine.step()
        for pa, pb in zip(a, b):
            assert torch.allclose(pa, pb, rtol=2e-6, atol=1e-7), step
    assert float(mine.param_groups[0]["step"]) == 7.0
    assert mine.state[b[0]]["step"] is mine.param_groups[0]["step"]  # exposed for state snapshots


def test_fused_rmsprop_host_logic_matches_torch_rmsprop():
    """FusedRMSprop / rmsprop_step_many (CPU branch = the same formula the HIP kernel implements, in torch's operation order):
    several optimisers with different learning rates stepped together equal torch.optim.RMSprop stepped one by one; a
    parameter without a gradient is skipped; state_dict round trip."""
    from feature_level_style_transfer_for_tsc_amd.optim import FusedRMSprop, rmsprop_step_many
    g = torch.Generator().manual_seed(1)
    mk = lambda shapes: [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    a1, a2 = mk([(4, 3), (6,)]), mk([(2, 2, 2), (5,)])
    b1, b2 = [torch.nn.Parameter(p.detach().clone()) for p in a1], [torch.nn.Parameter(p.detach().clone()) for p in a2]
    refs = [torch.optim.RMSprop(a1, lr=0.001), torch.optim.RMSprop(a2, lr=0.003)]
    mine = [FusedRMSprop(b1, lr=0.001), FusedRMSprop(b2, lr=0.003)]
    for step in range(5):
        for pa, pb in zip(a1 + a2, b1 + b2):
            gr = torch.randn(pa.shape, generator=g)
            pa.grad, pb.grad = gr.clone(), gr.clone()
        if step == 2:
            a2[1].grad = b2[1].grad = None
        for r in refs:
            r.step()
        rmsprop_step_many(mine)
        for pa, pb in zip(a1 + a2, b1 + b2):
            assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7), step
    sd = mine[0].state_dict()
    fresh = FusedRMSprop([torch.nn.Parameter(p.detach().clone()) for p in b1], lr=0.001)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.state[fresh.param_groups[0]["params"][0]]["square_avg"], mine[0].state[b1[0]]["square_avg"])


def test_push_words_writes_a_slice_in_place():
    from feature_level_style_transfer_for_tsc_amd.optim import push_words
    words = torch.zeros(4, dtype=torch.int32)
    push_words(words[:2], torch.tensor([7, 9], dtype=torch.int32))
    assert words.tolist() == [7, 9, 0, 0]


def test_exchanged_swaps_back_and_restores_flag_and_caches_even_when_the_body_raises():
    import pytest
    from types import SimpleNamespace
    from feature_level_style_transfer_for_tsc_amd import ops
    from feature_level_style_transfer_for_tsc_amd.optim import exchanged
    a, b = [torch.tensor([1.0, 2.0])], [torch.tensor([3.0, 4.0])]
    owner, cache = SimpleNamespace(inside=False), SimpleNamespace(W_inverse="live")
    with pytest.raises(KeyError):
        with exchanged(a, b, [cache], owner, "inside", "scope()") as got:
            assert got is owner and owner.inside and not hasattr(cache, "W_inverse")
            assert a[0].tolist() == [3.0, 4.0] and b[0].tolist() == [1.0, 2.0]
            cache.W_inverse = "of the exchanged weights"
            with pytest.raises(RuntimeError, match=r"scope\(\).*nest"):
                exchanged(a, b, [cache], owner, "inside", "scope()").__enter__()
            raise KeyError("body")
    assert not owner.inside and cache.W_inverse == "live" and a[0].tolist() == [1.0, 2.0] and b[0].tolist() == [3.0, 4.0]
    with ops.pack_cache():
        with pytest.raises(RuntimeError, match=r"scope\(\).*pack_cache"):
            exchanged(a, b, [], owner, "inside", "scope()").__enter__()
    assert a[0].tolist() == [1.0, 2.0] and not owner.inside
