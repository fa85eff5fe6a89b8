"""Device-resident datasets on the CPU branch of ``ops.feed_batch``: ``DeviceDataset`` / ``EpochFeeder`` against ``DeviceLoader`` for
the same generator state, the order of the generator draws, the rank slices, the end of a plan, bad indices, the checkpoint round
trip and ``NoiseTransfer.planned_ratios`` against ``advance``.  Everything is compared with ``torch.equal`` (on int32 views where
the bits matter): a gather copies, it does not compute."""
import os
import re

import pytest
import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = "cpu"


def dataset(n, c=2, l=5, seed=0, classes=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, l, generator=g, dtype=torch.float64), torch.randint(classes, (n,), generator=g)


def bits(t):
    return t.contiguous().view(torch.int32)


def buffers(feeder):
    out = []
    for d, b in zip(feeder.sets, feeder.batch):
        out += [torch.full((b,) + tuple(d.x.shape[1:]), 7.0), torch.full((b,), -7, dtype=torch.int64)]
    return out


def drain(feeder, rounds, scalars=False):
    """The next ``rounds`` rounds as clones (with ``scalars``: t and r behind the batch)."""
    got = []
    bufs, t, r = buffers(feeder), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    for _ in range(rounds):
        feeder.feed(*bufs, t=t, r=r)
        got.append(tuple(b.clone() for b in bufs) + ((t.clone(), r.clone()) if scalars else ()))
    return got


def test_abi_version_and_symbol():
    text = open(os.path.join(ROOT, "include", "fst_hip.h")).read()
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 25
    assert "fst_feed_batch" in _lib.EXPORTED_SYMBOLS
    for name in ("DeviceDataset", "EpochFeeder", "feed_batch"):
        assert hasattr(fst, name), name


def test_device_dataset_casts_once_and_batches_are_views():
    x, y = dataset(10)
    ds = fst.DeviceDataset(x, y.to(torch.int32), CPU)
    assert ds.x.dtype == torch.float32 and ds.y.dtype == torch.int64 and ds.x.is_contiguous() and len(ds) == 10
    assert torch.equal(ds.x, x.float()) and torch.equal(ds.y, y)
    got = list(ds.batches(4))
    assert [b[0].size(0) for b in got] == [4, 4, 2]
    assert torch.equal(torch.cat([b[0] for b in got]), ds.x) and torch.equal(torch.cat([b[1] for b in got]), ds.y)
    assert all(b[0].data_ptr() == ds.x[4 * i].data_ptr() for i, b in enumerate(got))          # views: nothing was copied
    with pytest.raises(ValueError):
        fst.DeviceDataset(x, y[:-1], CPU)


@pytest.mark.parametrize("n_t,n_s,b_t,b_s", [(10, 10, 3, 3),       # a tail of one series is dropped
                                             (11, 7, 3, 3),        # N_s < N_t: the rounds follow the shorter side
                                             (12, 9, 4, 2),        # unequal batch sizes; the target side is the shorter one
                                             (9, 20, 2, 5)])
def test_epoch_equals_device_loader(n_t, n_s, b_t, b_s):
    (x_t, y_t), (x_s, y_s) = dataset(n_t, seed=1), dataset(n_s, c=3, l=4, seed=2)
    feeder = fst.EpochFeeder(fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU), batch_size=(b_t, b_s),
                             generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(5)
    for epoch in range(2):                                                     # the second epoch: the generator ran on
        rounds = feeder.begin_epoch()
        assert rounds == min(n_t // b_t, n_s // b_s) == feeder.rounds
        # the loaders draw their permutation at the first next(): target first, then source, as the feeder does
        want_t = list(fst.DeviceLoader(x_t, y_t, b_t, CPU, generator=gen, drop_last=True))
        want_s = list(fst.DeviceLoader(x_s, y_s, b_s, CPU, generator=gen, drop_last=True))
        got = drain(feeder, rounds)
        for i in range(rounds):
            for a, b in zip(got[i], want_t[i] + want_s[i]):
                assert a.dtype == b.dtype and torch.equal(bits(a), bits(b)), (epoch, i)
        with pytest.raises(StopIteration):
            feeder.feed(*buffers(feeder))
        feeder.check()
        words = feeder.counters()
        assert int(words[ops.FEED_CURSOR]) == rounds == int(words[ops.FEED_STEPS]) and int(words[ops.FEED_FED]) == (epoch + 1) * rounds


def test_single_batch_size_and_target_only_feeder():
    x, y = dataset(10, seed=3)
    feeder = fst.EpochFeeder(fst.DeviceDataset(x, y, CPU), batch_size=3, generator=torch.Generator().manual_seed(9))
    assert feeder.begin_epoch() == 3
    want = list(fst.DeviceLoader(x, y, 3, CPU, generator=torch.Generator().manual_seed(9), drop_last=True))
    for (gx, gy), (wx, wy) in zip(drain(feeder, 3), want):
        assert torch.equal(bits(gx), bits(wx)) and torch.equal(gy, wy)


def test_order_of_draws():
    """randperm(N_t), randperm(N_s), randint(cpc_timestep // 2, (rounds, 2)), in this order, from the feeder's generator."""
    (x_t, y_t), (x_s, y_s) = dataset(10, seed=1), dataset(8, seed=2)
    feeder = fst.EpochFeeder(fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU), batch_size=(3, 2),
                             generator=torch.Generator().manual_seed(11), cpc_timestep=12)
    rounds = feeder.begin_epoch(ratios=[(1.0, 1.0), (0.1, 1 / 3), (3 / 7, 0.7)])
    gen = torch.Generator().manual_seed(11)
    p_t, p_s = torch.randperm(10, generator=gen), torch.randperm(8, generator=gen)
    t = torch.randint(6, (rounds, 2), generator=gen)
    assert rounds == 3
    want_r = torch.tensor([(1.0, 1.0), (0.1, 1 / 3), (3 / 7, 0.7)], dtype=torch.float64).float()
    for i, (gx_t, gy_t, gx_s, gy_s, gt, gr) in enumerate(drain(feeder, rounds, scalars=True)):
        assert torch.equal(gx_t, x_t.float()[p_t[3 * i: 3 * i + 3]]) and torch.equal(gy_t, y_t[p_t[3 * i: 3 * i + 3]])
        assert torch.equal(gx_s, x_s.float()[p_s[2 * i: 2 * i + 2]]) and torch.equal(gy_s, y_s[p_s[2 * i: 2 * i + 2]])
        assert gt.dtype == torch.int32 and torch.equal(gt.long(), t[i])
        assert torch.equal(bits(gr), bits(want_r[i]))
    # the generator stands where the three draws left it
    assert torch.equal(feeder.generator.get_state(), gen.get_state())


def test_no_shuffle_draws_only_the_cpc_indices():
    (x_t, y_t), (x_s, y_s) = dataset(7, seed=1), dataset(9, seed=2)
    feeder = fst.EpochFeeder(fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU), batch_size=2,
                             generator=torch.Generator().manual_seed(4), shuffle=False, cpc_timestep=9)
    rounds = feeder.begin_epoch()
    t = torch.randint(4, (rounds, 2), generator=torch.Generator().manual_seed(4))
    for i, (gx_t, gy_t, gx_s, gy_s, gt, gr) in enumerate(drain(feeder, rounds, scalars=True)):
        assert torch.equal(gx_t, x_t.float()[2 * i: 2 * i + 2]) and torch.equal(gy_s, y_s[2 * i: 2 * i + 2])
        assert torch.equal(gt.long(), t[i]) and torch.equal(gr, torch.ones(2))


def test_two_ranks_concatenated_are_the_single_rank_batches_of_twice_the_size():
    (x_t, y_t), (x_s, y_s) = dataset(21, seed=1), dataset(17, seed=2)
    sets = fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU)
    B = (3, 2)
    whole = fst.EpochFeeder(*sets, batch_size=(2 * B[0], 2 * B[1]), generator=torch.Generator().manual_seed(6), cpc_timestep=8)
    ranks = [fst.EpochFeeder(*sets, batch_size=B, generator=torch.Generator().manual_seed(6), cpc_timestep=8, rank=r, world=2)
             for r in range(2)]
    rounds = whole.begin_epoch()
    assert [f.begin_epoch() for f in ranks] == [rounds, rounds] and rounds == 3
    want = drain(whole, rounds, scalars=True)
    got = [drain(f, rounds, scalars=True) for f in ranks]
    for i in range(rounds):
        for k in range(4):
            assert torch.equal(torch.cat([got[0][i][k], got[1][i][k]]), want[i][k]), (i, k)
        assert torch.equal(got[0][i][4], want[i][4]) and torch.equal(got[1][i][4], want[i][4])       # the same CPC indices on every rank


def raw_call(n=6, batch=4, steps=2, index=None):
    src_x = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) + 0.5
    src_y = torch.arange(n, dtype=torch.int64) + 100
    if index is None:
        index = torch.tensor([[1, 0, 5, 2], [3, 3, 4, 0]], dtype=torch.int32)
    dst_x, dst_y = torch.full((batch, 3), -1.0), torch.full((batch,), -1, dtype=torch.int64)
    table = torch.tensor([[11, 12], [21, 22]], dtype=torch.int32)
    out = torch.full((2,), -1, dtype=torch.int32)
    state = torch.zeros(8, dtype=torch.int32)
    state[ops.FEED_STEPS] = steps
    streams = [(src_x, dst_x, index), (src_y, dst_y, index)]
    scalars = [(table, out[0:1]), (table, out[1:2])]
    return streams, scalars, state, (src_x, src_y, dst_x, dst_y, out)


def test_raw_feed_serves_rows_and_overruns_without_writing():
    streams, scalars, state, (src_x, src_y, dst_x, dst_y, out) = raw_call()
    ops.feed_batch(streams, scalars, state)
    assert torch.equal(dst_x, src_x[[1, 0, 5, 2]]) and torch.equal(dst_y, src_y[[1, 0, 5, 2]]) and out.tolist() == [11, 12]
    assert state.tolist() == [1, 2, 1, 0, 0, 0, 0, 0]
    ops.feed_batch(streams, scalars, state)
    assert torch.equal(dst_x, src_x[[3, 3, 4, 0]]) and torch.equal(dst_y, src_y[[3, 3, 4, 0]]) and out.tolist() == [21, 22]
    assert state.tolist() == [2, 2, 2, 0, 0, 0, 0, 0]
    dst_x.fill_(-3.0); dst_y.fill_(-3); out.fill_(-3)
    ops.feed_batch(streams, scalars, state)                                   # cursor == steps
    assert (dst_x == -3).all() and (dst_y == -3).all() and (out == -3).all()
    assert state.tolist() == [2, 2, 2, 1, 0, 0, 0, 0]


def test_bad_indices_are_skipped_counted_and_reported():
    index = torch.tensor([[1, -1, 6, 2], [0, 0, 0, 0]], dtype=torch.int32)     # -1 and N = 6
    streams, scalars, state, (src_x, src_y, dst_x, dst_y, out) = raw_call(index=index)
    ops.feed_batch(streams[:1], scalars, state)
    assert torch.equal(dst_x[[0, 3]], src_x[[1, 2]]) and (dst_x[[1, 2]] == -1).all()
    assert state.tolist() == [1, 2, 1, 0, 2, 0, 0, 0]
    x, y = dataset(6)
    feeder = fst.EpochFeeder(fst.DeviceDataset(x, y, CPU), batch_size=2, generator=torch.Generator().manual_seed(1))
    feeder.begin_epoch()
    feeder.check()
    feeder._plan[0] = 6                                                        # corrupt the uploaded plan: an index of N
    bufs = buffers(feeder)
    feeder.feed(*bufs)
    assert (bufs[0][0] == 7.0).all() and bufs[1][0] == -7 and not (bufs[0][1] == 7.0).all()
    with pytest.raises(RuntimeError, match="outside"):
        feeder.check()


def test_feed_batch_refuses_bad_arguments():
    streams, scalars, state, _ = raw_call()
    with pytest.raises(ValueError):
        ops.feed_batch(streams * 5, scalars, state)                            # 10 streams
    with pytest.raises(ValueError):
        ops.feed_batch(streams, scalars, state[:7])
    with pytest.raises(ValueError):
        ops.feed_batch([(streams[0][0], streams[0][1], streams[0][2].long())], [], state)
    with pytest.raises(ValueError):
        ops.feed_batch([(streams[0][0], streams[1][1], streams[0][2])], [], state)      # fp32 source, int64 destination
    with pytest.raises(ValueError):
        ops.feed_batch(streams, scalars[:1], state)                            # a [steps, 2] table for one scalar
    assert state.tolist() == [0, 2, 0, 0, 0, 0, 0, 0]


def test_state_dict_round_trip_mid_epoch():
    (x_t, y_t), (x_s, y_s) = dataset(16, seed=1), dataset(11, seed=2)
    sets = fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU)
    a = fst.EpochFeeder(*sets, batch_size=(3, 2), generator=torch.Generator().manual_seed(8), cpc_timestep=10)
    assert a.begin_epoch(ratios=[(1 / (i + 1), 1 / (i + 2)) for i in range(5)]) == 5
    drain(a, 2)
    sd = a.state_dict()
    rest = drain(a, 3, scalars=True)
    next_epoch_rounds = a.begin_epoch()
    nxt = drain(a, next_epoch_rounds, scalars=True)
    b = fst.EpochFeeder(*sets, batch_size=(3, 2), generator=torch.Generator().manual_seed(12345), cpc_timestep=10)
    b.load_state_dict(sd)
    assert (b.epoch, b.cursor, b.steps) == (1, 2, 5)
    got = drain(b, 3, scalars=True)
    with pytest.raises(StopIteration):
        b.feed(*buffers(b))
    for g, w in zip(got, rest):
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(g, w))
    assert b.begin_epoch() == next_epoch_rounds                                # the generator state came along: the same next epoch
    for g, w in zip(drain(b, next_epoch_rounds, scalars=True), nxt):
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(g, w))
    b.check()
    with pytest.raises(ValueError):
        fst.EpochFeeder(*sets, batch_size=(3, 3), generator=torch.Generator()).load_state_dict(sd)


def test_peek_is_row_zero_and_moves_nothing():
    (x_t, y_t), (x_s, y_s) = dataset(9, seed=1), dataset(9, seed=2)
    f = fst.EpochFeeder(fst.DeviceDataset(x_t, y_t, CPU), fst.DeviceDataset(x_s, y_s, CPU), batch_size=4,
                        generator=torch.Generator().manual_seed(2), cpc_timestep=6)
    with pytest.raises(RuntimeError):
        f.peek()
    with pytest.raises(RuntimeError):
        f.feed(*buffers(f))
    f.begin_epoch(ratios=[(0.5, 0.25), (0.125, 2.0)])
    before = f.counters().clone()
    peeked = f.peek()
    assert torch.equal(f.counters(), before) and f.cursor == 0
    first = drain(f, 1, scalars=True)[0]
    assert all(p.dtype == q.dtype and torch.equal(bits(p), bits(q)) for p, q in zip(peeked, first))


def test_planned_ratios_equal_advance_to_the_bit_and_leave_the_counters():
    for start in (0, 1, 4):                                                   # from a fresh module, after one call, mid-run
        noise, twin = fst.NoiseTransfer(2, 4), fst.NoiseTransfer(2, 4)
        for _ in range(start):
            noise.advance(5, 3); twin.advance(5, 3)
        before = (noise.time, noise.cal_num_target, noise.cal_num_source)
        plan = noise.planned_ratios(6, 7, 3)
        assert (noise.time, noise.cal_num_target, noise.cal_num_source) == before
        want = [twin.advance(7, 3) for _ in range(6)]
        assert plan == want                                                    # the same Python floats ...
        a, b = torch.tensor(plan, dtype=torch.float64).float(), torch.tensor(want, dtype=torch.float64).float()
        assert torch.equal(bits(a), bits(b))                                   # ... so the same float32 words
        # and the words the feeder uploads are those
        x, y = dataset(42, seed=start)
        f = fst.EpochFeeder(fst.DeviceDataset(x, y, CPU), fst.DeviceDataset(x, y, CPU), batch_size=(7, 3), generator=torch.Generator())
        assert f.begin_epoch(ratios=plan) == 6
        assert torch.equal(bits(torch.stack([row[5] for row in drain(f, 6, scalars=True)])), bits(b))
