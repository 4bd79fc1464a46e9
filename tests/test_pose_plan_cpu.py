"""`repdepth.pose_pair_plan`: which pose pairs the lookup frames need, which of them are the gradient passes again (replayed
as a running-statistics update, not recomputed), the chain's predecessors, and the order of the running-statistics updates
-- the reference's (repdepth.py:443-509): gradient passes in `frame_ids[1:]` order, then the no_grad passes in
`matching_ids[1:]` order."""
import pytest
import torch

FRAME_IDS = [0, -1, 1]
GRAD = [("grad", 0), ("grad", 1)]               # pairs (-1, 0) and (0, 1)

# matching_ids -> (pairs, frames as (frame, pair, invert, pred, replay), no_grad updates)
EXPECTED = {
    (0, -1): ([(-1, 0), (0, 1)],
              [(-1, 0, True, -1, True)],
              [("replay", 0)]),
    (0, 1, -1): ([(-1, 0), (0, 1)],
                 [(1, 1, False, -1, True), (-1, 0, True, -1, True)],
                 [("replay", 1), ("replay", 0)]),
    (0, -1, -2): ([(-1, 0), (0, 1), (-2, -1)],
                  [(-1, 0, True, -1, True), (-2, 2, True, 0, False)],
                  [("replay", 0), ("new", 2)]),
    (0, -1, -2, -3): ([(-1, 0), (0, 1), (-2, -1), (-3, -2)],
                      [(-1, 0, True, -1, True), (-2, 2, True, 0, False), (-3, 3, True, 1, False)],
                      [("replay", 0), ("new", 2), ("new", 3)]),
    (0, 1, -1, -2, -3): ([(-1, 0), (0, 1), (-2, -1), (-3, -2)],
                         [(1, 1, False, -1, True), (-1, 0, True, -1, True), (-2, 2, True, 1, False), (-3, 3, True, 2, False)],
                         [("replay", 1), ("replay", 0), ("new", 2), ("new", 3)]),
}
NEW_PASSES = {(0, -1): 0, (0, 1, -1): 0, (0, -1, -2): 1, (0, -1, -2, -3): 2, (0, 1, -1, -2, -3): 2}


@pytest.mark.parametrize("ids", list(EXPECTED))
def test_pose_pair_plan(ids):
    from ppeadepth.networks.repdepth import pose_pair_plan
    plan = pose_pair_plan(FRAME_IDS, list(ids))
    pairs, frames, updates = EXPECTED[ids]
    assert plan.pairs == pairs
    assert [tuple(f) for f in plan.frames] == frames
    assert [f.frame for f in plan.frames] == list(ids[1:])
    # gradient passes first, in frame_ids[1:] order; then one update per lookup frame, in matching_ids[1:] order
    assert plan.updates == GRAD + updates
    assert [plan.pairs[p] for _, p in plan.updates[:2]] == [(-1, 0), (0, 1)]
    assert [p for _, p in plan.updates[2:]] == [f.pair for f in plan.frames]
    assert sum(kind == "new" for kind, _ in plan.updates) == NEW_PASSES[ids]
    for f in plan.frames:
        a, b = plan.pairs[f.pair]
        assert b == a + 1 and f.frame in (a, b)                          # temporal order, and the frame is in its pair
        assert (f.frame, f.invert) == ((a, True) if f.frame < 0 else (b, False))
        assert f.replay == (plan.pairs[f.pair] in [(-1, 0), (0, 1)])
        near = a if f.frame > 0 else b
        assert (f.pred == -1 and near == 0) or plan.frames[f.pred].frame == near
        assert f.pred < plan.frames.index(f)                             # predecessors first: one pass over the chain


@pytest.mark.parametrize("frame_ids,ids", [([0, -1], [0, -1]), ([0, -2, -1, 1, 2], [0, -1]), ([0, -1, 1], [0, -2]),
                                           ([0, -1, 1], [0, -2, -1]), ([0, -1, 1], [0]), ([0, -1, 1], [0, -1, -2, -3, -4, -5])])
def test_pose_pair_plan_refuses_what_the_batched_path_does_not_serve(frame_ids, ids):
    from ppeadepth.networks.repdepth import pose_pair_plan
    with pytest.raises(ValueError):
        pose_pair_plan(frame_ids, ids)


def test_host_pose_chain_equals_the_sequential_composite():
    """`layers.pose_chain` on the host (the device path is one HIP launch, tests/test_multiframe_train_gpu.py): the chain
    0 -> -1 -> -2 with item 1's frame -1 missing; frame -2 of that item is zero too, as in the reference."""
    from ppeadepth.layers import pose_chain, transformation_from_parameters
    g = torch.Generator().manual_seed(0)
    pairs = [(0.3 * torch.randn(3, 1, 3, generator=g), torch.randn(3, 1, 3, generator=g)) for _ in range(2)]
    keep = torch.ones(3, 2)
    keep[1, 0] = 0
    rel = pose_chain(pairs, [(0, True, -1), (1, True, 0)], keep)
    first = transformation_from_parameters(*pairs[0], invert=True) * keep[:, 0, None, None]
    second = torch.matmul(transformation_from_parameters(*pairs[1], invert=True), first)
    assert rel.shape == (3, 2, 4, 4)
    assert torch.equal(rel[:, 0], first) and torch.equal(rel[:, 1], second)
    assert float(rel[1].abs().sum()) == 0 and float(rel[0, 1].abs().sum()) > 0
