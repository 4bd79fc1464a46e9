"""The one-source-frame training step (`--frame_ids 0 -1`, what DDAD's two-frame items train with), host side: the pose
planner, the model's pose plan and the fixtures written by the REFERENCE's unmodified process_batch + backward
(tools/gen_ddad_step_golden.py)."""
import pytest
import torch

MASK_MEAN = (0.05, 0.95)          # tools/gen_ddad_step_golden.py: both branches of the consistency mask are exercised


def test_step_planner_serves_the_one_source_frame_step():
    from ppeadepth.networks.repdepth import PoseFrame, PosePlan, pose_pair_plan, pose_step_plan
    plan = pose_step_plan([0, -1], [0, -1])
    assert isinstance(plan, PosePlan)
    assert plan.pairs == [(-1, 0)]
    assert plan.frames == [PoseFrame(-1, 0, True, -1, True)]
    assert plan.updates == [("grad", 0), ("replay", 0)]           # the reference's order: the gradient pass, then the replay
    # [0, -1, 1] by delegation, for every set of lookup frames the pair planner serves
    for ids in ([0, -1], [0, 1, -1], [0, -1, -2], [0, 1, -1, -2, -3]):
        assert pose_step_plan([0, -1, 1], ids) == pose_pair_plan([0, -1, 1], ids)


@pytest.mark.parametrize("frame_ids,matching_ids", [([0, -1], [0, 1, -1]), ([0, -1], [0, -1, -2]), ([0, -1], [0]),
                                                    ([0, -1], [0, 1]), ([0, 1], [0, -1]), ([0, 1], [0, 1]),
                                                    ([0, -1, 1, -2], [0, -1]), ([0, -2, -1], [0, -1]),
                                                    ([0, -1, 1], [0, -2]), ([0, -1, 1], [-1, 0])])
def test_step_planner_refuses_everything_else(frame_ids, matching_ids):
    from ppeadepth.networks.repdepth import pose_step_plan
    with pytest.raises(ValueError):
        pose_step_plan(frame_ids, matching_ids)


def test_pair_planner_keeps_its_contract():
    from ppeadepth.networks.repdepth import pose_pair_plan
    with pytest.raises(ValueError, match=r"frame_ids \[0, -1, 1\]"):
        pose_pair_plan([0, -1], [0, -1])


def test_model_with_one_source_frame_has_a_pose_plan():
    from ppeadepth import networks, options
    opt = options.default_options(height=64, width=96, batch_size=2, use_checkpoint=False, frame_ids=[0, -1],
                                  selec_reproj=False)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    plan = model.pose_plan()
    assert plan is not None and plan.pairs == [(-1, 0)] and plan.updates == [("grad", 0), ("replay", 0)]
    # still none for what is unserved
    model.matching_ids = [0, -1, -2]
    assert model.pose_plan() is None


@pytest.mark.parametrize("name", ["e2e_ddad_small", "e2e_ddad_small_c"])
def test_ddad_step_fixtures_hold_one_source_frame(golden, name):
    g = golden(name)
    assert [int(v) for v in g["meta"]] == [2, 64, 96, 2, 1]
    assert "out:cam_T_cam|0|-1" in g and "out:color|-1|0" in g and "out:sample|-1|0" in g and "in:relative_pose|-1" in g
    frame1 = [k for k in g if k.startswith(("out:cam_T_cam|0|1", "out:axisangle|0|1", "out:translation|0|1", "out:color|1|",
                                            "out:sample|1|", "out:color_identity|1|"))]
    assert not frame1, frame1
    dead = [k for k in g if k.startswith("grad_abs:") and float(g[k]) == 0.0]
    assert len([k for k in g if k.startswith("grad_abs:")]) == 15 and not dead, dead
    if name == "e2e_ddad_small":
        mean = float(g["out:consistency_mask"].float().mean())
        assert MASK_MEAN[0] <= mean <= MASK_MEAN[1], mean
        assert sorted(float(v) for v in g["out:augmentation_mask"].flatten()) == [0.0, 1.0]   # both mask branches
