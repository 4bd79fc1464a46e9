"""TEST INFRASTRUCTURE ONLY -- the DDAD training-step fixtures (one source frame: `--frame_ids 0 -1`), from the REFERENCE
itself.

    python tools/gen_ddad_step_golden.py

Runs only where the reference tree exists (oracle.ref_harness.reference_available).  Writes
  tests/golden/e2e_ddad_small.npz     the reference's unmodified Trainer.process_batch + backward at B = 2, 64 x 96 with
                                      `--frame_ids 0 -1 --selec_reproj` (oracle.gen_golden.gen_e2e).  `--selec_reproj` is
                                      store_false: with the default (on) the reference reads the warped frame +1
                                      (trainer.py:1077-1083), which a two-frame item does not have
  tests/golden/e2e_ddad_small_c.npz   the same on the well-conditioned construction (rendered frames, conditioned=True):
                                      the fixture the bf16 step is held to absolute bounds on
Only arrays and key names are stored.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

EXTRA = ["--frame_ids", "0", "-1", "--selec_reproj"]
MASK_MEAN = (0.05, 0.95)      # both branches of the consistency mask are exercised (e2e_small: 0.137)


def main():
    if not rh.reference_available():
        raise SystemExit("reference tree not present: goldens can only be regenerated in the build container")
    rh.install_stubs()
    torch.set_num_threads(8)
    gg.gen_e2e("e2e_ddad_small", 2, 64, 96, extra=EXTRA, stride=2)
    gg.gen_e2e("e2e_ddad_small_c", 2, 64, 96, extra=EXTRA, stride=2, conditioned=True)
    ref = os.path.getsize(os.path.join(gg.OUT, "e2e_small.npz"))
    for name in ("e2e_ddad_small", "e2e_ddad_small_c"):
        got = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
        print(f"{name}.npz {got} bytes (e2e_small.npz: {ref})")
        assert got <= ref, f"{name}.npz larger than e2e_small.npz"
        z = np.load(os.path.join(gg.OUT, name + ".npz"))
        dead = [k for k in gg.GRAD_KEYS if float(z["grad_abs:" + k]) == 0.0]
        assert not dead, f"{name}: the reference's gradient is exactly zero: {dead}"
    z = np.load(os.path.join(gg.OUT, "e2e_ddad_small.npz"))
    mean = float(z["out:consistency_mask"].mean())
    print(f"e2e_ddad_small.npz consistency mask mean {mean:.3f}")
    assert MASK_MEAN[0] <= mean <= MASK_MEAN[1], f"consistency mask mean {mean} outside {MASK_MEAN}"
    frame1 = [k for k in z.files if k.startswith(("out:cam_T_cam|0|1", "out:axisangle|0|1", "out:translation|0|1",
                                                  "out:color|1|", "out:sample|1|", "out:color_identity|1|"))]
    assert "out:cam_T_cam|0|-1" in z.files and not frame1, frame1


if __name__ == "__main__":
    main()
