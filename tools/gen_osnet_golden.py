"""Write tests/golden/osnet_{mild,sharp,half,odd}.npz: the reference's crop + torchvision pre-processing (through Pillow) and the fp32 torch
restatement of torchreid's OSNet (tests/osnet_common.py, eval mode, L2 normalised as the reference does; its fp32 weights and pixels
evaluated in float64 and the features rounded to float32, so that the file reproduces on any CPU) on the CPU, for the seeded
synthetic weight sets of weights.OSNET_SETS and the 37 golden boxes of tests/reid_common.py.  Weights and frames are not stored: they are
regenerated from their seeds; the file keeps the boxes, the frame seed and shape, and the features.

    python tools/gen_osnet_golden.py [tag ...]     (default: every tag)
"""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import osnet_common as O  # noqa: E402


def golden(tag):
    frames = O.golden_frames()
    boxes, owner = O.golden_boxes()
    model, _ = O.osnet_model(tag)
    feats = O.osnet_features(model, O.reference_pixels(frames, boxes, owner)).astype(np.float32)
    return boxes, owner, feats


TAGS = ("mild", "sharp", "half", "odd")


def main():
    for tag in sys.argv[1:] or TAGS:
        boxes, owner, feats = golden(tag)
        path = os.path.join(ROOT, "tests", "golden", f"osnet_{tag}.npz")
        np.savez_compressed(path, boxes=boxes, owner=owner, features=feats, frame_seed=np.int64(O.R.FRAME_SEED),
                            frame_hw=np.array([O.R.FRAME_H, O.R.FRAME_W], np.int32))
        print("wrote", path, feats.shape)


if __name__ == "__main__":
    main()
