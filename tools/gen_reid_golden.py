"""Write tests/golden/reid_{mild,sharp,tiny,p56}.npz: HF `CLIPImageProcessorPil` + `CLIPVisionModelWithProjection` (`image_embeds`, then L2
normalised as the reference does) in fp32 on the CPU, for the seeded synthetic CLIP weight sets of weights.CLIP_SETS and the golden
boxes of tests/reid_common.py.  The weights and the frames are not stored: they are regenerated from their seeds
(weights.synth_clip_weights, frames.structured_frames); the file keeps the boxes, the frame seed and shape, and the features.

    python tools/gen_reid_golden.py [tag ...]     (default: every tag)
"""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import reid_common as R  # noqa: E402


TAGS = ("mild", "sharp", "tiny", "p56")


def main():
    frames = R.golden_frames()
    boxes, owner = R.golden_boxes()
    pv = R.hf_pixel_values(frames, boxes, owner)
    for tag in sys.argv[1:] or TAGS:
        model, _ = R.hf_model(tag)
        feats = R.hf_features(model, pv).astype(np.float32)
        path = os.path.join(ROOT, "tests", "golden", f"reid_{tag}.npz")
        np.savez_compressed(path, boxes=boxes, owner=owner, features=feats, frame_seed=np.int64(R.FRAME_SEED),
                            frame_hw=np.array([R.FRAME_H, R.FRAME_W], np.int32))
        print("wrote", path, feats.shape)


if __name__ == "__main__":
    main()
