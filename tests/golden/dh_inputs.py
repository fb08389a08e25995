"""Deterministic inputs of the Double-Head R-CNN tests: shared by tests/golden/gen_dh_golden.py
(which runs the reference on them) and the tests.  Nothing here reads the reference."""
import numpy as np

import inputs

# ----------------------------------------------------------------- whole detector
WHOLE_DH = ('dh', 'dh_rcnn_r50_fpn.py', {'rcnn': {'min_score': 0.0}}, inputs.FTRAIN_SHAPE)

# ----------------------------------------------------------------- the head alone
HEAD_ROIS = 37   # not a multiple of the kernel's RoI group


def head_rois(seed=2024):
    """A seeded [HEAD_ROIS, 256, 7, 7] f32 RoI batch of both signs (FPN levels carry no ReLU)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((HEAD_ROIS, 256, 7, 7)).astype(np.float32)
