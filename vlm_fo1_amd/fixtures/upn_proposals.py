"""Seeded stand-ins for the UPN detector's raw outputs (pred_boxes cx, cy, w, h in [0, 1] and pred_logits), for the post-process
tests and scripts/upn_post_bench.py: clustered proposals (a detector puts many near-duplicates on each object, which is what NMS is
for) and one set built from the reference's real UPN box lists (box_fixtures.json)."""
from __future__ import annotations

import numpy as np


def clustered_proposals(Q: int = 900, n_clusters: int = 60, seed: int = 0, logit_mean: float = -0.5, logit_std: float = 2.0):
    """Q proposals as jittered copies of n_clusters seeded object boxes (n_clusters = 0: independent boxes) and normal logits.
    -> (boxes fp32 [Q, 4] cxcywh in [0, 1], logits fp32 [Q])."""
    rng = np.random.default_rng(seed)
    if n_clusters > 0:
        centres = np.concatenate([rng.uniform(0.15, 0.85, (n_clusters, 2)), rng.uniform(0.04, 0.3, (n_clusters, 2))], 1)
        which = rng.integers(0, n_clusters, Q)
        boxes = centres[which] + rng.normal(0.0, 1.0, (Q, 4)) * centres[which][:, 2:].repeat(2, 1) * np.array([0.08, 0.08, 0.12, 0.12])
    else:
        boxes = np.concatenate([rng.uniform(0.1, 0.9, (Q, 2)), rng.uniform(0.02, 0.25, (Q, 2))], 1)
    boxes[:, 2:] = np.clip(boxes[:, 2:], 0.005, 1.0)
    boxes[:, :2] = np.clip(boxes[:, :2], 0.0, 1.0)
    logits = rng.normal(logit_mean, logit_std, Q)
    return boxes.astype(np.float32), logits.astype(np.float32)


def fixture_proposals(Q: int = 900, seed: int = 0):
    """Q proposals from the reference's real UPN box lists (the longest CountBench / Pixmo lists, each normalised by its own image
    extent), every box followed by jittered duplicates until Q are there; logits fall with the list position as a detector's do.
    -> (boxes fp32 [Q, 4] cxcywh in [0, 1], logits fp32 [Q])."""
    from .hfre_cases import box_fixtures
    fx = box_fixtures()
    items = sorted(fx["countbench"] + fx["pixmo"], key=lambda x: -len(x["bboxes"]))
    real = []
    for it in items:
        ex, ey = it["extent"]
        for b in it["bboxes"]:
            real.append([(b[0] + b[2]) / 2 / ex, (b[1] + b[3]) / 2 / ey, (b[2] - b[0]) / ex, (b[3] - b[1]) / ey])
        if len(real) >= Q // 3:
            break
    real = np.asarray(real[:Q // 3], dtype=np.float64)
    rng = np.random.default_rng(seed)
    which = np.concatenate([np.arange(len(real)), rng.integers(0, len(real), Q - len(real))])
    jitter = rng.normal(0.0, 1.0, (Q, 4)) * real[which][:, 2:].repeat(2, 1) * np.array([0.05, 0.05, 0.1, 0.1])
    jitter[:len(real)] = 0.0
    boxes = real[which] + jitter
    boxes[:, 2:] = np.clip(boxes[:, 2:], 0.005, 1.0)
    boxes[:, :2] = np.clip(boxes[:, :2], 0.0, 1.0)
    logits = 2.0 - 4.0 * np.arange(Q) / Q + rng.normal(0.0, 0.3, Q)
    perm = rng.permutation(Q)                               # the detector's query order is not the score order
    return boxes[perm].astype(np.float32), logits[perm].astype(np.float32)


# the sets DESIGN §9 reports (three synthetic, one from the fixture box lists): name -> (builder, min_score)
BENCH_SETS = {
    "clusters60_min0.3": (lambda: clustered_proposals(900, 60, seed=11), 0.3),
    "clusters300_min0.3": (lambda: clustered_proposals(900, 300, seed=12), 0.3),
    "noclusters_min0.05": (lambda: clustered_proposals(900, 0, seed=13, logit_mean=-1.0), 0.05),
    "fixture_boxes_min0.3": (lambda: fixture_proposals(900, seed=14), 0.3),
}
