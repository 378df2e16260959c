"""UPN post-process: the host path (UPNWrapper.postprocess + filter: device-to-host copy, box conversion, argsort, threshold, numpy NMS)
against the device path (ops.upn_post + one copy back + host rounding), in one process on the MI355X.

    python scripts/upn_post_bench.py [--out profiles/upn_postprocess.json] [--rounds 5] [--iters 50] [--no-detector]

Part 1, per proposal set (vlm_fo1_amd.fixtures.upn_proposals.BENCH_SETS: three seeded synthetic sets and one built from the fixture box
lists, 900 proposals, nms_value 0.8), starting from device tensors: wall clock with a synchronise before and after each call, `rounds`
rounds alternating the two paths, `iters` calls per round; the kernel alone between two device events (per launch, over `iters`
back-to-back launches).  Part 2: the full-size detector (Swin-L 2-2-18-2, 6 + 6 layers, 900 queries, random weights) on a 640 x 480
image (800 x 1066 resized): inference + filter against propose, per image, same protocol.  Medians over the rounds and the
round-to-round spread (max - min) of each side are reported; both paths' results are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the seeded detector weights (tests/upn_cases.py)

import numpy as np   # noqa: E402
import torch         # noqa: E402

NMS = 0.8
SIZE_HW = (480, 640)


def wall_ms(fn, iters):
    total = 0.0
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t
    return total / iters * 1e3


def summary(xs):
    return dict(median_ms=statistics.median(xs), spread_ms=max(xs) - min(xs), rounds_ms=[round(x, 5) for x in xs])


def alternate(parent, new, rounds, iters):
    a, b = [], []
    for _ in range(rounds):
        a.append(wall_ms(parent, iters))
        b.append(wall_ms(new, iters))
    pa, nw = summary(a), summary(b)
    gain = pa["median_ms"] - nw["median_ms"]
    return dict(parent=pa, new=nw, gain_ms=gain, gain_exceeds_spread=bool(gain > pa["spread_ms"] + nw["spread_ms"]))


def proposal_sets(rounds, iters):
    from detect_tools.upn.inference_wrapper import UPNWrapper, kept_lists
    from vlm_fo1_amd import ops
    from vlm_fo1_amd.fixtures.upn_proposals import BENCH_SETS
    me = object.__new__(UPNWrapper)
    out = {}
    for name, (make, min_score) in BENCH_SETS.items():
        b, l = make()
        boxes, logits = torch.from_numpy(b).cuda(), torch.from_numpy(l).cuda()
        prm = ops.upn_post_params([SIZE_HW], min_score, NMS, len(l), "cuda")
        dev_out = dict(pred_boxes=boxes[None], pred_logits=logits[None, :, None])

        def parent():
            return me.filter(me.postprocess(dev_out, [list(SIZE_HW)]), min_score, NMS)

        def new():
            return kept_lists([ops.upn_post(boxes, logits, prm)])

        want, got = parent(), new()
        same_boxes = got["original_xyxy_boxes"] == want["original_xyxy_boxes"]
        row = dict(proposals=len(l), over_min_score=int((1 / (1 + np.exp(-l.astype(np.float64))) >= min_score).sum()), kept=len(got["scores"][0]),
                   min_score=min_score, nms_value=NMS, same_result_as_host_path=bool(same_boxes and got["scores"] == want["scores"]))
        for _ in range(3):
            parent(), new()
        row.update(alternate(parent, new, rounds, iters))
        ev = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                ops.upn_post(boxes, logits, prm)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / iters)
        row["kernel_events"] = summary(ev)
        out[name] = row
        print(name, json.dumps(row), flush=True)
    return out


def detector(rounds, iters):
    import upn_cases as C
    from PIL import Image
    from detect_tools.upn import UPNWrapper
    state = C.upn_state(depths=[2, 2, 18, 2], n_enc=6, n_dec=6, n_queries=900)
    w = UPNWrapper(state, "cuda")
    rng = np.random.default_rng(5)
    img = [Image.fromarray(rng.integers(0, 256, (SIZE_HW[0], SIZE_HW[1], 3), dtype=np.uint8), "RGB")]
    res = w.inference(img)
    min_score = float(res["scores"][0, 300, 0])                # random weights: a threshold that leaves 300 candidates

    def parent():
        return w.filter(w.inference(img), min_score, NMS)

    def new():
        return w.propose(img, min_score, NMS)

    for _ in range(4):                                          # sighting, capture, replay
        want, got = parent(), new()
    row = dict(image="640x480 -> 800x1066", queries=900, min_score=min_score, nms_value=NMS, kept=len(got["scores"][0]),
               same_boxes_as_host_path=bool(got["original_xyxy_boxes"] == want["original_xyxy_boxes"]))
    row.update(alternate(parent, new, rounds, iters))
    x = w.transform_image(img[0])
    row["forward_graph_only"] = summary([wall_ms(lambda: w.model.forward_graph(x), iters) for _ in range(rounds)])
    print("detector", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upn_postprocess.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-detector", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upn_post_bench: needs the GPU (a CPU run measures nothing)")
    result = dict(device=torch.cuda.get_device_name(0), protocol=f"{a.rounds} rounds alternating host path / device path, {a.iters} calls per round, "
                  "wall clock with a synchronise before and after each call; medians over rounds, spread = max - min over rounds; kernel_events = device "
                  "events around back-to-back launches, per launch", sets=proposal_sets(a.rounds, a.iters))
    if not a.no_detector:
        result["detector_per_image"] = detector(a.rounds, max(10, a.iters // 5))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
