#!/usr/bin/env python3
"""Decode-pool step time by head, on the GPU: ms per step of llm.DecodePool with every slot live at the metric configuration's context
(the 3B shapes, 651-token prompts; scripts/pool_bench.py's workload), the step ending in
  greedy     fo1_decode_argmax_accept (every sequence plain greedy),
  sampled    the general head fo1_decode_head_accept, every sequence sampled (T = 0.7, top_k = 50, top_p = 0.9),
  penalised  the same with repetition_penalty = 1.3 on every sequence (seen bitmap read in every pass),
  greedy_lp0 / greedy_lp8   the greedy head followed by the log-probability record (fo1_decode_logprob_record), every sequence asking for
             it with top-n = 0 / 8,
  greedy_general   the general head with every sequence a greedy row (no draw, no penalty, no rule): what `banned` and `min_new` add to,
  banned     the ruled general head fo1_decode_head_ruled_accept, every sequence greedy with one shared mask row of 1000 banned ids,
  sampled_banned   the same row on every sequence of `sampled`,
  min_new    every sequence greedy with an early_row (16 ids) that is live on every timed step,
  guided     the guided general head fo1_decode_head_guided_accept, every sequence greedy with one shared two-state guide whose states both
             ban `banned`'s 1000 ids (one live mask row) and which changes state with every token: what the guide adds to `banned`,
  sampled_guided   the same guide on every sequence of `sampled`: what it adds to `sampled_banned`,
  one_banned / one_guided   one such ruled / guided greedy sequence among 127 plain ones,
  closing    the closing form of the guided head, fo1_decode_head_closing_accept: every sequence greedy with one shared two-state guide over
             three classes (banned ids, even ids, odd ids: an even id changes the state, an odd one keeps it) whose state 0 is accepting, so
             D = 1 and the budget's last pick alone reads a closing row — every timed step pays the closing form's two table reads and
             resolves to the state's plain row, the steady state of a closing sequence,
  guided_open   the same guide without accepting states through fo1_decode_head_guided_accept: what `closing` adds to,
  sampled_closing / sampled_guided_open   the two on every sequence of `sampled`,
  biased     the steered general head fo1_decode_head_steered_accept, every sequence greedy with one shared logit bias of 300 entries (one row
             of the bias table): what the bias adds to `greedy_general`,
  sampled_biased   the same bias on every sequence of `sampled`,
  counted    every sequence of `sampled` with frequency_penalty = presence_penalty = 0.2: the count rows are read (their gate bitmaps first)
             and the accepted token counted every step,
  greedy_counted   the same penalties on every sequence of `greedy_general`.
The heads are timed alternately, `--rounds` times each in one process, so the spread of a figure is the spread between its rounds; the pool is
drained and re-joined for every timing.  Prints one JSON object.

    python scripts/pool_head_bench.py [--slots 128] [--steps 64] [--rounds 5] [--heads greedy sampled penalised ...] [--root DIR]

With `greedy` among the heads the output also holds each other head's increment over it (difference of the medians of this process), and
for a ruled head its increment over the same head without a rule (banned, min_new: greedy_general; sampled_banned: sampled), for a guided
head its increment over the ruled head with the same mask row (guided: banned; sampled_guided: sampled_banned; one_guided: one_banned), for
a closing head its increment over the guided head with the same guide (closing: guided_open; sampled_closing: sampled_guided_open), for
a steered head its increment over the same head without the steer (biased, greedy_counted: greedy_general; sampled_biased, counted: sampled)
beside this process's penalised - sampled, the increment of the other per-token transformation behind a gate bitmap.

--root DIR imports the package from another checkout (e.g. the parent commit, for the greedy figure of both on one box; only `greedy`
exists there; a head the other checkout lacks cannot be named)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    HEADS = ["greedy", "sampled", "penalised", "greedy_lp0", "greedy_lp8", "greedy_general", "banned", "sampled_banned", "min_new", "guided",
             "sampled_guided", "one_banned", "one_guided", "closing", "guided_open", "sampled_closing", "sampled_guided_open",
             "biased", "sampled_biased", "counted", "greedy_counted"]
    ap.add_argument("--heads", nargs="+", default=HEADS[:3], choices=HEADS)
    ap.add_argument("--root", default=None, help="import vlm_fo1_amd from this checkout instead of the script's own")
    args = ap.parse_args()
    sys.path.insert(0, HERE)                 # bench.py (the workload builder)
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import vlm_fo1_amd                       # (first: bench.py puts its own checkout in front of sys.path, the package is then already bound)
    import bench as B
    from vlm_fo1_amd.llm import DecodePool
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cases = [B.build_workload(dev, n_boxes=100, seed=1234 + i) for i in range(32)]
    pipe = B.Pipeline(cases[0], dev, inflight=1, batch=32, cases=cases)
    eng = pipe.eng
    eng.prefill_batch(pipe.requests, use_graph=False)
    torch.cuda.synchronize()
    hp, first = eng._last_batch, eng._last_next_tokens.clone()
    logits0 = eng._last_logits.clone()       # the first tokens' records are scored on the prefill's logits
    prompts = [list(r["ids"]) for r in pipe.requests]
    P = args.slots
    pool = DecodePool(eng.llm, slots=P)
    sampling = dict(greedy=None,
                    sampled=dict(temperature=0.7, top_p=0.9, top_k=50, seed=11),
                    penalised=dict(temperature=0.7, top_p=0.9, top_k=50, seed=11, repetition_penalty=1.3), greedy_lp0=None, greedy_lp8=None)
    top_n = dict(greedy_lp0=0, greedy_lp8=8)
    budget = 4 + args.steps + 8
    V = eng.cfg.llm.vocab_size
    ban = list(range(5, V, max(1, V // 1000)))[:1000]      # one set for every sequence: one shared row of the mask table
    sampling.update(greedy_general=dict(greedy=True), banned=dict(greedy=True, ban=ban), sampled_banned=dict(sampling["sampled"], ban=ban),
                    min_new=dict(greedy=True, ban_until=(budget + 1, list(range(3, 19)))))
    unruled = dict(banned="greedy_general", min_new="greedy_general", sampled_banned="sampled")
    unguided = dict(guided="banned", sampled_guided="sampled_banned", one_guided="one_banned")
    lone = dict(one_banned="banned", one_guided="guided")      # heads whose first sequence alone carries the other head's dict
    if any(h in unguided for h in args.heads):
        import numpy as np
        from vlm_fo1_amd.guide import TokenGuide
        cls = np.zeros(V, np.uint16)
        cls[ban] = 1
        guide = TokenGuide(cls, np.array([[1, -1], [0, -1]], np.int32), 0, V)      # both states ban `ban`: one shared mask row, as `banned` has
        sampling.update(guided=dict(greedy=True, guide=guide), sampled_guided=dict(sampling["sampled"], guide=guide))
    sampling.update(one_banned=None, one_guided=None)
    unclosed = dict(closing="guided_open", sampled_closing="sampled_guided_open")
    if any(h in unclosed or h in unclosed.values() for h in args.heads):
        import numpy as np
        from vlm_fo1_amd.guide import TokenGuide
        cls = (np.arange(V) % 2 * 2).astype(np.uint16)      # class 0: even ids, class 2: odd ids, class 1: `ban`
        cls[ban] = 1
        nx = np.array([[1, -1, 0], [0, -1, 1]], np.int32)
        for name, accept in (("closing", [0]), ("guided_open", None)):
            g3 = TokenGuide(cls, nx, 0, V, accept=accept)
            sampling[name] = dict(greedy=True, guide=g3)
            sampling["sampled_" + name] = dict(sampling["sampled"], guide=g3)

    bias = {t: (1.5 if i % 2 else -1.5) for i, t in enumerate(range(7, V, max(1, V // 300))[:300])}      # one vector for every sequence: one shared row
    sampling.update(biased=dict(greedy=True, bias=bias), sampled_biased=dict(sampling["sampled"], bias=bias),
                    counted=dict(sampling["sampled"], frequency_penalty=0.2, presence_penalty=0.2),
                    greedy_counted=dict(greedy=True, frequency_penalty=0.2, presence_penalty=0.2))
    unsteered = dict(biased="greedy_general", greedy_counted="greedy_general", sampled_biased="sampled", counted="sampled")

    def one(head):
        left, base = P, 0
        while left > 0:
            n = min(32, left)
            kw = {} if sampling[head] is None else dict(sampling=dict(sampling[head], stream=base), prompt_ids=prompts[:n])
            if head in lone and base == 0:
                kw = dict(sampling=[dict(sampling[lone[head]], stream=0)] + [None] * (n - 1), prompt_ids=prompts[:n])
            if head in top_n:
                from vlm_fo1_amd import ops
                kw.update(logprobs=top_n[head], first_logprobs=ops.logprob_rows(logits0[:n], first[:n].to(torch.int32).contiguous(), top_n[head]))
            pool.join(eng.llm.kcache, eng.llm.vtcache, hp["seqs"][:n], hp["delta"][:n], first[:n], budget, (), **kw)
            left -= n
            base += n
        for _ in range(4):
            pool.step(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pool.step(True)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / args.steps
        live = len(pool.live)
        pool.drain(poll=8)                   # to the budget: every slot is free again for the next timing
        return t * 1e3, live

    for h in args.heads:                     # captures and first touches outside the timed rounds
        one(h)
    times = {h: [] for h in args.heads}
    for _ in range(args.rounds):
        for h in args.heads:
            ms, live = one(h)
            assert live == P, f"{live} of {P} sequences were live through the timed steps"
            times[h].append(round(ms, 4))
    out = dict(package=os.path.dirname(os.path.abspath(vlm_fo1_amd.__file__)), slots=P, live=P, steps=args.steps, rounds=args.rounds,
               prompt_tokens=hp["seqs"][0][1], vocab=eng.cfg.llm.vocab_size, heads={})
    for h, v in times.items():
        out["heads"][h] = dict(ms_per_step=v, median=round(statistics.median(v), 4), min=min(v), max=max(v),
                               spread_pct=round(100.0 * (max(v) - min(v)) / statistics.median(v), 3))
    if "greedy" in times:
        out["increment_over_greedy_ms"] = {h: round(out["heads"][h]["median"] - out["heads"]["greedy"]["median"], 4) for h in times if h != "greedy"}
    ruled = {h: round(out["heads"][h]["median"] - out["heads"][u]["median"], 4) for h, u in unruled.items() if h in times and u in times}
    if ruled:
        out["increment_over_unruled_ms"] = ruled
    guided = {h: round(out["heads"][h]["median"] - out["heads"][u]["median"], 4) for h, u in unguided.items() if h in times and u in times}
    if guided:
        out["increment_over_ruled_ms"] = guided
    closing = {h: round(out["heads"][h]["median"] - out["heads"][u]["median"], 4) for h, u in unclosed.items() if h in times and u in times}
    if closing:
        out["increment_over_guided_ms"] = closing
    steered = {h: round(out["heads"][h]["median"] - out["heads"][u]["median"], 4) for h, u in unsteered.items() if h in times and u in times}
    if steered:
        out["increment_over_unsteered_ms"] = steered
        if "penalised" in times and "sampled" in times:
            out["penalised_minus_sampled_ms"] = round(out["heads"]["penalised"]["median"] - out["heads"]["sampled"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
