"""Every greedy-decode route of vlm_fo1_amd/llm.py against the CPU oracle, logits row by logits row (tests/decode_route_cases.py: model,
sequences, oracle and the one bound BOUND, calibrated by tests/test_decode_route_cases.py):
  * single sequence: QwenLLM.decode_step (eager) and decode_step_graph;
  * BatchDecoder at B = 1, 2 (the o-projection sums the attention partials), 9 (one 16-column MFMA group), 17 and 32 (two groups), graph
    and eager, and B = 9 through the C entry fo1_llm_decode_step (stage_abi.ENABLED);
  * DecodePool at 64 and 128 slots, FUSED_SPLITK on and off: partly occupied (s2040 included: 4096-row slots); a sequence leaves and a new
    one joins its slot while the others are mid-flight (s250 the longest: the 256-key bucket changes); a shared-prefix pair (relocated in
    two pieces).
step() is driven by hand and each step's logits rows are cloned (step 0's come from the prefill).  For every (route, sequence, step):
  1. the logits row is within BOUND of the oracle teacher-forced on that route's ids;
  2. the id is the oracle's argmax where the oracle's top-1 margin exceeds 2 x BOUND, and never more than 2 x BOUND below its maximum;
  3. all routes produce the same ids up to the first step where any route's oracle margin falls below 2 x BOUND."""
import pytest
import torch

import decode_route_cases as C

pytestmark = pytest.mark.gpu
K = C.STEPS
KEY = [s.name for s in C.KEY]
FILL = [s.name for s in C.FILL]
POOL_SCENARIOS = ("partly", "leave_join", "shared_prefix")
ROUTES = (["single-eager", "single-graph"] + [f"batch{B}-{m}" for B in (1, 2, 9, 17, 32) for m in ("graph", "eager")] + ["batch9-stage"]
          + [f"pool{P}-{'splitk' if sk else 'plain'}-{sc}" for P in (64, 128) for sk in (True, False) for sc in POOL_SCENARIOS])


def _llm():
    from vlm_fo1_amd.llm import LLMConfig, QwenLLM
    return QwenLLM(LLMConfig(num_layers=C.N_LAYERS, vocab_size=C.VOCAB, max_seq=1024), C.state(), "cuda")


def _prefill(llm, names, share=False):
    """One packed prefill pass (QwenLLM.plan_batch + prefill_packed) -> (plan, step-0 logits rows [B, V] on the host, first ids on the device)."""
    imgs, base, img_base = [], {}, []
    for n in names:
        s = C.BY_NAME[n]
        im = s.image if s.image >= 0 else s.seed
        if im not in base:
            base[im] = sum(t.shape[0] for t in imgs)
            imgs.append(C.prompt(n)[2])
        img_base.append(base[im])
    grids = [C.BY_NAME[n].grid for n in names]
    hp = llm.plan_batch([C.prompt_ids(n) for n in names], [g[0] * g[1] for g in grids], [0] * len(names), grids, img_base=img_base,
                        share_prefix=share)
    llm.reserve(hp["rows"])
    emb = llm.embed_rows(hp["plan"].cuda(), torch.cat(imgs, 0).cuda(), None)
    _, logits, toks = llm.prefill_packed(emb, hp["cos"].cuda(), hp["sin"].cuda(), hp["seqs"], hp["last"].cuda())
    return hp, logits.float().cpu(), toks.clone()


def _single(llm, graph):
    out = {}
    for n in KEY:
        x, pos, delta = C.inputs(n)
        llm.reserve(x.shape[0] + K + 1)
        _, lg, tok = llm.prefill(x.cuda(), pos, delta)
        rows, ids = [lg[0].float().cpu()], [int(tok.item())]
        if graph:
            llm.sync_decode_state()
        for i in range(K - 1):
            if graph:
                lg, tok = llm.decode_step_graph(tok if i == 0 else None)
            else:
                _, lg, tok = llm.decode_step(tok)
            rows.append(lg[0].float().cpu())
            ids.append(int(tok.item()))
        out[n] = (ids, torch.stack(rows))
    return out


def _batch(llm, B, graph, stage=False):
    from vlm_fo1_amd import stage_abi
    from vlm_fo1_amd.llm import BatchDecoder
    groups = {1: [[n] for n in KEY], 2: [["s40", "s2040"], ["s250", "s1000"]]}.get(B, [KEY + FILL[:B - len(KEY)]])
    out = {}
    for names in groups:
        hp, lg0, first = _prefill(llm, names)
        dec = BatchDecoder(llm)
        dec.start(hp["seqs"], hp["delta"], first, K)
        rows = [lg0]
        was = stage_abi.ENABLED
        stage_abi.ENABLED = stage
        try:
            for _ in range(K - 1):
                rows.append(dec.step(graph)[:len(names)].float().cpu())
        finally:
            stage_abi.ENABLED = was
        ids = dec.results()
        for b, n in enumerate(names):
            out[n] = (ids[b], torch.stack([r[b] for r in rows]))
    return out


def _pool(llm, P, splitk, scenario):
    from vlm_fo1_amd.llm import DecodePool
    pool = DecodePool(llm, slots=P, slot_rows=4096 if scenario == "partly" else 1024)
    pool.FUSED_SPLITK = splitk
    track = {}                                              # slot -> [name, budget, rows]
    out = {}

    def join(names, budget, share=False):
        hp, lg0, first = _prefill(llm, names, share)
        if share:
            pre = [sq[3:] for n, sq in zip(names, hp["seqs"]) if n.startswith("sh")]
            assert pre == [(pre[0][0], C.PREFIX_ROWS)] * 2, f"the pair does not share its first {C.PREFIX_ROWS} rows: {hp['seqs']}"
        slots = pool.join(llm.kcache, llm.vtcache, hp["seqs"], hp["delta"], first, budget, (), tags=list(names))
        for b, (sl, n) in enumerate(zip(slots, names)):
            track[sl] = [n, budget, [lg0[b]]]
        return slots

    def step():
        lg = pool.step(True).float().cpu()
        for sl, (n, budget, rows) in track.items():
            if len(rows) < budget:
                rows.append(lg[sl])

    def harvest():
        for sl, tag, ids in pool.harvest(pool.snapshot()):
            n, budget, rows = track.pop(sl)
            assert tag == n and len(ids) == budget == len(rows), (n, len(ids), budget, len(rows))
            out[n] = (ids, torch.stack(rows))

    if scenario == "partly":
        join(KEY + FILL[:5], K)
    elif scenario == "shared_prefix":
        join(["shA", "s40", "shB"], K, share=True)
    else:
        (gone,) = join(["s40"], 5)
        join(["s250"] + FILL[:4], K)
        for _ in range(4):
            step()
        harvest()
        assert "s40" in out and gone in pool.free
        assert join([FILL[4]], K) == [gone], "the new sequence did not take the freed slot"
    while track:
        step()
        harvest()
    assert not pool.live
    return out


def _run(llm, route):
    kind, *rest = route.split("-")
    if kind == "single":
        return _single(llm, rest[0] == "graph")
    if kind.startswith("batch"):
        return _batch(llm, int(kind[5:]), rest[0] != "eager", stage=rest[0] == "stage")
    return _pool(llm, int(kind[4:]), rest[0] == "splitk", rest[1])


@pytest.fixture(scope="module")
def runs():
    llm = _llm()
    return {r: _run(llm, r) for r in ROUTES}


@pytest.mark.parametrize("route", ROUTES)
def test_route_logits_and_ids_against_the_oracle(route, runs):
    O = C.Oracle.get()
    bad = []
    for n, (ids, rows) in runs[route].items():
        assert len(ids) == rows.shape[0] and len(ids) >= 5, (n, len(ids))
        ref = O.logits(n, ids)
        err = (rows - ref).abs().amax(-1)
        t = int(err.argmax())
        if err[t] > C.BOUND:
            bad.append(f"{n} step {t}: logit error {err[t]:.3f} > {C.BOUND}")
        for t, i in enumerate(ids):
            if C.margin(ref[t]) > 2 * C.BOUND and i != int(ref[t].argmax()):
                bad.append(f"{n} step {t}: id {i} is not the oracle's argmax {int(ref[t].argmax())} (margin {C.margin(ref[t]):.2f})")
            if float(ref[t].max() - ref[t][i]) > 2 * C.BOUND:
                bad.append(f"{n} step {t}: id {i} is {float(ref[t].max() - ref[t][i]):.2f} below the oracle's maximum")
    assert not bad, f"{route}: " + "; ".join(bad[:8])


def test_routes_agree_until_the_first_near_tie(runs, capsys):
    O = C.Oracle.get()
    worst = {}
    for route, res in runs.items():
        worst[route] = max(float((rows - O.logits(n, ids)).abs().max()) for n, (ids, rows) in res.items()) / C.BOUND
    with capsys.disabled():
        print("\n[decode routes] worst logit error / BOUND: " + ", ".join(f"{r} {w:.2f}" for r, w in worst.items()))
    names = sorted({n for res in runs.values() for n in res})
    compared = 0
    for n in names:
        got = {r: res[n][0] for r, res in runs.items() if n in res}
        cut = min(len(ids) for ids in got.values())
        for r, ids in got.items():
            ref = O.logits(n, ids)
            cut = min([cut] + [t for t in range(len(ids)) if C.margin(ref[t]) <= 2 * C.BOUND])
        first = next(iter(got.values()))[:cut]
        for r, ids in got.items():
            assert ids[:cut] == first, f"{n}: {r} gives {ids[:cut]}, another route {first} (no near-tie before step {cut})"
        compared += cut * (len(got) - 1)
    assert compared > 0
