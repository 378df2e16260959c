"""Per-request sampling and repetition penalty in the decode pool (vlm_fo1_amd.llm.DecodePool's per-slot parameter table and seen bitmap, the
general head fo1_decode_head_accept) on the tiny engine of tests/test_batched_decode_gpu.py with the requests of
tests/test_sampling_gpu.py: 8 sequences, 16 tokens, a 64-slot pool.

  * a submission of four kinds — plain greedy, greedy with p = 1.3, sampled (T = 0.7, top_k = 50, top_p = 1), sampled with p = 1.3 — stepped
    by graph replay: every recorded id meets the rule of its kind against the oracle on THAT step's logits and the seen set replayed on the
    host (greedy rows exactly, sampled rows inside the accept rule, exact draws equal to the oracle's id; at least half the draws are exact);
  * the plain greedy sequences' ids are bitwise those of an all-greedy pool run; a sampled sequence draws the same ids in slot 0 alone and in
    slot 37 among 7 neighbours, graph == eager;
  * once the last non-plain sequence has been harvested the next step's graph key is the all-greedy key; a sampled submission joining
    mid-flight leaves the live greedy sequences' ids unchanged;
  * PoolService: generate_batch(reqs, sampling=[...]) with the pool enabled returns the direct run's ids; a seed repeats, another differs;
  * the plug-in: generate_many takes a mixed batch with the pool on and refuses it with the pool off; repetition_penalty = 0 / nan raise."""
import numpy as np
import pytest
import torch

import penalty_cases as P
import sampling_cases as S

pytestmark = pytest.mark.gpu

N_SEQ, N_TOK, SEED, PEN = 8, 16, 0x5a17ab1e5eed, 1.3
T, TOP_K = 0.7, 50


def _kinds(seed=SEED):
    samp = dict(temperature=T, top_p=1.0, top_k=TOP_K, seed=seed)
    four = [None, dict(greedy=True, repetition_penalty=PEN), samp, dict(samp, repetition_penalty=PEN)]
    return [None if four[b % 4] is None else dict(four[b % 4], stream=b) for b in range(N_SEQ)]


class _Fx:
    pass


@pytest.fixture(scope="module")
def fx():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    from vlm_fo1_amd.llm import DecodePool
    f = _Fx()
    _, _, f.eng = build()
    f.reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    f.per = _kinds()
    f.eng.prefill_batch(f.reqs, use_graph=False)
    f.hp = f.eng._last_batch
    f.logits0 = f.eng._last_logits[:N_SEQ].clone()
    f.first_greedy = f.eng._last_next_tokens[:N_SEQ].clone()
    f.first = f.eng._first_tokens(f.per, f.reqs).clone()
    f.pool = DecodePool(f.eng.llm, slots=64)
    f.V = f.eng.cfg.llm.vocab_size
    return f


def _join(f, sel, per, first, budget=N_TOK):
    pool, eng = f.pool, f.eng
    return pool.join(eng.llm.kcache, eng.llm.vtcache, [f.hp["seqs"][b] for b in sel], [f.hp["delta"][b] for b in sel],
                     torch.stack([first[b] for b in sel]), budget, (), tags=[("t", b) for b in sel],
                     sampling=None if per is None else [per[b] for b in sel], prompt_ids=[f.reqs[b]["ids"] for b in sel])


def _run(f, sel, per, first, graph=True):
    _join(f, sel, per, first)
    got = {tag[1]: ids for _, tag, ids in f.pool.drain(use_graph=graph, poll=5)}
    assert not f.pool.live and len(f.pool.free) == f.pool.P and f.pool.n_general == 0
    return [got[b] for b in sel]


def _prefill(f):
    """The requests' K / V^T rows back into the engine's prefill cache (another test's generate calls overwrite it)."""
    f.eng.prefill_batch(f.reqs, use_graph=False)
    f.hp = f.eng._last_batch


def _mixed(f):
    """The ids of the mixed submission's direct pool run (computed once)."""
    if not hasattr(f, "mixed_ids"):
        _prefill(f)
        f.mixed_ids = _run(f, list(range(N_SEQ)), f.per, f.first)
    return f.mixed_ids


def _bits(row: torch.Tensor) -> np.ndarray:
    return row.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def test_every_id_of_a_mixed_submission_meets_the_rule_of_its_kind_on_its_steps_logits(fx):
    f = fx
    _prefill(f)
    slots = _join(f, list(range(N_SEQ)), f.per, f.first)
    assert f.pool.n_general == 6 and f.pool.seen is not None
    logits = [f.logits0]
    for _ in range(N_TOK - 1):
        logits.append(f.pool.step(use_graph=True)[slots].clone())
    assert any("general" in k for k in f.pool._graphs)
    got = {tag[1]: ids for _, tag, ids in f.pool.harvest(f.pool.snapshot())}
    ids = [got[b] for b in range(N_SEQ)]
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == f.first.cpu().tolist()
    assert not f.pool.live and f.pool.n_general == 0
    n_exact = n_draws = 0
    for b in range(N_SEQ):
        sp = f.per[b]
        pen = (sp or {}).get("repetition_penalty", 0.0)
        seen = [t for t in f.reqs[b]["ids"] if 0 <= t < f.V]
        assert len(seen) < len(f.reqs[b]["ids"]), "the prompt has placeholder ids that must be skipped"
        for t in range(N_TOK):
            pb = P.penalise(_bits(logits[t][b]), seen, pen)
            if sp is None or sp.get("greedy"):
                assert ids[b][t] == P.greedy_pick(pb), (b, t, ids[b][t], P.greedy_pick(pb))
            else:
                o, u = S.oracle(pb, T, 1.0, TOP_K), S.draw_u(t, b, SEED)
                assert S.accepts(o, u, ids[b][t]), (b, t, u, ids[b][t], S.pick(o, u))
                n_draws += 1
                if S.is_exact(o, u):
                    n_exact += 1
                    assert ids[b][t] == S.pick(o, u), (b, t, u)
            seen.append(ids[b][t])
    assert n_draws == 4 * N_TOK and n_exact >= n_draws // 2
    assert ids == _mixed(f), "the same mixed submission decoded differently the second time"


def test_plain_sequences_equal_the_all_greedy_pool_and_a_sampled_sequence_ignores_slot_and_neighbours(fx):
    f = fx
    _prefill(f)
    allg = _run(f, list(range(N_SEQ)), None, f.first_greedy)
    mixed = _mixed(f)
    assert mixed[0] == allg[0] and mixed[4] == allg[4], "a plain greedy sequence changed beside sampled neighbours"
    assert any(mixed[b] != allg[b] for b in (1, 5)) and any(mixed[b] != allg[b] for b in (2, 6)), "penalty / sampling changed nothing"
    assert _run(f, list(range(N_SEQ)), f.per, f.first, graph=False) == mixed, "eager and graph-replayed steps differ"
    for b in (2, 3, 1):      # sampled, sampled + penalty, greedy + penalty: alone in slot 0
        assert _run(f, [b], f.per, f.first) == [mixed[b]], f"sequence {b} decodes differently alone in slot 0"
    # slot 37 with 7 neighbours behind it (the join takes the lowest free slots: hide 0 .. 36 from it)
    f.pool.free = list(range(37, 64))
    try:
        order = [2, 0, 1, 3, 4, 5, 6, 7]
        slots = _join(f, order, f.per, f.first)
        assert slots[0] == 37
        got = {tag[1]: ids for _, tag, ids in f.pool.drain(use_graph=True, poll=5)}
    finally:
        f.pool.free = list(range(64))
    assert [got[b] for b in range(N_SEQ)] == mixed, "ids depend on the slot"


def test_head_switches_back_to_the_greedy_key_and_a_late_sampled_join_leaves_greedy_ids_alone(fx):
    f = fx
    pool = f.pool
    mixed = _mixed(f)
    _prefill(f)
    allg = _run(f, [0, 4, 5], None, f.first_greedy)

    def todays_key():
        return (pool.slot_rows, pool.kv_bucket(), pool.llm.rope_epoch, pool.llm.rope_cos.data_ptr(), bool(pool.FUSED_SPLITK),
                tuple(sorted(pool.SPLITS.items())), bool(pool.TILED_WEIGHTS))
    # greedy sequences in flight; a sampled submission joins after 5 steps with a budget of 4 and leaves again
    _join(f, [0, 4, 5], None, f.first_greedy)
    for _ in range(5):
        pool.step()
    assert pool.n_general == 0
    _join(f, [2, 3], f.per, f.first, budget=4)
    assert pool.n_general == 2
    got = {}
    for _ in range(3):
        pool.step()
    for _, tag, ids in pool.harvest(pool.snapshot()):
        got[tag[1]] = ids
    assert sorted(got) == [2, 3] and pool.n_general == 0 and sorted(pool.live) == [0, 1, 2]
    assert got[2] == mixed[2][:4] and got[3] == mixed[3][:4]
    pool._graphs.clear()
    key = todays_key()
    pool.step()
    assert list(pool._graphs) == [key], "with only plain sequences live the step's graph key is not the all-greedy key"
    for _, tag, ids in pool.drain(poll=4):
        got[tag[1]] = ids
    assert [got[b] for b in (0, 4, 5)] == allg, "a sampled submission joining mid-flight changed the greedy sequences' ids"


def test_pool_service_path_returns_the_direct_runs_ids_and_seeds_repeat_and_differ(fx):
    f = fx
    eng = f.eng
    mixed = _mixed(f)
    per = [None if sp is None else {k: v for k, v in sp.items() if k != "stream"} for sp in f.per]      # (request i draws on stream i)
    eng.enable_decode_pool(slots=64)
    try:
        got = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per)
        assert got == mixed, "the scheduler's pool gave other ids than the direct pool run"
        assert eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per) == got, "the same seeds gave other ids"
        other = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=[None if sp is None else ({**sp, "seed": SEED + 1} if "seed" in sp else sp) for sp in per])
        assert [other[b] for b in (0, 1, 4, 5)] == [got[b] for b in (0, 1, 4, 5)], "a seed moved a greedy sequence"
        assert any(other[b] != got[b] for b in (2, 3, 6, 7)), "another seed changed no sampled sequence"
        # one dict for the whole batch: request i on stream i, like the BatchDecoder path
        samp = dict(temperature=T, top_p=1.0, top_k=TOP_K, seed=SEED)
        pooled = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=samp)
        assert [pooled[b] for b in (2, 6)] == [got[b] for b in (2, 6)]
    finally:
        eng.disable_decode_pool()
    # without the pool the BatchDecoder groups take the same dicts (other kernels: the logits differ in last bits, the rules are the same)
    bd = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per)
    assert [len(r) for r in bd] == [N_TOK] * N_SEQ
    assert bd == eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=False, sampling=per), "BatchDecoder general head: graph != eager"
    plain = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True)
    assert any(bd[b] != plain[b] for b in (1, 5)), "the penalty changed no greedy sequence of the BatchDecoder"


def _generate_kwargs(r):
    gh, gw = r["grid"]
    return dict(inputs=torch.tensor([r["ids"]]), images=[r["pix"]], images_aux=[r["aux"]], image_grid_thws=[torch.tensor([[1, gh, gw]])],
                bbox_list=[r["boxes"]])


class _Collect:
    def __init__(self):
        self.parts, self.ended = [], False

    def put(self, t):
        self.parts.append(t)

    def end(self):
        self.ended = True


def test_plug_in_mixed_batch_needs_the_pool_and_bad_penalties_raise(fx):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
    f = fx
    eng = f.eng
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {}), eng)
    kws = [dict(_generate_kwargs(r), max_new_tokens=6) for r in f.reqs[:4]]
    batch = [kws[0], dict(kws[1], do_sample=True, temperature=0.7, top_p=0.9, seed=3), dict(kws[2], repetition_penalty=PEN),
             dict(kws[3], do_sample=True, temperature=1.0, top_k=0, seed=4, repetition_penalty=PEN)]
    with pytest.raises(ValueError, match="share do_sample, temperature, top_p and top_k"):
        m.generate_many(batch)
    for bad in (0, float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            m.generate(**kws[0], repetition_penalty=bad)
        with pytest.raises(ValueError, match="repetition_penalty"):
            m.generate_many([kws[0], dict(kws[1], repetition_penalty=bad)])
    # without the pool: a penalised greedy request, device loop == streamer loop (a BatchDecoder of one either way), != the plain ids
    plain = m.generate(**kws[2])
    pen = m.generate(**kws[2], repetition_penalty=PEN)
    L = kws[2]["inputs"].shape[1]
    assert tuple(pen.shape) == (1, L + 6) and pen[0, :L].tolist() == f.reqs[2]["ids"]
    assert m.generate(**kws[2], repetition_penalty=1.0).tolist() == plain.tolist() == m.generate(**kws[2], repetition_penalty=None).tolist()
    st = _Collect()
    assert m.generate(**kws[2], repetition_penalty=PEN, streamer=st).tolist() == pen.tolist() and st.ended
    same = m.generate_many([dict(k, repetition_penalty=PEN) for k in kws[:3]])      # a uniform penalised batch needs no pool
    assert [tuple(o.shape) for o in same] == [(1, k["inputs"].shape[1] + 6) for k in kws[:3]]
    eng.enable_decode_pool(slots=64)
    try:
        out = m.generate_many(batch)
        assert [tuple(o.shape) for o in out] == [(1, k["inputs"].shape[1] + 6) for k in kws]
        assert out[0].tolist() == m.generate(**kws[0]).tolist(), "the plain request of a mixed batch != the same request alone"
        assert out[2].tolist() == m.generate(**kws[2], repetition_penalty=PEN).tolist()
        assert [o.tolist() for o in m.generate_many(batch)] == [o.tolist() for o in out], "the same seeds gave other ids"
        assert [o.tolist() for o in m.generate_many_async(batch).result()] == [o.tolist() for o in out]
    finally:
        eng.disable_decode_pool()
