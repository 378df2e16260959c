"""CPU checks of the log-probability surface: the C ABI additions (lib.SIGNATURES, the library's exports and its argument checks, which run
before any HIP call), generate()'s two keywords and their errors, the per-request plan of generate_many, and the `logprobs` argument of the
decode loops."""
import inspect

import pytest
import torch

from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
from vlm_fo1_amd import lib as L


def test_abi_additions():
    for name in ("fo1_logprob_rows_bf16", "fo1_decode_logprob_record"):
        assert name in L.SIGNATURES
    lib = L.load()
    assert lib.fo1_abi_version() == 9
    P = [4096 * (i + 1) for i in range(9)]      # fake device pointers: every call below is rejected before any HIP call
    LG, IDS, LP, TI, TL, WANT, ST, NREC, GEN = P

    def rows(**k):
        a = dict(logits=LG, ld=4096, V=4096, B=4, ids=IDS, top_n=3, lp=LP, ti=TI, tl=TL, top_ld=8)
        a.update(k)
        return lib.fo1_logprob_rows_bf16(a["logits"], a["ld"], a["V"], a["B"], a["ids"], a["top_n"], a["lp"], a["ti"], a["tl"], a["top_ld"], None)

    def record(**k):
        a = dict(logits=LG, ld=4096, V=4096, B=4, want=WANT, state=ST, ids=GEN, ids_ld=64, n_rec=NREC, lp=LP, ti=TI, tl=TL)
        a.update(k)
        return lib.fo1_decode_logprob_record(a["logits"], a["ld"], a["V"], a["B"], a["want"], a["state"], a["ids"], a["ids_ld"], a["n_rec"], a["lp"],
                                             a["ti"], a["tl"], None)

    common = ((dict(B=0), b"B=0"), (dict(B=257), b"B=257"), (dict(ld=4095), b"ld_logits=4095"), (dict(V=0), b"n_vocab=0"), (dict(logits=None), b"NULL"),
              (dict(lp=None), b"NULL"))
    for call, prefix, own in ((rows, b"logprob_rows", ((dict(ids=None), b"NULL"), (dict(top_n=-1), b"top_n=-1"), (dict(top_n=9), b"top_n=9"),
                                                       (dict(ti=None), b"NULL top output"), (dict(tl=None), b"NULL top output"),
                                                       (dict(top_ld=2), b"top_ld=2"))),
                              (record, b"decode_logprob_record", ((dict(want=None), b"NULL"), (dict(state=None), b"NULL"), (dict(ids=None), b"NULL"),
                                                                  (dict(n_rec=None), b"NULL"), (dict(ti=None), b"NULL"), (dict(tl=None), b"NULL"),
                                                                  (dict(ids_ld=0), b"ids_ld=0")))):
        for kw, word in common + own:
            assert call(**kw) == -1, (prefix, kw)
            msg = lib.fo1_last_error()
            assert msg.startswith(prefix + b":") and word in msg, msg


def _model():
    m = FO1ForCausalLM.__new__(FO1ForCausalLM)
    m.config = FO1HFConfig({}, {"eos_token_id": 7, "top_k": 20})
    return m


def test_generate_keywords_and_errors():
    sig = inspect.signature(FO1ForCausalLM.generate)
    assert sig.parameters["output_logprobs"].default is False and sig.parameters["top_logprobs"].default == 0
    plan = FO1ForCausalLM._logprob_plan
    assert plan({}) is None and plan(dict(output_logprobs=False, top_logprobs=0)) is None
    assert plan(dict(output_logprobs=True)) == 0 and plan(dict(output_logprobs=True, top_logprobs=8)) == 8
    m = _model()
    for kw in (dict(output_logprobs=True, top_logprobs=9), dict(output_logprobs=True, top_logprobs=-1), dict(output_logprobs=True, top_logprobs=2.5),
               dict(output_logprobs=True, top_logprobs=True)):
        with pytest.raises(ValueError, match="top_logprobs must be an integer in 0..8"):
            m.generate(inputs=torch.zeros(1, 4, dtype=torch.long), **kw)
    with pytest.raises(ValueError, match="top_logprobs needs output_logprobs=True"):
        m.generate(inputs=torch.zeros(1, 4, dtype=torch.long), top_logprobs=3)
    with pytest.raises(ValueError, match="keeps at most 4096 records"):
        m.generate(inputs=torch.zeros(1, 4, dtype=torch.long), output_logprobs=True, max_new_tokens=4097)


def test_batch_plan_accepts_requests_that_differ_only_in_the_logprob_keywords():
    m = _model()
    base = dict(max_new_tokens=8)
    # the requests pass every check of the plan and fail only where the requests themselves are read (there are none here) — as a uniform
    # batch does (tests/test_sampling_surface.py)
    for batch in ([base, dict(base, output_logprobs=True)], [dict(base, output_logprobs=True, top_logprobs=3), dict(base, output_logprobs=True, top_logprobs=8)],
                  [dict(base, do_sample=True, temperature=0.7, seed=3, output_logprobs=True, top_logprobs=1), dict(base, do_sample=True, temperature=0.7, seed=3)]):
        with pytest.raises(ValueError, match="inputs"):
            m._batch_plan(batch)
    with pytest.raises(ValueError, match="top_logprobs must be an integer in 0..8"):
        m._batch_plan([base, dict(base, output_logprobs=True, top_logprobs=9)])
    with pytest.raises(ValueError, match="top_logprobs needs output_logprobs=True"):
        m._batch_plan([base, dict(base, top_logprobs=2)])


def test_the_loops_logprobs_argument():
    from vlm_fo1_amd.llm import BatchDecoder, DecodePool, logprob_wants
    from vlm_fo1_amd.model import FO1Engine
    from vlm_fo1_amd.serving import PoolGroup, PoolHandle, PoolService
    assert logprob_wants(None, 3) == [-1, -1, -1] and logprob_wants(2, 2) == [2, 2] and logprob_wants([None, 0, 8], 3) == [-1, 0, 8]
    for bad in ([9], [-1], [1.5], [True]):
        with pytest.raises(ValueError, match="top-n must be an integer in 0..8"):
            logprob_wants(bad, 1)
    with pytest.raises(ValueError, match="2 entries for 3 sequences"):
        logprob_wants([1, 2], 3)
    for fn in (BatchDecoder.start, DecodePool.join, PoolService.submit, PoolGroup.submit, FO1Engine.submit_batch, FO1Engine.generate_batch):
        assert inspect.signature(fn).parameters["logprobs"].default is None, fn
    h = PoolHandle(2)
    h._set(0, [1, 2])
    h._set(1, [3], "rec")
    assert h.result() == [[1, 2], [3]] and h.logprobs() == [None, "rec"]
