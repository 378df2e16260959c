"""CPU checks of the steering surface: FO1ForCausalLM._steer_plan / _decode_plan (the keyword forms, their errors, "off" is today's plan),
the engine's token_steer and sampling_table, the BiasTable's acquire / release / room bookkeeping, the mixed-batch refusal of generate_many,
and the C ABI additions (include/fo1.h, the library's exports, lib.SIGNATURES and the argument checks, which run before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
from vlm_fo1_amd import lib as L, ops
from vlm_fo1_amd.llm import BiasTable, DecodePool, bf16_bits, has_steer, sampling_steers, sampling_table, token_steer

splan = FO1ForCausalLM._steer_plan
dplan = FO1ForCausalLM._decode_plan
V = 4099


def test_off_is_the_plan_it_was():
    for kw in ({}, dict(logit_bias=None), dict(logit_bias={}), dict(logit_bias={5: 0.0}), dict(sequence_bias={}), dict(sequence_bias=[]),
               dict(frequency_penalty=0, presence_penalty=0.0), dict(frequency_penalty=None, presence_penalty=None),
               dict(logit_bias={5: 1.5}, sequence_bias={(5,): -1.5})):
        assert splan(kw) is None, kw
        assert dplan(kw, None, (7,)) is None, kw      # plain greedy: the same object (None) as without the keywords
        sampled = dict(kw, do_sample=True, temperature=0.7, seed=3)
        assert dplan(sampled, None, (7,)) == dplan(dict(do_sample=True, temperature=0.7, seed=3), None, (7,)) == \
            dict(temperature=0.7, top_p=1.0, top_k=50, seed=3)
    # ... and the engine plans such a dict as one without the keys: a plain draw, no steer
    for sp in (dict(temperature=0.7, seed=1), dict(temperature=0.7, seed=1, bias={}, frequency_penalty=0.0, presence_penalty=None),
               dict(temperature=0.7, seed=1, bias={3: 0.0, 4: -0.0})):
        assert not has_steer(sp) and token_steer(sp, V) is None
        assert sampling_table([sp], 1)[1] == ["sampled"]
    assert sampling_table([None], 1)[1] == ["plain"]


def test_keyword_forms_and_their_sum():
    assert splan(dict(logit_bias={5: 1.5, 9: -2})) == dict(bias={5: 1.5, 9: -2.0})
    assert splan(dict(logit_bias={"5": 1.5})) == dict(bias={5: 1.5})                                 # an OpenAI-shaped caller's string keys
    assert splan(dict(logit_bias={np.int64(5): np.float32(1.5), torch.tensor(9): torch.tensor(2.0)})) == dict(bias={5: 1.5, 9: 2.0})
    assert splan(dict(sequence_bias={(5,): 1.5, (9,): -2.0})) == dict(bias={5: 1.5, 9: -2.0})        # HF's dict form
    assert splan(dict(sequence_bias=[[[5], 1.5], [[9], -2.0]])) == dict(bias={5: 1.5, 9: -2.0})      # HF's list form
    assert splan(dict(sequence_bias=[[torch.tensor([5]), 1.5]])) == dict(bias={5: 1.5})
    # both keywords: summed per id before any rounding; an id whose sum is 0 has no bias
    assert splan(dict(logit_bias={5: 1.5, 9: 1.0}, sequence_bias={(5,): 0.25, (9,): -1.0, (11,): 3.0})) == dict(bias={5: 1.75, 11: 3.0})
    assert splan(dict(frequency_penalty=0.25, presence_penalty=-1)) == dict(frequency_penalty=0.25, presence_penalty=-1.0)
    assert splan(dict(presence_penalty=np.float32(0.5))) == dict(presence_penalty=0.5)
    # the plan the engine takes: a greedy request becomes dict(greedy=True, ...), a sampled one keeps its parameters
    assert dplan(dict(logit_bias={5: 1.5}, presence_penalty=1.0), None, (7,)) == dict(greedy=True, bias={5: 1.5}, presence_penalty=1.0)
    full = dplan(dict(do_sample=True, temperature=0.7, seed=3, logit_bias={5: 1.5}, frequency_penalty=0.5, repetition_penalty=1.3, suppress_tokens=[4]), None, (7,))
    assert full == dict(temperature=0.7, top_p=1.0, top_k=50, seed=3, repetition_penalty=1.3, ban=(4,), bias={5: 1.5}, frequency_penalty=0.5)
    assert sampling_table([full], 1)[1] == ["general"] and sampling_table([dict(greedy=True, presence_penalty=1.0)], 1)[1] == ["general"]


@pytest.mark.parametrize("kw, err, match", [
    (dict(logit_bias=[5, 1.0]), ValueError, "logit_bias: a dict"),
    (dict(logit_bias={5.0: 1.0}), ValueError, "token ids are integers"),
    (dict(logit_bias={True: 1.0}), ValueError, "token ids are integers"),
    (dict(logit_bias={"five": 1.0}), ValueError, "token ids are integers"),
    (dict(logit_bias={5: True}), ValueError, "finite number"),
    (dict(logit_bias={5: None}), ValueError, "finite number"),
    (dict(logit_bias={5: "high"}), ValueError, "finite number"),
    (dict(logit_bias={5: float("inf")}), ValueError, "suppress_tokens"),
    (dict(logit_bias={5: float("-inf")}), ValueError, "suppress_tokens"),
    (dict(logit_bias={5: float("nan")}), ValueError, "finite number"),
    (dict(logit_bias={5: 1e39}), ValueError, "finite number"),
    (dict(sequence_bias={(5, 6): 1.0}), NotImplementedError, r"single-token entries.*\[5, 6\]"),
    (dict(sequence_bias=[[[5, 6, 7], 1.0]]), NotImplementedError, r"single-token entries.*\[5, 6, 7\]"),
    (dict(sequence_bias={(): 1.0}), NotImplementedError, "single-token entries"),
    (dict(sequence_bias="abc"), ValueError, "sequence_bias"),
    (dict(sequence_bias=[[[5], 1.0, 2.0]]), ValueError, "an entry is"),
    (dict(frequency_penalty=True), ValueError, "frequency_penalty"),
    (dict(presence_penalty=False), ValueError, "presence_penalty"),
    (dict(frequency_penalty=float("nan")), ValueError, "frequency_penalty"),
    (dict(presence_penalty=float("inf")), ValueError, "presence_penalty"),
    (dict(presence_penalty=1e39), ValueError, "presence_penalty"),
    (dict(frequency_penalty="high"), ValueError, "frequency_penalty"),
])
def test_steer_plan_errors(kw, err, match):
    with pytest.raises(err, match=match):
        splan(kw)


def test_token_steer_rounds_to_bf16_once_and_checks_the_vocabulary():
    t = token_steer(dict(greedy=True, bias={5: 0.1, 4098: -2.0, 7: 0.0}, frequency_penalty=0.1), V)
    row = np.frombuffer(t.bias, dtype=np.uint16)
    assert len(row) == ops.count_words(V) == 4104 and np.nonzero(row)[0].tolist() == [5, 4098]
    assert row[5] == 0x3dcd and row[4098] == 0xc000      # bf16(0.1) = 0.10009765625, -2
    assert t.f == float(np.float32(0.1)) and t.q == 0.0 and t.counting
    assert token_steer(dict(greedy=True, bias={5: 1.0}), V).counting is False
    only = token_steer(dict(greedy=True, presence_penalty=0.5), V)
    assert only.bias is None and only.counting
    assert token_steer(dict(greedy=True, bias={5: 1e-45}), V) is None      # rounds to zero: no bias, no steer
    assert (bf16_bits([1.0, -0.0, 3.0e38, np.inf, np.nan]) == [0x3f80, 0x8000, 0x7f62, 0x7f80, 0x7fc0]).all()
    for bad, match in ((dict(bias={V: 1.0}), "outside"), (dict(bias={-1: 1.0}), "outside"), (dict(bias={1.5: 1.0}), "integers"),
                       (dict(bias=[(1, 1.0)]), "a dict"), (dict(bias={1: "x"}), "is a number"), (dict(bias={1: True}), "is a number"),
                       (dict(bias={1: float("inf")}), "use `ban`"), (dict(bias={1: 3.4e38}), "use `ban`"), (dict(bias={1: float("nan")}), "use `ban`"),
                       (dict(frequency_penalty=float("nan")), "frequency_penalty"), (dict(presence_penalty=True), "presence_penalty"),
                       (dict(presence_penalty=1e39), "presence_penalty")):
        with pytest.raises(ValueError, match=match):
            token_steer(dict(greedy=True, **bad), V)
    per = [None, dict(greedy=True, bias={1: 2.0}), dict(temperature=1.0, seed=0)]
    st = sampling_steers(per, 3, V)
    assert st[0] is None and st[2] is None and st[1].bias is not None
    # equal biases give equal bytes whatever the order of the dict and the type of the numbers: they share a table row
    assert token_steer(dict(bias={1: 2.0, 9: 0.5}), V).bias == token_steer(dict(bias={9: np.float32(0.5), 1: 2}), V).bias
    # the table rows ops builds: (bias_row, f, q, 0) as int32 / fp32 bit patterns
    tab = ops.token_steers([None, (3, 0.25, -1.0)])
    assert tab.tolist() == [[-1, 0, 0, 0], [3, 0x3e800000, -0x40800000, 0]] and tab.dtype == torch.int32
    assert ops.count_penalty_on(0.0, 1.0) and ops.count_penalty_on(-0.5, 0.0) and not ops.count_penalty_on(0.0, 0.0)
    assert not ops.count_penalty_on(float("nan"), 1.0) and not ops.count_penalty_on(1.0, 1e39) and not ops.count_penalty_on(None, None)


def _bias(i, v=1.0):
    return token_steer(dict(bias={i: v}), V).bias


def test_bias_table_acquire_release_and_room():
    bt = BiasTable(4, V, "cpu")
    a, b, c, d, e = (_bias(i) for i in range(5))
    assert bt.room([a, b, c, d]) and not bt.room([a, b, c, d, e]) and bt.room([a, a, a, a, a])
    ra, rb = bt.acquire(a), bt.acquire(b)
    assert (ra, rb) == (0, 1) and bt.acquire(a) == 0 and bt.users == [2, 1, 0, 0]
    # the table row holds the bias, the gate its non-zero entries
    assert bt.table[0].view(torch.int16).numpy().view(np.uint16).tolist() == np.frombuffer(a, np.uint16).tolist()
    g = bt.gate.numpy().view(np.uint32)
    assert g[0, 0] == 1 and g[1, 0] == 2 and not g[0, 1:].any() and not g[2:].any()
    last = token_steer(dict(bias={V - 1: -0.5, 64: 1.0}), V).bias
    rl = bt.acquire(last)
    gl = bt.gate.numpy().view(np.uint32)[rl]
    assert gl[2] == 1 and gl[(V - 1) >> 5] == 1 << ((V - 1) & 31) and np.count_nonzero(gl) == 2
    assert bt.room([c]) and not bt.room([c, d]) and bt.room([a, b, last, c])
    rc = bt.acquire(c)
    assert sorted((ra, rb, rl, rc)) == [0, 1, 2, 3] and not bt.room([d]) and bt.room([a])
    with pytest.raises(RuntimeError, match="4 different logit-bias vectors are live"):
        bt.acquire(d)
    bt.release(ra)
    assert not bt.room([d])      # a still has a user
    bt.release(ra)
    assert bt.room([d]) and bt.room([a]) and not bt.room([d, e])
    # a row without users keeps its content until it is needed: a comes back to its row without an upload, d takes it otherwise
    assert bt.acquire(a) == ra
    bt.release(ra)
    assert bt.acquire(d) == ra and bt.users[ra] == 1
    assert bt.table[ra].view(torch.int16).numpy().view(np.uint16).tolist() == np.frombuffer(d, np.uint16).tolist()
    bt.release(-1)      # (a steer without a bias holds no row)
    with pytest.raises(ValueError, match="bytes"):
        bt.acquire(a[:-2])
    # the bookkeeping alone, as the pool asks before it has allocated anything
    assert BiasTable(2, V, None).room([a, b]) and BiasTable(2, V, None).acquire(a) == 0


def test_the_pools_room_check_knows_the_bias_table():
    pool = DecodePool.__new__(DecodePool)
    pool.btab, pool.masks, pool.gtab = None, None, None
    st = lambda n: sampling_steers([dict(greedy=True, bias={i: 1.0}) for i in range(n)], n, V)      # noqa: E731
    assert DecodePool.MAX_BIAS == 16
    assert pool._table_without_room([None] * 16, (), st(16)) is None
    assert "16 different logit-bias vectors" in pool._table_without_room([None] * 17, (), st(17))
    assert pool._table_without_room([None] * 40, (), sampling_steers([dict(greedy=True, bias={1: 1.0}, stream=i) for i in range(40)], 40, V)) is None
    assert pool._table_without_room([None], (), sampling_steers([dict(greedy=True, presence_penalty=1.0)], 1, V)) is None
    pool.btab = BiasTable(16, V, None)
    for t in st(16):
        pool.btab.acquire(t.bias)
    assert pool._table_without_room([None], (), st(1)) is None and pool._mask_room([None], (), st(3))
    assert "logit-bias" in pool._table_without_room([None], (), sampling_steers([dict(greedy=True, bias={99: 1.0})], 1, V))


def test_generate_many_refuses_a_batch_mixed_in_the_steering_keywords():
    m = FO1ForCausalLM.__new__(FO1ForCausalLM)
    m.config = FO1HFConfig({}, {"eos_token_id": 7})
    base = dict(max_new_tokens=8, logit_bias={5: 1.0}, presence_penalty=0.5)
    for other in (dict(base, logit_bias={5: 2.0}), dict(base, presence_penalty=0.0), dict(base, frequency_penalty=0.1), dict(max_new_tokens=8)):
        with pytest.raises(ValueError, match="steering keywords"):
            m._batch_plan([base, other])
    with pytest.raises(NotImplementedError):
        m._batch_plan([base, dict(base, sequence_bias={(1, 2): 1.0})])


def test_header_exports_and_signatures_agree():
    hdr = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "fo1.h")).read()
    lib = L.load()
    closing = dict(rows=L.SIGNATURES["fo1_sample_rows_closing_bf16"][1], accept=L.SIGNATURES["fo1_decode_head_closing_accept"][1])
    extra = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong,
             ctypes.c_void_p]
    for name, form in (("fo1_sample_rows_steered_bf16", "rows"), ("fo1_decode_head_steered_accept", "accept")):
        assert hasattr(lib, name) and L.SIGNATURES[name] == (ctypes.c_int, closing[form] + extra)      # the _closing entry's list plus nine
        decl = re.search(r"int " + name + r"\((.*?)\);", hdr, re.S).group(1)
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert len(params) == len(L.SIGNATURES[name][1])
        assert [p.split()[-1].lstrip("*") for p in params[-9:]] == ["bias", "bias_gate", "bias_rows", "ld_bias", "counts", "count_gate", "ld_counts",
                                                                  "gate_ld_words", "steers"]
    assert hasattr(lib, "fo1_count_mark") and len(L.SIGNATURES["fo1_count_mark"][1]) == 9
    steer = re.search(r"typedef struct fo1_token_steer \{(.*?)\} fo1_token_steer_t;", hdr, re.S).group(1)
    fields = re.findall(r"(int32_t|float) (\w+);", steer)
    assert fields == [("int32_t", "bias_row"), ("float", "frequency_penalty"), ("float", "presence_penalty"), ("int32_t", "reserved")]      # 16 bytes
    assert lib.fo1_abi_version() == 9


def test_argument_checks_run_before_any_launch():
    lib = L.load()
    ok = 0x1000      # (never dereferenced: every call below fails its checks first)
    V_, B = 4099, 4
    ldw = ops.seen_words(V_)

    def rows(**kw):
        a = dict(bias=ok, bias_gate=ok, bias_rows=1, ld_bias=V_, counts=ok, count_gate=ok, ld_counts=V_ + 1, gate_ld_words=ldw, steers=ok)
        a.update(kw)
        return lib.fo1_sample_rows_steered_bf16(ok, V_, V_, B, ok, None, 1, None, ok, ok, 4096, None, 0, None, 0, 0, None, None,
                                                None, 0, 0, None, 0, None, 0, None, None, None, 0, None, None,
                                                a["bias"], a["bias_gate"], a["bias_rows"], a["ld_bias"], a["counts"], a["count_gate"], a["ld_counts"],
                                                a["gate_ld_words"], a["steers"])
    for bad in (dict(bias_gate=None), dict(count_gate=None), dict(bias_rows=0), dict(ld_bias=V_ - 1), dict(ld_counts=V_), dict(ld_counts=V_ - 1),
                dict(gate_ld_words=ldw - 4), dict(gate_ld_words=ldw + 1), dict(bias=ok + 1), dict(counts=ok + 2), dict(bias_gate=ok + 2),
                dict(steers=ok + 1)):
        assert rows(**bad) != 0, bad
    assert lib.fo1_count_mark(None, V_ + 1, ok, ldw, V_, ok, ok, 1, None) != 0
    assert lib.fo1_count_mark(ok, V_, ok, ldw, V_, ok, ok, 1, None) != 0            # an odd ld_counts
    assert lib.fo1_count_mark(ok, V_ + 1, ok, ldw - 4, V_, ok, ok, 1, None) != 0
    assert lib.fo1_count_mark(ok, V_ + 1, ok, ldw, V_, None, None, 0, None) == 0    # nothing to mark: no launch
