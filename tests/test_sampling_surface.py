"""CPU checks of the sampling surface: FO1ForCausalLM._sampling_plan (defaults, errors, seeding), the mixed-batch refusal of generate_many,
and the C ABI additions (lib.SIGNATURES, the library's exports and its argument checks, which run before any HIP call)."""
import pytest
import torch

from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
from vlm_fo1_amd import lib as L

plan = FO1ForCausalLM._sampling_plan


def test_sampling_is_on_iff_do_sample():
    assert plan({}, None) is None
    assert plan(dict(do_sample=False, temperature=0.7, top_p=0.9), None) is None         # as HF: a temperature alone decodes greedily
    assert plan(dict(do_sample=False, temperature=0.0), {"top_k": 20}) is None
    p = plan(dict(do_sample=True, temperature=0.7, top_p=0.9, seed=5), None)
    assert p == dict(temperature=0.7, top_p=0.9, top_k=50, seed=5)                       # HF's default top_k
    assert plan(dict(do_sample=True, temperature=1, seed=1), {"top_k": 20}) == dict(temperature=1.0, top_p=1.0, top_k=20, seed=1)
    assert plan(dict(do_sample=True, temperature=1.5, top_k=0, top_p=1.0, seed=2 ** 64 - 1), {"top_k": 20})["top_k"] == 0
    assert plan(dict(do_sample=True, temperature=1.5, top_k=7, seed=3), {"top_k": 20})["top_k"] == 7


def test_temperature_is_any_real_scalar_but_not_a_bool():
    import numpy as np
    for t in (np.float32(0.5), np.float64(0.5), torch.tensor(0.5), torch.tensor(0.5, dtype=torch.bfloat16), 0.5):
        p = plan(dict(do_sample=True, temperature=t, seed=1), None)
        assert p["temperature"] == 0.5 and type(p["temperature"]) is float
    assert plan(dict(do_sample=True, temperature=2, seed=1), None)["temperature"] == 2.0
    for t in (True, "hot", [0.5], torch.tensor([0.5, 0.7]), 1e-40, 1e300):      # (1e-40: its fp32 reciprocal overflows; 1e300: inf as fp32)
        with pytest.raises(ValueError, match="positive finite temperature"):
            plan(dict(do_sample=True, temperature=t, seed=1), None)


@pytest.mark.parametrize("bad", [dict(temperature=0.0), dict(temperature=None), dict(temperature=-1.0), dict(temperature=float("nan")),
                                 dict(temperature=float("inf")), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.5),
                                 dict(temperature=1.0, top_p=-0.1), dict(temperature=1.0, top_k=-1)])
def test_sampling_plan_errors(bad):
    with pytest.raises(ValueError):
        plan(dict(do_sample=True, seed=0, **bad), None)


def test_seed_comes_from_torchs_default_generator():
    kw = dict(do_sample=True, temperature=1.0)
    torch.manual_seed(1234)
    a, b = plan(kw, None)["seed"], plan(kw, None)["seed"]
    torch.manual_seed(1234)
    assert plan(kw, None)["seed"] == a != b and 0 <= a < 2 ** 63
    state = torch.get_rng_state()
    assert plan(dict(kw, seed=9), None)["seed"] == 9 and torch.equal(torch.get_rng_state(), state)      # an explicit seed draws nothing


def test_generate_many_refuses_a_mixed_batch():
    m = FO1ForCausalLM.__new__(FO1ForCausalLM)
    m.config = FO1HFConfig({}, {"eos_token_id": 7, "top_k": 20})
    base = dict(do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=8)
    for other in (dict(base, temperature=0.8), dict(base, top_p=0.5), dict(base, top_k=5), dict(base, do_sample=False), dict(base, temperature=0.0, do_sample=False)):
        with pytest.raises(ValueError, match="share do_sample, temperature, top_p and top_k"):
            m._batch_plan([base, other])
    with pytest.raises(ValueError, match="share max_new_tokens"):
        m._batch_plan([base, dict(base, max_new_tokens=9)])
    with pytest.raises(ValueError, match="share do_sample"):
        m._batch_plan([dict(max_new_tokens=8), base])
    with pytest.raises(ValueError, match="positive finite temperature"):       # no NotImplementedError any more: a bad request is a ValueError
        m._batch_plan([dict(do_sample=True, temperature=0.0)])
    # a uniform sampled batch passes the checks and fails only where the requests themselves are read (there are none here)
    with pytest.raises(ValueError, match="inputs"):
        m._batch_plan([dict(base, seed=3), dict(base, seed=3)])
    # one seed per batch (request i draws on stream i of it): an explicit seed that the others do not share is refused, not ignored
    for a, b in ((base, dict(base, seed=3)), (dict(base, seed=3), base), (dict(base, seed=3), dict(base, seed=4))):
        with pytest.raises(ValueError, match="share seed"):
            m._batch_plan([a, b])


def test_abi_additions():
    for name in ("fo1_sample_rows_workspace_bytes", "fo1_sample_rows_bf16", "fo1_decode_sample_accept"):
        assert name in L.SIGNATURES
    lib = L.load()
    assert lib.fo1_abi_version() == 9
    assert lib.fo1_sample_rows_workspace_bytes(151936, 32) > 0
    assert lib.fo1_sample_rows_workspace_bytes(151936, 257) == 0 and lib.fo1_sample_rows_workspace_bytes(0, 1) == 0
    P = [4096 * (i + 1) for i in range(8)]      # fake device pointers: every call below is rejected before any HIP call
    LG, PR, OUT, WS, ST, PL, IDS, DN = P

    def rows(**k):
        a = dict(logits=LG, ld=4096, V=4096, B=4, params=PR, out=OUT, ws=WS, wsb=1 << 12)
        a.update(k)
        return lib.fo1_sample_rows_bf16(a["logits"], a["ld"], a["V"], a["B"], a["params"], None, 1, None, a["out"], a["ws"], a["wsb"], None)

    def accept(**k):
        a = dict(logits=LG, ld=4096, V=4096, B=4, params=PR, state=ST, ids_ld=64, n_stop=0, wsb=1 << 12)
        a.update(k)
        return lib.fo1_decode_sample_accept(a["logits"], a["ld"], a["V"], a["B"], a["params"], a["state"], PL, IDS, a["ids_ld"], None, a["n_stop"], DN,
                                            WS, a["wsb"], None)

    for call, prefix in ((rows, b"sample_rows"), (accept, b"decode_sample_accept")):
        for kw, rc, word in ((dict(B=0), -1, b"B=0"), (dict(B=257), -1, b"B=257"), (dict(ld=4095), -1, b"ld_logits=4095"), (dict(V=0), -1, b"n_vocab=0"),
                             (dict(logits=None), -1, b"NULL"), (dict(params=None), -1, b"NULL"), (dict(wsb=8), -2, b"workspace")):
            assert call(**kw) == rc, (prefix, kw)
            msg = lib.fo1_last_error()
            assert msg.startswith(prefix + b":") and word in msg, msg
    assert rows(out=None) == -1 and b"NULL out" in lib.fo1_last_error()
    assert accept(state=None) == -1 and accept(ids_ld=0) == -1 and accept(n_stop=2) == -1 and b"bad arguments" in lib.fo1_last_error()
