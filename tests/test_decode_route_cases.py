"""The decode-route logit bound can fail (CPU, no GPU): tests/decode_route_cases.BOUND against the cases every route of
tests/test_decode_routes_gpu.py decodes.
  * the memoised teacher-forced oracle is LO.greedy_decode(..., forced=ids), bit for bit;
  * a float64 run differs from the fp32 oracle by far less than BOUND;
  * the q/k scaling peaks decode attention (largest weight well above uniform);
  * noise: the oracle with bf16 rounding at the engine's rounding points stays within BOUND / 2 of the fp32 oracle on every case;
  * sensitivity: each decode-step fault (position without the rope delta, the new K/V row missing at its own step, the first key dropped,
    a neighbour sequence's K/V row read for the first key, the previous step's K row left at the current position) moves some logit row
    by at least 2 x BOUND."""
import pytest
import torch

import decode_route_cases as C
from oracle import llm_oracle as LO


def test_memoised_oracle_is_teacher_forced_greedy_decode():
    O = C.Oracle()
    ids = O.greedy("s40")
    forced = ids[:5] + [7, 7, 4000] + ids[8:]           # somebody else's ids part of the way
    x, pos, delta = C.inputs("s40")
    ref_ids, ref = LO.greedy_decode(C.state(), x, pos, delta, len(forced), forced=forced, **C.KW)
    assert torch.equal(O.logits("s40", forced), ref)
    assert ref_ids[:5] == ids[:5]
    assert torch.equal(O.logits("s40", ids[:3] + [1]), ref[:4])        # a memoised prefix


def test_float64_run_is_far_inside_the_bound(capsys):
    ids = C.Oracle.get().greedy("s250")
    ref = C.Oracle.get().logits("s250", ids)
    d = (C.run("s250", ids, dtype=torch.float64) - ref.double()).abs().max().item()
    with capsys.disabled():
        print(f"\n[decode routes] float64 oracle vs fp32 oracle (s250): {d:.2e} = {d / C.BOUND:.1e} x BOUND")
    assert d <= C.BOUND / 100


def test_q_k_scaling_peaks_decode_attention(capsys):
    med, frac = C.peak_stats(["s40", "s250", "s1000"])
    with capsys.disabled():
        print(f"\n[decode routes] largest attention weight x keys: median {med:.1f}, >= 8 in {100 * frac:.0f} % of (layer, head, step)")
    assert med >= 16 and frac >= 0.8


def test_bound_noise_and_fault_sensitivity(capsys):
    O = C.Oracle.get()
    noise = {}
    for s in C.SEQS:
        ids = O.greedy(s.name)
        emu = C.run(s.name, ids, bf16=True)
        noise[s.name] = (emu - O.logits(s.name, ids)).abs().max().item()
    worst = max(noise, key=noise.get)
    effect = {f: 0.0 for f in C.FAULTS}
    for s in C.KEY:
        ids = O.greedy(s.name)
        pre = C.forward(*C.inputs(s.name)[:2])
        base = C.run(s.name, ids, prefill=pre)
        for f in C.FAULTS:
            mut = C.run(s.name, ids, fault=f, key=0, neighbour="s2040" if s.name != "s2040" else "s1000", prefill=pre)
            effect[f] = max(effect[f], (mut - base).abs().max().item())
    weakest = min(effect, key=effect.get)
    with capsys.disabled():
        print(f"\n[decode routes] BOUND {C.BOUND} (absolute logit error); worst bf16 noise {noise[worst] / C.BOUND:.2f} x BOUND ({worst}); "
              f"smallest fault effect {effect[weakest] / C.BOUND:.1f} x BOUND ({weakest}); "
              + ", ".join(f"{f} {e / C.BOUND:.1f}" for f, e in effect.items()))
    assert noise[worst] <= C.BOUND / 2, f"bf16 rounding noise {noise[worst]:.3f} on {worst}: BOUND {C.BOUND} leaves no margin"
    for f, e in effect.items():
        assert e >= 2 * C.BOUND, f"fault '{f}' moves no logit row by 2 x BOUND (at most {e:.3f})"
