"""The decode attention tolerance can fail (CPU, no GPU): on every case the GPU tests use (tests/decode_attention_cases.ALL_CASES: the route
sweep, the o-projection, single-sequence, tiles-per-item and graph-replay cases; contexts capped at 2048 keys here to keep the run short) the emulated kernel roundings stay within TOL / 2 of the fp64 reference, and each of these wrong
computations exceeds TOL at least twice on every live sequence:
  * one planted key dropped (the first, the last, the one after the first 64-key boundary);
  * one poison row included (kv_start - 1 or pos + 1);
  * kv_start off by one (either way; the single-sequence entry's range starts at row 0: one way);
  * query head h read against KV head h % KV instead of h // group (only where the two maps differ)."""
import pytest
import torch

import decode_attention_cases as C


def _worst_per_sequence(mut, ref, state):
    r = C.row_ratios(mut, ref).amax(-1) / C.TOL            # [B]: the worst head of each sequence, in units of TOL
    return [(b, r[b].item()) for b in range(ref.shape[0]) if not int(state[b, 3])]


def _cpu_cases():
    seen, out = set(), []
    for c in C.ALL_CASES:
        c = C.scale_down(c, 2048)
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _cpu_cases(), ids=lambda c: c.name)
def test_tolerance_passes_the_emulated_kernel_and_fails_every_mutation(case):
    d = C.build(case)
    ref = C.reference(d)
    st = d["state"]
    emu = C.row_ratios(C.emulate(d), ref).max().item()
    assert emu <= C.TOL / 2, f"emulated kernel roundings {emu:.4g} of the row maximum: TOL {C.TOL:.4g} leaves no margin"
    muts = {
        "drop first key": dict(drop_rel=0),
        "drop last key": dict(drop_rel=-1),
        "drop key 64": dict(drop_rel=64),
        "poison pos + 1": dict(hi_delta=1),
        "kv_start + 1": dict(lo_delta=1),
    }
    if not case.single:                             # (the single-sequence entry's keys start at row 0)
        muts["kv_start - 1"] = dict(lo_delta=-1)
    if case.Hq != case.Hkv:
        muts["head h -> h % KV"] = dict(head_map=lambda h: h % case.Hkv)
    for what, m in muts.items():
        drop_rel = m.pop("drop_rel", None)
        if drop_rel is None:
            mut = C.reference(d, **m)
        else:
            mut = torch.zeros_like(ref)
            for b in range(case.B):
                n = d["ctx"][b]
                r = n - 1 if drop_rel < 0 else drop_rel
                if r >= n:                          # no such key in this context: nothing to drop
                    mut[b] = torch.nan
                    continue
                mut[b] = C.reference(d, drop=(r,), seqs=(b,))[b]
        for b, worst in _worst_per_sequence(mut, ref, st):
            if torch.isnan(mut[b]).all():
                continue
            assert worst >= 2.0, f"{case.name} sequence {b} (ctx {d['ctx'][b]}): '{what}' is only {worst:.3g} x TOL off the reference"
