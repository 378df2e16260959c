"""The prefill / window attention tolerance can fail (CPU, no GPU): on every case the GPU sweep uses (tests/prefill_attention_cases.SWEEP;
segments capped at 1100 rows here to keep the run short) the emulated kernel roundings stay within TOL / 2 of the fp64 reference, and
every fault of prefill_attention_cases.FAULTS that applies to the case moves some row of every unit (segment, window, prefix item) it
changes by at least 2 TOL — and changes at least one unit of the case:
  * drop_first / drop_last / drop_tile_lo / drop_tile_hi: one key of the own range left out (the first, the last, either side of the first
    key-tile boundary past kv_start);
  * leak_after / leak_before: kv_end or kv_start - 1 included (leak_after: non-causal ranges only, a causal mask hides kv_end);
  * zero_key: one more key with a zero K row and V column (a guarded load past the range whose mask is missing);
  * causal_ahead / no_self: key q + 1 visible, or key q hidden;
  * head_map: query head h read against KV head h % KV instead of h // group;
  * prefix_end+1 / prefix_end-1 / prefix_skip: the shared-prefix range off by one, or skipped;
  * swin_no_mask / swin_region_off: no shift-region mask, or its Hp - shift boundary one row up;
  * bias_transposed / bias_head: bias[h][j][i], or the bias of head h + 1;
  * pad_zero / pad_drop: the map form's padded tokens read as zeros, or left out;
  * row_base_off: *q_row_base off by one."""
import pytest

import prefill_attention_cases as C


def _cpu_cases():
    return [C.scale_down(c) for c in C.SWEEP]


@pytest.mark.parametrize("case", _cpu_cases(), ids=lambda c: c.name)
def test_tolerance_passes_the_emulated_kernel_and_fails_every_fault(case):
    d = C.build(case)
    ref = C.reference(d)
    emu = C.row_ratios(C.emulate(d), ref)
    worst = emu[~emu.isnan()].max().item()
    assert worst <= C.TOL / 2, f"emulated kernel roundings {worst:.4g} of the row maximum: TOL {C.TOL:.4g} leaves no margin"
    faults = C.applicable_faults(case, d)
    assert faults, case.name
    for fault in faults:
        mut = C.reference(d, fault)
        hit = 0
        for un in d["units"]:
            changed, w = C.unit_worst(mut, ref, un)
            if not changed:
                continue
            hit += 1
            assert w >= 2.0, f"{case.name} {un.label}: '{fault}' is only {w:.3g} x TOL off the reference"
        assert hit, f"{case.name}: '{fault}' changes no unit"
