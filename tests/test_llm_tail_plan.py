"""Host side of the trimmed last LLM layer (vlm_fo1_amd/llm.py: packed_item_rows / tail_item_rows / last_rows_of): the attention work
list the last layer runs when only each sequence's last real row is read after it.  For every needed row the reduced list must hold the
UNMODIFIED entry of the full list that contains it — same query block, same key range, same shared-prefix range — because that is what
makes the row's attention output the same bits as in the full launch; and it must hold nothing else.  No device needed: the planners
are host code."""
import pytest

from vlm_fo1_amd import lib as L
from vlm_fo1_amd.llm import LLMConfig, QwenLLM, last_rows_of, packed_item_rows, tail_item_rows
from vlm_fo1_amd.model import synthetic_prompt


def planner():
    llm = QwenLLM.__new__(QwenLLM)       # plan_batch / plan_inputs are host code over cfg alone: no weights, no device
    llm.cfg = LLMConfig()
    return llm


def bench_batch():
    """25 prompts of the benchmark's shape: 18 + 1 + 200 + 41 prompt entries over a 17 x 23 merged grid = 651 rows each, 100 regions."""
    n = 25
    prompts = [synthetic_prompt(100, n_text=60, seed=1234 + i) for i in range(n)]
    return dict(prompts=prompts, n_img=[391] * n, n_regions=[100] * n, grids_merged=[(17, 23)] * n)


def ragged_batch():
    shapes = [((18, 13), 7), ((12, 25), 33), ((2, 2), 1), ((15, 15), 100)]
    return dict(prompts=[synthetic_prompt(nb, vocab=4096, seed=i) for i, (_, nb) in enumerate(shapes)], n_img=[g[0] * g[1] for g, _ in shapes],
                n_regions=[nb for _, nb in shapes], grids_merged=[g for g, _ in shapes])


def shared_prefix_batch():
    """Three prompts over ONE image with the same preamble: the preamble and the image block (18 + 391 rows -> 408) run once."""
    prompts = [synthetic_prompt(nb, n_text=60, seed=50 + k, lead_seed=50) for k, nb in enumerate((100, 100, 37))]
    return dict(prompts=prompts, n_img=[391] * 3, n_regions=[100, 100, 37], grids_merged=[(17, 23)] * 3, img_base=[0, 0, 0], share_prefix=True)


CASES = {"bench_25x651": bench_batch, "ragged": ragged_batch, "shared_prefix": shared_prefix_batch}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reduced_list_is_one_unmodified_entry_per_sequence(name):
    llm = planner()
    c = llm.cfg
    hp = llm.plan_batch(**CASES[name]())
    seqs = hp["seqs"]
    if name == "bench_25x651":
        assert hp["rows"] == 25 * 652 and all(sq[1] == 651 for sq in seqs)      # 651 rows, padded to the packing granule
    if name == "shared_prefix":
        assert all(len(sq) == 5 and sq[4] == 408 and sq[3] == seqs[0][3] for sq in seqs), seqs
    needed = last_rows_of(seqs)
    assert needed == hp["last"][:, 1].tolist() and hp["last"][:, 0].tolist() == [0] * len(seqs)      # the gather plan the head uses names the same rows
    rows, rng, blk, _ = packed_item_rows(seqs, c.num_heads, c.head_dim, c.num_kv_heads)
    full = [tuple(r) + tuple(p) for r, p in zip(rows, rng)]
    assert len(set(full)) == len(full)
    t_rows, t_rng, flops = tail_item_rows(rows, rng, needed)
    tail = [tuple(r) + tuple(p) for r, p in zip(t_rows, t_rng)]
    assert len(tail) == len(seqs) < len(full) and flops > 0
    # every entry is an entry of the full list, unmodified, and the launch order of the full list is kept
    at = [full.index(e) for e in tail]
    assert at == sorted(at)
    # one entry per sequence: its last row lies in the entry's query block, and in no other entry's
    for r in needed:
        holds = [e for e in tail if e[0] <= r < e[1]]
        assert len(holds) == 1, (r, holds)
        q0, q1, k0, k1 = holds[0][:4]
        assert k0 <= q0 and q1 <= k1 and q1 - q0 <= blk
    if name == "shared_prefix":     # the prefix segment holds no last row and drops out; every kept entry still reads the prefix as its second range
        po, P = seqs[0][3], seqs[0][4]
        assert all(e[4:] == (po, po + P) for e in tail) and any(e[4:] == (0, 0) for e in full)
    else:
        assert all(e[4:] == (0, 0) for e in full)


def test_one_sequence_keeps_the_block_of_its_last_row():
    llm = planner()
    for L_ in (1, 64, 65, 515, 651, 652, 1500):
        rows, blk = llm._item_rows(0, L_)
        kept, _, _ = tail_item_rows(rows, [[0, 0]] * len(rows), [L_ - 1])
        assert len(kept) == 1 and kept[0] in rows and kept[0][0] <= L_ - 1 < kept[0][1] == L_


def test_new_entries_are_bound_and_exported():
    lib = L.load()
    for name in ("fo1_llm_prefill_tail", "fo1_llm_prefill_tail_workspace_bytes", "fo1_argmax_rows_bf16"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.fo1_llm_prefill_tail_workspace_bytes(None, 4) == 0
    assert lib.fo1_llm_prefill_tail(None, None, 0, None, 0, None, 1, None, None, None, None, 0, None) == -1 and b"NULL" in lib.fo1_last_error()
    assert lib.fo1_argmax_rows_bf16(None, 0, 16, 1, None, None, None) == -1
