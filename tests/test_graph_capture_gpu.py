"""ops.capture_graph / ops.replay_graph, the one recipe every hipGraph of the package is captured with: warm-up on a side stream,
roll back, capture, replay under the shared side of the capture lock.  No engine: tensors of 8 int32 and one project launch."""
import pytest
import torch

from vlm_fo1_amd import ops

pytestmark = pytest.mark.gpu


def _lock_is_free():
    return ops.graph_lock._writer is False and ops.graph_lock._readers == 0


def test_the_warm_up_is_rolled_back_and_every_replay_runs_once():
    x = torch.zeros(8, dtype=torch.int32, device="cuda")
    g, out = ops.capture_graph(lambda: x.add_(1), rollback=(x,))
    torch.cuda.synchronize()
    assert out is x
    assert x.cpu().tolist() == [0] * 8, "the warm-up was rolled back and the capture itself executed nothing"
    for _ in range(3):
        ops.replay_graph(g)
    torch.cuda.synchronize()
    assert x.cpu().tolist() == [3] * 8
    assert _lock_is_free()


def test_without_rollback_the_warm_up_step_stays():
    x = torch.zeros(8, dtype=torch.int32, device="cuda")
    g, _ = ops.capture_graph(lambda: x.add_(1))
    torch.cuda.synchronize()
    assert x.cpu().tolist() == [1] * 8, "the contract: what the warm-up changed and `rollback` does not name stays changed"
    ops.replay_graph(g)
    torch.cuda.synchronize()
    assert x.cpu().tolist() == [2] * 8


def test_a_capture_under_inference_mode_makes_ordinary_tensors():
    x = torch.arange(8, dtype=torch.int32, device="cuda")
    with torch.inference_mode():
        g, y = ops.capture_graph(lambda: x + 1)
        assert not y.is_inference()
    assert not y.is_inference() and not torch.is_inference_mode_enabled()
    x.mul_(2)                      # the caller's in-place refresh of a static input, outside inference mode
    ops.replay_graph(g)
    torch.cuda.synchronize()
    assert y.cpu().tolist() == [2 * i + 1 for i in range(8)]


def test_the_lock_is_released_after_a_return_and_after_a_run_that_raises():
    x = torch.zeros(8, dtype=torch.int32, device="cuda")
    ops.capture_graph(lambda: x.add_(1), rollback=(x,))
    assert _lock_is_free()

    def run():                     # raises on the warm-up call, before it touches any tensor: nothing is launched
        raise RuntimeError("refused")

    with torch.inference_mode():
        with pytest.raises(RuntimeError, match="refused"):
            ops.capture_graph(run, rollback=(x,))
        assert torch.is_inference_mode_enabled(), "the caller's mode is back"
    assert _lock_is_free()
    g, _ = ops.capture_graph(lambda: x.add_(1), rollback=(x,))      # and the next capture goes through
    ops.replay_graph(g)
    torch.cuda.synchronize()
    assert x.cpu().tolist() == [1] * 8 and _lock_is_free()


def test_a_project_launch_replays_on_refreshed_inputs():
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(8, 8, generator=gen).bfloat16().cuda()
    b = torch.randn(8, 8, generator=gen).bfloat16().cuda()
    g, out = ops.capture_graph(lambda: ops.add(a, b))
    stale = ops.add(a, b)
    a.copy_(torch.randn(8, 8, generator=gen).bfloat16())
    ops.replay_graph(g)
    torch.cuda.synchronize()
    got = out.clone()
    assert torch.equal(got, ops.add(a, b)), "replay on the new input = the eager launch on the new input"
    assert not torch.equal(got, stale), "and not the sum the capture's warm-up saw"
