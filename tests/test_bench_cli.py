"""bench.py's launcher contract (no GPU): `python bench.py --gpus N` starts itself, as a child process, as one rank per GPU under
torch.distributed.run on 127.0.0.1 (the docstring's own invocation used to assert out for N > 1), and the
measurement tool imports nothing from tests/."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_self_spawn_command():
    p = _run(["--gpus", "4", "--steps", "7", "--warmup", "2"], FO1_BENCH_SPAWN_DRYRUN="1")
    assert p.returncode == 0, p.stderr[-2000:]
    cmd = json.loads(p.stdout.strip().splitlines()[-1])
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 1024
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"]


def test_no_spawn_under_a_launcher_or_for_one_gpu():
    # under a launcher (WORLD_SIZE set) or with N = 1 the process goes straight on: on this box it stops at the GPU check
    for args, env in ((["--gpus", "2"], dict(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", FO1_BENCH_SPAWN_DRYRUN="1")),
                      (["--gpus", "1"], dict(FO1_BENCH_SPAWN_DRYRUN="1"))):
        p = _run(args, **env)
        assert "torch.distributed.run" not in p.stdout
        import torch
        if not torch.cuda.is_available():
            assert p.returncode != 0 and "bench.py needs a GPU" in p.stderr


def test_measurement_tools_do_not_import_tests():
    for f in ("bench.py", "__graft_entry__.py", "bench_workloads.py"):
        src = open(os.path.join(ROOT, f)).read()
        assert not re.search(r"""['"]tests['"]""", src), f"{f} puts tests/ on sys.path"
        assert "hfre_cases import" not in src.replace("fixtures.hfre_cases import", ""), f"{f} imports the test helper module"


def test_steps_must_be_positive():
    p = _run(["--gpus", "1", "--steps", "0"])
    assert p.returncode == 2 and "--steps must be >= 1" in p.stderr


def test_dump_outputs(tmp_path):
    """--dump-outputs on the default pass's shapes (25 requests x 391 image tokens, 100 region tokens, 151936 logits): every array a caller
    of the timed step receives, rows of all requests concatenated, float32 / float64 (exact token ids), <= 64 MB in all; the small arrays'
    unused shares go to the larger ones, so only image_tokens is sampled, with the same seeded rows in every run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    outs = [dict(image_tokens=torch.randn(391, 2048, generator=g).bfloat16(), region_tokens=torch.randn(100, 2048, generator=g).bfloat16(),
                 last_hidden=torch.randn(1, 2048, generator=g).bfloat16(), logits=torch.randn(1, 151936, generator=g),
                 next_token=torch.tensor([151000 + i]), embeds=None) for i in range(25)]
    shapes = bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    assert shapes["region_tokens"] == [2500, 2048] and shapes["last_hidden"] == [25, 2048] and shapes["logits"] == [25, 151936]
    assert 1000 < shapes["image_tokens"][0] < 9775 and shapes["image_tokens"][1] == 2048
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == sorted([n + ".npy" for n in bench.DUMP_NAMES] + ["image_tokens_rows.npy"])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 10 ** 6
    for f in (tmp_path / "a").iterdir():
        a, b = np.load(f), np.load(tmp_path / "b" / f.name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f.name
    rows = np.load(tmp_path / "a" / "image_tokens_rows.npy").astype(np.int64)
    full = torch.cat([o["image_tokens"] for o in outs]).float().numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "image_tokens.npy"), full[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "logits.npy"), torch.cat([o["logits"] for o in outs]).numpy())
    assert np.load(tmp_path / "a" / "next_token.npy").tolist() == [151000.0 + i for i in range(25)]
