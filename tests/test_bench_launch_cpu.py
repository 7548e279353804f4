"""CPU: `python bench.py --gpus N` launches its own ranks.  The parent never touches the GPU;
the ranks rendezvous on 127.0.0.1 and each owns a contiguous block of the ensemble (members are what
separate `ens_id` processes are in the reference, src/greb.f90:153,1064-1068)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _json_line(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text
    return json.loads(lines[0])


def test_dry_launch_two_ranks_partition():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--members", "6", "--dry-launch"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["dry_launch"] is True
    parts = out["partition"]
    assert [p["rank"] for p in parts] == [0, 1] and [p["local_rank"] for p in parts] == [0, 1]
    assert [(p["first"], p["count"]) for p in parts] == [(0, 6), (6, 6)]  # weak scaling: M members per GPU
    assert parts[0]["co2_first"] == 280.0 and 280.0 < parts[1]["co2_first"] < 1120.0
    # the toy record went through the timed run's gather path: both ranks seen, every member in its own slot
    assert out["ranks_seen"] == 2 and out["backend"] == "gloo"
    assert out["gather_verified"] is True and out["inversions"] == 0 and out["members_checked"] == 12
    # every rank's own timings reach the line (a straggling rank 0 must show the first time)
    pr = out["per_rank_s"]
    assert set(pr) == {"total", "gather_wait", "integrate"}
    for k, v in pr.items():
        assert len(v["per_rank"]) == 2 and v["min"] <= v["max"] and v["rank_of_max"] in (0, 1), (k, v)
        assert v["max"] == max(v["per_rank"]) and v["per_rank"][v["rank_of_max"]] == v["max"]
    assert out["root_members"] == 6 and out["members_total"] == 12


def test_dry_launch_root_rank_with_a_smaller_share():
    """--root-members: rank 0 (which also hosts the receive side of every gather) integrates fewer members; the blocks
    stay contiguous in rank order and the gathered members -- rank 0's padded slots dropped -- are in global order."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--members", "6", "--root-members", "2", "--dry-launch"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert [(p["first"], p["count"]) for p in out["partition"]] == [(0, 2), (2, 6), (8, 6)]
    assert out["members_total"] == 14 and out["root_members"] == 2
    assert out["gather_verified"] is True and out["members_checked"] == 14 and out["inversions"] == 0
    assert len(out["per_rank_s"]["total"]["per_rank"]) == 3


def test_gather_order_check_finds_a_misplaced_block():
    import numpy as np
    sys.path.insert(0, ROOT)
    from greb_climate_model_amd import ensemble
    v = ensemble.co2_sweep(16).astype(np.float64)
    assert ensemble.gather_order_check(v)["gather_verified"] is True
    swapped = np.concatenate([v[8:], v[:8]])  # the two ranks' blocks in each other's slots
    bad = ensemble.gather_order_check(swapped)
    assert bad["gather_verified"] is False and bad["inversions"] == 1
    assert ensemble.gather_order_check(swapped, block=8)["block_inversions"] == 1
    # a very fine sweep with rounding noise between neighbours is still in order at the stride the check uses
    fine = np.linspace(280.0, 1120.0, 4096) + 0.15 * np.sin(np.arange(4096) * 1.7)
    ok = ensemble.gather_order_check(fine, block=512)
    assert ok["gather_verified"] is True and ok["inversions"] > 0 and ok["stride"] == 8 and ok["inversions_at_stride"] == 0
    v[3] = np.nan
    assert ensemble.gather_order_check(v)["gather_verified"] is False


def test_gpus_flag_must_match_world_size():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--dry-launch"], env=_env(WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_failing_rank_fails_the_launch():
    # no visible GPU: every rank fails at its first GPU call; the parent must report failure, not a JSON line
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--members", "1"],
                       env=_env(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_plain_run_options():
    """A plain run measures the headline only (--full is off by default); --steps must be a real count of timed steps."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a = m.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 2)
    a = m.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, BENCH, *bad], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--steps" in r.stderr, bad
    assert m.DUMP_MEMBERS * 12 * 5 * 96 * 48 * 4 <= 64 * 2 ** 20  # the monthly sample of a dump stays within 64 MB
