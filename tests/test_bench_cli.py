"""bench.py's launcher contract (no GPU needed): `--gpus N` without a launcher starts N ranks itself under
torch.distributed.run with the rendezvous on 127.0.0.1; a mismatch between --gpus and WORLD_SIZE is refused
(`--gpus` used to be parsed and ignored)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_respawns_n_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2"])
    with pytest.raises(SystemExit) as e:
        bench._respawn_under_torchrun(4)
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "2"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_gpus_flag_is_checked_against_visible_devices_and_world_size():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr          # this container has no GPU
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_steps_and_leg_flags_are_validated_before_any_work():
    """--steps 0 would divide by zero; --config4-leg only selects a leg of --full (a plain run is the headline alone)."""
    for argv, msg in ((["--steps", "0"], "--steps must be >= 1"), (["--warmup", "-1"], "--warmup >= 0"),
                      (["--config4-leg"], "pass --full too")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (argv, r.stderr[-500:])
