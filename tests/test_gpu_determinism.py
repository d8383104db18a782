"""Bit-reproducibility of the training step under load (round-2 verdict: two-rank runs with captured graphs once ended
5-6 ulp apart on a shared device and the multirank test's tolerance was loosened instead of root-caused).

Harness: tools/stress/step_probe.py (forward + criterion + backward of one fixed batch, every gradient word compared)
and tools/stress/trajectory_probe.py (two ranks, every trial = four full steps from one restored initial state:
loss bits and reduced-gradient checksums of every step compared), both optionally next to extra training processes on
the same device.  What they established: 5 configurations x 119 single-process iterations and
5 x 59 x 2 two-rank trajectories — graphs, prefetch stream, bucketed and single all-reduce, 0-2 competing processes —
without ONE differing bit, before and after the library's fused attention (AOTriton, atomics in its backward) was
replaced by this package's one-launch kernel.  The step is a deterministic function of its inputs; the tests below keep
it that way."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import free_port as _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _backend():
    import torch
    return "nccl" if torch.cuda.device_count() >= 2 else "gloo"


def _torchrun(script_args, port, env_extra=None, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + script_args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_single_process_step_is_bit_reproducible_under_load():
    """40 repetitions of forward + criterion + backward (captured decoder passes, prefetch stream) while a second
    training process hammers the same device: every gradient word equal to the first repetition's."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "stress", "step_probe.py"), "--iters", "40", "--graphs",
           "--prefetch", "--load", "1"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"RESULT .*: (\d+) of (\d+) iterations differ", out.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) == 39, out.stdout[-2000:]


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_two_rank_trajectories_are_bit_reproducible_under_load(overlap):
    """Two ranks (RCCL on a multi-GPU box, else gloo on the shared device), 16 trials of four full steps each from one
    restored state, next to a third training process: loss bits and the reduced gradients of every step identical."""
    out = _torchrun([os.path.join(ROOT, "tools", "stress", "trajectory_probe.py"), "--trials", "16", "--load", "1"],
                    _free_port(), {"USC3D_OVERLAP_ALLREDUCE": overlap})
    # the two ranks share one stdout pipe: a report may follow the other's without a newline, so no match may cross a ':'
    res = re.findall(r"RESULT rank (\d) [^:]*: (\d+) of (\d+) trials differ", out)
    assert sorted(r[0] for r in res) == ["0", "1"], out[-2000:]
    assert all(int(r[1]) == 0 and int(r[2]) == 15 for r in res), out[-2000:]


def test_two_rank_runs_are_bit_reproducible_across_processes():
    """The multirank test's own command, two separate launches per mode: the loss after four steps has the same
    bits every time and in both gradient-exchange modes."""
    losses = set()
    for k in range(2):
        for overlap in ("1", "0"):
            out = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--voxels",
                             "40000", "--dist-backend", _backend(), "--no-cpu-baseline", "--rotate", "0"], _free_port(),
                            {"USC3D_OVERLAP_ALLREDUCE": overlap})
            rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            losses.add(rec["config"]["loss"])
    assert len(losses) == 1, losses
