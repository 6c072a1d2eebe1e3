"""``sucre.pooled_uncertainty`` through RCCL: what --shared-water --save-uncertainty does under ``torchrun`` with one GPU per rank,
where ``dist.init_process_group`` picks 'nccl' and a host tensor cannot be reduced.  A one-rank 'nccl' group on the GPU box with
every collective forced through it (tests/uncertainty_rccl_worker.py).  Runs in a child process: a process group must not leak
into the test session."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.timeout(300)
def test_pooled_uncertainty_over_a_one_rank_rccl_group_equals_the_plain_sum():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR')}
    env.update(MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, str(ROOT / 'tests' / 'uncertainty_rccl_worker.py')], env=env, capture_output=True, text=True,
                         timeout=250)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert 'RCCL_POOL_OK backend=nccl world=1' in out.stdout, out.stdout[-1500:]
    print(out.stdout.strip().splitlines()[-1])
