"""Guarded optimizer step with world_size 2: two rank processes (forked from the fork server that was started before the GPU
was initialised) share the box's one MI355X and exchange the flat gradient through gloo, as tests/test_hip_ddp.py runs them.
The guard's decision is taken on the all-reduced gradient, so a NaN in ONE rank's shard makes EVERY rank skip that step."""
import multiprocessing as mp
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_every_rank_skips_the_step_one_rank_poisoned(tmp_path):
    import grad_guard_worker as W
    world, nsteps = 2, 3
    ctx = mp.get_context("forkserver")
    port = _free_port()
    procs = [ctx.Process(target=W.run, args=(r, world, port, nsteps, 1, 1, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(30)                                  # reaped before the next test opens the GPU
    assert not hung, f"ranks {hung} did not finish within 300 s"
    for p in procs:
        assert p.exitcode == 0, p.exitcode
    r0 = np.load(tmp_path / "rank0.npz")
    r1 = np.load(tmp_path / "rank1.npz")
    for r in (r0, r1):
        assert int(r["skipped"]) == 1 and int(r["step_count"]) == 2 and int(r["consecutive"]) == 0
    for k in ("param", "m", "v"):
        assert np.isfinite(r0[k]).all(), k
        assert np.array_equal(r0[k], r1[k]), k
