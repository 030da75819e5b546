#!/usr/bin/env python
"""Node beliefs on strips that are PROCESSES (stereo_amd.strips.TrwsStripRank.own_min_marginals): one strip per rank,
hand-over through HIP IPC as in tools/strips_ipc_check.py, every rank keeps the beliefs of its own nodes and exchanges
nothing for them.

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29547 tools/strips_beliefs_ipc_check.py [H W K]
Every rank compares its own rows, bit for bit, with a single plan it solves itself -- after two iterations, then with
the flag turned off and on again in mid-run and three more -- and rank 0 prints IPC_BELIEFS_OK if all ranks agree."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    H, W, K = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (40, 46, 16)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    ndev = torch.cuda.device_count()
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(ndev, 1)
    backend = "nccl" if ndev >= world else "gloo"   # RCCL refuses two ranks on one GPU
    torch.cuda.set_device(local)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group("gloo")
    from stereo_amd import _lib
    from stereo_amd.strips import TrwsStripRank
    from stereo_amd.trws import TrwsPlan
    from helpers import trws_problem
    _lib.lib().stereo_hip_set_device(local)
    dev = torch.device("cuda", local) if backend == "nccl" else torch.device("cpu")
    p = trws_problem(7, H, W, K, kind="general")
    s = TrwsStripRank(1, K, H, W, p["conn"].T, rank, world, dist, dev,
                      max_workgroups=max(2, (int(_lib.lib().stereo_hip_device_cus()) or 256) // world) if ndev < world else 0)
    s.keep_min_marginals()
    s.upload(p["unary"].T, p["alphas"], 3.0, q=p["q"].T, qprim=p["qprim"].T)
    one = TrwsPlan(1, K, H * W, p["conn"].T)
    one.upload(p["unary"].T, p["alphas"], 3.0, q=p["q"].T, qprim=p["qprim"].T)
    one.keep_min_marginals()
    ok = True
    for step, iters in enumerate((2, 3)):
        if step == 1:   # off and on again between iterations: the beliefs are back with the next one
            s.keep_min_marginals(False)
            s.keep_min_marginals(True)
        done, _ = s.iterate(iters, max_relgap=-1e300)
        assert done == iters
        one.iterate(iters, max_relgap=-1e300)
        idx, mm, conf, am = s.own_min_marginals()
        mm1, conf1, am1 = one.min_marginals()
        good = (bool(np.array_equal(idx, np.nonzero(s.owner == rank)[0])) and bool(np.array_equal(mm, mm1[:, idx])) and
                bool(np.array_equal(conf, conf1[idx])) and bool(np.array_equal(am, am1[idx])))
        print("rank %d of %d backend %s device %d iterations %d own nodes %d beliefs_equal %s" %
              (rank, world, backend, local, s.iterations, len(idx), good), flush=True)
        ok = ok and good
    one.close()
    verdicts = [None] * world
    dist.all_gather_object(verdicts, ok)
    if rank == 0:
        print("IPC_BELIEFS_OK" if all(verdicts) else "IPC_BELIEFS_MISMATCH")
    dist.barrier()
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if all(verdicts) else 1)


if __name__ == "__main__":
    main()
