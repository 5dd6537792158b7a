"""Child process of tests/test_gpu_dqn_fused.py::test_collective_path_equals_the_single_launch: in a one-rank process group on
cuda:0, ``FusedDqnTrainer(force_collective=True)`` -- gradient kernel into the bucket, RCCL all-reduce, apply kernel with scale
1 / world -- against the single-launch update of a second trainer, bit for bit.  A process of its own for the reason
rccl_one_rank_update.py gives.  Exit code 0 = equal; prints one line."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from support import dqn_cases  # noqa: E402
from trajtrack_mpcndqn_rlboost_amd import dqn_fused  # noqa: E402


def main():
    dev = "cuda:0"
    torch.cuda.set_device(0)
    with socket.socket() as sk:                                   # a free port for the one-rank rendezvous
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(dev))
    try:
        rng = np.random.default_rng(5)
        batches = [{k: torch.from_numpy(v).to(dev) for k, v in dqn_cases.random_batch(rng, 32, weights=i % 2 == 1).items()}
                   for i in range(6)]
        torch.manual_seed(0)
        single = dqn_fused.FusedDqnTrainer(device=dev, target_update_interval=4)
        torch.manual_seed(0)
        coll = dqn_fused.FusedDqnTrainer(device=dev, target_update_interval=4, force_collective=True)
        assert coll.collective and not single.collective and torch.equal(single.state, coll.state)
        for b in batches:
            la, lb = single.update(b), coll.update(b)
            assert torch.equal(la, lb) and torch.equal(single.last_td_error, coll.last_td_error)
            assert torch.equal(single.state, coll.state) and torch.equal(single._bucket, coll._bucket)
        assert single.step_count == coll.step_count == 6 and single.num_target_syncs == coll.num_target_syncs == 1
        print(f"fused gradient -> RCCL all-reduce -> apply == fused step over 6 updates, bit for bit (backend {dist.get_backend()}, "
              f"world {dist.get_world_size()})")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
