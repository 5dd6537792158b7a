#!/usr/bin/env python3
"""`fleet_share_kernel` alone: B robots in worlds of R, random predictions, `reps` launches -- the workload for
`rocprofv3 --kernel-trace --stats -- python tools/probes/fleet_share_probe.py 8192 4` (kernel time next to the bytes a launch moves).

usage: fleet_share_probe.py [B] [R] [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    import torch
    from trajtrack_mpcndqn_rlboost_amd import MpcConfig
    from trajtrack_mpcndqn_rlboost_amd.device_tracker import DeviceTracker
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    cfg = MpcConfig()
    trk = DeviceTracker(cfg, B)
    trk.set_groups([list(range(i, min(i + R, B))) for i in range(0, B, R)])
    trk.pred_states.normal_()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    trk.share_predictions()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        trk.share_predictions()
    ev[1].record()
    torch.cuda.synchronize()
    per = 8 * 3 * int(cfg.N_hor)
    print(json.dumps({"tool": "fleet_share_probe", "batch": B, "robots_per_world": R, "launches": reps,
                      "us_per_launch_back_to_back": 1e3 * ev[0].elapsed_time(ev[1]) / reps,
                      "bytes_written_per_launch": B * per * int(cfg.Nother),
                      "bytes_read_per_launch": B * per * min(R - 1, int(cfg.Nother)) + 16 * B,
                      "nonzero_slots_per_robot": float((trk.other.view(B, int(cfg.Nother), -1) != 0).any(dim=2).sum(dim=1).double().mean())}))
