"""Cost of a whole agent tick -- frame in, steer / throttle / brake out -- with the controller on the host and on the device.

    python scripts/bench_agent_tick.py [--dtype bf16] [--ticks 200] [--blocks 6] [--warmup 1] [--agents 1,4,16] [--out FILE]

Workload: the ResNet-34 image model (the oracle's synthetic weights, soft-argmax rows moved below the horizon so that the controller
has waypoints to work on), random uint8 camera frames, random speeds and commands.
  arm "host_controller":  PolicySession.run_step (batch 1, captured graph, 40 bytes back) followed by the double-precision numpy /
                          Python restatement of the controller on the host (tests/test_agent_control.py Twin) -- what a user of the
                          package had to do so far;
  arm "driving_session_N": DrivingSession.run_step with N agents: one captured graph that ends in the controller, one block back.
All arms run INTERLEAVED in blocks of --ticks ticks each (host, N = 1, N = 4, ..., host, ...), so that clock and thermal drift
meets every arm; a block is timed on the host between two device synchronisations, because the tick IS a host round trip.  Reported
per arm: mean / median / min / max of the per-tick time over the blocks; the margin to quote for a difference is the block-to-block
spread.  Then the controller launch alone: 200 back-to-back lbc_agent_control calls at every N between two HIP events.
Prints one JSON line and writes it to --out (default profiles/agent_tick.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))


def build_model(dtype, seed=3):
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS
    from oracle import lbc_oracle as O
    sd = O.make_state_dict("image", "resnet34", seed)
    for name in sd:
        if name.endswith("pos_y"):
            sd[name] = sd[name] * 0.35 + 0.55
    net = ImagePolicyModelSS("resnet34")
    net.load_state_dict(sd)
    net.precision = {"bf16": "bf16", "f32": "fp32", "fp32": "fp32"}[dtype]
    return net


def controller_alone(device, n, calls=200):
    from learningbycheating_amd.agent import ControllerConfig, WaypointController
    from tests.test_agent_control import draw_episodes, one_hot
    pred, speed, command = draw_episodes("image", n, 1, seed=77)
    pred, speed, rows = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (pred[:, 0], speed[:, 0], one_hot(command)[:, 0]))
    c = WaypointController(ControllerConfig.image(), n, device)
    for _ in range(10):
        c.step(pred, speed, rows)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        c.step(pred, speed, rows)
    e1.record()
    torch.cuda.synchronize()
    assert not (c.out.cpu().numpy()[:, 7] != 0).any()
    return {"us_per_call": round(e0.elapsed_time(e1) * 1000.0 / calls, 2), "calls": calls, "what": "back-to-back launches, host enqueue included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--agents", default="1,4,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agent_tick.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_agent_tick.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    from learningbycheating_amd.agent import ControllerConfig, DrivingSession
    from learningbycheating_amd.inference import PolicySession
    from tests.test_agent_control import Twin, one_hot
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    agents = [int(x) for x in args.agents.split(",")]
    nmax = max(agents)
    rng = np.random.RandomState(1)
    frames = rng.randint(0, 256, size=(8, nmax, 160, 384, 3)).astype(np.uint8)
    speeds = rng.uniform(0.0, 8.0, size=(args.ticks, nmax)).astype(np.float32)
    commands = rng.randint(1, 5, size=(args.ticks, nmax))
    rows = one_hot(commands)
    cfg = ControllerConfig.image()
    host = PolicySession(build_model(args.dtype), device)          # (every session owns its model: engines are cached per module)
    twin = Twin(cfg)
    sessions = {n: DrivingSession(build_model(args.dtype), device, n_agents=n, config=cfg) for n in agents}

    def host_block():
        last = None
        for t in range(args.ticks):
            wp = host.run_step(frames[t & 7, 0], speeds[t, 0], commands[t, 0])
            last = twin.step(wp, speeds[t, 0], rows[t, 0])[:3]
        return last

    def session_block(n):
        s, last = sessions[n], None
        for t in range(args.ticks):
            last = s.run_step(frames[t & 7, :n], speeds[t, :n], commands[t, :n])
        return last

    arms = {"host_controller": host_block}
    arms.update({"driving_session_%d" % n: (lambda n=n: session_block(n)) for n in agents})
    blocks = {k: [] for k in arms}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    for _ in range(args.blocks):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) * 1e3 / args.ticks)
    res = {}
    for name, bl in blocks.items():
        res[name] = {"ms_per_tick_mean": round(statistics.mean(bl), 4), "ms_per_tick_median": round(statistics.median(bl), 4),
                     "ms_per_tick_min": round(min(bl), 4), "ms_per_tick_max": round(max(bl), 4),
                     "spread_percent_of_median": round(100.0 * (max(bl) - min(bl)) / statistics.median(bl), 2),
                     "blocks_ms_per_tick": [round(x, 4) for x in bl]}
    if 1 in agents:
        res["session_1_minus_host_percent_of_median"] = round(
            100.0 * (res["driving_session_1"]["ms_per_tick_median"] / res["host_controller"]["ms_per_tick_median"] - 1.0), 2)
    res["controller_alone"] = {"N_%d" % n: controller_alone(device, n) for n in agents}
    line = json.dumps({"workload": "agent tick, ImagePolicyModelSS(resnet34): PolicySession + host controller (batch 1) vs DrivingSession (N agents), "
                                   "interleaved in blocks", "dtype": args.dtype, "ticks_per_block": args.ticks, "blocks": args.blocks,
                       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
