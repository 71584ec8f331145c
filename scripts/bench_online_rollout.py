"""Cost of the on-policy tick of phase 2 -- N observations in, N controls out, the tick scored and recorded -- on the device and by hand.

    python scripts/bench_online_rollout.py [--dtype bf16] [--ticks 100] [--blocks 5] [--warmup 1] [--agents 1,4,16] [--out FILE]

Workload: ResNet-34 camera student and ResNet-18 bird-view teacher (the oracle's synthetic weights, soft-argmax rows moved below the
horizon), random uint8 camera frames and 320 x 320 maps, random speeds and commands.  A block is --ticks ticks followed by the hand-over of
the block's frames to a copying DeviceReplayBuffer.
  arm "two_sessions_N":  what the package offered before TeachingSession: two DrivingSessions per tick (student, teacher), both waypoint
                         sets read back, the reference's _get_weight in numpy (train_image_phase2.py:74-81 on the unprojected student
                         waypoints), get_control with numpy's generator, the frames and the cropped maps appended to host lists, and one
                         add_batch of the lists at the end of the block;
  arm "teaching_session_N": TeachingSession.run_step (one captured graph, one block back) and commit at the end of the block.
All arms run INTERLEAVED in blocks, so that clock and thermal drift meets every arm; a block is timed on the host between two device
synchronisations, because the tick IS a host round trip.  Reported per arm: mean / median / min / max of the per-tick time over the
blocks (the hand-over included); the margin to quote for a difference is the block-to-block spread.  Then lbc_rollout_decide and
lbc_rollout_stage_u8 alone: 200 back-to-back launches at every N between two HIP events, with the bytes the copy moves.
Prints one JSON line and writes it to --out (default profiles/online_rollout.json)."""
import argparse
import json
import math
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

RGB_BYTES, BV_BYTES = 160 * 384 * 3, 192 * 192 * 7


def build_models(dtype, seed=3):
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS, ImagePolicyModelSS
    from oracle import lbc_oracle as O
    out = []
    for kind, backbone, cls in (("image", "resnet34", ImagePolicyModelSS), ("birdview", "resnet18", BirdViewPolicyModelSS)):
        sd = O.make_state_dict(kind, backbone, seed)
        for name in sd:
            if name.endswith("pos_y"):
                sd[name] = sd[name] * 0.35 + 0.55
        net = cls(backbone)
        net.load_state_dict(sd)
        net.precision = {"bf16": "bf16", "f32": "fp32", "fp32": "fp32"}[dtype]
        out.append(net)
    return out


def get_weight_numpy(student_wp, teacher_wp):
    """_get_weight(birdview_points, image_points) of the reference's rollout (:74-81, :116-119) on normalised camera-space student waypoints
    (N,5,2) and normalised map-space teacher waypoints: the CoordConverter's unprojection, then mean((|a - b| * xy_bias).sum(-1) * decay)"""
    w, h, fov, world_y, fixed_offset, ppm, crop = 384.0, 160.0, 90.0, 1.4, 4.0, 5.0, 192.0
    f = w / (2.0 * math.tan(fov * math.pi / 360.0))
    cx, cy = (student_wp[..., 0] + 1) * w / 2, (student_wp[..., 1] + 1) * h / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        wz = world_y / ((cy - h / 2) / f)
        wx = wz * ((cx - w / 2) / f)
        mx, my = wx * ppm + crop / 2, crop - wz * ppm + fixed_offset * ppm
        image_points = np.stack([mx, my], -1) / (0.5 * crop) - 1
        decay, xy_bias = np.array([0.7 ** i for i in range(5)]), np.array([0.7, 0.3])
        return np.mean((np.abs(teacher_wp - image_points) * xy_bias).sum(axis=-1) * decay, axis=-1)


def launches_alone(device, n, calls=200):
    """decide and stage back to back, each `calls` times between two events (the cursors are zeroed by a memset between the timed runs)"""
    from learningbycheating_amd import _lib
    lib = _lib.get()
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=device)
    ctl, onehot, weight, speed = z(n, 8, dt=torch.float64), z(n, 4), z(n), z(n)
    onehot[:, 1] = 1
    p, tick, cursor, dropped, slot = torch.full((1,), 0.7, dtype=torch.float64, device=device), z(1, dt=torch.int64), z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.int32)
    meta = [z(n * calls, dt=torch.int32), z(n * calls), z(n * calls)]
    out = z(n, 16, dt=torch.float64)
    rgb, bv = torch.randint(0, 256, (n, RGB_BYTES), dtype=torch.uint8, device=device), torch.randint(0, 256, (n, BV_BYTES), dtype=torch.uint8, device=device)
    rows = 4                                                             # staging rows per agent: the copy cycles through them
    rs, bs = z(n * rows, RGB_BYTES, dt=torch.uint8), z(n * rows, BV_BYTES, dt=torch.uint8)
    slots = [(torch.arange(n, dtype=torch.int32) * rows + k).to(device) for k in range(rows)]
    s = _lib.stream_for(out)

    def decide():
        _lib.check(lib.lbc_rollout_decide(_lib.ptr(ctl), _lib.ptr(ctl), _lib.ptr(weight), _lib.ptr(speed), _lib.ptr(onehot), None, n, calls, 1, _lib.ptr(p),
                                          _lib.ptr(tick), _lib.ptr(cursor), _lib.ptr(dropped), _lib.ptr(slot), _lib.ptr(meta[0]), _lib.ptr(meta[1]),
                                          _lib.ptr(meta[2]), _lib.ptr(out), s), "rollout_decide")

    def stage(k):
        _lib.check(lib.lbc_rollout_stage_u8(_lib.ptr(rgb), RGB_BYTES, _lib.ptr(bv), BV_BYTES, _lib.ptr(slots[k % rows]), n, n * rows, _lib.ptr(rs), _lib.ptr(bs), s),
                   "rollout_stage_u8")
    res = {}
    for name, fn in (("decide", lambda k: decide()), ("stage", stage)):
        for k in range(10):
            fn(k)
        if name == "decide":
            cursor.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(calls):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        res[name] = {"us_per_call": round(e0.elapsed_time(e1) * 1000.0 / calls, 2), "calls": calls, "what": "back-to-back launches, host enqueue included"}
    moved = 2.0 * n * (RGB_BYTES + BV_BYTES)
    res["stage"].update(bytes_read_plus_written=int(moved), gb_per_s=round(moved / (res["stage"]["us_per_call"] * 1e-6) / 1e9, 1),
                        note="the same N source rows are read on every call and four staging rows per agent are written in turn: the traffic is "
                             "served by the caches, this is not an HBM rate; at small N the figure is the launch, not the copy")
    assert int(cursor.cpu()[0]) == calls and torch.equal(rs[slots[0].long()], rgb)
    return res


def stage_from_hbm(device, n=256, sets=4, calls=100):
    """lbc_rollout_stage_u8 where the copy, not the launch, is the time: N = 256 agents (113 MB read, 113 MB written per call), `sets`
    source sets and as many staging rows per agent used in turn, so that a call's 227 MB were last touched 3 calls (680 MB) ago"""
    from learningbycheating_amd import _lib
    lib = _lib.get()
    rgb = torch.randint(0, 256, (sets, n, RGB_BYTES), dtype=torch.uint8, device=device)
    bv = torch.randint(0, 256, (sets, n, BV_BYTES), dtype=torch.uint8, device=device)
    rs = torch.zeros((n * sets, RGB_BYTES), dtype=torch.uint8, device=device)
    bs = torch.zeros((n * sets, BV_BYTES), dtype=torch.uint8, device=device)
    slots = [(torch.arange(n, dtype=torch.int32) * sets + k).to(device) for k in range(sets)]
    s = _lib.stream_for(rs)

    def stage(k):
        k %= sets
        _lib.check(lib.lbc_rollout_stage_u8(_lib.ptr(rgb[k]), RGB_BYTES, _lib.ptr(bv[k]), BV_BYTES, _lib.ptr(slots[k]), n, n * sets, _lib.ptr(rs), _lib.ptr(bs), s),
                   "rollout_stage_u8")
    for k in range(2 * sets):
        stage(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(calls):
        stage(k)
    e1.record()
    torch.cuda.synchronize()
    assert torch.equal(rs[slots[1].long()], rgb[1]) and torch.equal(bs[slots[sets - 1].long()], bv[sets - 1])
    us = e0.elapsed_time(e1) * 1000.0 / calls
    moved = 2.0 * n * (RGB_BYTES + BV_BYTES)
    return {"N": n, "us_per_call": round(us, 2), "calls": calls, "bytes_read_plus_written": int(moved), "gb_per_s": round(moved / (us * 1e-6) / 1e9, 1),
            "what": "back-to-back launches over %d source sets and staging rows in turn (a footprint of %d MB): read + written bytes over time"
                    % (sets, int(sets * moved / 1e6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--agents", default="1,4,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_rollout.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_online_rollout.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    from learningbycheating_amd.agent import DrivingSession
    from learningbycheating_amd.teaching import TeachingSession, p_student
    from learningbycheating_amd.training.replay import DeviceReplayBuffer
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    agents = [int(x) for x in args.agents.split(",")]
    nmax, ticks = max(agents), args.ticks
    rng = np.random.RandomState(1)
    frames = rng.randint(0, 256, size=(4, nmax, 160, 384, 3)).astype(np.uint8)
    maps = ((rng.rand(4, nmax, 320, 320, 7) < 0.1) * 255).astype(np.uint8)
    speeds = rng.uniform(0.0, 8.0, size=(ticks, nmax)).astype(np.float32)
    commands = rng.randint(1, 5, size=(ticks, nmax))
    prob = p_student(3)
    arms, keep = {}, []
    for n in agents:
        # (every arm owns its models: engines are cached per module)
        (s1, t1), (s2, t2) = build_models(args.dtype), build_models(args.dtype)
        ds, dt = DrivingSession(s1, device, n_agents=n), DrivingSession(t1, device, n_agents=n)
        ts = TeachingSession(s2, t2, device, n, ticks, seed=1)
        ts.set_episode(3)
        buf_a, buf_b = DeviceReplayBuffer(device, buffer_limit=n * ticks, seed=0), DeviceReplayBuffer(device, buffer_limit=n * ticks, seed=0)
        keep.append((ds, dt, ts, buf_a, buf_b))
        draw = np.random.RandomState(2)

        def by_hand(n=n, ds=ds, dt=dt, buf=buf_a, draw=draw):
            data = {k: [] for k in ("rgb", "birdview", "cmd", "speed", "weight")}
            control = None
            for t in range(ticks):
                rgb, bv = frames[t & 3, :n], maps[t & 3, :n]
                cs = ds.run_step(rgb, speeds[t, :n], commands[t, :n])
                ct = dt.run_step(bv, speeds[t, :n], commands[t, :n])
                weight = get_weight_numpy(ds.debug["waypoints"].astype(np.float64), dt.debug["waypoints"].astype(np.float64))
                control = np.where((draw.uniform(0, 1, size=n) < prob)[:, None], cs, ct)
                data["rgb"].append(rgb.copy())
                data["birdview"].append(bv[:, 58:250, 64:256].copy())
                data["cmd"].append(commands[t, :n])
                data["speed"].append(speeds[t, :n])
                data["weight"].append(weight)
            buf.n = 0                                                     # (a fresh buffer per block: every block appends)
            cat = lambda k: np.concatenate(data[k])
            w = np.nan_to_num(cat("weight"), nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)
            buf.add_batch(torch.from_numpy(cat("rgb")), torch.from_numpy(np.ascontiguousarray(cat("birdview"))), torch.from_numpy(cat("cmd")),
                          torch.from_numpy(cat("speed")), torch.from_numpy(w))
            return control

        def on_device(n=n, ts=ts, buf=buf_b):
            control = None
            for t in range(ticks):
                control = ts.run_step(frames[t & 3, :n], maps[t & 3, :n], speeds[t, :n], commands[t, :n])
            buf.n = 0
            ts.commit(buf)
            return control
        arms["two_sessions_%d" % n] = by_hand
        arms["teaching_session_%d" % n] = on_device
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
            blocks[name].append((time.perf_counter() - t0) * 1e3 / ticks)
    res = {}
    for name, bl in blocks.items():
        res[name] = {"ms_per_tick_mean": round(statistics.mean(bl), 4), "ms_per_tick_median": round(statistics.median(bl), 4),
                     "ms_per_tick_min": round(min(bl), 4), "ms_per_tick_max": round(max(bl), 4),
                     "spread_percent_of_median": round(100.0 * (max(bl) - min(bl)) / statistics.median(bl), 2),
                     "blocks_ms_per_tick": [round(x, 4) for x in bl]}
    for n in agents:
        res["teaching_%d_over_two_sessions_%d_median" % (n, n)] = round(
            res["teaching_session_%d" % n]["ms_per_tick_median"] / res["two_sessions_%d" % n]["ms_per_tick_median"], 4)
    res["launches_alone"] = {"N_%d" % n: launches_alone(device, n) for n in agents}
    del keep, arms
    torch.cuda.empty_cache()
    res["stage_from_hbm"] = stage_from_hbm(device)
    line = json.dumps({"workload": "phase-2 tick, ImagePolicyModelSS(resnet34) student + BirdViewPolicyModelSS(resnet18) teacher: two DrivingSessions + numpy "
                                   "weight + host lists + add_batch vs TeachingSession + commit, interleaved in blocks; the per-tick time includes the "
                                   "block's hand-over to the replay buffer", "dtype": args.dtype, "ticks_per_block": ticks, "blocks": args.blocks,
                       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
