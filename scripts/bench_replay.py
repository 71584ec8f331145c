"""Phase-2 step with the host replay buffer against the device-resident one (train_image_phase2.py --replay host | device), measured
in one process.

    python scripts/bench_replay.py [--batch 128] [--dtypes fp32,bf16] [--frames 2048] [--steps 40] [--block 5] [--warmup 5] [--out FILE]

Per precision: one student / teacher / NativeTrainer (bench.py's models and L1 warm start below the horizon) and two buffers over the
same synthetic frames, both with normalised weights (the steady state: weighted draws).  An arm's step is the loop body of its
training function: `_train`'s (np.random.choice on the host, float batches from torch ops, the weights copied back to the host every
step) or `_device_step` (lbc_replay_sample / gather_u8 / meta / writeback, no host round trip).  The arms run INTERLEAVED in blocks of
--block steps (host, device, host, ...), each block between two HIP events and a synchronize, so that clock and thermal drift meets
both.  Reported per arm: mean, median and the block-to-block spread (population standard deviation) of the block times per step.
"not slower" = the device arm's mean is below the host arm's mean + the host arm's spread.
Then the gather alone: lbc_replay_gather_u8 of --batch rgb + bird-view rows into preallocated outputs, 80 back-to-back pairs of calls
rotating over 8 index sets and 8 output pairs (a working set beyond the Infinity Cache), bytes read + written over the time.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))


def run_precision(prec, batch, frames, steps, block, warmup, init_steps, device):
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    from learningbycheating_amd.training import train_image_phase2 as P2
    from learningbycheating_amd.training.native import NativeTrainer
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = prec
    host, devb = P2.synthetic_buffer(frames, device, seed=0), P2.synthetic_buffer_device(frames, device, seed=0)
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    for _ in range(init_steps):
        rgb, _, command, speed = devb.batch(devb.sample_indices(batch))
        warm.step(rgb, speed, command, target=tgt)
    del warm
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4)
    config = {"batch_size": batch, "speed_noise": 0.0, "batch_aug": 1}

    def host_step():
        idx = host.sample_indices(batch)
        rgb, bv, cmd, speed = host.batch(idx)
        tr.step(rgb, speed, one_hot(cmd).to(device), birdview=bv)
        host.update_weights(idx, P2.phase2_weights(tr, tr.last_pred[0], tr.last_teacher[0]))

    def device_step():
        P2._device_step(devb, tr, config)

    # one shuffled epoch's worth of write-backs is not needed to reach the steady state: give both buffers the same non-uniform weights
    w = (torch.rand(frames, generator=g) + 0.05)
    host.init_new_weights(); host._new_weights[:] = w.double().numpy(); host.normalize_weights(); host.init_new_weights()
    devb.init_new_weights(); devb.new_weights[:frames].copy_(w); devb.normalize_weights(); devb.init_new_weights()
    arms = {"host": {"fn": host_step, "blocks": []}, "device": {"fn": device_step, "blocks": []}}
    for a in arms.values():
        for _ in range(warmup):
            a["fn"]()
    torch.cuda.synchronize()
    for _ in range((steps + block - 1) // block):
        for name in ("host", "device"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                arms[name]["fn"]()
            e1.record()
            torch.cuda.synchronize()
            arms[name]["blocks"].append(e0.elapsed_time(e1) / block)
    out = {}
    for name, a in arms.items():
        out[name] = {"ms_per_step_mean": round(statistics.mean(a["blocks"]), 4), "ms_per_step_median": round(statistics.median(a["blocks"]), 4),
                     "ms_per_step_spread": round(statistics.pstdev(a["blocks"]), 4), "blocks_ms_per_step": [round(x, 4) for x in a["blocks"]],
                     "timed_steps": block * len(a["blocks"])}
    out["device_over_host_mean"] = round(out["device"]["ms_per_step_mean"] / out["host"]["ms_per_step_mean"], 4)
    out["device_not_slower"] = bool(out["device"]["ms_per_step_mean"] < out["host"]["ms_per_step_mean"] + out["host"]["ms_per_step_spread"])
    # the gather alone, over a working set far beyond the 256 MB Infinity Cache: 8 index sets and 8 output pairs in rotation (453 MB
    # written per round, rows drawn from all `frames` x 442 KB of the buffer), so that reads and writes meet HBM
    sets = 8
    lib = _lib.get()
    rb, bb = int(devb.rgb[0].numel()), int(devb.birdview[0].numel())
    idxs = [devb.sample_indices(batch) for _ in range(sets)]
    outs = [(torch.empty_like(devb.rgb[:batch]), torch.empty_like(devb.birdview[:batch])) for _ in range(sets)]

    def gather(k):
        rgb, bv = outs[k % sets]
        s = _lib.stream_for(rgb)
        _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(devb.rgb), rb, _lib.ptr(idxs[k % sets]), batch, 1, _lib.ptr(rgb), s), "gather")
        _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(devb.birdview), bb, _lib.ptr(idxs[k % sets]), batch, 1, _lib.ptr(bv), s), "gather")
    for k in range(2 * sets):
        gather(k)
    torch.cuda.synchronize()
    reps = 10 * sets
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        gather(k)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000.0 / reps
    moved = 2 * batch * (rb + bb)
    out["gather"] = {"us_per_batch": round(us, 2), "bytes_read_plus_written": moved, "GBps": round(moved / (us * 1e-6) / 1e9, 1),
                     "working_set_MB": round(sets * moved / 2 / 1e6 + frames * (rb + bb) / 1e6),
                     "what": "two lbc_replay_gather_u8 launches (rgb + bird view) of %d rows out of %d, %d back-to-back pairs rotating over %d "
                             "index sets and output pairs" % (batch, frames, reps, sets)}
    del arms, tr, host, devb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {}
    for prec in args.dtypes.split(","):
        res[prec] = run_precision(prec, args.batch, args.frames, args.steps, args.block, args.warmup, args.init_steps, device)
        print("# %s: %s" % (prec, json.dumps(res[prec])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "phase-2 replay step (train_image_phase2.py), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18), host "
                                   "ReplayBuffer vs DeviceReplayBuffer, weighted sampling, interleaved blocks",
                       "batch": args.batch, "frames": args.frames, "steps": args.steps, "block": args.block, "warmup": args.warmup,
                       "init_steps": args.init_steps, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
