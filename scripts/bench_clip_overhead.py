"""Cost of gradient clipping by global norm (NativeTrainer(max_grad_norm=X)) over the non-finite step guard it extends, on bench.py's
phase-1 step, measured in one process.

    python scripts/bench_clip_overhead.py [--batches 256,32] [--dtype bf16] [--steps 60] [--block 10] [--warmup 10] [--out FILE]

Two trainers per batch size -- guarded (skip_nonfinite=True) and clipped (max_grad_norm set so that every step IS clipped: a quarter of
the norm measured at the end of the warm-up) -- over their own copies of the same models, bench.py's L1 warm start below the horizon, the
synthetic dataset resident in HBM.  The arms run INTERLEAVED in blocks of --block steps (guarded, clipped, guarded, ...), each block
between two HIP events, so that clock and thermal drift meets both.  Reported per arm: mean, median and the block times per step; the
comparison is clipped against guarded OF THIS PROCESS, and its margin is the guarded arm's own block-to-block spread (max - min and the
standard deviation of its blocks), also reported.  Then the gradient pass alone: both entry points on a gradient buffer with one infinity
in it (the update kernel returns at once) give scan / norm pass + bookkeeping + an empty grid, 50 back-to-back calls each, interleaved in
rounds.  Prints one JSON line; --out also writes it to a file."""
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

ARMS = ("guarded", "clipped")


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_batch(prec, batch, steps, block, warmup, init_steps, device, pool_frames):
    from learningbycheating_amd.training.native import NativeTrainer
    host_pool = bench.FramePool(pool_frames, batch, device, 1000, need_rgb=True, slots=True)
    pool = bench.DevicePool(host_pool)
    pool.batch = batch
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    state = {"i": 0}

    def run(tr, n, warm=False):
        for _ in range(n):
            k = state["i"] & 1
            state["i"] += 1
            b = pool.get(k)
            if warm:
                tr.step(b["rgb"], b["speed"], b["onehot"], target=tgt)
            else:
                tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"])
            pool.release(k)
            pool.prefetch(k)

    pool.pos = 0
    pool.prefetch(0); pool.prefetch(1)
    arms = {}
    for name in ARMS:
        student, teacher = bench.build_models(device, "phase1")
        student.precision = teacher.precision = prec
        warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
        run(warm, init_steps, warm=True)
        del warm
        tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4, skip_nonfinite=True,
                           max_grad_norm=0.0 if name == "clipped" else None)
        run(tr, warmup)
        arms[name] = {"tr": tr, "blocks": []}
    torch.cuda.synchronize()
    clipped = arms["clipped"]["tr"]
    warm_stats = clipped.grad_stats()
    clipped.opt.max_grad_norm = warm_stats["grad_norm"] / 4.0        # from here on every step is clipped (checked below)
    applied0 = clipped.opt.step_count
    for _ in range((steps + block - 1) // block):
        for name in ARMS:
            arms[name]["blocks"].append(_timed(lambda: run(arms[name]["tr"], block)) / block)
    out = {}
    for name, a in arms.items():
        out[name] = {"ms_per_step_mean": round(statistics.mean(a["blocks"]), 4), "ms_per_step_median": round(statistics.median(a["blocks"]), 4),
                     "blocks_ms_per_step": [round(x, 4) for x in a["blocks"]], "timed_steps": block * len(a["blocks"]),
                     "skipped": list(a["tr"].skipped()), "adam_step": a["tr"].opt.step_count}
    gb = arms["guarded"]["blocks"]
    out["guarded"]["block_spread_ms"] = {"max_minus_min": round(max(gb) - min(gb), 4), "stdev": round(statistics.pstdev(gb), 4)}
    st = clipped.grad_stats()
    out["clipped"].update(max_grad_norm=clipped.opt.max_grad_norm, grad_norm_after_warmup=warm_stats["grad_norm"], grad_norm_last=st["grad_norm"],
                          clip_coef_last=st["clip_coef"], clipped_steps=st["clipped_total"], applied_steps_timed=clipped.opt.step_count - applied0)
    out["clipped_minus_guarded_ms_mean"] = round(out["clipped"]["ms_per_step_mean"] - out["guarded"]["ms_per_step_mean"], 4)
    out["clipped_minus_guarded_ms_median"] = round(out["clipped"]["ms_per_step_median"] - out["guarded"]["ms_per_step_median"], 4)
    out["clipped_over_guarded_percent_of_median"] = round(100.0 * (out["clipped"]["ms_per_step_median"] / out["guarded"]["ms_per_step_median"] - 1.0), 3)
    out["inside_guarded_block_spread"] = bool(abs(out["clipped_minus_guarded_ms_median"]) <= out["guarded"]["block_spread_ms"]["max_minus_min"])
    # the gradient pass alone: a skipped call = scan / norm pass + bookkeeping + an update grid that returns at once
    elems = sum(n for _, n in clipped.opt.offsets.values())
    calls = {n: [] for n in ARMS}
    for name in ARMS:
        arms[name]["tr"].eng.grad_flat[0] = float("inf")
        for _ in range(5):
            arms[name]["tr"].opt.step()
    torch.cuda.synchronize()
    for _ in range(5):
        for name in ARMS:
            opt = arms[name]["tr"].opt
            calls[name].append(_timed(lambda: [opt.step() for _ in range(50)]) * 1000.0 / 50)
    out["skipped_call"] = {"what": "scan (guarded) / norm pass (clipped) + bookkeeping + early-returning update grid, 5 interleaved rounds of 50 "
                                   "back-to-back calls", "gradient_bytes": 4 * elems}
    for name in ARMS:
        us = statistics.median(calls[name])
        out["skipped_call"][name] = {"us_median": round(us, 2), "us_rounds": [round(x, 2) for x in calls[name]],
                                     "GBps_lower_bound": round(4 * elems / (us * 1e-6) / 1e9, 1)}
        assert arms[name]["tr"].skipped()[1] == 5 + 5 * 50
    del arms, clipped
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--pool-frames", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_overhead.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {}
    for b in [int(x) for x in args.batches.split(",")]:
        res["batch_%d" % b] = run_batch(args.dtype, b, args.steps, args.block, args.warmup, args.init_steps, device, args.pool_frames)
        print("# batch %d: %s" % (b, json.dumps(res["batch_%d" % b])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "phase1 (bench.py phase1_bs256 step), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18), guarded vs "
                                   "clipped (every step clipped), interleaved",
                       "dtype": args.dtype, "steps": args.steps, "block": args.block, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
