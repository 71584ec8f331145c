"""Cost of the non-finite step guard (NativeTrainer(skip_nonfinite=True)) on bench.py's phase-1 step, measured in one process.

    python scripts/bench_guard_overhead.py [--batches 256,32] [--dtype bf16] [--steps 60] [--block 10] [--warmup 10] [--out FILE]

Two trainers per batch size -- guard off (the default path bench.py times) and guard on -- over their own copies of the same models,
bench.py's L1 warm start below the horizon, the synthetic dataset resident in HBM.  The arms run INTERLEAVED in blocks of --block steps
(off, on, off, on, ...), each block between two HIP events, so that clock and thermal drift meets both; reported per arm: mean and
median of the block times per step.  Then the scan alone: the guarded entry point on a gradient buffer with one infinity in it (the
update kernel returns at once) gives the time of scan + bookkeeping + an empty grid, and from it a lower bound on the scan's GB/s.
Prints one JSON line; --out also writes it to a file."""
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
    for name, guard in (("guard_off", False), ("guard_on", True)):
        student, teacher = bench.build_models(device, "phase1")
        student.precision = teacher.precision = prec
        warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
        run(warm, init_steps, warm=True)
        del warm
        tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4, skip_nonfinite=guard)
        run(tr, warmup)
        arms[name] = {"tr": tr, "blocks": []}
    torch.cuda.synchronize()
    for _ in range((steps + block - 1) // block):
        for name in ("guard_off", "guard_on"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(arms[name]["tr"], block)
            e1.record()
            torch.cuda.synchronize()
            arms[name]["blocks"].append(e0.elapsed_time(e1) / block)
    out = {}
    for name, a in arms.items():
        out[name] = {"ms_per_step_mean": round(statistics.mean(a["blocks"]), 4), "ms_per_step_median": round(statistics.median(a["blocks"]), 4),
                     "blocks_ms_per_step": [round(x, 4) for x in a["blocks"]], "timed_steps": block * len(a["blocks"])}
    on = arms["guard_on"]["tr"]
    out["guard_on"]["skipped"] = list(on.skipped())
    out["guard_on"]["adam_step"] = on.opt.step_count
    out["overhead_percent_of_mean"] = round(100.0 * (out["guard_on"]["ms_per_step_mean"] / out["guard_off"]["ms_per_step_mean"] - 1.0), 3)
    out["overhead_percent_of_median"] = round(100.0 * (out["guard_on"]["ms_per_step_median"] / out["guard_off"]["ms_per_step_median"] - 1.0), 3)
    # the scan alone: a skipped call = scan + bookkeeping thread + a grid that returns at once
    elems = sum(n for _, n in on.opt.offsets.values())
    on.eng.grad_flat[0] = float("inf")
    for _ in range(5):
        on.opt.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        on.opt.step()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000.0 / 50
    out["skipped_call"] = {"us": round(us, 2), "gradient_bytes": 4 * elems, "scan_GBps_lower_bound": round(4 * elems / (us * 1e-6) / 1e9, 1),
                           "what": "scan + bookkeeping + early-returning update grid, 50 back-to-back calls"}
    assert on.skipped()[1] == 55
    del arms, on
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
        raise SystemExit("bench_guard_overhead.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {}
    for b in [int(x) for x in args.batches.split(",")]:
        res["batch_%d" % b] = run_batch(args.dtype, b, args.steps, args.block, args.warmup, args.init_steps, device, args.pool_frames)
        print("# batch %d: %s" % (b, json.dumps(res["batch_%d" % b])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "phase1 (bench.py phase1_bs256 step), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18), guard off vs on, interleaved",
                       "dtype": args.dtype, "steps": args.steps, "block": args.block, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
