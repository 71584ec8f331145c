"""Cost of a validation pass with and without --val-metrics on the phase-1 step, measured in one process.

    python scripts/bench_val_metrics.py [--batches 256,32] [--dtype bf16] [--pass-batches 40] [--blocks 6] [--warmup 1] [--out FILE]

Workload: the scripts' validation pass, NativeTrainer.step(update=False, train_mode=False) on bench.py's phase-1 models (warm-started
below the horizon as bench.py does), --pass-batches batches per pass, the synthetic dataset resident in HBM.
  arm A "item_per_batch": today's loop, `loss.mean().item()` after every batch (one device-to-host sync per batch) -- the baseline;
  arm B "metrics":        step(..., metrics=m) and one m.result() after the last batch (--val-metrics).
Both arms run over the SAME trainer (a non-updating eval-mode step changes nothing) INTERLEAVED in blocks of one pass each
(A, B, A, B, ...), so that clock and thermal drift meets both; a block is timed on the host between two device synchronisations,
because arm A's cost IS host round trips.  Reported per arm: mean / median / spread of the block times; the margin to quote for the
difference is arm A's own block-to-block spread.  Then the update launch alone: 50 back-to-back lbc_waypoint_metrics_update calls at
N = 256 and N = 32 between two HIP events.  Prints one JSON line and writes it to --out (default profiles/val_metrics.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))


def run_batch(prec, batch, pass_batches, blocks, warmup, init_steps, device, pool_frames):
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

    def batches(n):
        for _ in range(n):
            k = state["i"] & 1
            state["i"] += 1
            yield pool.get(k)
            pool.release(k)
            pool.prefetch(k)

    pool.pos = 0
    pool.prefetch(0); pool.prefetch(1)
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = prec
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    for b in batches(init_steps):
        warm.step(b["rgb"], b["speed"], b["onehot"], target=tgt)
    del warm
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4)
    m = tr.make_metrics()

    def pass_a():
        last = None
        for b in batches(pass_batches):
            last = tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"], update=False, train_mode=False).mean().item()
        return last

    def pass_b():
        m.reset()
        for b in batches(pass_batches):
            tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"], update=False, train_mode=False, metrics=m)
        return m.result()

    arms = {"item_per_batch": {"fn": pass_a, "blocks": []}, "metrics": {"fn": pass_b, "blocks": []}}
    for _ in range(warmup):
        pass_a()
        pass_b()
    torch.cuda.synchronize()
    res = None
    for _ in range(blocks):
        for name in ("item_per_batch", "metrics"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = arms[name]["fn"]()
            torch.cuda.synchronize()
            arms[name]["blocks"].append((time.perf_counter() - t0) * 1e3)
            if name == "metrics":
                res = r
    out = {}
    for name, a in arms.items():
        bl = a["blocks"]
        out[name] = {"ms_per_pass_mean": round(statistics.mean(bl), 3), "ms_per_pass_median": round(statistics.median(bl), 3),
                     "ms_per_pass_min": round(min(bl), 3), "ms_per_pass_max": round(max(bl), 3),
                     "ms_per_pass_stdev": round(statistics.stdev(bl), 3) if len(bl) > 1 else None,
                     "ms_per_batch_median": round(statistics.median(bl) / pass_batches, 4), "blocks_ms_per_pass": [round(x, 3) for x in bl]}
    a, b = out["item_per_batch"], out["metrics"]
    out["metrics_minus_item_percent_of_median"] = round(100.0 * (b["ms_per_pass_median"] / a["ms_per_pass_median"] - 1.0), 3)
    out["item_per_batch_spread_percent_of_median"] = round(100.0 * (a["ms_per_pass_max"] - a["ms_per_pass_min"]) / a["ms_per_pass_median"], 3)
    out["last_result"] = {k: res[k] for k in ("samples", "ade", "fde", "bad_rows", "loss_mean")}
    del tr, m, arms
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def update_alone(device, n, calls=50):
    """`calls` back-to-back updates (rows = 20, with the loss) between two HIP events -> microseconds per call"""
    from learningbycheating_amd.training.metrics import WaypointMetrics
    g = torch.Generator().manual_seed(9)
    pred = torch.rand((n, 4, 5, 2), generator=g)
    pred[..., 0] = pred[..., 0] * 1.8 - 0.9
    pred[..., 1] = pred[..., 1] * 0.8 + 0.1
    target = torch.rand((n, 4, 5, 2), generator=g) * 1.8 - 0.9
    command = torch.zeros((n, 4))
    command[torch.arange(n), torch.randint(0, 4, (n,), generator=g)] = 1.0
    loss = torch.rand(n, generator=g)
    pred, target, command, loss = (t.to(device) for t in (pred, target, command, loss))
    m = WaypointMetrics(device)
    for _ in range(5):
        m.update(pred, target, command, loss)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        m.update(pred, target, command, loss)
    e1.record()
    torch.cuda.synchronize()
    assert m.result()["samples"] == (calls + 5) * n
    return {"us_per_call": round(e0.elapsed_time(e1) * 1000.0 / calls, 2), "calls": calls, "rows": 20, "what": "back-to-back launches, host enqueue included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--pass-batches", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--pool-frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_metrics.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_val_metrics.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {}
    for b in [int(x) for x in args.batches.split(",")]:
        res["batch_%d" % b] = run_batch(args.dtype, b, args.pass_batches, args.blocks, args.warmup, args.init_steps, device, args.pool_frames)
        res["batch_%d" % b]["update_alone"] = update_alone(device, b)
        print("# batch %d: %s" % (b, json.dumps(res["batch_%d" % b])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "phase-1 validation pass (update=False, train_mode=False), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18): "
                                   "loss.mean().item() per batch vs metrics= with one result() per pass, interleaved in blocks of one pass",
                       "dtype": args.dtype, "pass_batches": args.pass_batches, "blocks": args.blocks, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
