"""Cost of the optimizer's recipe path (NativeTrainer(lr_schedule=..., weight_decay=..., ema_decay=...): csrc/adam.hip) over the
clipped step it is built like, on bench.py's phase-1 step, measured in one process.

    python scripts/bench_recipe_overhead.py [--batches 256,32] [--dtype bf16] [--steps 60] [--block 10] [--warmup 10] [--out FILE]

Three trainers per batch size over their own copies of the same models, bench.py's L1 warm start below the horizon, the synthetic dataset
resident in HBM: `clipped` (max_grad_norm=0: measures the norm, never clips), `recipe` (warm-up + cosine schedule and decoupled weight
decay; the bytes of the clipped step) and `recipe_ema` (the same with the moving average: 8 B/element more).  The arms run INTERLEAVED in
blocks of --block steps, each block between two HIP events, so that clock and thermal drift meets all three.  Reported per arm: mean,
median, the block times per step and the block-to-block spread; the comparison is against `clipped` OF THIS PROCESS, its margin that arm's
own spread.  No threshold is fixed: the figures are recorded.  Then the optimizer alone, 5 interleaved rounds of 50 back-to-back calls
per arm: a clean call (gradient pass + bookkeeping + update) and a skipped one (one infinity in the gradients: the update grid returns at
once); their difference is the update launch alone.  Prints one JSON line; --out also writes it to a file."""
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

ARMS = ("clipped", "recipe", "recipe_ema")
SCHEDULE = {"kind": "cosine", "warmup_steps": 20, "warmup_start": 0.1, "total_steps": 100000, "min_lr": 1e-6}
ARM_KW = {"clipped": dict(max_grad_norm=0.0),
          "recipe": dict(lr_schedule=SCHEDULE, weight_decay=0.01),
          "recipe_ema": dict(lr_schedule=SCHEDULE, weight_decay=0.01, ema_decay=0.999)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _spread(blocks):
    return {"max_minus_min": round(max(blocks) - min(blocks), 4), "stdev": round(statistics.pstdev(blocks), 4)}


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
        tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4, **ARM_KW[name])
        run(tr, warmup)
        arms[name] = {"tr": tr, "blocks": []}
    torch.cuda.synchronize()
    for _ in range((steps + block - 1) // block):
        for name in ARMS:
            arms[name]["blocks"].append(_timed(lambda: run(arms[name]["tr"], block)) / block)
    out = {}
    for name, a in arms.items():
        st = a["tr"].lr_stats()
        out[name] = {"ms_per_step_mean": round(statistics.mean(a["blocks"]), 4), "ms_per_step_median": round(statistics.median(a["blocks"]), 4),
                     "blocks_ms_per_step": [round(x, 4) for x in a["blocks"]], "block_spread_ms": _spread(a["blocks"]),
                     "timed_steps": block * len(a["blocks"]), "skipped": list(a["tr"].skipped()), "adam_step": a["tr"].opt.step_count,
                     "lr_last": st["lr"], "ema_updates": st["ema_updates"], "grad_norm_last": a["tr"].grad_stats()["grad_norm"]}
    base = out["clipped"]
    for name in ARMS[1:]:
        d = out[name]["ms_per_step_median"] - base["ms_per_step_median"]
        out[name + "_vs_clipped"] = {"ms_mean": round(out[name]["ms_per_step_mean"] - base["ms_per_step_mean"], 4), "ms_median": round(d, 4),
                                     "percent_of_median": round(100.0 * d / base["ms_per_step_median"], 3),
                                     "inside_clipped_block_spread": bool(abs(d) <= base["block_spread_ms"]["max_minus_min"])}
    # the optimizer alone: clean calls on the gradients the last step left, then skipped calls (one infinity: the update grid returns at once)
    elems = sum(n for _, n in arms["clipped"]["tr"].opt.offsets.values())
    alone = {"what": "opt.step() alone, 5 interleaved rounds of 50 back-to-back calls per arm; clean = gradient pass + bookkeeping + update, skipped "
                     "= the same with an update grid that returns at once, update = clean - skipped", "elements": elems}
    for kind in ("clean", "skipped"):
        calls = {n: [] for n in ARMS}
        for name in ARMS:
            if kind == "skipped":
                arms[name]["tr"].eng.grad_flat[0] = float("inf")
            for _ in range(5):
                arms[name]["tr"].opt.step()
        torch.cuda.synchronize()
        for _ in range(5):
            for name in ARMS:
                opt = arms[name]["tr"].opt
                calls[name].append(_timed(lambda: [opt.step() for _ in range(50)]) * 1000.0 / 50)
        for name in ARMS:
            alone.setdefault(name, {})[kind + "_us_median"] = round(statistics.median(calls[name]), 2)
            alone[name][kind + "_us_rounds"] = [round(x, 2) for x in calls[name]]
    for name in ARMS:
        a = alone[name]
        a["update_us"] = round(a["clean_us_median"] - a["skipped_us_median"], 2)
        bytes_per = 36.0 if name == "recipe_ema" else 28.0          # (the update launch: p, g, m, v read, p, m, v written; e read and written)
        a["update_GBps_lower_bound"] = round(bytes_per * elems / (a["update_us"] * 1e-6) / 1e9, 1) if a["update_us"] > 0 else None
        assert arms[name]["tr"].skipped()[1] == 5 + 5 * 50
    out["optimizer_alone"] = alone
    del arms
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
        raise SystemExit("bench_recipe_overhead.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {}
    for b in [int(x) for x in args.batches.split(",")]:
        res["batch_%d" % b] = run_batch(args.dtype, b, args.steps, args.block, args.warmup, args.init_steps, device, args.pool_frames)
        print("# batch %d: %s" % (b, json.dumps(res["batch_%d" % b])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "phase1 (bench.py phase1_bs256 step), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18), clipped "
                                   "(measure-only) vs recipe vs recipe + moving average, interleaved",
                       "dtype": args.dtype, "steps": args.steps, "block": args.block, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
