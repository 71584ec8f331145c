"""Cost of gradient accumulation (NativeTrainer(accumulate=K)) on bench.py's phase-1 step: the same 256 images per optimizer step as
one batch of 256 or as K micro-batches of 256 / K, measured in one process.

    python scripts/bench_accum_overhead.py [--arms 256x1,128x2,64x4,32x8] [--dtype bf16] [--updates 24] [--block 4] [--warmup 4] [--out FILE]

One trainer per arm (batch b, accumulate K) over its own copy of the same models, bench.py's L1 warm start below the horizon, the synthetic
dataset resident in HBM.  The arms run INTERLEAVED in blocks of --block optimizer steps (= block * K calls of step()), each block between
two HIP events, so that clock and thermal drift meets all of them.  Reported per arm: mean, median and the block times per OPTIMIZER step,
and the block-to-block spread of the K = 1 arm, which is the margin of every comparison against it.  The arms differ in more than the
accumulation: K micro-batches launch every kernel of the forward and the backward K times, at batch b instead of 256 (DESIGN.md section 6:
small batches are launch-bound), so "ms per optimizer step" compares whole recipes.  The accumulation's own share comes from the built-in
launch profiler: one further window per arm on one stream with HIP events around every launch; `grad_accumulate` over the sum of all
classes.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
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


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class Arm:
    def __init__(self, prec, batch, K, init_steps, device, frames):
        """frames: the resident dataset (a bench.DevicePool's tensors), shared by the arms; every arm walks it at its own position"""
        from learningbycheating_amd.training.native import NativeTrainer
        self.batch, self.K, self.frames, self.pos = batch, K, frames, 0
        g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
        tgt = torch.rand((batch, 4, 5, 2), generator=g)
        tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
        tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
        tgt = tgt.to(device)
        student, teacher = bench.build_models(device, "phase1")
        student.precision = teacher.precision = prec
        warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
        for _ in range(init_steps):
            b = self.next_batch()
            warm.step(b["rgb"], b["speed"], b["onehot"], target=tgt)
        del warm
        self.tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4, accumulate=K)
        self.blocks = []

    def next_batch(self):
        n = self.frames["speed"].shape[0]
        if self.pos + self.batch > n:
            self.pos = 0
        s = slice(self.pos, self.pos + self.batch)
        self.pos += self.batch
        return {key: v[s] for key, v in self.frames.items()}

    def updates(self, n):
        """n optimizer steps = n windows of K micro-batches"""
        for _ in range(n * self.K):
            b = self.next_batch()
            self.tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"])
        assert self.tr.accum_index == 0

    def profile_window(self):
        """{kernel class: {"launches", "ms", "gbyte"}} of one window on one stream under the launch profiler"""
        from learningbycheating_amd import _lib
        lib = _lib.get()
        self.tr.overlap_teacher = False
        lib.lbc_profile_enable(1)
        self.updates(1)
        torch.cuda.synchronize()
        lib.lbc_profile_enable(0)
        self.tr.overlap_teacher = True
        buf = ctypes.create_string_buffer(1 << 16)
        nbytes = lib.lbc_profile_report(buf, len(buf))
        out = {}
        for line in buf.raw[:nbytes].decode().strip().splitlines():
            name, cnt, ms, fl, by = line.split()
            out[name] = {"launches": int(cnt), "ms": float(ms), "gbyte": float(by) / 1e9}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="256x1,128x2,64x4,32x8", help="batch x micro-batches per update, comma separated; the first is the baseline")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--updates", type=int, default=24, help="timed optimizer steps per arm")
    ap.add_argument("--block", type=int, default=4, help="optimizer steps per timed block")
    ap.add_argument("--warmup", type=int, default=4, help="untimed optimizer steps per arm")
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--pool-frames", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accum_overhead.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    specs = [tuple(int(x) for x in spec.lower().split("x")) for spec in args.arms.split(",")]
    frames = bench.DevicePool(bench.FramePool(args.pool_frames, max(b for b, _ in specs), device, 1000, need_rgb=True, slots=False)).t
    arms = []
    for b, k in specs:
        arms.append(Arm(args.dtype, b, k, args.init_steps, device, frames))
        arms[-1].updates(args.warmup)
    torch.cuda.synchronize()
    for _ in range((args.updates + args.block - 1) // args.block):
        for a in arms:
            a.blocks.append(_timed(lambda: a.updates(args.block)) / args.block)
    res = {}
    base = arms[0]
    for a in arms:
        prof = a.profile_window()
        total = sum(v["ms"] for v in prof.values())
        acc = prof.get("grad_accumulate", {"launches": 0, "ms": 0.0, "gbyte": 0.0})
        r = {"batch": a.batch, "accumulate": a.K, "images_per_optimizer_step": a.batch * a.K,
             "ms_per_optimizer_step_mean": round(statistics.mean(a.blocks), 4), "ms_per_optimizer_step_median": round(statistics.median(a.blocks), 4),
             "blocks_ms_per_optimizer_step": [round(x, 4) for x in a.blocks], "timed_optimizer_steps": args.block * len(a.blocks),
             "adam_step": a.tr.opt.step_count,
             "profiled_window": {"what": "one window on one stream, HIP events around every launch (serialized: the sum exceeds the timed step)",
                                 "kernel_ms_total": round(total, 4), "launches_total": sum(v["launches"] for v in prof.values()),
                                 "grad_accumulate_launches": acc["launches"], "grad_accumulate_ms": round(acc["ms"], 4),
                                 "grad_accumulate_us_per_micro_step": round(1000.0 * acc["ms"] / a.K, 2),
                                 "grad_accumulate_gbyte": round(acc["gbyte"], 4),
                                 "grad_accumulate_GBps": round(acc["gbyte"] / (acc["ms"] * 1e-3), 1) if acc["ms"] > 0 else None,
                                 "grad_accumulate_percent_of_kernel_ms": round(100.0 * acc["ms"] / total, 3) if total > 0 else None}}
        r["ms_per_optimizer_step_over_baseline"] = round(r["ms_per_optimizer_step_median"] / statistics.median(base.blocks), 4)
        res["%dx%d" % (a.batch, a.K)] = r
        print("# %dx%d: %s" % (a.batch, a.K, json.dumps(r)), file=sys.stderr, flush=True)
    bb = base.blocks
    res["baseline_block_spread_ms"] = {"max_minus_min": round(max(bb) - min(bb), 4), "stdev": round(statistics.pstdev(bb), 4)}
    line = json.dumps({"workload": "phase1 (bench.py phase1_bs256 step), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18), "
                                   "batch x accumulate arms interleaved in blocks of optimizer steps",
                       "dtype": args.dtype, "updates": args.updates, "block": args.block, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
