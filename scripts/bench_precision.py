"""Throughput of the precision modes that keep every tensor f32, on bench.py's phase1_bs256 workload, in one process.

    python scripts/bench_precision.py [--modes fp32,bf16_mfma,bf16x3] [--batch 256] [--steps 20] [--warmup 5]

bench.py is the project's fixed yardstick and its --dtype does not offer "bf16x3"; this script runs the same step for each mode in
turn: the models of bench.build_models, bench.py's L1 warm start below the horizon (run in the mode being measured, as bench.py does),
the synthetic dataset resident in HBM (bench.DevicePool, a different batch every step), warmup steps, then timed steps between two
HIP events.  After the timed steps one extra step runs serialized on one stream under the launch profiler and gives the convolution
family's algorithmic rate (FLOPs booked per launch = 2 * M * K * C * taps, whatever the kernel multiplies).  --batch 32 is the
per-GPU load of the 8-GPU run.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

# (the host threads come from the environment -- OMP_NUM_THREADS -- not from the machine's core count)
if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))


def conv_profile(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    nbytes = lib.lbc_profile_report(buf, len(buf))
    ms = gf = 0.0
    classes = {}
    for line in buf.raw[:nbytes].decode().strip().splitlines():
        name, cnt, t, fl, _ = line.split()
        if name.startswith("conv_"):
            ms += float(t); gf += float(fl) / 1e9
            classes[name] = int(cnt)
    return ms, gf, classes


def run_mode(prec, batch, steps, warmup, init_steps, device, host_pool, tgt):
    from learningbycheating_amd import _lib
    from learningbycheating_amd.training.native import NativeTrainer
    pool = bench.DevicePool(host_pool)
    pool.batch = batch
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = prec

    def run(tr, n, warm=False):
        for i in range(n):
            k = i & 1
            b = pool.get(k)
            if warm:
                tr.step(b["rgb"], b["speed"], b["onehot"], target=tgt)
            else:
                tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"])
            pool.release(k)
            pool.prefetch(k)

    pool.pos = 0
    pool.prefetch(0); pool.prefetch(1)
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    run(warm, init_steps, warm=True)
    del warm
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4)
    run(tr, warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(tr, steps)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    lib = _lib.get()
    lib.lbc_profile_enable(1)
    tr.overlap_teacher = False
    run(tr, 1)
    torch.cuda.synchronize()
    lib.lbc_profile_enable(0)
    cms, cgf, classes = conv_profile(lib)
    out = {"ms_per_step": round(ms, 3), "img_per_s": round(batch * 1000.0 / ms, 1),
           "conv_ms_serialized": round(cms, 3), "conv_algorithmic_tflops": round(cgf / cms, 2) if cms > 0 else None,
           "conv_classes": classes}
    del tr, student, teacher, pool
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32,bf16_mfma,bf16x3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--pool-frames", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_precision.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    host_pool = bench.FramePool(args.pool_frames, args.batch, device, 1000, need_rgb=True, slots=True)
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((args.batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    res = {}
    for prec in args.modes.split(","):
        res[prec] = run_mode(prec, args.batch, args.steps, args.warmup, args.init_steps, device, host_pool, tgt)
        print("# %s: %s" % (prec, json.dumps(res[prec])), file=sys.stderr, flush=True)
    if "fp32" in res:
        for v in res.values():
            v["speedup_vs_fp32"] = round(res["fp32"]["ms_per_step"] / v["ms_per_step"], 3)
    print(json.dumps({"workload": "phase1 (bench.py phase1_bs256 step), ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18)",
                      "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "init_steps": args.init_steps,
                      "device": torch.cuda.get_device_name(0), "modes": res}))


if __name__ == "__main__":
    main()
