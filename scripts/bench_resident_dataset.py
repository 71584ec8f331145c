"""The LMDB dataset through the host loader (DeviceLoader) and held in HBM (ResidentLoader, --resident), measured in one process.

    python scripts/bench_resident_dataset.py [--episodes 4] [--frames 89] [--loader-batches 32,256] [--step-batches 256] [--dtype bf16]
                                             [--block-batches 5] [--blocks 6] [--out FILE]

Dataset: write_synthetic_dataset (random frames in the reference's LMDB format) in a temporary directory, --episodes x (--frames - 25)
samples per split.  Three arms, each interleaved in blocks so that clock and thermal drift meets every contestant, a block timed on
the host between two device synchronisations:
  (a) "loader_alone": batches per second of DeviceLoader and of ResidentLoader, nothing consuming the batch;
  (b) "step": the phase-1 training step (NativeTrainer.step, bench.py's models, warm-started below the horizon as bench.py does) fed by
      DeviceLoader, by ResidentLoader and by the --synthetic loader.  What to read off: resident minus synthetic against the
      synthetic arm's own block-to-block spread, and host over resident as measured;
  (c) "kernels": lbc_dataset_gather_crop_u8 (camera frames; the map's fixed window out of whole maps), lbc_dataset_gather_warp_crop_u8
      and lbc_dataset_targets alone, 50 back-to-back launches between two HIP events rotating over 8 index sets: microseconds per launch
      and algorithmic bytes (window read once + written once) per second.  With a dataset of a few hundred frames the source stays in
      the 256 MB Infinity Cache: these are not HBM figures.
Prints one JSON line and writes it to --out (default profiles/resident_dataset.json)."""
import argparse
import itertools
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))


def summary(blocks_ms, per_block):
    med = statistics.median(blocks_ms)
    return {"ms_per_batch_median": round(med / per_block, 4), "ms_per_batch_mean": round(statistics.mean(blocks_ms) / per_block, 4),
            "ms_per_batch_min": round(min(blocks_ms) / per_block, 4), "ms_per_batch_max": round(max(blocks_ms) / per_block, 4),
            "batches_per_s_median": round(1e3 * per_block / med, 2), "blocks_ms": [round(x, 3) for x in blocks_ms]}


def interleave(arms, per_block, blocks, warmup=1):
    """arms: {name: fn(n) that consumes n batches}; -> {name: summary}"""
    times = {k: [] for k in arms}
    for r in range(warmup + blocks):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(per_block)
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: summary(v, per_block) for k, v in times.items()}


def endless(loader):
    while True:
        yield from loader


def make_loaders(root, batch, device):
    from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
    from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
    train = os.path.join(root, "train")
    host = D.DeviceLoader(D.ImageDataset(train), batch, 1 << 30, device, seed=1)
    res = ResidentLoader(D.ImageDataset(train), batch, 1 << 30, device, seed=1)
    return host, res


def loader_alone(root, batch, device, per_block, blocks):
    host, res = make_loaders(root, batch, device)
    its = {"host": endless(host), "resident": endless(res)}
    arms = {k: (lambda n, it=it: [None for _ in itertools.islice(it, n)]) for k, it in its.items()}
    out = interleave(arms, per_block, blocks)
    out["host_over_resident"] = round(out["host"]["ms_per_batch_median"] / out["resident"]["ms_per_batch_median"], 2)
    out["resident_bytes"], out["resident_load_s"] = res.resident_bytes, round(res.load_seconds, 3)
    for it in its.values():
        it.close()
    return out


def step_arm(root, prec, batch, device, per_block, blocks, init_steps, synthetic_frames):
    from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    from learningbycheating_amd.training.data import _SyntheticLoader
    from learningbycheating_amd.training.native import NativeTrainer
    host, res = make_loaders(root, batch, device)
    syn = _SyntheticLoader(SyntheticFrames(synthetic_frames, device, seed=0), batch, 1 << 30)
    its = {"synthetic": endless(syn), "resident": endless(res), "host": endless(host)}
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = prec
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    for rgb, bv, loc, cmd, speed in itertools.islice(its["synthetic"], init_steps):
        warm.step(rgb, speed, one_hot(cmd).to(device), target=tgt)
    del warm
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4)

    def feed(it):
        def run(n):
            for rgb, bv, loc, cmd, speed in itertools.islice(it, n):
                tr.step(rgb, speed, one_hot(cmd).to(device), birdview=bv)
        return run
    out = interleave({k: feed(it) for k, it in its.items()}, per_block, blocks)
    syn_s, res_s, host_s = out["synthetic"], out["resident"], out["host"]
    out["resident_minus_synthetic_ms"] = round(res_s["ms_per_batch_median"] - syn_s["ms_per_batch_median"], 4)
    out["synthetic_block_spread_ms"] = round(syn_s["ms_per_batch_max"] - syn_s["ms_per_batch_min"], 4)
    out["resident_within_synthetic_spread"] = bool(out["resident_minus_synthetic_ms"] <= out["synthetic_block_spread_ms"])
    out["host_over_resident"] = round(host_s["ms_per_batch_median"] / res_s["ms_per_batch_median"], 2)
    for it in its.values():
        it.close()
    del tr
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def kernels_alone(root, batch, device, calls=50, sets=8):
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.utils.datasets import birdview_lmdb as B
    from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
    from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
    lib = _lib.get()
    train = os.path.join(root, "train")
    img = ResidentLoader(D.ImageDataset(train), batch, 1, device)
    bvl = ResidentLoader(B.BirdViewDataset(train, crop_x_jitter=5, crop_y_jitter=5, angle_jitter=15), batch, 1, device)
    rng = np.random.RandomState(2)
    F = img.frames
    recs = []
    for _ in range(sets):
        r = np.empty((batch, 4), np.int32)
        r[:, 0] = rng.randint(F, size=batch)
        r[:, 1], r[:, 2], r[:, 3] = rng.randint(-15, 16, size=batch), rng.randint(-5, 6, size=batch), rng.randint(-10, -4, size=batch)
        recs.append(torch.from_numpy(r).to(device))
    idxs = [r[:, 0].contiguous() for r in recs]
    rgb = [torch.empty((batch, 160, 384, 3), dtype=torch.uint8, device=device) for _ in range(sets)]
    bv = [torch.empty((batch, 192, 192, 7), dtype=torch.uint8, device=device) for _ in range(sets)]
    loc, speed = torch.empty((batch, 5, 2), device=device), torch.empty(batch, device=device)
    s = _lib.stream_for(loc)
    P = _lib.ptr
    launches = {
        "gather_crop_rgb": (lambda k: lib.lbc_dataset_gather_crop_u8(P(img.rgb), P(idxs[k]), batch, 1, 160, 384, 3, 0, 0, 160, 384, P(rgb[k]), s),
                            2.0 * batch * 160 * 384 * 3),
        "gather_crop_map_window": (lambda k: lib.lbc_dataset_gather_crop_u8(P(bvl.birdview), P(idxs[k]), batch, 1, 320, 320, 7, 58, 64, 192, 192, P(bv[k]), s),
                                   2.0 * batch * 192 * 192 * 7),
        "gather_warp_crop": (lambda k: lib.lbc_dataset_gather_warp_crop_u8(P(bvl.birdview), P(recs[k]), P(bvl.warp_table), 15, batch, 1, 320, 320, 7, 192, 192,
                                                                           P(bv[k]), s), 2.0 * batch * 192 * 192 * 7),
        "targets": (lambda k: lib.lbc_dataset_targets(P(bvl.table), P(bvl.row_of_sample), P(recs[k]), batch, 1, 5, 5, 320, 192, P(loc), P(speed), s),
                    batch * (6 * 20.0 + 16 + 44)),
    }
    out = {}
    for name, (fn, nbytes) in launches.items():
        for k in range(sets):
            _lib.check(fn(k), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for c in range(calls):
            _lib.check(fn(c % sets), name)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / calls
        out[name] = {"us_per_launch": round(us, 2), "algorithmic_bytes": int(nbytes), "GB_per_s": round(nbytes / us / 1e3, 1)}
    out["what"] = ("%d back-to-back launches (host enqueue included) rotating over %d index sets and outputs, %d resident frames: the source "
                   "fits the Infinity Cache, not an HBM figure" % (calls, sets, F))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--frames", type=int, default=89, help="stored frames per episode (25 of them only serve as futures)")
    ap.add_argument("--loader-batches", default="32,256")
    ap.add_argument("--step-batches", default="256")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--block-batches", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--synthetic", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_dataset.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident_dataset.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.utils.datasets.image_lmdb import write_synthetic_dataset
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    root = tempfile.mkdtemp(prefix="lbc_resident_bench_")
    try:
        t0 = time.time()
        write_synthetic_dataset(root, episodes=args.episodes, frames=args.frames, seed=11)
        print("# dataset written in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
        res = {"loader_alone": {}, "step": {}}
        for b in [int(x) for x in args.loader_batches.split(",")]:
            res["loader_alone"]["batch_%d" % b] = loader_alone(root, b, device, args.block_batches, args.blocks)
            print("# loader alone, batch %d: %s" % (b, json.dumps(res["loader_alone"]["batch_%d" % b])), file=sys.stderr, flush=True)
        for b in [int(x) for x in args.step_batches.split(",")]:
            res["step"]["batch_%d" % b] = step_arm(root, args.dtype, b, device, args.block_batches, args.blocks, args.init_steps, args.synthetic)
            print("# step, batch %d: %s" % (b, json.dumps(res["step"]["batch_%d" % b])), file=sys.stderr, flush=True)
        res["kernels"] = kernels_alone(root, 256, device)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps({"workload": "LMDB dataset (write_synthetic_dataset, %d episodes x %d frames per split) through DeviceLoader and ResidentLoader; "
                                   "phase-1 training step, ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18)" % (args.episodes, args.frames),
                       "dtype": args.dtype, "block_batches": args.block_batches, "blocks": args.blocks, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
