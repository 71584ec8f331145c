"""The frozen teacher's waypoints cached per frame (ResidentLoader(teacher=...), --cache-teacher) against the teacher's forward in every
step, measured in one process.

    python scripts/bench_teacher_cache.py [--episodes 4] [--frames 89] [--step-batches 256,32] [--dtype bf16] [--block-batches 5]
                                          [--blocks 6] [--out FILE]

Dataset: write_synthetic_dataset (random frames in the reference's LMDB format) in a temporary directory, --episodes x (--frames - 25)
samples per split.  What is measured:
  (a) "step": the phase-1 training step (NativeTrainer.step, bench.py's models, warm-started below the horizon as bench.py does) at every
      batch size of --step-batches, fed by a ResidentLoader without a cache (`live`: today's path, the teacher's forward on the side
      stream of every step) and by one with a cache (`cached`: step(teacher_out=...), no teacher launch).  One trainer serves both arms
      -- the cached arm never touches its teacher engine -- and the arms alternate in blocks, a block timed on the host between two
      device synchronisations.  What to read off: live minus cached against each arm's own block-to-block spread;
  (b) "build": the seconds the cache took to build (one teacher forward per chunk of `batch` frames, the maps through the staging
      buffer) and the frames per second that is, beside the whole load;
  (c) "resident_bytes": what either loader keeps on the device, and the peak while the cache is built;
  (d) "gather": lbc_dataset_gather_rows_f32 alone, 50 back-to-back launches between two HIP events rotating over 8 records: microseconds
      per launch (host enqueue included);
  (e) "cache_vs_live": in fp32 and bf16, the cached rows against live forwards of a frozen engine -- the same chunks in the same order
      (values that differ: expected none), a shuffled batch with repeated frames and another batch size (largest deviation: expected 0,
      samples do not mix in an eval-mode forward).
Prints one JSON line and writes it to --out (default profiles/teacher_cache.json)."""
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
            "block_spread_ms": round((max(blocks_ms) - min(blocks_ms)) / per_block, 4), "blocks_ms": [round(x, 3) for x in blocks_ms]}


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


def step_arm(root, prec, batch, device, per_block, blocks, init_steps, synthetic_frames):
    from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
    from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
    from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    from learningbycheating_amd.training.data import _SyntheticLoader
    from learningbycheating_amd.training.native import NativeTrainer
    train = os.path.join(root, "train")
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = prec
    teacher.eval()
    live = ResidentLoader(D.ImageDataset(train), batch, 1 << 30, device, seed=1)
    cached = ResidentLoader(D.ImageDataset(train), batch, 1 << 30, device, seed=1, teacher=teacher)
    its = {"live": endless(live), "cached": endless(cached)}
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    syn = _SyntheticLoader(SyntheticFrames(synthetic_frames, device, seed=0), batch, init_steps)
    for rgb, bv, loc, cmd, speed in syn:
        warm.step(rgb, speed, one_hot(cmd).to(device), target=tgt)
    del warm, syn
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4)

    def feed_live(n):
        for rgb, bv, loc, cmd, speed in itertools.islice(its["live"], n):
            tr.step(rgb, speed, one_hot(cmd).to(device), birdview=bv)

    def feed_cached(n):
        for rgb, tw, loc, cmd, speed in itertools.islice(its["cached"], n):
            tr.step(rgb, speed, one_hot(cmd).to(device), teacher_out=tw)
    out = interleave({"live": feed_live, "cached": feed_cached}, per_block, blocks)
    saved = out["live"]["ms_per_batch_median"] - out["cached"]["ms_per_batch_median"]
    spread = max(out["live"]["block_spread_ms"], out["cached"]["block_spread_ms"])
    out["live_minus_cached_ms"] = round(saved, 4)
    out["larger_block_spread_ms"] = round(spread, 4)
    out["saving_outside_spread"] = bool(saved > spread)
    out["build"] = {"teacher_batch": cached.teacher_batch, "frames": cached.frames, "build_s": round(cached.build_seconds, 4),
                    "frames_per_s": round(cached.frames / max(cached.build_seconds, 1e-9), 1), "load_s_with_cache": round(cached.load_seconds, 4),
                    "load_s_without": round(live.load_seconds, 4)}
    out["resident_bytes"] = {"live": live.resident_bytes, "cached": cached.resident_bytes, "cache": cached.cache_bytes,
                             "cached_peak_while_building": cached.peak_bytes, "per_frame_live": live.resident_bytes // max(live.frames, 1),
                             "per_frame_cached": cached.resident_bytes // max(cached.frames, 1)}
    for it in its.values():
        it.close()
    del tr
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def gather_alone(frames, batches, device, calls=50, sets=8):
    from learningbycheating_amd import _lib
    lib, P = _lib.get(), _lib.ptr
    rng = np.random.RandomState(2)
    rows = torch.randn((frames, 50), device=device)
    out = {}
    for batch in batches:
        recs = []
        for _ in range(sets):
            r = np.zeros((batch, 4), np.int32)
            r[:, 0] = rng.randint(frames, size=batch)
            recs.append(torch.from_numpy(r).to(device))
        dst = [torch.empty((batch, 50), device=device) for _ in range(sets)]
        s = _lib.stream_for(rows)
        fn = lambda k: lib.lbc_dataset_gather_rows_f32(P(rows), P(recs[k]), 4, batch, 1, 50, P(dst[k]), s)
        for k in range(sets):
            _lib.check(fn(k), "dataset_gather_rows_f32")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for c in range(calls):
            _lib.check(fn(c % sets), "dataset_gather_rows_f32")
        e1.record()
        torch.cuda.synchronize()
        out["batch_%d" % batch] = {"us_per_launch": round(e0.elapsed_time(e1) * 1000.0 / calls, 2), "bytes_moved": 2 * batch * 200}
    out["what"] = "%d back-to-back launches (host enqueue included) rotating over %d records and outputs, %d cached frames" % (calls, sets, frames)
    return out


def cache_vs_live(root, device, teacher_batch=32, other_batch=24):
    from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
    from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    train = os.path.join(root, "train")
    plain = ResidentLoader(D.ImageDataset(train), teacher_batch, 1, device)
    F = plain.frames
    rng = np.random.RandomState(3)
    out = {}
    for prec in ("fp32", "bf16"):
        _, teacher = bench.build_models(device, "phase1")
        teacher.precision = prec
        teacher.eval()
        rows = ResidentLoader(D.ImageDataset(train), teacher_batch, 1, device, teacher=teacher, teacher_batch=teacher_batch).teacher_rows
        eng = teacher.engine((teacher_batch, 7, 192, 192), device, max_batch=teacher_batch, with_grads=False)
        eng.set_frozen(True)

        def live(idx):
            _, bv, _, speed = plain.gather(idx)
            sel, every = eng.forward(bv, speed, one_hot(plain.cmd_host[torch.from_numpy(idx.astype(np.int64))]).to(device), False)
            return torch.cat([every.reshape(len(idx), 40), sel.reshape(len(idx), 10)], dim=1)
        differing = sum(int((live(np.arange(f0, min(f0 + teacher_batch, F))) != rows[f0:f0 + teacher_batch]).sum()) for f0 in range(0, F, teacher_batch))
        shuffled = [np.repeat(rng.randint(F, size=teacher_batch // 2), 2)[rng.permutation(teacher_batch)] for _ in range(4)]
        dev_shuffled = max(float((live(i) - rows[torch.from_numpy(i).to(device)]).abs().max()) for i in shuffled)
        dev_other = max(float((live(np.arange(f0, min(f0 + other_batch, F))) - rows[f0:f0 + other_batch]).abs().max()) for f0 in range(0, F, other_batch))
        out[prec] = {"same_chunks_values_differing": differing, "shuffled_repeated_max_abs": dev_shuffled,
                     "batch_%d_max_abs" % other_batch: dev_other, "cache_built_at_batch": teacher_batch, "frames": F}
        del eng, teacher
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--frames", type=int, default=89, help="stored frames per episode (25 of them only serve as futures)")
    ap.add_argument("--step-batches", default="256,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--block-batches", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--synthetic", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher_cache.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_teacher_cache.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.utils.datasets.image_lmdb import write_synthetic_dataset
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    batches = [int(x) for x in args.step_batches.split(",")]
    root = tempfile.mkdtemp(prefix="lbc_teacher_cache_bench_")
    try:
        t0 = time.time()
        write_synthetic_dataset(root, episodes=args.episodes, frames=args.frames, seed=11)
        print("# dataset written in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
        res = {"step": {}}
        for b in batches:
            res["step"]["batch_%d" % b] = step_arm(root, args.dtype, b, device, args.block_batches, args.blocks, args.init_steps, args.synthetic)
            print("# step, batch %d: %s" % (b, json.dumps(res["step"]["batch_%d" % b])), file=sys.stderr, flush=True)
        res["gather"] = gather_alone(args.episodes * (args.frames - 25), batches, device)
        res["cache_vs_live"] = cache_vs_live(root, device)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps({"workload": "LMDB dataset (write_synthetic_dataset, %d episodes x %d frames per split) held by ResidentLoader with and without "
                                   "the teacher cache; phase-1 training step, ImagePolicyModelSS(resnet34) vs BirdViewPolicyModelSS(resnet18)"
                                   % (args.episodes, args.frames),
                       "dtype": args.dtype, "block_batches": args.block_batches, "blocks": args.blocks, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
