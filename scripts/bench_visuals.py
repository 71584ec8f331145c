"""Cost of the training visuals (csrc/visuals.hip, training/visuals.py), measured in one process.

    python scripts/bench_visuals.py [--batch 32] [--dtype bf16] [--pass-batches 40] [--blocks 6] [--warmup 1] [--out FILE]

(a) "render_alone": the render launch at the three default configurations -- phase 0 (32 panels, sorted), phase 1 (8, unsorted),
    bird-view (16, sorted) -- on uint8 frames of this project's sizes, `calls` back-to-back launches between two HIP events (host
    enqueue included), next to the bytes the launch moves: the image written once, the shown samples' frames and bird-views read once.
(b) "validation_pass": the scripts' phase-1 validation pass with --val-metrics (NativeTrainer.step(update=False, train_mode=False,
    metrics=m), one m.result() after the last batch) on bench.py's phase-1 models, without and with visuals= on every batch plus the
    one image() after the last batch.  Both arms run over the SAME trainer INTERLEAVED in blocks of one pass each (A, B, A, B, ...); a
    block is timed on the host between two device synchronisations.  The margin to quote for the difference is arm A's own
    block-to-block spread.
(c) "host_baseline": what the reference does -- the same inputs copied to the host and drawn there, by the numpy twin of
    tests/test_visuals.py -- against the device path INCLUDING its read-back (render + image()), both on the host clock.
Prints one JSON line and writes it to --out (default profiles/visuals.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))

H, W, BH, BW = 160, 384, 192, 192


def _inputs(mode, n, device, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (n, 4, 5, 2) if mode == 1 else (n, 5, 2)
    pred = torch.rand(shape, generator=g) * 1.8 - 0.9
    if mode != 2:
        pred[..., 1] = torch.rand(shape[:-1], generator=g) * 0.8 + 0.1
    teach = torch.rand(shape, generator=g) * (192.0 if mode == 2 else 1.8) - (0.0 if mode == 2 else 0.9)
    command = torch.zeros((n, 4))
    command[torch.arange(n), torch.randint(0, 4, (n,), generator=g)] = 1.0
    loss = torch.rand(n, generator=g)
    rgb = None if mode == 2 else torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    bv = (torch.rand((n, BH, BW, 7), generator=g) < 0.1).to(torch.uint8)
    return [None if t is None else t.to(device) for t in (rgb, bv, pred, teach, command, loss)]


def render_alone(device, mode, n, calls=50):
    from learningbycheating_amd.training.visuals import PanelRenderer
    v = PanelRenderer(device, mode=mode)
    args = _inputs(mode, n, device, 11 + mode)
    for _ in range(5):
        out = v.render(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        v.render(*args)
    e1.record()
    torch.cuda.synchronize()
    shown = min(n, v.size)
    moved = out.numel() + shown * ((0 if mode == 2 else H * W * 3) + BH * BW * 7)
    us = e0.elapsed_time(e1) * 1000.0 / calls
    res = {"mode": mode, "panels": shown, "sorted": v.sort, "image": list(out.shape), "us_per_call": round(us, 2), "calls": calls,
           "bytes_moved": int(moved), "gb_per_s": round(moved / us / 1e3, 1), "what": "back-to-back launches, host enqueue included"}
    # (c) the device path with its read-back against copy-everything-and-draw-on-the-host
    from tests.test_visuals import CAM_FULL, _twin
    dev_ms, host_ms = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v.render(*args)
        img = v.image()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host = [None if t is None else t.cpu().numpy() for t in args]
        ref = _twin(mode, CAM_FULL, (H, W, BH, BW), v.size, v.sort, v.ncols, *host, strict=False)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["host_baseline"] = {"device_render_plus_readback_ms": round(statistics.median(dev_ms), 3), "host_copy_plus_numpy_ms": round(statistics.median(host_ms), 3),
                            "ratio": round(statistics.median(host_ms) / statistics.median(dev_ms), 1), "identical": bool(np.array_equal(img, ref))}
    return res


def validation_pass(prec, batch, pass_batches, blocks, warmup, init_steps, device, pool_frames):
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
    m, v = tr.make_metrics(), tr.make_visuals()

    def pass_a():
        m.reset()
        for b in batches(pass_batches):
            tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"], update=False, train_mode=False, metrics=m)
        return m.result()

    def pass_b():
        m.reset()
        for b in batches(pass_batches):
            tr.step(b["rgb"], b["speed"], b["onehot"], birdview=b["bv"], update=False, train_mode=False, metrics=m, visuals=v)
        return m.result(), v.image()

    arms = {"metrics": {"fn": pass_a, "blocks": []}, "metrics_and_visuals": {"fn": pass_b, "blocks": []}}
    for _ in range(warmup):
        pass_a()
        pass_b()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name in ("metrics", "metrics_and_visuals"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arms[name]["fn"]()
            torch.cuda.synchronize()
            arms[name]["blocks"].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for name, a in arms.items():
        bl = a["blocks"]
        out[name] = {"ms_per_pass_mean": round(statistics.mean(bl), 3), "ms_per_pass_median": round(statistics.median(bl), 3),
                     "ms_per_pass_min": round(min(bl), 3), "ms_per_pass_max": round(max(bl), 3),
                     "ms_per_batch_median": round(statistics.median(bl) / pass_batches, 4), "blocks_ms_per_pass": [round(x, 3) for x in bl]}
    a, b = out["metrics"], out["metrics_and_visuals"]
    out["visuals_minus_plain_percent_of_median"] = round(100.0 * (b["ms_per_pass_median"] / a["ms_per_pass_median"] - 1.0), 3)
    out["plain_spread_percent_of_median"] = round(100.0 * (a["ms_per_pass_max"] - a["ms_per_pass_min"]) / a["ms_per_pass_median"], 3)
    del tr, m, v, arms
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--pass-batches", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--pool-frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visuals.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visuals.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"render_alone": {name: render_alone(device, mode, 32) for name, mode in (("phase0", 0), ("phase1", 1), ("birdview", 2))}}
    print("# render alone: %s" % json.dumps(res["render_alone"]), file=sys.stderr, flush=True)
    res["validation_pass"] = validation_pass(args.dtype, args.batch, args.pass_batches, args.blocks, args.warmup, args.init_steps, device, args.pool_frames)
    line = json.dumps({"workload": "(a) lbc_visuals_render alone at the three default configurations; (b) phase-1 validation pass with metrics=, without and "
                                   "with visuals= on every batch, interleaved in blocks of one pass; (c) copy to the host + numpy against render + read-back",
                       "dtype": args.dtype, "batch": args.batch, "pass_batches": args.pass_batches, "blocks": args.blocks, "warmup": args.warmup,
                       "init_steps": args.init_steps, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
