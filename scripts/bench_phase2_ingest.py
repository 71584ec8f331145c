"""Phase 2 on a recorded dataset (train_image_phase2.py --dataset_dir): what the offline rollout and the indexed replay buffer cost,
measured in one process.

    python scripts/bench_phase2_ingest.py [--batch 128] [--precision bf16] [--blocks 8] [--block 5] [--warmup 3] [--out FILE]

A 256-sample synthetic LMDB split is written to a temporary directory and held resident (ResidentLoader).  One student / teacher /
NativeTrainer (bench.py's models and L1 warm start below the horizon).  Three measurements, each with its arms INTERLEAVED in blocks
(a, b, a, b, ...) so that clock and thermal drift meets both; reported per arm: mean, median and the block-to-block spread (population
standard deviation) of the block times.
  (a) scoring   OfflineRollout.score over the 256 frames at --batch (both networks in eval mode + lbc_phase2_weight, no read-back),
                a block between two HIP events -> frames / s.
  (b) admit     lbc_replay_admit at n = limit = 100,000, m = 4,000 (launch + the read-back of its 16-byte record) against the decision path
                of DeviceReplayBuffer.add_batch on the same weights (torch.cat / topk / nonzero / bool(any()), its host syncs included; no
                frame is copied in either arm).  Wall clock per call, the device idle before and after.
  (c) step      the phase-2 training step (_device_step) fed by the indexed buffer (gather through the slot's frame index out of the
                resident dataset) against the copying DeviceReplayBuffer holding the same 256 frames; and the two gather launches alone.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
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


def summary(blocks, unit):
    return {unit + "_mean": round(statistics.mean(blocks), 4), unit + "_median": round(statistics.median(blocks), 4),
            unit + "_spread": round(statistics.pstdev(blocks), 4), "blocks": [round(x, 4) for x in blocks]}


def interleave(arms, blocks, block, warmup, wall=False):
    """arms: {name: fn}; -> {name: [ms per call of every block]}; wall: host clock around a drained device instead of HIP events"""
    out = {name: [] for name in arms}
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, fn in arms.items():
            if wall:
                t0 = time.perf_counter()
                for _ in range(block):
                    fn()
                torch.cuda.synchronize()
                out[name].append((time.perf_counter() - t0) * 1e3 / block)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(block):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[name].append(e0.elapsed_time(e1) / block)
    return out


def bench_admit(device, blocks, block, warmup, limit=100000, m=4000):
    from learningbycheating_amd import _lib
    lib = _lib.get()
    g = torch.Generator().manual_seed(7)
    F = limit + m
    stored = (torch.rand(limit, generator=g) * 3).to(device)
    cw = (torch.rand(m, generator=g) * 3).to(device)
    weights, frame = stored.clone(), torch.arange(limit, dtype=torch.int32, device=device)
    cmd, speed = torch.ones(limit, dtype=torch.int32, device=device), torch.ones(limit, device=device)
    sof = torch.full((F,), -1, dtype=torch.int32, device=device)
    sof[:limit] = frame
    state0 = [t.clone() for t in (weights, frame, sof)]
    cf = torch.arange(limit, F, dtype=torch.int32, device=device)
    cc, cs = torch.ones(m, dtype=torch.int32, device=device), torch.ones(m, device=device)
    need = int(lib.lbc_replay_admit_workspace(limit, m))
    ws, rec = torch.empty(need, dtype=torch.uint8, device=device), torch.zeros(4, dtype=torch.int32, device=device)
    last = {}

    def admit():
        for t, t0 in zip((weights, frame, sof), state0):           # (the call changes the buffer: every call starts from the same one)
            t.copy_(t0)
        _lib.check(lib.lbc_replay_admit(_lib.ptr(weights), _lib.ptr(frame), _lib.ptr(cmd), _lib.ptr(speed), _lib.ptr(sof), F, limit, limit, _lib.ptr(cw),
                                        _lib.ptr(cf), _lib.ptr(cc), _lib.ptr(cs), m, _lib.ptr(ws), need, _lib.ptr(rec), _lib.stream_for(ws)), "replay_admit")
        last["admit"] = [int(v) for v in rec.cpu()]

    def add_batch_decision():
        # DeviceReplayBuffer.add_batch on a full buffer (k = 0), up to the point where it knows which slots take which new frames
        for t, t0 in zip((weights, frame, sof), state0):           # (the same three copies, so that the arms differ in the decision only)
            t.copy_(t0)
        keep = torch.zeros(limit + m, dtype=torch.bool, device=device)
        keep[torch.topk(torch.cat([weights[:limit], cw]), limit).indices] = True
        evicted = torch.nonzero(~keep[:limit]).reshape(-1)
        survivors = torch.nonzero(keep[limit:]).reshape(-1)
        gone = evicted >= limit
        if bool(gone.any()):
            raise AssertionError
        last["add_batch"] = int(survivors.numel())
    times = interleave({"lbc_replay_admit": admit, "add_batch_decision": add_batch_decision}, blocks, block, warmup, wall=True)
    assert last["admit"][2] == last["add_batch"], (last, "the two paths admit different numbers of candidates")
    out = {name: summary(t, "ms_per_call") for name, t in times.items()}
    out.update(n=limit, limit=limit, m=m, admitted=last["admit"][2],
               what="wall clock per call with the device drained after every block; both arms first restore weights / frame / slot_of_frame (3 copies)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--init-steps", type=int, default=40, help="bench.py's below-horizon warm start")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_phase2_ingest.py needs a ROCm GPU")
    from learningbycheating_amd import _lib
    from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
    from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
    from learningbycheating_amd.training import train_image_phase2 as P2
    from learningbycheating_amd.training.native import NativeTrainer, camera_struct
    from learningbycheating_amd.training.replay import DeviceReplayBuffer
    from learningbycheating_amd.training.rollout import OfflineRollout
    assert _lib.backend() == "hip-gfx950"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    batch, res = args.batch, {}
    tmp = tempfile.TemporaryDirectory()               # (lives until the process ends: the dataset keeps its LMDB files open)
    D.write_synthetic_dataset(tmp.name, episodes=2, frames=128 + 25, seed=0)         # 2 x 128 samples per split
    store = ResidentLoader(D.ImageDataset(os.path.join(tmp.name, "train")), batch, 0, device, reserve_gb=0.0)
    F = store.frames
    student, teacher = bench.build_models(device, "phase1")
    student.precision = teacher.precision = args.precision
    every = np.arange(F)
    indexed = DeviceReplayBuffer(device, buffer_limit=F, seed=0, source=store)
    copying = DeviceReplayBuffer(device, buffer_limit=F, seed=0)
    cmd, speed = store.cmd_host.to(torch.int32).to(device), store.gather(every)[3]
    indexed.admit(every, cmd, speed, torch.ones(F, device=device))
    copying.add_batch(store.rgb, store.birdview, cmd, speed, torch.ones(F))
    g = torch.Generator().manual_seed(5)              # bench.py's warm-start targets
    tgt = torch.rand((batch, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    tgt = tgt.to(device)
    warm = NativeTrainer(student, None, batch, (3, 160, 384), device, phase="l1_all", lr=1e-3)
    for _ in range(args.init_steps):
        rgb, _, command, sp = copying.batch(copying.sample_indices(batch))
        warm.step(rgb, sp, command, target=tgt)
    del warm
    tr = NativeTrainer(student, teacher, batch, (3, 160, 384), device, phase=1, lr=1e-4, camera=camera_struct())
    # (a) the scoring pass
    rollout = OfflineRollout(store, tr, indexed, 0, seed=0)
    times = interleave({"score": lambda: rollout.score(every)}, args.blocks, 1, args.warmup)["score"]
    res["scoring"] = summary([F / (t * 1e-3) for t in times], "frames_per_s")
    res["scoring"].update(frames=F, ms_per_pass=summary(times, "ms"),
                          what="OfflineRollout.score over %d resident frames in chunks of %d: gather, student + teacher in eval mode, lbc_phase2_weight" % (F, batch))
    # (b) admission
    res["admit"] = bench_admit(device, args.blocks, args.block, args.warmup)
    # (c) the training step on either buffer
    w = torch.rand(F, generator=g) + 0.05
    for buf in (indexed, copying):
        buf.init_new_weights(); buf.new_weights[:F].copy_(w); buf.normalize_weights(); buf.init_new_weights()
    config = {"batch_size": batch, "speed_noise": 0.0, "batch_aug": 1}
    times = interleave({"copying": lambda: P2._device_step(copying, tr, config), "indexed": lambda: P2._device_step(indexed, tr, config)},
                       args.blocks, args.block, args.warmup)
    step = {name: summary(t, "ms_per_step") for name, t in times.items()}
    step["indexed_over_copying_mean"] = round(step["indexed"]["ms_per_step_mean"] / step["copying"]["ms_per_step_mean"], 4)
    step["indexed_not_slower"] = bool(step["indexed"]["ms_per_step_mean"] < step["copying"]["ms_per_step_mean"] + step["copying"]["ms_per_step_spread"])
    idx = indexed.sample_indices(batch)
    times = interleave({"copying": lambda: copying.batch(idx), "indexed": lambda: indexed.batch(idx)}, args.blocks, 4 * args.block, args.warmup)
    step["gather_ms_per_batch"] = {name: summary(t, "ms") for name, t in times.items()}
    step["what"] = "_device_step at batch %d, %s; gather_ms_per_batch = batch(): the two frame gathers + lbc_replay_meta + their output allocations" % (batch, args.precision)
    res["step"] = step
    line = json.dumps({"workload": "phase 2 on a recorded dataset: scoring pass, admission, training step on the indexed buffer", "batch": batch,
                       "precision": args.precision, "blocks": args.blocks, "block": args.block, "warmup": args.warmup, "init_steps": args.init_steps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
