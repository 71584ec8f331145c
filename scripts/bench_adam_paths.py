"""The four optimizer steps (lbc_adam_step, _guarded, _clipped, _recipe) of this tree's library against those of another build of the
library, loaded by path into the same process, on the student's table (136 tensors, 23.1 M elements).

    python scripts/bench_adam_paths.py --other /path/to/liblbc_hip.so [--steps 1000] [--rounds 7] [--warmup 100] [--out FILE]

Per step kind, three arms share one set of p / g / m / v / e buffers and one chunk table (each arm has its own record): `other_a` and
`other_b` are both the other library, `this` is the tree's.  The arms run ALTERNATING (other_a, this, other_b, other_a, ...) in windows of
--steps back-to-back calls between two HIP events, after --warmup calls each, so that clock and thermal drift meets all three.  Reported
per arm: the median and every window, in microseconds per step.  The other library against itself gives the margin, fixed here before
anything is measured: the spread (max - min) of all windows of other_a and other_b.  `inside_spread` says whether the median of `this`
lies within that margin of the median over both other arms; the difference of the two other arms' medians is reported beside it.
The clipped and recipe steps clip on every call (max_norm 1 against a norm near 4800); the recipe step is its most expensive
instantiation (cosine schedule with warm-up, decoupled decay, moving average).  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from learningbycheating_amd import _lib  # noqa: E402

KINDS = ("plain", "guarded", "clipped", "recipe")
ARMS = ("other_a", "this", "other_b")
LR, BETAS, EPS, WD, MAX_NORM = 1e-4, (0.9, 0.999), 1e-8, 0.01, 1.0


def student_table():
    from learningbycheating_amd.bird_view.models import ImagePolicyModelSS
    return [p.numel() for n, p in ImagePolicyModelSS("resnet34", all_branch=True).named_parameters() if not n.startswith("conv.fc.")]


class Table:
    """p, g, m, v, e as FusedAdam lays them out: every tensor on a 64-element boundary, chunks of 32768 elements"""

    def __init__(self, dev, sizes):
        off = np.cumsum([0] + [(n + 63) // 64 * 64 for n in sizes])
        total = int(off[-1])
        gen = torch.Generator().manual_seed(7)
        self.t = {"p": torch.randn(total, generator=gen), "g": torch.randn(total, generator=gen), "m": torch.randn(total, generator=gen) * 0.1,
                  "v": torch.rand(total, generator=gen) * 0.01, "e": torch.randn(total, generator=gen)}
        self.t = {k: x.to(dev) for k, x in self.t.items()}
        rows, eptr = [], []
        for o, n in zip(off[:-1], sizes):
            for c in range(0, n, 32768):
                rows.append(tuple(self.t[k].data_ptr() + 4 * (int(o) + c) for k in "pgmv") + (min(32768, n - c), 0))
                eptr.append(self.t["e"].data_ptr() + 4 * (int(o) + c))
        tab = np.zeros(len(rows), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("pad", "<i4")])
        for i, r in enumerate(rows):
            tab[i] = r
        self.nchunks, self.elements = len(rows), int(sum(sizes))
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self.ema_table = torch.from_numpy(np.array(eptr, dtype=np.uint64).view(np.int64).copy()).to(dev)


def make_step(lib, kind, tb, dev):
    """-> (a callable that enqueues one step, a callable that reads the record's header back or None)"""
    args = (_lib.ptr(tb.table), tb.nchunks)
    stream = _lib.stream_for(tb.table)
    if kind == "plain":
        count = [0]

        def step():
            count[0] += 1
            _lib.check(lib.lbc_adam_step(*args, LR, BETAS[0], BETAS[1], EPS, WD, count[0], stream), "adam_step")
        return step, None
    State, nbytes = {"guarded": (_lib.AdamState, lib.lbc_adam_state_bytes()), "clipped": (_lib.AdamClipState, lib.lbc_adam_clip_state_bytes(tb.nchunks)),
                     "recipe": (_lib.AdamRecipeState, lib.lbc_adam_recipe_state_bytes(tb.nchunks))}[kind]
    record = torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)
    rec = _lib.ptr(record)
    if kind == "guarded":
        step = lambda: _lib.check(lib.lbc_adam_step_guarded(*args, LR, BETAS[0], BETAS[1], EPS, WD, rec, stream), "adam_step_guarded")
    elif kind == "clipped":
        step = lambda: _lib.check(lib.lbc_adam_step_clipped(*args, LR, BETAS[0], BETAS[1], EPS, WD, MAX_NORM, rec, stream), "adam_step_clipped")
    else:
        rc = _lib.AdamRecipe(schedule=_lib.LR_SCHEDULES["cosine"], base_lr=LR, warmup_steps=100, warmup_start=0.25, total_steps=10 ** 6, min_lr=1e-6,
                             weight_decay=WD, decoupled=1, max_norm=MAX_NORM, ema_decay=0.999, beta1=BETAS[0], beta2=BETAS[1], eps=EPS)
        step = lambda: _lib.check(lib.lbc_adam_step_recipe(*args, ctypes.byref(rc), _lib.ptr(tb.ema_table), rec, stream), "adam_step_recipe")

    def read():
        torch.cuda.synchronize()
        return State.from_buffer_copy(record[:ctypes.sizeof(State)].cpu().numpy().tobytes())
    return step, read            # (read keeps the record alive)


def timed_us(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def run_kind(kind, libs, tb, dev, steps, rounds, warmup):
    arms = {a: make_step(libs[a], kind, tb, dev) for a in ARMS}
    for a in ARMS:
        timed_us(arms[a][0], warmup)
    windows = {a: [] for a in ARMS}
    for _ in range(rounds):
        for a in ARMS:
            windows[a].append(timed_us(arms[a][0], steps))
    out = {a: {"us_per_step_median": round(statistics.median(w), 3), "us_per_step_windows": [round(x, 3) for x in w]} for a, w in windows.items()}
    both = windows["other_a"] + windows["other_b"]
    other = statistics.median(both)
    out["other_us_per_step_median"] = round(other, 3)
    out["margin_us"] = round(max(both) - min(both), 3)
    out["other_a_minus_other_b_us"] = round(out["other_a"]["us_per_step_median"] - out["other_b"]["us_per_step_median"], 3)
    out["this_minus_other_us"] = round(out["this"]["us_per_step_median"] - other, 3)
    out["this_over_other_percent"] = round(100.0 * (out["this"]["us_per_step_median"] / other - 1.0), 3)
    out["inside_spread"] = bool(abs(out["this_minus_other_us"]) <= out["margin_us"])
    for a in ARMS:
        if arms[a][1] is not None:
            r = arms[a][1]()
            assert r.step == warmup + rounds * steps and r.skipped_total == 0, (kind, a, r.step, r.skipped_total)
            if kind != "guarded":
                assert r.clipped_total == r.step and r.clip_coef < 1.0, (kind, a, r.clipped_total)
    for k in "pmve":
        assert bool(torch.isfinite(tb.t[k]).all()), (kind, k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the library to compare with (a liblbc_hip.so of another build)")
    ap.add_argument("--other-name", default="other", help="what to call it in the output (a commit, say)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam_paths.py needs a ROCm GPU")
    other = _lib.load(os.path.abspath(args.other))
    this = _lib.load()
    assert other is not this and this.lbc_backend().decode() == other.lbc_backend().decode() == "hip-gfx950"
    libs = {"other_a": other, "this": this, "other_b": other}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = student_table()
    tb = Table(dev, sizes)
    res = {}
    for kind in KINDS:
        res[kind] = run_kind(kind, libs, tb, dev, args.steps, args.rounds, args.warmup)
        print("# %s: %s" % (kind, json.dumps(res[kind])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "the four optimizer steps on the ResNet-34 student's table, this tree's library against another build, alternating",
                       "other": args.other_name, "tensors": len(sizes), "elements": tb.elements, "chunks": tb.nchunks, "steps_per_window": args.steps,
                       "rounds": args.rounds, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
