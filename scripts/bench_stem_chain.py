"""The five kernels of the input side of the step (lbc_u8nhwc_to_input, lbc_stem_fwd, lbc_maxpool3x3s2_fwd, lbc_maxpool3x3s2_bwd,
lbc_stem_wgrad) of this tree's library against those of another build of the library, loaded by path into the same process, at the
flagship workload's shapes: the student's 256 x 3 x 160 x 384 frames and the teacher's 256 x 7 x 192 x 192 bird views, bf16 tensors.

    python scripts/bench_stem_chain.py --other /path/to/liblbc_hip.so [--steps 50] [--rounds 7] [--warmup 10] [--out FILE]

Per kernel and shape, three arms share the inputs and the output buffers: `other_a` and `other_b` are both the other library, `this` is
the tree's.  The arms run ALTERNATING (other_a, this, other_b, other_a, ...) in windows of --steps back-to-back calls between two HIP
events, after --warmup calls each, so that clock and thermal drift meets all three.  The other library against itself gives the margin,
fixed before `this` is looked at: the spread (max - min) of all windows of other_a and other_b.  `faster` says whether the median of
`this` lies below the median over both other arms by more than that margin.  The input pass alternates between three sets of buffers:
one set would stay in the 256 MiB memory-side cache, which it does not in the step; every other kernel moves more than the cache holds.

Before anything is timed both libraries run the chain once on the same seeded inputs: the padded image, the stem output, the pooled
tensor, the taps and the masked gradient must be bit-identical (torch.equal); the statistics rows (summed over rows, taken with f32
outputs so that the float64 sums of y are their exact reference) and the weight gradient (against a float64 product of the unfolded
image and the gradient) may be summed in another order: `this` may err at most twice what the other library errs on that input, and
both errors are written out.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learningbycheating_amd import _lib  # noqa: E402

P = _lib.ptr
ARMS = ("other_a", "this", "other_b")
SHAPES = {"student_256x3x160x384": (256, 3, 160, 384), "teacher_256x7x192x192": (256, 7, 192, 192)}
OPS = ("prep_input", "stem_fwd", "bn_relu_maxpool_fwd", "maxpool_relu_bwd_reduce", "stem_wgrad")
PREP_SETS = 3


class Chain:
    """inputs and outputs of the five kernels at one shape; every method enqueues one call of `lib`"""

    def __init__(self, shape, dev, seed):
        N, C, H, W = self.shape = shape
        OH, OW = H // 2, W // 2
        g = torch.Generator(device=dev).manual_seed(seed)
        bf = torch.bfloat16
        self.u8 = [torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8, device=dev) for _ in range(PREP_SETS)]
        self.xps = [torch.empty((N, H + 6, W + 6, C), dtype=bf, device=dev) for _ in range(PREP_SETS)]
        self.xp = self.xps[0]
        self.w = torch.randn((64, 7, 7, C), generator=g, device=dev) * (2.0 / (49 * 64)) ** 0.5
        self.y0 = torch.empty((N, OH, OW, 64), dtype=bf, device=dev)
        self.p = torch.empty((N, OH // 2, OW // 2, 64), dtype=bf, device=dev)
        self.idx = torch.empty((N, OH // 2, OW // 2, 64), dtype=torch.uint8, device=dev)
        self.dp = torch.randn((N, OH // 2, OW // 2, 64), generator=g, device=dev).to(bf)
        self.g0 = torch.empty((N, OH, OW, 64), dtype=bf, device=dev)
        self.dw = torch.empty((64, 7, 7, C), device=dev)
        self.scale = torch.rand(64, generator=g, device=dev) + 0.5
        self.shift = torch.randn(64, generator=g, device=dev) * 0.2
        self.mean = torch.randn(64, generator=g, device=dev) * 0.1
        self.invstd = torch.rand(64, generator=g, device=dev) + 0.5
        self.stream = _lib.stream_for(self.xp)
        self.turn = 0

    def rows(self, lib, mode=2):
        N, C, H, W = self.shape
        r, rb = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.lbc_stem_fwd(None, None, None, None, ctypes.byref(r), N, H, W, C, mode, None))
        _lib.check(lib.lbc_maxpool3x3s2_bwd(None, None, None, None, None, None, None, None, None, ctypes.byref(rb), N, H // 2, W // 2, 64, 1, None))
        return r.value, rb.value

    def alloc(self, lib):
        """row and workspace buffers of the size `lib` asks for"""
        N, C, H, W = self.shape
        r, rb = self.rows(lib)
        self.stats = torch.empty((r, 2, 64), device=self.xp.device)
        self.part = torch.empty((rb, 2, 64), device=self.xp.device)
        self.ws = torch.empty(lib.lbc_stem_wgrad_workspace(N, H, W, C) // 4 + 1, device=self.xp.device)
        return r, rb, self.ws.numel()

    def prep_input(self, lib):
        N, C, H, W = self.shape
        k = self.turn = (self.turn + 1) % PREP_SETS
        _lib.check(lib.lbc_u8nhwc_to_input(P(self.u8[k]), P(self.xps[k]), 1, N, C, H, W, int(C == 3), self.stream))

    def stem_fwd(self, lib, y=None, stats=None, mode=2):
        N, C, H, W = self.shape
        r = ctypes.c_int(0)
        _lib.check(lib.lbc_stem_fwd(P(self.xp), P(self.w), P(self.y0 if y is None else y), P(self.stats if stats is None else stats),
                                    ctypes.byref(r), N, H, W, C, mode, self.stream))

    def bn_relu_maxpool_fwd(self, lib):
        N, C, H, W = self.shape
        _lib.check(lib.lbc_maxpool3x3s2_fwd(P(self.y0), P(self.scale), P(self.shift), P(self.p), P(self.idx), N, H // 2, W // 2, 64, 1, self.stream))

    def maxpool_relu_bwd_reduce(self, lib):
        N, C, H, W = self.shape
        r = ctypes.c_int(0)
        _lib.check(lib.lbc_maxpool3x3s2_bwd(P(self.dp), P(self.idx), P(self.y0), P(self.scale), P(self.shift), P(self.mean), P(self.invstd),
                                            P(self.g0), P(self.part), ctypes.byref(r), N, H // 2, W // 2, 64, 1, self.stream))

    def stem_wgrad(self, lib):
        N, C, H, W = self.shape
        _lib.check(lib.lbc_stem_wgrad(P(self.xp), P(self.g0), P(self.dw), P(self.ws), N, H, W, C, 2, self.stream))

    def run_all(self, lib):
        """the chain once, into fresh copies of every output: name -> tensor"""
        self.alloc(lib)
        self.turn = PREP_SETS - 1                       # -> set 0, the one the stem reads
        for op in OPS:
            getattr(self, op)(lib)
        torch.cuda.synchronize()
        return {"xp": self.xp.clone(), "y0": self.y0.clone(), "p": self.p.clone(), "idx": self.idx.clone(), "g0": self.g0.clone(),
                "partial": self.part.clone(), "dW": self.dw.clone()}

    def stats_f32(self, lib):
        """(statistics rows summed in float64 [2][64], float64 sums of the f32 output they were taken from [2][64])"""
        N, C, H, W = self.shape
        r, _ = self.rows(lib, 1)
        y = torch.empty((N, H // 2, W // 2, 64), device=self.xp.device)
        st = torch.empty((r, 2, 64), device=self.xp.device)
        self.stem_fwd(lib, y, st, 1)
        torch.cuda.synchronize()
        yd = y.view(-1, 64).double()
        return st.double().sum(0), torch.stack([yd.sum(0), (yd * yd).sum(0)])

    def dw_reference(self):
        """float64 weight gradient [64][7][7][C] of the chain's padded image and masked gradient"""
        N, C, H, W = self.shape
        ref = torch.zeros((64, 49 * C), dtype=torch.float64, device=self.xp.device)
        for n0 in range(0, N, 32):                      # (the unfolded image of 32 frames is about 1 GB in float64)
            pat = self.xp[n0:n0 + 32].double().unfold(1, 7, 2).unfold(2, 7, 2)          # [n][OH][OW][C][7][7]
            pat = pat.permute(0, 1, 2, 4, 5, 3).reshape(-1, 49 * C)
            ref += self.g0[n0:n0 + 32].double().reshape(-1, 64).t() @ pat
        return ref.view(64, 7, 7, C)


def compare(ch, libs):
    """-> (dict of findings, ok)"""
    other, this = ch.run_all(libs["other_a"]), ch.run_all(libs["this"])
    out = {k: bool(torch.equal(other[k], this[k])) for k in ("xp", "y0", "p", "idx", "g0")}
    ok = all(out.values())
    out["partial_rows_identical"] = bool(other["partial"].shape == this["partial"].shape and torch.equal(other["partial"], this["partial"]))
    ref = ch.dw_reference()
    scale = ref.abs().max().item()
    eo, et = ((other["dW"].double() - ref).abs().max().item() / scale, (this["dW"].double() - ref).abs().max().item() / scale)
    out["dW_max_error_over_largest_entry"] = {"other": eo, "this": et}
    ok = ok and et <= 2 * eo
    so, ro = ch.stats_f32(libs["other_a"])
    st, rt = ch.stats_f32(libs["this"])
    for i, name in enumerate(("stats_sum", "stats_sum_of_squares")):
        eo = ((so[i] - ro[i]).abs() / ro[i].abs().max()).max().item()
        et = ((st[i] - rt[i]).abs() / rt[i].abs().max()).max().item()
        out[name + "_max_error_over_largest_column"] = {"other": eo, "this": et}
        ok = ok and et <= 2 * eo
    out["ok"] = bool(ok)
    return out, ok


def timed_us(call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def run_op(ch, op, libs, steps, rounds, warmup):
    calls = {a: (lambda lib=libs[a]: getattr(ch, op)(lib)) for a in ARMS}
    for a in ARMS:
        timed_us(calls[a], warmup)
    windows = {a: [] for a in ARMS}
    for _ in range(rounds):
        for a in ARMS:
            windows[a].append(timed_us(calls[a], steps))
    out = {a: {"us_median": round(statistics.median(w), 2), "us_windows": [round(x, 2) for x in w]} for a, w in windows.items()}
    both = windows["other_a"] + windows["other_b"]
    other = statistics.median(both)
    out["other_us_median"] = round(other, 2)
    out["margin_us"] = round(max(both) - min(both), 2)
    out["this_minus_other_us"] = round(out["this"]["us_median"] - other, 2)
    out["this_over_other_percent"] = round(100.0 * (out["this"]["us_median"] / other - 1.0), 2)
    out["faster"] = bool(out["this_minus_other_us"] < -out["margin_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the library to compare with (a liblbc_hip.so of another build)")
    ap.add_argument("--other-name", default="other", help="what to call it in the output (a commit, say)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_chain.py needs a ROCm GPU")
    other = _lib.load(os.path.abspath(args.other))
    this = _lib.load()
    assert other is not this and this.lbc_backend().decode() == other.lbc_backend().decode() == "hip-gfx950"
    libs = {"other_a": other, "this": this, "other_b": other}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res, same = {}, {}
    for name, shape in SHAPES.items():
        ch = Chain(shape, dev, 11)
        same[name], ok = compare(ch, libs)
        print("# %s outputs: %s" % (name, json.dumps(same[name])), file=sys.stderr, flush=True)
        assert ok, "outputs differ from the other library's: %s" % json.dumps(same[name])
        sizes = ch.alloc(other)
        ch.run_all(this)                                  # every timed kernel reads what the chain produced
        assert ch.alloc(this) == sizes, "the libraries ask for different row counts: time them into buffers of their own"
        res[name] = {}
        for op in OPS:
            res[name][op] = run_op(ch, op, libs, args.steps, args.rounds, args.warmup)
            print("# %s %s: %s" % (name, op, json.dumps(res[name][op])), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "the five kernels of the input side of the step, this tree's library against another build, alternating",
                       "other": args.other_name, "steps_per_window": args.steps, "rounds": args.rounds, "warmup": args.warmup,
                       "device": torch.cuda.get_device_name(0), "outputs": same, "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
