"""Device-resident replay buffer of phase 2: the lbc_replay_* kernels (csrc/replay.hip) against numpy twins, DeviceReplayBuffer
(training/replay.py) against the host ReplayBuffer, and train_image_phase2.py --replay device (augmentation, --batch_aug, resume).

Every kernel test runs twice at the same small shapes: on the CPU emulator (the unmodified kernel source) and, marked gpu, on the
gfx950 library.  All comparisons with the twins are bitwise: the prefix sums use small integer weights (exact in double in any order),
the draws are integer hashes and one double product, rows are copied, the write-back is one f32 sum in index order."""
import ctypes

import numpy as np
import pytest
import torch

from learningbycheating_amd import _lib
from learningbycheating_amd.training.replay import DeviceReplayBuffer

gpu = pytest.mark.gpu
M32 = np.uint64(0xFFFFFFFF)


def both(fn):
    """fn(dev) as two tests: emulator and (marked gpu) the real library"""
    def cpu_test(env):
        fn(env[0])

    def gpu_test(env):
        fn(env[0])
    cpu_test.__doc__ = gpu_test.__doc__ = fn.__doc__
    return cpu_test, gpu(gpu_test)


# ---- numpy twins ------------------------------------------------------------------------------------------------
def np_hash_u32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def np_hash3(seed, a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    inner = np_hash_u32((b + np.uint64(0x85EBCA6B)) & M32)
    return np_hash_u32(np.uint64(seed) ^ np_hash_u32((a * np.uint64(0x9E3779B9) + inner) & M32))


def np_cdf(w):
    w = np.asarray(w, dtype=np.float32)
    ok = np.isfinite(w) & (w >= 0)
    return np.cumsum(np.where(ok, w, np.float32(0)).astype(np.float64)), int((~ok).sum())


def np_sample(cdf, seed, step, B):
    n = len(cdf)
    j = np.arange(B, dtype=np.uint64)
    t_lo, t_hi = step & 0xFFFFFFFF, step >> 32
    h1, h2 = np_hash3(seed ^ t_hi, 2 * j, t_lo), np_hash3(seed ^ t_hi, 2 * j + 1, t_lo)
    u01 = ((h1 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (h2 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    u = u01 * cdf[-1]
    idx = np.searchsorted(cdf, u, side="right")
    idx[idx >= n] = np.searchsorted(cdf, cdf[-1], side="left")
    return idx.astype(np.int32)


def np_writeback(new_w, w_batch, idx, reps, n):
    out = new_w.copy()
    for b, i in enumerate(idx):
        if 0 <= i < n:
            s = np.float32(0)
            for k in range(reps):
                s = np.float32(s + w_batch[b * reps + k])
            out[i] = np.float32(s / np.float32(reps))
    return out


def np_one_hot(cmd):
    out = np.zeros((len(cmd), 4), np.float32)
    out[np.arange(len(cmd)), np.clip(np.asarray(cmd) - 1, 0, 3)] = 1
    return out


# ---- raw kernel calls ---------------------------------------------------------------------------------------------
def k_cdf(w, dev):
    w = torch.as_tensor(w, dtype=torch.float32).to(dev)
    cdf = torch.full((w.numel(),), -1.0, dtype=torch.float64, device=dev)
    bad = torch.full((1,), -7, dtype=torch.int64, device=dev)
    _lib.check(_lib.get().lbc_replay_cdf(_lib.ptr(w), w.numel(), _lib.ptr(cdf), _lib.ptr(bad), _lib.stream_for(w)), "replay_cdf")
    return cdf.cpu().numpy(), int(bad.cpu()[0])


def k_sample(cdf_dev, seed, step, B):
    idx = torch.full((B,), -1, dtype=torch.int32, device=cdf_dev.device)
    _lib.check(_lib.get().lbc_replay_sample(_lib.ptr(cdf_dev), cdf_dev.numel(), seed, step, B, _lib.ptr(idx), _lib.stream_for(cdf_dev)), "replay_sample")
    return idx.cpu().numpy()


def zero_run_weights(n, g):
    """small integer weights with zero runs at the start, in the middle and at the end"""
    w = torch.randint(1, 9, (n,), generator=g).float()
    if n >= 32:
        w[:5] = 0; w[n // 2:n // 2 + 7] = 0; w[n - 9:] = 0
    return w


# ---- cdf -------------------------------------------------------------------------------------------------------------
def check_cdf(dev):
    """inclusive double prefix sums, bitwise equal to np.cumsum(float64) across tile boundaries; unusable weights count as 0"""
    g = torch.Generator().manual_seed(3)
    for n in (1, 255, 256, 257, 100003):
        w = zero_run_weights(n, g)
        got, bad = k_cdf(w, dev)
        want, _ = np_cdf(w.numpy())
        assert bad == 0 and np.array_equal(got, want), n
    w = zero_run_weights(2500, g)
    w[3], w[1023], w[1024], w[2499] = float("nan"), float("inf"), float("-inf"), -1.0
    got, bad = k_cdf(w, dev)
    want, nbad = np_cdf(w.numpy())
    assert nbad == 4 and bad == 4 and np.array_equal(got, want)


test_cdf, test_cdf_gpu = both(check_cdf)


# ---- sample ----------------------------------------------------------------------------------------------------------
CHI2_SEED = 12345


def chi2_of(idx):
    counts = np.bincount(idx, minlength=8).astype(np.float64)
    expect = np.arange(1, 9) / 36.0 * len(idx)
    return float(((counts - expect) ** 2 / expect).sum())


def check_sample(dev):
    """the draws are exactly the numpy twin's (np.searchsorted side='right' on the same cdf), never a zero-weight entry, a function of
    (seed, step) alone; 2^16 draws over weights 1..8 pass a chi-square test at the 99.9 % point (7 degrees of freedom: 24.32)"""
    g = torch.Generator().manual_seed(4)
    w = zero_run_weights(257, g)
    cdf, _ = np_cdf(w.numpy())
    cdf_dev = torch.from_numpy(cdf).to(dev)
    streams = {}
    for seed in (0, 0xDEADBEEF):
        for step in (0, 1, 2 ** 32 + 3):
            for B in (1, 5, 128, 1024):
                got = k_sample(cdf_dev, seed, step, B)
                assert np.array_equal(got, np_sample(cdf, seed, step, B)), (seed, step, B)
                assert (w.numpy()[got] > 0).all()
                assert np.array_equal(got, k_sample(cdf_dev, seed, step, B))
            streams[(seed, step)] = got
    keys = list(streams)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert not np.array_equal(streams[keys[a]], streams[keys[b]]), (keys[a], keys[b])
    cdf8 = np.cumsum(np.arange(1, 9, dtype=np.float64))
    assert chi2_of(np_sample(cdf8, CHI2_SEED, 7, 1 << 16)) < 24.32           # the twin, on the CPU, first
    got = k_sample(torch.from_numpy(cdf8).to(dev), CHI2_SEED, 7, 1 << 16)
    assert chi2_of(got) < 24.32


test_sample, test_sample_gpu = both(check_sample)


def check_sample_rounding_edge(dev):
    """a cdf whose total is reached early (zero weights behind it): whatever u is, the index is the last entry of non-zero weight at most"""
    cdf = np.array([0.0, 0.0, 5.0, 5.0, 5.0])
    got = k_sample(torch.from_numpy(cdf).to(dev), 1, 0, 64)
    assert (got == 2).all() and np.array_equal(got, np_sample(cdf, 1, 0, 64))


test_sample_rounding_edge, test_sample_rounding_edge_gpu = both(check_sample_rounding_edge)


# ---- gather / scatter / meta -----------------------------------------------------------------------------------------
def make_idx(B, n, g):
    idx = torch.randint(0, n, (B,), generator=g, dtype=torch.int32)
    idx[0] = 0
    if B >= 5:
        idx[1], idx[2], idx[3] = n - 1, 7, 7
    elif B == 1:
        idx[0] = n - 1
    return idx


def check_gather_scatter_meta(dev):
    """gather = src[idx].repeat_interleave(reps, 0), scatter = dst[slot] = src, meta = speed[idx] / one_hot(cmd[idx]) with the fan-out,
    all bitwise; a row size that is no multiple of 16 is refused by name"""
    lib = _lib.get()
    g = torch.Generator().manual_seed(5)
    n = 37
    for row_bytes in (16, 48, 184320):
        src = torch.randint(0, 256, (n, row_bytes), generator=g, dtype=torch.uint8)
        src_d = src.to(dev)
        for B in ((1, 5) if row_bytes > 48 else (1, 5, 128)):
            idx = make_idx(B, n, g)
            if B == 5:
                assert 0 in idx and n - 1 in idx and len(set(idx.tolist())) < B
            idx_d = idx.to(dev)
            for reps in (1, 3):
                dst = torch.zeros((B * reps, row_bytes), dtype=torch.uint8, device=dev)
                _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(src_d), row_bytes, _lib.ptr(idx_d), B, reps, _lib.ptr(dst), _lib.stream_for(dst)), "gather")
                assert torch.equal(dst.cpu(), src[idx.long()].repeat_interleave(reps, 0)), (row_bytes, B, reps)
        M = 5 if row_bytes > 48 else 20
        slots = torch.randperm(n, generator=g)[:M].to(torch.int32)
        base = torch.randint(0, 256, (n, row_bytes), generator=g, dtype=torch.uint8)
        dst = base.clone().to(dev)
        slots_d = slots.to(dev)
        _lib.check(lib.lbc_replay_scatter_u8(_lib.ptr(src_d), row_bytes, _lib.ptr(slots_d), M, _lib.ptr(dst), _lib.stream_for(dst)), "scatter")
        want = base.clone()
        want[slots.long()] = src[:M]
        assert torch.equal(dst.cpu(), want), row_bytes
    src_d = torch.zeros((4, 24), dtype=torch.uint8, device=dev)
    idx_d = torch.zeros(1, dtype=torch.int32, device=dev)
    dst = torch.zeros((1, 24), dtype=torch.uint8, device=dev)
    rc = lib.lbc_replay_gather_u8(_lib.ptr(src_d), 24, _lib.ptr(idx_d), 1, 1, _lib.ptr(dst), _lib.stream_for(dst))
    assert rc == -1 and "row_bytes" in lib.lbc_last_error().decode()          # LBC_EINVAL
    # meta
    speed = torch.rand(n, generator=g) * 10
    cmd = torch.randint(1, 5, (n,), generator=g, dtype=torch.int32)
    cmd[0], cmd[n - 1], cmd[7] = 0, 9, -3                                      # clamped like train_utils.one_hot
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    speed_d, cmd_d = speed.to(dev), cmd.to(dev)              # (named: a temporary's memory is handed out again before the kernel runs)
    for B in (1, 5, 128):
        idx = make_idx(B, n, g)
        idx_d = idx.to(dev)
        for reps in (1, 3):
            so = torch.zeros(B * reps, dtype=torch.float32, device=dev)
            oo = torch.full((B * reps, 4), -1.0, dtype=torch.float32, device=dev)
            _lib.check(lib.lbc_replay_meta(_lib.ptr(speed_d), _lib.ptr(cmd_d), _lib.ptr(idx_d), B, reps, _lib.ptr(so), _lib.ptr(oo),
                                           _lib.stream_for(so)), "meta")
            assert torch.equal(so.cpu(), speed[idx.long()].repeat_interleave(reps))
            want = one_hot(cmd[idx.long()]).repeat_interleave(reps, 0)
            assert torch.equal(oo.cpu(), want) and np.array_equal(want.numpy(), np.repeat(np_one_hot(cmd[idx.long()].numpy()), reps, 0))


test_gather_scatter_meta, test_gather_scatter_meta_gpu = both(check_gather_scatter_meta)


def check_wide_copy(dev):
    """above 2^20 16-byte words per launch the copy runs its four-words-per-lane form (16 KB spans): rows of 48 KB + 16 bytes = 3,073
    words (three whole spans and a last span of one word), gather of 128 x 3 rows and scatter of 384 rows (1.18 M words each), bitwise"""
    lib = _lib.get()
    g = torch.Generator().manual_seed(12)
    n, row_bytes, B, reps = 37, 48 * 1024 + 16, 128, 3
    assert B * reps * (row_bytes // 16) >= 1 << 20 and (row_bytes // 16) % 1024 not in (0, 1023)
    src = torch.randint(0, 256, (n, row_bytes), generator=g, dtype=torch.uint8)
    idx = make_idx(B, n, g)
    src_d, idx_d = src.to(dev), idx.to(dev)
    dst = torch.zeros((B * reps, row_bytes), dtype=torch.uint8, device=dev)
    _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(src_d), row_bytes, _lib.ptr(idx_d), B, reps, _lib.ptr(dst), _lib.stream_for(dst)), "gather")
    gathered = src[idx.long()].repeat_interleave(reps, 0)
    assert torch.equal(dst.cpu(), gathered)
    # scatter: the 384 gathered rows into distinct slots of a 400-row table
    M, rows = B * reps, 400
    slots = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    base = torch.randint(0, 256, (rows, row_bytes), generator=g, dtype=torch.uint8)
    table, slots_d = base.clone().to(dev), slots.to(dev)
    _lib.check(lib.lbc_replay_scatter_u8(_lib.ptr(dst), row_bytes, _lib.ptr(slots_d), M, _lib.ptr(table), _lib.stream_for(table)), "scatter")
    base[slots.long()] = gathered
    assert torch.equal(table.cpu(), base)


test_wide_copy, test_wide_copy_gpu = both(check_wide_copy)


# ---- write-back -------------------------------------------------------------------------------------------------------
def check_writeback(dev):
    """new_w[idx[b]] = f32 mean of sample b's reps weights, the last of equal indices wins, indices outside [0, n) are ignored, the rest
    is untouched; identical over 20 launches"""
    lib = _lib.get()
    g = torch.Generator().manual_seed(6)
    n = 50
    for B in (1, 7, 128):
        for reps in (1, 4):
            idx = torch.randint(0, n - 10, (B,), generator=g, dtype=torch.int32)            # (entries 40..49 stay untouched)
            if B >= 7:
                idx[0], idx[3], idx[6] = 11, 11, 11
                idx[1], idx[2], idx[4] = -1, 50, 10 ** 6
            if B == 128:
                idx[100], idx[127] = 11, 5
            w_batch = torch.rand(B * reps, generator=g) * 3
            base = torch.rand(n, generator=g)
            want = np_writeback(base.numpy(), w_batch.numpy(), idx.numpy(), reps, n)
            assert np.array_equal(want[40:], base.numpy()[40:])
            first, w_d, idx_d = None, w_batch.to(dev), idx.to(dev)
            for _ in range(20):
                new_w = base.clone().to(dev)
                _lib.check(lib.lbc_replay_writeback(_lib.ptr(w_d), _lib.ptr(idx_d), B, reps, n, _lib.ptr(new_w), _lib.stream_for(new_w)),
                           "writeback")
                got = new_w.cpu().numpy()
                first = got if first is None else first
                assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
            assert np.array_equal(first.view(np.uint32), want.view(np.uint32)), (B, reps)


test_writeback, test_writeback_gpu = both(check_writeback)


# ---- DeviceReplayBuffer against the host ReplayBuffer -----------------------------------------------------------------
RGB, BV = (4, 4, 3), (4, 4, 7)


def small_frames(m, g):
    rgb = torch.randint(0, 256, (m,) + RGB, generator=g, dtype=torch.uint8)
    bv01 = (torch.rand((m,) + BV, generator=g) < 0.3).to(torch.uint8)
    return rgb, bv01, torch.randint(1, 5, (m,), generator=g), torch.rand(m, generator=g) * 10


def fill_pair(dev, limit=16, adds=(10, 12, 3), seed=7):
    """the same frames with distinct weights into both classes (bird view 0/1 on the host, 0/255 on the device)"""
    from learningbycheating_amd.training.phase2_utils import ReplayBuffer
    g = torch.Generator().manual_seed(seed)
    host = ReplayBuffer(torch.device("cpu"), buffer_limit=limit, seed=1)
    devb = DeviceReplayBuffer(dev, buffer_limit=limit, seed=1, rgb_shape=RGB, birdview_shape=BV)
    weights = (torch.randperm(sum(adds), generator=g).float() + 1) / 2             # distinct, exact in f32
    at = 0
    for m in adds:
        rgb, bv01, cmd, speed = small_frames(m, g)
        w = weights[at:at + m]
        at += m
        host.add_batch(rgb, bv01, cmd, speed, w.tolist())
        devb.add_batch(rgb, bv01 * 255, cmd, speed, w)
    return host, devb


def records(rgb, bv01, cmd, speed, weights):
    chk = lambda t: (t.reshape(t.shape[0], -1).long() * torch.arange(1, t[0].numel() + 1)).sum(1).tolist()
    return sorted(zip([float(w) for w in weights], chk(rgb), chk(bv01), [int(c) for c in cmd], [float(s) for s in speed]))


def check_buffer_against_host(dev):
    """eviction keeps the same samples as the host class; an un-normalised epoch visits every sample once (drop_last); update_weights +
    normalize_weights give the host's weights; get_highest_k the same set; all-zero weights raise"""
    host, devb = fill_pair(dev)
    n = len(devb)
    assert n == len(host) == 16
    rec_h = records(host.rgb, host.birdview, host.cmd, host.speed, host._weights)
    rec_d = records(devb.rgb[:n].cpu(), devb.birdview[:n].cpu() // 255, devb.cmd[:n].cpu(), devb.speed[:n].cpu(), devb.weights[:n].cpu())
    assert rec_h == rec_d
    assert set(devb.birdview[:n].cpu().unique().tolist()) <= {0, 255}
    to_host = {i: int(np.nonzero(host._weights == float(w))[0][0]) for i, w in enumerate(devb.weights[:n].cpu())}     # slot -> host row
    # one epoch before normalisation: batches of 5 -> 3 batches, 15 distinct samples, the remainder dropped
    host.init_new_weights(); devb.init_new_weights()
    seen = []
    g = torch.Generator().manual_seed(8)
    for _ in range(n // 5):
        idx = devb.sample_indices(5)
        assert idx.dtype == torch.int32 and idx.device.type == dev.type
        vals = torch.rand(5, generator=g)
        devb.update_weights(idx, vals.to(dev))
        host.update_weights(np.array([to_host[i] for i in idx.cpu().tolist()]), vals)
        seen += idx.cpu().tolist()
    assert len(seen) == 15 and len(set(seen)) == 15
    assert devb.normalize_weights() == 0
    host.normalize_weights()
    assert devb.normalized
    wd = devb.weights[:n].cpu().numpy()
    assert np.array_equal(np.array([host._weights[to_host[i]] for i in range(n)], dtype=np.float32), wd)
    assert np.array_equal(devb.cdf[:n].cpu().numpy(), np_cdf(wd)[0])
    top_h = host.get_highest_k(4)[0]
    top_d, rgb, bv, onehot, speed = devb.get_highest_k(4)
    assert {to_host[i] for i in top_d.cpu().tolist()} == set(top_h.tolist())
    assert torch.equal(rgb.cpu(), devb.rgb[top_d.long()].cpu()) and onehot.shape == (4, 4)
    # weighted draws come from the kernel stream (seed, counter)
    d0 = devb.draws
    idx = devb.sample_indices(6).cpu().numpy()
    assert devb.draws == d0 + 1 and np.array_equal(idx, np_sample(np_cdf(wd)[0], devb.seed, d0, 6))
    devb.init_new_weights()
    devb.new_weights.zero_()
    with pytest.raises(ValueError, match="nothing to sample"):
        devb.normalize_weights()


test_buffer_against_host, test_buffer_against_host_gpu = both(check_buffer_against_host)


def check_buffer_batch_and_state(dev):
    """batch() with the fan-out equals torch indexing; state_dict -> load_state_dict into a fresh buffer: the next 5 index streams and
    batches are bitwise equal, in the shuffled epoch and in the weighted one; a state without frames checks n"""
    _, devb = fill_pair(dev)
    n = len(devb)
    idx = torch.tensor([3, 0, 3, 15], dtype=torch.int32)
    rgb, bv, onehot, speed = devb.batch(idx.to(dev), reps=2)
    li = idx.long().repeat_interleave(2)
    assert torch.equal(rgb.cpu(), devb.rgb.cpu()[li]) and torch.equal(bv.cpu(), devb.birdview.cpu()[li])
    assert torch.equal(speed.cpu(), devb.speed.cpu()[li]) and np.array_equal(onehot.cpu().numpy(), np_one_hot(devb.cmd.cpu().numpy()[li]))
    for normalised in (False, True):
        devb.init_new_weights()
        devb.sample_indices(3)                                         # (stand in the middle of a shuffled epoch)
        if normalised:
            devb.update_weights(torch.arange(n, dtype=torch.int32), torch.arange(n).float() % 5)
            devb.normalize_weights()
            devb.sample_indices(3)
        sd = devb.state_dict(include_frames=True)
        fresh = DeviceReplayBuffer(dev, buffer_limit=devb.buffer_limit, seed=99, rgb_shape=RGB, birdview_shape=BV)
        fresh.load_state_dict(sd)
        assert len(fresh) == n and fresh.normalized == normalised
        for _ in range(5):
            ia, ib = devb.sample_indices(3), fresh.sample_indices(3)
            assert torch.equal(ia.cpu(), ib.cpu())
            for ta, tb in zip(devb.batch(ia), fresh.batch(ib)):
                assert torch.equal(ta.cpu(), tb.cpu())
    light = devb.state_dict()
    assert "rgb" not in light
    empty = DeviceReplayBuffer(dev, buffer_limit=devb.buffer_limit, rgb_shape=RGB, birdview_shape=BV)
    with pytest.raises(ValueError, match="without frames"):
        empty.load_state_dict(light)
    devb.load_state_dict(light)


test_buffer_batch_and_state, test_buffer_batch_and_state_gpu = both(check_buffer_batch_and_state)


def test_add_data_and_growth(env):
    """add_data is add_batch of one sample; a buffer that is not full appends in order"""
    dev, _ = env
    g = torch.Generator().manual_seed(9)
    buf = DeviceReplayBuffer(dev, buffer_limit=4, rgb_shape=RGB, birdview_shape=BV)
    rgb, bv01, cmd, speed = small_frames(3, g)
    for i in range(3):
        buf.add_data(rgb[i].numpy(), int(cmd[i]), float(speed[i]), None, (bv01[i] * 255).numpy(), float(i + 1))
    assert len(buf) == 3 and torch.equal(buf.rgb[:3].cpu(), rgb) and buf.weights[:3].cpu().tolist() == [1.0, 2.0, 3.0]
    assert buf.cmd[:3].cpu().tolist() == cmd.tolist()


# ---- the script (GPU, batch 4) -----------------------------------------------------------------------------------------
SCRIPT = ["--synthetic", "64", "--max_episode", "1", "--batch_size", "4", "--precision", "fp32", "--log_iterations", "8", "--replay", "device"]


def run_script(tmp, extra, on_epoch_end=None):
    from learningbycheating_amd.training import train_image_phase2 as P2
    return P2.main(["--log_dir", str(tmp)] + SCRIPT + extra, on_epoch_end=on_epoch_end)


def warm_student(dev):
    """a seeded student, warm-started 30 L1 steps towards waypoints below the horizon as tests/test_step.py and bench.py do: the reference
    chains phase 0 -> phase 1 -> phase 2, an untrained student predicts ON the 1 / y pole of the unprojection"""
    from learningbycheating_amd.bird_view.models.image import ImagePolicyModelSS
    from learningbycheating_amd.training.native import NativeTrainer
    torch.manual_seed(61)
    student = ImagePolicyModelSS("resnet34", all_branch=True).to(dev)
    g = torch.Generator().manual_seed(65)
    x = torch.randint(0, 256, (4, 160, 384, 3), generator=g, dtype=torch.uint8).to(dev)
    speed, onehot = (torch.rand(4, generator=g) * 10).to(dev), torch.eye(4).to(dev)
    tgt = torch.rand((4, 4, 5, 2), generator=g)
    tgt[..., 0] = tgt[..., 0] * 1.2 - 0.6
    tgt[..., 1] = tgt[..., 1] * 0.5 + 0.3
    warm = NativeTrainer(student, None, 4, (3, 160, 384), dev, phase="l1_all", lr=1e-3)
    for _ in range(30):
        warm.step(x, speed, onehot, target=tgt.to(dev))
    torch.cuda.synchronize()
    del warm
    return student


@pytest.fixture(scope="module")
def warm_ckpt(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib._inject_for_tests(None)
    path = tmp_path_factory.mktemp("p2_warm") / "student.th"
    torch.save(warm_student(torch.device("cuda", 0)).state_dict(), str(path))
    return ["--ckpt", str(path)]


@pytest.fixture(scope="module")
def full_run(tmp_path_factory, warm_ckpt):
    """the uninterrupted 3-epoch run with --seed 3 (shared by the base and the resume test)"""
    tmp = tmp_path_factory.mktemp("p2_full")
    after_first = {}

    def hook(episode, epoch, buf, trainer):
        if epoch == 0:
            after_first["new_bits"] = buf.weights[:len(buf)].cpu().numpy().view(np.uint32).copy()
    out = run_script(tmp, warm_ckpt + ["--epoch_per_episode", "3", "--seed", "3"], hook)
    torch.cuda.synchronize()
    return tmp, out, after_first


@gpu
def test_script_device_replay_runs(env, full_run):
    """--replay device trains, writes model-0.th; after the first epoch every one of the 64 weights has been written (none holds the
    initial 1.0), and the weights stay finite"""
    tmp, out, after_first = full_run
    assert (tmp / "model-0.th").exists()
    buf = out["buffer"]
    assert len(buf) == 64 and buf.normalized
    assert not (after_first["new_bits"] == np.float32(1.0).view(np.uint32)).any()
    assert torch.isfinite(buf.weights[:64]).all()


@gpu
def test_script_augment_and_batch_aug(env, tmp_path, warm_ckpt):
    """--augment super_hard --batch_aug 2: the trainer runs 8 images per step, a step writes the weights of its 4 source samples only"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    out = run_script(tmp_path, warm_ckpt + ["--epoch_per_episode", "3", "--augment", "super_hard", "--batch_aug", "2", "--seed", "3"])
    buf, trainer = out["buffer"], out["trainer"]
    assert trainer.batch == 8 and (tmp_path / "model-0.th").exists()
    assert torch.isfinite(buf.weights[:64]).all()
    config = {"batch_size": 4, "batch_aug": 2, "speed_noise": 0.0, "augment": "super_hard", "aug_fix_iter": 1000000, "rank": 0}
    aug = P2.make_augmenter(config)
    buf.init_new_weights()
    before = buf.new_weights[:64].clone()
    idx, loss = P2._device_step(buf, trainer, config, aug)
    assert loss.shape == (8,) and idx.shape == (4,)
    changed = torch.nonzero(buf.new_weights[:64] != before).reshape(-1).cpu().tolist()
    assert set(changed) <= set(idx.cpu().tolist()) and len(changed) >= 1
    # the augmenter changes the gathered copies (each of a sample's two copies in its own way), not the stored frames
    plain = buf.batch(idx, 2)[0]
    assert torch.equal(plain[0], buf.rgb[idx[0].long()]) and torch.equal(plain[0], plain[1])
    augmented = aug.augment_batch(plain.clone())
    assert not torch.equal(augmented, plain) and not torch.equal(augmented[0::2], augmented[1::2])
    assert torch.equal(buf.batch(idx, 2)[0], plain)
    assert P2.make_augmenter(dict(config, augment="None")) is None


@gpu
def test_script_resume_is_bitwise(env, full_run, warm_ckpt, tmp_path):
    """stopped after epoch 1 with --save_state and continued with --resume: student and buffer weights bitwise equal to the
    uninterrupted run with the same --seed"""
    _, ref, _ = full_run
    run_script(tmp_path, warm_ckpt + ["--epoch_per_episode", "2", "--seed", "3", "--save_state"])
    assert (tmp_path / "train_state.th").exists() and not (tmp_path / "train_state.th.tmp").exists()
    state = torch.load(str(tmp_path / "train_state.th"), map_location="cpu")
    assert (state["episode"], state["epoch"]) == (0, 1) and "rgb" not in state["buffer"] and "optimizer" not in state
    seen = []
    out = run_script(tmp_path, warm_ckpt + ["--epoch_per_episode", "3", "--seed", "3", "--save_state", "--resume"], lambda ep, e, b, t: seen.append((ep, e)))
    assert seen == [(0, 2)]
    sa, sb = ref["net"].state_dict(), out["net"].state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(ref["buffer"].weights[:64], out["buffer"].weights[:64])
    assert ref["buffer"].draws == out["buffer"].draws


def test_script_flag_check(tmp_path):
    """--augment / --batch_aug / --save_state without --replay device exit with a message that names them"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    with pytest.raises(SystemExit) as e:
        P2.main(["--log_dir", str(tmp_path), "--augment", "super_hard", "--replay", "host"])
    assert "--augment" in str(e.value) and "--replay device" in str(e.value)
    with pytest.raises(SystemExit) as e:
        P2.main(["--log_dir", str(tmp_path), "--batch_aug", "2"])
    assert "--batch_aug" in str(e.value)


# ---- the two paths compute the same step ------------------------------------------------------------------------------
@gpu
def test_device_path_equals_host_path(env):
    """one phase-2 step at batch 4, fp32, same indices, through NativeTrainer.step in training mode (what _train / _device_step run),
    one trainer per path over the same warm-started student.

    (1) The device buffer's uint8 batch against the SAME frames as ToTensor floats (u8.float() / 255 computed on the host, as
        tests/test_model.py:1224 builds its float input): loss and phase2_weights bitwise equal, in eval and in training mode -- the
        tolerance of tests/test_model.py:1231 (torch.equal between the u8 and the float input paths) holds where its premise holds,
        the same input values.
    (2) The host ReplayBuffer.batch (bird view 0/1 there, 0/255 here) against the device path, a full step each.  The host class
        divides on the device, `float().div_(255.0)`, which torch evaluates there as a product with the rounded reciprocal: its
        pixels differ from ToTensor's in the last place (two roundings instead of one: asserted below, <= 2^-23), so the two paths do not
        compute on the same values and bit equality is not defined for them.  The bound is then the other one tests/test_model.py
        holds between the uint8 input path and the forward on ToTensor floats: 1e-4 (tests/test_model.py:1457), here on the student's
        waypoints, the per-sample loss and phase2_weights.  (An input perturbation of 6e-8 through a network whose f32 forward the
        same file holds to 1e-4 of the oracle sits far inside it.)  Each figure is printed before it is asserted."""
    from learningbycheating_amd.bird_view.models.birdview import BirdViewPolicyModelSS
    from learningbycheating_amd.bird_view.models.image import ImagePolicyModelSS
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    from learningbycheating_amd.training.native import NativeTrainer, camera_struct
    from learningbycheating_amd.training.train_image_phase2 import phase2_weights, synthetic_buffer, synthetic_buffer_device
    dev, _ = env
    net_h = warm_student(dev)
    net_d = ImagePolicyModelSS("resnet34", all_branch=True).to(dev)
    net_d.load_state_dict(net_h.state_dict())
    torch.manual_seed(5)
    teacher = BirdViewPolicyModelSS("resnet18", all_branch=True).to(dev)
    tr_h = NativeTrainer(net_h, teacher, 4, (3, 160, 384), dev, phase=1, camera=camera_struct())
    teacher_d = BirdViewPolicyModelSS("resnet18", all_branch=True).to(dev)          # (a module caches its executor: one teacher per trainer)
    teacher_d.load_state_dict(teacher.state_dict())
    tr_d = NativeTrainer(net_d, teacher_d, 4, (3, 160, 384), dev, phase=1, camera=camera_struct())
    host, devb = synthetic_buffer(12, dev, seed=2), synthetic_buffer_device(12, dev, seed=2)
    assert torch.equal(host.rgb, devb.rgb[:12]) and torch.equal(host.birdview * 255, devb.birdview[:12])
    idx = np.array([7, 0, 11, 7])
    rgb, bv, cmd, speed = host.batch(idx)
    rgb8, bv8, onehot, speed8 = devb.batch(torch.from_numpy(idx))
    assert rgb8.dtype == torch.uint8 and torch.equal(onehot.cpu(), one_hot(cmd)) and torch.equal(speed8, speed)

    def step(tr, x, b, **kw):
        loss = tr.step(x, speed8, onehot, birdview=b, **kw).clone()
        return loss, phase2_weights(tr, tr.last_pred[0], tr.last_teacher[0]).clone(), tr.last_pred[1].clone()

    # (1) same values, two input passes: exact
    exact = (rgb8.cpu().float() / 255.0).permute(0, 3, 1, 2).contiguous().to(dev)
    exact_bv = (bv8.cpu().float() / 255.0).permute(0, 3, 1, 2).contiguous().to(dev)
    assert torch.equal(exact_bv, bv)
    for kw in (dict(update=False, train_mode=False), dict(update=False)):
        lf, wf, _ = step(tr_d, exact, exact_bv, **kw)
        lu, wu, _ = step(tr_d, rgb8, bv8, **kw)
        assert torch.isfinite(lf).all() and torch.equal(lf, lu) and torch.equal(wf, wu), kw
    # (2) the host class's batch: a last-place rounding away in the pixels, a full training step on each path
    d_in = float((rgb - exact).abs().max())
    print("host batch vs ToTensor: max |pixel difference| = %.3e" % d_in)
    assert d_in <= 2.0 ** -23
    before = net_d.deconv[1].weight.detach().clone()
    lh, wh, ph = step(tr_h, rgb, bv)
    ld, wd, pd = step(tr_d, rgb8, bv8)
    figures = {"waypoints": float((ph - pd).abs().max()), "loss": float((lh - ld).abs().max()), "phase2_weights": float((wh - wd).abs().max())}
    print("host path vs device path, one training step: " + ", ".join("%s %.3e" % kv for kv in figures.items()))
    assert torch.isfinite(lh).all() and torch.isfinite(wh).all()
    assert all(v < 1e-4 for v in figures.values()), figures
    assert not torch.equal(net_d.deconv[1].weight.detach(), before)                  # (the step did update)
