"""The device-resident LMDB dataset (bird_view/utils/datasets/resident.py ResidentLoader, csrc/dataset.hip): the three kernels against
numpy, the existing warp kernel and ImageDataset.raw(); the loader against DeviceLoader batch by batch, states exchanged between the
two classes; the memory budget; the training script with --resident.  Kernel cases run on the CPU emulator and, marked gpu, on the
MI355X, where every launch runs helpers.REPEATS times with bit-identical results."""
import json
import os

import numpy as np
import pytest
import torch

from learningbycheating_amd import _lib
from learningbycheating_amd.bird_view.utils.datasets import birdview_lmdb as B
from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
from learningbycheating_amd.bird_view.utils.datasets.resident import RESERVE_GB, ResidentLoader
from tests.helpers import WHERE, repeat

gpu = pytest.mark.gpu
SENTINEL, PAD = 0xA5, 256            # bytes around every gathered output (PAD keeps the output 16-byte aligned)
LOC_TOL = 1e-3                       # px: f64 cos / sin ulp over a lever arm below 500 px (1e-13) + the f32 rounding of a value below 256 (1.5e-5), x 60


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("lbc_resident")
    D.write_synthetic_dataset(str(root), episodes=2, frames=40, seed=3)
    return str(root)


def fenced(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def check_fence(buf, shape):
    n = int(np.prod(shape))
    b = buf.cpu()
    assert bool((b[:PAD] == SENTINEL).all()) and bool((b[PAD + n:] == SENTINEL).all()), "the kernel wrote outside its output"
    return b[PAD:PAD + n].view(shape).numpy()


def gather_crop(dev, src_d, idx, reps, y0, x0, H, W):
    """-> the output as numpy, launched through helpers.repeat into fenced buffers"""
    F, SH, SW, C = src_d.shape
    idx_d = torch.tensor(idx, dtype=torch.int32).to(dev)
    shape = (len(idx) * reps, H, W, C)

    def launch():
        buf, out = fenced(shape, dev)
        _lib.check(_lib.get().lbc_dataset_gather_crop_u8(_lib.ptr(src_d), _lib.ptr(idx_d), len(idx), reps, SH, SW, C, y0, x0, H, W, _lib.ptr(out),
                                                         _lib.stream_for(out)), "dataset_gather_crop_u8")
        return (buf,)
    return check_fence(repeat(dev, launch)[0], shape)


INDEX_SETS = {1: [5], 3: [4, 2, 2], 5: [5, 3, 3, 1, 0]}      # repeated and descending; first and last frame


# ---- 1. gather-crop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_gather_crop_equals_numpy_slicing(env, where):
    """rows of 35 bytes (byte path), the stored map's 1,344-byte rows at the 448-byte offset (16-byte path), a column offset that is no
    multiple of 16 bytes, the whole frame (the camera frames' gather); B in {1, 3, 5}, reps in {1, 3}; bit for bit, fences untouched"""
    dev, _ = env
    rng = np.random.RandomState(21)
    cases = [((9, 11, 7), (2, 3, 4, 5)),                     # 35-byte rows
             ((320, 320, 7), (58, 64, 192, 192)),            # the fixed window of the stored map
             ((320, 320, 7), (311, 65, 9, 192)),             # x0 * C = 455: the byte path on 1,344-byte rows, up to the last source row
             ((160, 384, 3), (0, 0, 160, 384)),              # the whole frame
             ((24, 16, 16), (3, 5, 21, 11))]                 # 176-byte rows: a window narrower than one 256-lane span per row
    for (SH, SW, C), (y0, x0, H, W) in cases:
        src = rng.randint(0, 256, size=(6, SH, SW, C)).astype(np.uint8)
        src_d = torch.from_numpy(src).to(dev)
        for nb, idx in INDEX_SETS.items():
            for reps in (1, 3):
                got = gather_crop(dev, src_d, idx, reps, y0, x0, H, W)
                want = np.repeat(src[idx][:, y0:y0 + H, x0:x0 + W], reps, axis=0)
                assert np.array_equal(got, want), ((SH, SW, C), (y0, x0, H, W), idx, reps)


@pytest.mark.parametrize("where", WHERE)
def test_gather_crop_wide_launch(env, where):
    """66 windows of 16,128 words pass 2^20 words per launch: the four-words-per-lane form (15 whole spans and a last span of 768 words
    per window)"""
    dev, _ = env
    rng = np.random.RandomState(22)
    src = rng.randint(0, 256, size=(4, 320, 320, 7)).astype(np.uint8)
    idx = [int(i) for i in rng.randint(0, 4, size=22)]
    assert len(idx) * 3 * 192 * 84 >= 1 << 20 and (192 * 84) % 1024 != 0
    got = gather_crop(dev, torch.from_numpy(src).to(dev), idx, 3, 58, 64, 192, 192)
    assert np.array_equal(got, np.repeat(src[idx][:, 58:250, 64:256], 3, axis=0))


# ---- 2. indexed warp-crop ------------------------------------------------------------------------------------------------------------
WARP_CASES = [(0, 0, -10), (1, 5, -5), (-1, -5, -10), (15, 5, -10), (-15, -5, -5), (15, -5, -5), (3, -60, 40), (-15, 70, -90)]    # the last two leave the map


def warp_through_index(dev, src_d, rec, A, reps):
    table = torch.from_numpy(np.stack([D.warp_params(a, 0, 0) for a in range(-A, A + 1)])).to(dev)
    draws = torch.from_numpy(np.asarray(rec, np.int32)).to(dev)
    shape = (len(rec) * reps, 192, 192, 7)

    def launch():
        buf, out = fenced(shape, dev)
        _lib.check(_lib.get().lbc_dataset_gather_warp_crop_u8(_lib.ptr(src_d), _lib.ptr(draws), _lib.ptr(table), A, len(rec), reps, 320, 320, 7, 192, 192,
                                                              _lib.ptr(out), _lib.stream_for(out)), "dataset_gather_warp_crop_u8")
        return (buf,)
    return check_fence(repeat(dev, launch)[0], shape)


def warp_in_place(dev, frames_d, jitters):
    """the existing kernel on contiguous frames: the reference of the indexed one"""
    params = torch.from_numpy(np.stack([D.warp_params(a, dx, dy) for a, dx, dy in jitters])).to(dev)
    out = torch.empty((len(jitters), 192, 192, 7), dtype=torch.uint8, device=dev)
    _lib.check(_lib.get().lbc_birdview_warp_crop_u8(_lib.ptr(frames_d), _lib.ptr(out), _lib.ptr(params), len(jitters), 320, 320, 7, 192, 192,
                                                    _lib.stream_for(out)), "birdview_warp_crop_u8")
    return out.cpu().numpy()


@pytest.mark.parametrize("where", WHERE)
def test_gather_warp_crop_equals_the_warp_kernel_on_gathered_frames(env, where):
    """angles 0, +-1, +-15, dx / dy at both extremes, windows that reach the zero border; frames through repeated and descending indices"""
    dev, _ = env
    rng = np.random.RandomState(23)
    src = rng.randint(0, 256, size=(6, 320, 320, 7)).astype(np.uint8)
    src_d = torch.from_numpy(src).to(dev)
    idx = [5, 3, 3, 1, 0, 4, 2, 5]
    rec = [(i,) + j for i, j in zip(idx, WARP_CASES)]
    want = warp_in_place(dev, torch.from_numpy(src[idx]).to(dev), WARP_CASES)
    assert np.array_equal(want[0], src[5, 58:250, 64:256])                       # (angle 0: the plain window)
    assert (want[6] == 0).any() and (want[7] == 0).all(axis=-1).any()           # (the border is reached)
    for reps in (1, 2):
        got = warp_through_index(dev, src_d, rec, 15, reps)
        assert np.array_equal(got, np.repeat(want, reps, axis=0)), reps
    one = warp_through_index(dev, src_d, rec[3:4], 15, 1)                        # B = 1
    assert np.array_equal(one, want[3:4])


# ---- 3. targets ----------------------------------------------------------------------------------------------------------------------
JITTERS = [(0, 0, -10)] + [(a, dx, dy) for a in (15, -15) for dx in (5, -5) for dy in (-10, -5)]


@pytest.mark.parametrize("where", WHERE)
def test_targets_equal_raw_for_every_sample(env, dataset_dir, where):
    """every sample of both episodes (the last of one and the first of the other among them) at nine jitters: speed bit-equal, waypoints
    within 1e-3 px of raw()'s float64 (worst case printed; measured on the MI355X: 7.6e-6 px, which is the f32 rounding of the result --
    none of the 5,400 values differs from float32(raw))"""
    dev, _ = env
    ds = B.BirdViewDataset(os.path.join(dataset_dir, "train"), crop_x_jitter=5, crop_y_jitter=5, angle_jitter=15)
    ld = ResidentLoader(ds, 3, 1, dev, seed=1, reserve_gb=0)
    n = len(ds)
    assert n == 30 and ds.file_map[14] != ds.file_map[15] and ld.rows == 2 * 40
    worst, differing = 0.0, 0
    for a, dx, dy in JITTERS:
        rec = np.array([(i, a, dx, dy) for i in range(n)], np.int32)
        for reps in (1, 2):
            _, loc, speed = repeat(dev, lambda: ld.gather(rec, reps)[1:])
            loc, speed = loc.cpu().numpy()[::reps], speed.cpu().numpy()[::reps]
            for i in range(n):
                _, _, l, c, s = ds.raw(i, a, dx, dy)
                assert speed[i].tobytes() == np.float32(s).tobytes(), (i, speed[i], s)
                worst = max(worst, float(np.abs(loc[i].astype(np.float64) - l).max()))
                differing += int((loc[i] != l.astype(np.float32)).sum())
    print("targets: worst |loc - raw| = %.3e px, %d of %d values differ from float32(raw)" % (worst, differing, len(JITTERS) * 2 * n * 10))
    assert worst <= LOC_TOL, worst


# ---- 4. loader equivalence -----------------------------------------------------------------------------------------------------------
def _datasets(dataset_dir):
    train = os.path.join(dataset_dir, "train")
    return {"image": (lambda: D.ImageDataset(train), {}),
            "image_batch_aug": (lambda: D.ImageDataset(train, batch_aug=3), {"batch_aug": 3}),
            "image_medium": (lambda: D.ImageDataset(train, augment_strategy="medium"), {"augment": "medium"}),
            "birdview_jitter": (lambda: B.BirdViewDataset(train, crop_x_jitter=5, crop_y_jitter=5, angle_jitter=15), {}),
            "birdview_biased": (lambda: B.BiasedBirdViewDataset(train, crop_x_jitter=5, crop_y_jitter=5, angle_jitter=15), {})}


def host_copy(batch):
    return tuple(None if t is None else t.detach().cpu().clone() for t in batch)


def assert_same_batch(got, want, what):
    """(rgb, birdview, loc, cmd, speed): everything bit for bit but loc, which is as in test 3"""
    for k, name in enumerate(("rgb", "birdview", "loc", "cmd", "speed")):
        g, w = got[k], want[k]
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "loc":
            assert float((g.double() - w.double()).abs().max()) <= LOC_TOL, (what, float((g.double() - w.double()).abs().max()))
        else:
            assert torch.equal(g, w), (what, name)


@pytest.mark.parametrize("kind", ["image", "image_batch_aug", "image_medium", "birdview_jitter", "birdview_biased"])
@pytest.mark.parametrize("where", WHERE)
def test_resident_loader_hands_out_device_loaders_batches(env, dataset_dir, where, kind):
    dev, _ = env
    make, kw = _datasets(dataset_dir)[kind]
    host = D.DeviceLoader(make(), 3, 3, dev, seed=5, **kw)
    res = ResidentLoader(make(), 3, 3, dev, seed=5, reserve_gb=0, **kw)
    assert len(res) == len(host) == 3
    n = 0
    for want, got in zip(host, res):
        assert not got[3].is_cuda and got[3].dtype == torch.float32                       # the command stays on the host
        assert all(t is None or t.device.type == dev.type for k, t in enumerate(got) if k != 3)
        assert got[1].shape == (3 * kw.get("batch_aug", 1), 192, 192, 7) and got[1].dtype == torch.uint8
        assert (got[0] is None) == kind.startswith("birdview")
        assert_same_batch(host_copy(got), host_copy(want), (kind, n))
        n += 1
    assert n == 3 and res.images_seen == host.images_seen
    if kind == "image_medium":                                 # the augmentation did something, identically (checked above)
        plain = next(iter(ResidentLoader(make(), 3, 1, dev, seed=5, reserve_gb=0)))
        first = next(iter(ResidentLoader(make(), 3, 1, dev, seed=5, reserve_gb=0, **kw)))
        assert not torch.equal(plain[0], first[0]) and torch.equal(plain[1], first[1])


# ---- 5. state interchange ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["image_medium", "birdview_jitter"])
@pytest.mark.parametrize("direction", ["host_to_resident", "resident_to_host"])
@pytest.mark.parametrize("where", WHERE)
def test_states_move_between_the_two_loader_classes(env, dataset_dir, where, direction, kind):
    """saved after batch 1 of 3 by one class, loaded into a fresh instance of the other: the rest of the pass, the state between the
    passes and a second pass equal the uninterrupted loader's"""
    dev, _ = env
    make, kw = _datasets(dataset_dir)[kind]
    mk_host = lambda seed: D.DeviceLoader(make(), 3, 3, dev, seed=seed, **kw)
    mk_res = lambda seed: ResidentLoader(make(), 3, 3, dev, seed=seed, reserve_gb=0, **kw)
    first, other = (mk_host, mk_res) if direction == "host_to_resident" else (mk_res, mk_host)
    a = first(9)
    it = iter(a)
    host_copy(next(it))
    mid = a.state_dict()
    assert mid["position"] == 1 and set(mid) == {"images_seen", "position", "frames", "rng", "aug"}
    b = other(1234)                                            # (another seed: everything must come from the state)
    b.load_state_dict(mid)
    rest_a, rest_b = [host_copy(x) for x in it], [host_copy(x) for x in b]
    assert len(rest_a) == len(rest_b) == 2
    for k, (x, y) in enumerate(zip(rest_a, rest_b)):
        assert_same_batch(y, x, (direction, kind, "rest", k))
    between = a.state_dict()
    assert between["position"] == 0 and b.state_dict()["images_seen"] == between["images_seen"]
    c = other(77)
    c.load_state_dict(between)
    second_a, second_b, second_c = [host_copy(x) for x in a], [host_copy(x) for x in b], [host_copy(x) for x in c]
    assert len(second_a) == len(second_b) == len(second_c) == 3
    for k in range(3):
        assert_same_batch(second_b[k], second_a[k], (direction, kind, "second pass, continued", k))
        assert_same_batch(second_c[k], second_a[k], (direction, kind, "second pass, restored between passes", k))
    with pytest.raises(ValueError, match="frames"):
        b.load_state_dict(dict(mid, frames=7))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_budget_and_index_refusals(env, dataset_dir, where):
    dev, _ = env
    ds = D.ImageDataset(os.path.join(dataset_dir, "train"))
    ok = ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=lambda: (2 * 10 ** 9, 4 * 10 ** 9))
    need = ok.resident_bytes
    assert need == 30 * (160 * 384 * 3 + 192 * 192 * 7) + 80 * 20 + 30 * 4 + 56 and ok.reserved_bytes == 10 ** 9
    # a reserve larger than the free memory: needed, free and reserved bytes are named, nothing falls back to the host loader
    with pytest.raises(RuntimeError) as e:
        ResidentLoader(ds, 3, 1, dev, reserve_gb=3.0, mem_info=lambda: (2 * 10 ** 9, 4 * 10 ** 9))
    assert all(s in str(e.value) for s in (str(need), "2000000000", "3000000000")), str(e.value)
    with pytest.raises(RuntimeError, match=str(need)):         # exactly one byte short
        ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=lambda: (10 ** 9 + need - 1, 4 * 10 ** 9))
    ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=lambda: (10 ** 9 + need, 4 * 10 ** 9))
    if dev.type == "cuda":                                     # the device's own figure, and the default reserve
        free = torch.cuda.mem_get_info(dev)[0]
        with pytest.raises(RuntimeError, match=str(int(round((free / 1e9 + 1.0) * 1e9)))):
            ResidentLoader(ds, 3, 1, dev, reserve_gb=free / 1e9 + 1.0)
    assert RESERVE_GB == 20
    with pytest.raises(RuntimeError, match="reserved"):
        ResidentLoader(ds, 3, 1, dev, mem_info=lambda: (RESERVE_GB * 10 ** 9 + need - 1, 288 * 10 ** 9))
    # indices are checked on the host before anything is launched
    for bad in ([30], [0, -1], [5, 2, 31]):
        with pytest.raises(RuntimeError, match="outside the 30 resident frames"):
            ok.gather(np.array(bad))
    with pytest.raises(RuntimeError, match="window is fixed"):
        ok.gather(np.array([[0, 0, 1, -10]]))
    bv = ResidentLoader(B.BirdViewDataset(os.path.join(dataset_dir, "train"), angle_jitter=5), 3, 1, dev, reserve_gb=0)
    with pytest.raises(RuntimeError, match="delta_angle 6"):
        bv.gather(np.array([[0, 6, 0, -10]]))
    # the entry point refuses a window outside the source
    src = torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros((1, 4, 8, 4), dtype=torch.uint8, device=dev)
    rc = _lib.get().lbc_dataset_gather_crop_u8(_lib.ptr(src), _lib.ptr(idx), 1, 1, 8, 8, 4, 5, 0, 4, 8, _lib.ptr(out), _lib.stream_for(out))
    assert rc == -1 and "outside" in _lib.get().lbc_last_error().decode()


def test_flags_and_make_loaders(env, dataset_dir):
    """--resident / --resident-reserve-gb become data_args entries only when given, need --dataset_dir, and make_loaders then builds
    ResidentLoaders for both splits, image and bird-view alike; phase 2 does not take the flag"""
    import argparse
    from learningbycheating_amd.training import resume
    from learningbycheating_amd.training.data import make_loaders
    dev, _ = env
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset_dir", default=None)
    resume.add_arguments(parser)
    assert resume.resident_entries(parser.parse_args(["--dataset_dir", "d"])) == {}
    assert resume.resident_entries(parser.parse_args(["--dataset_dir", "d", "--resident"])) == {"resident": True}
    assert resume.resident_entries(parser.parse_args(["--dataset_dir", "d", "--resident", "--resident-reserve-gb", "2.5"])) == {"resident": True, "resident_reserve_gb": 2.5}
    for bad in (["--resident"], ["--dataset_dir", "d", "--resident-reserve-gb", "1"], ["--dataset_dir", "d", "--resident", "--resident-reserve-gb", "-1"]):
        with pytest.raises(SystemExit):
            resume.resident_entries(parser.parse_args(bad))
    from learningbycheating_amd.training import evaluate, train_birdview, train_image_phase0, train_image_phase1, train_image_phase2
    # every script that reads the dataset takes the flag and checks it before it touches the device: with or without a GPU
    for mod, required in ((evaluate, ["--phase", "1", "--model_path", "unused"]), (train_birdview, ["--log_dir", "unused"]),
                          (train_image_phase0, ["--log_dir", "unused"]), (train_image_phase1, ["--log_dir", "unused"])):
        with pytest.raises(SystemExit, match="--dataset_dir"):
            mod.main(required + ["--resident"])
    with pytest.raises(SystemExit) as usage:
        train_image_phase2.main(["--log_dir", "unused", "--resident"])
    assert usage.value.code == 2, "argparse's usage error: phase 2 does not take the flag"
    base = {"dataset_dir": dataset_dir, "batch_size": 3, "n_step": 5, "gap": 5}
    for extra, cls_name in (({}, "ImageDataset"), ({"crop_x_jitter": 5, "crop_y_jitter": 5, "angle_jitter": 5, "cmd_biased": True}, "BiasedBirdViewDataset")):
        host = make_loaders({"data_args": dict(base, **extra), "iters_per_epoch": 200, "synthetic": 0}, dev)
        res = make_loaders({"data_args": dict(base, resident=True, resident_reserve_gb=0.0, **extra), "iters_per_epoch": 200, "synthetic": 0}, dev)
        assert all(type(l) is D.DeviceLoader for l in host) and all(type(l) is ResidentLoader for l in res)
        assert type(res[0].data).__name__ == cls_name and (len(res[0]), len(res[1])) == (len(host[0]), len(host[1])) == (200, 2)
        assert res[0].reserved_bytes == 0
        assert_same_batch(host_copy(next(iter(res[1]))), host_copy(next(iter(host[1]))), cls_name)


# ---- 7. the script -------------------------------------------------------------------------------------------------------------------
@gpu
def test_phase1_script_runs_resident(env, dataset_dir, tmp_path, capsys):
    """train_image_phase1 --dataset_dir D --resident: one short epoch pair, the resident frame and byte counts logged once per split,
    model-1.th written, `resident` in config.json of that run only"""
    from learningbycheating_amd.training import train_image_phase1
    common = ["--dataset_dir", dataset_dir, "--batch_size", "4", "--iters_per_epoch", "2", "--log_iterations", "1", "--augment", "medium",
              "--skip-nonfinite", "--seed", "3"]
    d1, d2 = tmp_path / "resident", tmp_path / "host"
    capsys.readouterr()
    train_image_phase1.main(["--log_dir", str(d1), "--max_epoch", "1", "--resident", "--resident-reserve-gb", "4"] + common)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("ResidentLoader:")]
    nbytes = 30 * (160 * 384 * 3 + 192 * 192 * 7) + 80 * 20 + 30 * 4 + 56
    assert len(lines) == 2 and all("30 frames, %d bytes resident" % nbytes in l for l in lines), lines
    assert (d1 / "model-1.th").exists()
    log = [json.loads(l) for l in open(d1 / "log.jsonl")]
    assert len(log) == 2 and all("val_loss_mean" in r and "train_loss_mean" in r for r in log)
    train_image_phase1.main(["--log_dir", str(d2), "--max_epoch", "0"] + common)
    assert "ResidentLoader" not in capsys.readouterr().out
    c1, c2 = json.loads((d1 / "config.json").read_text()), json.loads((d2 / "config.json").read_text())
    assert c1["data_args"].pop("resident") is True and c1["data_args"].pop("resident_reserve_gb") == 4.0
    assert not any("resident" in k for k in list(c2) + list(c2["data_args"]))
    for c in (c1, c2):
        c.pop("log_dir"), c.pop("max_epoch")
    assert c1 == c2


# ---- 8. offsets past 2^31 and 2^32 ---------------------------------------------------------------------------------------------------
@gpu
def test_frame_offsets_beyond_32_bits(env):
    """6,000 map-sized frames (4.3 GB, only five of them written): frames whose byte offsets pass 2^31 and 2^32 come out as the same
    frames stored at low indices do, through the 16-byte copy, the byte copy and the warp"""
    dev, _ = env
    F, frame = 6000, 320 * 320 * 7
    high = [2996, 3001, 5992, 5999]
    assert high[0] * frame >= 1 << 31 > (high[0] - 1) * frame and high[2] * frame >= 1 << 32 > (high[2] - 1) * frame
    low = [0, 1, 2, 3]
    rng = np.random.RandomState(24)
    frames = rng.randint(0, 256, size=(4, 320, 320, 7)).astype(np.uint8)
    store = torch.empty((F, 320, 320, 7), dtype=torch.uint8, device=dev)
    store[low] = torch.from_numpy(frames).to(dev)
    store[high] = torch.from_numpy(frames).to(dev)
    order = [3, 0, 2, 2, 1]
    for y0, x0, H, W in ((58, 64, 192, 192), (300, 65, 20, 100)):
        lo = gather_crop(dev, store, [low[k] for k in order], 2, y0, x0, H, W)
        hi = gather_crop(dev, store, [high[k] for k in order], 2, y0, x0, H, W)
        assert np.array_equal(hi, lo) and np.array_equal(lo, np.repeat(frames[order][:, y0:y0 + H, x0:x0 + W], 2, axis=0))
    jit = WARP_CASES[:5]
    lo = warp_through_index(dev, store, [(low[k],) + j for k, j in zip(order, jit)], 15, 1)
    hi = warp_through_index(dev, store, [(high[k],) + j for k, j in zip(order, jit)], 15, 1)
    assert np.array_equal(hi, lo) and np.array_equal(lo, warp_in_place(dev, torch.from_numpy(frames[order]).to(dev), jit))
