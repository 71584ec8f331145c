"""The frozen teacher's waypoints cached per frame of the resident dataset (--cache-teacher): the row-gather kernel
(csrc/dataset.hip lbc_dataset_gather_rows_f32) against numpy, bit for bit; the cache ResidentLoader builds, against the teacher applied
to every frame alone; a loader with a cache against one without, batch by batch, states exchanged; the memory plan; the stale-teacher
check; NativeTrainer.step(teacher_out=...) against the step that runs the teacher itself; the real teacher's cache against its live
forwards; the training script.  Kernel and loader cases run on the CPU emulator and, marked gpu, on the MI355X, where every kernel
launch runs helpers.REPEATS times with bit-identical results."""
import json
import os

import numpy as np
import pytest
import torch

from learningbycheating_amd import WAYPOINT_TOLERANCE, _lib
from learningbycheating_amd.bird_view.utils.datasets import birdview_lmdb as B
from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
from learningbycheating_amd.bird_view.utils.datasets.resident import TEACHER_ROW, ResidentLoader, TeacherWaypoints
from learningbycheating_amd.bird_view.utils.train_utils import one_hot
from tests.helpers import WHERE, repeat

gpu = pytest.mark.gpu
SENTINEL, PAD = 0xA5, 256            # bytes around every gathered output (PAD keeps the output 16-byte aligned)
FRAMES = 30                          # samples of either split of the synthetic dataset: 2 episodes x (40 - gap * n_step)
RGB_BYTES, MAP_BYTES = 160 * 384 * 3, 192 * 192 * 7
TABLES = 80 * 20 + FRAMES * 4 + 56   # measurement table, row_of_sample, one warp entry


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("lbc_teacher_cache")
    D.write_synthetic_dataset(str(root), episodes=2, frames=40, seed=3)
    return str(root)


def bits(t):
    """a float32 tensor's bits as a numpy uint32 array (NaN payloads and the sign of zero compare)"""
    return t.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32)


# ---- 1. the gather kernel ------------------------------------------------------------------------------------------------------------
INDEX_SETS = {1: [5], 3: [4, 2, 2], 5: [5, 3, 3, 1, 0]}      # repeated and descending; first and last frame
SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF],
                    np.uint32)      # quiet / payload / negative / signalling NaN, +-Inf, -0.0, 0.0, the smallest and a negative denormal


def gather_rows(dev, src_bits, idx, reps, stride, offset=0):
    """lbc_dataset_gather_rows_f32 on rows given as uint32 bits -> the output's bits; src and dst start `offset` bytes behind a 16-byte
    boundary, dst between sentinel fences; through helpers.repeat"""
    F, R = src_bits.shape
    sbuf = torch.zeros(F * R * 4 + 16, dtype=torch.uint8, device=dev)
    src = sbuf[offset:offset + F * R * 4].view(torch.int32)
    src.copy_(torch.from_numpy(src_bits.view(np.int32).reshape(-1)).to(dev))
    if stride == 4:                                          # the loader's records: only column 0 may be read
        rec = np.full((len(idx), 4), -123456, np.int32)
        rec[:, 0] = idx
    else:
        rec = np.asarray(idx, np.int32)
    draws = torch.from_numpy(rec).to(dev)
    n = len(idx) * reps * R

    def launch():
        buf = torch.full((n * 4 + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev)
        out = buf[PAD + offset:PAD + offset + n * 4].view(torch.int32)
        assert src.data_ptr() % 16 == offset and out.data_ptr() % 16 == offset
        _lib.check(_lib.get().lbc_dataset_gather_rows_f32(_lib.ptr(src), _lib.ptr(draws), stride, len(idx), reps, R, _lib.ptr(out),
                                                          _lib.stream_for(out)), "dataset_gather_rows_f32")
        return (buf,)
    b = repeat(dev, launch)[0].cpu()
    lo, hi = PAD + offset, PAD + offset + n * 4
    assert bool((b[:lo] == SENTINEL).all()) and bool((b[hi:] == SENTINEL).all()), "the kernel wrote outside its output"
    return b[lo:hi].clone().view(torch.int32).numpy().view(np.uint32).reshape(len(idx) * reps, R)


@pytest.mark.parametrize("where", WHERE)
def test_gather_rows_equals_numpy_indexing(env, where):
    """F = 6 rows of R in {50, 40, 10, 7, 1} floats (the 8-byte path at the cache's own width and at a 16-byte-capable one, odd widths
    on the 4-byte path), B in {1, 3, 5}, reps in {1, 3}, the record (stride 4) and a dense index vector (stride 1), and R = 50 and 7
    with src and dst 4 bytes behind a 16-byte boundary; NaNs with payloads, infinities, -0.0 and denormals among the values; bit for
    bit against src[idx].repeat(reps, 0), fences untouched"""
    dev, _ = env
    rng = np.random.RandomState(31)
    for R in (50, 40, 10, 7, 1):
        src = rng.randint(0, 1 << 32, size=(6, R), dtype=np.uint64).astype(np.uint32)
        flat = src.reshape(-1)
        where_special = rng.choice(flat.size, size=min(flat.size, len(SPECIALS)), replace=False)
        flat[where_special] = SPECIALS[:len(where_special)]
        for nb, idx in INDEX_SETS.items():
            for reps in (1, 3):
                for stride in (4, 1):
                    got = gather_rows(dev, src, idx, reps, stride)
                    assert np.array_equal(got, np.repeat(src[idx], reps, axis=0)), (R, idx, reps, stride)
        if R in (50, 7):
            got = gather_rows(dev, src, INDEX_SETS[5], 3, 4, offset=4)
            assert np.array_equal(got, np.repeat(src[INDEX_SETS[5]], 3, axis=0)), (R, "offset 4")
    lib = _lib.get()
    t = torch.zeros(8, dtype=torch.float32, device=dev)
    i = torch.zeros(2, dtype=torch.int32, device=dev)
    for B_, reps, R, stride in ((0, 1, 4, 1), (1, 0, 4, 1), (1, 1, 0, 1), (1, 1, 4, 0)):
        assert lib.lbc_dataset_gather_rows_f32(_lib.ptr(t), _lib.ptr(i), stride, B_, reps, R, _lib.ptr(t), _lib.stream_for(t)) == -1
    assert lib.lbc_dataset_gather_rows_f32(None, _lib.ptr(i), 1, 1, 1, 4, _lib.ptr(t), _lib.stream_for(t)) == -1


# ---- a cheap teacher -----------------------------------------------------------------------------------------------------------------
def window_teacher(bv, speed, cmd):
    """a deterministic function of the bytes: 50 sums over fixed 12 x 12 windows of one channel each (integers below 2^24: exact in f32
    in any order), mixed with the speed and the command.  Every sample is computed on its own: the result does not depend on the batch"""
    assert bv.dtype == torch.uint8 and tuple(bv.shape[1:]) == (192, 192, 7) and speed.shape == (bv.shape[0],) and cmd.shape == (bv.shape[0], 4)
    n = bv.shape[0]
    sums = torch.stack([bv[:, (37 * k) % 180:(37 * k) % 180 + 12, (53 * k) % 180:(53 * k) % 180 + 12, k % 7].to(torch.int32).sum(dim=(1, 2))
                        for k in range(TEACHER_ROW)], dim=1).to(torch.float32)
    weight = torch.arange(1, TEACHER_ROW + 1, dtype=torch.float32, device=bv.device)
    mix = sums / 1024.0 + speed[:, None] * weight + cmd.argmax(dim=1).to(torch.float32)[:, None] * 0.125
    return mix[:, 40:].reshape(n, 5, 2), mix[:, :40].reshape(n, 4, 5, 2)


class CountingTeacher:
    def __init__(self):
        self.batches = []

    def __call__(self, bv, speed, cmd):
        self.batches.append(int(bv.shape[0]))
        return window_teacher(bv, speed, cmd)


def frame_alone(ds, i, dev):
    """the teacher's three inputs of dataset frame i from ImageDataset.raw(): the fixed window, the speed, the one-hot command"""
    _, bv, _, cmd, speed = ds.raw(i)
    window = np.ascontiguousarray(bv[D.CROP_Y0:D.CROP_Y0 + 192, D.CROP_X0:D.CROP_X0 + 192])
    return (torch.from_numpy(window)[None].to(dev), torch.tensor([speed], dtype=torch.float32).to(dev),
            one_hot(torch.tensor([float(cmd)])).to(dev))


def row_of(sel, every):
    return torch.cat([every.reshape(every.shape[0], 40), sel.reshape(sel.shape[0], 10)], dim=1)


# ---- 2. the cache's contents ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("teacher_batch", [7, 1])
@pytest.mark.parametrize("where", WHERE)
def test_cache_holds_the_teacher_of_every_frame(env, dataset_dir, capsys, where, teacher_batch):
    """teacher_rows[i] = (all, sel) of the callable on frame i alone, for every i; chunks of 7 (the last one holds 2 frames) and of 1, in
    dataset order; the bird-view frames are not resident, and the constructor's line names the cache's bytes and its build time"""
    dev, _ = env
    ds = D.ImageDataset(os.path.join(dataset_dir, "train"))
    teacher = CountingTeacher()
    capsys.readouterr()
    ld = ResidentLoader(ds, 3, 1, dev, reserve_gb=0, teacher=teacher, teacher_batch=teacher_batch)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("ResidentLoader:")]
    assert len(line) == 1 and "teacher cache %d bytes" % (FRAMES * 200) in line[0] and "built in" in line[0], line
    assert teacher.batches == [teacher_batch] * (FRAMES // teacher_batch) + ([FRAMES % teacher_batch] if FRAMES % teacher_batch else [])
    assert ld.birdview is None and ld.build_seconds > 0 and ld.cache_bytes == FRAMES * 200
    assert ld.teacher_rows.shape == (FRAMES, TEACHER_ROW) and ld.teacher_rows.dtype == torch.float32 and ld.teacher_rows.device.type == dev.type
    assert ld.resident_bytes == FRAMES * (RGB_BYTES + 200) + TABLES
    got = bits(ld.teacher_rows)
    for i in range(FRAMES):
        want = bits(row_of(*window_teacher(*frame_alone(ds, i, dev))))[0]
        assert np.array_equal(got[i], want), i
    assert len(np.unique(got, axis=0)) == FRAMES              # (the rows tell the frames apart)
    # gather() hands the rows out in the bird-view's position, through the record and through plain indices
    idx = np.array([29, 0, 7, 7])
    _, tw, _, _ = ld.gather(idx, reps=2)
    assert isinstance(tw, TeacherWaypoints) and tw.sel.shape == (8, 5, 2) and tw.all.shape == (8, 4, 5, 2)
    assert np.array_equal(bits(row_of(tw.sel, tw.all)), np.repeat(got[idx], 2, axis=0))
    with pytest.raises(RuntimeError, match="outside the 30 resident frames"):
        ld.gather(np.array([30]))


# ---- 3. a loader with a cache against one without ---------------------------------------------------------------------------------------
def host_copy(batch):
    return tuple(None if t is None else (TeacherWaypoints(*(x.detach().cpu().clone() for x in t)) if isinstance(t, TeacherWaypoints)
                                         else t.detach().cpu().clone()) for t in batch)


def same_state(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same_state(a[k], b[k]) for k in a)
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


def assert_same_but_slot_1(cached, plain, what):
    """rgb, loc, cmd and speed bit for bit; slot 1 of the cached batch = the callable on the plain batch's bird-view, speed and command"""
    for k, name in ((0, "rgb"), (2, "loc"), (3, "cmd"), (4, "speed")):
        assert cached[k].dtype == plain[k].dtype and torch.equal(cached[k], plain[k]), (what, name)
    assert np.array_equal(bits(cached[2]), bits(plain[2])) and np.array_equal(bits(cached[4]), bits(plain[4])), what
    assert isinstance(cached[1], TeacherWaypoints) and cached[1].sel.dtype == cached[1].all.dtype == torch.float32
    sel, every = window_teacher(plain[1], plain[4], one_hot(plain[3]))
    assert cached[1].sel.shape == sel.shape and cached[1].all.shape == every.shape, what
    assert np.array_equal(bits(cached[1].sel), bits(sel)) and np.array_equal(bits(cached[1].all), bits(every)), what


@pytest.mark.parametrize("batch_aug", [1, 3])
@pytest.mark.parametrize("where", WHERE)
def test_cached_loader_hands_out_the_plain_loaders_batches(env, dataset_dir, where, batch_aug):
    """same seed, augmentation on, two passes of three batches: everything but slot 1 is equal bit for bit, slot 1 holds the teacher of
    the other loader's bird-view batch (every frame batch_aug times); a state saved by either loader continues in the other"""
    dev, _ = env
    train = os.path.join(dataset_dir, "train")
    make = lambda: D.ImageDataset(train, augment_strategy="medium", batch_aug=batch_aug)
    kw = dict(augment="medium", batch_aug=batch_aug, reserve_gb=0)
    plain = ResidentLoader(make(), 3, 3, dev, seed=5, **kw)
    cached = ResidentLoader(make(), 3, 3, dev, seed=5, teacher=window_teacher, teacher_batch=4, **kw)
    for p in range(2):
        n = 0
        for got, want in zip(cached, plain):
            assert all(t.device.type == dev.type for t in (got[0], got[1].sel, got[1].all, got[2], got[4])) and not got[3].is_cuda
            assert got[1].sel.shape == (3 * batch_aug, 5, 2) and got[1].all.shape == (3 * batch_aug, 4, 5, 2)
            assert_same_but_slot_1(host_copy(got), host_copy(want), (p, n))
            n += 1
        assert n == 3 and cached.images_seen == plain.images_seen
    assert same_state(cached.state_dict(), plain.state_dict())
    # states: saved after batch 1 of a pass by one kind of loader, loaded into a fresh loader of the other kind built with another seed
    for first_cached in (True, False):
        mk = lambda with_cache, seed: ResidentLoader(make(), 3, 3, dev, seed=seed, teacher=window_teacher if with_cache else None, **kw)
        a, ref = mk(first_cached, 9), mk(not first_cached, 9)
        it, it_ref = iter(a), iter(ref)
        next(it), next(it_ref)
        mid = a.state_dict()
        assert mid["position"] == 1 and set(mid) == {"images_seen", "position", "frames", "rng", "aug"}
        b = mk(not first_cached, 1234)
        b.load_state_dict(mid)
        rest_b, rest_ref, rest_a = [host_copy(x) for x in b], [host_copy(x) for x in it_ref], [host_copy(x) for x in it]
        assert len(rest_b) == len(rest_ref) == len(rest_a) == 2
        for k in range(2):                                   # b continues a's pass: equal to the uninterrupted loader of b's own kind
            c, pl = (rest_a[k], rest_b[k]) if first_cached else (rest_b[k], rest_a[k])
            assert_same_but_slot_1(c, pl, (first_cached, k))
            for s in (0, 2, 3, 4):
                assert torch.equal(rest_b[k][s], rest_ref[k][s]), (first_cached, k, s)
        assert same_state(b.state_dict(), a.state_dict()) and same_state(b.state_dict(), ref.state_dict())


# ---- 4. the memory plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_memory_plan_counts_the_cache_instead_of_the_maps(env, dataset_dir, where):
    """F x 184,320 + F x 200 bytes plus the tables stay; while the cache is built one chunk of teacher_batch maps (and, for a policy
    model, its engine's workspace -- none for a callable) stands beside them, and that peak is what must fit"""
    dev, _ = env
    ds = D.ImageDataset(os.path.join(dataset_dir, "train"))
    G = 10 ** 9
    uncached = FRAMES * (RGB_BYTES + MAP_BYTES) + TABLES
    steady = FRAMES * (RGB_BYTES + 200) + TABLES
    peak = steady + 3 * MAP_BYTES
    assert peak < uncached
    info = lambda free: (lambda: (free, 4 * G))
    ok = ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=info(G + peak), teacher=window_teacher, teacher_batch=3)
    assert (ok.resident_bytes, ok.cache_bytes, ok.build_bytes, ok.peak_bytes, ok.reserved_bytes) == (steady, FRAMES * 200, 3 * MAP_BYTES, peak, G)
    with pytest.raises(RuntimeError, match=str(uncached)):     # the same free memory does not hold the dataset with its maps
        ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=info(G + peak))
    with pytest.raises(RuntimeError) as e:                     # one byte below the cached loader's own sum
        ResidentLoader(ds, 3, 1, dev, reserve_gb=1.0, mem_info=info(G + peak - 1), teacher=window_teacher, teacher_batch=3)
    assert all(s in str(e.value) for s in (str(steady), str(FRAMES * 200), str(3 * MAP_BYTES), str(peak), str(G + peak - 1), str(G))), str(e.value)
    # a larger chunk raises the peak, not the steady state; a chunk never holds more than the dataset
    big = ResidentLoader(ds, 3, 1, dev, reserve_gb=0, mem_info=info(2 * uncached), teacher=window_teacher, teacher_batch=100)
    assert big.resident_bytes == steady and big.peak_bytes == steady + FRAMES * MAP_BYTES
    without = ResidentLoader(ds, 3, 1, dev, reserve_gb=0, mem_info=info(uncached))
    assert without.resident_bytes == without.peak_bytes == uncached and without.cache_bytes == 0 and without.teacher_rows is None
    # a window that moves per draw is refused, and so is a chunk of no frames
    jittered = B.BirdViewDataset(os.path.join(dataset_dir, "train"), crop_x_jitter=5, crop_y_jitter=5, angle_jitter=15)
    with pytest.raises(ValueError, match="not a function of the frame index"):
        ResidentLoader(jittered, 3, 1, dev, reserve_gb=0, teacher=window_teacher)
    with pytest.raises(ValueError, match="teacher_batch"):
        ResidentLoader(ds, 3, 1, dev, reserve_gb=0, teacher=window_teacher, teacher_batch=0)


# ---- 5. a teacher written after the build -----------------------------------------------------------------------------------------------
class ModuleTeacher(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.ones(1))
        self.register_buffer("shift", torch.zeros(1))

    def forward(self, bv, speed, cmd):
        sel, every = window_teacher(bv, speed, cmd)
        return sel * self.gain + self.shift, every * self.gain + self.shift


@pytest.mark.parametrize("where", WHERE)
def test_teacher_written_in_place_makes_the_next_pass_raise(env, dataset_dir, where):
    dev, _ = env
    ds = D.ImageDataset(os.path.join(dataset_dir, "train"))
    teacher = ModuleTeacher().to(dev)
    ld = ResidentLoader(ds, 3, 2, dev, reserve_gb=0, teacher=teacher, teacher_batch=8)
    assert len(list(ld)) == 2 and len(list(ld)) == 2          # untouched: pass after pass
    with torch.no_grad():
        teacher.gain.mul_(2.0)
    with pytest.raises(RuntimeError, match="teacher cache is stale"):
        next(iter(ld))
    ld2 = ResidentLoader(ds, 3, 2, dev, reserve_gb=0, teacher=teacher, teacher_batch=8)     # built again: the new teacher's rows
    assert np.array_equal(bits(ld2.teacher_rows), bits(ld.teacher_rows * 2.0))
    with torch.no_grad():
        teacher.shift.add_(1.0)                                # a buffer counts too
    with pytest.raises(RuntimeError, match="teacher cache is stale"):
        next(iter(ld2))


# ---- 6. the trainer ----------------------------------------------------------------------------------------------------------------------
def small_model(kind, dev, seed):
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS, ImagePolicyModelSS
    torch.manual_seed(seed)
    if kind == "image":
        return ImagePolicyModelSS("resnet18", all_branch=True, input_hw=(32, 64)).to(dev)
    return BirdViewPolicyModelSS("resnet18", all_branch=True, input_hw=(64, 64)).to(dev)


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("where", WHERE)
def test_step_with_given_teacher_waypoints_equals_the_step_that_runs_the_teacher(env, where, phase):
    """ResNet-18 at 32 x 64 frames / 64 x 64 maps (tests/test_step.py's small shapes), N = 2, two steps: a trainer that runs its teacher
    (birdview=) and a trainer built with teacher=None that is handed clones of the first one's last_teacher (teacher_out=) give the same
    per-sample loss and the same student parameters and buffers, bit for bit; the refusals"""
    from learningbycheating_amd.training.native import NativeTrainer
    from oracle import lbc_oracle as O
    from oracle.make_golden import seeded_inputs
    dev, _ = env
    n = 2
    student_a, teacher = small_model("image", dev, 61), small_model("birdview", dev, 62)
    x, speed, cmd = seeded_inputs("image", n, 63, 32, 64)
    x, speed, onehot = x.contiguous().to(dev), speed.to(dev), O.one_hot(cmd).to(dev)
    bv = seeded_inputs("birdview", n, 64, 64, 64)[0].to(dev)
    # (a few L1 steps towards targets below the horizon, as tests/test_step.py: the phase-1 loss has a 1 / y pole on the horizon row)
    g = torch.Generator().manual_seed(65)
    tgt = torch.rand((n, 4, 5, 2), generator=g)
    tgt[..., 0], tgt[..., 1] = tgt[..., 0] * 1.2 - 0.6, tgt[..., 1] * 0.5 + 0.3
    warm = NativeTrainer(student_a, None, n, (3, 32, 64), dev, phase="l1_all", lr=1e-3)
    for _ in range(3):
        warm.step(x, speed, onehot, target=tgt.to(dev))
    del warm
    student_b = small_model("image", dev, 99)
    student_b.load_state_dict(student_a.state_dict())
    tr_a = NativeTrainer(student_a, teacher, n, (3, 32, 64), dev, phase=phase, lr=1e-4, teacher_shape=(7, 64, 64))
    tr_b = NativeTrainer(student_b, None, n, (3, 32, 64), dev, phase=phase, lr=1e-4)
    assert tr_b.teng is None and tr_b.side is None and tr_b.teacher is None
    for t in range(2):
        loss_a = tr_a.step(x, speed, onehot, birdview=bv).clone()
        given = tuple(w.clone() for w in tr_a.last_teacher)
        handed = given
        if t == 1:        # as a loader's cache hands them out: views of (n,50) rows, row pitch 50 floats; the step packs what its loss reads
            rows = row_of(*given)
            handed = TeacherWaypoints(rows[:, 40:].unflatten(1, (5, 2)), rows[:, :40].unflatten(1, (4, 5, 2)))
            assert not handed.all.is_contiguous() and not handed.sel.is_contiguous()
        loss_b = tr_b.step(x, speed, onehot, teacher_out=handed).clone()
        assert bool(torch.isfinite(loss_a).all()) and np.array_equal(bits(loss_a), bits(loss_b)), (t, loss_a, loss_b)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(tr_b.last_teacher, given))
    sa, sb = student_a.state_dict(), student_b.state_dict()
    assert list(sa) == list(sb) and tr_a.opt.step_count == tr_b.opt.step_count == 2
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), k
    # refusals, each before anything is launched: Adam's count and the parameters stay
    before = {k: v.detach().cpu().clone() for k, v in student_b.state_dict().items()}
    sel, every = given
    with pytest.raises(ValueError, match="built without a teacher"):
        tr_b.step(x, speed, onehot)
    with pytest.raises(ValueError, match="built without a teacher"):
        tr_b.step(x, speed, onehot, birdview=bv)
    for tr in (tr_a, tr_b):
        with pytest.raises(ValueError, match="together"):
            tr.step(x, speed, onehot, birdview=bv, teacher_out=given)
        for bad in ((sel[:1], every), (sel, every[:1]), (every, sel), (sel.double(), every), (sel, every.reshape(n, 40)), (sel,), sel,
                    (sel.cpu().numpy(), every)):
            with pytest.raises(ValueError, match="teacher_out"):
                tr.step(x, speed, onehot, teacher_out=bad)
    if dev.type == "cuda":
        with pytest.raises(ValueError, match="teacher_out.sel"):
            tr_b.step(x, speed, onehot, teacher_out=(sel.cpu(), every))
    assert tr_b.opt.step_count == 2 and all(torch.equal(v.cpu(), before[k]) for k, v in student_b.state_dict().items())
    # a trainer with a teacher engine takes given waypoints too, and launches no teacher forward for them
    forwards = tr_a.teng.generation
    loss = tr_a.step(x, speed, onehot, teacher_out=given, update=False).clone()
    assert tr_a.teng.generation == forwards
    assert np.array_equal(bits(loss), bits(tr_b.step(x, speed, onehot, teacher_out=given, update=False)))


def test_flags_and_make_loaders_with_a_cache(env, dataset_dir):
    """--cache-teacher becomes a data_args entry only when given, needs --resident, is refused by the script that trains the teacher and
    unknown to phase 2; make_loaders then builds both splits with a cache"""
    import argparse
    from learningbycheating_amd.training import evaluate, resume, train_birdview, train_image_phase2
    from learningbycheating_amd.training.data import make_loaders
    dev, _ = env
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset_dir", default=None)
    resume.add_arguments(parser)
    assert resume.resident_entries(parser.parse_args(["--dataset_dir", "d", "--resident"])) == {"resident": True}
    assert resume.resident_entries(parser.parse_args(["--dataset_dir", "d", "--resident", "--cache-teacher"])) == {"resident": True, "cache_teacher": True}
    for bad in (["--dataset_dir", "d", "--cache-teacher"], ["--cache-teacher"]):
        with pytest.raises(SystemExit, match="--cache-teacher needs --resident"):
            resume.resident_entries(parser.parse_args(bad))
    with pytest.raises(SystemExit, match="trains the teacher itself"):
        resume.resident_entries(parser.parse_args(["--dataset_dir", "d", "--resident", "--cache-teacher"]), teacher=False)
    with pytest.raises(SystemExit, match="trains the teacher itself"):
        train_birdview.main(["--log_dir", "unused", "--dataset_dir", dataset_dir, "--resident", "--cache-teacher"])
    with pytest.raises(SystemExit, match="trains the teacher itself"):
        evaluate.main(["--phase", "birdview", "--model_path", "unused", "--dataset_dir", dataset_dir, "--resident", "--cache-teacher"])
    with pytest.raises(SystemExit):                            # (argparse: phase 2 has no such flag)
        train_image_phase2.main(["--log_dir", "unused", "--cache-teacher"])
    base = {"dataset_dir": dataset_dir, "batch_size": 3, "n_step": 5, "gap": 5, "resident": True, "resident_reserve_gb": 0.0}
    config = {"data_args": dict(base, cache_teacher=True), "iters_per_epoch": 200, "synthetic": 0}
    train, val = make_loaders(config, dev, teacher=window_teacher)
    plain_val = make_loaders({"data_args": base, "iters_per_epoch": 200, "synthetic": 0}, dev, teacher=window_teacher)[1]
    assert all(type(l) is ResidentLoader and l.teacher_rows.shape == (FRAMES, TEACHER_ROW) and l.birdview is None for l in (train, val))
    assert plain_val.teacher_rows is None and resume.teacher_for_trainer(config, "t") is None
    assert resume.teacher_for_trainer({"data_args": base}, "t") == "t"
    assert_same_but_slot_1(host_copy(next(iter(val))), host_copy(next(iter(plain_val))), "val")
    bv = next(iter(plain_val))[1]
    assert resume.teacher_arguments(bv) == {"birdview": bv} and set(resume.teacher_arguments(next(iter(val))[1])) == {"teacher_out"}
    with pytest.raises(ValueError, match="cache_teacher"):
        make_loaders(config, dev)


# ---- 7. the real teacher ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cache_of_the_real_teacher_equals_its_live_forwards(env, dataset_dir, precision):
    """ResNet-18 at 7 x 192 x 192 over the 30 synthetic frames, cache built at batch 4 (the last chunk holds 2 frames).
    (a) live eval-mode forwards of a frozen engine over the same chunks in the same order: the cached rows bit for bit;
    (b) a live forward over a shuffled batch with repeated frames, and forwards at batch 3: within WAYPOINT_TOLERANCE[precision] of the
    cached rows (the declared bar between two correct evaluations; samples do not mix in an eval-mode forward, so zero is expected --
    measured on the MI355X: 0.0 in fp32 and in bf16, both cases)"""
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS
    from oracle import lbc_oracle as O
    dev, _ = env
    ds = D.ImageDataset(os.path.join(dataset_dir, "train"))
    teacher = BirdViewPolicyModelSS("resnet18", all_branch=True)
    teacher.load_state_dict(O.make_state_dict("birdview", "resnet18", 7))
    teacher.precision = precision
    teacher.to(dev).eval()
    plain = ResidentLoader(ds, 4, 1, dev, reserve_gb=0)
    cached = ResidentLoader(ds, 4, 1, dev, reserve_gb=0, teacher=teacher, teacher_batch=4)
    assert cached.build_bytes > 4 * MAP_BYTES and cached.peak_bytes == cached.resident_bytes + cached.build_bytes      # (the engine's workspace counts)
    rows = cached.teacher_rows
    assert bool(torch.isfinite(rows).all()) and len(np.unique(bits(rows), axis=0)) == FRAMES
    eng = teacher.engine((4, 7, 192, 192), dev, max_batch=4, with_grads=False)
    eng.set_frozen(True)

    def live(idx):
        idx = np.asarray(idx)
        _, bv, _, speed = plain.gather(idx)
        cmd = one_hot(plain.cmd_host[torch.from_numpy(idx.astype(np.int64))]).to(dev)
        return row_of(*eng.forward(bv, speed, cmd, False))

    for f0 in range(0, FRAMES, 4):                               # (a)
        idx = np.arange(f0, min(f0 + 4, FRAMES))
        assert np.array_equal(bits(live(idx)), bits(rows[f0:f0 + len(idx)])), (precision, f0)
    worst = {}
    shuffled = [np.array([29, 3, 3, 0]), np.array([17, 17, 17, 5])]   # (b)
    worst["shuffled batch, repeated frames"] = max(float((live(i) - rows[torch.from_numpy(i).to(dev)]).abs().max()) for i in shuffled)
    worst["batch 3"] = max(float((live(np.arange(f0, f0 + 3)) - rows[f0:f0 + 3]).abs().max()) for f0 in range(0, FRAMES, 3))
    print("teacher cache, %s: max |live - cached| = %s (tolerance %g)" % (precision, json.dumps(worst), WAYPOINT_TOLERANCE[precision]))
    assert max(worst.values()) <= WAYPOINT_TOLERANCE[precision], worst
    # the loader's batches carry these rows, and the trainer-facing tuple has the forward's shapes
    idx = np.array([29, 3, 3, 0])
    _, tw, _, _ = cached.gather(idx, reps=2)
    assert np.array_equal(bits(row_of(tw.sel, tw.all)), np.repeat(bits(rows)[idx], 2, axis=0))
    # the teacher's parameters were not touched by the build, and a write after it is noticed
    with torch.no_grad():
        next(teacher.parameters()).mul_(1.0)
    with pytest.raises(RuntimeError, match="teacher cache is stale"):
        next(iter(cached))


# ---- 8. the scripts ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_phase1_script_runs_with_a_teacher_cache(env, dataset_dir, tmp_path, capsys):
    """train_image_phase1 --dataset_dir D --resident --cache-teacher --val-metrics: the dry-run epoch and one training epoch; both splits
    report their cache, no bird-view frames are resident, model-1.th is written, the epoch record holds a finite val_ade, and
    `cache_teacher` appears in config.json of that run only"""
    from learningbycheating_amd.training import train_image_phase1
    common = ["--dataset_dir", dataset_dir, "--batch_size", "4", "--iters_per_epoch", "2", "--log_iterations", "1", "--augment", "medium",
              "--skip-nonfinite", "--seed", "3"]
    d1, d2 = tmp_path / "cached", tmp_path / "host"
    capsys.readouterr()
    train_image_phase1.main(["--log_dir", str(d1), "--max_epoch", "1", "--resident", "--resident-reserve-gb", "4", "--cache-teacher", "--val-metrics"]
                            + common)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("ResidentLoader:")]
    nbytes = FRAMES * (RGB_BYTES + 200) + TABLES
    assert len(lines) == 2 and all("30 frames, %d bytes resident" % nbytes in l and "teacher cache 6000 bytes" in l for l in lines), lines
    assert (d1 / "model-1.th").exists()
    log = [json.loads(l) for l in open(d1 / "log.jsonl")]
    assert len(log) == 2 and all("val_loss_mean" in r and "train_loss_mean" in r for r in log)
    assert all(r["val_ade"]["n"] == 1 and np.isfinite(r["val_ade"]["mean"]) and r["val_ade"]["mean"] > 0 for r in log), log      # (metres)
    # the same run with the teacher's forward in every step: the cached rows are that forward's own (test 7), so the records agree
    d3 = tmp_path / "live"
    train_image_phase1.main(["--log_dir", str(d3), "--max_epoch", "1", "--resident", "--resident-reserve-gb", "4", "--val-metrics"] + common)
    capsys.readouterr()
    live = [json.loads(l) for l in open(d3 / "log.jsonl")]
    for r, w in zip(log, live):
        for k in ("val_loss_mean", "val_ade", "val_fde", "train_loss_mean"):
            assert r[k]["mean"] == w[k]["mean"], (k, r[k], w[k])
    train_image_phase1.main(["--log_dir", str(d2), "--max_epoch", "0"] + common)
    assert "ResidentLoader" not in capsys.readouterr().out
    c1, c2 = json.loads((d1 / "config.json").read_text()), json.loads((d2 / "config.json").read_text())
    assert c1["data_args"].pop("resident") is True and c1["data_args"].pop("resident_reserve_gb") == 4.0 and c1["data_args"].pop("cache_teacher") is True
    assert c1.pop("val_metrics") is True
    assert not any("cache" in k or "resident" in k for k in list(c2) + list(c2["data_args"]))
    for c in (c1, c2):
        c.pop("log_dir"), c.pop("max_epoch")
    assert c1 == c2
    from learningbycheating_amd.training import train_birdview
    with pytest.raises(SystemExit, match="trains the teacher itself"):
        train_birdview.main(["--log_dir", str(tmp_path / "bv"), "--dataset_dir", dataset_dir, "--resident", "--cache-teacher"])
    with pytest.raises(SystemExit, match="speed_noise"):
        train_image_phase1.main(["--log_dir", str(tmp_path / "noise"), "--resident", "--cache-teacher", "--speed_noise", "0.1"] + common)
