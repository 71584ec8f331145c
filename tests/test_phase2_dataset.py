"""Phase 2 on a recorded dataset: DeviceReplayBuffer(source=ResidentLoader) (training/replay.py), OfflineRollout (training/rollout.py)
and train_image_phase2 --dataset_dir.

The buffer and the rollout's glue run on the CPU emulator and, marked gpu, on the MI355X; the emulator drives the rollout with a stand-in
for the trainer (two fixed functions of the batch in place of the networks -- one emulated eval step of the real pair takes 25 s), the
GPU runs it with the real NativeTrainer and runs the script.  Everything is compared bitwise: frames are copied, admission moves values
(tests/replay_twin.py), and a scoring pass made twice over the same chunks runs the same kernels on the same bytes."""
import json

import numpy as np
import pytest
import torch

from learningbycheating_amd import _lib
from learningbycheating_amd.bird_view.utils.datasets import image_lmdb as D
from learningbycheating_amd.bird_view.utils.datasets.resident import ResidentLoader
from learningbycheating_amd.bird_view.utils.train_utils import one_hot
from learningbycheating_amd.training.replay import DeviceReplayBuffer
from learningbycheating_amd.training.rollout import OfflineRollout, shard_frames
from tests.helpers import WHERE
from tests.replay_twin import np_admit

gpu = pytest.mark.gpu
LIMIT = 16


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("lbc_phase2")
    D.write_synthetic_dataset(str(root), episodes=2, frames=40)
    return str(root)


def make_store(dev, dataset_dir, **kw):
    return ResidentLoader(D.ImageDataset(dataset_dir + "/train"), 4, 0, dev, reserve_gb=0.0, **kw)


def np_one_hot(cmd):
    out = np.zeros((len(cmd), 4), np.float32)
    out[np.arange(len(cmd)), np.clip(np.asarray(cmd).astype(np.int64) - 1, 0, 3)] = 1
    return out


def buffer_arrays(buf):
    """-> (weights, frame, cmd, speed, slot_of_frame, n) on the host"""
    return (buf.weights.cpu().numpy().copy(), buf.frame.cpu().numpy().copy(), buf.cmd.cpu().numpy().copy(), buf.speed.cpu().numpy().copy(),
            buf.slot_of_frame.cpu().numpy().copy(), len(buf))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def admit_checked(buf, frames, cmd, speed, weight, admit=None):
    """buf.admit(...) next to the twin on the buffer's arrays: the record and all five arrays, bit for bit -> the record"""
    before = buffer_arrays(buf)
    cands = (weight.cpu().numpy().astype(np.float32), np.asarray(frames, np.int32), cmd.cpu().numpy().astype(np.int32), speed.cpu().numpy().astype(np.float32))
    rec = (admit or buf.admit)(frames, cmd, speed, weight)
    want = np_admit(*before, *cands)
    assert (rec["n"], rec["refreshed"], rec["admitted"], rec["evicted"]) == want[5]
    n = rec["n"]
    for name, g, w in zip(("weights", "frame", "cmd", "speed"), buffer_arrays(buf)[:4], want[:4]):
        assert np.array_equal(bits(g[:n]), bits(w[:n])), name
    assert np.array_equal(buf.slot_of_frame.cpu().numpy(), want[4]) and len(buf) == n and not buf.normalized
    return rec


def fill(buf, store, rng, counts=(12, 10)):
    """two admissions with small integer weights: 12 frames into the empty buffer, then 10 more of which 3 are stored (16 slots: the second
    one refreshes, appends and competes)"""
    dev, F = buf.device, store.frames
    perm = rng.permutation(F)
    first = perm[:counts[0]]
    second = np.concatenate([first[:3], perm[counts[0]:counts[0] + counts[1] - 3]])[rng.permutation(counts[1])]
    recs = []
    for frames in (first, second):
        cmd = store.cmd_host[torch.from_numpy(frames)].to(torch.int32).to(dev)
        speed = store.gather(frames)[3]
        weight = torch.from_numpy(rng.randint(0, 5, size=len(frames)).astype(np.float32)).to(dev)
        recs.append(admit_checked(buf, frames, cmd, speed, weight))
    return recs


# ---- the buffer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_indexed_buffer_admit_batch_and_highest_k(env, dataset_dir, where):
    """admit against the twin; batch(idx, reps) = the store's own frames, command one-hot and speed of frame[idx] with the fan-out;
    get_highest_k through the indirect gather; the buffer allocates no frame storage"""
    dev, _ = env
    store = make_store(dev, dataset_dir)
    assert store.frames == 30
    buf = DeviceReplayBuffer(dev, buffer_limit=LIMIT, seed=1, source=store)
    assert buf.rgb is store.rgb and buf.birdview is store.birdview and buf.frame.shape == (LIMIT,) and buf.slot_of_frame.shape == (30,)
    recs = fill(buf, store, np.random.RandomState(41))
    assert recs[0] == {"n": 12, "refreshed": 0, "admitted": 12, "evicted": 0}
    assert recs[1]["n"] == LIMIT and recs[1]["refreshed"] == 3 and recs[1]["evicted"] >= 1
    frame = buf.frame.cpu().numpy().astype(np.int64)
    idx = np.array([3, 0, 3, LIMIT - 1])
    for reps in (1, 2):
        rgb, bv, onehot, speed = buf.batch(torch.from_numpy(idx).to(dev), reps)
        f = np.repeat(frame[idx], reps)
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (4 * reps, 160, 384, 3) and tuple(bv.shape) == (4 * reps, 192, 192, 7)
        assert np.array_equal(rgb.cpu().numpy(), store.rgb.cpu().numpy()[f]) and np.array_equal(bv.cpu().numpy(), store.birdview.cpu().numpy()[f])
        assert np.array_equal(onehot.cpu().numpy(), np_one_hot(store.cmd_host.numpy()[f]))
        assert np.array_equal(onehot.cpu().numpy(), one_hot(store.cmd_host[torch.from_numpy(f)]).numpy())
        assert np.array_equal(bits(speed.cpu().numpy()), bits(store.gather(f)[3].cpu().numpy()))
    top, rgb, bv, onehot, speed = buf.get_highest_k(4)
    w = buf.weights[:LIMIT].cpu().numpy()
    assert sorted(w[top.cpu().numpy()].tolist()) == sorted(w.tolist())[-4:]
    assert np.array_equal(rgb.cpu().numpy(), store.rgb.cpu().numpy()[frame[top.cpu().numpy()]])
    assert np.array_equal(bv.cpu().numpy(), store.birdview.cpu().numpy()[frame[top.cpu().numpy()]])


@pytest.mark.parametrize("where", WHERE)
def test_indexed_buffer_state_round_trip(env, dataset_dir, where):
    """state_dict -> load_state_dict into a fresh buffer over the same store: indices only (no frames in the state), slot_of_frame is
    rebuilt, and the next 4 index streams and batches are bitwise equal, in the shuffled epoch and in the weighted one"""
    dev, _ = env
    store = make_store(dev, dataset_dir)
    buf = DeviceReplayBuffer(dev, buffer_limit=LIMIT, seed=1, source=store)
    fill(buf, store, np.random.RandomState(42))
    n = len(buf)
    for normalised in (False, True):
        buf.init_new_weights()
        buf.sample_indices(3)
        if normalised:
            buf.update_weights(torch.arange(n, dtype=torch.int32), torch.arange(n).float() % 5)
            buf.normalize_weights()
            buf.sample_indices(3)
        sd = buf.state_dict(include_frames=True)
        assert "rgb" not in sd and "birdview" not in sd and sd["source_frames"] == 30 and sd["frame"].dtype == torch.int32
        assert sum(v.numel() * v.element_size() for v in sd.values() if torch.is_tensor(v)) < 64 * n
        fresh = DeviceReplayBuffer(dev, buffer_limit=LIMIT, seed=99, source=store)
        fresh.load_state_dict(sd)
        assert len(fresh) == n and fresh.normalized == normalised
        assert torch.equal(fresh.slot_of_frame.cpu(), buf.slot_of_frame.cpu()) and torch.equal(fresh.frame[:n].cpu(), buf.frame[:n].cpu())
        for _ in range(4):
            ia, ib = buf.sample_indices(3), fresh.sample_indices(3)
            assert torch.equal(ia.cpu(), ib.cpu())
            for ta, tb in zip(buf.batch(ia, 2), fresh.batch(ib, 2)):
                assert torch.equal(ta.cpu(), tb.cpu())
    # an admission into both continues equally
    frames = np.array([int(f) for f in range(30) if buf.slot_of_frame[f] < 0][:5])
    args = (torch.ones(5, dtype=torch.int32, device=dev), torch.ones(5, device=dev), torch.full((5,), 9.0, device=dev))
    assert buf.admit(frames, *args) == fresh.admit(frames, *args)
    assert torch.equal(buf.frame.cpu(), fresh.frame.cpu()) and torch.equal(buf.slot_of_frame.cpu(), fresh.slot_of_frame.cpu())


@pytest.mark.parametrize("where", WHERE)
def test_indexed_buffer_refusals(env, dataset_dir, where):
    """a store with a teacher cache, a store with a jittered window, add_batch on an indexed buffer, admit on a storing one, duplicate
    and out-of-range frames, a state for another frame count, a state of the other kind: each raises with its reason, and the buffer
    is unchanged by a refused admit"""
    import types
    dev, _ = env
    cached = make_store(dev, dataset_dir, teacher=lambda bv, speed, cmd: (torch.zeros((bv.shape[0], 5, 2), device=dev), torch.zeros((bv.shape[0], 4, 5, 2), device=dev)))
    with pytest.raises(ValueError, match="teacher cache"):
        DeviceReplayBuffer(dev, buffer_limit=LIMIT, source=cached)
    store = make_store(dev, dataset_dir)
    moving = types.SimpleNamespace(rgb=store.rgb, birdview=store.birdview, teacher_rows=None, whole_map=True, jitter=True, device=dev, frames=30)
    with pytest.raises(ValueError, match="jittered"):
        DeviceReplayBuffer(dev, buffer_limit=LIMIT, source=moving)
    buf = DeviceReplayBuffer(dev, buffer_limit=LIMIT, seed=1, source=store)
    fill(buf, store, np.random.RandomState(43))
    before = buffer_arrays(buf)
    one = lambda m: (torch.ones(m, dtype=torch.int32, device=dev), torch.ones(m, device=dev), torch.ones(m, device=dev))
    with pytest.raises(RuntimeError, match="frame indices"):
        buf.add_batch(store.rgb[:1], store.birdview[:1], torch.tensor([1]), torch.tensor([1.0]), [1.0])
    with pytest.raises(ValueError, match="repeats"):
        buf.admit(np.array([4, 7, 4]), *one(3))
    for bad in ([0, 30], [-1, 2]):
        with pytest.raises(ValueError, match="outside"):
            buf.admit(np.array(bad), *one(2))
    with pytest.raises(ValueError, match="at least one"):
        buf.admit(np.zeros(0, np.int64), *one(0))
    with pytest.raises(ValueError, match="2 frames with"):
        buf.admit(np.array([1, 2]), *one(3))
    for a, b in zip(buffer_arrays(buf), before):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    sd = buf.state_dict()
    with pytest.raises(ValueError, match="29 frames"):
        buf.load_state_dict(dict(sd, source_frames=29))
    plain = DeviceReplayBuffer(dev, buffer_limit=LIMIT, rgb_shape=(4, 4, 3), birdview_shape=(4, 4, 7))
    with pytest.raises(RuntimeError, match="no source"):
        plain.admit(np.array([1]), *one(1))
    with pytest.raises(ValueError, match="frame indices into a source"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="frame indices into a source"):
        buf.load_state_dict(plain.state_dict())
    buf.load_state_dict(sd)


# ---- the rollout -------------------------------------------------------------------------------------------------------------
class StandInTrainer:
    """what OfflineRollout asks of a trainer: batch, cam and step(...) leaving last_pred / last_teacher.  The 'networks' are two fixed
    functions of the batch (heat-map-space waypoints from the frames' means and the speed) -- enough for lbc_phase2_weight to score."""

    def __init__(self, dev, batch=4):
        from learningbycheating_amd.training.native import camera_struct
        self.batch, self.cam, self.dev, self.calls = batch, camera_struct(), dev, []

    def step(self, x, speed, command, birdview=None, update=True, train_mode=True):
        assert not update and not train_mode and x.dtype == torch.uint8 and birdview.dtype == torch.uint8
        n = x.shape[0]
        self.calls.append(n)
        a = x.reshape(n, -1).float().mean(1) / 255 - 0.5
        b = birdview.reshape(n, -1).float().mean(1) / 255
        t = torch.arange(5, dtype=torch.float32, device=x.device)
        branch = command.argmax(1).float()
        pred = torch.stack([(a + 0.05 * branch)[:, None] * (1 + t), 0.3 + 0.1 * t[None] + 0.01 * speed[:, None]], -1)
        teach = torch.stack([(b - 0.05)[:, None] * (1 + t), 0.35 + 0.1 * t[None].expand(n, 5)], -1)
        self.last_pred, self.last_teacher = (pred.contiguous(), None), (teach.contiguous(), None)
        return torch.zeros(n, device=x.device)


def by_hand(store, trainer, frames):
    """the scoring pass spelled out: the same chunks, the same calls -> weights"""
    from learningbycheating_amd.training.train_image_phase2 import phase2_weights
    out = []
    for c0 in range(0, len(frames), trainer.batch):
        chunk = frames[c0:c0 + trainer.batch]
        rgb, bv, _, speed = store.gather(chunk)
        trainer.step(rgb, speed, one_hot(store.cmd_host[torch.from_numpy(chunk)]).to(store.device), birdview=bv, update=False, train_mode=False)
        out.append(phase2_weights(trainer, trainer.last_pred[0], trainer.last_teacher[0]).clone())
    return torch.cat(out)


def test_rollout_windows_partition_the_shard():
    """shard_frames: f = rank (mod world); the windows of one permutation are disjoint and cover the shard; a window that no longer fits
    starts a fresh permutation (a window never holds a frame twice); 0 = the whole shard; the state continues the order"""
    assert shard_frames(30).tolist() == list(range(30))
    assert shard_frames(31, 0, 2).tolist() == list(range(0, 31, 2)) and shard_frames(31, 1, 2).tolist() == list(range(1, 31, 2))
    with pytest.raises(ValueError):
        shard_frames(30, 2, 2)
    import types
    for world, rank, per, windows in ((1, 0, 6, 5), (2, 0, 5, 3), (2, 1, 5, 3), (1, 0, 7, 4), (1, 0, 0, 1), (1, 0, 99, 1)):
        store = types.SimpleNamespace(frames=30)
        buf = types.SimpleNamespace(source=store)
        ro = OfflineRollout(store, None, buf, per, seed=5, rank=rank, world=world)
        shard = set(shard_frames(30, rank, world).tolist())
        assert ro.window == (len(shard) if per in (0, 99) else per)
        for _ in range(2):                                       # two permutations
            seen = []
            for _ in range(windows):
                w = ro.next_window().tolist()
                assert len(w) == ro.window == len(set(w)) and set(w) <= shard
                seen += w
            assert len(set(seen)) == len(seen) and (set(seen) == shard or per == 7)
        twin = OfflineRollout(store, None, buf, per, seed=6, rank=rank, world=world)
        twin.load_state_dict(ro.state_dict())
        for _ in range(windows + 1):
            assert twin.next_window().tolist() == ro.next_window().tolist()
    with pytest.raises(ValueError, match="window"):
        OfflineRollout(store, None, buf, 4).load_state_dict(ro.state_dict())


def check_rollout(dev, store, trainer, unchanged=()):
    """two run()s of 10 frames at batch 4 (a short last chunk) into 16 slots: the weights handed to admit are bitwise those of the same
    calls made by hand, the buffer after each run equals the twin on the read-back weights, `unchanged` tensors keep their bytes"""
    buf = DeviceReplayBuffer(dev, buffer_limit=LIMIT, seed=1, source=store)
    ro = OfflineRollout(store, trainer, buf, 10, seed=3)
    handed = []
    admit = buf.admit

    def spy(frames, cmd, speed, weight):
        handed.append((np.asarray(frames).copy(), cmd.clone(), speed.clone(), weight.clone()))
        return admit_checked(buf, frames, cmd, speed, weight, admit)      # (the twin, on the weights as read back)
    buf.admit = spy
    try:
        frozen = [t.detach().clone() for t in unchanged]
        order = OfflineRollout(store, trainer, buf, 10, seed=3)
        for episode in range(2):
            rec = ro.run()
            frames, cmd, speed, weight = handed[-1]
            assert frames.tolist() == order.next_window().tolist() and rec["frames"] == 10 and rec["n"] == (10, 16)[episode]
            assert np.array_equal(cmd.cpu().numpy(), store.cmd_host.numpy()[frames].astype(np.int32))
            assert np.array_equal(bits(speed.cpu().numpy()), bits(store.gather(frames)[3].cpu().numpy()))
            want = by_hand(store, trainer, frames)
            assert torch.isfinite(weight).all() and np.array_equal(bits(weight.cpu().numpy()), bits(want.cpu().numpy()))
            assert len(set(weight.cpu().tolist())) > 1
        for t, t0 in zip(unchanged, frozen):
            assert torch.equal(t.detach(), t0)
    finally:
        del buf.admit
    return buf


@pytest.mark.parametrize("where", WHERE)
def test_rollout_glue(env, dataset_dir, where):
    """OfflineRollout with the stand-in trainer: chunks of 4, 4, 2; eval-mode, non-updating steps only; weights, buffer and record as
    check_rollout states"""
    dev, _ = env
    store = make_store(dev, dataset_dir)
    trainer = StandInTrainer(dev)
    check_rollout(dev, store, trainer)
    assert trainer.calls[:3] == [4, 4, 2]
    with pytest.raises(ValueError, match="same store"):
        OfflineRollout(store, trainer, DeviceReplayBuffer(dev, buffer_limit=4, source=make_store(dev, dataset_dir)), 4)


# ---- the real networks and the script (GPU) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warm_ckpt(tmp_path_factory):
    """a warm-started student (tests/test_replay_device.py warm_student: an untrained one predicts on the pole of the unprojection)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_replay_device import warm_student
    _lib._inject_for_tests(None)
    path = tmp_path_factory.mktemp("p2d_warm") / "student.th"
    torch.save(warm_student(torch.device("cuda", 0)).state_dict(), str(path))
    return str(path)


@gpu
def test_rollout_with_the_networks(env, dataset_dir, warm_ckpt):
    """the real NativeTrainer at batch 4, fp32: check_rollout, and the student's parameters and BatchNorm running statistics are
    unchanged by run()"""
    from learningbycheating_amd.bird_view.models.birdview import BirdViewPolicyModelSS
    from learningbycheating_amd.bird_view.models.image import ImagePolicyModelSS
    from learningbycheating_amd.training.native import NativeTrainer, camera_struct
    dev, _ = env
    net = ImagePolicyModelSS("resnet34", all_branch=True).to(dev)
    net.load_state_dict(torch.load(warm_ckpt, map_location=dev))
    torch.manual_seed(5)
    teacher = BirdViewPolicyModelSS("resnet18", all_branch=True).to(dev)
    trainer = NativeTrainer(net, teacher, 4, (3, 160, 384), dev, phase=1, camera=camera_struct())
    store = make_store(dev, dataset_dir)
    tensors = list(net.parameters()) + list(net.buffers())
    assert any("running_mean" in k for k, _ in net.named_buffers())
    check_rollout(dev, store, trainer, unchanged=tensors)
    assert net.training


SCRIPT = ["--batch_size", "4", "--precision", "fp32", "--log_iterations", "1", "--replay", "device", "--buffer_limit", "16", "--rollout_frames", "12",
          "--epoch_per_episode", "1", "--seed", "3", "--save_state", "--resident-reserve-gb", "0"]


def run_script(tmp, dataset_dir, warm_ckpt, episodes, extra=()):
    """-> (what main returns, [(buffer arrays before, candidates, record)] per rollout of this run)"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    seen = []
    admit = DeviceReplayBuffer.admit

    def spy(self, frames, cmd, speed, weight):
        before = buffer_arrays(self)
        cands = (weight.cpu().numpy().copy(), np.asarray(frames, np.int32), cmd.cpu().numpy().copy(), speed.cpu().numpy().copy())
        rec = admit(self, frames, cmd, speed, weight)
        seen.append((before, cands, rec))                         # (run() adds "frames" to this record)
        return rec
    DeviceReplayBuffer.admit = spy
    try:
        out = P2.main(["--log_dir", str(tmp), "--dataset_dir", dataset_dir, "--ckpt", warm_ckpt, "--max_episode", str(episodes)] + SCRIPT + list(extra))
    finally:
        DeviceReplayBuffer.admit = admit
    torch.cuda.synchronize()
    return out, seen


@pytest.fixture(scope="module")
def full_run(tmp_path_factory, dataset_dir, warm_ckpt):
    tmp = tmp_path_factory.mktemp("p2d_full")
    return (tmp,) + run_script(tmp, dataset_dir, warm_ckpt, 3)


@gpu
def test_script_trains_from_the_dataset(env, full_run, dataset_dir):
    """three episodes at batch 4: episode 0 fills 12 slots, episode 1 reaches 16 with 8 candidates competing for slots, episode 2 starts a
    fresh permutation and refreshes; the logged counters are the twin's on the weights the rollout handed over; config.json gains the
    new keys"""
    tmp, out, seen = full_run
    assert len(seen) == 3 and (tmp / "model-2.th").exists()
    log = [json.loads(l) for l in open(tmp / "log.jsonl")]
    assert len(log) == 3
    for episode, ((before, cands, rec), line) in enumerate(zip(seen, log)):
        want = np_admit(*before, *cands)[5]
        assert (rec["n"], rec["refreshed"], rec["admitted"], rec["evicted"]) == want and rec["frames"] == 12
        got = tuple(int(line["train_" + k]["mean"]) for k in ("buffer_size", "rollout_refreshed", "rollout_admitted", "rollout_evicted"))
        assert got == want and line["train_rollout_frames"]["mean"] == 12 and line["train_rollout_frames"]["n"] == 1, (episode, got, want)
    print("rollout records:", [s[2] for s in seen])
    assert seen[0][2] == {"n": 12, "refreshed": 0, "admitted": 12, "evicted": 0, "frames": 12}
    # episode 1: 12 new frames for 4 free slots, so 8 compete; who wins is the weights' business (the twin above), the balance is not
    assert seen[1][2]["n"] == 16 and seen[1][2]["refreshed"] == 0 and seen[1][2]["admitted"] - seen[1][2]["evicted"] == 4
    assert seen[2][2]["n"] == 16 and seen[2][2]["refreshed"] >= 1 and seen[2][2]["admitted"] == seen[2][2]["evicted"]
    buf = out["buffer"]
    assert len(buf) == 16 and buf.normalized and torch.isfinite(buf.weights[:16]).all()
    config = json.loads((tmp / "config.json").read_text())
    assert config["dataset_dir"] == dataset_dir and config["rollout_frames"] == 12 and config["buffer_limit"] == 16 and config["resident_reserve_gb"] == 0.0
    state = torch.load(str(tmp / "train_state.th"), map_location="cpu")
    assert "rgb" not in state["buffer"] and state["buffer"]["frame"].numel() == 16 and state["rollout"]["pos"] == 12
    assert sum(v.numel() * v.element_size() for v in state["buffer"].values() if torch.is_tensor(v)) < 64 * 16 + 4 * 5000   # (indices, not 7 MB of frames)


@gpu
def test_script_resume_is_bitwise(env, full_run, dataset_dir, warm_ckpt, tmp_path):
    """stopped after episode 1 and continued with --resume: student, buffer and rollout state bitwise equal to the uninterrupted run"""
    _, ref, ref_seen = full_run
    run_script(tmp_path, dataset_dir, warm_ckpt, 2)
    state = torch.load(str(tmp_path / "train_state.th"), map_location="cpu")
    assert (state["episode"], state["epoch"]) == (1, 0)
    out, seen = run_script(tmp_path, dataset_dir, warm_ckpt, 3, ["--resume"])
    assert len(seen) == 1 and seen[0][2] == ref_seen[2][2]
    sa, sb = ref["net"].state_dict(), out["net"].state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for a, b in zip(buffer_arrays(ref["buffer"]), buffer_arrays(out["buffer"])):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    assert ref["buffer"].draws == out["buffer"].draws and ref["buffer"].normalized == out["buffer"].normalized
    ra, rb = ref["rollout"].state_dict(), out["rollout"].state_dict()
    assert torch.equal(ra.pop("perm"), rb.pop("perm")) and ra["pos"] == rb["pos"] == 12
    rng_a, rng_b = ra.pop("rng"), rb.pop("rng")
    assert torch.equal(rng_a.pop("keys"), rng_b.pop("keys")) and rng_a == rng_b and ra == rb


# ---- flags and config (no device) ------------------------------------------------------------------------------------------------
PARENT_KEYS = {"log_dir", "log_iterations", "epoch_per_episode", "batch_size", "speed_noise", "device", "rank", "world_size", "precision", "model_args",
               "agent_args"}
PARENT_DEVICE_KEYS = {"replay", "augment", "aug_fix_iter", "batch_aug", "lr", "synthetic_frames"}


def test_script_flags_and_config_keys(tmp_path):
    """--dataset_dir with --replay host, and with an explicit --synthetic, exit in build_config with their messages, and so do the
    dataset's flags without it; a run without --dataset_dir builds the config it always built; with it, the new keys and only those"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    base = ["--log_dir", str(tmp_path)]
    for extra, words in ((["--dataset_dir", "D"], ["--dataset_dir", "--replay device"]),
                         (["--dataset_dir", "D", "--replay", "host"], ["--dataset_dir", "--replay device"]),
                         (["--dataset_dir", "D", "--replay", "device", "--synthetic", "64"], ["--dataset_dir", "--synthetic"]),
                         (["--dataset_dir", "D", "--replay", "device", "--buffer_limit", "0"], ["--buffer_limit"]),
                         (["--replay", "device", "--rollout_frames", "8"], ["--rollout_frames", "--dataset_dir"]),
                         (["--replay", "device", "--buffer_limit", "8", "--resident-reserve-gb", "1"], ["--buffer_limit", "--resident-reserve-gb", "--dataset_dir"])):
        with pytest.raises(SystemExit) as e:
            P2.main(base + extra)
        assert all(w in str(e.value) for w in words), (extra, str(e.value))
    build = lambda argv: P2.build_config(P2.parse_arguments(base + argv), 0, 1, torch.device("cuda", 0))
    assert set(build([])) == PARENT_KEYS
    assert set(build(["--synthetic", "64"])) == PARENT_KEYS
    assert set(build(["--replay", "device"])) == PARENT_KEYS | PARENT_DEVICE_KEYS
    parsed = P2.parse_arguments(base)
    P2.build_config(parsed, 0, 1, torch.device("cuda", 0))
    assert parsed.synthetic == 20000 and parsed.rollout_frames == 4000 and parsed.buffer_limit == 100000
    with_data = build(["--replay", "device", "--dataset_dir", "D"])
    assert set(with_data) == PARENT_KEYS | PARENT_DEVICE_KEYS | {"dataset_dir", "rollout_frames", "buffer_limit"}
    assert (with_data["dataset_dir"], with_data["rollout_frames"], with_data["buffer_limit"], with_data["synthetic_frames"]) == ("D", 4000, 100000, False)
    assert build(["--replay", "device", "--dataset_dir", "D", "--resident-reserve-gb", "2"])["resident_reserve_gb"] == 2.0
