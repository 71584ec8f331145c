"""numpy twins of the on-policy tick of phase 2 (lbc_rollout_decide / lbc_rollout_stage_u8, include/lbc_hip.h) and a restatement of the
reference's rollout lists (training/train_image_phase2.py:86-149) with ReplayBuffer.add_data (phase2_utils.py:256-265), shared by the
cases of tests/test_online_rollout.py."""
import numpy as np

M32 = 0xFFFFFFFF


def hash_u32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def hash3(seed, a, b):
    """csrc/lbc_hash.hpp hash3 on Python integers"""
    return hash_u32((seed & M32) ^ hash_u32(((a & M32) * 0x9E3779B9 + hash_u32((b + 0x85EBCA6B) & M32)) & M32))


def draw(seed, tick, agent):
    """u of lbc_rollout_decide: exact in double (a 32-bit integer times 2^-32)"""
    return hash3(seed ^ ((tick >> 32) & M32), tick & M32, agent) / 4294967296.0


class DecideState:
    """what lbc_rollout_decide keeps in device memory, as numpy"""

    def __init__(self, n, capacity, tick=0, p_student=0.5, cursor=None, fill=None):
        self.n, self.capacity, self.tick, self.p_student = n, capacity, int(tick), float(p_student)
        self.cursor = np.zeros(n, np.int32) if cursor is None else np.asarray(cursor, np.int32).copy()
        self.dropped = np.zeros(n, np.int32)
        rng = np.random.RandomState(5) if fill is None else fill
        # what lies in the slots before the first tick: anything, so that an untouched slot shows
        self.slot_cmd = rng.randint(-9, -1, size=n * capacity).astype(np.int32)
        self.slot_speed = rng.rand(n * capacity).astype(np.float32) + 100
        self.slot_weight = rng.rand(n * capacity).astype(np.float32) + 100


def np_decide(st, seed, student, teacher, weight, speed, onehot, active=None):
    """one tick on `st` (in place) -> (out (N,16) float64, slot (N,) int32)"""
    n, cap = st.n, st.capacity
    out, slot = np.zeros((n, 16), np.float64), np.full(n, -1, np.int32)
    for a in range(n):
        if active is not None and not active[a]:
            continue
        who = draw(seed, st.tick, a) < st.p_student
        cur = int(st.cursor[a])
        room = 0 <= cur < cap
        if room:
            at = a * cap + cur
            c = 0
            for k in range(4):
                c = k if onehot[a, k] == 1.0 else c
            st.slot_cmd[at], st.slot_speed[at], st.slot_weight[at] = c + 1, speed[a], weight[a]
            slot[a] = at
            st.cursor[a] = cur + 1
        else:
            st.dropped[a] += 1
        out[a, 0:3] = student[a, :3] if who else teacher[a, :3]
        out[a, 3] = 1.0 if who else 0.0
        out[a, 4] = np.float64(weight[a])
        out[a, 5] = st.cursor[a]
        out[a, 6], out[a, 7] = student[a, 7], teacher[a, 7]
        out[a, 8:11], out[a, 11:14] = student[a, :3], teacher[a, :3]
        out[a, 14] = 0.0 if room else 1.0
    st.tick += 1
    return out, slot


def np_stage(rgb, birdview, slot, rgb_stage, birdview_stage):
    """rows of the agents with slot >= 0 -> row slot of the staging arrays (in place)"""
    for a, s in enumerate(slot):
        if s >= 0:
            rgb_stage[s], birdview_stage[s] = rgb[a], birdview[a]


# ---- the reference's lists ------------------------------------------------------------------------------------------------
class ReferenceBuffer:
    """ReplayBuffer.add_data, phase2_utils.py:256-265: append, and beyond the limit pop the lowest weight"""

    def __init__(self, limit):
        self.limit, self.data, self.weights = limit, [], []

    def add_data(self, datum, weight):
        self.data.append(datum)
        self.weights.append(weight)
        if len(self.data) > self.limit:
            idx = int(np.argsort(self.weights)[0])
            self.data.pop(idx)
            self.weights.pop(idx)

    def samples(self):
        """the buffer as a sorted list of (rgb bytes, bird-view bytes, cmd, speed bits, weight bits)"""
        return sorted((d["rgb"], d["birdview"], d["cmd"], d["speed"], np.float32(w).view(np.uint32).item()) for d, w in zip(self.data, self.weights))


def reference_rollout(buffer, observe_tick, episode_length):
    """train_image_phase2.py:86-149 for ONE weather / environment slot.  observe_tick(data_len) -> (datum, weight, ended, collided) drives
    one tick of the current environment episode: it is called while the episode runs, `ended` says that the loop condition `not
    env.is_success() and not env.collided` fails after this tick; a new episode starts with the next call.  -> (ticks, collisions, skipped)"""
    data, ticks, collisions = [], 0, 0
    while len(data) < episode_length:
        while True:                                                        # one environment episode
            datum, weight, ended, collided = observe_tick(len(data))
            ticks += 1
            data.append((datum, weight))
            if len(data) >= episode_length:
                break
            if ended:
                break
        if collided:
            collisions += 1
            data = data[:-5]
    skipped = 0
    for datum, weight in data:
        if not np.isfinite(weight):                                       # (the issue's rule: a non-finite weight is left out and counted)
            skipped += 1
            continue
        buffer.add_data(datum, weight)
    return ticks, collisions, skipped
