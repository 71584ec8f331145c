"""numpy twins of the replay buffer's admission (lbc_replay_admit, include/lbc_hip.h), shared by tests/test_replay_admit.py (the kernel)
and tests/test_phase2_dataset.py (buffer, rollout, script)."""
import numpy as np


def np_key(w):
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(w) & (w >= 0), w, np.float32(-1)).astype(np.float32)


def np_admit(weights, frame, cmd, speed, slot_of_frame, n, cw, cframe, ccmd, cspeed):
    """the semantics of lbc_replay_admit (include/lbc_hip.h) on copies -> (weights, frame, cmd, speed, slot_of_frame, record)"""
    weights, frame, cmd, speed, sof = weights.copy(), frame.copy(), cmd.copy(), speed.copy(), slot_of_frame.copy()
    limit, m = len(weights), len(cw)
    before = set(frame[:n].tolist())
    at = sof[cframe]
    fresh = at >= 0                                                    # 1. refresh
    weights[at[fresh]] = cw[fresh]
    wait = np.nonzero(~fresh)[0]

    def put(slots, cands):
        weights[slots], frame[slots], cmd[slots], speed[slots] = cw[cands], cframe[cands], ccmd[cands], cspeed[cands]
        sof[cframe[cands]] = slots
    room = min(limit - n, len(wait))                                   # 2. append
    put(np.arange(n, n + room), wait[:room])
    n_after, rest = n + room, wait[room:]
    if len(rest):                                                      # 3. compete
        keys = np.concatenate([np_key(weights), np_key(cw[rest])])
        order = np.argsort(-keys, kind="stable")                       # key descending; stored before waiting, lower index first
        stay = np.zeros(len(keys), bool)
        stay[order[:limit]] = True
        evicted = np.nonzero(~stay[:limit])[0]
        survivors = rest[stay[limit:]]
        assert len(evicted) == len(survivors)
        sof[frame[evicted]] = -1
        put(evicted, survivors)
    after = set(frame[:n_after].tolist())
    record = (n_after, int(fresh.sum()), len(after & set(cframe[~fresh].tolist())), len(before - after))
    return weights, frame, cmd, speed, sof, record
