"""Generator of tests/golden/agent_controls.npz: what the REAL reference agents answer, recorded on a CPU.

Runs only where the reference tree is present (oracle/ref_shim.py).  The reference's ImageAgent.run_step / BirdViewAgent.run_step
(bird_view/models/image.py, birdview.py, with controller.py and common.py behind them) are driven unchanged; what is stood in for is
what they import and cannot have here -- torchvision / carla / cv2 through oracle.ref_shim's stubs, a carla.VehicleControl that is a
plain attribute bag, a ToTensor that ignores the frame -- and the network: a stub module that returns the waypoints of the tick.

Per kind 16 episodes of 35 ticks (longer than both PID windows: the rings wrap), inputs from tests/test_agent_control.py
draw_episodes.  Recorded per tick: the float32 waypoints, the measured speed, the command, the reference's steer / throttle / brake /
target_speed / target, and the conditioning |det| / (Suu Svv) of ITS circle fit (taken from the points it hands to ls_circle).
Asserted on every tick: conditioning >= 1e-2, |target_speed - threshold| >= 1e-3; per kind: both sides of the threshold occur.
The test's numpy twin runs over the same inputs; its largest deviation from the reference goes into twin_max_dev_<kind>.
The file holds recorded inputs and results only.

    python tests/golden/make_agent_fixture.py        # rewrites tests/golden/agent_controls.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPISODES, TICKS = 16, 35
SEEDS = {"image": 20240, "birdview": 20241}
SLOW = {"image": (), "birdview": (2, 7, 11)}          # bird-view episodes that slow down to 0.2 m/s
THRESHOLD = {"image": 2.0, "birdview": 1.0}
CAMERA_ARGS = {"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": 4.0}      # (the reference's default dict says 'x' and fails)


class _VehicleControl:
    pass


class _PresetWaypoints(torch.nn.Module):
    """stands in for the policy network: answers the waypoints set for this tick, float32 (1,5,2) as the network does"""
    all_branch = False

    def forward(self, image, speed, command):
        return torch.from_numpy(self.next)[None]


def _reference_agents():
    from oracle import ref_shim
    ref_shim._install_stubs()
    sys.modules["carla"].VehicleControl = _VehicleControl
    with ref_shim._cuda_noop():
        import models.birdview as ref_birdview
        import models.image as ref_image
    return ref_image, ref_birdview


def _conditioning(points):
    xs, ys = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    us, vs = xs - xs.mean(), ys - ys.mean()
    Suu, Suv, Svv = (us * us).sum(), (us * vs).sum(), (vs * vs).sum()
    return abs(Suu * Svv - Suv * Suv) / (Suu * Svv)


def _run_kind(kind, module, twin_mod):
    pred, speed, command = twin_mod.draw_episodes(kind, EPISODES, TICKS, SEEDS[kind], slow=SLOW[kind])
    ref = np.empty((EPISODES, TICKS, 6), dtype=np.float64)
    cond = np.empty((EPISODES, TICKS), dtype=np.float64)
    twin_dev = 0.0
    seen = []
    real_ls_circle = module.ls_circle

    def recording_ls_circle(points):
        seen.append(np.array(points, dtype=np.float64))
        return real_ls_circle(points)
    module.ls_circle = recording_ls_circle
    try:
        for e in range(EPISODES):
            model = _PresetWaypoints()
            agent = module.ImageAgent(model=model, camera_args=dict(CAMERA_ARGS)) if kind == "image" else module.BirdViewAgent(model=model)
            agent.transform = lambda frame: torch.zeros(1)
            twin = twin_mod.Twin(twin_mod._config(kind))
            for t in range(TICKS):
                model.next = pred[e, t]
                obs = {"velocity": np.array([speed[e, t], 0.0, 0.0], dtype=np.float32), "command": int(command[e, t])}
                obs["rgb" if kind == "image" else "birdview"] = np.zeros((4, 4, 3) if kind == "image" else (320, 320, 7), dtype=np.uint8)
                speed[e, t] = np.linalg.norm(obs["velocity"])          # what the reference measures: the float32 norm (an ulp off at times)
                control = agent.run_step(obs)
                ref[e, t] = [control.steer, control.throttle, control.brake, agent.debug["target_speed"], agent.debug["target"][0],
                             agent.debug["target"][1]]
                cond[e, t] = _conditioning(seen[-1])
                mine = twin.step(pred[e, t], speed[e, t], twin_mod.one_hot(command[e, t:t + 1])[0])
                assert mine[7] == 0.0
                twin_dev = max(twin_dev, float(np.abs(mine[:6] - ref[e, t]).max()))
    finally:
        module.ls_circle = real_ls_circle
    assert len(seen) == EPISODES * TICKS and np.isfinite(ref).all()
    ts, thr = ref[..., 3], THRESHOLD[kind]
    assert cond.min() >= 1e-2, "conditioning %g" % cond.min()
    assert np.abs(ts - thr).min() >= 1e-3, "a target speed within %g of the threshold" % np.abs(ts - thr).min()
    assert (ts > thr).any() and (ts < thr).any(), "both sides of the threshold"
    assert (ref[..., 2] == 1.0).any() and (ref[..., 2] == 0.0).any() and (ref[..., 1] > 0.0).any() and (np.abs(ref[..., 0]) > 0.0).any()
    if kind == "birdview":
        assert ts.min() < 0.3, "the slow episodes reach 0.2 m/s"
    return {kind + "_pred": pred, kind + "_speed": speed, kind + "_command": command, kind + "_ref": ref, kind + "_cond": cond,
            "twin_max_dev_" + kind: np.float64(twin_dev)}


def generate():
    """-> dict of numpy arrays, the contents of agent_controls.npz"""
    import importlib
    twin_mod = importlib.import_module("tests.test_agent_control")
    ref_image, ref_birdview = _reference_agents()
    out = {"numpy_version": np.array(np.__version__)}
    out.update(_run_kind("image", ref_image, twin_mod))
    out.update(_run_kind("birdview", ref_birdview, twin_mod))
    return out


if __name__ == "__main__":
    data = generate()
    np.savez(os.path.join(HERE, "agent_controls.npz"), **data)
    for k in sorted(data):
        if data[k].ndim == 0:
            print(k, data[k])
    for kind in ("image", "birdview"):
        print(kind, "conditioning min %.3g, target speed %.3g .. %.3g" % (data[kind + "_cond"].min(), data[kind + "_ref"][..., 3].min(),
                                                                          data[kind + "_ref"][..., 3].max()))
