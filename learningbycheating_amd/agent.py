"""The agent half of the tick: waypoints -> steer / throttle / brake on the device (csrc/agent.hip, include/lbc_hip.h lbc_agent_control).

The reference's agents (bird_view/models/image.py:93-219 ImageAgent, birdview.py:82-174 BirdViewAgent) read the five waypoints back,
unproject them, fit a least-squares circle and run two windowed PID controllers in numpy, once per simulator tick.  Here that is ONE
launch behind the network's last kernel, for N agents at once; the two PID windows of every agent live in device memory, so a captured
tick (DrivingSession) ends in the controls and replaying it advances the controllers with no host involvement.

ControllerConfig     the numbers of a controller, built from the reference's argument shapes
WaypointController   the launch and its device state, on tensors
DrivingSession       PolicySession for N agents with the controller as the last launch of the same captured graph
Agent                what ImageAgent / BirdViewAgent (bird_view/models) derive from: the reference's run_step(observations) interface
"""
import ctypes
import math
import types

import numpy as np
import torch

from . import _lib

KINDS = {"image": 0, "birdview": 1}                       # LBC_AGENT_IMAGE / LBC_AGENT_BIRDVIEW
FLAG_DEGENERATE, FLAG_BAD, FLAG_INACTIVE = 1, 2, 4        # LBC_AGENT_FLAG_*
STATE_WORDS = ctypes.sizeof(_lib.AgentState) // 8         # one agent's record as 8-byte words
OUT_FIELDS = ("steer", "throttle", "brake", "target_speed", "target_x", "target_y", "alpha", "flags")
MAP_SIZE, CROP_SIZE, CROP_Y0, CROP_X0 = 320, 192, 58, 64  # common.crop_birdview(map, dx=-10): rows 58..250, columns 64..256

_IMAGE_STEER_POINTS = {"1": 4, "2": 3, "3": 2, "4": 2}
_IMAGE_PID = {"1": {"Kp": 0.5, "Ki": 0.20, "Kd": 0.0}, "2": {"Kp": 0.7, "Ki": 0.10, "Kd": 0.0},
              "3": {"Kp": 1.0, "Ki": 0.10, "Kd": 0.0}, "4": {"Kp": 1.0, "Ki": 0.50, "Kd": 0.0}}
_BIRDVIEW_STEER_POINTS = {"1": 3, "2": 2, "3": 2, "4": 2}
_BIRDVIEW_PID = {"1": {"Kp": 1.0, "Ki": 0.1, "Kd": 0}, "2": {"Kp": 1.0, "Ki": 0.1, "Kd": 0},
                 "3": {"Kp": 0.8, "Ki": 0.1, "Kd": 0}, "4": {"Kp": 0.8, "Ki": 0.1, "Kd": 0}}
_CAMERA = {"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": 4.0}


class ControllerConfig:
    """every number of lbc_agent_desc under the descriptor's field names; build one with image() / birdview(), change fields, pass it on"""

    FIELDS = ("kind", "n_steps", "speed_steps", "w", "h", "fov", "world_y", "fixed_offset", "crop_size", "pixels_per_meter", "gap", "dt",
              "steer_points", "turn_pid", "speed_pid", "turn_window", "speed_window", "engine_brake_threshold", "brake_threshold",
              "stop_threshold")

    def __init__(self, kind, steer_points, turn_pid, speed_pid, gap=5, camera=None):
        if kind not in KINDS:
            raise ValueError("ControllerConfig: kind must be 'image' or 'birdview', got %r" % (kind,))
        cam = dict(_CAMERA, **(camera or {}))
        self.kind, self.n_steps, self.speed_steps = kind, 5, 3
        self.w, self.h, self.fov = float(cam["w"]), float(cam["h"]), float(cam["fov"])
        self.world_y, self.fixed_offset = float(cam["world_y"]), float(cam["fixed_offset"])
        self.crop_size, self.pixels_per_meter = float(CROP_SIZE), 5.0
        self.gap, self.dt = float(gap), 0.1
        # (the reference's steer_points.get(str(cmd), 1) / controller_args[str(cmd)]: dicts keyed "1".."4")
        self.steer_points = [int(steer_points.get(str(c), 1)) for c in range(1, 5)]
        self.turn_pid = [[float(turn_pid[str(c)][k]) for k in ("Kp", "Ki", "Kd")] for c in range(1, 5)]
        self.speed_pid = [float(v) for v in speed_pid]
        self.turn_window, self.speed_window = 10, 30
        self.engine_brake_threshold, self.brake_threshold, self.stop_threshold = 2.0, 2.0, 1.0

    @classmethod
    def image(cls, camera_args=None, steer_points=None, pid=None, gap=5):
        """ImageAgent's arguments (reference image.py:94-120).  camera_args: the reference's default dict carries the frame width under 'x'
        where its constructor reads 'w' (it fails on its own default); either key is accepted here.  The reference reads w, h and
        fixed_offset from it and unprojects with fov = 90, world_y = 1.4 whatever the dict says; here the dict's fov / world_y count."""
        cam = dict(camera_args or {})
        if "w" not in cam and "x" in cam:
            cam["w"] = cam.pop("x")
        cam.pop("x", None)
        return cls("image", steer_points or _IMAGE_STEER_POINTS, pid or _IMAGE_PID, (0.8, 0.08, 0.0), gap, cam)

    @classmethod
    def birdview(cls, steer_points=None, pid=None, gap=5):
        """BirdViewAgent's arguments (reference birdview.py:83-102)"""
        return cls("birdview", steer_points or _BIRDVIEW_STEER_POINTS, pid or _BIRDVIEW_PID, (1.0, 0.1, 2.5), gap)

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def desc(self):
        d = _lib.AgentDesc(kind=KINDS[self.kind] if isinstance(self.kind, str) else int(self.kind), n_steps=int(self.n_steps),
                           speed_steps=int(self.speed_steps), turn_window=int(self.turn_window), speed_window=int(self.speed_window))
        for k in ("w", "h", "fov", "world_y", "fixed_offset", "crop_size", "pixels_per_meter", "gap", "dt", "engine_brake_threshold",
                  "brake_threshold", "stop_threshold"):
            setattr(d, k, float(getattr(self, k)))
        for c in range(4):
            d.steer_points[c] = int(self.steer_points[c])
            for k in range(3):
                d.turn_pid[c][k] = float(self.turn_pid[c][k])
        for k in range(3):
            d.speed_pid[k] = float(self.speed_pid[k])
        return d


class WaypointController:
    """the controllers of n_agents agents on `device`.

    step(pred, speed, command_onehot, active=None): pred (N,5,2), speed (N,), command_onehot (N,4) contiguous float32, active (N,) uint8 or
      None (all), all on this device -> the (N,8) float64 device tensor `out` (OUT_FIELDS), THE SAME tensor on every call: one launch on
      the current stream, no sync, no allocation (so the call can be captured into a graph).
    reset(agents=None): fresh controllers for the given agent indices (None: all), a launch on the current stream.
    state_dict() / load_state_dict(): the device records (a sync) with the window lengths they belong to."""

    def __init__(self, config, n_agents, device):
        if int(n_agents) < 1:
            raise ValueError("WaypointController: n_agents must be at least 1, got %r" % (n_agents,))
        self.config, self.n_agents, self.device = config, int(n_agents), torch.device(device)
        lib = _lib.get()
        if lib.lbc_agent_state_bytes(self.n_agents) != self.n_agents * STATE_WORDS * 8:
            raise RuntimeError("WaypointController: the library's record has %d bytes per agent, this binding was written for %d"
                               % (lib.lbc_agent_state_bytes(1), STATE_WORDS * 8))
        self._desc = config.desc()
        self.state = torch.zeros((self.n_agents, STATE_WORDS), dtype=torch.int64, device=self.device)
        self.out = torch.zeros((self.n_agents, len(OUT_FIELDS)), dtype=torch.float64, device=self.device)
        self._mask = torch.zeros(self.n_agents, dtype=torch.uint8, device=self.device)

    def step(self, pred, speed, command_onehot, active=None):
        n = self.n_agents
        for name, t, shape, dt in (("pred", pred, (n, 5, 2), torch.float32), ("speed", speed, (n,), torch.float32),
                                   ("command_onehot", command_onehot, (n, 4), torch.float32), ("active", active, (n,), torch.uint8)):
            if t is None and name == "active":
                continue
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.state.device:
                raise ValueError("WaypointController.step: %s must be a contiguous %s tensor of shape %s on %s, got %s %s on %s"
                                 % (name, dt, shape, self.state.device, t.dtype, tuple(t.shape), t.device))
        _lib.require_device(pred)
        _lib.check(_lib.get().lbc_agent_control(ctypes.byref(self._desc), _lib.ptr(pred), _lib.ptr(speed), _lib.ptr(command_onehot),
                                                _lib.ptr(active), n, _lib.ptr(self.state), _lib.ptr(self.out), _lib.stream_for(pred)),
                   "agent_control")
        return self.out

    def reset(self, agents=None):
        mask = None
        if agents is not None:
            host = torch.zeros(self.n_agents, dtype=torch.uint8)
            idx = [int(i) for i in agents]
            if any(not 0 <= i < self.n_agents for i in idx):
                raise ValueError("WaypointController.reset: agent indices must lie in 0..%d, got %r" % (self.n_agents - 1, idx))
            host[idx] = 1
            self._mask.copy_(host)
            mask = self._mask
        _lib.check(_lib.get().lbc_agent_reset(_lib.ptr(mask), self.n_agents, _lib.ptr(self.state), _lib.stream_for(self.state)), "agent_reset")

    def state_dict(self):
        return {"state": self.state.cpu().clone(), "kind": self.config.kind, "turn_window": int(self.config.turn_window),
                "speed_window": int(self.config.speed_window)}

    def load_state_dict(self, sd):
        for k in ("kind", "turn_window", "speed_window"):
            if sd[k] != getattr(self.config, k):
                raise ValueError("WaypointController.load_state_dict: the records were saved with %s = %r, this controller has %r"
                                 % (k, sd[k], getattr(self.config, k)))
        st = torch.as_tensor(sd["state"])
        if st.dtype != torch.int64 or tuple(st.shape) != tuple(self.state.shape):
            raise ValueError("WaypointController.load_state_dict: expected an int64 tensor of shape %s, got %s %s"
                             % (tuple(self.state.shape), st.dtype, tuple(st.shape)))
        self.state.copy_(st)


def controls_dict(rec, waypoints=None):
    """an (N,8) record as numpy -> the `.debug` dict"""
    out = {"target_speed": rec[:, 3].copy(), "target": rec[:, 4:6].copy(), "alpha": rec[:, 6].copy(), "flags": rec[:, 7].astype(np.int64)}
    if waypoints is not None:
        out["waypoints"] = waypoints
    return out


class DrivingSession:
    """model: ImagePolicyModelSS / BirdViewPolicyModelSS with its weights loaded.  One tick for n_agents agents:
    run_step(frames, speeds, commands, active=None) -> (N,3) float64 numpy array of (steer, throttle, brake).

    frames: uint8 (N,H,W,3) camera frames, or for a bird-view model the simulator's (N,320,320,7) maps (the agent's 192 x 192 crop,
    common.crop_birdview(map, dx=-10), is the first launch of the tick); speeds (N,) in m/s; commands (N,) in 1..4; active (N,) or None:
    an inactive agent's controllers keep their state and its row is zero.  Per tick the host uploads the N frames and 5 N floats
    (the mask only when it changes), replays ONE captured graph -- crop, forward, controller -- and reads one block back: the (N,8)
    records and the N x 5 x 2 normalised waypoints behind them.  `.debug` then holds target_speed, target, alpha, flags, waypoints.
    reset(agents=None) is launched eagerly on the same stream, outside the graph."""

    def __init__(self, model, device, n_agents=1, use_graph=True, config=None):
        self.model = model.to(device).eval()
        self.device = torch.device(device)
        self.n_agents = n = int(n_agents)
        c = model.input_channel
        self.kind = "image" if c == 3 else "birdview"
        h, w = tuple(getattr(model, "input_hw", (160, 384) if c == 3 else (192, 192)))
        if config is None:
            config = ControllerConfig.image() if self.kind == "image" else ControllerConfig.birdview()
        if config.kind != self.kind:
            raise ValueError("DrivingSession: a %s model needs a %s controller, got %r" % (self.kind, self.kind, config.kind))
        self.config = config
        self.eng = model.engine((n, c, h, w), self.device, max_batch=n, with_grads=False)
        self.frame = torch.zeros((n, h, w, c), dtype=torch.uint8, device=self.device)
        self.map = torch.zeros((n, MAP_SIZE, MAP_SIZE, c), dtype=torch.uint8, device=self.device) if self.kind == "birdview" else None
        if self.map is not None and (h, w) != (CROP_SIZE, CROP_SIZE):
            raise ValueError("DrivingSession: the bird-view crop is %d x %d, the model takes %d x %d" % (CROP_SIZE, CROP_SIZE, h, w))
        self.upload = self.map if self.map is not None else self.frame
        # host staging is pageable memory on purpose (see inference.PolicySession)
        self.h_small = torch.zeros(5 * n, dtype=torch.float32)              # N speeds, then N one-hot commands
        self.small = torch.zeros(5 * n, dtype=torch.float32, device=self.device)
        self.speed, self.command = self.small[:n], self.small[n:].view(n, 4)
        self.h_active = torch.ones(n, dtype=torch.uint8)
        self.active = torch.ones(n, dtype=torch.uint8, device=self.device)
        self.controller = WaypointController(config, n, self.device)
        # one block comes back per tick: the controller's (N,8) doubles, then the (N,5,2) f32 waypoints copied behind them
        self.block = torch.zeros(n * (64 + 40), dtype=torch.uint8, device=self.device)
        self.controller.out = self.block[:n * 64].view(torch.float64).view(n, 8)
        self.waypoints = self.block[n * 64:].view(torch.float32).view(n, 5, 2)
        self.debug = {}
        self.graph = None
        for _ in range(2):                                                  # warm-up outside the capture (lazy allocations, zero page)
            self._tick()
        self.controller.reset()
        if use_graph and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._tick()                                                # (a capture launches nothing: the controllers are still fresh)

    def _tick(self):
        if self.map is not None:
            _lib.check(_lib.get().lbc_birdview_crop_u8(_lib.ptr(self.map), _lib.ptr(self.frame), self.n_agents, MAP_SIZE, MAP_SIZE,
                                                       self.map.shape[3], CROP_Y0, CROP_X0, CROP_SIZE, CROP_SIZE, _lib.stream_for(self.map)),
                       "birdview_crop_u8")
        self.out_sel, self.out_all = self.eng.forward(self.frame, self.speed, self.command, False)
        self.controller.step(self.out_sel, self.speed, self.command, self.active)
        self.waypoints.copy_(self.out_sel)                                  # a device-to-device copy of 40 N bytes

    def run_step(self, frames, speeds, commands, active=None):
        n = self.n_agents
        f = torch.as_tensor(np.ascontiguousarray(frames) if isinstance(frames, np.ndarray) else frames)
        if f.dtype != torch.uint8 or tuple(f.shape) != tuple(self.upload.shape):
            raise ValueError("run_step: expected uint8 frames of shape %s, got %s %s" % (tuple(self.upload.shape), f.dtype, tuple(f.shape)))
        speeds, commands = np.asarray(speeds, dtype=np.float64).reshape(-1), np.asarray(commands).reshape(-1)
        if speeds.shape[0] != n or commands.shape[0] != n:
            raise ValueError("run_step: %d agents need %d speeds and commands, got %d and %d" % (n, n, speeds.shape[0], commands.shape[0]))
        self.h_small.zero_()
        for i in range(n):
            self.h_small[i] = float(speeds[i])
            self.h_small[n + 4 * i + min(max(int(commands[i]) - 1, 0), 3)] = 1.0
        want = torch.ones(n, dtype=torch.uint8) if active is None else torch.as_tensor(np.asarray(active).reshape(-1) != 0).to(torch.uint8)
        if want.shape[0] != n:
            raise ValueError("run_step: active must have %d entries, got %d" % (n, want.shape[0]))
        if not torch.equal(want, self.h_active):
            self.h_active.copy_(want)
            self.active.copy_(self.h_active)
        self.upload.copy_(f)
        self.small.copy_(self.h_small)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._tick()
        host = self.block.cpu()                                             # waits for the stream
        rec = host[:n * 64].view(torch.float64).view(n, 8).numpy()
        self.debug = controls_dict(rec, host[n * 64:].view(torch.float32).view(n, 5, 2).numpy().copy())
        return rec[:, :3].copy()

    def reset(self, agents=None):
        self.controller.reset(agents)


def _vehicle_control():
    """carla.VehicleControl() where carla imports (tried here, never at module load), a plain namespace otherwise"""
    try:
        import carla
        return carla.VehicleControl()
    except Exception:
        return types.SimpleNamespace()


class Agent:
    """reference bird_view/models/agent.py Agent: `model=` is required, unknown keywords are reported and ignored"""
    _kind = None

    def __init__(self, model=None, config=None, **kwargs):
        assert model is not None
        if len(kwargs) > 0:
            print("Unused kwargs: %s" % kwargs)
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.session = DrivingSession(model, self.device, n_agents=1, config=config)
        self.model = self.session.model
        self.debug = dict()

    def postprocess(self, steer, throttle, brake):
        control = _vehicle_control()
        control.steer = float(np.clip(steer, -1.0, 1.0))
        control.throttle = float(np.clip(throttle, 0.0, 1.0))
        control.brake = float(np.clip(brake, 0.0, 1.0))
        control.manual_gear_shift = False
        return control

    def reset(self):
        """fresh controllers (the reference builds a new agent per episode)"""
        self.session.reset()

    def _observe(self, observations, key):
        frame = np.ascontiguousarray(observations[key])
        speed = float(np.linalg.norm(observations["velocity"]))
        steer, throttle, brake = self.session.run_step(frame[None], [speed], [int(observations["command"])])[0]
        d = self.session.debug
        self.debug = {"target_speed": float(d["target_speed"][0]), "target": d["target"][0], "alpha": float(d["alpha"][0]),
                      "flags": int(d["flags"][0]), "waypoints": d["waypoints"][0]}
        return self.postprocess(steer, throttle, brake), d["waypoints"][0]
