"""The on-policy tick of phase 2 (DAgger; reference training/train_image_phase2.py:61-149 rollout, :45-58 get_control): the student
drives, the privileged teacher watches the same states and labels them, and what the agents saw is recorded on the device.

TeachingSession is agent.DrivingSession for BOTH networks at once: per tick the host uploads N camera frames, N bird-view maps and 5 N
floats, replays ONE captured graph on one stream -- bird-view crop, teacher forward, teacher controller, student forward, student
controller, lbc_phase2_weight, lbc_rollout_decide, lbc_rollout_stage_u8 (csrc/rollout.hip), two small device-to-device copies -- and
reads one block back: the (N,16) decision rows and both waypoint sets behind them.  Both controllers step every tick whichever control
is applied, as both reference agents do.  The frames, commands, speeds and weights of the tick land in per-agent staging rows
(`capacity` per agent); commit(buffer) hands them to a copying DeviceReplayBuffer.

The session runs on the engines the modules cache (PolicyBase._engine_for) -- the ones NativeTrainer trains on, with the parameters
updated in place, so a replayed tick sees the trained weights.  A forward at a larger batch through the module replaces the cached
engine; the session notices before every tick and captures again on the new one.  It never declares an engine frozen."""
import ctypes

import numpy as np
import torch

from . import _lib
from .agent import CROP_SIZE, CROP_X0, CROP_Y0, MAP_SIZE, ControllerConfig, WaypointController

ROW = 16                                                  # doubles per agent in lbc_rollout_decide's output
ROW_BYTES, WAYPOINT_BYTES = ROW * 8, 40


def p_student(episode, beta=0.95):
    """get_control's probability of the student's control (reference train_image_phase2.py:51), in double"""
    return 0.5 + 0.5 * (1.0 - float(beta) ** int(episode))


def _engine_of(model, shape, device):
    """the module's cached engine for `shape`; an engine that its holder declared frozen (NativeTrainer's teacher) stays frozen"""
    frozen = {id(e): bool(getattr(e, "_frozen", False)) for e in getattr(model, "_engines", {}).values()}
    eng = model.engine(shape, device, max_batch=shape[0], with_grads=False)
    if frozen.get(id(eng)):
        eng.set_frozen(True)
    return eng


def _is_cached(model, eng):
    engines = getattr(model, "_engines", None)
    return engines is None or any(e is eng for e in engines.values())


class TeachingSession:
    """student: an image model (3 channels), teacher: a bird-view model (7 channels), both with their weights loaded.

    run_step(rgb, maps, speeds, commands, active=None) -> (N,3) float64 applied (steer, throttle, brake).  rgb (N,160,384,3) uint8, maps
    (N,320,320,7) uint8 (the teacher's 192 x 192 crop, common.crop_birdview(map, dx=-10), is the first launch), speeds (N,) m/s, commands
    (N,) in 1..4, active (N,) or None: an inactive agent's controllers, cursor and staging rows are untouched and its row is zero.
    `.debug` then holds who (1 student, 0 teacher), weight, staged (rows staged for the agent after the tick), dropped (1 where the
    agent's staging was full and the tick was not recorded), student / teacher (both controllers' (N,3) controls), student_flags /
    teacher_flags, student_waypoints / teacher_waypoints (N,5,2).
    set_episode(episode, beta=0.95) writes p_student = 0.5 + 0.5 (1 - beta^episode).
    end_episode(agents, collided) resets both controllers of the listed agents (the reference builds fresh agents per environment
    episode, :108-109) and, where collided, takes the last five staged ticks -- or as many as there are -- off the agent's list
    (`data = data[:-5]`, :144-145; the list spans episodes since the last commit, as the reference's does).
    commit(buffer) -> {"frames", "skipped_nonfinite", "dropped", "n"}: every agent's staged rows go to buffer.add_batch in agent order,
    rows whose weight is not finite left out; the cursors are zeroed.  The one sync of a rollout besides the per-tick block."""

    def __init__(self, student, teacher, device, n_agents, capacity, camera=None, seed=0, use_graph=True, student_config=None, teacher_config=None,
                 map_size=MAP_SIZE, crop_origin=(CROP_Y0, CROP_X0)):
        from .training.native import camera_struct
        self.device = torch.device(device)
        # (moved, not put into eval mode: the forwards below say train = False themselves, and the student may be a trainer's)
        self.student, self.teacher = (m.to(self.device) if isinstance(m, torch.nn.Module) else m for m in (student, teacher))
        self.n_agents = n = int(n_agents)
        self.capacity = cap = int(capacity)
        if not 1 <= n <= 1024:
            raise ValueError("TeachingSession: n_agents must lie in 1..1024 (one workgroup decides a tick), got %r" % (n_agents,))
        if cap < 1 or n * cap > 0x7fffffff:
            raise ValueError("TeachingSession: capacity must be at least 1 with n_agents * capacity below 2^31, got %r" % (capacity,))
        if student.input_channel != 3 or teacher.input_channel != 7:
            raise ValueError("TeachingSession: the student is a camera model (3 channels) and the teacher a bird-view model (7), got %d and %d"
                             % (student.input_channel, teacher.input_channel))
        sh, sw = tuple(getattr(student, "input_hw", (160, 384)))
        th, tw = tuple(getattr(teacher, "input_hw", (CROP_SIZE, CROP_SIZE)))
        self.map_size, (self.crop_y0, self.crop_x0) = int(map_size), (int(crop_origin[0]), int(crop_origin[1]))
        if min(self.crop_y0, self.crop_x0) < 0 or self.crop_y0 + th > self.map_size or self.crop_x0 + tw > self.map_size:
            raise ValueError("TeachingSession: a %d x %d crop at (%d, %d) does not lie inside the %d x %d map"
                             % (th, tw, self.crop_y0, self.crop_x0, self.map_size, self.map_size))
        for name, nbytes in (("camera", sh * sw * 3), ("bird-view", th * tw * 7)):
            if nbytes % 16:
                raise ValueError("TeachingSession: a %s frame is %d bytes, rows move as 16-byte words" % (name, nbytes))
        self.student_config = student_config or ControllerConfig.image()
        self.teacher_config = teacher_config or ControllerConfig.birdview()
        if self.student_config.kind != "image" or self.teacher_config.kind != "birdview":
            raise ValueError("TeachingSession: the student needs an image controller and the teacher a bird-view one, got %r and %r"
                             % (self.student_config.kind, self.teacher_config.kind))
        self.cam = camera or camera_struct()
        self.seed = int(seed) & 0xFFFFFFFF
        self.use_graph = bool(use_graph) and self.device.type == "cuda"
        dev = self.device
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
        self.rgb, self.map, self.crop = u8(n, sh, sw, 3), u8(n, self.map_size, self.map_size, 7), u8(n, th, tw, 7)
        # host staging is pageable memory on purpose (see inference.PolicySession)
        self.h_small = torch.zeros(5 * n, dtype=torch.float32)              # N speeds, then N one-hot commands
        self.small = torch.zeros(5 * n, dtype=torch.float32, device=dev)
        self.speed, self.command = self.small[:n], self.small[n:].view(n, 4)
        self.h_active = torch.ones(n, dtype=torch.uint8)
        self.active = torch.ones(n, dtype=torch.uint8, device=dev)
        self.student_controller = WaypointController(self.student_config, n, dev)
        self.teacher_controller = WaypointController(self.teacher_config, n, dev)
        self.weight = torch.zeros(n, dtype=torch.float32, device=dev)
        # device state of the rollout: [p_student as a double's bits, the tick counter], cursors, dropped counts
        self.scalars = torch.zeros(2, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(n, dtype=torch.int32, device=dev)
        self.dropped = torch.zeros(n, dtype=torch.int32, device=dev)
        self.slot = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.slot_cmd = torch.zeros(n * cap, dtype=torch.int32, device=dev)
        self.slot_speed = torch.zeros(n * cap, dtype=torch.float32, device=dev)
        self.slot_weight = torch.zeros(n * cap, dtype=torch.float32, device=dev)
        self.rgb_stage, self.birdview_stage = u8(n * cap, sh, sw, 3), u8(n * cap, th, tw, 7)
        # one block comes back per tick: the (N,16) doubles, then both (N,5,2) f32 waypoint sets copied behind them
        self.block = u8(n * (ROW_BYTES + 2 * WAYPOINT_BYTES))
        self.out = self.block[:n * ROW_BYTES].view(torch.float64).view(n, ROW)
        self.student_waypoints = self.block[n * ROW_BYTES:n * (ROW_BYTES + WAYPOINT_BYTES)].view(torch.float32).view(n, 5, 2)
        self.teacher_waypoints = self.block[n * (ROW_BYTES + WAYPOINT_BYTES):].view(torch.float32).view(n, 5, 2)
        self.debug = {}
        self.graph, self.captures = None, 0
        self.s_eng = self.t_eng = None
        self.set_episode(0)
        self._prepare()

    # ---- engines and the captured graph ----------------------------------------------------------------------------
    def _prepare(self):
        """(re)fetch the modules' cached engines, warm up outside the capture and capture the tick; the rollout's device state (tick
        counter, cursors, dropped counts, both controllers' records) is put back afterwards: a capture launches nothing, the warm-up does"""
        n = self.n_agents
        self.graph = None
        self.s_eng = _engine_of(self.student, (n, 3) + tuple(self.rgb.shape[1:3]), self.device)
        self.t_eng = _engine_of(self.teacher, (n, 7) + tuple(self.crop.shape[1:3]), self.device)
        keep = [t.clone() for t in self._state_tensors()]
        staged = (self.slot_cmd.clone(), self.slot_speed.clone(), self.slot_weight.clone())
        first = (self.rgb_stage[::self.capacity].clone(), self.birdview_stage[::self.capacity].clone())
        self.cursor.zero_()                                                 # (the warm-up writes slot 0 of every agent and nothing else)
        for _ in range(2):                                                  # lazy allocations, zero page
            self._tick()
            self.cursor.zero_()
        for t, k in zip(self._state_tensors(), keep):
            t.copy_(k)
        for t, k in zip((self.slot_cmd, self.slot_speed, self.slot_weight), staged):
            t.copy_(k)
        self.rgb_stage[::self.capacity].copy_(first[0])
        self.birdview_stage[::self.capacity].copy_(first[1])
        if self.use_graph:
            torch.cuda.synchronize(self.device)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._tick()
        self.captures += 1

    def _state_tensors(self):
        return (self.scalars, self.cursor, self.dropped, self.student_controller.state, self.teacher_controller.state)

    def _tick(self):
        lib, n = _lib.get(), self.n_agents
        s = _lib.stream_for(self.map)
        th, tw = self.crop.shape[1:3]
        _lib.check(lib.lbc_birdview_crop_u8(_lib.ptr(self.map), _lib.ptr(self.crop), n, self.map_size, self.map_size, 7, self.crop_y0, self.crop_x0,
                                            th, tw, s), "birdview_crop_u8")
        self.t_sel, _ = self.t_eng.forward(self.crop, self.speed, self.command, False)
        t_out = self.teacher_controller.step(self.t_sel, self.speed, self.command, self.active)
        self.s_sel, _ = self.s_eng.forward(self.rgb, self.speed, self.command, False)
        s_out = self.student_controller.step(self.s_sel, self.speed, self.command, self.active)
        _lib.check(lib.lbc_phase2_weight(ctypes.byref(self.cam), _lib.ptr(self.s_sel), _lib.ptr(self.t_sel), n, _lib.ptr(self.weight), s), "phase2_weight")
        _lib.check(lib.lbc_rollout_decide(_lib.ptr(s_out), _lib.ptr(t_out), _lib.ptr(self.weight), _lib.ptr(self.speed), _lib.ptr(self.command),
                                          _lib.ptr(self.active), n, self.capacity, self.seed, _lib.ptr(self.scalars[0:]), _lib.ptr(self.scalars[1:]),
                                          _lib.ptr(self.cursor), _lib.ptr(self.dropped), _lib.ptr(self.slot), _lib.ptr(self.slot_cmd),
                                          _lib.ptr(self.slot_speed), _lib.ptr(self.slot_weight), _lib.ptr(self.out), s), "rollout_decide")
        _lib.check(lib.lbc_rollout_stage_u8(_lib.ptr(self.rgb), int(self.rgb[0].numel()), _lib.ptr(self.crop), int(self.crop[0].numel()), _lib.ptr(self.slot),
                                            n, n * self.capacity, _lib.ptr(self.rgb_stage), _lib.ptr(self.birdview_stage), s), "rollout_stage_u8")
        self.student_waypoints.copy_(self.s_sel)                            # two device-to-device copies of 40 N bytes
        self.teacher_waypoints.copy_(self.t_sel)

    # ---- the tick ------------------------------------------------------------------------------------------------------
    def run_step(self, rgb, maps, speeds, commands, active=None):
        n = self.n_agents
        frames = []
        for name, f, dst in (("rgb", rgb, self.rgb), ("maps", maps, self.map)):
            f = torch.as_tensor(np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f)
            if f.dtype != torch.uint8 or tuple(f.shape) != tuple(dst.shape):
                raise ValueError("run_step: expected uint8 %s of shape %s, got %s %s" % (name, tuple(dst.shape), f.dtype, tuple(f.shape)))
            frames.append(f)
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
        if not (_is_cached(self.student, self.s_eng) and _is_cached(self.teacher, self.t_eng)):
            self._prepare()                     # a larger batch went through the module: its cached engine was replaced, capture on the new one
        if not torch.equal(want, self.h_active):
            self.h_active.copy_(want)
            self.active.copy_(self.h_active)
        self.rgb.copy_(frames[0])
        self.map.copy_(frames[1])
        self.small.copy_(self.h_small)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._tick()
        host = self.block.cpu()                                             # waits for the stream
        rec = host[:n * ROW_BYTES].view(torch.float64).view(n, ROW).numpy()
        wp = host[n * ROW_BYTES:].view(torch.float32).view(2, n, 5, 2).numpy()
        self.debug = {"who": rec[:, 3].astype(np.int64), "weight": rec[:, 4].astype(np.float32), "staged": rec[:, 5].astype(np.int64),
                      "dropped": rec[:, 14].astype(np.int64), "student": rec[:, 8:11].copy(), "teacher": rec[:, 11:14].copy(),
                      "student_flags": rec[:, 6].astype(np.int64), "teacher_flags": rec[:, 7].astype(np.int64),
                      "student_waypoints": wp[0].copy(), "teacher_waypoints": wp[1].copy()}
        return rec[:, :3].copy()

    # ---- episodes --------------------------------------------------------------------------------------------------------
    def set_episode(self, episode, beta=0.95):
        self.p_student = p_student(episode, beta)
        self.scalars[0:1].copy_(torch.tensor([self.p_student], dtype=torch.float64).view(torch.int64))

    def set_p_student(self, p):
        self.p_student = float(p)
        self.scalars[0:1].copy_(torch.tensor([self.p_student], dtype=torch.float64).view(torch.int64))

    def reset(self, agents=None):
        """fresh controllers, both networks' (None: all agents)"""
        self.student_controller.reset(agents)
        self.teacher_controller.reset(agents)

    def end_episode(self, agents, collided=False):
        idx = [int(i) for i in agents]
        if not idx:
            return
        flags = [bool(collided)] * len(idx) if np.ndim(collided) == 0 else [bool(c) for c in collided]
        if len(flags) != len(idx):
            raise ValueError("end_episode: %d agents with %d collision flags" % (len(idx), len(flags)))
        self.reset(idx)
        hit = [i for i, c in zip(idx, flags) if c]
        if hit:
            at = torch.tensor(hit, dtype=torch.int64, device=self.device)
            self.cursor[at] = (self.cursor[at] - 5).clamp_(min=0)

    def commit(self, buffer):
        n, cap = self.n_agents, self.capacity
        if getattr(buffer, "source", None) is not None:
            raise ValueError("TeachingSession.commit: the buffer holds frame indices into a dataset; on-policy frames need a copying DeviceReplayBuffer")
        host = torch.cat([self.cursor.float(), self.dropped.float(), self.slot_weight]).cpu().numpy()      # the one read-back
        cursor, dropped, weight = host[:n].astype(np.int64), host[n:2 * n].astype(np.int64), host[2 * n:]
        rows = np.concatenate([a * cap + np.arange(min(int(cursor[a]), cap)) for a in range(n)]).astype(np.int64)
        finite = np.isfinite(weight[rows])
        take = rows[finite]
        if len(take):
            at = torch.from_numpy(take).to(self.device)
            whole = len(take) == n * cap
            pick = (lambda t: t) if whole else (lambda t: t[at])
            buffer.add_batch(pick(self.rgb_stage), pick(self.birdview_stage), pick(self.slot_cmd), pick(self.slot_speed), pick(self.slot_weight))
        self.cursor.zero_()
        self.dropped.zero_()
        return {"frames": int(len(take)), "skipped_nonfinite": int(len(rows) - len(take)), "dropped": int(dropped.sum()), "n": int(len(buffer))}

    # ---- resumable state -------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"format": 1, "n_agents": self.n_agents, "seed": int(self.seed), "tick": int(self.scalars[1].item()), "p_student": float(self.p_student),
                "cursor": self.cursor.cpu().clone(), "dropped": self.dropped.cpu().clone(), "student_controller": self.student_controller.state_dict(),
                "teacher_controller": self.teacher_controller.state_dict()}

    def load_state_dict(self, sd):
        if sd.get("format") != 1:
            raise ValueError("TeachingSession.load_state_dict: unknown state format %r" % (sd.get("format"),))
        if int(sd["n_agents"]) != self.n_agents:
            raise ValueError("TeachingSession.load_state_dict: the state is of %d agents, this session has %d" % (sd["n_agents"], self.n_agents))
        if int(torch.as_tensor(sd["cursor"]).max()) > self.capacity:
            raise ValueError("TeachingSession.load_state_dict: a cursor of the state lies beyond this session's capacity of %d" % self.capacity)
        self.seed = int(sd["seed"]) & 0xFFFFFFFF
        if self.graph is not None:              # the seed is an argument of the captured launch
            self._prepare()
        self.set_p_student(sd["p_student"])
        self.scalars[1:2].copy_(torch.tensor([int(sd["tick"])], dtype=torch.int64))
        self.cursor.copy_(torch.as_tensor(sd["cursor"]))
        self.dropped.copy_(torch.as_tensor(sd["dropped"]))
        self.student_controller.load_state_dict(sd["student_controller"])
        self.teacher_controller.load_state_dict(sd["teacher_controller"])
