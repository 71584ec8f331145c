"""Training visuals on the device (csrc/visuals.hip, include/lbc_hip.h lbc_visuals_render): the grid of waypoint panels the reference's
four training scripts draw on every logging iteration (`_log_visuals`: the bird-view coloured by carla_utils.visualize_birdview, the
teacher's waypoints as blue squares, the student's as red ones, command and per-sample loss written on the canvas, the camera frame
beside it), rendered by one launch from the tensors the loss launch has just read into one uint8 image that stays on the device.
`PanelRenderer.render()` is that launch and reads nothing back; `image()` is the one synchronising copy; `write_png()` writes the file
with the standard library alone.

Where this departs from the reference: the canvas is not resampled to the frame's height (cv2.resize there; here the 160-row frame sits
between two black bands beside the 192-row canvas, every pixel exact); the text is a 5 x 7 font of this project (FONT) instead of
cv2's Hershey face; the grid is not min / max normalised (make_grid(normalize=True) there); the white marker the reference aims at
canvas pixel (0, 0) is an empty numpy slice there and is left out."""
import ctypes
import struct
import zlib

import numpy as np
import torch

from .. import _lib

# carla_utils.py:47-56, restated as data: the canvas colour of an empty pixel and of the seven bird-view channels
# (road, lane, red light, yellow light, green light, vehicle, pedestrian); csrc/visuals.hip holds the same numbers
BACKGROUND = (0, 47, 0)
COLORS = ((102, 102, 102), (253, 253, 17), (204, 6, 5), (250, 210, 1), (39, 232, 51), (0, 0, 142), (220, 20, 60))
BLUE, RED, WHITE = (0, 0, 255), (255, 0, 0), (255, 255, 255)
COMMANDS = ("LEFT", "RIGHT", "STRAIGHT", "FOLLOW")
MODES = {0: 0, 1: 1, "birdview": 2}                        # NativeTrainer phase -> lbc_visuals_desc.mode (phase 2 draws mode 1)
# (size, sort) of the reference's three _log_visuals: 32 sorted (phase 0), 8 unsorted (phase 1), 16 sorted (bird-view)
DEFAULTS = {0: (32, 1), 1: (8, 0), 2: (16, 1)}
MAX_SIZE = 32
GLYPH_W, GLYPH_H, ADVANCE, LINE_PITCH, PAD = 5, 7, 6, 19, 2

# The glyphs: printable ASCII 32..126, seven row bytes each, top row first, bit 4 = the left column of the five.
_GLYPHS = (
    "00000000000000", "04040404040004", "0A0A0A00000000", "0A0A1F0A1F0A0A", "040F140E051E04", "18190204081303", "0C12140815120D",   # space ! " # $ % &
    "04040800000000", "02040808080402", "08040202020408", "0004150E150400", "0004041F040400", "000000000C0408", "0000001F000000",   # ' ( ) * + , -
    "00000000000C0C", "00010204081000",                                                                                             # . /
    "0E11131519110E", "040C040404040E", "0E11010204081F", "1F02040201110E", "02060A121F0202", "1F101E0101110E", "0608101E11110E",   # 0 .. 6
    "1F010204080808", "0E11110E11110E", "0E11110F01020C",                                                                           # 7 8 9
    "000C0C000C0C00", "000C0C000C0408", "02040810080402", "00001F001F0000", "08040201020408", "0E110102040004", "0E11010D15150E",   # : ; < = > ? @
    "0E1111111F1111", "1E11111E11111E", "0E11101010110E", "1C12111111121C", "1F10101E10101F", "1F10101E101010", "0E11101711110F",   # A .. G
    "1111111F111111", "0E04040404040E", "0702020202120C", "11121418141211", "1010101010101F", "111B1515111111", "11111915131111",   # H .. N
    "0E11111111110E", "1E11111E101010", "0E11111115120D", "1E11111E141211", "0F10100E01011E", "1F040404040404", "1111111111110E",   # O .. U
    "11111111110A04", "1111111515150A", "11110A040A1111", "1111110A040404", "1F01020408101F",                                       # V .. Z
    "0E08080808080E", "00100804020100", "0E02020202020E", "040A1100000000", "0000000000001F", "08040200000000",                     # [ \ ] ^ _ `
    "00000E010F110F", "1010161911111E", "00000E1010110E", "01010D1311110F", "00000E111F100E", "0609081C080808",   # a .. f
    "000F11110F010E", "10101619111111", "04000C0404040E", "0200060202120C", "10101214181412", "0C04040404040E", "00001A15151111",   # g .. m
    "00001619111111", "00000E1111110E", "00001E111E1010", "00000D130F0101", "00001619101010", "00000E100E011E", "08081C08080906",   # n .. t
    "0000111111130D", "00001111110A04", "0000111115150A", "0000110A040A11", "000011110F010E", "00001F0204081F",   # u .. z
    "02040408040402", "04040404040404", "08040402040408", "00000815020000",                                                         # { | } ~
)
FONT = bytes.fromhex("".join(_GLYPHS))
assert len(_GLYPHS) == 95 and len(FONT) == 95 * GLYPH_H and max(FONT) < 32


def write_png(path, array):
    """an (H, W, 3) uint8 array -> an 8-bit RGB PNG, every scanline with filter type 0; zlib and struct only"""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: an (H, W, 3) uint8 array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = a.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(str(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


class PanelRenderer:
    """the panels of one pass, on the device.

    mode 0: phase 0; 1: phases 1 and 2; 2: bird-view (include/lbc_hip.h lbc_visuals_render has the definition of every pixel).
    size: panels at most (1..32), the first min(N, size) samples of a batch; sort: order them by loss, descending (the reference
    does in phase 0 and for the bird-view); ncols: panels per row of the grid.

    render(rgb, birdview, pred, teacher, command, loss): one launch on the current stream, nothing read back -> the device uint8
      (rows, cols, 3) tensor, which this object owns and reuses for every batch of the same shape.  rgb: the camera frames, uint8
      (N,H,W,3) or float32 (N,3,H,W) in [0,1] (None in mode 2); birdview: uint8 (N,BH,BW,7) or float32 (N,7,BH,BW), or None in modes 0
      and 1 (a run that caches the teacher holds no bird-view: the canvas is background and dots, crop_size pixels square); pred /
      teacher: float32 (N,5,2) in modes 0 and 2, (N,4,5,2) in mode 1; command one-hot (N,4); loss (N,).
    image(): the last rendered grid as a numpy array, after one synchronising copy; `rendered` -- the launches since the previous
      image() -- starts again at 0."""

    def __init__(self, device, camera=None, mode=1, size=None, sort=None, ncols=4):
        if mode not in (0, 1, 2):
            raise ValueError("PanelRenderer: mode must be 0 (phase 0), 1 (phases 1 and 2) or 2 (bird-view), got %r" % (mode,))
        size = DEFAULTS[mode][0] if size is None else int(size)
        if not 1 <= size <= MAX_SIZE:
            raise ValueError("PanelRenderer: size must lie in 1..%d, got %r" % (MAX_SIZE, size))
        if int(ncols) < 1:
            raise ValueError("PanelRenderer: ncols must be at least 1, got %r" % (ncols,))
        if camera is None:
            from .native import camera_struct
            camera = camera_struct()
        self.device, self.camera, self.mode, self.size, self.ncols = torch.device(device), camera, mode, size, int(ncols)
        self.sort = int(bool(DEFAULTS[mode][1] if sort is None else sort))
        self.font = torch.tensor(list(FONT), dtype=torch.uint8, device=self.device)      # uploaded once
        self.rendered = 0
        self._buffers, self._last = {}, None

    def _desc(self, rgb, birdview, n):
        h = w = 0
        rgb_f32 = bv_f32 = 0
        if self.mode != 2:
            rgb_f32 = int(rgb.dtype == torch.float32)
            ok = rgb.dim() == 4 and rgb.shape[0] == n and ((rgb_f32 and rgb.shape[1] == 3) or (rgb.dtype == torch.uint8 and rgb.shape[3] == 3))
            if not ok:
                raise ValueError("PanelRenderer.render: rgb must be uint8 (N,H,W,3) or float32 (N,3,H,W) for N = %d, got %s %s"
                                 % (n, rgb.dtype, tuple(rgb.shape)))
            h, w = (rgb.shape[2], rgb.shape[3]) if rgb_f32 else (rgb.shape[1], rgb.shape[2])
        if birdview is None:
            bh = bw = int(self.camera.crop_size)
        else:
            bv_f32 = int(birdview.dtype == torch.float32)
            ok = birdview.dim() == 4 and birdview.shape[0] == n and ((bv_f32 and birdview.shape[1] == 7) or
                                                                       (birdview.dtype == torch.uint8 and birdview.shape[3] == 7))
            if not ok:
                raise ValueError("PanelRenderer.render: birdview must be uint8 (N,BH,BW,7) or float32 (N,7,BH,BW) for N = %d, got %s %s"
                                 % (n, birdview.dtype, tuple(birdview.shape)))
            bh, bw = (birdview.shape[2], birdview.shape[3]) if bv_f32 else (birdview.shape[1], birdview.shape[2])
        return _lib.VisualsDesc(camera=self.camera, mode=self.mode, size=self.size, sort=self.sort, ncols=self.ncols, N=n, H=h, W=w,
                                BH=bh, BW=bw, rgb_f32=rgb_f32, birdview_f32=bv_f32)

    def render(self, rgb, birdview, pred, teacher, command, loss):
        n = pred.shape[0]
        rows = (n, 4, 5, 2) if self.mode == 1 else (n, 5, 2)
        if n < 1 or tuple(pred.shape) != rows or tuple(teacher.shape) != rows:
            raise ValueError("PanelRenderer.render: mode %d wants pred and teacher of shape %s with N >= 1, got %s and %s"
                             % (self.mode, ("N",) + rows[1:], tuple(pred.shape), tuple(teacher.shape)))
        if tuple(command.shape) != (n, 4) or tuple(loss.shape) != (n,):
            raise ValueError("PanelRenderer.render: command must be (N,4) and loss (N,) for N = %d" % n)
        if self.mode == 2 and birdview is None:
            raise ValueError("PanelRenderer.render: mode 2 draws the bird-view and needs it")
        if self.mode != 2 and rgb is None:
            raise ValueError("PanelRenderer.render: mode %d draws the camera frame and needs rgb" % self.mode)
        for name, t in (("pred", pred), ("teacher", teacher), ("command", command), ("loss", loss)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.font.device:
                raise ValueError("PanelRenderer.render: %s must be a contiguous float32 tensor on %s" % (name, self.font.device))
        for name, t in (("rgb", rgb if self.mode != 2 else None), ("birdview", birdview)):
            if t is not None and (not t.is_contiguous() or t.device != self.font.device):
                raise ValueError("PanelRenderer.render: %s must be a contiguous tensor on %s" % (name, self.font.device))
        d = self._desc(rgb, birdview, n)
        lib = _lib.get()
        r, c = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.lbc_visuals_image_shape(ctypes.byref(d), ctypes.byref(r), ctypes.byref(c)), "visuals_image_shape")
        out = self._buffers.get((r.value, c.value))
        if out is None:
            out = self._buffers[(r.value, c.value)] = torch.empty((r.value, c.value, 3), dtype=torch.uint8, device=self.device)
        _lib.require_device(pred)
        _lib.check(lib.lbc_visuals_render(ctypes.byref(d), _lib.ptr(rgb if self.mode != 2 else None), _lib.ptr(birdview), _lib.ptr(pred),
                                          _lib.ptr(teacher), _lib.ptr(command), _lib.ptr(loss), _lib.ptr(self.font), _lib.ptr(out),
                                          _lib.stream_for(pred)), "visuals_render")
        self.rendered += 1
        self._last = out
        return out

    def image(self):
        if self._last is None:
            raise RuntimeError("PanelRenderer.image: nothing has been rendered")
        self.rendered = 0
        return self._last.cpu().numpy()
