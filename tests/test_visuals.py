"""Training visuals on the device (csrc/visuals.hip, training/visuals.py, NativeTrainer.step(visuals=), --visuals).

The yardstick is `_twin` below: a numpy restatement of the definition in include/lbc_hip.h (lbc_visuals_render), written from that
text and not from the kernel -- it paints the way the reference's _log_visuals paints (background, channel colours in order, dots in
order, text last, panels pasted into a grid), where the kernel decides every pixel once.  The comparison is byte for byte: every
coordinate is computed in double from the same f32 inputs on both sides, and the seeded waypoints are redrawn until every dot
coordinate lies at least 1e-6 from an integer (`_draw`; the twin asserts it), so that a last-bit difference -- the compiler may
contract a multiply and an add on the device -- cannot move a truncation.  Exact-integer centres appear only where no arithmetic
touches them (the bird-view mode's ground truth in pixels).

1. byte-exact parity, every mode; 2. dots at and beyond every edge; 3. text; 4. order; 5. entry-point refusals;
6. NativeTrainer.step(visuals=); 7. the scripts; 8. write_png.  Every kernel case runs on the emulator and, gpu-marked, on gfx950; the
output lies between fences of a uint8 pattern, and on the GPU every launch runs three times, bit-identical (helpers.repeat)."""
import ctypes
import json
import math
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests.helpers import WHERE, guarded, guarded_input, on_both, repeat
from tests.test_resume_guard import _script, _sync

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
BLUE, RED, WHITE, BLACK = (0, 0, 255), (255, 0, 0), (255, 255, 255), (0, 0, 0)
NAN, INF = float("nan"), float("inf")


def _cam(**kw):
    """the camera as the f32 values lbc_camera carries (both sides compute in double from these)"""
    c = dict(w=384.0, h=160.0, fov=90.0, world_y=1.4, fixed_offset=4.0, pixels_per_meter=5.0, crop_size=192.0)
    c.update(kw)
    return {k: float(np.float32(v)) for k, v in c.items()}


FULL = (160, 384, 192, 192)                    # (H, W, BH, BW) of this project
SMALL = (12, 20, 16, 16)
CAM_FULL = _cam()
CAM_SMALL = _cam(w=20.0, h=12.0, crop_size=16.0, pixels_per_meter=1.0, fixed_offset=1.0)


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------------
def _command(row):
    nz = np.flatnonzero(np.asarray(row) != 0)
    return int(nz[0]) if len(nz) else -1


def _centres(mode, cam, pred, teach, c):
    """the dots of one sample in drawing order: [(where, x, y, colour)], where = "canvas" / "frame"; double from the f32 inputs"""
    w, h, crop, ppm = cam["w"], cam["h"], cam["crop_size"], cam["pixels_per_meter"]
    f = w / (2.0 * math.tan(cam["fov"] * 3.14159265358979323846 / 360.0))
    if mode == 1:
        if c < 0:
            return []
        pred, teach = pred[c], teach[c]
    p = [(float(x), float(y)) for x, y in np.asarray(pred, dtype=np.float32)]
    t = [(float(x), float(y)) for x, y in np.asarray(teach, dtype=np.float32)]
    out = []
    with np.errstate(all="ignore"):
        if mode == 2:
            out += [("canvas", x, y, BLUE) for x, y in t]
            out += [("canvas", (x + 1.0) * crop / 2.0, (y + 1.0) * crop / 2.0, RED) for x, y in p]
            return out
        out += [("canvas", (x + 1.0) * crop / 2.0, (y + 1.0) * crop / 2.0, BLUE) for x, y in t]
        if mode == 1:
            for x, y in p:
                lx, ly = (x + 1.0) * w / 2.0, (y + 1.0) * h / 2.0
                xt, yt = np.float64(lx - w / 2.0) / f, np.float64(ly - h / 2.0) / f
                wz = np.float64(cam["world_y"]) / yt
                wx = wz * xt
                out.append(("canvas", float(wx * ppm + crop / 2.0), float(crop - wz * ppm + cam["fixed_offset"] * ppm), RED))
        if mode == 0:
            for x, y in t:
                mx, my = (x + 1.0) * crop / 2.0, (y + 1.0) * crop / 2.0
                X, Z = np.float64(mx - crop / 2.0) / ppm, np.float64(crop - my) / ppm + cam["fixed_offset"]
                u, v = f * X / Z + w / 2.0, np.float64(f * cam["world_y"]) / Z + h / 2.0
                out.append(("frame", float(np.clip(u, 0.0, w)), float(np.clip(v, 0.0, h)), BLUE))
        out += [("frame", (x + 1.0) * w / 2.0, (y + 1.0) * h / 2.0, RED) for x, y in p]
    return out


def _drawable(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 30


def _dot(img, x, y, colour, strict):
    if not (_drawable(x) and _drawable(y)):
        return
    if strict:
        assert min(abs(x - round(x)), abs(y - round(y))) >= 1e-6, "a dot coordinate within 1e-6 of an integer: draw the inputs again"
    ix, iy = int(x), int(y)                                  # truncates toward zero
    r0, r1, c0, c1 = max(iy - 2, 0), min(iy + 3, img.shape[0]), max(ix - 2, 0), min(ix + 3, img.shape[1])
    if r0 < r1 and c0 < c1:
        img[r0:r1, c0:c1] = colour


def _loss_text(v):
    return "Loss: " + "%.2f" % float(np.float32(v))


def _command_text(c):
    from learningbycheating_amd.training.visuals import COMMANDS
    return "Command: " + (COMMANDS[c] if c >= 0 else "???")


def _write(canvas, line, text):
    from learningbycheating_amd.training.visuals import FONT
    top = 19 * line - 6
    for i, ch in enumerate(text):
        glyph = FONT[(ord(ch) - 32) * 7:(ord(ch) - 32) * 7 + 7]
        for gy in range(7):
            for gx in range(5):
                y, x = top + gy, 6 * i + gx
                if y < canvas.shape[0] and x < canvas.shape[1] and (glyph[gy] >> (4 - gx)) & 1:
                    canvas[y, x] = WHITE


def _panel(mode, cam, geom, rgb, bv, pred, teach, cmd, loss, strict=True):
    """one sample's panel; rgb / bv are that sample's slice in the layout the kernel is given (u8 HWC or f32 CHW), bv may be None"""
    from learningbycheating_amd.training.visuals import BACKGROUND, COLORS
    H, W, BH, BW = geom
    canvas = np.empty((BH, BW, 3), dtype=np.uint8)
    canvas[...] = BACKGROUND
    if bv is not None:
        planes = bv if bv.dtype == np.uint8 else bv.transpose(1, 2, 0)
        for i in range(7):
            canvas[planes[:, :, i] > 0] = COLORS[i]
    frame = None
    if mode != 2:
        frame = rgb.copy() if rgb.dtype == np.uint8 else np.uint8(rgb.transpose(1, 2, 0) * np.float32(255.0))
        assert frame.shape == (H, W, 3)
    c = _command(cmd)
    for where, x, y, colour in _centres(mode, cam, pred, teach, c):
        _dot(canvas if where == "canvas" else frame, x, y, colour, strict)
    _write(canvas, 1, _command_text(c))
    _write(canvas, 2, _loss_text(loss))
    if mode == 2:
        return canvas
    panel = np.zeros((BH, W + BW, 3), dtype=np.uint8)
    top = (BH - H) // 2
    panel[top:top + H, :W] = frame
    panel[:, W:] = canvas
    return panel


def _order(loss, n, size, sort):
    m = min(n, size)
    if not sort:
        return list(range(m))
    key = lambda i: (0, 0.0) if math.isnan(loss[i]) else (1, -float(loss[i]))       # NaN first, then descending; sorted() is stable
    return sorted(range(m), key=key)


def _twin(mode, cam, geom, size, sort, ncols, rgb, bv, pred, teach, cmd, loss, strict=True):
    n = pred.shape[0]
    order = _order(loss, n, size, sort)
    H, W, BH, BW = geom
    PH, PW = BH, (BW if mode == 2 else W + BW)
    grid = np.zeros((2 + -(-len(order) // ncols) * (PH + 2), 2 + ncols * (PW + 2), 3), dtype=np.uint8)
    for k, s in enumerate(order):
        r, c = 2 + (k // ncols) * (PH + 2), 2 + (k % ncols) * (PW + 2)
        grid[r:r + PH, c:c + PW] = _panel(mode, cam, geom, None if rgb is None else rgb[s], None if bv is None else bv[s], pred[s], teach[s],
                                          cmd[s], loss[s], strict)
    return grid


def _slot(grid, k, mode, geom, ncols):
    H, W, BH, BW = geom
    PH, PW = BH, (BW if mode == 2 else W + BW)
    r, c = 2 + (k // ncols) * (PH + 2), 2 + (k % ncols) * (PW + 2)
    return grid[r:r + PH, c:c + PW]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _draw(mode, cam, geom, n, seed, rgb_f32=False, bv="u8"):
    """seeded numpy inputs (rgb, bv, pred, teach, cmd, loss); every dot coordinate at least 1e-6 from an integer (a sample that comes
    closer is drawn again); commands cycle through the four branches and an all-zero row"""
    rng = np.random.RandomState(seed)
    H, W, BH, BW = geom
    shape = (4, 5, 2) if mode == 1 else (5, 2)

    def waypoints():
        p = rng.uniform(-1.1, 1.1, size=shape)
        if mode != 2:
            p[..., 1] = rng.uniform(-0.2, 1.1, size=shape[:-1])          # mostly below the horizon
        t = rng.uniform(-4.0, BW + 4.0, size=shape) if mode == 2 else rng.uniform(-1.1, 1.1, size=shape)
        return p.astype(np.float32), t.astype(np.float32)
    cmd = np.zeros((n, 4), dtype=np.float32)
    for s in range(n):
        if s % 5 != 4:
            cmd[s, s % 5] = 1.0
    pred, teach = np.zeros((n,) + shape, dtype=np.float32), np.zeros((n,) + shape, dtype=np.float32)
    for s in range(n):
        for _ in range(50):
            pred[s], teach[s] = waypoints()
            cs = [v for _, x, y, _ in _centres(mode, cam, pred[s], teach[s], _command(cmd[s])) for v in (x, y) if _drawable(v)]
            if all(abs(v - round(v)) >= 1e-6 for v in cs):
                break
        else:
            raise AssertionError("could not draw dots away from the integers")
    rgb = None
    if mode != 2:
        rgb = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
        if rgb_f32:
            rgb = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)
    birdview = None
    if bv is not None:
        birdview = (rng.uniform(size=(n, BH, BW, 7)) < 0.12).astype(np.uint8) * rng.randint(1, 256, size=(n, BH, BW, 7)).astype(np.uint8)
        if bv == "f32":
            birdview = np.ascontiguousarray(birdview.transpose(0, 3, 1, 2) > 0).astype(np.float32)
    loss = rng.uniform(0.0, 3.0, size=n).astype(np.float32)
    return rgb, birdview, pred, teach, cmd, loss


def _dev(dev, *arrays):
    return [None if a is None else guarded_input(torch.from_numpy(np.ascontiguousarray(a)).to(dev)) for a in arrays]


def _desc(mode, cam, geom, n, panels, by_loss, per_row, rgb=None, bv=None, **kw):
    """kw: descriptor fields that replace the ones derived here"""
    from learningbycheating_amd import _lib
    from learningbycheating_amd.training.native import camera_struct
    H, W, BH, BW = geom
    d = dict(camera=camera_struct(**cam), mode=mode, size=panels, sort=by_loss, ncols=per_row, N=n, H=0 if mode == 2 else H, W=0 if mode == 2 else W,
             BH=BH, BW=BW, rgb_f32=int(rgb is not None and rgb.dtype == np.float32), birdview_f32=int(bv is not None and bv.dtype == np.float32))
    d.update(kw)
    return _lib.VisualsDesc(**d)


_FONT_DEV = {}


def _font(dev):
    from learningbycheating_amd.training.visuals import FONT
    key = str(dev)
    if key not in _FONT_DEV:
        _FONT_DEV[key] = torch.tensor(list(FONT), dtype=torch.uint8, device=dev)
    return _FONT_DEV[key]


def _fences_ok(buf, n):
    return bool((buf[:256] == FILL).all() and (buf[256 + n:] == FILL).all())


def _render(dev, mode, cam, geom, size, sort, ncols, arrays):
    """the C entry points on numpy inputs -> the grid (numpy); output between fences, three bit-identical launches on the GPU"""
    from learningbycheating_amd import _lib
    lib = _lib.get()
    rgb, bv, pred, teach, cmd, loss = arrays
    d = _desc(mode, cam, geom, pred.shape[0], size, sort, ncols, rgb, bv)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.lbc_visuals_image_shape(ctypes.byref(d), ctypes.byref(r), ctypes.byref(c)))
    t = _dev(dev, *arrays)

    def launch():
        buf, out = guarded((r.value, c.value, 3), dev, fill=FILL, dtype=torch.uint8)
        _lib.check(lib.lbc_visuals_render(ctypes.byref(d), _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), _lib.ptr(t[4]),
                                          _lib.ptr(t[5]), _lib.ptr(_font(dev)), _lib.ptr(out), _lib.stream_for(out)), "visuals_render")
        _sync(dev)
        assert _fences_ok(buf, out.numel()), "the kernel wrote outside the image"
        return (out,)
    return repeat(dev, launch)[0].cpu().numpy()


def _check(dev, mode, cam, geom, size, sort, ncols, arrays, strict=True):
    got = _render(dev, mode, cam, geom, size, sort, ncols, arrays)
    want = _twin(mode, cam, geom, size, sort, ncols, *arrays, strict=strict)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%d pixels differ, the first at (row, col) %s: kernel %s, twin %s"
                             % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
    return got


# ---- the data restated from the reference ---------------------------------------------------------------------------------------------
def test_colours_are_the_references_table():
    from learningbycheating_amd.training import visuals as V
    assert tuple(V.COLORS) == ((102, 102, 102), (253, 253, 17), (204, 6, 5), (250, 210, 1), (39, 232, 51), (0, 0, 142), (220, 20, 60))
    assert tuple(V.BACKGROUND) == (0, 47, 0)
    assert len(V.FONT) == 95 * 7 and V.DEFAULTS == {0: (32, 1), 1: (8, 0), 2: (16, 1)}


# ---- 1. byte-exact parity ---------------------------------------------------------------------------------------------------------------
# (mode, N, size, ncols, geometry, rgb f32, bird-view u8 / f32 / None); sorted as the reference sorts (modes 0 and 2)
PARITY = [(mode, n, size, ncols, geom, rgb_f32, bv)
          for (n, size, ncols), per_mode in (((1, 8, 4), ((FULL, False, "u8"), (SMALL, True, None), (SMALL, False, "f32"))),
                                             ((3, 8, 4), ((SMALL, True, "f32"), (FULL, False, None), (SMALL, False, "u8"))),
                                             ((8, 8, 4), ((SMALL, False, None), (SMALL, False, "u8"), (FULL, False, "u8"))),
                                             ((9, 8, 4), ((SMALL, False, "u8"), (SMALL, True, "f32"), (SMALL, False, "f32"))),
                                             ((5, 32, 2), ((SMALL, True, "u8"), (SMALL, False, "f32"), (SMALL, False, "u8"))),
                                             ((33, 32, 4), ((SMALL, False, "f32"), (SMALL, False, None), (SMALL, False, "u8"))))
          for mode, (geom, rgb_f32, bv) in enumerate(per_mode)]
# eight full rows at this project's geometry: the largest image the defaults produce (1,554 x 2,314 pixels)
PARITY_REAL = [(0, 33, 32, 4, FULL, False, "u8")]


@pytest.mark.parametrize("case", on_both("case", PARITY, edge=[("full-8-rows", PARITY_REAL[0])]))
def test_kernel_matches_the_twin(env, case):
    dev, _ = env
    mode, n, size, ncols, geom, rgb_f32, bv = case
    cam = CAM_FULL if geom == FULL else CAM_SMALL
    arrays = _draw(mode, cam, geom, n, seed=100 * mode + n, rgb_f32=rgb_f32, bv=bv)
    got = _check(dev, mode, cam, geom, size, mode != 1, ncols, arrays)
    shown = min(n, size)
    H, W, BH, BW = geom
    assert got.shape == (2 + -(-shown // ncols) * (BH + 2), 2 + ncols * ((BW if mode == 2 else W + BW) + 2), 3)
    for k in range(shown, -(-shown // ncols) * ncols):
        assert not _slot(got, k, mode, geom, ncols).any(), "an unused slot of the last row is black"
    assert (got == RED).all(axis=2).any() and (got == BLUE).all(axis=2).any() and (got == WHITE).all(axis=2).any()


# ---- 2. dots at and beyond every edge ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_dots_are_clipped_on_all_four_sides(env, where):
    """bird-view mode, one BLUE dot per sample at an exact pixel centre (the ground truth is not touched by arithmetic): centres at
    -3, -2, 0, 1, last - 1, last, last + 2 along each axis; NaN, +-inf and 1e12 draw nothing"""
    dev, _ = env
    BH, BW = 48, 30
    geom, cam = (0, 0, BH, BW), _cam(crop_size=30.0)
    xs = [(float(v), 25.0) for v in (-3, -2, 0, 1, BW - 2, BW - 1, BW + 1)]
    ys = [(15.0, float(v)) for v in (-3, -2, 0, 1, BH - 2, BH - 1, BH + 1)]
    bad = [(NAN, 25.0), (15.0, INF), (-INF, 25.0), (15.0, 1e12), (-1e12, 25.0), (2.0 ** 30, 25.0)]
    centres = xs + ys + bad
    n = len(centres)
    teach = np.full((n, 5, 2), NAN, dtype=np.float32)
    teach[:, 2] = np.array(centres, dtype=np.float32)
    pred = np.full((n, 5, 2), NAN, dtype=np.float32)
    cmd = np.tile(np.array([[0, 1, 0, 0]], dtype=np.float32), (n, 1))
    loss = np.arange(n, dtype=np.float32)
    bv = np.zeros((n, BH, BW, 7), dtype=np.uint8)
    got = _check(dev, 2, cam, geom, 32, 0, 5, (None, bv, pred, teach, cmd, loss), strict=False)
    visible = lambda v, last: len([i for i in range(int(v) - 2, int(v) + 3) if 0 <= i <= last])
    for s, (x, y) in enumerate(centres):
        blue = int((_slot(got, s, 2, geom, 5) == BLUE).all(axis=2).sum())
        want = 0 if s >= len(xs) + len(ys) else visible(x, BW - 1) * visible(y, BH - 1)
        assert blue == want, (s, x, y, blue, want)
    assert [visible(v, BW - 1) for v, _ in xs] == [0, 1, 3, 4, 4, 3, 1]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("mode", [0, 1])
def test_frame_dots_stay_inside_the_frame(env, where, mode):
    """the student's RED dots at and beyond the frame's edges (centres at half-integers: (p + 1) w / 2 is arithmetic): nothing bleeds
    into the canvas beside the frame or the black bands above and below it; -0.5 truncates to 0"""
    dev, _ = env
    H, W, BH, BW = geom = (12, 20, 24, 16)
    cam = _cam(w=20.0, h=12.0, crop_size=16.0, pixels_per_meter=1.0, fixed_offset=1.0)
    px = [(-2.5, 6.5), (-0.5, -0.5), (0.5, 6.5), (W - 0.5, 6.5), (W + 1.5, 6.5), (10.5, -2.5), (10.5, H - 0.5), (10.5, H + 1.5), (10.5, H + 2.5),
          (W + 2.5, 6.5)]
    n = 2
    shape = (n, 4, 5, 2) if mode == 1 else (n, 5, 2)
    norm = np.array([[(x * 2.0 / W - 1.0, y * 2.0 / H - 1.0) for x, y in px[5 * s:5 * s + 5]] for s in range(n)], dtype=np.float32)
    pred = np.full(shape, NAN, dtype=np.float32)
    cmd = np.zeros((n, 4), dtype=np.float32)
    cmd[:, 2] = 1.0
    if mode == 1:
        pred[:, 2] = norm
    else:
        pred[:] = norm
    teach = np.full(shape, NAN, dtype=np.float32)
    rng = np.random.RandomState(5)
    rgb = rng.randint(0, 200, size=(n, H, W, 3)).astype(np.uint8)             # (no frame byte is pure red)
    loss = np.array([0.25, 0.5], dtype=np.float32)
    got = _check(dev, mode, cam, geom, 8, 0, 4, (rgb, None, pred, teach, cmd, loss))
    top = (BH - H) // 2
    for s in range(n):
        panel = _slot(got, s, mode, geom, 4)
        red = (panel == RED).all(axis=2)
        assert not panel[:top, :W].any() and not panel[top + H:, :W].any(), "the bands above and below the frame are black"
        if mode == 0:
            assert not red[:, W:].any(), "a frame dot reached the canvas"
        assert red[top:top + H, :W].sum() == [3 * 3 + 3 * 5 + 3 * 5, 5 * 3 + 5 * 1][s], red[top:top + H, :W].sum()
    first = _slot(got, 0, mode, geom, 4)
    assert (first[top:top + 3, :3] == RED).all(), "(-0.5, -0.5) truncates to (0, 0): rows and columns 0..2"


@pytest.mark.parametrize("where", WHERE)
def test_later_dots_cover_earlier_ones_and_text_covers_dots(env, where):
    dev, _ = env
    BH, BW = 48, 60
    geom, cam = (0, 0, BH, BW), _cam(crop_size=60.0)
    teach = np.full((1, 5, 2), NAN, dtype=np.float32)
    pred = np.full((1, 5, 2), NAN, dtype=np.float32)
    teach[0, 0] = (15.0, 25.0)
    pred[0, 0] = (17.5 / 30.0 - 1.0, 25.5 / 30.0 - 1.0)        # RED centre (17, 25): covers columns 15..17 of the BLUE square 13..17
    teach[0, 1] = (3.0, 15.0)                                  # under the 'C' of line 1 (rows 13..19, columns 0..4)
    cmd = np.array([[1, 0, 0, 0]], dtype=np.float32)
    got = _check(dev, 2, cam, geom, 8, 1, 1, (None, np.zeros((1, BH, BW, 7), dtype=np.uint8), pred, teach, cmd, np.array([1.0], dtype=np.float32)),
                 strict=False)
    panel = _slot(got, 0, 2, geom, 1)
    assert tuple(panel[25, 13]) == BLUE and tuple(panel[25, 14]) == BLUE and tuple(panel[25, 16]) == RED and tuple(panel[25, 19]) == RED
    # 'C' row 0 is .XXX. : columns 1..3 white over the dot's rows 13..17, columns 1..5
    assert [tuple(panel[13, x]) for x in range(1, 6)] == [WHITE, WHITE, WHITE, BLUE, BLUE] and tuple(panel[13, 0]) == (0, 47, 0)


# ---- 3. text ------------------------------------------------------------------------------------------------------------------------------
LOSSES = [0.0, 0.005, float(np.float32(0.015)), 0.125, 12.345, 99999.99, -1.5, NAN, INF, -INF, -0.0, 0.995, 1e30, 3.4028234663852886e38,
          -3.0e38, 2.0 ** 53 / 100.0, 1.0e-10]


def test_percent_2f_is_rint_of_hundredths():
    """the definition of the number: c = rint(v * 100) in double, printed as integer part, '.', two digits.  An f32 times 100 is exact
    in double, so this IS Python's '%.2f' of the value, ties included -- over the listed losses and 20,000 random f32 bit patterns"""
    rng = np.random.RandomState(1)
    vals = [np.float32(v) for v in LOSSES] + list(rng.randint(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32))
    from fractions import Fraction
    for v in vals:
        v = float(v)
        if not math.isfinite(v):
            continue
        assert Fraction(v) * 100 == Fraction(abs(v) * 100.0) * (1 if v >= 0 else -1), "v * 100 is exact in double"
        c = int(np.rint(abs(v) * 100.0))
        text = ("-" if math.copysign(1.0, v) < 0 else "") + "%d.%02d" % (c // 100, c % 100)
        assert text == "%.2f" % v, (v, text)


@pytest.mark.parametrize("case", on_both("case", [(40, 320), (40, 50), (30, 13)]))
def test_text_commands_and_losses(env, case):
    """the four commands and a zero row, the losses of the issue (and the largest f32, a negative zero, a value past 2^53 hundredths) as
    '%.2f' prints them; a canvas of 50 columns cuts "Command: STRAIGHT" (102 columns), one of 30 rows cuts the second line"""
    dev, _ = env
    BH, BW = case
    geom, cam = (0, 0, BH, BW), _cam(crop_size=float(BW))
    n = len(LOSSES)
    cmd = np.zeros((n, 4), dtype=np.float32)
    for s in range(n):
        if s % 5 != 4:
            cmd[s, s % 5] = 0.5 + s                            # (the first NON-ZERO entry, whatever its value)
    cmd[3, 3], cmd[3, 1] = 1.0, 1.0                            # two entries: the first one counts
    nan = np.full((n, 5, 2), NAN, dtype=np.float32)
    loss = np.array(LOSSES, dtype=np.float32)
    got = _check(dev, 2, cam, geom, 32, 0, 3, (None, np.zeros((n, BH, BW, 7), dtype=np.uint8), nan, nan.copy(), cmd, loss))
    if BW >= 320:
        # every string is on the canvas in full: the white pixels of a line, read back through the glyph table, spell it
        from learningbycheating_amd.training.visuals import FONT
        glyphs = {FONT[7 * i:7 * i + 7]: chr(32 + i) for i in range(95)}
        for s in range(n):
            panel = _slot(got, s, 2, geom, 3)
            for line, want in ((1, _command_text(_command(cmd[s]))), (2, _loss_text(loss[s]))):
                white = (panel[19 * line - 6:19 * line + 1] == WHITE).all(axis=2)
                read = "".join(glyphs[bytes(int("".join("1" if b else "0" for b in white[gy, 6 * i:6 * i + 5]), 2) for gy in range(7))]
                               for i in range(len(want)))
                assert read == want and not white[:, 6 * len(want):].any(), (s, line, read, want)


@pytest.mark.parametrize("where", WHERE)
def test_loss_text_on_random_f32_bit_patterns(env, where):
    dev, _ = env
    BH, BW = 40, 330
    geom, cam = (0, 0, BH, BW), _cam(crop_size=float(BW))
    loss = np.random.RandomState(7).randint(0, 2 ** 32, size=32, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    cmd = np.zeros((32, 4), dtype=np.float32)
    nan = np.full((32, 5, 2), NAN, dtype=np.float32)
    _check(dev, 2, cam, geom, 32, 0, 4, (None, np.zeros((32, BH, BW, 7), dtype=np.uint8), nan, nan.copy(), cmd, loss))


def test_glyphs_in_use_are_distinct():
    from learningbycheating_amd.training.visuals import COMMANDS, FONT
    used = set("Command: Loss: ???naninf-.0123456789") | set("".join(COMMANDS))
    glyph = {ch: FONT[(ord(ch) - 32) * 7:(ord(ch) - 32) * 7 + 7] for ch in used}
    assert not any(glyph[" "]), "the space is blank"
    for ch, g in glyph.items():
        assert ch == " " or any(g), "glyph %r is empty" % ch
        assert all(b < 32 for b in g)
    assert len(set(glyph.values())) == len(glyph), "two characters share a glyph"
    every = [FONT[7 * i:7 * i + 7] for i in range(95)]
    assert len(set(every)) == 95 and all(any(g) for g in every[1:])


# ---- 4. order -------------------------------------------------------------------------------------------------------------------------------
def test_the_twins_order():
    assert _order(np.array([1, NAN, 1, 3, NAN, 0, 3], dtype=np.float32), 7, 32, 1) == [1, 4, 3, 6, 0, 2, 5]
    assert _order(np.array([1, 5, 2, 9], dtype=np.float32), 4, 3, 1) == [1, 2, 0] and _order(np.array([1, 5, 2, 9], dtype=np.float32), 4, 3, 0) == [0, 1, 2]


@pytest.mark.parametrize("case", on_both("case", [(0, 1), (2, 1), (1, 0), (2, 0)]))
def test_panels_are_ordered_by_loss(env, case):
    """equal losses keep their index order, a NaN comes first, only the first `size` samples are candidates (sample 8 has the largest
    loss and is not shown); sort = 0 leaves the order.  Every slot is compared with the panel of the sample that belongs there."""
    dev, _ = env
    mode, sort = case
    geom, cam, n, size = SMALL, CAM_SMALL, 9, 8
    arrays = list(_draw(mode, cam, geom, n, seed=40 + mode, bv="u8"))
    arrays[5] = np.array([1.0, NAN, 1.0, 3.0, NAN, 0.0, 3.0, -INF, 100.0], dtype=np.float32)
    got = _check(dev, mode, cam, geom, size, sort, 4, arrays)
    want = [1, 4, 3, 6, 0, 2, 5, 7] if sort else list(range(8))
    rgb, bv, pred, teach, cmd, loss = arrays
    for k, s in enumerate(want):
        panel = _panel(mode, cam, geom, None if rgb is None else rgb[s], bv[s], pred[s], teach[s], cmd[s], loss[s])
        assert np.array_equal(_slot(got, k, mode, geom, 4), panel), (k, s)


# ---- 5. entry-point refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_entry_point_refusals(env, where):
    from learningbycheating_amd import _lib
    dev, _ = env
    lib = _lib.get()
    geom, cam, n = SMALL, CAM_SMALL, 3
    arrays = _draw(1, cam, geom, n, seed=9, bv="u8")
    rgb, bv, pred, teach, cmd, loss = _dev(dev, *arrays)
    good = lambda mode=1, **kw: _desc(mode, cam, geom, n, 8, 0, 4, **kw)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.lbc_visuals_image_shape(ctypes.byref(good()), ctypes.byref(r), ctypes.byref(c)) == 0
    assert (r.value, c.value) == (2 + 18, 2 + 4 * 38)
    buf, out = guarded((r.value, c.value, 3), dev, fill=FILL, dtype=torch.uint8)
    font = _font(dev)

    def call(d, **kw):
        a = dict(rgb=rgb, bv=bv, pred=pred, teach=teach, cmd=cmd, loss=loss, font=font, out=_lib.ptr(out))
        a.update(kw)
        p = lambda t: t if (t is None or isinstance(t, ctypes.c_void_p)) else _lib.ptr(t)
        return lib.lbc_visuals_render(ctypes.byref(d) if d is not None else None, p(a["rgb"]), p(a["bv"]), p(a["pred"]), p(a["teach"]), p(a["cmd"]),
                                      p(a["loss"]), p(a["font"]), p(a["out"]), _lib.stream_for(out))
    refusals = {"struct_size 0": (dict(d=good(struct_size=0)), "struct_size"),
                "struct_size + 4": (dict(d=good(struct_size=ctypes.sizeof(_lib.VisualsDesc) + 4)), "struct_size"),
                "null descriptor": (dict(d=None), "descriptor"),
                "mode 3": (dict(d=good(mode=3)), "mode"), "mode -1": (dict(d=good(mode=-1)), "mode"),
                "size 0": (dict(d=good(size=0)), "size"), "size 33": (dict(d=good(size=33)), "size"),
                "ncols 0": (dict(d=good(ncols=0)), "ncols"), "N 0": (dict(d=good(N=0)), "N ="),
                "null rgb, mode 1": (dict(d=good(), rgb=None), "rgb"), "null rgb, mode 0": (dict(d=good(mode=0), rgb=None), "rgb"),
                "null pred": (dict(d=good(), pred=None), "pred"), "null teacher": (dict(d=good(), teach=None), "teacher_or_target"),
                "null command": (dict(d=good(), cmd=None), "command"), "null loss": (dict(d=good(), loss=None), "loss"),
                "null font": (dict(d=good(), font=None), "font"), "null out": (dict(d=good(), out=None), "out"),
                "null birdview, mode 2": (dict(d=good(mode=2), bv=None), "birdview"),
                "misaligned out": (dict(d=good(), out=ctypes.c_void_p(out.data_ptr() + 2)), "aligned")}
    for what, (kw, reason) in refusals.items():
        assert call(**kw) == -1, what                          # LBC_EINVAL
        assert reason in lib.lbc_last_error().decode(), (what, lib.lbc_last_error().decode())
        _sync(dev)
        assert bool((buf == FILL).all()), what + ": the output was touched"
    for d in (good(size=0), good(mode=5), good(ncols=0), good(N=0), good(struct_size=8)):
        assert lib.lbc_visuals_image_shape(ctypes.byref(d), ctypes.byref(r), ctypes.byref(c)) == -1
    # what is allowed: no bird-view in modes 0 and 1, no rgb in mode 2
    assert call(good(), bv=None) == 0 and call(good(mode=0), bv=None, pred=pred[:, 0].contiguous(), teach=teach[:, 0].contiguous()) == 0
    _sync(dev)
    assert _fences_ok(buf, out.numel()) and not bool((out == FILL).all())
    # the Python object refuses what the kernel cannot read
    from learningbycheating_amd.training.visuals import PanelRenderer
    v = PanelRenderer(dev, mode=1)
    with pytest.raises(ValueError):
        v.render(rgb, bv, pred[:, 0].contiguous(), teach, cmd, loss)
    with pytest.raises(ValueError):
        v.render(None, bv, pred, teach, cmd, loss)
    with pytest.raises(ValueError):
        v.render(rgb, bv, pred.double(), teach.double(), cmd, loss)
    with pytest.raises(RuntimeError):
        v.image()
    for bad in (dict(mode=3), dict(mode=1, size=0), dict(mode=1, size=33), dict(mode=1, ncols=0)):
        with pytest.raises(ValueError):
            PanelRenderer(dev, **bad)
    assert v.rendered == 0 and (v.size, v.sort) == (8, 0) and (PanelRenderer(dev, mode=0).size, PanelRenderer(dev, mode=2).sort) == (32, 1)


# ---- 6. NativeTrainer.step(visuals=) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("phase", [1, 0, "birdview"])
def test_trainer_renders_behind_the_loss(env, where, phase):
    from learningbycheating_amd.training.visuals import PanelRenderer
    from tests.test_model import _launch_counts
    from tests.test_waypoint_metrics import CAM, _params_and_moments, _TrainerCase
    dev, _ = env
    case = _TrainerCase(dev, phase)
    a, b = case.make(), case.make()                      # b: the twin that never sees a renderer
    v = a.make_visuals()
    mode = {0: 0, 1: 1, "birdview": 2}[phase]
    assert (v.mode, v.size, v.sort, v.ncols, v.rendered) == ((mode,) + {0: (32, 1), 1: (8, 0), 2: (16, 1)}[mode] + (4, 0))
    cam = dict(CAM)

    def twin_of(args, kw, birdview):
        _sync(dev)
        x, cmd = args[0].cpu().numpy(), args[2].cpu().numpy()
        pred, teach = case.seen(a, kw)
        loss = a.loss[:case.n].cpu().numpy()
        if mode == 2:
            geom, rgb, bv = (0, 0) + tuple(x.shape[2:]), None, x
        else:
            bhw = tuple(birdview.shape[2:]) if birdview is not None else (192, 192)
            geom, rgb, bv = tuple(x.shape[2:]) + bhw, x, None if birdview is None else birdview.cpu().numpy()
        return _twin(mode, cam, geom, v.size, v.sort, 4, rgb, bv, pred, teach, cmd, loss, strict=False)
    args, kw = case.inputs(0)
    la = a.step(*args, update=False, train_mode=False, visuals=v, **kw).cpu().clone()
    assert v.rendered == 1
    want = twin_of(args, kw, kw.get("birdview"))
    got = v.image()
    assert v.rendered == 0 and got.dtype == np.uint8 and np.array_equal(got, want)
    assert (got == WHITE).all(axis=2).any() and (got[:, :, 1] == 47).any()
    lb = b.step(*args, update=False, train_mode=False, **kw)        # (also the twin's first eval-mode step: it prepares what a's did)
    _sync(dev)
    assert torch.equal(la, lb.cpu()), "per-sample loss with and without visuals"
    # launches: one more, of a class of its own
    args, kw = case.inputs(1)
    plain = _launch_counts(lambda: b.step(*args, update=False, train_mode=False, **kw))
    drawn = _launch_counts(lambda: a.step(*args, update=False, train_mode=False, visuals=v, **kw))
    assert "visuals" not in plain and drawn == dict(plain, visuals=1)
    buffer = v._last
    # an updating train-mode step: loss, gradients, parameters and moments bit-identical to the twin's
    args, kw = case.inputs(2)
    la, lb = a.step(*args, visuals=v, **kw), b.step(*args, **kw)
    pa, pb = _params_and_moments(a, dev), _params_and_moments(b, dev)
    assert torch.equal(la.cpu(), lb.cpu()) and torch.equal(a.eng.grad_flat.cpu(), b.eng.grad_flat.cpu())
    assert pa.keys() == pb.keys() and all(torch.equal(pa[k], pb[k]) for k in pa) and a.opt.step_count == b.opt.step_count == 1
    assert v._last is buffer and v.rendered == 2, "the image buffer is reused"
    assert np.array_equal(v.image(), twin_of(args, kw, kw.get("birdview")))
    # a renderer of another mode is refused before anything is launched
    wrong = PanelRenderer(dev, a.cam, mode=(mode + 1) % 3)
    with pytest.raises(ValueError):
        a.step(*args, update=False, train_mode=False, visuals=wrong, **kw)
    assert wrong.rendered == 0
    if phase != "birdview":
        # the teacher's waypoints given instead of its bird-view: the canvas is background and dots, crop_size pixels square
        given = tuple(t.clone() for t in a.last_teacher)
        a.step(*args[:3], update=False, train_mode=False, visuals=v, teacher_out=given)
        got = v.image()
        assert np.array_equal(got, twin_of(args, {}, None))
        H, W = args[0].shape[2:]
        canvas = _slot(got, 0, mode, (H, W, 192, 192), 4)[:, W:]
        known = [(0, 47, 0), BLUE, RED, WHITE]
        assert all(tuple(px) in known for px in np.unique(canvas.reshape(-1, 3), axis=0)) and (canvas == BLUE).all(axis=2).any()
    a.phase = "l1_all"                                   # (a phase with nothing to draw)
    with pytest.raises(ValueError):
        a.make_visuals()


# ---- 7. the scripts ------------------------------------------------------------------------------------------------------------------------------
def _read_png(path):
    """an 8-bit RGB PNG with filter type 0 on every scanline -> (H, W, 3) uint8; zlib and struct only"""
    raw = open(str(path), "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        (length,), tag = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        data = raw[pos + 8:pos + 8 + length]
        assert struct.unpack(">I", raw[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        pos += 12 + length
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any(), "filter type 0"
    return rows[:, 1:].reshape(h, w, 3).copy()


@pytest.mark.parametrize("shape", [(5, 7), (1, 1), (31, 64)])
def test_write_png_round_trip(tmp_path, shape):
    from learningbycheating_amd.training.visuals import write_png
    a = np.random.RandomState(3).randint(0, 256, size=shape + (3,)).astype(np.uint8)
    write_png(tmp_path / "a.png", a)
    assert np.array_equal(_read_png(tmp_path / "a.png"), a)
    write_png(str(tmp_path / "b.png"), a[:, ::-1])                # (a view that is not contiguous)
    assert np.array_equal(_read_png(tmp_path / "b.png"), a[:, ::-1])
    for bad in (a.astype(np.float32), a[:, :, :2], a[0]):
        with pytest.raises(ValueError):
            write_png(tmp_path / "c.png", bad)


@pytest.mark.parametrize("module", ["train_birdview", "train_image_phase0", "train_image_phase1"])
def test_script_loops_emulated(env, tmp_path, monkeypatch, module):
    """the scripts' own loop functions on the emulator (the scripts themselves need a GPU: test_scripts_write_pngs): with --visuals a
    pass renders on its logging iterations and reads back once, after its last batch -- with --val-metrics the validation loop still
    reads nothing back inside the loop -- and the files hold the renderer's last grid; without the flag nothing is written or logged
    that was not before"""
    import importlib
    from learningbycheating_amd.bird_view.utils import bz_utils as bzu
    from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
    from learningbycheating_amd.training.data import _SyntheticLoader
    from learningbycheating_amd.training.visuals import PanelRenderer
    from tests.test_waypoint_metrics import PARENT_TRAIN_KEYS, PARENT_VAL_KEYS, PHASE_OF, _TrainerCase
    dev, _ = env
    script = importlib.import_module("learningbycheating_amd.training." + module)
    flags = lambda *argv: script.build_config(script.parse_arguments(["--log_dir", str(tmp_path)] + list(argv)), 0, 1, dev)
    assert "visuals" not in flags() and "visuals_size" not in flags()
    assert flags("--visuals")["visuals"] is True and "visuals_size" not in flags("--visuals") and flags("--visuals", "--visuals-size", "4")["visuals_size"] == 4
    for bad in (("--visuals-size", "4"), ("--visuals", "--visuals-size", "33"), ("--visuals", "--visuals-size", "0")):
        with pytest.raises(SystemExit):
            flags(*bad)
    case = _TrainerCase(dev, PHASE_OF[module])
    trainer = case.make()
    frames = SyntheticFrames(4 * case.n, dev, seed=3, rgb_hw=(32, 64), birdview_hw=(64, 64))
    loader = lambda nb: _SyntheticLoader(frames, case.n, nb)
    base = dict(device=dev, log_iterations=2, rank=0, world_size=1, speed_noise=0.0)
    calls = {"item": 0, "cpu": 0, "render": 0}

    def counting(cls, name, key):
        real = getattr(cls, name)

        def counted(self, *a, **k):
            calls[key] += 1
            return real(self, *a, **k)
        monkeypatch.setattr(cls, name, counted)
    counting(torch.Tensor, "item", "item")
    counting(torch.Tensor, "cpu", "cpu")
    counting(PanelRenderer, "render", "render")
    bzu.log.init(str(tmp_path))
    # without the flag: the parent's keys, no directory, no renderer
    script.train_or_eval(trainer, loader(3), True, dict(base), False, epoch=1)
    plain = dict(calls)
    script.train_or_eval(trainer, loader(2), False, dict(base), False)
    rec = bzu.log.end_epoch()
    assert set(rec) - {"epoch", "time"} == PARENT_VAL_KEYS[module] | PARENT_TRAIN_KEYS[module]
    assert not (tmp_path / "visuals").exists() and calls["render"] == 0 and "_pass_visuals" not in trainer.__dict__
    # --visuals: logging iterations 0 and 2 of a training pass of three render; the one read-back more comes after the pass
    for k in calls:
        calls[k] = 0
    script.train_or_eval(trainer, loader(3), True, dict(base, visuals=True, visuals_size=2), False, epoch=1)
    assert calls == dict(plain, render=2, cpu=plain["cpu"] + 1), (calls, plain)
    # the validation pass with --val-metrics: every batch renders, nothing is read back inside the loop
    for k in calls:
        calls[k] = 0
    script.train_or_eval(trainer, loader(2), False, dict(base, visuals=True, visuals_size=2, val_metrics=True), False)
    assert calls == {"item": 0, "cpu": 2, "render": 2}, calls          # (the metrics record and the image, both after the loop)
    rec = bzu.log.end_epoch()
    assert not any("visual" in k or "birdview" in k for k in rec), "the picture adds no key to the epoch's record"
    mode = {0: 0, 1: 1, "birdview": 2}[PHASE_OF[module]]
    for is_train, name in ((True, "train_birdview_001.png"), (False, "val_birdview_001.png")):
        img = _read_png(tmp_path / "visuals" / name)
        v = trainer._pass_visuals[is_train]
        assert v.rendered == 0 and v.size == 2 and np.array_equal(img, v._last.cpu().numpy())
        assert img.shape == (2 + 66, 2 + 4 * ((64 if mode == 2 else 64 + 64) + 2), 3) and (img == WHITE).all(axis=2).any()
    assert sorted(p.name for p in (tmp_path / "visuals").iterdir()) == ["train_birdview_001.png", "val_birdview_001.png"]
    # another rank renders nothing and writes nothing
    script.train_or_eval(trainer, loader(1), False, dict(base, rank=1, visuals=True), False)
    assert calls["render"] == 2
    bzu.log.rank = 1
    bzu.log.image(is_train=True, birdview=np.zeros((2, 2, 3), dtype=np.uint8))
    bzu.log.rank = 0
    assert len(list((tmp_path / "visuals").iterdir())) == 2


@gpu
def test_scripts_write_pngs(env, tmp_path):
    """the scripts themselves on --synthetic data: epoch 0 (the dry run) and one training epoch with --visuals, then evaluate --visuals"""
    _script("train_birdview", tmp_path, 1, "--visuals", "--visuals-size", "3", "--val-metrics")
    names = sorted(p.name for p in (tmp_path / "visuals").iterdir())
    assert names == ["train_birdview_000.png", "train_birdview_001.png", "val_birdview_000.png", "val_birdview_001.png"]
    for name in names:
        img = _read_png(tmp_path / "visuals" / name)
        assert img.shape == (2 + 194, 2 + 4 * 194, 3) and (img == WHITE).all(axis=2).any() and (img == BLUE).all(axis=2).any()
        assert not _slot(img, 3, 2, (0, 0, 192, 192), 4).any(), "three panels, the fourth slot black"
    cfg = json.loads((tmp_path / "config.json").read_text())
    assert cfg["visuals"] == 1 and cfg["visuals_size"] == 3
    environ = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "learningbycheating_amd.training.evaluate", "--phase", "birdview", "--model_path", str(tmp_path / "model-1.th"),
                        "--synthetic", "64", "--batch_size", "4", "--batches", "2", "--visuals"], env=environ, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    img = _read_png(tmp_path / "visuals.png")
    assert img.shape == (2 + 194, 2 + 4 * 194, 3) and (tmp_path / "metrics.json").exists()


@gpu
def test_script_without_the_flag_writes_what_it_wrote(env, tmp_path):
    from tests.test_waypoint_metrics import PARENT_TRAIN_KEYS, PARENT_VAL_KEYS
    _script("train_birdview", tmp_path, 0)
    assert not (tmp_path / "visuals").exists()
    cfg = json.loads((tmp_path / "config.json").read_text())
    assert "visuals" not in cfg and "visuals_size" not in cfg
    for line in (tmp_path / "log.jsonl").read_text().splitlines():
        assert set(json.loads(line)) - {"epoch", "time"} == PARENT_VAL_KEYS["train_birdview"] | PARENT_TRAIN_KEYS["train_birdview"]
