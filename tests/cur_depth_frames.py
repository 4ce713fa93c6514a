"""Frames and configurations for the tests of the fused pass's depth source (the one-call step recomputes a candidate's current point from the
depth of its pixel instead of loading it): test_cur_from_depth_cpu.py holds the premise on the oracle, test_gpu_cur_from_depth.py the step
against the split route.  A helper module; plain numpy.

Frames are synth's seeded pairs rendered at the shape (raw 0 holes included), with three patches written into both frames of a pair:
  * a block of raw 0 (a hole larger than the stats window),
  * a block beyond max_distance and a block below min_distance (depths outside the converter's range: no point, index -1),
  * a depth step inside a row: the right part of a band of rows pushed 350 mm back.
"""
from __future__ import annotations

import numpy as np

from g2o_frontend_amd import synth
from oracle import oracle as O

F32 = np.float32
SCALE = 0.001
# rows x cols: cols < 256 with one partial 2048-pixel tile (a thread's 256-pixel stride crosses eight rows); cols < 256 and N no multiple of
# 2048; cols > 256 and no multiple of it; the workload's row geometry
SHAPES = [(24, 32), (120, 160), (60, 300), (480, 640)]


def camera(rows, cols):
    """(fx, fy, cx, cy) of the VGA camera's field of view at this image size"""
    f = synth.K_VGA[0] * cols / 640.0
    return (f, f, (cols - 1) / 2.0, (rows - 1) / 2.0)


def configuration(rows, cols):
    """(converter conf, aligner conf): the reference's VGA files at VGA, its imageScale-4 files below; at 24 x 32 a window that still holds points"""
    if cols >= 640:
        return dict(O.VGA_CONF_CONVERTER), dict(O.VGA_CONF_ALIGNER)
    conv, alig = dict(O.QVGA4_CONF_CONVERTER), dict(O.QVGA4_CONF_ALIGNER)
    if cols < 64:
        conv.update(min_image_radius=2, max_image_radius=4, min_points=6)
    return conv, alig


def patch(frame, conv):
    """the three patches, at places that scale with the shape"""
    rows, cols = frame.shape
    f = frame.copy()
    r0, c0 = rows // 6, cols // 5
    h, w = max(2, rows // 8), max(3, cols // 8)
    f[r0:r0 + h, c0:c0 + w] = 0                                                          # hole
    f[r0:r0 + h, c0 + 2 * w:c0 + 3 * w] = int(conv["max_distance"] / SCALE) + 1500       # beyond the range
    f[rows - r0 - h:rows - r0, c0:c0 + w] = max(1, int(conv["min_distance"] / SCALE) // 2)      # in front of it
    band = slice(rows // 2, rows // 2 + max(2, rows // 6))
    part = f[band, cols // 2 + 1:]
    f[band, cols // 2 + 1:] = np.where(part > 0, np.minimum(part.astype(np.int64) + 350, 65535), 0).astype(np.uint16)      # depth step in a row
    return f


def make_pair(seed, rows, cols):
    """(reference frame, current frame) uint16 millimetres"""
    conv, _ = configuration(rows, cols)
    ref, cur, _ = synth.make_pair(seed, rows, cols, camera(rows, cols))
    return patch(ref, conv), patch(cur, conv)
