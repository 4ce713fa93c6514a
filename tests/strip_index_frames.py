"""Frames for the tests of the fused pass's strip index (the one-call step ranks a candidate's current index from the depths of its 64-pixel strip
and the converter's strip offsets instead of loading the index image): test_strip_index_cpu.py holds the premise on the oracle,
test_gpu_strip_index.py the step against the split route.  A helper module; plain numpy.

The expression, as the kernel evaluates it (model()): with cols a multiple of 64, pixel pix lies in strip pix >> 6 of the row-major strip list,
  valid = in_range(raw_to_metres(raw)),   table[strip] = valid pixels in front of the strip,   index = table[pix >> 6] + valid pixels of the
  strip in the lanes below, or -1 where the pixel is not valid.

Shapes that take the path (cols % 64 == 0): 16 x 64 (one strip per row, fewer pixels than one 2048-pixel tile), 40 x 128 (N no multiple of 2048:
the lanes behind the last pixel vote false), 30 x 320 (cols above 256 and no multiple of it: a thread's 256-pixel stride lands on other strips of
other rows), 480 x 640.  Shapes that must fall back: 24 x 32, 120 x 160.

Contents (FAMILIES): every pixel invalid; every pixel valid; validity alternating per pixel; only lane 0, only lane 63 of each strip valid; empty
strips between full ones; the raw values at the converter's range ends and one unit either side, 0 and 65535, over a valid background; a seeded
natural frame (cur_depth_frames).
"""
from __future__ import annotations

import numpy as np

import cur_depth_frames as CF
import depth_frames

SCALE = CF.SCALE
STRIP = depth_frames.STRIP
SHAPES = [(16, 64), (40, 128), (30, 320), (480, 640)]
FALLBACK_SHAPES = [(24, 32), (120, 160)]
FAMILIES = ("all_invalid", "all_valid", "alternating", "lane0", "lane63", "empty_strips", "range_ends", "natural")

camera = CF.camera
configuration = CF.configuration


def range_end_values(conv):
    """[(label, raw value)]: the range ends, one unit either side, 0 and 65535"""
    lo, hi = int(round(conv["min_distance"] / SCALE)), int(round(conv["max_distance"] / SCALE))
    vals = [("zero", 0), ("top", 65535)]
    for name, v in (("min", lo), ("max", hi)):
        vals += [(f"{name}{k:+d}", v + k) for k in (-1, 0, 1)]
    return [(n, v) for n, v in vals if 0 <= v <= 65535]


def frame(kind, rows, cols, seed=0):
    """one uint16 frame (millimetres) of the family"""
    conv, _ = configuration(rows, cols)
    rng = np.random.default_rng([seed, rows, cols, FAMILIES.index(kind)])
    lo, hi = int(conv["min_distance"] / SCALE) + 50, min(int(conv["max_distance"] / SCALE) - 50, 60000)
    near = rng.integers(lo, min(hi, lo + 2500), (rows, cols)).astype(np.uint16)      # valid everywhere
    cc = np.arange(cols)[None, :] + np.zeros((rows, 1), np.int64)
    rr = np.arange(rows)[:, None] + np.zeros((1, cols), np.int64)
    lane, strip = cc % STRIP, (rr * (cols // STRIP) + cc // STRIP) if cols % STRIP == 0 else cc // STRIP
    far = np.uint16(min(65535, int(conv["max_distance"] / SCALE) + 1500))
    if kind == "all_invalid":
        return np.where((rr + cc) % 2 == 0, np.uint16(0), far).astype(np.uint16)
    if kind == "all_valid":
        return near
    if kind == "alternating":
        return np.where((rr + cc) % 2 == 0, near, np.uint16(0)).astype(np.uint16)
    if kind == "lane0":
        return np.where(lane == 0, near, far).astype(np.uint16)
    if kind == "lane63":
        return np.where(lane == STRIP - 1, near, np.uint16(0)).astype(np.uint16)
    if kind == "empty_strips":
        return np.where(strip % 3 == 1, np.uint16(0), near).astype(np.uint16)
    if kind == "range_ends":
        f = near.copy()
        vals = [v for _, v in range_end_values(conv)]
        flat = f.reshape(-1)
        where = rng.permutation(flat.size)[: min(flat.size // 2, 40 * len(vals))]
        flat[where] = np.resize(np.array(vals, np.uint16), where.size)
        return f
    if kind == "natural":
        return CF.make_pair(100 + seed, rows, cols)[1]
    raise ValueError(kind)


def valid_mask(raw, conv):
    return depth_frames.in_range(conv, depth_frames.raw_to_metres(raw, SCALE))


def model(raw, conv):
    """(table [rows * cols / 64], index image) by the kernel's expression"""
    rows, cols = raw.shape
    assert cols % STRIP == 0
    v = valid_mask(raw, conv).reshape(-1, STRIP)                     # one row per (row, strip), in table order
    counts = v.sum(1)
    table = np.cumsum(counts) - counts
    below = np.cumsum(v, axis=1) - v                                 # valid pixels in the lanes below
    index = np.where(v, table[:, None] + below, -1).astype(np.int32)
    return table.astype(np.int32), index.reshape(rows, cols)
