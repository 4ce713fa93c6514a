"""Injected depth frames for the converter's front end (the counting kernels, the offset scan, the integral-image kernels): frames no camera
produces, fed to the shipped kernels through pwn_hip_debug_front_end and to the oracle (unproject, project_intervals, integral_image).  A helper
module of the tests, imported by test_depth_frames_cpu.py and test_gpu_depth_frames.py; plain numpy, no GPU needed to generate.

A batch is MAX_FRAMES frames of one shape, one element type (float32 metres, or uint16 raw values with a scale) and one camera / range
configuration (CONFIGS), because the frames of a launch share one parameter set.  Its frames cycle through FRAME_KINDS:

* "edges": a dense random background with the threshold values (min / max distance exactly and 1, 2 ulps either side, zeros of both signs, a
  negative depth, a denormal, FLT_MAX, +-inf; raw 0, 1, 65535 and the raw values around min / scale and max / scale) and the interval boundaries
  (for every k in 1 .. max_image_radius + 2 the depth nearest to ivx / k and to ivy / k, and 1, 2 ulps -- raw: 1, 2 counts -- either side) at known
  pixels.  Where a frame has no room for all of them, frame i starts at another place of the list.
* "overflow", "nan": values whose float-to-int conversion is undefined in C++ (a NaN depth passes `!(d < min || d > max)`; a quotient of at least
  2^31 needs a tiny min_distance: configuration "tiny").  Batch.undefined_mask() marks exactly these pixels.
* occupancy patterns: all invalid, all valid, the four corners, one column (63, 64, 65, the last), strip 0 only, every other strip, every other
  band, checkerboards, one pixel per row at a moving column.
* "noise": random depths over the whole range with a per-frame share of dropouts.

The frames of a batch have pairwise distinct valid counts wherever the shape and the patterns leave enough pixels to choose from
(Batch.distinct_counts), so that a mix-up of frames in a kernel's decode shows up in the offsets.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F32 = np.float32
STRIP, BAND = 64, 8                      # kIR_Cols, kIR_Rows
MAX_FRAMES = 25
SINGLE_PASS_COUNTS = (1, 7, 8, 9, 16, 17, 24, 25)      # the 8 * ceil(n / 8) frame decode: below, at and above one and two and three groups
LATENCY_COUNTS = (1, 3, 15, 16)
LATENCY, SINGLE_PASS = 0, 1              # PWN_HIP_FRONT_END_LATENCY, PWN_HIP_FRONT_END_SINGLE_PASS
# rows x cols: the smallest shapes that reach each mechanism (1 / 2 / 3 strips, 1 / 2 / 3 / 9 / 17 bands, rows * strips and rows of 1024 and
# above for the chunks of k_row_offsets); float cols % 4 = 0, 1, 2, 3 and raw cols % 8 = 0, 4, odd for the choice of the counting kernel
SHAPES = [(1, 1), (1, 64), (1, 65), (7, 63), (8, 64), (9, 65), (9, 68), (16, 128), (17, 129), (65, 130), (128, 512), (129, 513), (1024, 65),
          (1025, 65)]
STATS = dict(world_radius=0.1, min_image_radius=2, max_image_radius=30, min_points=8)
# K = (fx, fy, cx, cy).  "kinect": the defaults' range, where 0.001f * 10 and the literal 0.01f are different floats.  "wide_x" / "wide_y": 60 m,
# fx > fy resp. fy > fx so that each arm of projectInterval's `px > py` decides; "wide_y" with the second raw scale 1 / 5000.  "tiny": a
# min_distance small enough for a quotient of 2^31 and above.
CONFIGS = {
    "kinect": dict(K=(525.0, 525.0, 63.5, 31.5), min_distance=0.01, max_distance=6.0, scale=0.001),
    "wide_x": dict(K=(590.0, 525.0, 63.5, 31.5), min_distance=0.01, max_distance=60.0, scale=0.001),
    "wide_y": dict(K=(525.0, 590.0, 63.5, 31.5), min_distance=0.5, max_distance=60.0, scale=1.0 / 5000.0),
    "tiny": dict(K=(525.0, 525.0, 63.5, 31.5), min_distance=1e-12, max_distance=6.0, scale=1e-9),
}
FRAME_KINDS = ["noise", "edges", "strip0_only", "alt_strips", "overflow", "empty_bands", "checkerboard", "all_valid", "moving_column", "all_invalid",
               "corners", "col63", "col64", "col65", "last_col", "nan", "noise_sparse", "edges", "alt_strips_odd", "empty_bands_odd",
               "checkerboard_odd", "noise_half", "overflow", "edges", "noise"]
assert len(FRAME_KINDS) == MAX_FRAMES
PATTERNS = ("all_invalid", "all_valid", "corners", "col63", "col64", "col65", "last_col", "strip0_only", "alt_strips", "empty_bands", "checkerboard",
            "moving_column")


def strips_of(cols):
    return (cols + STRIP - 1) // STRIP


def bands_of(rows):
    return (rows + BAND - 1) // BAND


def batch_plan():
    """(rows, cols, element kind, configuration) of every batch: every shape with both element types, the configurations dealt round-robin"""
    names = list(CONFIGS)
    return [(r, c, kind, names[(i + j) % len(names)]) for i, (r, c) in enumerate(SHAPES) for j, kind in enumerate(("float", "raw"))]


def converter_params(O, conf_name, **kw):
    conf = CONFIGS[conf_name]
    return O.converter_params(K=conf["K"], min_distance=conf["min_distance"], max_distance=conf["max_distance"], **dict(STATS, **kw))


def ulps(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
    return v


def interval_scales(conf):
    """K * (R, R, 0): pixels per metre of the world radius at unit depth (pinholepointprojector.h:264-274)"""
    fx, fy, cx, cy = [F32(k) for k in conf["K"]]
    R = F32(STATS["world_radius"])
    return (fx * R + F32(0) * R) + cx * F32(0), (F32(0) * R + fy * R) + cy * F32(0)


def raw_to_metres(raw, scale):
    """DepthImage_convert_16UC1_to_32FC1 (pwn_static.cpp:54-68): raw 0 stays 0 metres"""
    raw = np.asarray(raw)
    return np.where(raw != 0, F32(scale) * raw.astype(F32), F32(0)).astype(F32)


def in_range(conf, d):
    """the validity test of _unProject (pinholepointprojector.h:246-248): NaN passes on both sides"""
    d = np.asarray(d, F32)
    with np.errstate(invalid="ignore"):
        return ~((d < F32(conf["min_distance"])) | (d > F32(conf["max_distance"])))


def quotient(conf, d):
    """projectInterval before its truncation: the larger of ivx * (1 / d) and ivy * (1 / d), as `px > py ? px : py`"""
    ivx, ivy = interval_scales(conf)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / np.asarray(d, F32)
        px, py = ivx * inv, ivy * inv
        return np.where(px > py, px, py).astype(F32)


def undefined(conf, d):
    """valid pixels whose quotient does not fit an int (NaN, or 2^31 and above): (int)quotient is undefined in C++"""
    with np.errstate(invalid="ignore"):
        return in_range(conf, d) & ~(quotient(conf, d) < F32(2.0 ** 31))


# ------------------------------------------------------------------------------------------------ value lists
def threshold_values(conf, kind):
    """[(label, value)]: float32 depths, or raw uint16 values"""
    out = []
    if kind == "float":
        for name in ("min", "max"):
            for k in (-2, -1, 0, 1, 2):
                out.append((f"{name}{k:+d}ulp", ulps(conf[name + "_distance"], k)))
        fm = np.finfo(np.float32)
        out += [("+0", F32(0.0)), ("-0", F32(-0.0)), ("negative", F32(-1.5)), ("denormal", F32(1e-40)), ("flt_max", fm.max), ("+inf", F32(np.inf)),
                ("-inf", F32(-np.inf))]
    else:
        out += [("raw0", 0), ("raw1", 1), ("raw65535", 65535)]
        for name in ("min", "max"):
            q = int(round(float(F32(conf[name + "_distance"])) / float(F32(conf["scale"]))))
            for k in (-1, 0, 1):
                if 0 <= q + k <= 65535:
                    out.append((f"{name}{k:+d}raw", q + k))
    return out


def interval_values(conf, kind):
    """[(label "ivx/k" or "ivy/k", value)]: the boundaries of the truncation for k = 1 .. max_image_radius + 2 on both arms"""
    out = []
    for arm, iv in zip(("ivx", "ivy"), interval_scales(conf)):
        for k in range(1, STATS["max_image_radius"] + 3):
            d0 = float(iv) / k
            if kind == "float":
                for j in (-2, -1, 0, 1, 2):
                    out.append((f"{arm}/{k}", ulps(F32(d0), j)))
            else:
                q = int(round(d0 / float(F32(conf["scale"]))))
                for j in (-2, -1, 0, 1, 2):
                    if 1 <= q + j <= 65535:
                        out.append((f"{arm}/{k}", q + j))
    return out


def overflow_values(conf, kind):
    """depths in range whose quotient is 2^31 or above, and their nearest neighbours below it (defined, the largest ints a float holds)"""
    iv = max(float(v) for v in interval_scales(conf))
    edge = iv / 2.0 ** 31
    if not edge * 0.25 > conf["min_distance"]:
        return []
    if kind == "float":
        vals = [ulps(F32(edge), k) for k in (-3, -2, -1, 0, 1, 2, 3)] + [F32(edge * 0.5), F32(edge * 0.26), F32(conf["min_distance"] * 4)]
    else:
        q = int(edge / float(F32(conf["scale"])))
        vals = sorted({v for v in (1, 2, 3, q - 1, q, q + 1, q + 2) if 1 <= v <= 65535})
    return [("overflow", v) for v in vals]


# ------------------------------------------------------------------------------------------------ frames
class Batch:
    def __init__(self, rows, cols, kind, conf_name, frames, kinds, placed):
        self.rows, self.cols, self.kind, self.conf_name, self.conf = rows, cols, kind, conf_name, CONFIGS[conf_name]
        self.scale = float(F32(self.conf["scale"])) if kind == "raw" else 0.0
        self.frames, self.kinds, self.placed = frames, kinds, placed      # [n][rows][cols]; frame kind; [(label, r, c)] per frame

    def __len__(self):
        return len(self.frames)

    def depth(self, i=None):
        """float32 metres, as both implementations see the frames"""
        f = self.frames if i is None else self.frames[i]
        return raw_to_metres(f, self.scale) if self.kind == "raw" else f

    def valid(self):
        return in_range(self.conf, self.depth())

    def undefined_mask(self):
        return undefined(self.conf, self.depth())

    def counts(self):
        return self.valid().reshape(len(self), -1).sum(1)

    @property
    def distinct_counts(self):
        return len(set(self.counts().tolist())) == len(self)


def _background(rng, conf, kind, shape):
    """random valid depths over the range (raw: as far as 16 bits reach)"""
    lo, hi = conf["min_distance"], conf["max_distance"]
    if kind == "raw":
        s = float(F32(conf["scale"]))
        hi = min(hi, 65535 * s) * 0.999
        lo = max(lo * 1.01, min(0.3, hi / 10), 2 * s)
        return np.clip(np.round(rng.uniform(lo, hi, shape) / s), 1, 65535).astype(np.uint16)
    lo = max(lo * 1.01, 0.3)
    return rng.uniform(lo, hi * 0.999, shape).astype(F32)


def _invalid_fill(rng, conf, kind, shape):
    """what invalid pixels hold: mostly 0, some beyond the range"""
    if kind == "raw":
        far = int(min(65535, round(conf["max_distance"] * 1.5 / float(F32(conf["scale"])))))
        far = far if not in_range(conf, raw_to_metres(far, conf["scale"])) else 0
        return rng.choice(np.array([0, 0, 0, far], np.uint16), shape)
    return rng.choice(np.array([0.0, 0.0, -1.0, conf["max_distance"] * 1.5], F32), shape)


def _pattern(kind, rows, cols, i):
    """(valid mask, pixels the distinct-count pass may flip) of an occupancy pattern"""
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    none = np.zeros((rows, cols), bool)
    if kind == "all_invalid":
        return none, none
    if kind == "all_valid":
        return ~none, none
    if kind == "corners":
        v = none.copy(); v[[0, 0, -1, -1], [0, -1, 0, -1]] = True
        return v, none
    if kind in ("col63", "col64", "col65", "last_col"):
        c = min(cols - 1, {"col63": 63, "col64": 64, "col65": 65, "last_col": cols - 1}[kind])
        v = none.copy(); v[i % rows, c] = True
        return v, cc == c
    if kind == "strip0_only":
        v = cc < STRIP
        return v, v
    if kind in ("alt_strips", "alt_strips_odd"):
        v = (cc // STRIP) % 2 == (1 if kind.endswith("odd") else 0)
        return v, v if v.any() else ~none      # one strip: nothing odd, any pixel may go in
    if kind in ("empty_bands", "empty_bands_odd"):
        v = (rr // BAND) % 2 == (1 if kind.endswith("odd") else 0)
        return v, v if v.any() else ~none
    if kind in ("checkerboard", "checkerboard_odd"):
        v = (rr + cc) % 2 == (1 if kind.endswith("odd") else 0)
        return v, v
    if kind == "moving_column":
        return cc == (5 * rr + 3 * i + 1) % cols, none
    raise KeyError(kind)


def make_batch(rows, cols, kind, conf_name, n=MAX_FRAMES, seed=0):
    conf = CONFIGS[conf_name]
    rng = np.random.default_rng([seed, rows, cols, int(kind == "raw"), list(CONFIGS).index(conf_name)])
    dt = np.uint16 if kind == "raw" else F32
    frames = np.zeros((n, rows, cols), dt)
    kinds, placed_all, free_all = [], [], []
    N = rows * cols
    edge_list = threshold_values(conf, kind) + interval_values(conf, kind)
    over_list = overflow_values(conf, kind)
    nan_list = [("nan", F32(np.nan)), ("nan", -F32(np.nan)), ("nan", np.array(0x7F800001, np.uint32).view(F32))] if kind == "float" else []
    started = 0
    for i in range(n):
        fk = FRAME_KINDS[i % len(FRAME_KINDS)]
        if (fk == "overflow" and not over_list) or (fk == "nan" and not nan_list):
            fk = "edges"
        bg = _background(rng, conf, kind, (rows, cols))
        placed, free = [], np.ones((rows, cols), bool)
        if fk.startswith("noise") or fk in ("edges", "overflow", "nan"):
            drop = {"noise": 0.05, "noise_sparse": 0.9, "noise_half": 0.5}.get(fk, 0.1)
            f = np.where(rng.random((rows, cols)) < drop, _invalid_fill(rng, conf, kind, (rows, cols)), bg).astype(dt)
            values = {"edges": edge_list, "overflow": over_list + threshold_values(conf, kind), "nan": nan_list}.get(fk, [])
            if values:
                m = min(len(values), max(1, N // 3))
                if fk == "nan":
                    m = min(m, 2)                          # a NaN makes everything right of and below it NaN: two per frame
                pix = rng.choice(N, m, replace=False)
                for j, q in enumerate(pix):
                    label, v = values[(started + j) % len(values)]
                    f.flat[q] = v
                    placed.append((label, int(q // cols), int(q % cols)))
                    free.flat[q] = False
                if fk == "edges":
                    started += m
        else:
            v, free = _pattern(fk, rows, cols, i)
            f = np.where(v, bg, _invalid_fill(rng, conf, kind, (rows, cols))).astype(dt)
        frames[i] = f
        kinds.append(fk); placed_all.append(placed); free_all.append(free)
    # pairwise distinct valid counts, where the free pixels allow it
    seen = set()
    for i in sorted(range(n), key=lambda i: bool(free_all[i].any())):      # the frames that cannot change take their counts first
        d = raw_to_metres(frames[i], conf["scale"]) if kind == "raw" else frames[i]
        valid = in_range(conf, d)
        cnt = int(valid.sum())
        for _ in range(4 * n):
            if cnt not in seen:
                break
            vf, nf = np.flatnonzero(free_all[i] & valid), np.flatnonzero(free_all[i] & ~valid)
            if len(vf) and not kinds[i].startswith("col") and kinds[i] != "last_col":
                q = vf[rng.integers(len(vf))]; frames[i].flat[q] = 0; valid.flat[q] = False; cnt -= 1
            elif len(nf):
                q = nf[rng.integers(len(nf))]; frames[i].flat[q] = _background(rng, conf, kind, ())[()]; valid.flat[q] = True; cnt += 1
            else:
                break
            free_all[i].flat[q] = False
        seen.add(cnt)
    return Batch(rows, cols, kind, conf_name, frames, kinds, placed_all)


# ------------------------------------------------------------------------------------------------ the two implementations
def reference(O, batch):
    """the oracle on every frame of a batch: points, index image, interval image, planes, and the offsets as numpy cumulative sums of its validity"""
    p = converter_params(O, batch.conf_name)
    out = []
    S = strips_of(batch.cols)
    for i in range(len(batch)):
        depth = O.convert_16u_to_32f(batch.frames[i], batch.scale) if batch.kind == "raw" else batch.frames[i]
        pts, idx = O.unproject(p, depth)
        itv = O.project_intervals(p, depth)
        planes = O.integral_image(idx, pts)
        valid = idx >= 0
        per_row = valid.sum(1)
        per_strip = np.stack([valid[:, s * STRIP:(s + 1) * STRIP].sum(1) for s in range(S)], 1).ravel()
        out.append(dict(points=pts, index=idx, interval=itv, planes=planes, valid=valid,
                        rowoff=[(np.cumsum(per_row) - per_row).astype(np.int32), (np.cumsum(per_strip) - per_strip).astype(np.int32)]))
    return out


# ------------------------------------------------------------------------------------------------ grouped storage of the integral image
# Written from the sentence in include/pwn_hip_testing.h, not from the library: a frame's 10 N floats (N = rows * cols of the call) are three
# arrays of records -- (x y z n) at float 0, (xx xy xz yy) at float 4 N, (yz zz) at float 8 N -- one record per pixel in each array, pixels in
# row-major order.  Channel ch of the ten planes is therefore component ch % 4 of the record array ch // 4.
GROUPS = ((0, 4), (4, 4), (8, 2))        # (first channel, floats per record) of the three arrays
LEAN_GROUPED = 2                         # PWN_HIP_FRONT_END_LEAN_GROUPED


def _group_positions(N, g):
    """float positions [N][width] of the records of array g inside a frame's 10 N floats"""
    width = GROUPS[g][1]
    return 4 * g * N + np.arange(N)[:, None] * width + np.arange(width)[None, :]


def planes_to_grouped(planes):
    """[..., 10, rows, cols] planes -> [..., 10 * rows * cols] floats in the grouped form (any N, odd ones included)"""
    planes = np.asarray(planes, F32)
    lead, N = planes.shape[:-3], planes.shape[-2] * planes.shape[-1]
    flat = planes.reshape(lead + (10, N))
    out = np.empty(lead + (10 * N,), F32)
    for g, (first, width) in enumerate(GROUPS):
        out[..., _group_positions(N, g)] = np.moveaxis(flat[..., first:first + width, :], -2, -1)
    return out


def grouped_to_planes(buf, rows, cols):
    """the inverse: [..., 10 * rows * cols] floats in the grouped form -> [..., 10, rows, cols] planes"""
    buf = np.asarray(buf, F32)
    N = rows * cols
    lead = buf.shape[:-1]
    assert buf.shape[-1] == 10 * N
    out = np.empty(lead + (10, N), F32)
    for g, (first, width) in enumerate(GROUPS):
        out[..., first:first + width, :] = np.moveaxis(buf[..., _group_positions(N, g)], -1, -2)
    return out.reshape(lead + (10, rows, cols))


def run_gpu(ctx, p, batch, frames, path, lean, device_offset=None):
    """one pwn_hip_debug_front_end call on the given frames of the batch.  lean = 0, 1 or 2 as the hook takes it; with 2 the integral image comes
    back in the grouped form and is handed on as planes (grouped_to_planes).  device_offset: None = host frames; k = the frames in device
    memory, each k elements behind a 256-byte boundary"""
    from g2o_frontend_amd import api
    n, rows, cols = len(frames), batch.rows, batch.cols
    N = rows * cols
    src = np.ascontiguousarray(batch.frames[list(frames)])
    keep = None
    if device_offset is None:
        ptrs = [src[i].ctypes.data for i in range(n)]
    else:
        item = src.dtype.itemsize
        pitch = ((N + device_offset) * item + 255) // 256 * 256
        block = np.zeros(n * pitch, np.uint8)
        for i in range(n):
            block[i * pitch + device_offset * item: i * pitch + (device_offset + N) * item] = src[i].view(np.uint8).ravel()
        keep = ctx.upload(block)
        ptrs = [keep.data_ptr() + i * pitch + device_offset * item for i in range(n)]
    clouds = [api.Cloud(ctx, N) for _ in range(n)]
    noff = rows * (strips_of(cols) if path == SINGLE_PASS else 1)
    integral = np.full((n, 10, rows, cols), -7.0, F32)
    index = np.full((n, rows, cols), -7, np.int32)
    rowoff = np.full((n, noff), -7, np.int32)
    interval = None if lean else np.full((n, rows, cols), -7, np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ctx.check(ctx._L.pwn_hip_debug_front_end(ctx.h, C.addressof(p), (C.c_void_p * n)(*ptrs), batch.scale, n, rows, cols, path, int(lean),
                                             (C.c_void_p * n)(*[c.h.value for c in clouds]), vp(integral), vp(index), vp(interval), vp(rowoff)))
    if lean == LEAN_GROUPED:
        integral = grouped_to_planes(integral.reshape(n, 10 * N), rows, cols)
    sizes = [c.size() for c in clouds]
    points = None if lean else [c.arrays()["points"] for c in clouds]
    if keep is not None:
        keep.free()
    return dict(planes=integral, index=index, interval=interval, rowoff=rowoff, points=points, sizes=sizes)


def same_bits(a, b):
    """same bits, or NaN on both sides"""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def compare(batch, frames, ref, got, path, lean):
    """every output of a front-end call against the oracle's (lean = 2 as lean = 1: neither stores points or intervals); returns {field: number
    of differing elements}"""
    und = batch.undefined_mask()
    bad = dict(index=0, rowoff=0, planes=0, interval=0, points=0)
    for j, i in enumerate(frames):
        r = ref[i]
        bad["index"] += int((r["index"] != got["index"][j]).sum())
        bad["rowoff"] += int((r["rowoff"][path] != got["rowoff"][j]).sum())
        bad["planes"] += int((~same_bits(r["planes"], got["planes"][j])).sum())
        if lean:
            assert got["sizes"][j] == 0, "a lean front end stores no points: the cloud must report none"
        else:
            bad["interval"] += int(((r["interval"] != got["interval"][j]) & ~und[i]).sum())
            if got["points"][j].shape != r["points"].shape:
                bad["points"] += max(len(r["points"]), 1)
            else:
                bad["points"] += int((~same_bits(r["points"][:, :3], got["points"][j][:, :3])).sum())
    return bad


# ------------------------------------------------------------------------------------------------ against float64
def channel_terms(index, points):
    """the ten fp32 terms per pixel (PointAccumulator::operator+=, pointaccumulator.h:56-59): p, 1, the upper triangle of p p^T; 0 where no point"""
    v = index >= 0
    P = np.zeros(index.shape + (3,), F32)
    P[v] = points[index[v], :3]
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([x, y, z, v.astype(F32), x * x, x * y, x * z, y * y, y * z, z * z])


def float64_ratio(planes, terms):
    """max over elements of |plane - sum64| / (gamma_n * sum |term|), n = r + c + 1: every term of element (r, c) passes through at most c additions
    of its row chain and r of the column chain, so the sequential sums obey the standard bound with gamma_n = n u / (1 - n u), u = 2^-24.
    Elements whose sums are not finite are left out; an element with sum |term| = 0 must be exactly 0."""
    t64 = terms.astype(np.float64)
    with np.errstate(all="ignore"):
        s64 = np.cumsum(np.cumsum(t64, axis=2), axis=1)
        a64 = np.cumsum(np.cumsum(np.abs(t64), axis=2), axis=1)
    rows, cols = terms.shape[1:]
    n = (np.arange(rows)[:, None] + np.arange(cols)[None, :] + 1).astype(np.float64)
    u = 2.0 ** -24
    bound = (n * u / (1 - n * u))[None] * a64
    fin = np.isfinite(a64) & (a64 < 1e37)
    err = np.abs(planes.astype(np.float64) - s64)
    assert not (err[fin & (a64 == 0)] != 0).any(), "a plane element with no terms is not 0"
    sel = fin & (a64 > 0)
    return float((err[sel] / bound[sel]).max()) if sel.any() else 0.0
