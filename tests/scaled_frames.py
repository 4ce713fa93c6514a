"""Depth frames for the batched DepthImage_scale (pwn_core/pwn_static.cpp:5-36) and the *_scaled batch calls: which (source shape, step)
pairs are tested, the uint16 millimetre frames that go in, and numpy statements of the box arithmetic -- the reference's and four wrong ones.

  room    synth.render_depth_mm at the given shape: a smooth scene with 3 % holes.  Block variances are far from maxDepthCov, so it cannot
          tell a wrongly rounded variance from the right one.
  ladder  built for the variance test: every step x step block has a base depth a in 600...5000 mm, its pixels with odd (i * step + j) sit at
          a + delta, delta in 190...210 mm, and 5 % of all pixels are zero.  For an even split (steps 2 and 4) the block variance is
          (delta / 2)^2, which crosses maxDepthCov = 0.01 m^2 at delta = 200 mm; step 3 splits 4 : 5 and crosses at about 201 mm.
  signs   float only: negative depths, zeros and depths beyond max_distance (no NaN, no inf: docs/parity.md records those as undefined
          conversions downstream).
"""
import numpy as np

F32 = np.float32
MAX_DEPTH_COV = 0.01
RAW_SCALE = 0.001

# source shape, step: odd sizes, widths that are / are not a multiple of the 16-byte word, a dropped last row and column, more than one
# workgroup, VGA at the reference's steps, and the step-1 copy
CONFIGS = [((9, 65), 2), ((17, 129), 2), ((34, 136), 2), ((65, 131), 2), ((121, 163), 2), ((121, 163), 3), ((122, 164), 2),
           ((480, 640), 2), ((480, 640), 3), ((480, 640), 4), ((18, 40), 1)]
COUNTS = (1, 7, 8, 9, 25)
POOL = 25                      # frames per (shape, step): the largest call
ROOM_FRAMES = 5                # of which the first are room frames, the rest ladder frames


def config_id(cfg):
    (r, c), s = cfg
    return f"{r}x{c}-step{s}"


def camera(rows, cols):
    """(fx, fy, cx, cy) of a source frame: the VGA camera at 480 x 640, the same field of view at the other shapes"""
    from g2o_frontend_amd import synth
    if (rows, cols) == (480, 640):
        return synth.K_VGA
    f = 525.0 * cols / 640.0
    return (f, f, (cols - 1) / 2.0, (rows - 1) / 2.0)


def room(rows, cols, seed):
    from g2o_frontend_amd import synth
    return synth.render_depth_mm(seed, None, rows, cols, camera(rows, cols), hole_stream=seed)


def ladder(rows, cols, step, seed):
    rng = np.random.default_rng(1000 * step + seed)
    br, bc = rows // step, cols // step
    a = rng.integers(600, 5001, size=(br, bc))
    delta = rng.integers(190, 211, size=(br, bc))
    i, j = np.meshgrid(np.arange(step), np.arange(step), indexing="ij")
    odd = ((i * step + j) % 2 == 1)
    blocks = a[:, :, None, None] + delta[:, :, None, None] * odd[None, None]             # [br, bc, step, step]
    img = np.full((rows, cols), 1000, np.int64)                                            # the dropped last rows / columns
    img[:br * step, :bc * step] = blocks.transpose(0, 2, 1, 3).reshape(br * step, bc * step)
    img[rng.random((rows, cols)) < 0.05] = 0
    return img.astype(np.uint16)


def signs(rows, cols, seed):
    rng = np.random.default_rng(77 + seed)
    img = rng.uniform(0.4, 5.0, (rows, cols)).astype(F32)
    u = rng.random((rows, cols))
    img[u < 0.15] *= F32(-1.0)                      # negative depths: summed, not counted
    img[(u >= 0.15) & (u < 0.25)] = 0.0
    img[(u >= 0.25) & (u < 0.35)] += F32(6.0)       # beyond max_distance
    img[(u >= 0.35) & (u < 0.40)] = F32(-0.0)
    return img


def raw_pool(cfg):
    """the POOL uint16 frames of a configuration: room frames from different seeds, then ladder frames"""
    (rows, cols), step = cfg
    frames = [room(rows, cols, 40 + k) for k in range(ROOM_FRAMES)]
    frames += [ladder(rows, cols, step, k) for k in range(POOL - ROOM_FRAMES)]
    return np.stack(frames)


SIGNS_AT = (6, 13)             # frames of the float pool that are `signs` frames instead of converted uint16 frames


def float_pool(oracle, cfg, raw):
    (rows, cols), _ = cfg
    out = np.stack([oracle.convert_16u_to_32f(f, RAW_SCALE) for f in raw])
    for k in SIGNS_AT:
        out[k] = signs(rows, cols, k)
    return out


def block_counts(raw, step):
    """(rejected by the variance test, kept, with a dropout) blocks of a uint16 frame, from float64 statistics of the metres"""
    rows, cols = raw.shape[0] // step, raw.shape[1] // step
    m = raw[:rows * step, :cols * step].astype(np.float64) * 1e-3
    b = m.reshape(rows, step, cols, step).transpose(0, 2, 1, 3).reshape(rows, cols, step * step)
    npos = (b > 0).sum(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = b.sum(2) / npos
        sigma = (b * b).sum(2) / npos - mu * mu
    rejected = (npos > 0) & (sigma > MAX_DEPTH_COV)
    kept = (npos > 0) & ~rejected
    dropout = (npos > 0) & (npos < step * step)
    return int(rejected.sum()), int(kept.sum()), int(dropout.sum())


def _blocks(src, step):
    src = np.asarray(src, F32)
    rows, cols = src.shape[0] // step, src.shape[1] // step
    return [src[i:rows * step:step, j:cols * step:step] for i in range(step) for j in range(step)]      # the loop's order


def _fma32(a, b, c):
    """round32(a * b + c): the product of two fp32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def box_model(src, step, max_depth_cov=MAX_DEPTH_COV, variant=None):
    """DepthImage_scale in numpy fp32.  variant None is the reference's arithmetic; the others are what a kernel could get wrong:
    "fma_acc2" (acc2 accumulated with a fused multiply-add), "fma_sigma" (sigma with a fused mu * mu), "pairwise" (tree summation) and
    "reciprocal" (acc * (1 / np) instead of the division)."""
    blk = _blocks(src, step)
    cnt = np.zeros(blk[0].shape, np.int32)
    for b in blk:
        cnt += (b > 0)
    if variant == "pairwise":
        s1, s2 = list(blk), [b * b for b in blk]
        while len(s1) > 1:
            s1 = [s1[k] + s1[k + 1] if k + 1 < len(s1) else s1[k] for k in range(0, len(s1), 2)]
            s2 = [s2[k] + s2[k + 1] if k + 1 < len(s2) else s2[k] for k in range(0, len(s2), 2)]
        acc, acc2 = s1[0], s2[0]
    else:
        acc = np.zeros(blk[0].shape, F32); acc2 = np.zeros(blk[0].shape, F32)
        for b in blk:
            acc = acc + b
            acc2 = _fma32(b, b, acc2) if variant == "fma_acc2" else acc2 + b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        npf = cnt.astype(F32)
        if variant == "reciprocal":
            inv = F32(1.0) / npf
            mu, q = acc * inv, acc2 * inv
        else:
            mu, q = acc / npf, acc2 / npf
        sigma = _fma32(-mu, mu, q) if variant == "fma_sigma" else q - mu * mu
    out = np.zeros(blk[0].shape, F32)
    ok = (cnt > 0) & ~(sigma > F32(max_depth_cov))
    out[ok] = mu[ok]
    return out


VARIANT_FLOORS = {"fma_acc2": 10, "fma_sigma": 10, "pairwise": 1000, "reciprocal": 1000}


def same_bits(a, b):
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
