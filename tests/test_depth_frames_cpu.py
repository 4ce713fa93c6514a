"""The injected depth frames of tests/depth_frames.py held to their coverage with the oracle and numpy only (no GPU): the thresholds and interval
boundaries are hit from both sides, every pattern and shape is there, the inputs tell a wrong carry, summation order, validity test or interval
expression from the right one, and the oracle's planes obey the float64 bound the GPU test applies to the device's."""
import numpy as np
import pytest

import depth_frames as D

F32 = np.float32


@pytest.fixture(scope="module")
def batches(oracle):
    """every batch of the plan with the oracle's results, made once"""
    out = []
    for rows, cols, kind, conf in D.batch_plan():
        b = D.make_batch(rows, cols, kind, conf)
        out.append((b, D.reference(oracle, b)))
    return out


def _placed(batches, pred):
    """(batch, frame, label, r, c, reference of the frame) of every placed value whose label satisfies pred"""
    for b, ref in batches:
        for i, pl in enumerate(b.placed):
            for label, r, c in pl:
                if pred(label):
                    yield b, i, label, r, c, ref[i]


def test_plan_covers_shapes_patterns_and_element_types(batches):
    plan = D.batch_plan()
    assert {(r, c) for r, c, _, _ in plan} == set(D.SHAPES) and {k for _, _, k, _ in plan} == {"float", "raw"}
    assert {c % 4 for r, c, k, _ in plan if k == "float"} == {0, 1, 2, 3}
    assert {0, 4} <= {c % 8 for r, c, k, _ in plan if k == "raw"} and any(c % 2 for r, c, k, _ in plan if k == "raw")
    rs = {r * D.strips_of(c) for r, c in D.SHAPES}
    assert 1024 in rs and any(v > 1024 for v in rs) and {1024, 1025} <= {r for r, _ in D.SHAPES}
    assert any(D.bands_of(r) > 8 and D.strips_of(c) > 1 for r, c in D.SHAPES)
    for conf in D.CONFIGS:                                  # every configuration meets both element types and a multi-strip, multi-band shape
        mine = [(r, c, k) for r, c, k, cf in plan if cf == conf]
        assert {k for _, _, k in mine} == {"float", "raw"} and any(D.strips_of(c) > 1 and D.bands_of(r) > 1 for r, c, _ in mine), conf
    for b, ref in batches:
        assert set(D.PATTERNS) <= set(b.kinds) and "noise" in b.kinds and "edges" in b.kinds
        assert len(b) == D.MAX_FRAMES >= max(D.SINGLE_PASS_COUNTS + D.LATENCY_COUNTS)
        assert np.array_equal(np.stack([r["valid"] for r in ref]), b.valid()), "numpy's validity is not the oracle's"
        cnt = b.counts()
        if b.rows * b.cols >= 512:
            assert b.distinct_counts, (b.rows, b.cols, b.kind, sorted(cnt.tolist()))
        else:                                               # tiny shapes: as many different counts as there are pixels to choose from
            assert len(set(cnt.tolist())) >= min(len(b), b.rows * b.cols + 1) // 2
        for i in range(1, len(b)):
            assert b.rows * b.cols < 512 or not np.array_equal(b.frames[i], b.frames[i - 1])
        if b.rows * b.cols < 64:
            continue
        # the patterns are what they say (on a single pixel the distinct counts leave nothing of them)
        v = b.valid()
        k = b.kinds
        assert not v[k.index("all_invalid")].any() and v[k.index("all_valid")].all()
        s0 = v[k.index("strip0_only")]
        assert not s0[:, D.STRIP:].any() and s0[:, :D.STRIP].any()
        if D.strips_of(b.cols) > 2:
            a = v[k.index("alt_strips")]
            assert not a[:, D.STRIP:2 * D.STRIP].any() and a[:, 2 * D.STRIP:].any()
        if D.bands_of(b.rows) > 2:
            e = v[k.index("empty_bands")]
            assert not e[D.BAND:2 * D.BAND].any() and e[2 * D.BAND:].any()
        mc = v[k.index("moving_column")]
        assert (mc.sum(1) == 1).all() and (b.cols == 1 or b.rows == 1 or len(set(mc.argmax(1).tolist())) > 1)
        for name, col in (("col63", 63), ("col64", 64), ("col65", 65), ("last_col", b.cols - 1)):
            f = v[k.index(name)]
            col = min(col, b.cols - 1)
            assert f[:, col].any() and not np.delete(f, col, axis=1).any()


def test_thresholds_are_hit_on_both_sides(batches):
    """pixels exactly on min / max distance and 1, 2 ulps either side (raw: the counts around min / scale and max / scale), and the special values,
    by the oracle's own validity"""
    cover = {}
    for b, i, label, r, c, ref in _placed(batches, lambda s: "/" not in s and s not in ("nan", "overflow")):
        key = (b.conf_name, b.kind, label)
        n, v = cover.get(key, (0, 0))
        cover[key] = (n + 1, v + int(ref["valid"][r, c]))
    for conf in D.CONFIGS:
        for label in ("min-2ulp", "min-1ulp", "max+1ulp", "max+2ulp", "+0", "-0", "negative", "denormal", "flt_max", "+inf", "-inf"):
            n, v = cover[(conf, "float", label)]
            assert n >= 3 and v == 0, (conf, label, n, v)
        for label in ("min+0ulp", "min+1ulp", "min+2ulp", "max-2ulp", "max-1ulp", "max+0ulp"):
            n, v = cover[(conf, "float", label)]
            assert n >= 3 and v == n, (conf, label, n, v)
        raw = {k[2]: nv for k, nv in cover.items() if k[0] == conf and k[1] == "raw"}
        assert raw["raw0"][0] >= 3 and raw["raw0"][1] == 0 and raw["raw1"][0] >= 3 and raw["raw65535"][0] >= 3
        for name in ("min", "max"):
            side = [raw[f"{name}{k:+d}raw"] for k in (-1, 0, 1) if f"{name}{k:+d}raw" in raw]
            if len(side) == 3:                              # the threshold is within 16 bits at this scale: both sides are there
                assert any(v == 0 for _, v in side) and any(v == n for n, v in side), (conf, name, side)
    reach = {(conf, name) for conf in D.CONFIGS for name in ("min", "max") if (conf, "raw", f"{name}+1raw") in cover}
    assert {("kinect", "min"), ("kinect", "max"), ("wide_x", "max"), ("wide_y", "min")} <= reach
    k = D.CONFIGS["kinect"]
    assert F32(k["scale"]) * F32(10) != F32(k["min_distance"])      # 0.001f * 10 is not the literal 0.01f: raw 10 decides by the product
    print("threshold coverage (configuration, element type, label): (pixels, valid)")
    for key in sorted(cover):
        print("  ", key, cover[key])


def test_interval_boundaries_are_hit_on_both_sides(batches, oracle):
    """for every k in 1 .. max_image_radius + 2 the oracle's interval takes both k and k - 1 on the pixels placed around iv / k, on the arm that
    decides: ivx where fx > fy ("wide_x"), ivy where fy > fx ("wide_y")"""
    kmax = D.STATS["max_image_radius"] + 2
    for conf, arm in (("wide_x", "ivx"), ("wide_y", "ivy")):
        ivx, ivy = D.interval_scales(D.CONFIGS[conf])
        assert (ivx > ivy) == (arm == "ivx")
        for kind in ("float", "raw"):
            seen = {}
            for b, i, label, r, c, ref in _placed(batches, lambda s: s.startswith(arm + "/")):
                if b.conf_name == conf and b.kind == kind and ref["valid"][r, c]:
                    seen.setdefault(int(label.split("/")[1]), []).append(int(ref["interval"][r, c]))
            hit = [k for k in range(1, kmax + 1) if k in seen and {k, k - 1} <= set(seen[k])]
            print(f"interval boundaries {conf} {kind}: k hit on both sides {hit}; pixels per k {[len(seen.get(k, [])) for k in range(1, kmax + 1)]}")
            if kind == "float":
                assert hit == list(range(1, kmax + 1)), (conf, hit)
            else:                                           # raw counts are coarser than ulps: the boundary is still straddled where 16 bits reach it
                reachable = [k for k in range(1, kmax + 1) if float(max(ivx, ivy)) / k / D.CONFIGS[conf]["scale"] < 65533]
                assert set(reachable) <= set(hit), (conf, reachable, hit)


def test_undefined_conversions_are_the_placed_ones(batches):
    """the mask of undefined float-to-int conversions holds NaN and overflow pixels the generator placed (Batch.placed) and nothing else"""
    n_nan = n_over = 0
    for b, ref in batches:
        und = b.undefined_mask()
        placed = np.zeros_like(und)
        for i, pl in enumerate(b.placed):
            for label, r, c in pl:
                if D.undefined(b.conf, b.depth(i)[r, c]):      # "nan", "overflow", and raw 1 where the scale makes it one
                    placed[i, r, c] = True
        assert np.array_equal(und, placed)
        d = b.depth()
        n_nan += int(np.isnan(d[und]).sum()); n_over += int((~np.isnan(d[und])).sum())
        if b.conf_name == "tiny":
            assert (~np.isnan(d[und])).sum() >= 3, "no overflow pixel in a batch of the tiny-min_distance configuration"
        for i in range(len(b)):                             # a NaN depth is a valid pixel to the oracle
            assert ref[i]["valid"][np.isnan(d[i])].all()
    print(f"undefined conversions: {n_nan} NaN pixels, {n_over} pixels with a quotient of 2^31 or more")
    assert n_nan >= 20 and n_over >= 20


# ------------------------------------------------------------------------------------------------ sensitivity of the inputs
def _scan_rows(t, reset_at_strips=False, hillis_steele=False):
    if hillis_steele:                                       # a parallel scan's order: log2 steps of pairwise additions
        a = t.copy(); off = 1
        while off < a.shape[-1]:
            a[..., off:] = a[..., off:] + a[..., :-off].copy(); off *= 2
        return a
    if reset_at_strips:
        return np.concatenate([np.cumsum(t[..., s:s + D.STRIP], axis=-1, dtype=F32) for s in range(0, t.shape[-1], D.STRIP)], -1)
    return np.cumsum(t, axis=-1, dtype=F32)


def _scan_cols(t, reset_at_bands=False):
    if reset_at_bands:
        return np.concatenate([np.cumsum(t[:, s:s + D.BAND], axis=1, dtype=F32) for s in range(0, t.shape[1], D.BAND)], 1)
    return np.cumsum(t, axis=1, dtype=F32)


def test_inputs_tell_wrong_carries_and_orders_from_the_right_ones(batches):
    """numpy models of the planes from the oracle's own terms: the sequential one reproduces the oracle bit for bit; one that restarts the row sums
    at strip boundaries differs on every multi-strip shape, one that restarts the column sums at band boundaries on every multi-band shape, one
    that sums the rows in a parallel scan's pairwise order on every noise frame (dense, half and sparse) of every shape but 1 x 1, whose rows
    hold one term and so have one order"""
    for b, ref in batches:
        differs = dict(strip=False, band=False)
        for i, r in enumerate(ref):
            t = D.channel_terms(r["index"], r["points"])
            with np.errstate(all="ignore"):
                good = _scan_cols(_scan_rows(t))
                assert D.same_bits(good, r["planes"]).all(), "the sequential numpy model is not the oracle"
                differs["strip"] |= not D.same_bits(_scan_cols(_scan_rows(t, reset_at_strips=True)), r["planes"]).all()
                differs["band"] |= not D.same_bits(_scan_cols(_scan_rows(t), reset_at_bands=True), r["planes"]).all()
                if b.kinds[i].startswith("noise"):
                    pair = not D.same_bits(_scan_cols(_scan_rows(t, hillis_steele=True)), r["planes"]).all()
                    assert pair == (b.cols > 1), (b.rows, b.cols, b.kind, b.kinds[i])
        assert differs["strip"] == (D.strips_of(b.cols) > 1), (b.rows, b.cols, b.kind)
        assert differs["band"] == (D.bands_of(b.rows) > 1), (b.rows, b.cols, b.kind)


def test_inputs_tell_the_validity_test_and_the_interval_expression(batches, oracle):
    """The reference writes the validity as `d < min || d > max -> invalid` (NaN valid) and the interval as reciprocal-then-multiply
    (pinholepointprojector.h:246-248, 264-274; the oracle restates both).  `d >= min && d <= max` differs in the valid count on the NaN frames;
    one division instead of 1 / d and a product differs in at least one interval of every float configuration."""
    nan_frames = 0
    one_division = {}
    for b, ref in batches:
        d = b.depth()
        ivx, ivy = D.interval_scales(b.conf)
        for i, r in enumerate(ref):
            with np.errstate(all="ignore"):
                strict = (d[i] >= F32(b.conf["min_distance"])) & (d[i] <= F32(b.conf["max_distance"]))
                if np.isnan(d[i]).any():
                    nan_frames += 1
                    assert strict.sum() < r["valid"].sum()
                else:
                    assert np.array_equal(strict, r["valid"])
                ok = r["valid"] & ~D.undefined(b.conf, d[i])
                px, py = ivx / d[i], ivy / d[i]
                div = np.where(px > py, px, py)
                one = np.where(ok, np.where(ok, div, 0).astype(np.int32), r["interval"])
            # reciprocal-then-multiply in numpy is the oracle
            q = D.quotient(b.conf, d[i])
            assert np.array_equal(np.where(ok, np.where(ok, q, 0).astype(np.int32), r["interval"]), r["interval"])
            one_division[(b.conf_name, b.kind)] = one_division.get((b.conf_name, b.kind), 0) + int((one != r["interval"]).sum())
    print("intervals that one division gets differently:", one_division)
    assert nan_frames >= 10
    for conf in D.CONFIGS:
        assert one_division[(conf, "float")] >= 1, conf


def test_oracle_planes_against_float64(batches):
    """|plane - float64 sum of the same fp32 terms| <= gamma_n * sum |term|, n = r + c + 1 (depth_frames.float64_ratio); the worst ratio is printed
    for docs/parity.md"""
    worst = {}
    for b, ref in batches:
        for i, r in enumerate(ref):
            ratio = D.float64_ratio(r["planes"], D.channel_terms(r["index"], r["points"]))
            worst[b.kinds[i]] = max(worst.get(b.kinds[i], 0.0), ratio)
            assert ratio <= 1.0, (b.rows, b.cols, b.kind, i, ratio)
    print("worst |plane - sum64| / (gamma_n sum|term|) per frame kind:", {k: round(v, 4) for k, v in sorted(worst.items())})


# ------------------------------------------------------------------------------------------------ the grouped layout, stated a second time
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (4, 6), (61, 257)])
def test_grouped_layout_round_trip(shape):
    """planes -> grouped -> planes gives the planes back, bit for bit, for odd and even N and with leading frame dimensions"""
    rng = np.random.default_rng(3)
    rows, cols = shape
    planes = rng.standard_normal((2, 3, 10, rows, cols)).astype(F32)
    planes[0, 0, 3, 0, 0] = np.nan; planes[1, 2, 9, -1, -1] = -0.0
    buf = D.planes_to_grouped(planes)
    assert buf.shape == (2, 3, 10 * rows * cols)
    back = D.grouped_to_planes(buf, rows, cols)
    assert back.shape == planes.shape and np.array_equal(back.view(np.uint32), planes.view(np.uint32))
    one = D.planes_to_grouped(planes[1, 2])
    assert np.array_equal(one.view(np.uint32), buf[1, 2].view(np.uint32))
    assert np.array_equal(D.grouped_to_planes(one, rows, cols).view(np.uint32), planes[1, 2].view(np.uint32))


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (4, 6)])
def test_grouped_layout_puts_every_element_where_the_header_says(shape):
    """the value 1000 * ch + pix lands at float 4 * (ch // 4) * N + pix * width + ch % 4, width = 4, 4, 2 floats per record of the three arrays:
    (x y z n) at float 0, (xx xy xz yy) at float 4 N, (yz zz) at float 8 N (include/pwn_hip_testing.h)"""
    rows, cols = shape
    N = rows * cols
    ch, pix = np.meshgrid(np.arange(10), np.arange(N), indexing="ij")
    buf = D.planes_to_grouped((1000 * ch + pix).astype(F32).reshape(10, rows, cols))
    seen = np.zeros(10 * N, bool)
    for c in range(10):
        width = (4, 4, 2)[c // 4]
        for q in range(N):
            at = 4 * (c // 4) * N + q * width + c % 4
            assert buf[at] == 1000 * c + q, (c, q, at, buf[at])
            seen[at] = True
    assert seen.all(), "the ten channels of N pixels fill the 10 N floats exactly"
