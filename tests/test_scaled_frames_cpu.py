"""The generator of tests/scaled_frames.py held to what it claims, on the CPU (oracle and numpy only): the ladder frames put blocks on
both sides of DepthImage_scale's variance test and have dropouts, they tell four wrong ways of doing the block arithmetic from the
reference's, the room frame does not tell the two fused ones apart (which is why the ladder exists), the numpy model equals the oracle bit for
bit on every frame the GPU file uses, and the oracle's clouds of the scaled frames have normals to compare."""
import numpy as np
import pytest

import numpy_reference_model as M
import scaled_frames as S


@pytest.mark.parametrize("cfg", [c for c in S.CONFIGS if c[1] > 1], ids=S.config_id)
def test_every_ladder_frame_has_rejected_kept_and_dropout_blocks(cfg):
    (rows, cols), step = cfg
    for k in range(S.POOL - S.ROOM_FRAMES if rows * cols < 100000 else 3):
        rej, kept, drop = S.block_counts(S.ladder(rows, cols, step, k), step)
        if k == 0:
            print(f"  ladder {rows}x{cols} step {step}: {rej} rejected, {kept} kept, {drop} with a dropout")
        assert rej >= 10 and kept >= 10 and drop >= 10, (cfg, k, rej, kept, drop)


@pytest.mark.parametrize("step", [2, 3, 4])
def test_the_ladder_tells_wrong_arithmetic_apart_and_the_room_does_not(oracle, step):
    lad = oracle.convert_16u_to_32f(S.ladder(480, 640, step, 0), S.RAW_SCALE)
    rm = oracle.convert_16u_to_32f(S.room(480, 640, 40), S.RAW_SCALE)
    want_l, want_r = oracle.depth_scale(lad, step), oracle.depth_scale(rm, step)
    assert S.same_bits(S.box_model(lad, step), want_l) and S.same_bits(S.box_model(rm, step), want_r)
    for variant, floor in S.VARIANT_FLOORS.items():
        dl = int((S.box_model(lad, step, variant=variant).view(np.uint32) != want_l.view(np.uint32)).sum())
        dr = int((S.box_model(rm, step, variant=variant).view(np.uint32) != want_r.view(np.uint32)).sum())
        print(f"  step {step} {variant}: {dl} ladder pixels differ, {dr} room pixels")
        assert dl >= floor, (step, variant, dl)
        if variant.startswith("fma"):
            assert dr == 0, (step, variant, dr)


@pytest.mark.parametrize("cfg", S.CONFIGS, ids=S.config_id)
def test_numpy_model_equals_oracle_on_every_frame_of_the_gpu_file(oracle, cfg):
    _, step = cfg
    raw = S.raw_pool(cfg)
    flt = S.float_pool(oracle, cfg, raw)
    for k in range(S.POOL):
        d = oracle.convert_16u_to_32f(raw[k], S.RAW_SCALE)
        assert S.same_bits(M.depth_scale(d, step), oracle.depth_scale(d, step)), (cfg, k)
        if k in S.SIGNS_AT:
            assert (flt[k] < 0).any() and (flt[k] == 0).any() and (flt[k] > 6).any() and np.isfinite(flt[k]).all()
            assert S.same_bits(M.depth_scale(flt[k], step), oracle.depth_scale(flt[k], step)), (cfg, k, "signs")


@pytest.mark.parametrize("cfg", S.CONFIGS, ids=S.config_id)
def test_oracle_clouds_of_the_scaled_room_frames_have_normals(oracle, cfg):
    """QVGA4_CONF_CONVERTER with the scaled camera gives clouds whose points nearly all carry a normal, at every shape: the cloud comparisons of
    the GPU file compare something"""
    from g2o_frontend_amd import synth
    (rows, cols), step = cfg
    cp = oracle.converter_params(K=synth.scaled_K(S.camera(rows, cols), step), **oracle.QVGA4_CONF_CONVERTER)
    d = oracle.depth_scale(oracle.convert_16u_to_32f(S.room(rows, cols, 40), S.RAW_SCALE), step)
    c, _, _ = oracle.convert(cp, d)
    a = c.arrays()
    normals = int((np.abs(a["normals"][:, :3]).sum(1) > 0).sum())
    print(f"  {rows}x{cols} step {step}: {len(a['points'])} points, {normals} with a normal")
    assert len(a["points"]) >= 100 and normals >= 0.8 * len(a["points"]), (cfg, len(a["points"]), normals)
