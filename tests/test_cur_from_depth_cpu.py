"""The premise of the fused pass's depth source, held on the oracle (no GPU): in a cloud DepthImageConverter::compute made from a frame,
  * index[pix] is the rank of pixel pix among the frame's valid pixels in row-major order, so a candidate pixel with ci = index[pix] is the pixel
    point ci was unprojected from, and
  * point ci equals, bit for bit, the library's expression for that pixel and its depth (pwn_math.h converter_point, evaluated on the host by
    pwn_hip_debug_converter_points) -- with the identity and with a sensor offset.
The frames are those of the GPU test (tests/cur_depth_frames.py): holes, depths outside the range, a depth step inside a row."""
import ctypes as C

import numpy as np
import pytest

import cur_depth_frames as F
import depth_frames

OFFSET = np.array([[0.0, 0.0, 1.0, 0.1], [-1.0, 0.0, 0.0, 0.05], [0.0, -1.0, 0.0, 0.6], [0.0, 0.0, 0.0, 1.0]], np.float32)      # the robot's camera mount


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lib_params(K, conv, offset):
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    p = _lib.ConverterParams()
    L.pwn_hip_default_converter_params(C.byref(p))
    for i, v in enumerate([K[0], 0, 0, 0, K[1], 0, K[2], K[3], 1]):
        p.K[i] = v
    for k, v in conv.items():
        setattr(p, k, v)
    T = np.eye(4, dtype=np.float32) if offset is None else offset
    for i, v in enumerate(np.asarray(T, np.float32).T.reshape(-1)):      # column-major
        p.sensor_offset[i] = v
    return L, p


@pytest.mark.parametrize("rows,cols", F.SHAPES[:3] + [(480, 640)])
@pytest.mark.parametrize("offset", [None, OFFSET], ids=["identity", "offset"])
def test_a_converted_point_is_the_expression_of_its_own_pixel(oracle, rows, cols, offset):
    conv, _ = F.configuration(rows, cols)
    K = F.camera(rows, cols)
    raw = F.make_pair(5, rows, cols)[1]
    depth = oracle.convert_16u_to_32f(raw, F.SCALE)
    assert np.array_equal(_bits(depth), _bits(depth_frames.raw_to_metres(raw, F.SCALE)))
    cloud, index, _ = oracle.convert(oracle.converter_params(K=K, sensor_offset=offset, **conv), depth)
    points = cloud.arrays()["points"][:, :3]
    n = len(points)
    # what the frames are made to contain
    valid = depth_frames.in_range(conv, depth)
    assert (raw == 0).any() and (~valid & (raw != 0) & (depth > conv["max_distance"])).any() and (~valid & (raw != 0) & (depth < conv["min_distance"])).any()
    assert (np.abs(np.diff(raw.astype(np.int64), axis=1))[(raw[:, 1:] > 0) & (raw[:, :-1] > 0) & valid[:, 1:] & valid[:, :-1]] >= 300).any()
    # the index image is the rank in pixel order
    assert n == int(valid.sum()) and n > rows * cols // 3
    want = np.where(valid, np.cumsum(valid.ravel()).reshape(rows, cols) - 1, -1)
    assert np.array_equal(index, want)
    # the library's expression, on the host
    L, p = _lib_params(K, conv, offset)
    got = np.full((n, 3), np.nan, np.float32)
    idx = np.ascontiguousarray(index, np.int32)
    assert L.pwn_hip_debug_converter_points(C.byref(p), rows, cols, raw.ctypes.data_as(C.c_void_p), F.SCALE, idx.ctypes.data_as(C.c_void_p), n,
                                            got.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(_bits(got), _bits(points)), int((_bits(got) != _bits(points)).any(1).sum())
