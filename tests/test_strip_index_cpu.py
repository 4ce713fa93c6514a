"""The premise of the fused pass's strip index, held on the oracle (no GPU): in a cloud DepthImageConverter::compute made from a frame whose width
is a multiple of 64, the index of a valid pixel is
    (valid pixels in front of its 64-column strip, in row-major strip order)  +  (valid pixels of the strip to its left),
with validity the range test on the converted depth -- what the kernel evaluates from one table word, the wave's raw depths and one ballot
(tests/strip_index_frames.py model()).  The frames are those of the GPU test: every content family at every shape that takes the path."""
import numpy as np
import pytest

import strip_index_frames as S

CASES = [(r, c, k) for r, c in S.SHAPES[:3] for k in S.FAMILIES] + [(480, 640, "natural")]


@pytest.mark.parametrize("rows,cols,kind", CASES)
def test_table_word_plus_rank_is_the_converters_index(oracle, rows, cols, kind):
    conv, _ = S.configuration(rows, cols)
    raw = S.frame(kind, rows, cols)
    depth = oracle.convert_16u_to_32f(raw, S.SCALE)
    _, want, _ = oracle.convert(oracle.converter_params(K=S.camera(rows, cols), **conv), depth)
    table, index = S.model(raw, conv)
    assert np.array_equal(index, want), int((index != want).sum())
    # the table is the exclusive count of valid pixels, read off the oracle's image
    valid = (want >= 0).reshape(-1)
    before = np.cumsum(valid) - valid
    assert np.array_equal(table, before[:: S.STRIP])
    assert table[0] == 0 and (np.diff(table) >= 0).all() and (np.diff(table) <= S.STRIP).all()


@pytest.mark.parametrize("rows,cols", S.SHAPES[:3])
def test_every_family_occurs(rows, cols):
    conv, _ = S.configuration(rows, cols)
    v = {k: S.valid_mask(S.frame(k, rows, cols), conv) for k in S.FAMILIES}
    strips = lambda m: m.reshape(-1, S.STRIP)      # noqa: E731
    assert not v["all_invalid"].any() and v["all_valid"].all()
    assert (v["alternating"][:, 1:] != v["alternating"][:, :-1]).all() and (v["alternating"][1:] != v["alternating"][:-1]).all()
    assert strips(v["lane0"])[:, 0].all() and not strips(v["lane0"])[:, 1:].any()
    assert strips(v["lane63"])[:, -1].all() and not strips(v["lane63"])[:, :-1].any()
    per = strips(v["empty_strips"]).sum(1)
    assert set(per.tolist()) == {0, S.STRIP} and (per[1::3] == 0).all() and per[0] == S.STRIP
    if len(per) > 2:
        assert per[2] == S.STRIP                    # an empty strip with full ones on both sides
    raw = S.frame("range_ends", rows, cols)
    for label, value in S.range_end_values(conv):
        assert (raw == value).any(), label
    m = v["range_ends"]
    lo, hi = int(round(conv["min_distance"] / S.SCALE)), int(round(conv["max_distance"] / S.SCALE))
    assert not m[raw == 0].any() and not m[raw == 65535].any() and not m[raw == hi + 1].any() and m[raw == lo + 1].all() and m[raw == hi - 1].all()
    nat = v["natural"]
    assert 0.3 < nat.mean() < 1.0 and not nat.all()
    # the tile geometry the shapes are chosen for
    N = rows * cols
    assert cols % S.STRIP == 0 and all(c % S.STRIP for _, c in S.FALLBACK_SHAPES)
    assert (N < 2048) == ((rows, cols) == (16, 64)) and (N % 2048 != 0 or N < 2048)
