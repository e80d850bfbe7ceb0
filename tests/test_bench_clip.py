"""bench.py builds its clip with synth_clip, not frame by frame through tiler_amd.synth.frame: the pixels must be the same, for both
generators (literal and frozen columns), across the channel rotations at frames 100 and 200 and on sizes that are not multiples of 8."""
import numpy as np
import pytest

import bench
from tiler_amd import synth


@pytest.mark.parametrize("freeze", [False, True])
@pytest.mark.parametrize("w,h,nframes", [(64, 40, 3), (21, 13, 205)])
def test_bench_clip_equals_synth_video(w, h, nframes, freeze):
    got = bench.synth_clip(np.empty((nframes, h, w), np.int32), freeze=freeze)
    want = synth.video(nframes, w, h, freeze=freeze)
    assert np.array_equal(got.view(np.uint32), want)
